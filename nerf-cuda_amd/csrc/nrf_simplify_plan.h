// nrf_simplify_plan.h -- the simplification of an extracted mesh by vertex clustering on the extraction's own lattice (nrf_simplify_mesh)
// without a device: the cluster of a vertex, its key, the representative of a cluster, which triangles survive, the remap of vertices
// and triangles, and a serial host reference of all of it.  The kernels (nrf_kernels_simplify.hip) and host/simplify_plan_check.cpp
// compile this text, so the kernels' definition and the tests' replay are one.  Integers and copied float bits, but for the key's nine
// fp32 operations, each ONE rounding: the library is built with -ffp-contract=off -fno-fast-math, and a host build of this header has
// to be (host/Makefile: simplify_asan).
//
// Cluster    vertex v has the edge word w = (p << 3) | m (nrf_refine_plan.h); its owner point p = (i * ny + j) * nz + k lies in the block
//            b_c = index_c / factor of nb_c = (dims_c - 1) / factor + 1 blocks per axis; cid = (b_x * nb_y + b_y) * nb_z + b_z.
//            factor = 1 .. 256; factor 1 already merges the up to seven vertices one point owns.
// Key        cc_c = origin_c + (float)((2 * b_c + 1) * factor) * (0.5f * cell_c): the block's centre (conversion, half cell, product, sum:
//            one rounding each).  d_c = v_c - cc_c with v the vertex's CURRENT position; d2 = (d_x * d_x + d_y * d_y) + d_z * d_z.
//            hi = d2 < +inf ? bits(d2) : 0x7f800000 (NaN and inf rank last; d2 >= +0, so the bits order as the values do).
//            key = (uint64)hi << 32 | v.
// Rep        rep(v) = the low word of the minimum key over the vertices of v's cluster: the vertex nearest its block's centre, a tie
//            going to the smaller id.  A minimum does not depend on the order in which anything ran.
// Triangles  (a, b, c) maps to (rep a, rep b, rep c) in that order and survives iff the three are pairwise different; a triangle that
//            names a vertex >= n_vertices is dropped (meshcc_triangle_valid).  Survivors keep their relative order.  Duplicate and
//            mutually opposite triangles are KEPT: the vertex map commutes with the boundary operator, so a closed mesh stays closed
//            as a chain (every directed edge occurs as often as its opposite).
// Vertices   a vertex is kept iff it is a representative and a surviving triangle names it; new id = the number of kept vertices with
//            a smaller old id; float bits and edge word are copied.  No vertex of the result is unreferenced.
// Records    sources[new] = old id, ascending.  vertex_map[old v] = the new id of rep(v), or 0xffffffff where rep(v) was not kept.
// An edge word whose p is not a point of the lattice has no cluster (the entry points never make one): its vertex represents nothing,
// is represented by nothing, and a triangle that names it does not survive.
#pragma once
#include <vector>

#include "nrf_meshcc_plan.h"
#include "nrf_refine_plan.h"

namespace nrf {

constexpr uint32_t SIMPLIFY_MAX_FACTOR = 256;
constexpr uint32_t SIMPLIFY_NONE = 0xffffffffu;  // no cluster, no representative, no new id
constexpr uint64_t SIMPLIFY_KEY_EMPTY = ~0ull;   // the key table's fill: above every key
inline bool simplify_factor_valid(uint32_t factor) { return factor >= 1u && factor <= SIMPLIFY_MAX_FACTOR; }

NRF_MESH_HD inline uint32_t simplify_blocks(uint32_t dim, uint32_t factor) { return (dim - 1u) / factor + 1u; }
// clusters of the lattice: at most its points (factor 1), so at most 2^27
NRF_MESH_HD inline uint32_t simplify_clusters(const MeshLattice& L, uint32_t factor) {
  return simplify_blocks(L.dims[0], factor) * simplify_blocks(L.dims[1], factor) * simplify_blocks(L.dims[2], factor);
}
inline uint64_t simplify_key_bytes(uint64_t n_clusters) { return n_clusters * 8; }

// the block of edge word w's owner point and its cluster id; SIMPLIFY_NONE where p is not a point of the lattice
NRF_MESH_HD inline uint32_t simplify_cluster(const MeshLattice& L, uint32_t factor, uint32_t w, uint32_t (&b)[3]) {
  const uint32_t p = w >> 3;
  b[0] = b[1] = b[2] = 0u;
  if (p >= mesh_points(L)) return SIMPLIFY_NONE;
  uint32_t ijk[3];
  mesh_ijk(L, p, ijk);
  for (int c = 0; c < 3; ++c) b[c] = ijk[c] / factor;
  return (b[0] * simplify_blocks(L.dims[1], factor) + b[1]) * simplify_blocks(L.dims[2], factor) + b[2];
}

NRF_MESH_HD inline float simplify_centre(float origin, float cell, uint32_t b, uint32_t factor) {
  const float n = (float)((2u * b + 1u) * factor);
  const float half = 0.5f * cell;
  const float s = n * half;
  return origin + s;
}

NRF_MESH_HD inline uint32_t simplify_float_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}

// the key of vertex v at position x in block b
NRF_MESH_HD inline uint64_t simplify_key(const MeshLattice& L, uint32_t factor, const uint32_t (&b)[3], const float* x, uint32_t v) {
  const float dx = x[0] - simplify_centre(L.origin[0], L.cell[0], b[0], factor);
  const float dy = x[1] - simplify_centre(L.origin[1], L.cell[1], b[1], factor);
  const float dz = x[2] - simplify_centre(L.origin[2], L.cell[2], b[2], factor);
  const float xx = dx * dx;
  const float yy = dy * dy;
  const float zz = dz * dz;
  const float xy = xx + yy;
  const float d2 = xy + zz;
  const uint32_t hi = d2 < __builtin_huge_valf() ? simplify_float_bits(d2) : 0x7f800000u;
  return ((uint64_t)hi << 32) | (uint64_t)v;
}

// (cluster, key) of vertex v of the mesh: what the key pass lowers keys[cluster] to; false: no cluster
NRF_MESH_HD inline bool simplify_vertex_key(const MeshLattice& L, uint32_t factor, uint32_t n_clusters, const uint32_t* edges,
                                            const float* vertices, uint32_t v, uint32_t& cid, uint64_t& key) {
  uint32_t b[3];
  cid = simplify_cluster(L, factor, edges[v], b);
  if (cid >= n_clusters) return false;
  key = simplify_key(L, factor, b, vertices + 3 * (uint64_t)v, v);
  return true;
}

// rep(v) once the key table holds the minima; SIMPLIFY_NONE where v has no cluster or the table holds no vertex of the mesh for it
NRF_MESH_HD inline uint32_t simplify_rep(const MeshLattice& L, uint32_t factor, uint32_t n_clusters, const uint32_t* edges,
                                         const unsigned long long* keys, uint32_t n_vertices, uint32_t v) {
  uint32_t b[3];
  const uint32_t cid = simplify_cluster(L, factor, edges[v], b);
  if (cid >= n_clusters) return SIMPLIFY_NONE;
  const uint32_t r = (uint32_t)(keys[cid] & 0xffffffffull);
  return r < n_vertices ? r : SIMPLIFY_NONE;
}

// the three representatives of triangle t; true iff it survives
NRF_MESH_HD inline bool simplify_triangle(const MeshLattice& L, uint32_t factor, uint32_t n_clusters, const uint32_t* edges,
                                          const unsigned long long* keys, uint32_t n_vertices, const uint32_t* triangles, uint32_t t,
                                          uint32_t (&rep)[3]) {
  const uint32_t a = triangles[3 * (uint64_t)t], b = triangles[3 * (uint64_t)t + 1], c = triangles[3 * (uint64_t)t + 2];
  rep[0] = rep[1] = rep[2] = SIMPLIFY_NONE;
  if (!meshcc_triangle_valid(a, b, c, n_vertices)) return false;
  rep[0] = simplify_rep(L, factor, n_clusters, edges, keys, n_vertices, a);
  rep[1] = simplify_rep(L, factor, n_clusters, edges, keys, n_vertices, b);
  rep[2] = simplify_rep(L, factor, n_clusters, edges, keys, n_vertices, c);
  if (rep[0] == SIMPLIFY_NONE || rep[1] == SIMPLIFY_NONE || rep[2] == SIMPLIFY_NONE) return false;
  return rep[0] != rep[1] && rep[1] != rep[2] && rep[0] != rep[2];
}

// The scatter of item i (vertex i and triangle i) to the scanned places.  codes / vnew / tnew are the scan's (meshcc_scan_code of the
// used and the survive flags).  vertex_map [n_vertices] takes an entry for every vertex; every other write is checked against the
// counted sizes (kept_vertices, kept_triangles), is dropped where it would fall outside, and the function returns false: the scan
// and the scatter disagree.
struct SimplifyOut {
  uint32_t* vertices;    // [kept_vertices][3] bit patterns
  uint32_t* edges;       // [kept_vertices]
  uint32_t* sources;     // [kept_vertices]
  uint32_t* vertex_map;  // [n_vertices]
  uint32_t* triangles;   // [kept_triangles][3]
};
NRF_MESH_HD inline bool simplify_move(const MeshLattice& L, uint32_t factor, uint32_t n_clusters, const uint32_t* edges,
                                      const unsigned long long* keys, const uint32_t* vertices, uint32_t n_vertices, const uint32_t* triangles,
                                      uint32_t n_triangles, const uint32_t* codes, const uint32_t* vnew, const uint32_t* tnew,
                                      uint32_t kept_vertices, uint32_t kept_triangles, uint32_t i, const SimplifyOut& O) {
  bool ok = true;
  if (i < n_vertices) {
    const uint32_t r = simplify_rep(L, factor, n_clusters, edges, keys, n_vertices, i);
    uint32_t entry = SIMPLIFY_NONE;
    if (r != SIMPLIFY_NONE && (codes[r] & 2u)) {
      if (vnew[r] < kept_vertices) entry = vnew[r];
      else ok = false;
    }
    O.vertex_map[i] = entry;
    if (codes[i] & 2u) {
      const uint32_t to = vnew[i];
      if (meshcc_move_vertex(vertices, i, to, kept_vertices, O.vertices)) {
        O.edges[to] = edges[i];
        O.sources[to] = i;
      } else {
        ok = false;
      }
    }
  }
  if (i < n_triangles && (codes[i] & 0x100u)) {
    const uint32_t to = tnew[i];
    uint32_t rep[3];
    if (to < kept_triangles && simplify_triangle(L, factor, n_clusters, edges, keys, n_vertices, triangles, i, rep) &&
        (codes[rep[0]] & codes[rep[1]] & codes[rep[2]] & 2u) && vnew[rep[0]] < kept_vertices && vnew[rep[1]] < kept_vertices &&
        vnew[rep[2]] < kept_vertices) {
      O.triangles[3 * (uint64_t)to] = vnew[rep[0]];
      O.triangles[3 * (uint64_t)to + 1] = vnew[rep[1]];
      O.triangles[3 * (uint64_t)to + 2] = vnew[rep[2]];
    } else {
      ok = false;
    }
  }
  return ok;
}

// ---- the host's side: a serial reference of the whole thing ----
struct Simplified {
  std::vector<uint32_t> vertices;    // [kept_vertices][3] bit patterns
  std::vector<uint32_t> edges;       // [kept_vertices]
  std::vector<uint32_t> sources;     // [kept_vertices]
  std::vector<uint32_t> vertex_map;  // [n_vertices]
  std::vector<uint32_t> triangles;   // [kept_triangles][3]
  std::vector<unsigned long long> keys;  // [n_clusters]: the minima (SIMPLIFY_KEY_EMPTY: a cluster without a vertex)
  bool ok = true;
};
// vertices: [n_vertices][3] bit patterns; edges: [n_vertices]; factor: simplify_factor_valid
inline Simplified simplify_host(const MeshLattice& L, uint32_t factor, uint32_t n_vertices, const uint32_t* vertices, const uint32_t* edges,
                                const uint32_t* triangles, uint64_t n_triangles) {
  Simplified S;
  const uint32_t n_clusters = simplify_clusters(L, factor);
  S.keys.assign(n_clusters, SIMPLIFY_KEY_EMPTY);
  for (uint32_t v = 0; v < n_vertices; ++v) {
    float x[3];
    __builtin_memcpy(x, vertices + 3 * (size_t)v, 12);
    uint32_t b[3];
    const uint32_t cid = simplify_cluster(L, factor, edges[v], b);
    if (cid >= n_clusters) continue;
    const uint64_t key = simplify_key(L, factor, b, x, v);
    if (key < S.keys[cid]) S.keys[cid] = key;
  }
  const uint64_t n = n_vertices > n_triangles ? n_vertices : n_triangles;
  std::vector<uint32_t> used(n_vertices, 0u), codes(n), vnew(n), tnew(n);
  std::vector<uint8_t> survive(n_triangles, 0);
  for (uint64_t t = 0; t < n_triangles; ++t) {
    uint32_t rep[3];
    if (!simplify_triangle(L, factor, n_clusters, edges, S.keys.data(), n_vertices, triangles, (uint32_t)t, rep)) continue;
    survive[t] = 1;
    used[rep[0]] = used[rep[1]] = used[rep[2]] = 1u;
  }
  for (uint64_t i = 0; i < n; ++i) codes[i] = meshcc_scan_code(i < n_vertices && used[i], i < n_triangles && survive[i]);
  uint32_t nv = 0, nt = 0;
  for (uint64_t i = 0; i < n; ++i) {
    vnew[i] = nv;
    tnew[i] = nt;
    nv += (codes[i] >> 1) & 1u;
    nt += (codes[i] >> 8) & 1u;
  }
  // exactly the counted sizes: AddressSanitizer sees any write the bounds checks let through
  S.vertices.resize((size_t)nv * 3);
  S.edges.resize(nv);
  S.sources.resize(nv);
  S.vertex_map.resize(n_vertices);
  S.triangles.resize((size_t)nt * 3);
  const SimplifyOut O{S.vertices.data(), S.edges.data(), S.sources.data(), S.vertex_map.data(), S.triangles.data()};
  for (uint64_t i = 0; i < n; ++i)
    S.ok = simplify_move(L, factor, n_clusters, edges, S.keys.data(), vertices, n_vertices, triangles, (uint32_t)n_triangles, codes.data(),
                         vnew.data(), tnew.data(), nv, nt, (uint32_t)i, O) && S.ok;
  return S;
}

}  // namespace nrf
