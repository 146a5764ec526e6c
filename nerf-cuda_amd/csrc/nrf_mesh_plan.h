// nrf_mesh_plan.h -- the arithmetic of the mesh extraction (nrf_density_lattice, nrf_extract_mesh) without a device: the lattice's
// positions, which edges cross the iso value and where, the triangles of a cell by marching tetrahedra on its Kuhn split, and the
// numbering of vertices and triangles.  The kernels (nrf_kernels_points.hip, nrf_kernels_mesh.hip) and host/mesh_plan_check.cpp
// compile this text, so the kernels' definition and the tests' replay are one.  Every floating-point operation is ONE fp32
// rounding: the library is built with -ffp-contract=off -fno-fast-math, and a host build of this header has to be (host/Makefile:
// mesh_asan).
//
// Lattice    dims = (nx, ny, nz), each >= 2.  Point (i, j, k) has the linear index p = (i * ny + j) * nz + k (z innermost) and the
//            position x_c = origin_c + (float)index_c * cell_c (the product is rounded, then the sum).
// Inside     inside(p) = sigma[p] >= iso, an fp32 compare: NaN is outside.
// Edges      point p owns edge m, m = 1 .. 7, which runs to q = (i + (m & 1), j + ((m >> 1) & 1), k + ((m >> 2) & 1)) when q is in
//            the lattice: three axis edges, three face diagonals, the body diagonal -- exactly the edges of the Kuhn tetrahedra.
//            The edge crosses iff inside(p) != inside(q), and a crossing edge carries ONE vertex:
//              d = s_q - s_p;  u = (iso - s_p) / d;  if (!(u >= 0 && u <= 1)) u = 0.5 (infinite sigmas, every NaN);
//              v_c = x_p,c + u * (x_q,c - x_p,c)      (difference, product, sum: one rounding each)
//            Vertex ids: vbase[p] = exclusive prefix sum of the crossing-edge counts in order of p; the vertex of edge m of p is
//            vbase[p] + the number of crossing edges of p with smaller m.
// Tetrahedra the cell with min corner p exists iff i < nx - 1 && j < ny - 1 && k < nz - 1.  Its six tetrahedra follow the
//            permutations (a, b, c) of the axes in the order xyz, xzy, yxz, yzx, zxy, zyx: corners c0 = p, c1 = c0 + e_a,
//            c2 = c1 + e_b, c3 = p + (1, 1, 1).  By the inside mask of the four corners:
//              all equal                          no triangle
//              one corner L differs, the others   one triangle on the vertices of the edges L-r0, L-r1, L-r2
//              r0 < r1 < r2 in corner order
//              two inside A < B, two outside      the quad AC, AD, BD, BC as the triangles (AC, AD, BD) and (AC, BD, BC)
//              C < D
//            and the last two indices of a triangle are swapped where MESH_SWAP says so, so that (b - a) x (c - a) points from
//            the inside corners towards the outside corners.
// Triangles  tbase = exclusive prefix sum of the per-cell triangle counts in order of the min corner's p; within a cell the
//            triangles go in tetrahedron order, then in the order above.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NRF_MESH_HD __host__ __device__
#else
#define NRF_MESH_HD
#endif

namespace nrf {

struct MeshLattice {
  float origin[3];
  float cell[3];
  uint32_t dims[3];
};

NRF_MESH_HD inline uint32_t mesh_points(const MeshLattice& L) { return L.dims[0] * L.dims[1] * L.dims[2]; }  // (<= 2^27: mesh_lattice_valid)
NRF_MESH_HD inline void mesh_ijk(const MeshLattice& L, uint32_t p, uint32_t (&ijk)[3]) {
  const uint32_t ij = p / L.dims[2];
  ijk[2] = p - ij * L.dims[2];
  ijk[0] = ij / L.dims[1];
  ijk[1] = ij - ijk[0] * L.dims[1];
}
NRF_MESH_HD inline float mesh_coord(float origin, float cell, uint32_t index) {
  const float s = (float)index * cell;
  return origin + s;
}
NRF_MESH_HD inline void mesh_position(const MeshLattice& L, uint32_t i, uint32_t j, uint32_t k, float (&x)[3]) {
  x[0] = mesh_coord(L.origin[0], L.cell[0], i);
  x[1] = mesh_coord(L.origin[1], L.cell[1], j);
  x[2] = mesh_coord(L.origin[2], L.cell[2], k);
}
NRF_MESH_HD inline bool mesh_inside(float s, float iso) { return s >= iso; }

// A corner of a cell, and an edge m, is a code of three bits: bit 0 = +x, bit 1 = +y, bit 2 = +z.
NRF_MESH_HD inline uint32_t mesh_offset(const MeshLattice& L, uint32_t code) {
  return ((code & 1u) * L.dims[1] + ((code >> 1) & 1u)) * L.dims[2] + ((code >> 2) & 1u);
}
NRF_MESH_HD inline bool mesh_in_lattice(const MeshLattice& L, const uint32_t (&ijk)[3], uint32_t code) {
  return ijk[0] + (code & 1u) < L.dims[0] && ijk[1] + ((code >> 1) & 1u) < L.dims[1] && ijk[2] + ((code >> 2) & 1u) < L.dims[2];
}

// the vertex of a crossing edge from p (at xp, sigma sp) to q
NRF_MESH_HD inline void mesh_vertex(const float (&xp)[3], const float (&xq)[3], float sp, float sq, float iso, float (&v)[3]) {
  const float d = sq - sp;
  const float num = iso - sp;
  float u = num / d;
  if (!(u >= 0.0f && u <= 1.0f)) u = 0.5f;
  for (int c = 0; c < 3; ++c) {
    const float e = xq[c] - xp[c];
    const float ue = u * e;
    v[c] = xp[c] + ue;
  }
}

// Corner i (0 .. 3) of tetrahedron t (0 .. 5) as a corner code (selects and shifts: nothing is indexed)
NRF_MESH_HD constexpr uint32_t mesh_tet_axis_a(uint32_t t) { return t >> 1; }
NRF_MESH_HD constexpr uint32_t mesh_tet_axis_b(uint32_t t) {
  return (t & 1u) ? (mesh_tet_axis_a(t) == 2u ? 1u : 2u) : (mesh_tet_axis_a(t) == 0u ? 1u : 0u);
}
NRF_MESH_HD constexpr uint32_t mesh_tet_corner(uint32_t t, uint32_t i) {
  return i == 0 ? 0u : (i == 1 ? (1u << mesh_tet_axis_a(t)) : (i == 2 ? ((1u << mesh_tet_axis_a(t)) | (1u << mesh_tet_axis_b(t))) : 7u));
}
// bit `mask` of MESH_SWAP[t]: the triangles of tetrahedron t with inside mask `mask` (bit i = corner i inside) swap their last two indices
constexpr uint16_t MESH_SWAP[6] = {0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da};

// The triangles of every (tetrahedron, mask) as words: bit 31 = the triangle exists; bits 6 n .. 6 n + 5 = its n-th vertex as the
// edge (from, to) of two corner codes of the CELL, from in bits 0 .. 2, to in bits 3 .. 5; `from` is a subset of `to`, so the edge is
// owned by lattice point p + from with m = from ^ to.  The kernels index this table by run-time values: it lives in constant memory there.
struct MeshTable {
  uint32_t tri[6][16][2];
};
constexpr uint32_t mesh_edge_code(uint32_t t, uint32_t x, uint32_t y) {  // corners x, y of tetrahedron t, either order
  const uint32_t lo = x < y ? x : y, hi = x < y ? y : x;
  return mesh_tet_corner(t, lo) | (mesh_tet_corner(t, hi) << 3);
}
constexpr uint32_t mesh_tri_word(uint32_t t, uint32_t mask, uint32_t e0, uint32_t e1, uint32_t e2) {
  const bool swap = (MESH_SWAP[t] >> mask) & 1u;
  return 0x80000000u | e0 | ((swap ? e2 : e1) << 6) | ((swap ? e1 : e2) << 12);
}
constexpr MeshTable mesh_make_table() {
  MeshTable T{};
  for (uint32_t t = 0; t < 6; ++t)
    for (uint32_t mask = 1; mask < 15; ++mask) {
      uint32_t in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, n_in = 0, n_out = 0;
      for (uint32_t i = 0; i < 4; ++i) {
        if ((mask >> i) & 1u) in[n_in++] = i;
        else out[n_out++] = i;
      }
      if (n_in == 2) {
        const uint32_t ac = mesh_edge_code(t, in[0], out[0]), ad = mesh_edge_code(t, in[0], out[1]);
        const uint32_t bd = mesh_edge_code(t, in[1], out[1]), bc = mesh_edge_code(t, in[1], out[0]);
        T.tri[t][mask][0] = mesh_tri_word(t, mask, ac, ad, bd);
        T.tri[t][mask][1] = mesh_tri_word(t, mask, ac, bd, bc);
      } else {
        const uint32_t l = n_in == 1 ? in[0] : out[0];
        const uint32_t* r = n_in == 1 ? out : in;
        T.tri[t][mask][0] = mesh_tri_word(t, mask, mesh_edge_code(t, l, r[0]), mesh_edge_code(t, l, r[1]), mesh_edge_code(t, l, r[2]));
      }
    }
  return T;
}

NRF_MESH_HD inline uint32_t mesh_popcount(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
// triangles of a tetrahedron with that inside mask: 0, 1 or 2
NRF_MESH_HD inline uint32_t mesh_tet_triangles(uint32_t mask) {
  const uint32_t n = mesh_popcount(mask & 15u);
  return n == 0u || n == 4u ? 0u : (n == 2u ? 2u : 1u);
}
// the inside mask of tetrahedron t from the cell's eight inside bits (bit = corner code)
NRF_MESH_HD inline uint32_t mesh_tet_mask(uint32_t in8, uint32_t t) {
  return (in8 & 1u) | (((in8 >> mesh_tet_corner(t, 1)) & 1u) << 1) | (((in8 >> mesh_tet_corner(t, 2)) & 1u) << 2) | (((in8 >> 7) & 1u) << 3);
}

// ---- count: what lattice point p contributes.  Bits 1 .. 7: edge m of p crosses; bits 8 .. 11: the triangles of p's cell (0 .. 12).
NRF_MESH_HD inline uint32_t mesh_code_vertices(uint32_t code) { return mesh_popcount(code & 0xfeu); }
NRF_MESH_HD inline uint32_t mesh_code_triangles(uint32_t code) { return (code >> 8) & 15u; }
// the inside bits of the corners of p's cell that are in the lattice (bit = corner code)
NRF_MESH_HD inline uint32_t mesh_inside_bits(const MeshLattice& L, const float* sigma, float iso, uint32_t p, const uint32_t (&ijk)[3]) {
  uint32_t in8 = 0;
  for (uint32_t c = 0; c < 8; ++c)
    if (mesh_in_lattice(L, ijk, c) && mesh_inside(sigma[p + mesh_offset(L, c)], iso)) in8 |= 1u << c;
  return in8;
}
NRF_MESH_HD inline uint32_t mesh_count_point(const MeshLattice& L, const float* sigma, float iso, uint32_t p) {
  uint32_t ijk[3];
  mesh_ijk(L, p, ijk);
  const uint32_t in8 = mesh_inside_bits(L, sigma, iso, p, ijk);
  uint32_t code = 0;
  for (uint32_t m = 1; m < 8; ++m)
    if (mesh_in_lattice(L, ijk, m) && ((in8 >> m) & 1u) != (in8 & 1u)) code |= 1u << m;
  if (mesh_in_lattice(L, ijk, 7u)) {
    uint32_t n = 0;
    for (uint32_t t = 0; t < 6; ++t) n += mesh_tet_triangles(mesh_tet_mask(in8, t));
    code |= n << 8;
  }
  return code;
}

// ---- emit: the vertices of p's crossing edges and the triangles of p's cell at their scanned offsets.  Every write is checked
// against the element counts the buffers hold (n_vertices, n_triangles); a write that would fall outside, or a triangle that would
// name a vertex beyond n_vertices, is dropped and the function returns false: count and emit disagree (the sigmas changed in between).
NRF_MESH_HD inline bool mesh_emit_point(const MeshLattice& L, const float* sigma, float iso, uint32_t p, const uint32_t* codes,
                                        const uint32_t* vbase, const uint32_t* tbase, const MeshTable& T, uint32_t n_vertices,
                                        uint32_t n_triangles, float* vertices, uint32_t* triangles) {
  uint32_t ijk[3];
  mesh_ijk(L, p, ijk);
  const uint32_t in8 = mesh_inside_bits(L, sigma, iso, p, ijk);
  bool ok = true;
  float xp[3];
  mesh_position(L, ijk[0], ijk[1], ijk[2], xp);
  const float sp = sigma[p];
  uint32_t vid = vbase[p];
  for (uint32_t m = 1; m < 8; ++m) {
    if (!(mesh_in_lattice(L, ijk, m) && ((in8 >> m) & 1u) != (in8 & 1u))) continue;
    float xq[3], v[3];
    mesh_position(L, ijk[0] + (m & 1u), ijk[1] + ((m >> 1) & 1u), ijk[2] + ((m >> 2) & 1u), xq);
    mesh_vertex(xp, xq, sp, sigma[p + mesh_offset(L, m)], iso, v);
    if (vid < n_vertices) {
      vertices[3 * (uint64_t)vid] = v[0];
      vertices[3 * (uint64_t)vid + 1] = v[1];
      vertices[3 * (uint64_t)vid + 2] = v[2];
    } else {
      ok = false;
    }
    ++vid;
  }
  if (!mesh_in_lattice(L, ijk, 7u)) return ok;
  uint32_t tid = tbase[p];
  for (uint32_t t = 0; t < 6; ++t) {
    const uint32_t mask = mesh_tet_mask(in8, t);
    const uint32_t n = mesh_tet_triangles(mask);
    for (uint32_t w = 0; w < n; ++w) {
      const uint32_t word = T.tri[t][mask][w];
      uint32_t id[3];
      bool in_range = tid < n_triangles;
      for (uint32_t c = 0; c < 3; ++c) {
        const uint32_t e = (word >> (6 * c)) & 63u;
        const uint32_t from = e & 7u, m = from ^ (e >> 3);
        const uint32_t q = p + mesh_offset(L, from);
        id[c] = vbase[q] + mesh_popcount(codes[q] & ((1u << m) - 1u) & 0xfeu);
        in_range = in_range && id[c] < n_vertices;
      }
      if (in_range) {
        triangles[3 * (uint64_t)tid] = id[0];
        triangles[3 * (uint64_t)tid + 1] = id[1];
        triangles[3 * (uint64_t)tid + 2] = id[2];
      } else {
        ok = false;
      }
      ++tid;
    }
  }
  return ok;
}

// ---- the host's side ----
constexpr uint64_t MESH_MAX_POINTS = 1ull << 27;
// what the entry points accept: every dimension >= 2, at most 2^27 points, finite cells > 0, a finite origin
inline bool mesh_finite(float v) { return __builtin_fabsf(v) <= 3.4028234663852886e38f; }  // (false for NaN and +-inf)
inline bool mesh_lattice_valid(const float (&origin)[3], const float (&cell)[3], const uint32_t (&dims)[3]) {
  uint64_t n = 1;
  for (int c = 0; c < 3; ++c) {
    if (dims[c] < 2) return false;
    n *= dims[c];  // (a factor is below 2^32 and the running product at most 2^27: no overflow of 64 bits)
    if (n > MESH_MAX_POINTS) return false;
    if (!(cell[c] > 0.0f) || !mesh_finite(cell[c]) || !mesh_finite(origin[c])) return false;
  }
  return true;
}
inline bool mesh_iso_valid(float iso) { return mesh_finite(iso); }
inline uint64_t mesh_sigma_bytes(uint64_t n_points) { return n_points * 4; }
inline uint64_t mesh_vertex_bytes(uint64_t n_vertices) { return n_vertices * 12; }
inline uint64_t mesh_triangle_bytes(uint64_t n_triangles) { return n_triangles * 12; }
// codes -> vbase, tbase (exclusive prefix sums) and the totals: what the device's scan computes, serially
inline void mesh_scan_host(const uint32_t* codes, uint64_t n, uint32_t* vbase, uint32_t* tbase, uint64_t& n_vertices, uint64_t& n_triangles) {
  uint64_t v = 0, t = 0;
  for (uint64_t p = 0; p < n; ++p) {
    vbase[p] = (uint32_t)v;
    tbase[p] = (uint32_t)t;
    v += mesh_code_vertices(codes[p]);
    t += mesh_code_triangles(codes[p]);
  }
  n_vertices = v;
  n_triangles = t;
}

}  // namespace nrf
