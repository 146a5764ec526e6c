// nrf_meshcc_plan.h -- the connected components of an indexed triangle mesh and the filter by component size (nrf_mesh_components,
// nrf_filter_mesh) without a device: the root walk, the hook of one triangle, the keep rule, the key of the largest component, the
// remap of vertices and triangles, and a serial host reference of all of it.  The kernels (nrf_kernels_meshcc.hip) and
// host/meshcc_plan_check.cpp compile this text, so the kernels' definition and the tests' replay are one.  Integers only.
//
// Connected  two vertices are connected if a triangle names both; components are the classes of the transitive closure.  A vertex
//            that no triangle names is a component of its own with 0 triangles.
// Label      label[v] = the smallest vertex id of v's component: label[v] <= v, label[label[v]] == label[v].
// Forest     parent[] with the invariant (I): every value ever stored in parent[x] is <= x and is a member of x's component.
//            init      parent[v] = v.
//            root(x)   follow parent[x] while parent[x] != x.  By (I) the walk strictly descends, so it ends -- at a member of x's
//                      component -- whatever mix of older and newer values of parent[] its loads return.
//            hook      of triangle (a, b, c): the three roots, their minimum m, and every root r != m gets parent[r] = min(parent[r], m).
//                      m < r and m is in r's component (the triangle joins them), so (I) holds.
//            compress  parent[v] = root(v): <= v, in v's component, so (I) holds.
//            A round is hook over all triangles, then compress over all vertices; rounds repeat until a hook lowered nothing.  Then
//            every triangle's three roots agree, so a root stands for a whole component, and by (I) it is the component's minimum.
// Table      one row per component in ascending label: (label, n_vertices, n_triangles); a triangle belongs to the component of its
//            vertices.  row(label) = the number of roots below it (an exclusive prefix sum of the root flags).
// Keep       a component is kept iff n_triangles >= min_triangles and, with NRF_MESH_KEEP_LARGEST, it is the component with the most
//            triangles, a tie going to the smaller label: the one whose key (n_triangles << 32 | 0xffffffff - label) is the maximum.
// Remap      a vertex is kept iff its component is, a triangle likewise.  new id of a kept vertex = the number of kept vertices with
//            a smaller old id; kept triangles keep their relative order and the order of their three indices, each index remapped.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define NRF_MESHCC_HD __host__ __device__
#else
#define NRF_MESHCC_HD
#endif

namespace nrf {

constexpr uint32_t MESHCC_KEEP_LARGEST = 1u;  // NRF_MESH_KEEP_LARGEST (nerfhip.h)
constexpr uint32_t MESHCC_FLAGS = MESHCC_KEEP_LARGEST;
inline bool meshcc_flags_valid(uint32_t flags) { return (flags & ~MESHCC_FLAGS) == 0u; }

// root(x): ends by (I) whatever the loads return; a kernel's plain loads may return values older than another lane's store
NRF_MESHCC_HD inline uint32_t meshcc_root(const uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = parent[x];
    if (p >= x) return x;  // (p == x: a root.  p > x never happens under (I); it ends the walk rather than leaving the array's order)
    x = p;
  }
}

// the hook of one triangle: its three roots and their minimum; every root that is not the minimum is to get min(parent[root], low)
struct MeshccHook {
  uint32_t root[3];
  uint32_t low;
};
// (root(x): the walk from x.  host/meshcc_stale_check.cpp hands every walk loads of its own; to everyone else it is meshcc_root)
template <class Root>
NRF_MESHCC_HD inline MeshccHook meshcc_hook_of(Root&& root, uint32_t a, uint32_t b, uint32_t c) {
  MeshccHook h;
  h.root[0] = root(a);
  h.root[1] = root(b);
  h.root[2] = root(c);
  const uint32_t ab = h.root[0] < h.root[1] ? h.root[0] : h.root[1];
  h.low = ab < h.root[2] ? ab : h.root[2];
  return h;
}
NRF_MESHCC_HD inline MeshccHook meshcc_hook(const uint32_t* parent, uint32_t a, uint32_t b, uint32_t c) {
  return meshcc_hook_of([parent](uint32_t x) { return meshcc_root(parent, x); }, a, b, c);
}
// the stores of a hook: every root that is not the minimum gets lower(root, low), which makes parent[root] = min(parent[root], low) and
// returns the value it found there (the kernel's is one device-scope atomicMin); true if any of them was above low.  Three selects,
// not a loop over root[]: nothing private is indexed by a run-time value.  A root named twice is lowered once.
template <class Lower>
NRF_MESHCC_HD inline bool meshcc_hook_lower(const MeshccHook& h, Lower&& lower) {
  bool lowered = false;
  if (h.root[0] != h.low) lowered = (lower(h.root[0], h.low) > h.low) || lowered;
  if (h.root[1] != h.low && h.root[1] != h.root[0]) lowered = (lower(h.root[1], h.low) > h.low) || lowered;
  if (h.root[2] != h.low && h.root[2] != h.root[0] && h.root[2] != h.root[1]) lowered = (lower(h.root[2], h.low) > h.low) || lowered;
  return lowered;
}
// compress of one vertex: store(v, root(v)) unless parent[v] holds it already.  parent is what the lane's loads return, store writes
// the array itself (to the host they are one)
template <class Store>
NRF_MESHCC_HD inline void meshcc_compress(const uint32_t* parent, uint32_t v, Store&& store) {
  const uint32_t r = meshcc_root(parent, v);
  if (r != parent[v]) store(v, r);
}
// a triangle of a mesh of n_vertices vertices that names a vertex beyond them joins nothing (nrf_extract_mesh never makes one)
NRF_MESHCC_HD inline bool meshcc_triangle_valid(uint32_t a, uint32_t b, uint32_t c, uint32_t n_vertices) {
  return a < n_vertices && b < n_vertices && c < n_vertices;
}

// the key whose maximum over the components is the largest one, a tie going to the smaller label
NRF_MESHCC_HD inline uint64_t meshcc_key(uint32_t n_triangles, uint32_t label) {
  return ((uint64_t)n_triangles << 32) | (uint64_t)(0xffffffffu - label);
}
// the keep rule of a component with that row; best = the maximum key over all components
NRF_MESHCC_HD inline bool meshcc_keep(uint32_t label, uint32_t n_triangles, uint64_t min_triangles, uint32_t flags, uint64_t best) {
  if ((uint64_t)n_triangles < min_triangles) return false;
  if ((flags & MESHCC_KEEP_LARGEST) && meshcc_key(n_triangles, label) != best) return false;
  return true;
}
// the code word the mesh scan decodes (nrf_mesh_plan.h: mesh_code_vertices, mesh_code_triangles) for one 0 / 1 flag per channel
NRF_MESHCC_HD inline uint32_t meshcc_scan_code(bool vertex_flag, bool triangle_flag) {
  return (vertex_flag ? 2u : 0u) | (triangle_flag ? 0x100u : 0u);
}

// the scatter of one kept vertex / triangle to its scanned place.  Every write is checked against the counted sizes (kept_vertices,
// kept_triangles); a write that would fall outside, or a kept triangle that names a dropped vertex, is dropped and the function
// returns false: the scan and the scatter disagree.
NRF_MESHCC_HD inline bool meshcc_move_vertex(const uint32_t* vertices, uint32_t v, uint32_t to, uint32_t kept_vertices, uint32_t* out) {
  if (to >= kept_vertices) return false;
  out[3 * (uint64_t)to] = vertices[3 * (uint64_t)v];
  out[3 * (uint64_t)to + 1] = vertices[3 * (uint64_t)v + 1];
  out[3 * (uint64_t)to + 2] = vertices[3 * (uint64_t)v + 2];
  return true;
}
NRF_MESHCC_HD inline bool meshcc_move_triangle(const uint32_t* triangles, uint32_t t, uint32_t to, const uint32_t* codes, const uint32_t* vnew,
                                               uint32_t n_vertices, uint32_t kept_vertices, uint32_t kept_triangles, uint32_t* out) {
  const uint32_t a = triangles[3 * (uint64_t)t], b = triangles[3 * (uint64_t)t + 1], c = triangles[3 * (uint64_t)t + 2];
  if (to >= kept_triangles || !meshcc_triangle_valid(a, b, c, n_vertices)) return false;
  if (!(codes[a] & codes[b] & codes[c] & 2u)) return false;
  const uint32_t na = vnew[a], nb = vnew[b], nc = vnew[c];
  if (na >= kept_vertices || nb >= kept_vertices || nc >= kept_vertices) return false;
  out[3 * (uint64_t)to] = na;
  out[3 * (uint64_t)to + 1] = nb;
  out[3 * (uint64_t)to + 2] = nc;
  return true;
}

// ---- the host's side: a serial reference of the whole thing ----
struct MeshccParts {
  std::vector<uint32_t> labels;      // [n_vertices]
  std::vector<uint32_t> components;  // [n_components][3] = (label, n_vertices, n_triangles), ascending label
  std::vector<uint32_t> rows;        // [n_vertices]: the number of roots below v (row of a label at the label's own place)
  uint64_t best = 0;                 // the maximum key (0 for an empty mesh)
  uint32_t n_rounds = 0;
};
inline MeshccParts meshcc_label_host(uint32_t n_vertices, const uint32_t* triangles, uint64_t n_triangles) {
  MeshccParts P;
  std::vector<uint32_t>& parent = P.labels;
  parent.resize(n_vertices);
  for (uint32_t v = 0; v < n_vertices; ++v) parent[v] = v;
  for (bool changed = n_vertices != 0; changed;) {
    changed = false;
    for (uint64_t t = 0; t < n_triangles; ++t) {
      const uint32_t a = triangles[3 * t], b = triangles[3 * t + 1], c = triangles[3 * t + 2];
      if (!meshcc_triangle_valid(a, b, c, n_vertices)) continue;
      const MeshccHook h = meshcc_hook(parent.data(), a, b, c);
      changed = meshcc_hook_lower(h, [&parent](uint32_t root, uint32_t low) {
                  const uint32_t old = parent[root];
                  if (low < old) parent[root] = low;
                  return old;
                }) || changed;
    }
    for (uint32_t v = 0; v < n_vertices; ++v) meshcc_compress(parent.data(), v, [&parent](uint32_t x, uint32_t r) { parent[x] = r; });
    ++P.n_rounds;
  }
  P.rows.resize(n_vertices);
  uint32_t n_components = 0;
  for (uint32_t v = 0; v < n_vertices; ++v) {
    P.rows[v] = n_components;
    if (parent[v] == v) ++n_components;
  }
  P.components.assign((size_t)n_components * 3, 0u);
  for (uint32_t v = 0; v < n_vertices; ++v) {
    const uint32_t row = P.rows[parent[v]];
    if (parent[v] == v) P.components[3 * (size_t)row] = v;
    ++P.components[3 * (size_t)row + 1];
  }
  for (uint64_t t = 0; t < n_triangles; ++t) {
    const uint32_t a = triangles[3 * t];
    if (!meshcc_triangle_valid(a, triangles[3 * t + 1], triangles[3 * t + 2], n_vertices)) continue;
    ++P.components[3 * (size_t)P.rows[parent[a]] + 2];
  }
  for (uint32_t r = 0; r < n_components; ++r) {
    const uint64_t key = meshcc_key(P.components[3 * (size_t)r + 2], P.components[3 * (size_t)r]);
    if (key > P.best) P.best = key;
  }
  return P;
}

struct MeshccFiltered {
  std::vector<uint32_t> vertices;   // [kept_vertices][3]: the bit patterns of the kept vertices (empty when none were given)
  std::vector<uint32_t> triangles;  // [kept_triangles][3], remapped
  std::vector<uint32_t> old_vertex, old_triangle;  // the old ids of the kept ones, ascending
  bool ok = true;
};
// vertices: [n_vertices][3] bit patterns, or nullptr (indices only)
inline MeshccFiltered meshcc_filter_host(const MeshccParts& P, uint32_t n_vertices, const uint32_t* vertices, const uint32_t* triangles,
                                         uint64_t n_triangles, uint64_t min_triangles, uint32_t flags) {
  MeshccFiltered F;
  const uint64_t n = n_vertices > n_triangles ? n_vertices : n_triangles;
  std::vector<uint32_t> codes(n), vnew(n), tnew(n);
  auto kept = [&](uint32_t v) {
    const size_t row = P.rows[P.labels[v]];
    return meshcc_keep(P.components[3 * row], P.components[3 * row + 2], min_triangles, flags, P.best);
  };
  for (uint64_t i = 0; i < n; ++i) {
    const bool kv = i < n_vertices && kept((uint32_t)i);
    bool kt = false;
    if (i < n_triangles && meshcc_triangle_valid(triangles[3 * i], triangles[3 * i + 1], triangles[3 * i + 2], n_vertices)) kt = kept(triangles[3 * i]);
    codes[i] = meshcc_scan_code(kv, kt);
  }
  uint32_t nv = 0, nt = 0;
  for (uint64_t i = 0; i < n; ++i) {
    vnew[i] = nv;
    tnew[i] = nt;
    nv += (codes[i] >> 1) & 1u;
    nt += (codes[i] >> 8) & 1u;
  }
  // exactly the counted sizes: AddressSanitizer sees any write the bounds checks let through
  if (vertices) F.vertices.resize((size_t)nv * 3);
  F.triangles.resize((size_t)nt * 3);
  for (uint64_t i = 0; i < n; ++i) {
    if (codes[i] & 2u) {
      F.old_vertex.push_back((uint32_t)i);
      if (vertices) F.ok = meshcc_move_vertex(vertices, (uint32_t)i, vnew[i], nv, F.vertices.data()) && F.ok;
    }
    if (codes[i] & 0x100u) {
      F.old_triangle.push_back((uint32_t)i);
      F.ok = meshcc_move_triangle(triangles, (uint32_t)i, tnew[i], codes.data(), vnew.data(), n_vertices, nv, nt, F.triangles.data()) && F.ok;
    }
  }
  return F;
}

}  // namespace nrf
