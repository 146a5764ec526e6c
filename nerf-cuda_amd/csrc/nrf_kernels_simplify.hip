// nrf_kernels_simplify.hip -- the simplification of the context's mesh by vertex clustering on the extraction's lattice
// (nrf_simplify_mesh).  The definition is nrf_simplify_plan.h's (the functions below are that header's, the text
// host/simplify_plan_check.cpp compiles); this file holds the launches around them.  The two prefix sums are the mesh scan's
// (nrf_kernels_mesh.hip, launch_mesh_scan) over code words that decode to 0 / 1.
//   simplify_key_kernel        one lane per vertex: its cluster and its key, one device-scope 64-bit atomicMin into the dense key table
//                              (8 bytes per cluster, filled with ones by the caller)
//   simplify_triangle_kernel   one lane per triangle: its three representatives from the finished table, its survive flag, and
//                              used[rep] = 1 for a survivor -- a plain store, every writer stores the same value
//   simplify_codes_kernel      used[i] and survive[i] as one scan code word
//   simplify_scatter_kernel    kept vertices, their edge words and sources, vertex_map and the remapped surviving triangles into SECOND
//                              buffers (in place, a lane would overwrite what another lane has yet to read); every write but
//                              vertex_map's own entry is checked against the counted sizes, a dropped write raises *flag
// Nothing here waits for, or needs to see, what another workgroup writes during the same launch: the key table is only lowered in
// the key pass (atomics at the device's scope, performed in L2 / memory, never read back there) and only read in the launches after
// it; used[] is only written in the triangle pass and only read after it.  A minimum and a store of a constant do not depend on order.
#include "nrf_launch.h"
#include "nrf_simplify_plan.h"

namespace nrf {

constexpr uint32_t SIMPLIFY_BLOCK = 256;
// grid-stride launches: at most 2048 workgroups of 256 lanes
constexpr uint32_t SIMPLIFY_MAX_GROUPS = 2048;
static uint32_t simplify_groups(uint32_t n) {
  const uint32_t g = (n + SIMPLIFY_BLOCK - 1) / SIMPLIFY_BLOCK;
  return g < 1 ? 1 : (g > SIMPLIFY_MAX_GROUPS ? SIMPLIFY_MAX_GROUPS : g);
}
#define SIMPLIFY_FOR(i, n) for (uint32_t i = blockIdx.x * SIMPLIFY_BLOCK + threadIdx.x; i < (n); i += gridDim.x * SIMPLIFY_BLOCK)

__global__ __launch_bounds__(256) void simplify_key_kernel(const MeshLattice L, uint32_t factor, uint32_t n_clusters,
                                                           const uint32_t* __restrict__ edges, const float* __restrict__ vertices,
                                                           uint32_t n_vertices, unsigned long long* keys) {
  SIMPLIFY_FOR(v, n_vertices) {
    uint32_t cid;
    uint64_t key;
    if (simplify_vertex_key(L, factor, n_clusters, edges, vertices, v, cid, key)) atomicMin(&keys[cid], (unsigned long long)key);  // (cid < n_clusters)
  }
}

__global__ __launch_bounds__(256) void simplify_triangle_kernel(const MeshLattice L, uint32_t factor, uint32_t n_clusters,
                                                                const uint32_t* __restrict__ edges, const unsigned long long* __restrict__ keys,
                                                                uint32_t n_vertices, const uint32_t* __restrict__ triangles, uint32_t n_triangles,
                                                                uint32_t* __restrict__ survive, uint32_t* used) {
  SIMPLIFY_FOR(t, n_triangles) {
    uint32_t rep[3];
    const bool alive = simplify_triangle(L, factor, n_clusters, edges, keys, n_vertices, triangles, t, rep);
    survive[t] = alive ? 1u : 0u;
    if (alive) {  // (alive: the three are < n_vertices, the elements used[] holds)
      used[rep[0]] = 1u;
      used[rep[1]] = 1u;
      used[rep[2]] = 1u;
    }
  }
}

__global__ __launch_bounds__(256) void simplify_codes_kernel(const uint32_t* __restrict__ used, const uint32_t* __restrict__ survive,
                                                             uint32_t n_vertices, uint32_t n_triangles, uint32_t* __restrict__ codes) {
  const uint32_t n = n_vertices > n_triangles ? n_vertices : n_triangles;
  SIMPLIFY_FOR(i, n) codes[i] = meshcc_scan_code(i < n_vertices && used[i] != 0u, i < n_triangles && survive[i] != 0u);
}

__global__ __launch_bounds__(256) void simplify_scatter_kernel(const MeshLattice L, uint32_t factor, uint32_t n_clusters,
                                                               const uint32_t* __restrict__ edges, const unsigned long long* __restrict__ keys,
                                                               const uint32_t* __restrict__ vertices, uint32_t n_vertices,
                                                               const uint32_t* __restrict__ triangles, uint32_t n_triangles,
                                                               const uint32_t* __restrict__ codes, const uint32_t* __restrict__ vnew,
                                                               const uint32_t* __restrict__ tnew, uint32_t kept_vertices, uint32_t kept_triangles,
                                                               const SimplifyOut O, uint32_t* flag) {
  const uint32_t n = n_vertices > n_triangles ? n_vertices : n_triangles;
  bool ok = true;
  SIMPLIFY_FOR(i, n)
    ok = simplify_move(L, factor, n_clusters, edges, keys, vertices, n_vertices, triangles, n_triangles, codes, vnew, tnew, kept_vertices,
                       kept_triangles, i, O) && ok;
  if (!ok) *flag = 1u;
}

static bool simplify_args_valid(const SimplifyArgs& A) {
  return mesh_lattice_valid(A.L.origin, A.L.cell, A.L.dims) && simplify_factor_valid(A.factor) && A.n_vertices && A.vertices && A.edges && A.keys &&
         (!A.n_triangles || A.triangles) && A.n_clusters == simplify_clusters(A.L, A.factor);
}

hipError_t launch_simplify_mark(const SimplifyArgs& A, uint32_t* used, uint32_t* survive, uint32_t* codes, hipStream_t st) {
  if (!simplify_args_valid(A) || !used || !codes || (A.n_triangles && !survive)) return hipErrorInvalidValue;
  const uint32_t n = A.n_vertices > A.n_triangles ? A.n_vertices : A.n_triangles;
  hipLaunchKernelGGL(simplify_key_kernel, dim3(simplify_groups(A.n_vertices)), dim3(SIMPLIFY_BLOCK), 0, st, A.L, A.factor, A.n_clusters, A.edges,
                     A.vertices, A.n_vertices, A.keys);
  if (A.n_triangles)
    hipLaunchKernelGGL(simplify_triangle_kernel, dim3(simplify_groups(A.n_triangles)), dim3(SIMPLIFY_BLOCK), 0, st, A.L, A.factor, A.n_clusters,
                       A.edges, A.keys, A.n_vertices, A.triangles, A.n_triangles, survive, used);
  hipLaunchKernelGGL(simplify_codes_kernel, dim3(simplify_groups(n)), dim3(SIMPLIFY_BLOCK), 0, st, used, survive, A.n_vertices, A.n_triangles, codes);
  return hipGetLastError();
}

hipError_t launch_simplify_scatter(const SimplifyArgs& A, const uint32_t* codes, const uint32_t* vnew, const uint32_t* tnew, uint32_t kept_vertices,
                                   uint32_t kept_triangles, float* vertices_out, uint32_t* edges_out, uint32_t* sources, uint32_t* vertex_map,
                                   uint32_t* triangles_out, uint32_t* flag, hipStream_t st) {
  if (!simplify_args_valid(A) || !codes || !vnew || !tnew || !vertex_map || !flag) return hipErrorInvalidValue;
  if ((kept_vertices && (!vertices_out || !edges_out || !sources)) || (kept_triangles && !triangles_out)) return hipErrorInvalidValue;
  if (kept_vertices > A.n_vertices || kept_triangles > A.n_triangles) return hipErrorInvalidValue;
  const uint32_t n = A.n_vertices > A.n_triangles ? A.n_vertices : A.n_triangles;
  const SimplifyOut O{reinterpret_cast<uint32_t*>(vertices_out), edges_out, sources, vertex_map, triangles_out};
  hipLaunchKernelGGL(simplify_scatter_kernel, dim3(simplify_groups(n)), dim3(SIMPLIFY_BLOCK), 0, st, A.L, A.factor, A.n_clusters, A.edges, A.keys,
                     reinterpret_cast<const uint32_t*>(A.vertices), A.n_vertices, A.triangles, A.n_triangles, codes, vnew, tnew, kept_vertices,
                     kept_triangles, O, flag);
  return hipGetLastError();
}

}  // namespace nrf
