// nrf_kernels_meshcc.hip -- the connected components of the context's mesh and the filter by component size (nrf_mesh_components,
// nrf_filter_mesh).  The definition is nrf_meshcc_plan.h's (the functions below are that header's, the text host/meshcc_plan_check.cpp
// compiles); this file holds the launches around them.  The two prefix sums are the mesh scan's (nrf_kernels_mesh.hip,
// launch_mesh_scan) over code words that decode to 0 / 1.
//   meshcc_init_kernel                     parent[v] = v
//   meshcc_hook_kernel                     one lane per triangle: three root walks, one device-scope atomicMin per root that is not the minimum
//   meshcc_compress_kernel                 one lane per vertex: parent[v] = root(v)
//   meshcc_roots_kernel                    root flags as scan code words
//   meshcc_table_{vertices,triangles}_kernel   the table's labels and counts, integer atomicAdd; meshcc_best_kernel: one 64-bit atomicMax per row
//   meshcc_keep_kernel                     keep flags of vertex i and triangle i as one scan code word
//   meshcc_scatter_kernel                  kept vertices and remapped kept triangles into SECOND buffers (in place, a lane would overwrite
//                                          what another lane has yet to read); every write is checked against the counted sizes; a kept
//                                          vertex's edge word (nrf_refine_plan.h) travels with it into a second buffer of its own
//
// Why no launch here waits for, or needs to see, what another workgroup writes during it.  The labelling is a loop of launches on the
// host (nrf_api.hip), and within a launch only this invariant is relied on:
//   (I)  every value ever stored in parent[x] is <= x and is a member of x's component.
// init stores x.  hook stores m into parent[r] only by atomicMin with m < r, m the minimum of three roots of one triangle and r one of
// them, so m is in r's component.  compress stores root(v), a member of v's component that the walk reached by descending from v.
// Hence a root walk strictly descends and ends after at most x steps WHATEVER value of parent[] each of its plain loads returns -- the
// one from before the launch, or any later one another lane's atomicMin or store has put there: the per-XCD L2s are not coherent and
// a CU's L1 is never refreshed by other CUs' stores, so a load may return either.  A stale value is still a value that was stored, so
// (I) covers it; all it can cost is a root that is no longer one, an atomicMin onto a vertex that already hangs lower, and so one
// more round.  Nothing spins, nothing retries a compare-and-swap.
// The last round proves itself: a launch sees every write of the launches before it, so when a hook lowers nothing, parent[] did not
// change while it ran, every walk was exact, and every triangle's roots agreed.  In compress a vertex that reads parent[x] == x has
// found a true root: roots do not change in compress, and a non-root's parent was below it before the launch and only falls.
// A round that lowers something unhooks at least one vertex that was a root when the round began (a target of an atomicMin was read
// as its own parent, and parents only fall), so the host's loop ends after at most n_vertices + 1 rounds.
#include "nrf_launch.h"
#include "nrf_meshcc_plan.h"

namespace nrf {

constexpr uint32_t MESHCC_BLOCK = 256;
// grid-stride launches: at most 2048 workgroups of 256 lanes
constexpr uint32_t MESHCC_MAX_GROUPS = 2048;
static uint32_t meshcc_groups(uint32_t n) {
  const uint32_t g = (n + MESHCC_BLOCK - 1) / MESHCC_BLOCK;
  return g < 1 ? 1 : (g > MESHCC_MAX_GROUPS ? MESHCC_MAX_GROUPS : g);
}
#define MESHCC_FOR(i, n) for (uint32_t i = blockIdx.x * MESHCC_BLOCK + threadIdx.x; i < (n); i += gridDim.x * MESHCC_BLOCK)

__global__ __launch_bounds__(256) void meshcc_init_kernel(uint32_t* __restrict__ parent, uint32_t n_vertices) {
  MESHCC_FOR(v, n_vertices) parent[v] = v;
}

__global__ __launch_bounds__(256) void meshcc_hook_kernel(const uint32_t* __restrict__ triangles, uint32_t n_triangles, uint32_t n_vertices,
                                                          uint32_t* parent, uint32_t* changed) {
  bool lowered = false;
  MESHCC_FOR(t, n_triangles) {
    const uint32_t a = triangles[3 * (uint64_t)t], b = triangles[3 * (uint64_t)t + 1], c = triangles[3 * (uint64_t)t + 2];
    if (!meshcc_triangle_valid(a, b, c, n_vertices)) continue;
    const MeshccHook h = meshcc_hook(parent, a, b, c);
    lowered = meshcc_hook_lower(h, [parent](uint32_t root, uint32_t low) { return atomicMin(&parent[root], low); }) || lowered;
  }
  if (lowered) *changed = 1u;
}

__global__ __launch_bounds__(256) void meshcc_compress_kernel(uint32_t* parent, uint32_t n_vertices) {
  MESHCC_FOR(v, n_vertices) meshcc_compress(parent, v, [parent](uint32_t x, uint32_t r) { parent[x] = r; });
}

__global__ __launch_bounds__(256) void meshcc_roots_kernel(const uint32_t* __restrict__ labels, uint32_t n_vertices, uint32_t* __restrict__ codes) {
  MESHCC_FOR(v, n_vertices) codes[v] = meshcc_scan_code(labels[v] == v, false);
}

// ++components[row][column], the lanes of a wave that share the first active lane's row as ONE atomicAdd of their number (after
// compress, neighbours in id order mostly share a component)
__device__ __forceinline__ void meshcc_count(uint32_t* __restrict__ components, uint32_t row, uint32_t column) {
  const unsigned long long active = __ballot(1);
  const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)active) - 1u;
  const uint32_t leader_row = (uint32_t)__shfl((int)row, (int)leader);
  const unsigned long long same = __ballot(row == leader_row);
  if (row != leader_row) atomicAdd(&components[3 * (uint64_t)row + column], 1u);
  else if (lane == leader) atomicAdd(&components[3 * (uint64_t)row + column], (uint32_t)__popcll(same));
}

__global__ __launch_bounds__(256) void meshcc_table_vertices_kernel(const uint32_t* __restrict__ labels, const uint32_t* __restrict__ rows,
                                                                    uint32_t n_vertices, uint32_t n_components, uint32_t* __restrict__ components) {
  MESHCC_FOR(v, n_vertices) {
    const uint32_t label = labels[v];
    if (label >= n_vertices) continue;
    const uint32_t row = rows[label];
    if (row >= n_components) continue;
    if (label == v) components[3 * (uint64_t)row] = v;
    meshcc_count(components, row, 1u);
  }
}

__global__ __launch_bounds__(256) void meshcc_table_triangles_kernel(const uint32_t* __restrict__ triangles, uint32_t n_triangles,
                                                                     const uint32_t* __restrict__ labels, const uint32_t* __restrict__ rows,
                                                                     uint32_t n_vertices, uint32_t n_components, uint32_t* __restrict__ components) {
  MESHCC_FOR(t, n_triangles) {
    const uint32_t a = triangles[3 * (uint64_t)t];
    if (!meshcc_triangle_valid(a, triangles[3 * (uint64_t)t + 1], triangles[3 * (uint64_t)t + 2], n_vertices)) continue;
    const uint32_t label = labels[a];
    if (label >= n_vertices) continue;
    const uint32_t row = rows[label];
    if (row >= n_components) continue;
    meshcc_count(components, row, 2u);
  }
}

__global__ __launch_bounds__(256) void meshcc_best_kernel(const uint32_t* __restrict__ components, uint32_t n_components, unsigned long long* best) {
  MESHCC_FOR(r, n_components) atomicMax(best, (unsigned long long)meshcc_key(components[3 * (uint64_t)r + 2], components[3 * (uint64_t)r]));
}

// the keep flag of vertex v's component (false where the labelling's arrays do not hold: never, and no address is formed from it)
__device__ __forceinline__ bool meshcc_vertex_kept(uint32_t v, const uint32_t* __restrict__ labels, const uint32_t* __restrict__ rows,
                                                   const uint32_t* __restrict__ components, uint32_t n_vertices, uint32_t n_components,
                                                   uint64_t min_triangles, uint32_t flags, uint64_t best) {
  const uint32_t label = labels[v];
  if (label >= n_vertices) return false;
  const uint32_t row = rows[label];
  if (row >= n_components) return false;
  return meshcc_keep(components[3 * (uint64_t)row], components[3 * (uint64_t)row + 2], min_triangles, flags, best);
}

__global__ __launch_bounds__(256) void meshcc_keep_kernel(const uint32_t* __restrict__ triangles, uint32_t n_triangles,
                                                          const uint32_t* __restrict__ labels, const uint32_t* __restrict__ rows,
                                                          const uint32_t* __restrict__ components, uint32_t n_vertices, uint32_t n_components,
                                                          uint64_t min_triangles, uint32_t flags, const unsigned long long* __restrict__ best_word,
                                                          uint32_t* __restrict__ codes) {
  const uint64_t best = *best_word;
  const uint32_t n = n_vertices > n_triangles ? n_vertices : n_triangles;
  MESHCC_FOR(i, n) {
    const bool kv = i < n_vertices && meshcc_vertex_kept(i, labels, rows, components, n_vertices, n_components, min_triangles, flags, best);
    bool kt = false;
    if (i < n_triangles) {
      const uint32_t a = triangles[3 * (uint64_t)i];
      if (meshcc_triangle_valid(a, triangles[3 * (uint64_t)i + 1], triangles[3 * (uint64_t)i + 2], n_vertices))
        kt = meshcc_vertex_kept(a, labels, rows, components, n_vertices, n_components, min_triangles, flags, best);
    }
    codes[i] = meshcc_scan_code(kv, kt);
  }
}

__global__ __launch_bounds__(256) void meshcc_scatter_kernel(const uint32_t* __restrict__ vertices, const uint32_t* __restrict__ triangles,
                                                             uint32_t n_vertices, uint32_t n_triangles, const uint32_t* __restrict__ codes,
                                                             const uint32_t* __restrict__ vnew, const uint32_t* __restrict__ tnew,
                                                             uint32_t kept_vertices, uint32_t kept_triangles, uint32_t* __restrict__ vertices_out,
                                                             uint32_t* __restrict__ triangles_out, uint32_t* flag,
                                                             const uint32_t* __restrict__ edges, uint32_t* __restrict__ edges_out) {
  const uint32_t n = n_vertices > n_triangles ? n_vertices : n_triangles;
  bool ok = true;
  MESHCC_FOR(i, n) {
    const uint32_t code = codes[i];
    if (i < n_vertices && (code & 2u)) {
      const uint32_t to = vnew[i];
      const bool moved = meshcc_move_vertex(vertices, i, to, kept_vertices, vertices_out);
      if (moved && edges) edges_out[to] = edges[i];  // (moved: to < kept_vertices, the elements edges_out holds)
      ok = moved && ok;
    }
    if (i < n_triangles && (code & 0x100u))
      ok = meshcc_move_triangle(triangles, i, tnew[i], codes, vnew, n_vertices, kept_vertices, kept_triangles, triangles_out) && ok;
  }
  if (!ok) *flag = 1u;
}

static bool meshcc_args_valid(const MeshccArgs& A) { return A.n_vertices && A.labels && (!A.n_triangles || A.triangles); }

hipError_t launch_meshcc_init(const MeshccArgs& A, hipStream_t st) {
  if (!meshcc_args_valid(A)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(meshcc_init_kernel, dim3(meshcc_groups(A.n_vertices)), dim3(MESHCC_BLOCK), 0, st, A.labels, A.n_vertices);
  return hipGetLastError();
}

hipError_t launch_meshcc_round(const MeshccArgs& A, uint32_t* changed, hipStream_t st) {
  if (!meshcc_args_valid(A) || !changed) return hipErrorInvalidValue;
  if (A.n_triangles)
    hipLaunchKernelGGL(meshcc_hook_kernel, dim3(meshcc_groups(A.n_triangles)), dim3(MESHCC_BLOCK), 0, st, A.triangles, A.n_triangles, A.n_vertices,
                       A.labels, changed);
  hipLaunchKernelGGL(meshcc_compress_kernel, dim3(meshcc_groups(A.n_vertices)), dim3(MESHCC_BLOCK), 0, st, A.labels, A.n_vertices);
  return hipGetLastError();
}

hipError_t launch_meshcc_roots(const MeshccArgs& A, uint32_t* codes, hipStream_t st) {
  if (!meshcc_args_valid(A) || !codes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(meshcc_roots_kernel, dim3(meshcc_groups(A.n_vertices)), dim3(MESHCC_BLOCK), 0, st, A.labels, A.n_vertices, codes);
  return hipGetLastError();
}

hipError_t launch_meshcc_table(const MeshccArgs& A, hipStream_t st) {
  if (!meshcc_args_valid(A) || !A.rows || !A.components || !A.n_components || !A.best) return hipErrorInvalidValue;
  hipLaunchKernelGGL(meshcc_table_vertices_kernel, dim3(meshcc_groups(A.n_vertices)), dim3(MESHCC_BLOCK), 0, st, A.labels, A.rows, A.n_vertices,
                     A.n_components, A.components);
  if (A.n_triangles)
    hipLaunchKernelGGL(meshcc_table_triangles_kernel, dim3(meshcc_groups(A.n_triangles)), dim3(MESHCC_BLOCK), 0, st, A.triangles, A.n_triangles,
                       A.labels, A.rows, A.n_vertices, A.n_components, A.components);
  hipLaunchKernelGGL(meshcc_best_kernel, dim3(meshcc_groups(A.n_components)), dim3(MESHCC_BLOCK), 0, st, A.components, A.n_components, A.best);
  return hipGetLastError();
}

hipError_t launch_meshcc_keep(const MeshccArgs& A, uint64_t min_triangles, uint32_t flags, uint32_t* codes, hipStream_t st) {
  if (!meshcc_args_valid(A) || !A.rows || !A.components || !A.n_components || !A.best || !codes || !meshcc_flags_valid(flags)) return hipErrorInvalidValue;
  const uint32_t n = A.n_vertices > A.n_triangles ? A.n_vertices : A.n_triangles;
  hipLaunchKernelGGL(meshcc_keep_kernel, dim3(meshcc_groups(n)), dim3(MESHCC_BLOCK), 0, st, A.triangles, A.n_triangles, A.labels, A.rows, A.components,
                     A.n_vertices, A.n_components, min_triangles, flags, A.best, codes);
  return hipGetLastError();
}

hipError_t launch_meshcc_scatter(const MeshccArgs& A, const float* vertices, const uint32_t* codes, const uint32_t* vnew, const uint32_t* tnew,
                                 uint32_t kept_vertices, uint32_t kept_triangles, float* vertices_out, uint32_t* triangles_out, uint32_t* flag,
                                 hipStream_t st, const uint32_t* edges, uint32_t* edges_out) {
  if (!meshcc_args_valid(A) || !vertices || !codes || !vnew || !tnew || !flag) return hipErrorInvalidValue;
  if ((edges != nullptr) != (edges_out != nullptr) && kept_vertices) return hipErrorInvalidValue;
  if (!edges_out) edges = nullptr;
  if ((kept_vertices && !vertices_out) || (kept_triangles && !triangles_out)) return hipErrorInvalidValue;
  if (kept_vertices > A.n_vertices || kept_triangles > A.n_triangles) return hipErrorInvalidValue;
  if (!kept_vertices && !kept_triangles) return hipSuccess;
  const uint32_t n = A.n_vertices > A.n_triangles ? A.n_vertices : A.n_triangles;
  hipLaunchKernelGGL(meshcc_scatter_kernel, dim3(meshcc_groups(n)), dim3(MESHCC_BLOCK), 0, st, reinterpret_cast<const uint32_t*>(vertices), A.triangles,
                     A.n_vertices, A.n_triangles, codes, vnew, tnew, kept_vertices, kept_triangles, reinterpret_cast<uint32_t*>(vertices_out),
                     triangles_out, flag, edges, edges_out);
  return hipGetLastError();
}

}  // namespace nrf
