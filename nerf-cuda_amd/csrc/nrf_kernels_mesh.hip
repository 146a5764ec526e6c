// nrf_kernels_mesh.hip -- the polygoniser of nrf_extract_mesh: marching tetrahedra on the Kuhn split of a lattice's cells.  The
// arithmetic and the numbering are nrf_mesh_plan.h's (the functions below are that header's, the text host/mesh_plan_check.cpp
// compiles); this file holds the launches around them.
//   mesh_count_kernel          per lattice point: the crossing mask of its seven edges and the triangle count of its cell (one code word)
//   mesh_scan_{reduce,partials,write}_kernel   the two exclusive prefix sums of the codes' counts, three passes over tiles of
//                              MESH_SCAN_TILE points: tile sums, the scan of the tile sums (one workgroup), the scan inside the tiles
//                              (launch_mesh_scan: also the scan of nrf_kernels_meshcc.hip, over code words that decode to 0 / 1)
//   mesh_emit_kernel           the vertices and the triangles at their scanned offsets; every write is checked against the element
//                              counts the buffers hold, a write that would fall outside is dropped and raises *flag
//   mesh_edges_kernel          the edge word (p << 3) | m of every vertex, for nrf_refine_mesh; checked and flagged like emit's writes
// Streaming kernels: a lattice point reads its cell's eight sigmas (count, emit) and, where its cell has triangles, the codes and
// vertex bases of the corners that own its edges -- neighbours in the lattice, served by L2.  The triangle table is indexed by
// run-time values and lives in constant memory; nothing here has a private array that is.
#include "nrf_launch.h"
#include "nrf_refine_plan.h"

namespace nrf {

__constant__ MeshTable d_mesh_table = mesh_make_table();

constexpr uint32_t MESH_BLOCK = 256;
constexpr uint32_t MESH_ITEMS = MESH_SCAN_TILE / MESH_BLOCK;  // consecutive points of a lane in the scan
static_assert(MESH_ITEMS * MESH_BLOCK == MESH_SCAN_TILE && MESH_ITEMS == 8, "a lane of the scan holds 8 points");

__global__ __launch_bounds__(256) void mesh_count_kernel(const MeshLattice L, const float* __restrict__ sigma, float iso, uint32_t n,
                                                         uint32_t* __restrict__ codes) {
  for (uint32_t p = blockIdx.x * MESH_BLOCK + threadIdx.x; p < n; p += gridDim.x * MESH_BLOCK) codes[p] = mesh_count_point(L, sigma, iso, p);
}

// Exclusive prefix sum of one (vertices, triangles) pair per lane over the workgroup's 256 lanes; total = the workgroup's sum.
// (two barriers: the four wave sums travel through LDS, which the next call reuses)
__device__ __forceinline__ uint2 block_exclusive(uint2 mine, uint2& total) {
  __shared__ uint2 wave_sum[MESH_BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint2 inc = mine;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t a = __shfl_up(inc.x, d), b = __shfl_up(inc.y, d);
    if (lane >= d) {
      inc.x += a;
      inc.y += b;
    }
  }
  if (lane == 63u) wave_sum[wave] = inc;
  __syncthreads();
  uint2 before = make_uint2(0u, 0u);
  total = make_uint2(0u, 0u);
#pragma unroll
  for (uint32_t w = 0; w < MESH_BLOCK / 64; ++w) {
    const uint2 s = wave_sum[w];
    if (w < wave) {
      before.x += s.x;
      before.y += s.y;
    }
    total.x += s.x;
    total.y += s.y;
  }
  __syncthreads();
  return make_uint2(before.x + inc.x - mine.x, before.y + inc.y - mine.y);
}

// the counts of a lane's 8 consecutive points of tile blockIdx.x (zeros beyond n) and their sum
__device__ __forceinline__ uint2 lane_counts(const uint32_t* __restrict__ codes, uint32_t n, uint32_t first, uint32_t (&v)[MESH_ITEMS],
                                             uint32_t (&t)[MESH_ITEMS]) {
  uint2 sum = make_uint2(0u, 0u);
#pragma unroll
  for (uint32_t k = 0; k < MESH_ITEMS; ++k) {
    const uint32_t code = first + k < n ? codes[first + k] : 0u;
    v[k] = mesh_code_vertices(code);
    t[k] = mesh_code_triangles(code);
    sum.x += v[k];
    sum.y += t[k];
  }
  return sum;
}

__global__ __launch_bounds__(256) void mesh_scan_reduce_kernel(const uint32_t* __restrict__ codes, uint32_t n, uint2* __restrict__ partials) {
  uint32_t v[MESH_ITEMS], t[MESH_ITEMS];
  const uint2 mine = lane_counts(codes, n, blockIdx.x * MESH_SCAN_TILE + threadIdx.x * MESH_ITEMS, v, t);
  uint2 total;
  (void)block_exclusive(mine, total);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// one workgroup: the tile sums become their exclusive prefix sums, 256 at a time with a carry; totals = the sums over the lattice
__global__ __launch_bounds__(256) void mesh_scan_partials_kernel(uint2* __restrict__ partials, uint32_t n_tiles, uint32_t* __restrict__ totals) {
  uint2 carry = make_uint2(0u, 0u);
  for (uint32_t base = 0; base < n_tiles; base += MESH_BLOCK) {
    const uint32_t i = base + threadIdx.x;
    const uint2 mine = i < n_tiles ? partials[i] : make_uint2(0u, 0u);
    uint2 total;
    const uint2 ex = block_exclusive(mine, total);
    if (i < n_tiles) partials[i] = make_uint2(carry.x + ex.x, carry.y + ex.y);
    carry.x += total.x;
    carry.y += total.y;
  }
  if (threadIdx.x == 0) {
    totals[0] = carry.x;
    totals[1] = carry.y;
  }
}

__global__ __launch_bounds__(256) void mesh_scan_write_kernel(const uint32_t* __restrict__ codes, uint32_t n, const uint2* __restrict__ partials,
                                                              uint32_t* __restrict__ vbase, uint32_t* __restrict__ tbase) {
  uint32_t v[MESH_ITEMS], t[MESH_ITEMS];
  const uint32_t first = blockIdx.x * MESH_SCAN_TILE + threadIdx.x * MESH_ITEMS;
  const uint2 mine = lane_counts(codes, n, first, v, t);
  uint2 total;
  const uint2 ex = block_exclusive(mine, total);
  const uint2 tile = partials[blockIdx.x];
  uint32_t rv = tile.x + ex.x, rt = tile.y + ex.y;
#pragma unroll
  for (uint32_t k = 0; k < MESH_ITEMS; ++k) {
    if (first + k < n) {
      vbase[first + k] = rv;
      tbase[first + k] = rt;
    }
    rv += v[k];
    rt += t[k];
  }
}

__global__ __launch_bounds__(256) void mesh_emit_kernel(const MeshLattice L, const float* __restrict__ sigma, float iso, uint32_t n,
                                                        const uint32_t* __restrict__ codes, const uint32_t* __restrict__ vbase,
                                                        const uint32_t* __restrict__ tbase, uint32_t n_vertices, uint32_t n_triangles,
                                                        float* __restrict__ vertices, uint32_t* __restrict__ triangles, uint32_t* flag) {
  for (uint32_t p = blockIdx.x * MESH_BLOCK + threadIdx.x; p < n; p += gridDim.x * MESH_BLOCK) {
    if (!(codes[p] & 0xffeu)) continue;  // no crossing edge and no triangle: nothing to write
    if (!mesh_emit_point(L, sigma, iso, p, codes, vbase, tbase, d_mesh_table, n_vertices, n_triangles, vertices, triangles)) *flag = 1u;
  }
}

// the edge word of every vertex, in emit's numbering (nrf_refine_plan.h); every write is checked against n_vertices, as emit's are
__global__ __launch_bounds__(256) void mesh_edges_kernel(uint32_t n, const uint32_t* __restrict__ codes, const uint32_t* __restrict__ vbase,
                                                         uint32_t n_vertices, uint32_t* __restrict__ edges, uint32_t* flag) {
  for (uint32_t p = blockIdx.x * MESH_BLOCK + threadIdx.x; p < n; p += gridDim.x * MESH_BLOCK) {
    const uint32_t code = codes[p];
    if (!(code & 0xfeu)) continue;
    if (!refine_emit_edges(p, code, vbase[p], n_vertices, edges)) *flag = 1u;
  }
}

// grid-stride launches: at most 2048 workgroups of 256 lanes
constexpr uint32_t MESH_MAX_GROUPS = 2048;
static uint32_t mesh_groups(uint32_t n) {
  const uint32_t g = (n + MESH_BLOCK - 1) / MESH_BLOCK;
  return g < 1 ? 1 : (g > MESH_MAX_GROUPS ? MESH_MAX_GROUPS : g);
}

hipError_t launch_mesh_count(const MeshLattice& L, const float* sigma, float iso, uint32_t* codes, uint32_t* vbase, uint32_t* tbase,
                             void* partials, uint32_t* totals, hipStream_t st) {
  if (!mesh_lattice_valid(L.origin, L.cell, L.dims) || !sigma || !codes || !vbase || !tbase || !partials || !totals) return hipErrorInvalidValue;
  const uint32_t n = mesh_points(L);
  hipLaunchKernelGGL(mesh_count_kernel, dim3(mesh_groups(n)), dim3(MESH_BLOCK), 0, st, L, sigma, iso, n, codes);
  return launch_mesh_scan(codes, n, vbase, tbase, partials, totals, st);
}

hipError_t launch_mesh_scan(const uint32_t* codes, uint32_t n, uint32_t* vbase, uint32_t* tbase, void* partials, uint32_t* totals,
                            hipStream_t st) {
  if (!n || !codes || !vbase || !tbase || !partials || !totals) return hipErrorInvalidValue;
  const uint32_t tiles = mesh_scan_tiles(n);
  hipLaunchKernelGGL(mesh_scan_reduce_kernel, dim3(tiles), dim3(MESH_BLOCK), 0, st, codes, n, (uint2*)partials);
  hipLaunchKernelGGL(mesh_scan_partials_kernel, dim3(1), dim3(MESH_BLOCK), 0, st, (uint2*)partials, tiles, totals);
  hipLaunchKernelGGL(mesh_scan_write_kernel, dim3(tiles), dim3(MESH_BLOCK), 0, st, codes, n, (const uint2*)partials, vbase, tbase);
  return hipGetLastError();
}

hipError_t launch_mesh_emit(const MeshLattice& L, const float* sigma, float iso, const uint32_t* codes, const uint32_t* vbase,
                            const uint32_t* tbase, uint32_t n_vertices, uint32_t n_triangles, float* vertices, uint32_t* triangles,
                            uint32_t* flag, hipStream_t st) {
  if (!mesh_lattice_valid(L.origin, L.cell, L.dims) || !sigma || !codes || !vbase || !tbase || !flag) return hipErrorInvalidValue;
  if ((n_vertices && !vertices) || (n_triangles && !triangles)) return hipErrorInvalidValue;
  if (!n_vertices && !n_triangles) return hipSuccess;
  const uint32_t n = mesh_points(L);
  hipLaunchKernelGGL(mesh_emit_kernel, dim3(mesh_groups(n)), dim3(MESH_BLOCK), 0, st, L, sigma, iso, n, codes, vbase, tbase, n_vertices,
                     n_triangles, vertices, triangles, flag);
  return hipGetLastError();
}

hipError_t launch_mesh_edges(const MeshLattice& L, const uint32_t* codes, const uint32_t* vbase, uint32_t n_vertices, uint32_t* edges,
                             uint32_t* flag, hipStream_t st) {
  if (!mesh_lattice_valid(L.origin, L.cell, L.dims) || !codes || !vbase || !flag || (n_vertices && !edges)) return hipErrorInvalidValue;
  if (!n_vertices) return hipSuccess;
  const uint32_t n = mesh_points(L);
  hipLaunchKernelGGL(mesh_edges_kernel, dim3(mesh_groups(n)), dim3(MESH_BLOCK), 0, st, n, codes, vbase, n_vertices, edges, flag);
  return hipGetLastError();
}

}  // namespace nrf
