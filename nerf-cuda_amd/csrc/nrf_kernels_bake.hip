// nrf_kernels_bake.hip -- the mesh texture (nrf_bake_mesh_texture): the colours of the full network on a per-triangle texture atlas of
// the context's mesh, without leaving the device (the definition is nrf_bake_plan.h's, the text host/bake_plan_check.cpp compiles).
//   bake_kernel<NET>   NET = the model's stage instance (NET_HOT, NET_WIDE, NET_GENERIC: what launch_network selects) -- 3 instances
//   bake_uv_kernel     the UVs, one thread per triangle
// The frame is attr_kernel's (nrf_kernels_attr.hip): 4 waves per workgroup, lds_map<NET>(.., 4), the weight fragments and the level
// table staged once, a wave owns 64 work items per chunk.  A work item is one texel of one pair's cell; the lane finds its owner
// triangle and its (i, j) there (bake_texel), reads the triangle's three indices and nine floats, forms the position and the head-on
// direction itself, and queues both the way attr_kernel step 3 does.  ONE pass of the full network_dispatch<NET> per chunk.  An index
// is checked before it becomes an address (bake_triangle_ok), a position before it is queued (bake_position_ok): a refused lane queues
// the box's centre, drops the answer and writes nothing -- the caller has cleared both planes.  Refused texels of existing triangles
// are counted with one ballot and one atomicAdd per wave and chunk.  A lane writes its own texel and nothing else.
// (one family of kernel instances per translation unit: nrf_render.h)
#include "nrf_bake_plan.h"
#include "nrf_render.h"

namespace nrf {

template <int NET>
__global__ __launch_bounds__(256, 2) void bake_kernel(const DevModel M, const BakeArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool GEN = NET == NET_GENERIC;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = lane_id();
  const LdsMap lm = lds_map<NET>(smem, M, wave, 4);
  uint4* wl = lm.wl;
  LevelParams* lvs = lm.lvs;
  if constexpr (!GEN) stage_fragments<NET>(M, wl);
  if (threadIdx.x < 16) lvs[threadIdx.x] = M.lv[threadIdx.x];
  __syncthreads();
  WaveLds* W = lm.W;
  const uint32_t n = bake_work_items(A.B);
  const uint32_t wave_global = blockIdx.x * 4 + wave;
  const uint32_t n_waves = gridDim.x * 4;
  const uint32_t n_chunks = (n + 63u) >> 6;
  for (uint32_t chunk = wave_global; chunk < n_chunks; chunk += n_waves) {
    const uint32_t w = (chunk << 6) + lane;
    const int S = (int)min(64u, n - (chunk << 6));
    // 1. + 2. the lane's texel, its triangle, the position, the direction and the guard
    BakeTexel T = bake_texel(A.B, w < n ? w : 0u);
    float x[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    const bool exists = w < n && T.tri < A.B.n_triangles;
    bool ok = false;
    if (w < n && bake_triangle_ok(T.tri, A.B.n_triangles, A.triangles, A.n_vertices)) {
      const uint32_t ia = A.triangles[3 * (size_t)T.tri], ib = A.triangles[3 * (size_t)T.tri + 1], ic = A.triangles[3 * (size_t)T.tri + 2];
      const float va[3] = {A.vertices[3 * (size_t)ia], A.vertices[3 * (size_t)ia + 1], A.vertices[3 * (size_t)ia + 2]};
      const float vb[3] = {A.vertices[3 * (size_t)ib], A.vertices[3 * (size_t)ib + 1], A.vertices[3 * (size_t)ib + 2]};
      const float vc[3] = {A.vertices[3 * (size_t)ic], A.vertices[3 * (size_t)ic + 1], A.vertices[3 * (size_t)ic + 2]};
      bake_position(va, vb, vc, T.i, T.j, A.B.res, x);
      ok = bake_position_ok(x, A.bound);
      if (ok) bake_direction(va, vb, vc, d);
    }
    // 3. the slot and the direction as network_kernel queues them
    if (w < n) {
      W->pos[lane] = ok ? make_float4(x[0], x[1], x[2], __builtin_bit_cast(float, lane))
                        : make_float4(0.f, 0.f, 0.f, __builtin_bit_cast(float, lane));
      const float u0 = attr_dir01(ok ? d[0] : 0.f), u1 = attr_dir01(ok ? d[1] : 0.f), u2 = attr_dir01(ok ? d[2] : 0.f);
      if constexpr (GEN) {
        lm.gen.rayd[3 * lane] = u0;  // encoded per pass, for the pass's samples (gen_network_from_lds)
        lm.gen.rayd[3 * lane + 1] = u1;
        lm.gen.rayd[3 * lane + 2] = u2;
      } else {
        half_t e[16];
        encode_dir16(M, u0, u1, u2, e);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          half2_t h;
          h.x = e[2 * j];
          h.y = e[2 * j + 1];
          W->dirf[lane][j] = h2_bits(h);
        }
        if constexpr (NET == NET_WIDE) {
          lm.gen.rayd[3 * lane] = u0;
          lm.gen.rayd[3 * lane + 1] = u1;
          lm.gen.rayd[3 * lane + 2] = u2;
        }
      }
    }
    wave_sync();
    // 4. one pass of both networks
    network_dispatch<NET>(M, wl, lvs, W, lm.gen, S, lane, 1.0f);
    wave_sync();
    // 5. the float4 texel and the packed dword at (x0 + i', y0 + j'): T.px < cols (r + 2) <= width, T.py < rows (r + 1) = height
    if (ok) {
      const float4 so = W->out[lane];
      const size_t at = (size_t)T.py * A.B.width + T.px;
      reinterpret_cast<float4*>(A.texels)[at] = so;
      A.rgba8[at] = bake_rgba8(so.x, so.y, so.z);
    }
    const unsigned long long refused = __ballot(exists && !ok);
    if (lane == 0 && refused) atomicAdd(A.n_refused, (uint32_t)__popcll(refused));
    wave_sync();
  }
}

__global__ __launch_bounds__(256) void bake_uv_kernel(const BakeLayout B, float* __restrict__ uvs) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= B.n_triangles) return;
  float uv[6];
  bake_uv(B, t, uv);
  float2* out = reinterpret_cast<float2*>(uvs) + 3 * (size_t)t;
  out[0] = make_float2(uv[0], uv[1]);
  out[1] = make_float2(uv[2], uv[3]);
  out[2] = make_float2(uv[4], uv[5]);
}

// launch_network's sizes (nrf_kernels.hip): 64 work items per wave and chunk, at most 1024 workgroups
static int bake_grid(uint32_t n) {
  const uint64_t chunks = ((uint64_t)n + 63) / 64;
  const uint64_t g = (chunks + 3) / 4;
  return (int)(g < 1 ? 1 : (g > 256 * 4 ? 256 * 4 : g));
}

#define NRF_LAUNCH_BAKE(NET, LDS)                                                                            \
  do {                                                                                                       \
    hipError_t e_ = allow_lds(bake_kernel<NET>, LDS);                                                        \
    if (e_ != hipSuccess) return e_;                                                                         \
    hipLaunchKernelGGL((bake_kernel<NET>), dim3(bake_grid(bake_work_items(A.B))), dim3(256), LDS, st, M, A); \
  } while (0)

hipError_t launch_bake(const DevModel& M, const BakeArgs& A, hipStream_t st) {
  if (!A.B.n_triangles) return hipSuccess;
  if (!A.vertices || !A.triangles || !A.texels || !A.rgba8 || !A.n_refused) return hipErrorInvalidValue;
  // the layout the stores rely on: the parameters in range, the cells inside the atlas, the atlas inside the limits
  if (!bake_params_valid(A.B.res, A.B.width) || A.B.cols != bake_cols(A.B.res, A.B.width) || A.B.n_pairs != bake_pairs(A.B.n_triangles) ||
      A.B.height != bake_height64(A.B.n_triangles, A.B.res, A.B.width) || !bake_atlas_fits(A.B.width, A.B.height))
    return hipErrorInvalidValue;
  if (M.stage == NET_GENERIC) {
    const int lds = LDS_LEVEL_BYTES + 4 * ((int)sizeof(WaveLds) + (int)M.gen_wave_bytes);
    NRF_LAUNCH_BAKE(NET_GENERIC, lds);
  } else if (M.stage == NET_WIDE) {
    const int lds = LDS_TOTAL_BYTES + (LDS_WFRAG_WIDE_BYTES - LDS_WFRAG_BYTES) + 4 * LDS_RAYD_BYTES;
    NRF_LAUNCH_BAKE(NET_WIDE, lds);
  } else {
    NRF_LAUNCH_BAKE(NET_HOT, LDS_TOTAL_BYTES);
  }
  return hipGetLastError();
}

hipError_t launch_bake_uvs(const BakeLayout& B, float* uvs, hipStream_t st) {
  if (!B.n_triangles) return hipSuccess;
  if (!uvs || !B.width || !B.height || !B.cols) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bake_uv_kernel, dim3((B.n_triangles + 255u) / 256u), dim3(256), 0, st, B, uvs);
  return hipGetLastError();
}

}  // namespace nrf
