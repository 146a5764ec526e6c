// nrf_kernels_refine.hip -- the mesh refinement (nrf_refine_mesh): every vertex of the context's mesh is moved along its crossing edge
// of the lattice onto the iso value of the density network, by bisection and one secant step (the definition is nrf_refine_plan.h's,
// the text host/refine_plan_check.cpp compiles).
//   refine_kernel<NET>   NET = the model's stage instance (NET_HOT, NET_WIDE, NET_GENERIC: what launch_points selects) -- 3 instances
// The frame is points_kernel's (nrf_kernels_points.hip): 4 waves per workgroup, lds_map<NET>(.., 4), the weight fragments and the level
// table staged once, a wave owns 64 vertices per chunk.  n_steps + 2 network passes per chunk through network_dispatch<NET, ..,
// DENS = true>: the edge's two lattice points, then one midpoint per step.  A lane keeps its edge word and its bracket (lo, hi, s_lo,
// s_hi, two flags) in registers between the passes and forms every position anew from the word (refine_pass_position); positions exist
// in the wave's LDS slots only.  All lanes run all passes: an unbracketed lane asks for the edge's midpoint and drops the answer.  The
// guard (points_guard, centre only) is the one place where a coordinate could become an address: a refused position's lane queues the
// box's centre instead and its sigma is 0, as nrf_density has it.  A lane reads its own edge word and writes its own vertex and
// bracket record, nothing else; unbracketed vertices are counted with one atomicAdd per wave and chunk.
// (one family of kernel instances per translation unit: nrf_render.h)
#include "nrf_points_plan.h"
#include "nrf_refine_plan.h"
#include "nrf_render.h"

namespace nrf {

template <int NET>
__global__ __launch_bounds__(256, 2) void refine_kernel(const DevModel M, const RefineArgs A) {
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
  const uint32_t n = A.n;
  const uint32_t n_passes = A.n_steps + 2u;
  const uint32_t wave_global = blockIdx.x * 4 + wave;
  const uint32_t n_waves = gridDim.x * 4;
  const uint32_t n_chunks = (n + 63u) >> 6;
  for (uint32_t chunk = wave_global; chunk < n_chunks; chunk += n_waves) {
    const uint32_t i = (chunk << 6) + lane;
    const int S = (int)min(64u, n - (chunk << 6));
    const uint32_t word = i < n ? A.edges[i] : 0u;
    RefineState R = refine_start(0.f, 0.f, A.iso);
    float um = 0.f;
#pragma unroll 1
    for (uint32_t pass = 0; pass < n_passes; ++pass) {
      bool ok = false;
      if (i < n) {
        float x[3];
        um = refine_mid(R);
        refine_pass_position(A.L, word, R, pass, x);
        ok = points_guard(x, 0.f, A.bound, 1);
        W->pos[lane] = ok ? make_float4(x[0], x[1], x[2], __builtin_bit_cast(float, lane)) : make_float4(0.f, 0.f, 0.f, __builtin_bit_cast(float, lane));
      }
      wave_sync();
      network_dispatch<NET, false, GATHER_RUNTIME, 0, true>(M, wl, lvs, W, lm.gen, S, lane, 1.0f);
      wave_sync();
      const float s = ok ? W->out[lane].w : 0.f;
      wave_sync();
      if (pass == 0u) R.slo = s;
      else if (pass == 1u) R = refine_start(R.slo, s, A.iso);
      else refine_step(R, um, s, A.iso);
    }
    if (i < n) {
      reinterpret_cast<float4*>(A.brackets)[i] = make_float4(R.lo, R.hi, R.slo, R.shi);
      if (R.bracketed) {
        float xp[3], xq[3], v[3];
        refine_edge(A.L, word, xp, xq);
        refine_point(xp, xq, refine_finish(R, A.iso), v);
        A.vertices[3 * (size_t)i] = v[0];
        A.vertices[3 * (size_t)i + 1] = v[1];
        A.vertices[3 * (size_t)i + 2] = v[2];
      }
    }
    const unsigned long long open = __ballot(i < n && !R.bracketed);
    if (lane == 0 && open) atomicAdd(A.n_unbracketed, (uint32_t)__popcll(open));
  }
}

// launch_points' sizes (nrf_kernels_points.hip points_grid): 64 vertices per wave and chunk, at most 1024 workgroups
static int refine_grid(uint32_t n) {
  const uint64_t chunks = ((uint64_t)n + 63) / 64;
  const uint64_t g = (chunks + 3) / 4;
  return (int)(g < 1 ? 1 : (g > 256 * 4 ? 256 * 4 : g));
}

#define NRF_LAUNCH_REFINE(NET, LDS)                                                                  \
  do {                                                                                               \
    hipError_t e_ = allow_lds(refine_kernel<NET>, LDS);                                              \
    if (e_ != hipSuccess) return e_;                                                                 \
    hipLaunchKernelGGL((refine_kernel<NET>), dim3(refine_grid(A.n)), dim3(256), LDS, st, M, A);      \
  } while (0)

hipError_t launch_refine(const DevModel& M, const RefineArgs& A, hipStream_t st) {
  if (!A.n) return hipSuccess;
  if (!A.edges || !A.vertices || !A.brackets || !A.n_unbracketed) return hipErrorInvalidValue;
  if (!refine_steps_valid(A.n_steps) || !mesh_lattice_valid(A.L.origin, A.L.cell, A.L.dims)) return hipErrorInvalidValue;
  if (M.stage == NET_GENERIC) {
    const int lds = LDS_LEVEL_BYTES + 4 * ((int)sizeof(WaveLds) + (int)M.gen_wave_bytes);
    NRF_LAUNCH_REFINE(NET_GENERIC, lds);
  } else if (M.stage == NET_WIDE) {
    const int lds = LDS_TOTAL_BYTES + (LDS_WFRAG_WIDE_BYTES - LDS_WFRAG_BYTES) + 4 * LDS_RAYD_BYTES;
    NRF_LAUNCH_REFINE(NET_WIDE, lds);
  } else {
    NRF_LAUNCH_REFINE(NET_HOT, LDS_TOTAL_BYTES);
  }
  return hipGetLastError();
}

}  // namespace nrf
