// nrf_kernels_attr.hip -- the point-attribute kernels (nrf_point_attributes, nrf_mesh_attributes): the unit normal of the density and
// the colour of the full network at caller-supplied positions, in one launch and without leaving the device.
//   attr_kernel<NET, DIRS>   NET = the model's stage instance (NET_HOT, NET_WIDE, NET_GENERIC: what launch_network selects),
//                            DIRS = ATTR_DIR_NORMAL (a point is looked at along d = -n) | ATTR_DIR_GIVEN (the caller's) -- 6 instances
// The frame is points_kernel's (nrf_kernels_points.hip): 4 waves per workgroup, lds_map<NET>(.., 4), the weight fragments and the level
// table staged once, a wave owns 64 points per chunk.  SEVEN network passes per chunk: the six off-centre taps of points_tap through
// network_dispatch<NET, .., DENS = true>, as points_kernel runs them; then the lanes form g, |g| and d (nrf_attr_plan.h), write the
// direction the way network_kernel does for the stage, and the centre goes through the FULL network_dispatch<NET>: its sigma is the
// point's (nrf_density's sigma is nrf_network's bit for bit), its rgb the colour.  The guard (points_guard, 7 taps) is the one place
// where a caller's coordinate could become an address: a refused point's lane queues the box's centre for every pass and both its
// records are zeros.  A direction never becomes an address.
// (one family of kernel instances per translation unit: nrf_render.h)
#include "nrf_attr_plan.h"
#include "nrf_render.h"

namespace nrf {

enum : int { ATTR_DIR_NORMAL = 0, ATTR_DIR_GIVEN = 1 };

template <int NET, int DIRS>
__global__ __launch_bounds__(256, 2) void attr_kernel(const DevModel M, const AttrArgs A) {
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
  const uint32_t wave_global = blockIdx.x * 4 + wave;
  const uint32_t n_waves = gridDim.x * 4;
  const uint32_t n_chunks = (n + 63u) >> 6;
  for (uint32_t chunk = wave_global; chunk < n_chunks; chunk += n_waves) {
    const uint32_t i = (chunk << 6) + lane;
    const int S = (int)min(64u, n - (chunk << 6));
    // 1. the lane's centre and the guard
    float x[3] = {0.f, 0.f, 0.f};
    if (i < n) {
      x[0] = A.xyz[3 * (size_t)i];
      x[1] = A.xyz[3 * (size_t)i + 1];
      x[2] = A.xyz[3 * (size_t)i + 2];
    }
    const bool ok = i < n && points_guard(x, A.h, A.bound, POINTS_GRADIENT_TAPS);
    // 2. the six off-centre taps, one density pass each; a refused lane evaluates the box's centre and drops the result
    float sp = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll 1
    for (int tap = 1; tap < POINTS_GRADIENT_TAPS; ++tap) {
      if (i < n) {
        float tp[3] = {0.f, 0.f, 0.f};
        if (ok) points_tap(x, A.h, tap, tp);
        W->pos[lane] = make_float4(tp[0], tp[1], tp[2], __builtin_bit_cast(float, lane));
      }
      wave_sync();
      network_dispatch<NET, false, GATHER_RUNTIME, 0, true>(M, wl, lvs, W, lm.gen, S, lane, 1.0f);
      wave_sync();
      const float s = i < n ? W->out[lane].w : 0.f;
      wave_sync();
      if (tap & 1) {
        sp = s;
      } else {
        const float g = points_difference(sp, s, A.inv2h);
        gx = tap == 2 ? g : gx;
        gy = tap == 4 ? g : gy;
        gz = tap == 6 ? g : gz;
      }
    }
    // 3. the direction and the normal; the centre's slot and the direction as network_kernel queues them
    float d[3], nm[3], len;
    attr_direction(gx, gy, gz, d, nm, len);
    if (i < n) {
      W->pos[lane] = ok ? make_float4(x[0], x[1], x[2], __builtin_bit_cast(float, lane))
                        : make_float4(0.f, 0.f, 0.f, __builtin_bit_cast(float, lane));
      float v[3] = {d[0], d[1], d[2]};
      if constexpr (DIRS == ATTR_DIR_GIVEN) {
        v[0] = A.dir[3 * (size_t)i];
        v[1] = A.dir[3 * (size_t)i + 1];
        v[2] = A.dir[3 * (size_t)i + 2];
      }
      const float u0 = attr_dir01(v[0]), u1 = attr_dir01(v[1]), u2 = attr_dir01(v[2]);
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
    // 4. the centre through both networks
    network_dispatch<NET>(M, wl, lvs, W, lm.gen, S, lane, 1.0f);
    wave_sync();
    // 5. two float4 per point
    if (i < n) {
      const float4 so = W->out[lane];
      reinterpret_cast<float4*>(A.normal)[i] = ok ? make_float4(nm[0], nm[1], nm[2], so.w) : make_float4(0.f, 0.f, 0.f, 0.f);
      reinterpret_cast<float4*>(A.color)[i] = ok ? make_float4(so.x, so.y, so.z, len) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    wave_sync();
  }
}

// launch_network's sizes (nrf_kernels.hip): 64 points per wave and chunk, at most 1024 workgroups
static int attr_grid(uint32_t n) {
  const uint64_t chunks = ((uint64_t)n + 63) / 64;
  const uint64_t g = (chunks + 3) / 4;
  return (int)(g < 1 ? 1 : (g > 256 * 4 ? 256 * 4 : g));
}

#define NRF_LAUNCH_ATTR(NET, DIRS, LDS)                                                                    \
  do {                                                                                                     \
    hipError_t e_ = allow_lds(attr_kernel<NET, DIRS>, LDS);                                                \
    if (e_ != hipSuccess) return e_;                                                                       \
    hipLaunchKernelGGL((attr_kernel<NET, DIRS>), dim3(attr_grid(A.n)), dim3(256), LDS, st, M, A);          \
  } while (0)
#define NRF_LAUNCH_ATTR_DIRS(NET, LDS)                                                                     \
  do {                                                                                                     \
    if (A.dir) NRF_LAUNCH_ATTR(NET, ATTR_DIR_GIVEN, LDS);                                                  \
    else NRF_LAUNCH_ATTR(NET, ATTR_DIR_NORMAL, LDS);                                                       \
  } while (0)

hipError_t launch_attr(const DevModel& M, const AttrArgs& A, hipStream_t st) {
  if (!A.n) return hipSuccess;
  if (!A.xyz || !A.normal || !A.color) return hipErrorInvalidValue;
  if (M.stage == NET_GENERIC) {
    const int lds = LDS_LEVEL_BYTES + 4 * ((int)sizeof(WaveLds) + (int)M.gen_wave_bytes);
    NRF_LAUNCH_ATTR_DIRS(NET_GENERIC, lds);
  } else if (M.stage == NET_WIDE) {
    const int lds = LDS_TOTAL_BYTES + (LDS_WFRAG_WIDE_BYTES - LDS_WFRAG_BYTES) + 4 * LDS_RAYD_BYTES;
    NRF_LAUNCH_ATTR_DIRS(NET_WIDE, lds);
  } else {
    NRF_LAUNCH_ATTR_DIRS(NET_HOT, LDS_TOTAL_BYTES);
  }
  return hipGetLastError();
}

}  // namespace nrf
