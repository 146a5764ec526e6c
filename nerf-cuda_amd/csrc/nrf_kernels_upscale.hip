// nrf_kernels_upscale.hip -- the render buffer's spatial upscaler (nrf_rb_upscale): the developed surface at the render resolution ->
// a plane at the output resolution, both stages of nrf_upscale_plan.h (the text host/upscale_plan_check.cpp compiles) in ONE launch.
//   upscale_kernel<PACK8>   PACK8: also the packed 8-bit pixels -- 2 instances
// A workgroup of four waves owns a tile of 62 x 14 output pixels, one workgroup per tile (no loop over tiles: the grid is the tile
// count, at most 265 x 1171).  With the one-pixel apron stage 2 needs, that is 64 x 16 stage-1 values: one wave, one apron row per step.
//   1. the source footprint of the apron -- at most 68 x 20 texels at ratio 1, fewer at higher ratios -- goes into LDS as float4: a
//      source texel is fetched from global memory once per workgroup, and reused by up to 16 x ratio^2 taps from there.
//   2. stage 1: a lane owns one apron column for the four apron rows of its wave.  Its column's tap indices and weights are made once
//      per lane, a row's once per row (it is wave-uniform); the 16 taps are 16-byte LDS reads.  An apron pixel beyond the plane is
//      evaluated at the clamped coordinates, i.e. it is the border pixel's value: what stage 2's clamped neighbour indices ask for.
//      (The tap rows across, h_j, are recomputed per apron pixel.  Keeping them in a third LDS image, once per source row and apron
//      column, takes 40 % of the vector instructions away and was slower on the MI355X at every tile height tried: a third barrier and
//      fewer workgroups per CU cost more than the arithmetic saved.  DESIGN.md, render buffer measurements.)
//   3. after a barrier, stage 2: a lane owns one tile column for the rows of its wave; five 16-byte LDS reads, then the float4 store
//      and the packed dword, consecutive lanes on consecutive pixels.
// LDS reads (MI355X: ds_read_b128 is served in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32,
// 16 slots of 16 bytes per clock): every wave-instruction here reads ONE image row, so the row strides cannot make a conflict; what can
// is two lanes of a group on columns 16 apart.  Stage 2 reads 64 consecutive columns: each group 16 distinct slots.  In stage 1 the
// lanes of a group would span up to 28 r + 1 source columns (r = in / out <= 1): free of conflicts at ratio 1 and from ratio 2 up, 2-way
// in between.  So stage 1 hands a group's 16 lanes 16 CONSECUTIVE apron columns (apron_column): their taps lie on at most 16
// consecutive source columns at every ratio.  The row strides are the images' widths.
// No scratch, no global atomics, one code path for every amount.
#include <hip/hip_runtime.h>

#include "nrf_upscale_plan.h"

namespace nrf {

constexpr int UPS_TILE_W = 62, UPS_TILE_H = 14;                    // output pixels a workgroup writes
constexpr int UPS_APRON_W = UPS_TILE_W + 2, UPS_APRON_H = UPS_TILE_H + 2;  // 64 x 16 stage-1 values
constexpr int UPS_SRC_W = UPS_APRON_W + 4, UPS_SRC_H = UPS_APRON_H + 4;    // the footprint at ratio 1: (n - 1) r + 1 rounded up, + 3 taps
static_assert(UPS_APRON_W == 64 && UPS_APRON_H % 4 == 0, "one apron row per wave and step");

// the apron column of a lane: the 16 lanes of a ds_read_b128 group get 16 consecutive columns.  Of a 32-lane half, the quads
// 0, 3, 5, 6 form one group and 1, 2, 4, 7 the other; quad q's place among the eight quads of its half is nibble q of the constant
__device__ __forceinline__ int apron_column(int lane) {
  const int quad = (lane >> 2) & 7;
  const int place = (int)(0x73261540u >> (4 * quad)) & 7;
  return (lane & 32) | (place << 2) | (lane & 3);
}

template <bool PACK8>
__global__ __launch_bounds__(256) void upscale_kernel(const UpscalePlan P, const float4* __restrict__ src, float4* __restrict__ dst,
                                                      uint32_t* __restrict__ rgba8) {
  __shared__ float4 S[UPS_SRC_H][UPS_SRC_W];      // the source footprint, 21760 bytes
  __shared__ float4 U[UPS_APRON_H][UPS_APRON_W];  // stage 1 on the apron, 16384 bytes
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int x0 = (int)blockIdx.x * UPS_TILE_W, y0 = (int)blockIdx.y * UPS_TILE_H;  // the tile's first pixel: inside the plane

  // the footprint: from the first tap of the apron's first pixel to the last tap of its last one (s is monotonic in X)
  int i_lo, i_hi;
  float f_unused;
  upscale_source(upscale_clamp_index(x0 - 1, P.ow), P.rx, i_lo, f_unused);
  upscale_source(upscale_clamp_index(x0 + UPS_TILE_W, P.ow), P.rx, i_hi, f_unused);
  const int sx0 = upscale_clamp_index(i_lo - 1, P.iw), sw = upscale_clamp_index(i_hi + 2, P.iw) - sx0 + 1;
  upscale_source(upscale_clamp_index(y0 - 1, P.oh), P.ry, i_lo, f_unused);
  upscale_source(upscale_clamp_index(y0 + UPS_TILE_H, P.oh), P.ry, i_hi, f_unused);
  const int sy0 = upscale_clamp_index(i_lo - 1, P.ih), sh = upscale_clamp_index(i_hi + 2, P.ih) - sy0 + 1;
  if (sw > UPS_SRC_W || sh > UPS_SRC_H) return;  // (r <= 1 keeps the footprint inside; uniform, ahead of every barrier)

  // 1. the footprint into LDS: sx0 + x <= the last tap's clamped column < iw, likewise the rows
  for (int k = (int)threadIdx.x; k < sh * UPS_SRC_W; k += 256) {
    const int y = k / UPS_SRC_W, x = k - y * UPS_SRC_W;
    if (x < sw) S[y][x] = src[(size_t)(sy0 + y) * P.iw + (sx0 + x)];
  }

  // 2. stage 1.  The lane's column, once
  const int ax = apron_column(lane);
  int ix, cx[4];
  float fx, wx[4];
  upscale_source(upscale_clamp_index(x0 - 1 + ax, P.ow), P.rx, ix, fx);
  upscale_taps(ix, P.iw, cx);
  upscale_weights(fx, wx);
#pragma unroll
  for (int a = 0; a < 4; ++a) cx[a] -= sx0;  // in [0, sw)
  __syncthreads();
#pragma unroll
  for (int step = 0; step < UPS_APRON_H / 4; ++step) {
    const int ay = wave + 4 * step;
    int iy, cy[4];
    float fy, wy[4];
    upscale_source(upscale_clamp_index(y0 - 1 + ay, P.oh), P.ry, iy, fy);
    upscale_taps(iy, P.ih, cy);
    upscale_weights(fy, wy);
#pragma unroll
    for (int j = 0; j < 4; ++j) cy[j] -= sy0;  // in [0, sh)
    float4 h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = upscale_row(wx, S[cy[j]][cx[0]], S[cy[j]][cx[1]], S[cy[j]][cx[2]], S[cy[j]][cx[3]]);
    U[ay][ax] = upscale_column(wy, h[0], h[1], h[2], h[3], S[cy[1]][cx[1]], S[cy[1]][cx[2]], S[cy[2]][cx[1]], S[cy[2]][cx[2]]);
  }
  __syncthreads();

  // 3. stage 2 and the stores
  const int X = x0 + lane;
  if (lane >= UPS_TILE_W || X >= P.ow) return;  // (no barrier follows)
#pragma unroll
  for (int step = 0; step < (UPS_TILE_H + 3) / 4; ++step) {
    const int ty = wave + 4 * step, Y = y0 + ty;
    if (ty >= UPS_TILE_H || Y >= P.oh) break;
    const float4 out = upscale_sharpen(U[ty + 1][lane + 1], U[ty][lane + 1], U[ty + 2][lane + 1], U[ty + 1][lane], U[ty + 1][lane + 2], P.amount);
    const size_t at = (size_t)Y * P.ow + X;
    dst[at] = out;
    if constexpr (PACK8) rgba8[at] = upscale_rgba8(out);
  }
}

int launch_upscale(const UpscalePlan& P, const void* src, void* dst, void* rgba8, void* stream) {
  if (!src || !dst) return (int)hipErrorInvalidValue;
  // what the kernel's indices rely on: the resolutions in range and the ratios those of the plan
  UpscalePlan want;
  if (!upscale_plan(P.iw, P.ih, P.ow, P.oh, P.amount, want) || want.rx != P.rx || want.ry != P.ry) return (int)hipErrorInvalidValue;
  const dim3 grid((P.ow + UPS_TILE_W - 1) / UPS_TILE_W, (P.oh + UPS_TILE_H - 1) / UPS_TILE_H), block(256);
  if (rgba8) hipLaunchKernelGGL((upscale_kernel<true>), grid, block, 0, (hipStream_t)stream, P, (const float4*)src, (float4*)dst, (uint32_t*)rgba8);
  else hipLaunchKernelGGL((upscale_kernel<false>), grid, block, 0, (hipStream_t)stream, P, (const float4*)src, (float4*)dst, (uint32_t*)nullptr);
  return (int)hipGetLastError();
}

}  // namespace nrf
