// nrf_kernels_temporal.hip -- the render buffer's temporal upscaler (nrf_rb_upscale_temporal) and the motion vectors of a static scene
// (nrf_motion_vectors): nrf_temporal_plan.h (the text host/temporal_plan_check.cpp compiles) on the device.
//   temporal_kernel<PACK8, MOTION>   PACK8: also the packed 8-bit pixels; MOTION: a motion plane is present -- 4 instances
//   motion_kernel                    a grid-stride pass over the render pixels
// temporal_kernel has upscale_kernel's shape (nrf_kernels_upscale.hip): a workgroup of four waves owns a tile of 62 x 14 output pixels, one
// workgroup per tile; with the one-pixel apron the sharpening needs that is 64 x 16 blended values, one wave and one apron row per step.
//   1. the source footprint of the apron goes into LDS as float4.  The jitter moves it by at most one texel per side, so the image is
//      70 x 22 where the spatial kernel's is 68 x 20; the nearest texel (nx, ny) and its 3 x 3 neighbourhood lie within the taps' range.
//   2. per apron pixel the whole blend: the current estimate C from LDS (16 reads), the sample weight, the motion vector of render pixel
//      (nx, ny) and the history from global memory -- one float4 and one float on the static path, 16 + 1 where a vector is non-zero --,
//      the rectifying clamp from LDS, the blend.  An apron pixel beyond the plane is evaluated at the clamped coordinates, i.e. it is the
//      border pixel's value.  Every apron pixel keeps H' in LDS; only tile pixels inside the plane store H' and Wt'.
//   3. after a barrier, stage 2 on H': five LDS reads, the float4 store and the packed dword.
// Reset, rectify and max_history are run-time values, as the amount is.  No scratch, no global atomics, vector stores only.
#include <hip/hip_runtime.h>

#include "nrf_temporal_plan.h"

namespace nrf {

constexpr int TMP_TILE_W = 62, TMP_TILE_H = 14;                            // output pixels a workgroup writes
constexpr int TMP_APRON_W = TMP_TILE_W + 2, TMP_APRON_H = TMP_TILE_H + 2;  // 64 x 16 blended values
constexpr int TMP_SRC_W = TMP_APRON_W + 6, TMP_SRC_H = TMP_APRON_H + 6;    // the spatial footprint and one texel per side for the jitter
static_assert(TMP_APRON_W == 64 && TMP_APRON_H % 4 == 0, "one apron row per wave and step");

// the apron column of a lane: the 16 lanes of a ds_read_b128 group get 16 consecutive columns (nrf_kernels_upscale.hip, apron_column)
__device__ __forceinline__ int temporal_apron_column(int lane) {
  const int quad = (lane >> 2) & 7;
  const int place = (int)(0x73261540u >> (4 * quad)) & 7;
  return (lane & 32) | (place << 2) | (lane & 3);
}

// the first and last source index an axis of the apron touches: outputs first .. last (clamped to the plane), s monotonic in the index
__device__ __forceinline__ void temporal_footprint(int first, int last, int n_out, float r, float j, float o, int n_in, int& lo, int& count) {
  int i_lo, i_hi, n_unused;
  float f_unused, d_unused;
  temporal_source(upscale_clamp_index(first, n_out), r, j, o, n_in, i_lo, f_unused, n_unused, d_unused);
  temporal_source(upscale_clamp_index(last, n_out), r, j, o, n_in, i_hi, f_unused, n_unused, d_unused);
  lo = upscale_clamp_index(i_lo - 1, n_in);
  count = upscale_clamp_index(i_hi + 2, n_in) - lo + 1;
}

template <bool PACK8, bool MOTION>
__global__ __launch_bounds__(256) void temporal_kernel(const TemporalPlan T, const float4* __restrict__ src, const float2* __restrict__ motion,
                                                       const float4* __restrict__ hist_prev, const float* __restrict__ w_prev,
                                                       float4* __restrict__ hist_next, float* __restrict__ w_next, float4* __restrict__ dst,
                                                       uint32_t* __restrict__ rgba8) {
  __shared__ float4 S[TMP_SRC_H][TMP_SRC_W];      // the source footprint, 24640 bytes
  __shared__ float4 U[TMP_APRON_H][TMP_APRON_W];  // H' on the apron, 16384 bytes
  const UpscalePlan& P = T.U;
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int x0 = (int)blockIdx.x * TMP_TILE_W, y0 = (int)blockIdx.y * TMP_TILE_H;  // the tile's first pixel: inside the plane

  int sx0, sw, sy0, sh;
  temporal_footprint(x0 - 1, x0 + TMP_TILE_W, P.ow, P.rx, T.jx, T.ox, P.iw, sx0, sw);
  temporal_footprint(y0 - 1, y0 + TMP_TILE_H, P.oh, P.ry, T.jy, T.oy, P.ih, sy0, sh);
  if (sw > TMP_SRC_W || sh > TMP_SRC_H) return;  // (r <= 1 keeps the footprint inside; uniform, ahead of every barrier)

  // 1. the footprint into LDS: sx0 + x <= the last tap's clamped column < iw, likewise the rows
  for (int k = (int)threadIdx.x; k < sh * TMP_SRC_W; k += 256) {
    const int y = k / TMP_SRC_W, x = k - y * TMP_SRC_W;
    if (x < sw) S[y][x] = src[(size_t)(sy0 + y) * P.iw + (sx0 + x)];
  }

  // 2. the blend.  The lane's column, once
  const int ax = temporal_apron_column(lane);
  const int Xc = upscale_clamp_index(x0 - 1 + ax, P.ow);
  const bool column_stores = ax >= 1 && ax <= TMP_TILE_W && x0 - 1 + ax < P.ow;
  int ix, nx, cx[4];
  float fx, dx, wx[4];
  temporal_source(Xc, P.rx, T.jx, T.ox, P.iw, ix, fx, nx, dx);
  upscale_taps(ix, P.iw, cx);
  upscale_weights(fx, wx);
#pragma unroll
  for (int a = 0; a < 4; ++a) cx[a] -= sx0;  // in [0, sw)
  // the 3 x 3 neighbourhood's columns: nx - 1 .. nx + 1 clamped lie within the taps' range i - 1 .. i + 2 clamped
  const int rx0 = upscale_clamp_index(nx - 1, P.iw) - sx0, rx1 = nx - sx0, rx2 = upscale_clamp_index(nx + 1, P.iw) - sx0;
  __syncthreads();
#pragma unroll 1
  for (int step = 0; step < TMP_APRON_H / 4; ++step) {
    const int ay = wave + 4 * step;
    const int Yc = upscale_clamp_index(y0 - 1 + ay, P.oh);
    int iy, ny, cy[4];
    float fy, dy, wy[4];
    temporal_source(Yc, P.ry, T.jy, T.oy, P.ih, iy, fy, ny, dy);
    upscale_taps(iy, P.ih, cy);
    upscale_weights(fy, wy);
#pragma unroll
    for (int j = 0; j < 4; ++j) cy[j] -= sy0;  // in [0, sh)
    float4 out, hq;
    {
      float4 h[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = upscale_row(wx, S[cy[j]][cx[0]], S[cy[j]][cx[1]], S[cy[j]][cx[2]], S[cy[j]][cx[3]]);
      out = upscale_column(wy, h[0], h[1], h[2], h[3], S[cy[1]][cx[1]], S[cy[1]][cx[2]], S[cy[2]][cx[1]], S[cy[2]][cx[2]]);
    }
    hq = out;  // (read only where a history branch below has replaced it)
    const float wc = temporal_sample_weight(dx, dy);
    float w_out = wc;

    // the history: (nx, ny) < (iw, ih), (Xc, Yc) < (ow, oh), the resampling's indices clamped to the plane
    float mx = 0.0f, my = 0.0f;
    if constexpr (MOTION) {
      if (!(T.flags & TEMPORAL_RESET)) {
        const float2 m = motion[(size_t)ny * P.iw + nx];
        mx = m.x, my = m.y;
      }
    }
    const HistoryFetch F = temporal_history_fetch(Xc, Yc, MOTION, mx, my, P.ow, P.oh, T.flags);
    float wq = 0.0f;
    if (F.kind == HISTORY_TEXEL) {
      const size_t at = (size_t)Yc * P.ow + Xc;
      hq = hist_prev[at];
      wq = w_prev[at];
    } else if (MOTION && F.kind == HISTORY_RESAMPLE) {
      int qx[4], qy[4];
      float vx[4], vy[4];
      upscale_taps(F.bx, P.ow, qx);
      upscale_taps(F.by, P.oh, qy);
      upscale_weights(F.fx, vx);
      upscale_weights(F.fy, vy);
      float4 h[4], p11, p12, p21, p22;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4* row = hist_prev + (size_t)qy[j] * P.ow;
        const float4 t0 = row[qx[0]], t1 = row[qx[1]], t2 = row[qx[2]], t3 = row[qx[3]];
        h[j] = upscale_row(vx, t0, t1, t2, t3);
        if (j == 1) p11 = t1, p12 = t2;
        if (j == 2) p21 = t1, p22 = t2;
      }
      hq = upscale_column(vy, h[0], h[1], h[2], h[3], p11, p12, p21, p22);
      wq = w_prev[(size_t)F.wy * P.ow + F.wx];
    }
    const float wh = temporal_history_weight(wq, T.max_history);
    if (wh > 0.0f) {
      if (T.flags & TEMPORAL_RECTIFY) {
        const int ry[3] = {upscale_clamp_index(ny - 1, P.ih) - sy0, ny - sy0, upscale_clamp_index(ny + 1, P.ih) - sy0};
        float4 lo = S[ry[0]][rx0], hi = lo;
        temporal_fold_range(S[ry[0]][rx1], lo, hi);
        temporal_fold_range(S[ry[0]][rx2], lo, hi);
#pragma unroll
        for (int j = 1; j < 3; ++j) {
          temporal_fold_range(S[ry[j]][rx0], lo, hi);
          temporal_fold_range(S[ry[j]][rx1], lo, hi);
          temporal_fold_range(S[ry[j]][rx2], lo, hi);
        }
        hq = temporal_rectify(hq, lo, hi);
      }
      out = temporal_blend(hq, out, wh, wc, w_out);
    }
    U[ay][ax] = out;
    if (column_stores && ay >= 1 && ay <= TMP_TILE_H && y0 - 1 + ay < P.oh) {  // a tile pixel inside the plane: (Xc, Yc) is the pixel itself
      const size_t at = (size_t)Yc * P.ow + Xc;
      hist_next[at] = out;
      w_next[at] = w_out;
    }
  }
  __syncthreads();

  // 3. stage 2 and the stores
  const int X = x0 + lane;
  if (lane >= TMP_TILE_W || X >= P.ow) return;  // (no barrier follows)
#pragma unroll
  for (int step = 0; step < (TMP_TILE_H + 3) / 4; ++step) {
    const int ty = wave + 4 * step, Y = y0 + ty;
    if (ty >= TMP_TILE_H || Y >= P.oh) break;
    const float4 out = upscale_sharpen(U[ty + 1][lane + 1], U[ty][lane + 1], U[ty + 2][lane + 1], U[ty + 1][lane], U[ty + 1][lane + 2], P.amount);
    const size_t at = (size_t)Y * P.ow + X;
    dst[at] = out;
    if constexpr (PACK8) rgba8[at] = upscale_rgba8(out);
  }
}

int launch_temporal(const TemporalPlan& T, const void* src, const void* motion, const void* hist_prev, const void* w_prev, void* hist_next,
                    void* w_next, void* dst, void* rgba8, void* stream) {
  if (!src || !dst || !hist_next || !w_next) return (int)hipErrorInvalidValue;
  if (!(T.flags & TEMPORAL_RESET) && (!hist_prev || !w_prev)) return (int)hipErrorInvalidValue;
  if (hist_prev == hist_next || w_prev == w_next) return (int)hipErrorInvalidValue;  // a workgroup reads what its neighbours write
  // what the kernel's indices rely on: the resolutions in range, the ratios those of the plan, the jitter within half a texel
  TemporalPlan want;
  if (!temporal_plan(T.U.iw, T.U.ih, T.U.ow, T.U.oh, T.U.amount, T.jx, T.jy, T.max_history, T.flags, want) || want.U.rx != T.U.rx ||
      want.U.ry != T.U.ry || want.ox != T.ox || want.oy != T.oy)
    return (int)hipErrorInvalidValue;
  const dim3 grid((T.U.ow + TMP_TILE_W - 1) / TMP_TILE_W, (T.U.oh + TMP_TILE_H - 1) / TMP_TILE_H), block(256);
#define NRF_TEMPORAL_LAUNCH(PACK8, MOTION)                                                                                            \
  hipLaunchKernelGGL((temporal_kernel<PACK8, MOTION>), grid, block, 0, (hipStream_t)stream, T, (const float4*)src, (const float2*)motion, \
                     (const float4*)hist_prev, (const float*)w_prev, (float4*)hist_next, (float*)w_next, (float4*)dst, (uint32_t*)rgba8)
  if (rgba8 && motion) NRF_TEMPORAL_LAUNCH(true, true);
  else if (rgba8) NRF_TEMPORAL_LAUNCH(true, false);
  else if (motion) NRF_TEMPORAL_LAUNCH(false, true);
  else NRF_TEMPORAL_LAUNCH(false, false);
#undef NRF_TEMPORAL_LAUNCH
  return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void motion_kernel(const MotionPlan M, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                     const float4* __restrict__ rgba, const float* __restrict__ depth_t, float2* __restrict__ out) {
  const int n = M.iw * M.ih;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float o[3] = {rays_o[3 * (size_t)i], rays_o[3 * (size_t)i + 1], rays_o[3 * (size_t)i + 2]};
    const float d[3] = {rays_d[3 * (size_t)i], rays_d[3 * (size_t)i + 1], rays_d[3 * (size_t)i + 2]};
    float mx, my;
    motion_vector(M, o, d, rgba[i].w, depth_t[i], mx, my);
    out[i] = make_float2(mx, my);
  }
}

int launch_motion(const MotionPlan& M, const void* rays_o, const void* rays_d, const void* rgba, const void* depth_t, void* out, void* stream) {
  if (!rays_o || !rays_d || !rgba || !depth_t || !out) return (int)hipErrorInvalidValue;
  if (M.iw <= 0 || M.ih <= 0 || M.iw > UPSCALE_OUT_MAX || M.ih > UPSCALE_OUT_MAX || !motion_alpha_valid(M.min_alpha)) return (int)hipErrorInvalidValue;
  const int n = M.iw * M.ih;  // <= 2^28
  int grid = (n + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(motion_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, M, (const float*)rays_o, (const float*)rays_d,
                     (const float4*)rgba, (const float*)depth_t, (float2*)out);
  return (int)hipGetLastError();
}

}  // namespace nrf
