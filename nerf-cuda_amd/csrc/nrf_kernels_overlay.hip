// nrf_kernels_overlay.hip -- the render buffer's image and false-colour overlays and its error map (nrf_rb_overlay_image,
// nrf_rb_overlay_false_color, nrf_rb_error_map): the kernels of nrf_overlay_plan.h, the text host/overlay_plan_check.cpp compiles.
//   overlay_image_kernel<TYPE>    TYPE = IMG_BYTE, IMG_HALF, IMG_FLOAT -- 3 instances
//   overlay_false_color_kernel
//   error_map_kernel, error_average_kernel
// The two overlays are streams over the surface like overlay_depth_kernel: one lane per pixel, grid-stride, a 16-byte read and a
// 16-byte write of the surface per pixel and one gathered texel (4, 8 or 16 bytes) resp. one map value.  A lane's (x, y) is divided
// out once and then advanced by the stride.  The Byte instance keeps the 256-entry sRGB table (made on the host with libm) in LDS:
// three reads of a random 4-byte slot per pixel in place of three log / exp pairs.
// The error map is one wave per cell, four cells per workgroup: a lane walks the cell's pixels k = lane, lane + 64, ... row-major --
// its (row, column) inside the cell advanced by 64 without a division per pixel --, adds in that order, and the 64 partial sums fold
// through __shfl_down at widths 32 .. 1 (lane 0's chain reads only lanes that the step before completed).  The average is the same
// fold by a single wave over the map.  A fixed order, so a host replays both bit for bit; no atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "nrf_overlay_plan.h"

namespace nrf {

namespace {

constexpr int OVERLAY_BLOCK = 256, OVERLAY_GRID_MAX = 2048;
int overlay_grid(int n) { const int g = (n + OVERLAY_BLOCK - 1) / OVERLAY_BLOCK; return g < 1 ? 1 : (g > OVERLAY_GRID_MAX ? OVERLAY_GRID_MAX : g); }

// a lane's walk over the surface: pixel i = first, first + stride, ... as (x, y) without a division per pixel
struct PixelWalk {
  int i, x, y, step_x, step_y;
  __device__ __forceinline__ PixelWalk(int W) {
    const int stride = (int)(gridDim.x * blockDim.x);
    i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    x = i % W, y = i / W;
    step_x = stride % W, step_y = stride / W;
  }
  __device__ __forceinline__ void next(int W) {
    i += (int)(gridDim.x * blockDim.x);
    x += step_x, y += step_y;
    if (x >= W) x -= W, ++y;
  }
};

}  // namespace

template <int TYPE>
__global__ __launch_bounds__(OVERLAY_BLOCK) void overlay_image_kernel(const OverlayImage A, const void* __restrict__ image,
                                                                      const float* __restrict__ table, float4* __restrict__ surface) {
  __shared__ float T[TYPE == IMG_BYTE ? 256 : 1];
  if constexpr (TYPE == IMG_BYTE) {
    static_assert(OVERLAY_BLOCK == 256, "one table entry per lane");
    T[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
  }
  const int W = A.map.W, n = A.map.W * A.map.H;
  for (PixelWalk p(W); p.i < n; p.next(W)) {
    int srcx, srcy;
    overlay_source(A.map, p.x, p.y, srcx, srcy);
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (overlay_inside(srcx, srcy, A.map.iw, A.map.ih)) {
      const size_t at = (size_t)srcx + (size_t)A.map.iw * (size_t)srcy;
      if constexpr (TYPE == IMG_BYTE) val = overlay_read_byte<float4>(((const uint32_t*)image)[at], T);
      else if constexpr (TYPE == IMG_HALF) val = overlay_read_half<float4>(((const uint64_t*)image)[at]);
      else val = ((const float4*)image)[at];
    }
    surface[p.i] = overlay_image_pixel(A, val, surface[p.i]);
  }
}

__global__ __launch_bounds__(OVERLAY_BLOCK) void overlay_false_color_kernel(const OverlayFalseColor A, const float* __restrict__ map,
                                                                            const float* __restrict__ average, float4* __restrict__ surface) {
  const float error_map_scale = overlay_error_scale(A.brightness, average[0]);
  const int n = A.W * A.H;
  for (PixelWalk p(A.W); p.i < n; p.next(A.W)) {
    int srcx, srcy;
    overlay_false_color_source(A, p.x, p.y, srcx, srcy);
    if (!overlay_inside(srcx, srcy, A.mw, A.mh)) continue;
    surface[p.i] = overlay_false_color_pixel(A, map[(size_t)srcx + (size_t)A.mw * (size_t)srcy], error_map_scale, surface[p.i]);
  }
}

// the 64 partial sums of a wave into lane 0: v[l] = v[l] + v[l + s] for s = 32 .. 1
__device__ __forceinline__ float wave_fold(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);
  return v;
}

__global__ __launch_bounds__(256) void error_map_kernel(int W, int H, int mw, int mh, const float4* __restrict__ surface,
                                                        const float4* __restrict__ truth, float* __restrict__ map) {
  const int lane = (int)(threadIdx.x & 63u);
  const int cell = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (cell >= mw * mh) return;  // (wave-uniform; no barrier in this kernel)
  const int cy = cell / mw, cx = cell - cy * mw;
  const int x0 = error_cell_begin(cx, W, mw), y0 = error_cell_begin(cy, H, mh);
  const int cw = error_cell_begin(cx + 1, W, mw) - x0, ch = error_cell_begin(cy + 1, H, mh) - y0;  // >= 1 each; x0 + cw <= W, y0 + ch <= H
  const int count = cw * ch;
  const int step_row = 64 / cw, step_col = 64 - step_row * cw;
  int row = lane / cw, col = lane - row * cw;
  float v = 0.0f;
  for (int k = lane; k < count; k += 64) {
    const size_t at = (size_t)(y0 + row) * (size_t)W + (size_t)(x0 + col);
    v = v + error_pixel(surface[at], truth[at]);
    row += step_row, col += step_col;
    if (col >= cw) col -= cw, ++row;
  }
  v = wave_fold(v);
  if (lane == 0) map[cell] = v / (float)count;
}

__global__ __launch_bounds__(64) void error_average_kernel(int cells, const float* __restrict__ map, float* __restrict__ average) {
  const int lane = (int)threadIdx.x;
  float v = 0.0f;
  for (int k = lane; k < cells; k += 64) v = v + map[k];
  v = wave_fold(v);
  if (lane == 0) average[0] = v / (float)cells;
}

int launch_overlay_image(const OverlayImage& A, const void* image, int type, const float* table, void* surface, void* stream) {
  const OverlayMap& M = A.map;
  // what the kernel's indices rely on
  if (!image || !surface || M.W <= 0 || M.H <= 0 || M.W > OVERLAY_SIZE_MAX || M.H > OVERLAY_SIZE_MAX || M.iw <= 0 || M.ih <= 0 ||
      M.iw > OVERLAY_SIZE_MAX || M.ih > OVERLAY_SIZE_MAX || (M.fov_axis != 0 && M.fov_axis != 1) || (type == IMG_BYTE && !table))
    return (int)hipErrorInvalidValue;
  const dim3 grid(overlay_grid(M.W * M.H)), block(OVERLAY_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  if (type == IMG_BYTE) hipLaunchKernelGGL((overlay_image_kernel<IMG_BYTE>), grid, block, 0, st, A, image, table, (float4*)surface);
  else if (type == IMG_HALF) hipLaunchKernelGGL((overlay_image_kernel<IMG_HALF>), grid, block, 0, st, A, image, table, (float4*)surface);
  else if (type == IMG_FLOAT) hipLaunchKernelGGL((overlay_image_kernel<IMG_FLOAT>), grid, block, 0, st, A, image, table, (float4*)surface);
  else return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

int launch_overlay_false_color(const OverlayFalseColor& A, const float* map, const float* average, void* surface, void* stream) {
  if (!map || !average || !surface || A.W <= 0 || A.H <= 0 || A.W > OVERLAY_SIZE_MAX || A.H > OVERLAY_SIZE_MAX || A.mw <= 0 || A.mh <= 0 ||
      A.mw > ERROR_MAP_MAX || A.mh > ERROR_MAP_MAX || (A.fov_axis != 0 && A.fov_axis != 1))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(overlay_false_color_kernel, dim3(overlay_grid(A.W * A.H)), dim3(OVERLAY_BLOCK), 0, (hipStream_t)stream, A, map, average,
                     (float4*)surface);
  return (int)hipGetLastError();
}

int launch_error_map(int W, int H, int mw, int mh, const void* surface, const void* truth, float* map, float* average, void* stream) {
  if (!surface || !truth || !map || !average || W <= 0 || H <= 0 || W > OVERLAY_SIZE_MAX || H > OVERLAY_SIZE_MAX ||
      !error_map_axis_valid(W, mw) || !error_map_axis_valid(H, mh))
    return (int)hipErrorInvalidValue;
  const int cells = mw * mh;
  hipLaunchKernelGGL(error_map_kernel, dim3((cells + 3) / 4), dim3(256), 0, (hipStream_t)stream, W, H, mw, mh, (const float4*)surface,
                     (const float4*)truth, map);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(error_average_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, cells, (const float*)map, average);
  return (int)hipGetLastError();
}

}  // namespace nrf
