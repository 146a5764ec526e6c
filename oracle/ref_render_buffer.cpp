/*
 * ref_render_buffer.cpp -- the reference's own render-buffer kernels (accumulate, the film curves, tonemap, the turbo colour map,
 * the depth overlay), run on the CPU.
 *
 * TEST INFRASTRUCTURE ONLY.  This file holds no reference text: it includes src/render_buffer.cu from a reference tree named at
 * build time (oracle/Makefile, target `ref`), behind the stand-in headers of oracle/ref_shim/, and exports an extern "C" ABI
 * (refrb_*) that tests/ref_render_buffer_py.py binds.  The library it builds (oracle/_ref/libref_render_buffer.so) is never
 * committed.
 *
 * That file's host methods launch with `<<< >>>`: as ref_encodings.cpp, this unit is built by the ROCm clang as host-only HIP
 * without the HIP headers, `__global__` and `__device__` defined away, so every kernel is a plain host function -- and Eigen
 * is told to stay off its GPU path (-DEIGEN_NO_HIP) and off packets (-DEIGEN_DONT_VECTORIZE): its device path is its scalar path.
 * A launch of a plain function does not compile, so each kernel's DEFINITION is renamed `<kernel>_on_host` by a function-like
 * macro (it expands only where `(` follows the name, which at a launch it does not) and the launch sites see an object that is
 * never called (cuda_surface_on_cpu.h).  The kernels are launched here as CudaRenderBuffer's methods launch them (R = the
 * reference tree): threads {16, 8, 1}, blocks div_round_up per axis (R/src/render_buffer.cu:604-605, :621-622, :701-702).
 *
 * What a CPU compile cannot show, stated where tests use it: Eigen's cwiseMax / cwiseMin are std::max / std::min on the host
 * and keep a NaN that the device's fmaxf / fminf specialisation replaces (deviation D-11); `std::pow` is libm's.
 */
#include <cuda_surface_on_cpu.h>

#include <cstdint>
#include <string>
#include <vector>

namespace ngp {
static const refshim_never_launched accumulate_kernel, overlay_image_kernel, overlay_depth_kernel, overlay_false_color_kernel,
    tonemap_kernel, dlss_splat_kernel;
}
#define accumulate_kernel(...) accumulate_kernel_on_host(__VA_ARGS__)
#define overlay_image_kernel(...) overlay_image_kernel_on_host(__VA_ARGS__)
#define overlay_depth_kernel(...) overlay_depth_kernel_on_host(__VA_ARGS__)
#define overlay_false_color_kernel(...) overlay_false_color_kernel_on_host(__VA_ARGS__)
#define tonemap_kernel(...) tonemap_kernel_on_host(__VA_ARGS__)
#define dlss_splat_kernel(...) dlss_splat_kernel_on_host(__VA_ARGS__)

#include <src/render_buffer.cu>

#undef accumulate_kernel
#undef overlay_image_kernel
#undef overlay_depth_kernel
#undef overlay_false_color_kernel
#undef tonemap_kernel
#undef dlss_splat_kernel

thread_local refshim_dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace {

/* kernel<<<grid, block>>>: serial loops that set blockIdx / threadIdx, x innermost (ref_encodings.cpp's, two axes) */
template <typename Fn>
void launch(const dim3& grid, const dim3& block, Fn&& body) {
  gridDim = grid, blockDim = block;
  for (uint32_t by = 0; by < grid.y; ++by)
    for (uint32_t bx = 0; bx < grid.x; ++bx)
      for (uint32_t ty = 0; ty < block.y; ++ty)
        for (uint32_t tx = 0; tx < block.x; ++tx) {
          blockIdx.x = bx, blockIdx.y = by, blockIdx.z = 0;
          threadIdx.x = tx, threadIdx.y = ty, threadIdx.z = 0;
          body();
        }
}

/* the geometry of every launch in CudaRenderBuffer */
const dim3 kThreads = {16, 8, 1};
dim3 blocks_for(int W, int H) { return {tcnn::div_round_up((uint32_t)W, kThreads.x), tcnn::div_round_up((uint32_t)H, kThreads.y), 1}; }

/* float [n][4] <-> Array4f [n] (copies: the caller's memory need not have Eigen's alignment) */
std::vector<Eigen::Array4f> pixels(const float* p, size_t n) {
  std::vector<Eigen::Array4f> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = Eigen::Array4f{p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]};
  return v;
}
void unpixels(const std::vector<Eigen::Array4f>& v, float* p) {
  for (size_t i = 0; i < v.size(); ++i)
    for (int k = 0; k < 4; ++k) p[4 * i + k] = v[i][k];
}

}  // namespace

extern "C" {

/* the enumerators as integers, so that the Python side can assert the numbering nerfhip.h shares with them */
int refrb_enum_value(const char* name) {
  const std::string s = name;
  if (s == "EColorSpace::Linear") return (int)ngp::EColorSpace::Linear;
  if (s == "EColorSpace::SRGB") return (int)ngp::EColorSpace::SRGB;
  if (s == "EColorSpace::VisPosNeg") return (int)ngp::EColorSpace::VisPosNeg;
  if (s == "ETonemapCurve::Identity") return (int)ngp::ETonemapCurve::Identity;
  if (s == "ETonemapCurve::ACES") return (int)ngp::ETonemapCurve::ACES;
  if (s == "ETonemapCurve::Hable") return (int)ngp::ETonemapCurve::Hable;
  if (s == "ETonemapCurve::Reinhard") return (int)ngp::ETonemapCurve::Reinhard;
  return -1;
}

/* CudaRenderBuffer::accumulate (R/src/render_buffer.cu:595-615): frame, accum float [H][W][4], accum in place */
void refrb_accumulate(int W, int H, const float* frame, float* accum, float sample_count, int color_space) {
  const size_t n = (size_t)W * H;
  std::vector<Eigen::Array4f> f = pixels(frame, n), a = pixels(accum, n);
  launch(blocks_for(W, H), kThreads, [&] {
    ngp::accumulate_kernel_on_host(Eigen::Vector2i{W, H}, f.data(), a.data(), sample_count, (ngp::EColorSpace)color_space);
  });
  unpixels(a, accum);
}

/* CudaRenderBuffer::tonemap (R/src/render_buffer.cu:617-634) up to the DLSS branch: accum, surface float [H][W][4] */
void refrb_tonemap(int W, int H, float exposure, const float background[4], const float* accum, int color_space,
                   int output_color_space, int curve, int clamp_output_color, float* surface) {
  const size_t n = (size_t)W * H;
  std::vector<Eigen::Array4f> a = pixels(accum, n);
  refshim_plane plane{reinterpret_cast<float4*>(surface), W, H};
  const Eigen::Array4f bg{background[0], background[1], background[2], background[3]};
  launch(blocks_for(W, H), kThreads, [&] {
    ngp::tonemap_kernel_on_host(Eigen::Vector2i{W, H}, exposure, bg, a.data(), (ngp::EColorSpace)color_space,
                                (ngp::EColorSpace)output_color_space, (ngp::ETonemapCurve)curve, clamp_output_color != 0, &plane);
  });
}

/* tonemap(x, curve) (R/src/render_buffer.cu:261-318): the film curve alone on n colours [n][3] */
void refrb_film_curve(uint32_t n, const float* rgb, int curve, float* out) {
  for (uint32_t i = 0; i < n; ++i) {
    const Eigen::Array3f c = ngp::tonemap(Eigen::Array3f{rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]}, (ngp::ETonemapCurve)curve);
    for (int k = 0; k < 3; ++k) out[3 * i + k] = c[k];
  }
}

/* tonemap(col, exposure, curve, color_space, output_color_space) (R/src/render_buffer.cu:320-339) on n colours [n][3] */
void refrb_tonemap_color(uint32_t n, const float* rgb, const float exposure[3], int curve, int color_space, int output_color_space,
                         float* out) {
  const Eigen::Array3f e{exposure[0], exposure[1], exposure[2]};
  for (uint32_t i = 0; i < n; ++i) {
    const Eigen::Array3f c = ngp::tonemap(Eigen::Array3f{rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]}, e, (ngp::ETonemapCurve)curve,
                                          (ngp::EColorSpace)color_space, (ngp::EColorSpace)output_color_space);
    for (int k = 0; k < 3; ++k) out[3 * i + k] = c[k];
  }
}

/* colormap_turbo (R/src/render_buffer.cu:413-429): n values -> [n][3] */
void refrb_colormap_turbo(uint32_t n, const float* x, float* rgb) {
  for (uint32_t i = 0; i < n; ++i) {
    const Eigen::Array3f c = ngp::colormap_turbo(x[i]);
    for (int k = 0; k < 3; ++k) rgb[3 * i + k] = c[k];
  }
}

/* CudaRenderBuffer::overlay_depth (R/src/render_buffer.cu:690-714): surface float [H][W][4] in place, depth [img_h][img_w] */
void refrb_overlay_depth(int W, int H, float alpha, const float* depth, float depth_scale, int img_w, int img_h, int fov_axis,
                         float zoom, float center_x, float center_y, float* surface) {
  refshim_plane plane{reinterpret_cast<float4*>(surface), W, H};
  launch(blocks_for(W, H), kThreads, [&] {
    ngp::overlay_depth_kernel_on_host(Eigen::Vector2i{W, H}, alpha, depth, depth_scale, Eigen::Vector2i{img_w, img_h}, fov_axis, zoom,
                                      Eigen::Vector2f{center_x, center_y}, &plane);
  });
}

}  // extern "C"
