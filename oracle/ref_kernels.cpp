/*
 * ref_kernels.cpp -- the reference's own ray set-up, march, compaction and compositing kernels, run on the CPU.
 *
 * TEST INFRASTRUCTURE ONLY.  This file holds no reference text: it includes <nerf-cuda/render_utils.h> from a reference
 * tree named at build time (oracle/Makefile, target `ref`), behind the stand-in headers of oracle/ref_shim/, and exports
 * an extern "C" ABI (refk_*) that tests/ref_kernels_py.py binds.  The library it builds (oracle/_ref/) is never committed.
 *
 * A launch `kernel<<<grid, block>>>(args)` is emulated as two nested serial loops that set blockIdx / threadIdx.  Every
 * entry point uses the launch geometry of the reference's call site (R = the reference tree):
 *   block = m_num_thread = 128 (R/include/nerf-cuda/nerf_render.h:77), grid = div_round_up(n, 128)
 *   (R/src/nerf_render.cu:257-343), (n + 128) / 128 for the two ray kernels (R/src/nerf_render.cu:376).
 * grid * block >= n, so every grid-stride loop takes one trip per thread and a `return` inside one ends one ray, as on
 * the device.  The density-grid kernels are launched as R/src/nerf_render.cu:403-420 launches them (block = H).
 *
 * Layouts are the reference's (R/src/nerf_render.cu:193-230): RM m x n -> view strides (n, 1), CM m x n -> (1, m).
 */
#include <nerf-cuda/render_utils.h>

#include <cstdint>
#include <vector>

thread_local refshim_dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace {

constexpr uint32_t kThreads = 128;  // m_num_thread

template <typename F>
void launch(uint32_t grid, uint32_t block, F&& body) {
  gridDim.x = grid;
  blockDim.x = block;
  for (uint32_t b = 0; b < grid; ++b)
    for (uint32_t t = 0; t < block; ++t) {
      blockIdx.x = b;
      threadIdx.x = t;
      body();
    }
}

inline uint32_t blocks(uint32_t n) { return ngp::div_round_up(n, kThreads); }

template <typename T>
tcnn::MatrixView<T> rm(T* p, uint32_t cols) { return {p, cols, 1u}; }
template <typename T>
tcnn::MatrixView<T> cm(T* p, uint32_t rows) { return {p, 1u, rows}; }

Eigen::Matrix4f mat4(const float* p) {
  Eigen::Matrix4f m;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) m(r, c) = p[4 * r + c];
  return m;
}

}  // namespace

extern "C" {

int refk_ngpu(void) { return NGPU; }

void refk_nerf_matrix_to_ngp(const float pose[16], float scale, float out[16]) {
  const Eigen::Matrix4f m = ngp::nerf_matrix_to_ngp(mat4(pose), scale);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) out[4 * r + c] = m(r, c);
}

/* NerfRender::generate_rays (R/src/nerf_render.cu:369-386) for one device: rays_o, rays_d are RM [3][N] */
void refk_generate_rays(const float cam[4], const float pose[16], float scale, int W, int N, int gpuid, float* rays_o,
                        float* rays_d) {
  const Eigen::Matrix4f new_pose = ngp::nerf_matrix_to_ngp(mat4(pose), scale);
  ngp::Camera c{cam[0], cam[1], cam[2], cam[3]};
  const uint32_t grid_size = (uint32_t)((N + (int)kThreads) / (int)kThreads);
  const Eigen::Vector3f origin = new_pose.block<3, 1>(0, 3);
  const Eigen::Matrix3f rot = new_pose.block<3, 3>(0, 0);
  launch(grid_size, kThreads, [&] { ngp::set_rays_o(rm(rays_o, (uint32_t)N), origin, N); });
  launch(grid_size, kThreads, [&] { ngp::set_rays_d(rm(rays_d, (uint32_t)N), c, rot, W, N, gpuid); });
}

void refk_near_far_from_aabb(float* rays_o, float* rays_d, float* aabb, uint32_t N, float min_near, float* nears, float* fars) {
  launch(blocks(N), kThreads, [&] {
    ngp::kernel_near_far_from_aabb(rm(rays_o, N), rm(rays_d, N), aabb, N, min_near, rm(nears, N), rm(fars, N));
  });
}

/* rays_alive int [2][N], rays_t float [2][N] */
void refk_init_step0(int* rays_alive, float* rays_t, uint32_t N, int n_alive, float* nears) {
  launch(blocks((uint32_t)n_alive), kThreads, [&] { ngp::init_step0(rm(rays_alive, N), rm(rays_t, N), n_alive, rm(nears, N)); });
}

/* returns the alive counter (zeroed before the launch, read back after it: R/src/nerf_render.cu:280-292) */
int refk_compact_rays(int n_alive, int* rays_alive, float* rays_t, uint32_t N, int i1, int i2) {
  int counter = 0;
  launch(blocks((uint32_t)n_alive), kThreads,
         [&] { ngp::kernel_compact_rays(n_alive, rm(rays_alive, N), rm(rays_t, N), rm(&counter, 1u), i1, i2); });
  return counter;
}

/* xyzs, dirs CM [3][cap] (= [cap][3] in memory), deltas CM [2][cap] */
void refk_march_rays(uint32_t n_alive, uint32_t n_step, int* rays_alive, float* rays_t, uint32_t N, float* rays_o, float* rays_d,
                     float bound, float dt_gamma, uint32_t C, uint32_t H, float* grid, float mean_density, float* nears,
                     float* fars, float* xyzs, float* dirs, float* deltas, uint32_t perturb, int i) {
  launch(blocks(n_alive), kThreads, [&] {
    ngp::kernel_march_rays(n_alive, n_step, rm(rays_alive, N), rm(rays_t, N), rm(rays_o, N), rm(rays_d, N), bound, dt_gamma, C, H,
                           grid, mean_density, rm(nears, N), rm(fars, N), cm(xyzs, 3u), cm(dirs, 3u), cm(deltas, 2u), perturb, i);
  });
}

/* sigmas RM [1][cap], rgbs RM [cap][3], deltas CM [2][cap]; weights_sum, depth RM [1][N], image RM [N][3] */
void refk_composite_rays(uint32_t n_alive, uint32_t n_step, int* rays_alive, float* rays_t, uint32_t N, float* sigmas, float* rgbs,
                         float* deltas, uint32_t cap, float* weights_sum, float* depth, float* image, int i) {
  launch(blocks(n_alive), kThreads, [&] {
    ngp::kernel_composite_rays(n_alive, n_step, rm(rays_alive, N), rm(rays_t, N), rm(sigmas, cap), rm(rgbs, 3u), cm(deltas, 2u),
                               rm(weights_sum, N), rm(depth, N), rm(image, 3u), i);
  });
}

void refk_get_image_and_depth(float* image, float* depth, float* nears, float* fars, float* weights_sum, int bg_color, uint32_t N) {
  launch(blocks(N), kThreads, [&] {
    ngp::get_image_and_depth(rm(image, 3u), rm(depth, N), rm(nears, N), rm(fars, N), rm(weights_sum, N), bg_color, N);
  });
}

/* tcnn::linear_kernel launches 128 threads per block over n_elements; weight and bias arrive as the call site's doubles
 * (`1.0/(2 * m_bound)`, `0.5`: R/src/nerf_render.cu:311-314) and narrow to the kernel's float parameters here, as there */
void refk_linear_transformer(uint32_t n_elements, double weight, double bias, const float* input, float* output) {
  launch(blocks(n_elements), kThreads, [&] { ngp::linear_transformer<float>(n_elements, weight, bias, input, output); });
}

/* `a` arrives as the call site's float m_density_scale and narrows to the kernel's int parameter (R/src/nerf_render.cu:328) */
void refk_matrix_multiply_1x1n(float a, uint32_t N, float* b) {
  launch(blocks(N), kThreads, [&] { ngp::matrix_multiply_1x1n(a, N, rm(b, N)); });
}

/* network_output: fp16 bits, RM [rows][cap]; sigmas RM [1][cap], rgbs RM [cap][3] (R/src/nerf_render.cu:324-327) */
void refk_decompose_network_in_and_out(float* sigmas, float* rgbs, uint16_t* network_output, uint32_t cap, uint32_t N) {
  static_assert(sizeof(ngp::precision_t) == 2, "precision_t is the 16-bit stand-in");
  launch(blocks(N), kThreads, [&] {
    ngp::decompose_network_in_and_out(rm(sigmas, cap), rm(rgbs, 3u), rm(reinterpret_cast<ngp::precision_t*>(network_output), cap), N,
                                      1u, 3u);
  });
}

/* the density-grid kernels, launched as R/src/nerf_render.cu:403-420 launches them: block = H */
void refk_init_xyzs(float* dd, uint32_t N, uint32_t H) {
  launch(N / H, H, [&] { ngp::init_xyzs<float>(dd, N, H); });
}
void refk_dd_scale(const float* d_s, float* d_d, uint32_t N, uint32_t H, float k, float b) {
  launch(N / H, H, [&] { ngp::dd_scale<float>(d_s, d_d, N, k, b); });
}
/* the generator is passed by value to every thread, as R/src/nerf_render.cu:413 passes m_rng[0] = default_rng_t{seed} */
void refk_add_random(float* dd, uint32_t seed, uint32_t N, uint32_t H, float k, float b) {
  const ngp::default_rng_t rng{seed};
  launch(N / H, H, [&] { ngp::add_random<float>(dd, rng, N, k, b); });
}
void refk_dg_update(float* dg, float* tmp_dg, float decay, uint32_t N, uint32_t H) {
  launch(N / H, H, [&] { ngp::dg_update<float>(dg, tmp_dg, decay, N); });
}

void refk_srgb_to_linear(const float* in, float* out, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) out[i] = ngp::srgb_to_linear(in[i]);
}
void refk_linear_to_srgb(const float* in, float* out, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) out[i] = ngp::linear_to_srgb(in[i]);
}

float refk_pcg32_first_float(uint64_t initstate, uint64_t initseq) {
  tcnn::pcg32 rng(initstate, initseq);
  return rng.next_float();
}

/* (unsigned char)(255.0 * x) of R/src/nerf_render.cu:355-358 is host code inside render_frame: restated in the Python
 * driver (tests/ref_kernels_py.py), defined only where the product lies in [0, 256) */

}  // extern "C"
