/*
 * ref_encodings.cpp -- the reference's own grid, direction and activation kernels, and its grid constructor, run on the CPU.
 *
 * TEST INFRASTRUCTURE ONLY.  This file holds no reference text: it includes four tiny-cuda-nn encoding headers (and, through
 * them, the real tiny-cuda-nn/common_device.h) from a reference tree named at build time (oracle/Makefile, target `ref`),
 * behind the stand-in headers of oracle/ref_shim/, and exports an extern "C" ABI (refk_*) that tests/ref_kernels_py.py binds.
 * The library it builds (oracle/_ref/libref_encodings.so) is never committed.
 *
 * The headers' host code launches with `<<< >>>`, which only a compiler in HIP (or CUDA) mode parses: this unit is built by
 * the ROCm clang as host-only HIP without the HIP headers, `__global__` and `__device__` defined away, so every kernel is a
 * plain host function.  The three member functions of GridEncodingTemplated that launch (`forward_impl`, `backward_impl`,
 * `backward_backward_input_impl`) are never instantiated: explicit specialisations below stand in their place, so that the
 * CONSTRUCTOR -- the offset table, T/include/tiny-cuda-nn/encodings/grid.h:875-940 (T = the reference's tiny-cuda-nn) -- can
 * be.  The kernels are launched here as those member functions launch them, each entry point citing its call site.
 *
 * What a CPU cannot reproduce, stated where it is used: `exp2f` (grid.h:189) and `__sinf` (frequency.h:89) are libm's here,
 * as `__expf` is in cuda_on_cpu.h -- like for like with the oracle's non-contracted reading, silent about the device's own.
 * `(uint32_t)(int)floorf(pos)` of a negative pos is not compared: positions lie in [0, 1].
 */
#include <tiny-cuda-nn/encodings/grid.h>
#include <tiny-cuda-nn/encodings/spherical_harmonics.h>
#include <tiny-cuda-nn/encodings/frequency.h>
#include <tiny-cuda-nn/encodings/identity.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <vector>

thread_local refshim_dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace tcnn {

/* hyperparams() names it; the reference defines it in a .cu file that is not built here */
std::string to_string(InterpolationType t) {
  return t == InterpolationType::Nearest ? "Nearest" : t == InterpolationType::Linear ? "Linear" : "Smoothstep";
}

/* the launching members: never the reference's bodies (see above) */
#define REFK_NO_LAUNCH(F)                                                                                                        \
  template <>                                                                                                                    \
  std::unique_ptr<Context> GridEncodingTemplated<__half, 3, F>::forward_impl(cudaStream_t, const GPUMatrixDynamic<float>&,       \
                                                                             GPUMatrixDynamic<__half>*, bool, bool) {            \
    throw std::logic_error("forward_impl: launched by hand in ref_encodings.cpp");                                               \
  }                                                                                                                              \
  template <>                                                                                                                    \
  void GridEncodingTemplated<__half, 3, F>::backward_impl(cudaStream_t, const Context&, const GPUMatrixDynamic<float>&,          \
                                                          const GPUMatrixDynamic<__half>&, const GPUMatrixDynamic<__half>&,      \
                                                          GPUMatrixDynamic<float>*, bool, EGradientMode) {                       \
    throw std::logic_error("backward_impl: out of scope");                                                                       \
  }                                                                                                                              \
  template <>                                                                                                                    \
  void GridEncodingTemplated<__half, 3, F>::backward_backward_input_impl(                                                        \
      cudaStream_t, const Context&, const GPUMatrixDynamic<float>&, const GPUMatrixDynamic<float>&, const GPUMatrixDynamic<__half>&, \
      GPUMatrixDynamic<__half>*, GPUMatrixDynamic<float>*, bool, EGradientMode) {                                                \
    throw std::logic_error("backward_backward_input_impl: out of scope");                                                        \
  }
REFK_NO_LAUNCH(1)
REFK_NO_LAUNCH(2)
REFK_NO_LAUNCH(4)
REFK_NO_LAUNCH(8)
#undef REFK_NO_LAUNCH

}  // namespace tcnn

namespace {

using tcnn::GridType;
using tcnn::InterpolationType;

/* kernel<<<grid, block>>>: serial loops that set blockIdx / threadIdx, x innermost */
template <typename Fn>
void launch(const dim3& grid, const dim3& block, Fn&& body) {
  gridDim = grid, blockDim = block;
  for (uint32_t bz = 0; bz < grid.z; ++bz)
    for (uint32_t by = 0; by < grid.y; ++by)
      for (uint32_t bx = 0; bx < grid.x; ++bx)
        for (uint32_t tz = 0; tz < block.z; ++tz)
          for (uint32_t ty = 0; ty < block.y; ++ty)
            for (uint32_t tx = 0; tx < block.x; ++tx) {
              blockIdx.x = bx, blockIdx.y = by, blockIdx.z = bz;
              threadIdx.x = tx, threadIdx.y = ty, threadIdx.z = tz;
              body();
            }
}

__half* halves(uint16_t* p) {
  static_assert(sizeof(__half) == 2, "__half is the 16-bit stand-in");
  return reinterpret_cast<__half*>(p);
}
const __half* halves(const uint16_t* p) { return reinterpret_cast<const __half*>(p); }

/* GridEncodingTemplated<__half, 3, F>::forward_impl with an AoS output (grid.h:942-1018): positions CM 3 x n (= [n][3]), out
 * CM padded x n (= [n][padded]) */
template <uint32_t F>
void grid_forward(uint32_t n, uint32_t n_features, const uint32_t* offsets, uint32_t base_resolution, float per_level_scale,
                  InterpolationType interpolation, GridType grid_type, const uint16_t* grid, const float* positions, uint16_t* out,
                  uint32_t padded) {
  const uint32_t n_levels = tcnn::div_round_up(n_features, F);  // grid.h:892
  tcnn::GridOffsetTable table;
  for (uint32_t l = 0; l <= n_levels; ++l) table.data[l] = offsets[l];
  table.size = n_levels + 1;
  const tcnn::PitchedPtr<__half> out_rows(halves(out), padded);
  // grid.h:959-963: the padding columns are written as 0 by a device lambda inside forward_impl; restated
  for (uint32_t elem = 0; elem < n; ++elem)
    for (uint32_t dim = 0; dim < padded - n_features; ++dim) out_rows(elem)[n_features + dim] = __half(0.0f);
  std::vector<__half> soa((size_t)n * n_features);  // grid.h:978-983: the SoA workspace
  // grid.h:975-976, 989-1004: 512 threads, blocks {div_round_up(n, 512), n_levels, 1}; quantize_threshold and max_level are
  // GridEncoding's defaults (grid.h:850-856), max_level_gpu and dy_dx are null
  launch(dim3{tcnn::div_round_up(n, 512u), n_levels, 1}, dim3{512u}, [&] {
    tcnn::kernel_grid<__half, 3, F>(n, n_features, table, base_resolution, std::log2(per_level_scale), 0.f, 1000.f, nullptr, interpolation,
                                    grid_type, halves(grid), tcnn::MatrixView<const float>(positions, 1u, 3u), soa.data(), nullptr);
  });
  // grid.h:1006-1015
  const dim3 threads_transpose = {n_levels * F, 8, 1};
  launch(dim3{tcnn::div_round_up(n, threads_transpose.y)}, threads_transpose,
         [&] { tcnn::transpose_encoded_position<__half>(n, soa.data(), out_rows); });
}

/* the constructor (grid.h:875-940).  Its per-level resolution is a local: built with TCNN_VERBOSE_MEMORY_ALLOCS, the
 * constructor itself prints it (grid.h:925-927), and that line is read back here. */
template <uint32_t F>
int grid_table(uint32_t n_features, uint32_t log2_hashmap_size, uint32_t base_resolution, float per_level_scale, GridType grid_type,
               uint32_t* offsets, uint32_t* resolutions, uint64_t* n_params) {
  std::ostringstream said;
  std::streambuf* const before = std::cout.rdbuf(said.rdbuf());
  int rc = 0;
  try {
    tcnn::GridEncodingTemplated<__half, 3, F> enc{n_features, log2_hashmap_size, base_resolution, per_level_scale, false,
                                                  InterpolationType::Linear, grid_type};
    const uint32_t n_levels = tcnn::div_round_up(n_features, F);
    for (uint32_t l = 0; l <= n_levels; ++l) offsets[l] = (uint32_t)enc.level_params_offset(l);
    *n_params = enc.n_params();
    std::istringstream lines(said.str());
    std::string line;
    uint32_t l = 0;
    while (std::getline(lines, line)) {
      const size_t at = line.find("resolution=");
      if (at == std::string::npos || l >= n_levels) { rc = 2; break; }
      resolutions[l++] = (uint32_t)std::strtoul(line.c_str() + at + 11, nullptr, 10);
    }
    if (!rc && l != n_levels) rc = 2;
  } catch (const std::exception&) {
    rc = 1;  // the reference refuses this model
  }
  std::cout.rdbuf(before);
  return rc;
}

#define REFK_BY_F(F_, call)                 \
  switch (F_) {                             \
    case 1: { constexpr uint32_t F = 1; call; } break; \
    case 2: { constexpr uint32_t F = 2; call; } break; \
    case 4: { constexpr uint32_t F = 4; call; } break; \
    case 8: { constexpr uint32_t F = 8; call; } break; \
    default: return -1;                     \
  }

}  // namespace

extern "C" {

/* the enumerators as integers, so that the Python side can assert the order the stand-ins declare */
int refk_enum_value(const char* name) {
  const std::string s = name;
  if (s == "GridType::Hash") return (int)GridType::Hash;
  if (s == "GridType::Dense") return (int)GridType::Dense;
  if (s == "GridType::Tiled") return (int)GridType::Tiled;
  if (s == "InterpolationType::Nearest") return (int)InterpolationType::Nearest;
  if (s == "InterpolationType::Linear") return (int)InterpolationType::Linear;
  if (s == "InterpolationType::Smoothstep") return (int)InterpolationType::Smoothstep;
  if (s == "Activation::ReLU") return (int)tcnn::Activation::ReLU;
  if (s == "Activation::Exponential") return (int)tcnn::Activation::Exponential;
  if (s == "Activation::Sine") return (int)tcnn::Activation::Sine;
  if (s == "Activation::Sigmoid") return (int)tcnn::Activation::Sigmoid;
  if (s == "Activation::Squareplus") return (int)tcnn::Activation::Squareplus;
  if (s == "Activation::Softplus") return (int)tcnn::Activation::Softplus;
  if (s == "Activation::None") return (int)tcnn::Activation::None;
  return -1;
}

int refk_grid_encode(uint32_t n_features_per_level, uint32_t n, uint32_t n_features, const uint32_t* offsets, uint32_t base_resolution,
                     float per_level_scale, int interpolation, int grid_type, const uint16_t* grid, const float* positions, uint16_t* out,
                     uint32_t padded) {
  REFK_BY_F(n_features_per_level, grid_forward<F>(n, n_features, offsets, base_resolution, per_level_scale, (InterpolationType)interpolation,
                                                  (GridType)grid_type, grid, positions, out, padded));
  return 0;
}

/* 0: offsets[n_levels + 1], resolutions[n_levels], n_params filled; 1: the constructor threw */
int refk_grid_table(uint32_t n_features_per_level, uint32_t n_features, uint32_t log2_hashmap_size, uint32_t base_resolution,
                    float per_level_scale, int grid_type, uint32_t* offsets, uint32_t* resolutions, uint64_t* n_params) {
  int rc = -1;
  REFK_BY_F(n_features_per_level,
            rc = grid_table<F>(n_features, log2_hashmap_size, base_resolution, per_level_scale, (GridType)grid_type, offsets, resolutions, n_params));
  return rc;
}

/* grid_index<3, F> with feature 0 (grid.h:100-117) over n corner coordinates [n][3] */
int refk_grid_index(uint32_t n_features_per_level, int grid_type, uint32_t hashmap_size, uint32_t grid_resolution, uint32_t n,
                    const uint32_t* pos_grid, uint32_t* out) {
  REFK_BY_F(n_features_per_level, for (uint32_t i = 0; i < n; ++i) out[i] =
                                      (tcnn::grid_index<3, F>((GridType)grid_type, 0, hashmap_size, grid_resolution, pos_grid + 3 * (size_t)i)));
  return 0;
}

void refk_fast_hash3(uint32_t n, const uint32_t* pos_grid, uint32_t* out) {
  for (uint32_t i = 0; i < n; ++i) out[i] = tcnn::fast_hash<3>(pos_grid + 3 * (size_t)i);
}

/* SphericalHarmonicsEncoding::forward_impl (spherical_harmonics.h:424-430): dirs CM 3 x n, out CM padded x n */
void refk_sh(uint32_t n, uint32_t degree, uint32_t n_to_pad, const float* dirs, uint16_t* out) {
  const uint32_t padded = degree * degree + n_to_pad;
  tcnn::linear_kernel(tcnn::kernel_sh<__half>, 0, nullptr, n, degree, n_to_pad, tcnn::MatrixView<const float>(dirs, 1u, 3u),
                      tcnn::MatrixView<__half>(halves(out), 1u, padded));
}

/* FrequencyEncoding::forward_impl (frequency.h:142-150) */
void refk_frequency(uint32_t n, uint32_t n_frequencies, uint32_t n_to_pad, const float* dirs, uint16_t* out) {
  const uint32_t padded = 3 * n_frequencies * 2 + n_to_pad;
  tcnn::linear_kernel(tcnn::frequency_encoding<__half>, 0, nullptr, n * padded, n_frequencies, 3u, n_to_pad,
                      tcnn::MatrixView<const float>(dirs, 1u, 3u), tcnn::MatrixView<__half>(halves(out), 1u, padded), (float*)nullptr);
}

/* IdentityEncoding::forward_impl (identity.h:109-119); scale 1 and offset 0 are the constructor's defaults (identity.h:93) */
void refk_identity(uint32_t n, uint32_t n_to_pad, float scale, float offset, const float* dirs, uint16_t* out) {
  const uint32_t padded = 3 + n_to_pad;
  tcnn::linear_kernel(tcnn::identity<__half>, 0, nullptr, n * padded, n, 3u, n_to_pad, scale, offset,
                      tcnn::MatrixView<const float>(dirs, 1u, 3u), tcnn::MatrixView<__half>(halves(out), 1u, padded));
}

/* warp_activation<__half> on a one-element fragment (common_device.h:68-114) */
void refk_activation(int activation, uint32_t n, const uint16_t* in, uint16_t* out) {
  typedef tcnn::VectorFragment<tcnn::vector_t<__half, 1>> frag_t;
  for (uint32_t i = 0; i < n; ++i) {
    frag_t frag, result;
    std::memcpy(&frag.x[0], in + i, 2);
    result = frag;
    tcnn::warp_activation<__half>((tcnn::Activation)activation, frag, result);
    std::memcpy(out + i, &result.x[0], 2);
  }
}

/* the stand-in's half arithmetic, for the test of its rounding argument (cuda_fp16.h) */
void refk_half_add(uint32_t n, const uint16_t* a, const uint16_t* b, uint16_t* out) {
  for (uint32_t i = 0; i < n; ++i) {
    const __half r = halves(a)[i] + halves(b)[i];
    std::memcpy(out + i, &r, 2);
  }
}

}  // extern "C"
