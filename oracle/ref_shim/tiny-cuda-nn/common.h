/* Stand-in for tiny-cuda-nn/common.h on a host compiler: what the reference's render kernels, its encoding headers and the
 * vendored pcg32.h take from it.  TEST INFRASTRUCTURE ONLY (oracle/ref_kernels.cpp, oracle/ref_encodings.cpp); written from
 * those uses: names, signatures and the meaning the call sites rely on. */
#ifndef REF_SHIM_TCNN_COMMON_H_
#define REF_SHIM_TCNN_COMMON_H_

#include <cuda_fp16.h>

#include <algorithm>
#include <cctype>
#include <cstddef>
#include <cstdint>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

/* The three macros the vendored pcg32.h expands -- the namespace opener and closer and the host/device marker -- come
 * from the compiler's command line (oracle/Makefile, REF_FLAGS). */
#if !defined(TCNN_NAMESPACE_BEGIN) || !defined(TCNN_NAMESPACE_END) || !defined(TCNN_HOST_DEVICE)
#error "build with oracle/Makefile's `ref` target: it defines the tcnn namespace macros"
#endif
#define TCNN_HALF_PRECISION 1
#define TCNN_PRAGMA_UNROLL
#define CUDA_CHECK_THROW(x) ((void)(x))

/* ---- the launch vocabulary of the encoding headers' host code.  None of it runs: the member functions that launch are
 * never instantiated (ref_encodings.cpp), but their text has to parse.  `<<< >>>` needs a compiler in HIP mode, which asks
 * for the configuration call below; nothing defines it. */
struct dim3 : refshim_dim3 {
  dim3(uint32_t x_ = 1, uint32_t y_ = 1, uint32_t z_ = 1) { x = x_, y = y_, z = z_; }
};
typedef struct refshim_stream* cudaStream_t;
extern "C" unsigned __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem = 0, cudaStream_t stream = nullptr);

/* the one call of the formatting library the headers make: builds the text of an exception.  The arguments are dropped. */
namespace fmt {
template <typename... Args>
std::string format(const char* text, Args&&...) { return text; }
}  // namespace fmt

namespace tcnn {

typedef __half network_precision_t; /* the reference builds its network in half precision */

/* in the order the reference declares them: the values travel through the extern "C" boundary as integers, and
 * tests/test_reference_encodings_cpu.py asserts the order against the reference's header */
enum class Activation { ReLU, Exponential, Sine, Sigmoid, Squareplus, Softplus, None };

inline std::string to_lower(std::string s) {
  std::transform(s.begin(), s.end(), s.begin(), [](unsigned char c) { return (char)std::tolower(c); });
  return s;
}
inline bool equals_case_insensitive(const std::string& a, const std::string& b) { return to_lower(a) == to_lower(b); }

/* wrapping 32-bit power, as the grid constructor expects of it */
inline uint32_t powi(uint32_t base, uint32_t exponent) {
  uint32_t r = 1;
  while (exponent--) r *= base;
  return r;
}
template <typename T> T div_round_up(T v, T d) { return (v + d - 1) / d; }
template <typename T> T next_multiple(T v, T d) { return div_round_up(v, d) * d; }
template <typename T> T gcd(T a, T b) { return b == 0 ? a : gcd(b, (T)(a % b)); }
template <typename T> T lcm(T a, T b) { const T g = gcd(a, b); return g ? a / g * b : 0; }

/* tcnn's one-dimensional launch: 128 threads per block over n_elements, the kernel receiving n_elements first.  Here it IS
 * the emulated launch: serial loops over blockIdx.x / threadIdx.x. */
constexpr uint32_t n_threads_linear = 128;
template <typename T> constexpr uint32_t n_blocks_linear(T n) { return (uint32_t)((n + (T)n_threads_linear - 1) / (T)n_threads_linear); }
template <typename K, typename T, typename... Types>
inline void linear_kernel(K kernel, uint32_t, cudaStream_t, T n_elements, Types... args) {
  if (n_elements <= 0) return;
  gridDim = refshim_dim3{}, blockDim = refshim_dim3{}, blockIdx = refshim_dim3{}, threadIdx = refshim_dim3{};
  gridDim.x = n_blocks_linear(n_elements), blockDim.x = n_threads_linear;
  blockIdx.y = blockIdx.z = threadIdx.y = threadIdx.z = 0;
  for (uint32_t b = 0; b < gridDim.x; ++b)
    for (uint32_t t = 0; t < blockDim.x; ++t) {
      blockIdx.x = b, threadIdx.x = t;
      kernel(n_elements, args...);
    }
}

/* N values of T, indexable; `N` names the count */
template <typename T, uint32_t N_ELEMS>
struct vector_t {
  T data[N_ELEMS];
  static constexpr uint32_t N = N_ELEMS;
  T& operator[](uint32_t i) { return data[i]; }
  T operator[](uint32_t i) const { return data[i]; }
};
template <uint32_t N> using vector_fullp_t = vector_t<float, N>;
template <uint32_t N> using vector_halfp_t = vector_t<__half, N>;

/* rows of T at a byte pitch: (y) is the start of row y */
template <typename T>
struct PitchedPtr {
  T* ptr = nullptr;
  uint32_t stride_in_bytes = sizeof(T);
  PitchedPtr() = default;
  PitchedPtr(T* p, size_t stride_in_elements, size_t offset = 0, size_t extra_stride_bytes = 0)
      : ptr(p + offset), stride_in_bytes((uint32_t)(stride_in_elements * sizeof(T) + extra_stride_bytes)) {}
  T* operator()(uint32_t y) const { return (T*)((const char*)ptr + y * stride_in_bytes); }
};

}  // namespace tcnn

#endif
