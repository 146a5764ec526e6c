/*
 * cuda_on_cpu.h -- the handful of CUDA names the reference's plain-C kernels use, for a host compiler.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/ref_kernels.cpp, oracle/ref_encodings.cpp).  Written from the interfaces the kernels use, not from any CUDA or
 * tiny-cuda-nn header.  A "launch" is two nested serial loops that set blockIdx / threadIdx (ref_kernels.cpp), so there are
 * no real threads: the index variables are thread_local only so that a caller may run launches from several host threads.
 */
#ifndef REF_SHIM_CUDA_ON_CPU_H_
#define REF_SHIM_CUDA_ON_CPU_H_

#include <cmath>
#include <cstdint>
#include <cstring>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__

struct refshim_dim3 {
  uint32_t x = 1, y = 1, z = 1;
};
extern thread_local refshim_dim3 threadIdx, blockIdx, blockDim, gridDim;

struct float4 {
  float x, y, z, w;
};

/* IEEE binary16 storage with round-to-nearest-even conversions, bit-level (no F16C: the build takes no -m flag) */
struct __half {
  uint16_t bits;
  __half() = default;
  __half(float f) : bits(from_float(f)) {}
  operator float() const { return to_float(bits); }

  static uint16_t from_float(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const uint32_t mag = u & 0x7fffffffu;
    if (mag >= 0x7f800000u) return (uint16_t)(sign | (mag > 0x7f800000u ? 0x7e00u : 0x7c00u)); /* NaN / Inf */
    if (mag >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                 /* rounds to Inf */
    if (mag < 0x33000001u) return (uint16_t)sign;                                              /* <= 2^-25: zero */
    const int e = (int)(mag >> 23) - 127;
    uint32_t man = (mag & 0x7fffffu) | 0x800000u;
    int shift;
    uint32_t base;
    if (e < -14) { /* subnormal half: value = man * 2^(e-23), unit 2^-24 */
      shift = -e - 1;
      base = 0;
    } else {
      shift = 13;
      base = (uint32_t)(e + 14) << 10; /* the implicit bit adds one more to the exponent field */
    }
    const uint32_t q = man >> shift, rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1);
    uint32_t r = base + q;
    if (rem > half || (rem == half && (q & 1u))) ++r;
    return (uint16_t)(sign | r);
  }
  static float to_float(uint16_t h) {
    const uint32_t sign = ((uint32_t)h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1fu, man = h & 0x3ffu;
    uint32_t u;
    if (e == 0x1fu) {
      u = sign | 0x7f800000u | (man << 13);
    } else if (e != 0) {
      u = sign | ((e + 112u) << 23) | (man << 13);
    } else if (man == 0) {
      u = sign;
    } else {
      const float v = std::ldexp((float)man, -24);
      std::memcpy(&u, &v, 4);
      u |= sign;
    }
    float f;
    std::memcpy(&f, &u, 4);
    return f;
  }
};

/* one "thread" at a time: the plain read-modify-write is the atomic */
inline int atomicAdd(int* address, int val) {
  const int old = *address;
  *address = old + val;
  return old;
}
inline float atomicAdd(float* address, float val) {
  const float old = *address;
  *address = old + val;
  return old;
}

/* the device intrinsic's own rounding cannot be reproduced on a CPU: libm's expf stands in (tests account for it) */
inline float __expf(float x) { return expf(x); }
inline float __sinf(float x) { return sinf(x); }
inline float __cosf(float x) { return cosf(x); }
/* named by transfer functions of common_device.h that nothing here calls */
inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
inline float normcdff(float x) { return 0.5f * erfcf(-x * 0.70710678118654752440f); }
inline float __saturatef(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

inline int min(int a, int b) { return b < a ? b : a; }
inline int max(int a, int b) { return a < b ? b : a; }
inline unsigned min(unsigned a, unsigned b) { return b < a ? b : a; }
inline unsigned max(unsigned a, unsigned b) { return a < b ? b : a; }
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }

#endif
