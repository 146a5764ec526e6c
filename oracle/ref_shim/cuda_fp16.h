/*
 * cuda_fp16.h -- stand-in for the CUDA header of that name: the arithmetic the reference's encoding and activation kernels do
 * on `__half` values, for a host compiler.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/ref_encodings.cpp).  Written from the operators those kernels use (`+=`, `*`, `>`), not
 * from any CUDA header.  The storage type and its round-to-nearest-even conversions are cuda_on_cpu.h's.
 *
 * Every operator computes in binary32 and rounds the result to binary16 once.  That gives the bits of a native half
 * operation:
 *   `*`  the product of two 11-bit significands has at most 22 bits: it is exact in binary32, so there is one rounding.
 *   `+`  the sum of two binary16 values is exact in binary32 unless their exponents lie far apart (binary16 spans 2^-24 ..
 *        2^15, binary32 holds 24 bits).  Where it is not exact the smaller operand lies wholly below the larger one's sticky
 *        position, and binary32's p = 24 >= 2 * 11 + 2 makes the double rounding innocuous (Figueroa: rounding to p' >= 2p + 2
 *        bits and then to p bits equals rounding to p bits at once, for +, -, *, /, sqrt).
 *        tests/test_reference_encodings_cpu.py checks it over 2^16 x 256 pairs of bit patterns against an exact sum.
 *   `>`  the conversion to binary32 is exact and order preserving; NaN compares false, as on the device.
 */
#ifndef REF_SHIM_CUDA_FP16_H_
#define REF_SHIM_CUDA_FP16_H_

#include <cuda_on_cpu.h>

inline __half operator+(__half a, __half b) { return __half((float)a + (float)b); }
inline __half operator-(__half a, __half b) { return __half((float)a - (float)b); }
inline __half operator*(__half a, __half b) { return __half((float)a * (float)b); }
inline __half& operator+=(__half& a, __half b) { return a = a + b; }
inline bool operator>(__half a, __half b) { return (float)a > (float)b; }
inline bool operator<(__half a, __half b) { return (float)a < (float)b; }

#endif
