/* Stand-in for tiny-cuda-nn/random.h: the generator type, taken from the pcg32.h the reference vendors (found on the include
 * path at build time, never copied).  TEST INFRASTRUCTURE ONLY (oracle/ref_kernels.cpp). */
#ifndef REF_SHIM_TCNN_RANDOM_H_
#define REF_SHIM_TCNN_RANDOM_H_

#include <tiny-cuda-nn/common.h>

#include <pcg32/pcg32.h>

namespace tcnn {
typedef pcg32 default_rng_t;
}  // namespace tcnn

#endif
