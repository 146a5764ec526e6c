/* Stand-in for tiny-cuda-nn/random.h: the generator type, taken from the pcg32.h the reference vendors (found on the include
 * path at build time, never copied).  TEST INFRASTRUCTURE ONLY (oracle/ref_kernels.cpp, oracle/ref_encodings.cpp). */
#ifndef REF_SHIM_TCNN_RANDOM_H_
#define REF_SHIM_TCNN_RANDOM_H_

#include <tiny-cuda-nn/common.h>

#include <pcg32/pcg32.h>

namespace tcnn {
typedef pcg32 default_rng_t;
/* named by the grid encoding's `initialize_params`; there is no device to fill: calling it is an error */
template <typename T, typename RNG>
void generate_random_uniform(RNG&, size_t, T*, T = 0, T = 1) { throw std::logic_error("generate_random_uniform: not available on the CPU"); }
}  // namespace tcnn

#endif
