/* Stand-in for tiny-cuda-nn/common.h on a host compiler: the one type the reference's render kernels and the
 * vendored pcg32.h take from it.  TEST INFRASTRUCTURE ONLY (oracle/ref_kernels.cpp); written from those uses. */
#ifndef REF_SHIM_TCNN_COMMON_H_
#define REF_SHIM_TCNN_COMMON_H_

#include <cuda_on_cpu.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

/* The three macros the vendored pcg32.h expands -- the namespace opener and closer and the host/device marker -- come
 * from the compiler's command line (oracle/Makefile, REF_FLAGS). */
#if !defined(TCNN_NAMESPACE_BEGIN) || !defined(TCNN_NAMESPACE_END) || !defined(TCNN_HOST_DEVICE)
#error "build with oracle/Makefile's `ref` target: it defines the tcnn namespace macros"
#endif
#define TCNN_HALF_PRECISION 1

namespace tcnn {
typedef __half network_precision_t; /* the reference builds its network in half precision */
}

#endif
