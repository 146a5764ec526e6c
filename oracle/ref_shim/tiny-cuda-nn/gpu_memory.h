/* Stand-in for tiny-cuda-nn/gpu_memory.h: the render kernels include it and use nothing of it.
 * TEST INFRASTRUCTURE ONLY (oracle/ref_kernels.cpp). */
#ifndef REF_SHIM_TCNN_GPU_MEMORY_H_
#define REF_SHIM_TCNN_GPU_MEMORY_H_
#include <tiny-cuda-nn/common.h>
#endif
