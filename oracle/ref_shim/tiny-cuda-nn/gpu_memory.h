/* Stand-in for tiny-cuda-nn/gpu_memory.h: the render kernels include it and use nothing of it; the encoding headers' host
 * code names a workspace allocation (never made: ref_encodings.cpp instantiates no `forward_impl`).
 * TEST INFRASTRUCTURE ONLY (oracle/ref_kernels.cpp, oracle/ref_encodings.cpp). */
#ifndef REF_SHIM_TCNN_GPU_MEMORY_H_
#define REF_SHIM_TCNN_GPU_MEMORY_H_
#include <tiny-cuda-nn/common.h>

namespace tcnn {
struct GPUMemoryArena {
  struct Allocation {
    uint8_t* data() { return nullptr; }
  };
};
GPUMemoryArena::Allocation allocate_workspace(cudaStream_t stream, size_t n_bytes); /* declared only */
}  // namespace tcnn
#endif
