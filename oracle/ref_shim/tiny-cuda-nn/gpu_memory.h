/* Stand-in for tiny-cuda-nn/gpu_memory.h: the render kernels include it and use nothing of it; the encoding headers' host
 * code names a workspace allocation (never made: ref_encodings.cpp instantiates no `forward_impl`); the render buffer's class
 * keeps its planes in GPUMemory<T>, here a host vector with the members that class calls.
 * TEST INFRASTRUCTURE ONLY (oracle/ref_kernels.cpp, oracle/ref_encodings.cpp, oracle/ref_render_buffer.cpp). */
#ifndef REF_SHIM_TCNN_GPU_MEMORY_H_
#define REF_SHIM_TCNN_GPU_MEMORY_H_
#include <tiny-cuda-nn/common.h>

#include <cstring>
#include <vector>

namespace tcnn {
struct GPUMemoryArena {
  struct Allocation {
    uint8_t* data() { return nullptr; }
  };
};
GPUMemoryArena::Allocation allocate_workspace(cudaStream_t stream, size_t n_bytes); /* declared only */

template <typename T>
class GPUMemory {
 public:
  void resize(size_t n) { m_.resize(n); }
  void enlarge(size_t n) { if (n > m_.size()) m_.resize(n); }
  T* data() const { return const_cast<T*>(m_.data()); }
  size_t size() const { return m_.size(); }
  size_t bytes() const { return m_.size() * sizeof(T); }
  void copy_to_host(T* host) const { std::memcpy((void*)host, (const void*)m_.data(), bytes()); }
  void copy_from_host(const T* host) { std::memcpy((void*)m_.data(), (const void*)host, bytes()); }
  void copy_from_host(const std::vector<T>& host) { std::memcpy((void*)m_.data(), (const void*)host.data(), std::min(bytes(), host.size() * sizeof(T))); }

 private:
  std::vector<T> m_;
};
}  // namespace tcnn
#endif
