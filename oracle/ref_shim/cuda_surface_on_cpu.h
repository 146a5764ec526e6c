/*
 * cuda_surface_on_cpu.h -- the surface and array vocabulary of the reference's render buffer, for a host compiler.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/ref_render_buffer.cpp).  Written from the uses in that file's kernels and host methods, not
 * from any CUDA header.  A surface object is a handle to a host plane of float4 texels with its width; surf2Dread / surf2Dwrite
 * address it as the kernels do, x in BYTES and y in rows.  The array and surface create / destroy calls are plain allocations.
 */
#ifndef REF_SHIM_CUDA_SURFACE_ON_CPU_H_
#define REF_SHIM_CUDA_SURFACE_ON_CPU_H_

#include <tiny-cuda-nn/common.h>

#include <atomic>
#include <cassert>
#include <cstdlib>
#include <cstring>

struct refshim_plane {
  float4* texels;
  int width, height;
};
/* pointers: the render buffer assigns 0 to them and tests them as booleans */
typedef refshim_plane* cudaArray_t;
typedef refshim_plane* cudaSurfaceObject_t;
typedef int cudaError_t;
enum { cudaSuccess = 0 };

inline void surf2Dread(float4* out, cudaSurfaceObject_t s, int x_in_bytes, int y) {
  *out = s->texels[(size_t)y * s->width + (size_t)x_in_bytes / sizeof(float4)];
}
inline void surf2Dwrite(float4 v, cudaSurfaceObject_t s, int x_in_bytes, int y) {
  s->texels[(size_t)y * s->width + (size_t)x_in_bytes / sizeof(float4)] = v;
}

struct cudaChannelFormatDesc {
  int bytes;
};
template <typename T>
cudaChannelFormatDesc cudaCreateChannelDesc() { return {(int)sizeof(T)}; }
enum { cudaArraySurfaceLoadStore = 2 };
inline cudaError_t cudaMallocArray(cudaArray_t* array, const cudaChannelFormatDesc*, size_t width, size_t height, unsigned = 0) {
  *array = new refshim_plane{(float4*)std::calloc(width * height, sizeof(float4)), (int)width, (int)height};
  return cudaSuccess;
}
inline cudaError_t cudaFreeArray(cudaArray_t array) {
  if (array) std::free(array->texels);
  delete array;
  return cudaSuccess;
}
enum cudaResourceType { cudaResourceTypeArray = 0 };
struct cudaResourceDesc {
  cudaResourceType resType;
  struct {
    struct {
      cudaArray_t array;
    } array;
  } res;
};
/* the surface of an array is the array's own plane */
inline cudaError_t cudaCreateSurfaceObject(cudaSurfaceObject_t* surface, const cudaResourceDesc* desc) {
  *surface = desc->res.array.array;
  return cudaSuccess;
}
inline cudaError_t cudaDestroySurfaceObject(cudaSurfaceObject_t) { return cudaSuccess; }
inline cudaError_t cudaMemsetAsync(void* p, int value, size_t bytes, cudaStream_t) {
  std::memset(p, value, bytes);
  return cudaSuccess;
}

/* What stands where a kernel's name is LAUNCHED (`name<<<grid, block>>>(args)`): the compiler in HIP mode refuses a launch of a
 * plain function, and the kernels here are plain functions.  ref_render_buffer.cpp renames each kernel's DEFINITION with a
 * function-like macro -- it expands where the name is followed by `(`, not where `<<<` follows -- and declares one of these under
 * the kernel's own name, so that the host methods' launches parse.  They never run: that file launches by hand. */
struct refshim_never_launched {
  template <typename... Args>
  void operator()(Args&&...) const { std::abort(); }
};

#endif
