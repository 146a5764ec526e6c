/* Stand-in for the CUDA header of that name: the render buffer includes it for its GUI build (NGP_GUI), which is not built here.
 * TEST INFRASTRUCTURE ONLY (oracle/ref_render_buffer.cpp). */
#ifndef REF_SHIM_CUDA_GL_INTEROP_H_
#define REF_SHIM_CUDA_GL_INTEROP_H_
#include <cuda_surface_on_cpu.h>
#endif
