/* Stand-in for tiny-cuda-nn/gpu_matrix.h: the strided view the reference's kernels index.  Element (i, j) lives at
 * data[i * stride_i + j * stride_j], as in tiny-cuda-nn; a row-major m x n matrix is viewed with strides (n, 1), a
 * column-major one with (1, m).  TEST INFRASTRUCTURE ONLY (oracle/ref_kernels.cpp). */
#ifndef REF_SHIM_TCNN_GPU_MATRIX_H_
#define REF_SHIM_TCNN_GPU_MATRIX_H_

#include <tiny-cuda-nn/common.h>

namespace tcnn {

template <class T>
struct MatrixView {  /* (the name and operator() are the interface the kernels use) */
  T* data = nullptr;
  uint32_t stride_i = 0, stride_j = 0;

  MatrixView() = default;
  MatrixView(T* d, uint32_t si, uint32_t sj) : data(d), stride_i(si), stride_j(sj) {}
  T& operator()(uint32_t row, uint32_t col = 0) const {
    const uint32_t offset = row * stride_i + col * stride_j; /* 32-bit arithmetic, as tiny-cuda-nn's view has it */
    return data[offset];
  }
};

}  // namespace tcnn

#endif
