/* Stand-in for tiny-cuda-nn/gpu_matrix.h: the strided view the reference's kernels index, and the matrix descriptors the
 * encoding headers' host code names (those never run: ref_encodings.cpp instantiates no `forward_impl`).  Element (i, j) lives at
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
  /* move the origin by whole rows / columns */
  void advance(uint32_t rows, uint32_t cols) { data = &(*this)(rows, cols); }
  void advance_rows(uint32_t rows) { advance(rows, 0); }
  void advance_cols(uint32_t cols) { advance(0, cols); }
};

/* row-major = structure of arrays, column-major = array of structures: two names for each, as the headers use them */
enum class MatrixLayout { RowMajor = 0, SoA = 0, ColumnMajor = 1, AoS = 1 };
static constexpr MatrixLayout RM = MatrixLayout::RowMajor, SoA = MatrixLayout::SoA;
static constexpr MatrixLayout CM = MatrixLayout::ColumnMajor, AoS = MatrixLayout::AoS;

/* a non-owning m x n descriptor: only what the host code of the encoding headers asks of a matrix */
template <typename T>
class GPUMatrixDynamic {
 public:
  GPUMatrixDynamic() = default;
  GPUMatrixDynamic(T* data, uint32_t m, uint32_t n, MatrixLayout layout = CM) : m_data(data), m_m(m), m_n(n), m_layout(layout) {}
  uint32_t m() const { return m_m; }
  uint32_t n() const { return m_n; }
  uint32_t n_elements() const { return m_m * m_n; }
  uint32_t stride() const { return m_layout == CM ? m_m : m_n; }
  MatrixLayout layout() const { return m_layout; }
  T* data() const { return m_data; }
  PitchedPtr<T> pitched_ptr() const { return {m_data, stride()}; }
  MatrixView<T> view() const { return {m_data, m_layout == CM ? 1u : stride(), m_layout == CM ? stride() : 1u}; }

 private:
  T* m_data = nullptr;
  uint32_t m_m = 0, m_n = 0;
  MatrixLayout m_layout = CM;
};
template <typename T, MatrixLayout LAYOUT = CM>
class GPUMatrix : public GPUMatrixDynamic<T> {
 public:
  GPUMatrix() = default;
  GPUMatrix(uint32_t m, uint32_t n, cudaStream_t) : GPUMatrixDynamic<T>(nullptr, m, n, LAYOUT) {}
};

}  // namespace tcnn

#endif
