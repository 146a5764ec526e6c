/* Stand-in for tiny-cuda-nn/multi_stream.h: the grid encoding's `forward_impl` names a set of streams (never made:
 * ref_encodings.cpp instantiates no `forward_impl`).  TEST INFRASTRUCTURE ONLY (oracle/ref_encodings.cpp). */
#ifndef REF_SHIM_TCNN_MULTI_STREAM_H_
#define REF_SHIM_TCNN_MULTI_STREAM_H_
#include <tiny-cuda-nn/common.h>

namespace tcnn {
struct SyncedMultiStream {
  SyncedMultiStream(cudaStream_t stream, size_t n_streams);
  cudaStream_t get(size_t idx);
};
}  // namespace tcnn
#endif
