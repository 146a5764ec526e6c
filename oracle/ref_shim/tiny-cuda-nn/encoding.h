/* Stand-in for tiny-cuda-nn/encoding.h (and the object.h behind it): the enums the encoding kernels take and an empty
 * `Encoding<T>` base that declares the virtual members the four encoding classes override.  TEST INFRASTRUCTURE ONLY
 * (oracle/ref_encodings.cpp); written from those overrides.  `json` is the reference's own vendored json.hpp, found on the
 * include path at build time, never copied. */
#ifndef REF_SHIM_TCNN_ENCODING_H_
#define REF_SHIM_TCNN_ENCODING_H_

#include <tiny-cuda-nn/common.h>
#include <tiny-cuda-nn/gpu_matrix.h>
#include <tiny-cuda-nn/random.h>

#include <json/json.hpp>

#include <string>
#include <vector>

namespace tcnn {

using json = nlohmann::json;

/* in the order the reference declares them (asserted by tests/test_reference_encodings_cpu.py) */
enum class InterpolationType { Nearest, Linear, Smoothstep };
InterpolationType string_to_interpolation_type(const std::string& interpolation_type);
std::string to_string(InterpolationType interpolation_type);

enum class EGradientMode { Ignore, Overwrite, Accumulate };

struct Context {
  virtual ~Context() {}
};

template <typename T>
class Encoding {
 public:
  virtual ~Encoding() {}
  virtual std::unique_ptr<Context> forward_impl(cudaStream_t stream, const GPUMatrixDynamic<float>& input, GPUMatrixDynamic<T>* output = nullptr,
                                                bool use_inference_params = false, bool prepare_input_gradients = false) = 0;
  virtual void backward_impl(cudaStream_t stream, const Context& ctx, const GPUMatrixDynamic<float>& input, const GPUMatrixDynamic<T>& output,
                             const GPUMatrixDynamic<T>& dL_doutput, GPUMatrixDynamic<float>* dL_dinput = nullptr,
                             bool use_inference_params = false, EGradientMode param_gradients_mode = EGradientMode::Overwrite) = 0;
  virtual void backward_backward_input_impl(cudaStream_t stream, const Context& ctx, const GPUMatrixDynamic<float>& input,
                                            const GPUMatrixDynamic<float>& dL_ddLdinput, const GPUMatrixDynamic<T>& dL_doutput,
                                            GPUMatrixDynamic<T>* dL_ddLdoutput = nullptr, GPUMatrixDynamic<float>* dL_dinput = nullptr,
                                            bool use_inference_params = false, EGradientMode param_gradients_mode = EGradientMode::Overwrite) {}
  virtual uint32_t input_width() const = 0;
  virtual uint32_t padded_output_width() const = 0;
  virtual uint32_t output_width() const = 0;
  virtual uint32_t required_input_alignment() const = 0;
  virtual void set_alignment(uint32_t alignment) = 0;
  virtual uint32_t min_alignment() const = 0;
  virtual MatrixLayout preferred_output_layout() const = 0;
  virtual void set_params(T* params, T* inference_params, T* backward_params, T* gradients) {}
  virtual void initialize_params(pcg32& rnd, float* params_full_precision, T* params, T* inference_params, T* backward_params, T* gradients,
                                 float scale = 1) {}
  virtual size_t n_params() const { return 0; }
  virtual std::vector<std::pair<uint32_t, uint32_t>> layer_sizes() const { return {}; }
  virtual json hyperparams() const = 0;
};

}  // namespace tcnn

#endif
