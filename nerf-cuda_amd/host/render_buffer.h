// render_buffer.h -- C++ mirror of the reference's ngp::CudaRenderBuffer presentation API
// (include/nerf-cuda/render_buffer.h:160-315) on the C ABI: same method names for resize,
// reset_accumulation, spp, frame/depth/accumulate buffers, clear_frame, accumulate, tonemap,
// host_to_accumulate_buffer, accumulate_buffer_host, overlay_depth, overlay_image, overlay_false_color (error_map makes what the last one
// reads: the reference fills its error map while training); enable_upscale / set_upscale_sharpening / upscale stand where the
// reference has DLSS (a proprietary binary: the deterministic spatial upscaler of nrf_rb_upscale instead, and upscale_temporal, the
// accumulator over jittered frames of nrf_rb_upscale_temporal).  GL textures and CUDA surfaces of the reference class are out of scope
// (NVIDIA/GL presentation): the surface is a plain float4 plane.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/nerfhip.h"
#include "nerf_render.h"

namespace ngp {

enum class EColorSpace : int { Linear = NRF_CS_LINEAR, SRGB = NRF_CS_SRGB, VisPosNeg = NRF_CS_VISPOSNEG };
enum class EImageDataType : int { None = 0, Byte = NRF_IMG_BYTE, Half = NRF_IMG_HALF, Float = NRF_IMG_FLOAT };
enum class ETonemapCurve : int { Identity = NRF_TM_IDENTITY, ACES = NRF_TM_ACES, Hable = NRF_TM_HABLE, Reinhard = NRF_TM_REINHARD };

class RenderBuffer {
 public:
  explicit RenderBuffer(int device = 0) { ok(nrf_rb_create(device, &m_rb)); }
  ~RenderBuffer() { nrf_rb_destroy(m_rb); }
  RenderBuffer(const RenderBuffer&) = delete;
  RenderBuffer& operator=(const RenderBuffer&) = delete;

  void resize(const Vector2i& res) { ok(nrf_rb_resize(m_rb, res[0], res[1])); m_res = res; }
  Vector2i in_resolution() const { int i[2] = {0, 0}; ok(nrf_rb_resolutions(m_rb, i, nullptr)); return Vector2i(i[0], i[1]); }
  Vector2i out_resolution() const { int o[2] = {0, 0}; ok(nrf_rb_resolutions(m_rb, nullptr, o)); return Vector2i(o[0], o[1]); }
  // The upscaler, where the reference class has enable_dlss / disable_dlss / set_dlss_sharpening: a spatial bicubic reconstruction with
  // a clamped unsharp mask in one launch (nrf_rb_upscale), from the surface as it is to a plane of out_resolution().  Not DLSS: one
  // frame in, no motion vectors, no depth, and a host can replay it bit for bit (include/nerfhip.h).
  void enable_upscale(const Vector2i& out_res) { ok(nrf_rb_enable_upscale(m_rb, out_res[0], out_res[1])); }
  void disable_upscale() { ok(nrf_rb_disable_upscale(m_rb)); }
  void set_upscale_sharpening(float amount) { ok(nrf_rb_set_upscale_sharpening(m_rb, amount)); }
  // rgba8: optional device uint32 [out_h][out_w]
  void upscale(void* rgba8 = nullptr, void* stream = nullptr) { ok(nrf_rb_upscale(m_rb, rgba8, stream)); }
  void* upscaled() const { void* p = nullptr; ok(nrf_rb_upscaled(m_rb, &p)); return p; }
  std::vector<float> upscaled_host() {
    const Vector2i out = out_resolution();
    std::vector<float> v((size_t)out[0] * out[1] * 4);
    ok(nrf_rb_read_upscaled(m_rb, v.data()));
    return v;
  }
  // The temporal upscaler, driven the way the reference drives DLSS (render_buffer.cu:636-653): a sub-pixel jitter per frame
  // (upscale_jitter(k): render frame k with cam.cx - jitter[0], cam.cy - jitter[1]), a reset flag, optional motion vectors (device
  // float2 [in_h][in_w] in output pixels, NerfRender-independent: nrf_motion_vectors).  An accumulator at out_resolution(), defined in
  // include/nerfhip.h operation by operation; no learned filter
  static void upscale_jitter(uint32_t index, float jitter[2]) { ok(nrf_rb_upscale_jitter(index, jitter)); }
  void set_upscale_history(float max_history) { ok(nrf_rb_set_upscale_history(m_rb, max_history)); }
  void upscale_temporal(const float jitter[2], const void* motion = nullptr, bool reset = false, bool rectify = false, void* rgba8 = nullptr,
                        void* stream = nullptr) {
    nrf_upscale_temporal t{};
    t.motion = motion;
    t.jitter[0] = jitter[0], t.jitter[1] = jitter[1];
    t.flags = (reset ? (uint32_t)NRF_UPSCALE_T_RESET : 0u) | (rectify ? (uint32_t)NRF_UPSCALE_T_RECTIFY : 0u);
    ok(nrf_rb_upscale_temporal(m_rb, &t, rgba8, stream));
  }
  uint32_t upscale_frames() const { uint32_t n = 0; ok(nrf_rb_upscale_history(m_rb, nullptr, nullptr, &n)); return n; }
  // the history colour [out_h][out_w][4] (unsharpened) and its weight [out_h][out_w] as the last upscale_temporal left them
  void upscale_history_host(std::vector<float>& rgba, std::vector<float>& weight) {
    const Vector2i out = out_resolution();
    rgba.resize((size_t)out[0] * out[1] * 4);
    weight.resize((size_t)out[0] * out[1]);
    ok(nrf_rb_read_upscale_history(m_rb, rgba.data(), weight.data()));
  }
  void reset_accumulation() { ok(nrf_rb_reset_accumulation(m_rb)); }
  uint32_t spp() const { uint32_t v = 0; ok(nrf_rb_spp(m_rb, &v)); return v; }
  void set_color_space(EColorSpace cs) { ok(nrf_rb_set_color_space(m_rb, (int)cs)); }
  void set_tonemap_curve(ETonemapCurve c) { ok(nrf_rb_set_tonemap_curve(m_rb, (int)c)); }
  void* frame_buffer() const { void* p = nullptr; ok(nrf_rb_buffers(m_rb, &p, nullptr, nullptr, nullptr)); return p; }
  void* depth_buffer() const { void* p = nullptr; ok(nrf_rb_buffers(m_rb, nullptr, &p, nullptr, nullptr)); return p; }
  void* accumulate_buffer() const { void* p = nullptr; ok(nrf_rb_buffers(m_rb, nullptr, nullptr, &p, nullptr)); return p; }
  void* surface() const { void* p = nullptr; ok(nrf_rb_buffers(m_rb, nullptr, nullptr, nullptr, &p)); return p; }
  std::vector<float> accumulate_buffer_host() {
    std::vector<float> v((size_t)m_res[0] * m_res[1] * 4);
    ok(nrf_rb_read(m_rb, v.data(), nullptr));
    return v;
  }
  std::vector<float> surface_host() {
    std::vector<float> v((size_t)m_res[0] * m_res[1] * 4);
    ok(nrf_rb_read(m_rb, nullptr, v.data()));
    return v;
  }
  void host_to_accumulate_buffer(const unsigned char* rgb, int size) { ok(nrf_rb_host_to_accumulate_buffer(m_rb, rgb, size)); }
  void clear_frame(void* stream = nullptr) { ok(nrf_rb_clear_frame(m_rb, stream)); }
  void accumulate(float exposure, void* stream = nullptr) { ok(nrf_rb_accumulate(m_rb, exposure, stream)); }
  void tonemap(float exposure, const float background_color[4], EColorSpace output_color_space, void* stream = nullptr) {
    ok(nrf_rb_tonemap(m_rb, exposure, background_color, (int)output_color_space, stream));
  }
  // accumulate() + tonemap() as one pass over the planes (nrf_rb_present); rgba8: optional device uint32 [h][w]
  void present(float exposure, const float background_color[4], EColorSpace output_color_space, void* rgba8 = nullptr, void* stream = nullptr) {
    ok(nrf_rb_present(m_rb, exposure, background_color, (int)output_color_space, rgba8, stream));
  }
  // overlay_depth(), render_buffer.h:259-268: `depth` is a device float plane of `resolution` (e.g. depth_buffer())
  void overlay_depth(float alpha, const float* depth, float depth_scale, const Vector2i& resolution, int fov_axis, float zoom,
                     const float screen_center[2], void* stream = nullptr) {
    ok(nrf_rb_overlay_depth(m_rb, alpha, depth, depth_scale, resolution[0], resolution[1], fov_axis, zoom, screen_center, stream));
  }
  // overlay_image(), render_buffer.h:244-257: `image` is a device image of `image_resolution` texels of `image_data_type` (Byte: uint32
  // sRGB texels with straight alpha; Half / Float: four premultiplied linear values), put over `background_color`, developed with the
  // per-channel `exposure` and the buffer's curve, and blended over the surface with weight `alpha` (nrf_rb_overlay_image)
  void overlay_image(float alpha, const float exposure[3], const float background_color[4], EColorSpace output_color_space, const void* image,
                     EImageDataType image_data_type, const Vector2i& image_resolution, int fov_axis, float zoom, const float screen_center[2],
                     void* stream = nullptr) {
    ok(nrf_rb_overlay_image(m_rb, alpha, exposure, background_color, (int)output_color_space, image, (int)image_data_type, image_resolution[0],
                            image_resolution[1], fov_axis, zoom, screen_center, stream));
  }
  // overlay_false_color(), render_buffer.h:270: the surface's grey times the colour map of a device error map over its average.
  // `to_srgb` is accepted and ignored: it is dead in the reference's kernel (nrf_rb_overlay_false_color)
  void overlay_false_color(const Vector2i& training_resolution, bool to_srgb, int fov_axis, void* stream, const float* error_map,
                           const Vector2i& error_map_resolution, const float* average, float brightness, bool viridis) {
    (void)to_srgb;
    ok(nrf_rb_overlay_false_color(m_rb, training_resolution[0], training_resolution[1], fov_axis, error_map, error_map_resolution[0],
                                  error_map_resolution[1], average, brightness, viridis ? 1 : 0, stream));
  }
  // what overlay_false_color reads, made on the device: the per-cell mean squared error of the surface against a device float4 plane of
  // the surface's size, and the mean of the cells (nrf_rb_error_map); error_map: device float [h][w] of error_map_resolution,
  // average: one device float
  void error_map(const void* truth, const Vector2i& error_map_resolution, float* error_map, float* average, void* stream = nullptr) {
    ok(nrf_rb_error_map(m_rb, truth, error_map_resolution[0], error_map_resolution[1], error_map, average, stream));
  }

 private:
  static void ok(int rc) {
    if (rc != NRF_OK) throw std::runtime_error{std::string("render buffer: ") + nrf_last_error()};
  }
  nrf_render_buffer* m_rb = nullptr;
  Vector2i m_res;
};

}  // namespace ngp
