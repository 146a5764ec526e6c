// nrf_renderbuffer.hip -- the presentation chain behind the reference's CudaRenderBuffer on gfx950.
//
// What the reference does with a rendered frame (R/src/render_buffer.cu): fold it into a running mean over samples per
// pixel (accumulate, :224-259, :590-609), then develop that mean for display -- background blend, exposure, film curve,
// transfer function (tonemap, :261-342, :529-556, :611-627) -- two launches that each read and write whole planes
// (32 B read + 16 B written per pixel, twice).  Here the chain is ONE streaming pass, `present_kernel`: per pixel it reads
// the frame (and the mean so far, unless this is the first sample: nothing is cleared, nothing is read), writes the new
// mean, develops it in registers and writes the surface -- plus, on request, the surface as packed 8-bit RGBA, which is what
// a display or an encoder takes.  64 B per pixel (48 for the first sample) instead of 96 (+ a 16 B clear).  The two halves
// stay available on their own (nrf_rb_accumulate / nrf_rb_tonemap: the reference's call shape) as instances of the same
// kernel, so the fused pass is bit-identical to the two calls by construction.
// Everything that does not depend on the pixel is settled on the host once per call: 2^exposure, the background in the
// render colour space, the coefficients of the film curve (`FilmCurve`: identity, Reinhard, or a ratio of two quadratics --
// ACES and Hable differ only in six numbers).  A pure stream over 16-byte pixels: one lane per pixel, grid-stride.
// Where the reference class has DLSS (enable_dlss, set_dlss_sharpening, in_/out_resolution) this one has the upscaler: the state
// and the entry points are here, the definition is nrf_upscale_plan.h and the kernel nrf_kernels_upscale.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nerfhip.h"
#include "nrf_overlay_plan.h"
#include "nrf_temporal_plan.h"
#include "nrf_upscale_plan.h"

namespace {

thread_local std::string g_rb_err;
extern "C" const char* nrf_last_error(void);

// the sRGB pair, the film curves and the colour maps are nrf_overlay_plan.h's: one text for these kernels, the overlay kernels and the host
using nrf::colormap_turbo;
using nrf::decode_srgb;
using nrf::encode_srgb;
using nrf::film_curve;
using nrf::FilmCurve;
static_assert(nrf::CS_LINEAR == NRF_CS_LINEAR && nrf::CS_SRGB == NRF_CS_SRGB && nrf::CS_VISPOSNEG == NRF_CS_VISPOSNEG, "the plan's colour spaces");
static_assert(nrf::TM_IDENTITY == NRF_TM_IDENTITY && nrf::TM_ACES == NRF_TM_ACES && nrf::TM_HABLE == NRF_TM_HABLE && nrf::TM_REINHARD == NRF_TM_REINHARD,
              "the plan's curves");
static_assert(nrf::IMG_BYTE == NRF_IMG_BYTE && nrf::IMG_HALF == NRF_IMG_HALF && nrf::IMG_FLOAT == NRF_IMG_FLOAT, "the plan's image data types");

// one call's pixel-independent state
struct PresentArgs {
  int n;
  float samples_so_far;  // the mean in the accumulate plane is over this many frames (0: the plane's content is ignored)
  float gain;            // 2^exposure
  float4 backdrop;       // the background colour in the RENDER colour space, alpha untouched
  int render_space, display_space;  // NRF_CS_*
  int clamp_display;
  FilmCurve film;
};

// fold one frame sample into the mean over `k` earlier ones: (mean * k + x) / (k + 1)
__device__ __forceinline__ float fold1(float mean, float x, float k) { return (mean * k + x) / (k + 1); }
__device__ __forceinline__ float4 fold_sample(float4 mean, float4 x, const PresentArgs& A) {
  const float k = A.samples_so_far;
  if (A.render_space == NRF_CS_VISPOSNEG) {  // a signed quantity kept as (positive part, negative part) in r, g; b is left alone
    const float signed_mean = fold1(mean.x - mean.y, x.x - x.y, k);
    mean.x = fmaxf(signed_mean, 0.0f);
    mean.y = fmaxf(-signed_mean, 0.0f);
  } else {
    if (A.render_space == NRF_CS_SRGB) {  // the mean is kept in display-referred values
      x.x = encode_srgb(x.x);
      x.y = encode_srgb(x.y);
      x.z = encode_srgb(x.z);
    }
    mean.x = fold1(mean.x, x.x, k);
    mean.y = fold1(mean.y, x.y, k);
    mean.z = fold1(mean.z, x.z, k);
  }
  mean.w = fold1(mean.w, x.w, k);
  return mean;
}

// the mean as it goes to the display: over the backdrop, exposed, through the film curve, in the display's transfer function
__device__ __forceinline__ float4 develop(float4 mean, const PresentArgs& A) {
  const float uncovered = (1 - mean.w) * A.backdrop.w;
  float c[3] = {mean.x + A.backdrop.x * uncovered, mean.y + A.backdrop.y * uncovered, mean.z + A.backdrop.z * uncovered};
  const float alpha = mean.w + uncovered;
  const float gain[3] = {A.gain, A.gain, A.gain};
  nrf::develop_color(c, A.render_space, gain, A.film, A.display_space);
  float4 out = make_float4(c[0], c[1], c[2], alpha);
  if (A.clamp_display) {
    out.x = fminf(fmaxf(out.x, 0.f), 1.f);
    out.y = fminf(fmaxf(out.y, 0.f), 1.f);
    out.z = fminf(fmaxf(out.z, 0.f), 1.f);
    out.w = fminf(fmaxf(out.w, 0.f), 1.f);
  }
  return out;
}

// the library's 8-bit rule (nrf_render.h quant_u8, the reference's (unsigned char)(255.0 * x) made safe: saturating, NaN -> 0)
__device__ __forceinline__ uint32_t to_u8(float v) {
  const double s = 255.0 * (double)v;
  if (!(s > 0.0)) return 0u;
  if (s >= 255.0) return 255u;
  return (uint32_t)s;
}

// FOLD: frame -> mean; DEVELOP: mean -> surface (+ PACK8: the surface as r | g << 8 | b << 16 | a << 24); both: one pass
enum : int { PASS_FOLD = 1, PASS_DEVELOP = 2 };
template <int PASSES, bool PACK8>
__global__ __launch_bounds__(256) void present_kernel(const PresentArgs A, const float4* __restrict__ frame, float4* __restrict__ mean_plane,
                                                      float4* __restrict__ surface, uint32_t* __restrict__ rgba8) {
  const bool first = A.samples_so_far == 0.0f;  // wave-uniform: the mean plane is write-only for the first sample
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += gridDim.x * blockDim.x) {
    float4 mean;
    if constexpr ((PASSES & PASS_FOLD) != 0) {
      const float4 x = frame[i];
      mean = fold_sample(first ? make_float4(0.f, 0.f, 0.f, 0.f) : mean_plane[i], x, A);
      mean_plane[i] = mean;
    } else {
      mean = mean_plane[i];
    }
    if constexpr ((PASSES & PASS_DEVELOP) != 0) {
      const float4 out = develop(mean, A);
      surface[i] = out;
      if constexpr (PACK8) rgba8[i] = to_u8(out.x) | (to_u8(out.y) << 8) | (to_u8(out.z) << 16) | (to_u8(out.w) << 24);
    }
  }
}

}  // namespace

struct nrf_render_buffer {
  int device = 0, W = 0, H = 0;
  uint32_t spp = 0;
  int color_space = NRF_CS_LINEAR, curve = NRF_TM_IDENTITY;
  void *frame = nullptr, *depth = nullptr, *accum = nullptr, *surface = nullptr;
  // the upscaler (nrf_rb_enable_upscale): the output resolution (0: disabled), the sharpening amount and the plane float4 [OH][OW]
  int OW = 0, OH = 0;
  float sharpening = 0.0f;
  void* upscaled = nullptr;
  // the temporal upscaler (nrf_rb_upscale_temporal): the history colour and weight planes, twice each, allocated by the first call;
  // `latest` is the pair the last call wrote, n_frames the calls since the history began (0: the next call is a reset)
  void *history[2] = {nullptr, nullptr}, *weight[2] = {nullptr, nullptr};
  int latest = 0;
  uint32_t n_frames = 0;
  float max_history = nrf::TEMPORAL_HISTORY_DEFAULT;
  // the 256 floats of nrf_rb_srgb8_table on the device, made by the first nrf_rb_overlay_image of a Byte image; freed by destroy
  void* srgb8 = nullptr;
  hipStream_t stream = nullptr;
};

// error plumbing shared with nrf_api.hip through nrf_last_error(): this TU keeps its own message
// and exposes it via a tiny hook
extern "C" void nrf_set_last_error_(const char* msg);
namespace {
int rb_fail(int code, const std::string& m) { nrf_set_last_error_(m.c_str()); return code; }
int rb_hip(hipError_t e, const char* what) { return rb_fail(NRF_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
#define RB_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return rb_hip(_e, #x); } while (0)
void rb_free_history(nrf_render_buffer* rb) {
  for (void** p : {&rb->history[0], &rb->history[1], &rb->weight[0], &rb->weight[1]}) { if (*p) (void)hipFree(*p); *p = nullptr; }
  rb->latest = 0;
  rb->n_frames = 0;
}
void rb_free(nrf_render_buffer* rb) {
  for (void** p : {&rb->frame, &rb->depth, &rb->accum, &rb->surface, &rb->upscaled}) { if (*p) (void)hipFree(*p); *p = nullptr; }
  rb_free_history(rb);
}
int rb_grid(int n) { int g = (n + 255) / 256; return g < 1 ? 1 : (g > 2048 ? 2048 : g); }
}  // namespace

extern "C" {

int nrf_rb_create(int device, nrf_render_buffer** out) {
  if (!out) return rb_fail(NRF_E_INVALID, "null argument");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
    return rb_fail(NRF_E_NODEVICE, "no HIP device available (this library has no CPU fallback)");
  nrf_render_buffer* rb = new nrf_render_buffer;
  rb->device = device;
  RB_TRY(hipSetDevice(device));
  RB_TRY(hipStreamCreateWithFlags(&rb->stream, hipStreamNonBlocking));
  *out = rb;
  return NRF_OK;
}

int nrf_rb_destroy(nrf_render_buffer* rb) {
  if (!rb) return NRF_OK;
  (void)hipSetDevice(rb->device);
  (void)hipDeviceSynchronize();
  rb_free(rb);
  if (rb->srgb8) (void)hipFree(rb->srgb8);
  if (rb->stream) (void)hipStreamDestroy(rb->stream);
  delete rb;
  return NRF_OK;
}

int nrf_rb_resize(nrf_render_buffer* rb, int width, int height) {
  if (!rb || width <= 0 || height <= 0) return rb_fail(NRF_E_INVALID, "bad resolution");
  // with the upscaler enabled its output resolution stays: the new size has to fit it, and is checked before anything is freed
  if (rb->OW && (!nrf::upscale_axis_valid(width, rb->OW) || !nrf::upscale_axis_valid(height, rb->OH)))
    return rb_fail(NRF_E_INVALID, "the resolution does not fit the enabled upscale resolution (in <= out <= 8 * in per axis)");
  RB_TRY(hipSetDevice(rb->device));
  RB_TRY(hipDeviceSynchronize());
  rb_free(rb);
  const size_t n = (size_t)width * height;
  RB_TRY(hipMalloc(&rb->frame, n * 16));
  RB_TRY(hipMalloc(&rb->depth, n * 4));
  RB_TRY(hipMalloc(&rb->accum, n * 16));
  RB_TRY(hipMalloc(&rb->surface, n * 16));
  RB_TRY(hipMemsetAsync(rb->frame, 0, n * 16, rb->stream));
  RB_TRY(hipMemsetAsync(rb->depth, 0, n * 4, rb->stream));
  RB_TRY(hipMemsetAsync(rb->accum, 0, n * 16, rb->stream));
  RB_TRY(hipMemsetAsync(rb->surface, 0, n * 16, rb->stream));
  if (rb->OW) {
    RB_TRY(hipMalloc(&rb->upscaled, (size_t)rb->OW * rb->OH * 16));
    RB_TRY(hipMemsetAsync(rb->upscaled, 0, (size_t)rb->OW * rb->OH * 16, rb->stream));
  }
  RB_TRY(hipStreamSynchronize(rb->stream));
  rb->W = width;
  rb->H = height;
  rb->spp = 0;
  return NRF_OK;
}

int nrf_rb_reset_accumulation(nrf_render_buffer* rb) {
  if (!rb) return rb_fail(NRF_E_INVALID, "null argument");
  rb->spp = 0;
  return NRF_OK;
}
int nrf_rb_spp(nrf_render_buffer* rb, uint32_t* spp) {
  if (!rb || !spp) return rb_fail(NRF_E_INVALID, "null argument");
  *spp = rb->spp;
  return NRF_OK;
}
int nrf_rb_set_color_space(nrf_render_buffer* rb, int cs) {
  if (!rb || cs < 0 || cs > 2) return rb_fail(NRF_E_INVALID, "bad color space");
  rb->color_space = cs;
  return NRF_OK;
}
int nrf_rb_set_tonemap_curve(nrf_render_buffer* rb, int curve) {
  if (!rb || curve < 0 || curve > 3) return rb_fail(NRF_E_INVALID, "bad tonemap curve");
  rb->curve = curve;
  return NRF_OK;
}
int nrf_rb_buffers(nrf_render_buffer* rb, void** frame, void** depth, void** accumulate, void** surface) {
  if (!rb) return rb_fail(NRF_E_INVALID, "null argument");
  if (!rb->frame) return rb_fail(NRF_E_STATE, "resize has not been called");
  if (frame) *frame = rb->frame;
  if (depth) *depth = rb->depth;
  if (accumulate) *accumulate = rb->accum;
  if (surface) *surface = rb->surface;
  return NRF_OK;
}

#define RB_READY()                                                             \
  if (!rb) return rb_fail(NRF_E_INVALID, "null argument");                     \
  if (!rb->frame) return rb_fail(NRF_E_STATE, "resize has not been called");   \
  RB_TRY(hipSetDevice(rb->device));                                            \
  hipStream_t st = stream ? (hipStream_t)stream : rb->stream;                  \
  const int n = rb->W * rb->H;

int nrf_rb_clear_frame(nrf_render_buffer* rb, void* stream) {
  RB_READY();
  RB_TRY(hipMemsetAsync(rb->frame, 0, (size_t)n * 16, st));
  RB_TRY(hipMemsetAsync(rb->depth, 0, (size_t)n * 4, st));
  if (!stream) RB_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

}  // extern "C"
namespace {
// the whole launch of one call: grid sized for the plane, every pixel-independent value fixed here
template <int PASSES>
int launch_present(nrf_render_buffer* rb, hipStream_t st, float exposure, const float bg[4], int display_space, void* rgba8) {
  PresentArgs A{};
  A.n = rb->W * rb->H;
  A.samples_so_far = (float)rb->spp;
  A.gain = powf(2.0f, exposure);
  A.render_space = rb->color_space;
  A.display_space = display_space;
  A.clamp_display = 0;
  A.film = film_curve(rb->curve);
  A.backdrop = bg ? make_float4(bg[0], bg[1], bg[2], bg[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (rb->color_space != NRF_CS_SRGB) {  // backgrounds are given display-referred: into the render space once, on the host
    A.backdrop.x = decode_srgb(A.backdrop.x);
    A.backdrop.y = decode_srgb(A.backdrop.y);
    A.backdrop.z = decode_srgb(A.backdrop.z);
  }
  const dim3 grid(rb_grid(A.n)), block(256);
  if (rgba8) hipLaunchKernelGGL((present_kernel<PASSES, true>), grid, block, 0, st, A, (const float4*)rb->frame, (float4*)rb->accum,
                                (float4*)rb->surface, (uint32_t*)rgba8);
  else hipLaunchKernelGGL((present_kernel<PASSES, false>), grid, block, 0, st, A, (const float4*)rb->frame, (float4*)rb->accum,
                          (float4*)rb->surface, (uint32_t*)nullptr);
  RB_TRY(hipGetLastError());
  return NRF_OK;
}
}  // namespace
extern "C" {

int nrf_rb_accumulate(nrf_render_buffer* rb, float exposure, void* stream) {
  (void)exposure;  // unused in the reference as well (render_buffer.cu:595)
  RB_READY();
  (void)n;
  const int rc = launch_present<PASS_FOLD>(rb, st, 0.0f, nullptr, NRF_CS_LINEAR, nullptr);
  if (rc != NRF_OK) return rc;
  ++rb->spp;
  if (!stream) RB_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_rb_tonemap(nrf_render_buffer* rb, float exposure, const float bg[4], int output_color_space, void* stream) {
  if (!bg || output_color_space < 0 || output_color_space > 2) return rb_fail(NRF_E_INVALID, "bad argument");
  RB_READY();
  (void)n;
  const int rc = launch_present<PASS_DEVELOP>(rb, st, exposure, bg, output_color_space, nullptr);
  if (rc != NRF_OK) return rc;
  if (!stream) RB_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_rb_present(nrf_render_buffer* rb, float exposure, const float bg[4], int output_color_space, void* rgba8, void* stream) {
  if (!bg || output_color_space < 0 || output_color_space > 2) return rb_fail(NRF_E_INVALID, "bad argument");
  RB_READY();
  (void)n;
  const int rc = launch_present<PASS_FOLD | PASS_DEVELOP>(rb, st, exposure, bg, output_color_space, rgba8);
  if (rc != NRF_OK) return rc;
  ++rb->spp;
  if (!stream) RB_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

// overlay_depth_kernel, R/src/render_buffer.cu:431-477 with colormap_turbo (:413-429, nrf_overlay_plan.h)
__global__ __launch_bounds__(256) void overlay_depth_kernel(int W, int H, float alpha, const float* __restrict__ depth,
                                                            float depth_scale, int img_w, int img_h, int fov_axis, float zoom,
                                                            float center_x, float center_y, float4* __restrict__ surface) {
  const int n = W * H;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int x = i % W, y = i / W;
    const float scale = (float)(fov_axis == 0 ? img_w : img_h) / (float)(fov_axis == 0 ? W : H);
    float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    fx -= (float)W * 0.5f; fx /= zoom; fx += center_x * (float)W;
    fy -= (float)H * 0.5f; fy /= zoom; fy += center_y * (float)H;
    const float u = (fx - (float)W * 0.5f) * scale + (float)img_w * 0.5f;
    const float v = (fy - (float)H * 0.5f) * scale + (float)img_h * 0.5f;
    const int srcx = (int)floorf(u), srcy = (int)floorf(v);
    float4 color = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!(srcx >= img_w || srcy >= img_h || srcx < 0 || srcy < 0)) {
      float c[3];
      colormap_turbo(depth[(size_t)srcx + (size_t)img_w * srcy] * depth_scale, c);
      color = make_float4(c[0], c[1], c[2], 1.0f);
    }
    const float4 prev = surface[i];
    const float ia = 1.f - alpha;
    surface[i] = make_float4(color.x * alpha + prev.x * ia, color.y * alpha + prev.y * ia, color.z * alpha + prev.z * ia,
                             color.w * alpha + prev.w * ia);
  }
}

int nrf_rb_overlay_depth(nrf_render_buffer* rb, float alpha, const void* depth, float depth_scale, int image_width,
                         int image_height, int fov_axis, float zoom, const float screen_center[2], void* stream) {
  if (!depth || !screen_center || image_width <= 0 || image_height <= 0 || (fov_axis != 0 && fov_axis != 1))
    return rb_fail(NRF_E_INVALID, "bad argument");
  RB_READY();
  hipLaunchKernelGGL(overlay_depth_kernel, dim3(rb_grid(n)), dim3(256), 0, st, rb->W, rb->H, alpha, (const float*)depth, depth_scale,
                     image_width, image_height, fov_axis, zoom, screen_center[0], screen_center[1], (float4*)rb->surface);
  RB_TRY(hipGetLastError());
  if (!stream) RB_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

// ---- the image and false-colour overlays and the error map: nrf_overlay_plan.h is the definition, nrf_kernels_overlay.hip the launches ----
namespace {
const float* srgb8_table() {  // made once, on the host, with libm
  static const struct Table {
    float t[256];
    Table() { nrf::overlay_srgb8_table(t); }
  } table;
  return table.t;
}
bool overlay_size_valid(int v) { return v > 0 && v <= nrf::OVERLAY_SIZE_MAX; }
}  // namespace

int nrf_rb_srgb8_table(float table[256]) {
  if (!table) return rb_fail(NRF_E_INVALID, "null argument");
  std::memcpy(table, srgb8_table(), 256 * sizeof(float));
  return NRF_OK;
}

int nrf_rb_overlay_image(nrf_render_buffer* rb, float alpha, const float exposure[3], const float background_color[4], int output_color_space,
                         const void* image, int image_data_type, int image_width, int image_height, int fov_axis, float zoom,
                         const float screen_center[2], void* stream) {
  if (!exposure || !background_color || !image || !screen_center) return rb_fail(NRF_E_INVALID, "null argument");
  if (output_color_space < 0 || output_color_space > 2) return rb_fail(NRF_E_INVALID, "bad color space");
  if (image_data_type != NRF_IMG_BYTE && image_data_type != NRF_IMG_HALF && image_data_type != NRF_IMG_FLOAT)
    return rb_fail(NRF_E_INVALID, "bad image data type");
  if (!overlay_size_valid(image_width) || !overlay_size_valid(image_height)) return rb_fail(NRF_E_INVALID, "bad image resolution (1 .. 16384 per axis)");
  if (fov_axis != 0 && fov_axis != 1) return rb_fail(NRF_E_INVALID, "bad fov axis");
  if (!std::isfinite(zoom) || zoom == 0.0f) return rb_fail(NRF_E_INVALID, "bad zoom (finite and not zero)");
  if (!std::isfinite(screen_center[0]) || !std::isfinite(screen_center[1])) return rb_fail(NRF_E_INVALID, "bad screen center (finite)");
  RB_READY();
  (void)n;
  if (!overlay_size_valid(rb->W) || !overlay_size_valid(rb->H)) return rb_fail(NRF_E_INVALID, "the surface is larger than 16384 on an axis");
  if (image_data_type == NRF_IMG_BYTE && !rb->srgb8) {  // the table, once per buffer
    void* t = nullptr;
    RB_TRY(hipMalloc(&t, 256 * sizeof(float)));
    const hipError_t e = hipMemcpy(t, srgb8_table(), 256 * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(t);
      return rb_hip(e, "uploading the sRGB table");
    }
    rb->srgb8 = t;
  }
  nrf::OverlayImage A{};
  A.map = {rb->W, rb->H, image_width, image_height, fov_axis, zoom, screen_center[0], screen_center[1]};
  A.alpha = alpha;
  for (int k = 0; k < 3; ++k) A.gain[k] = powf(2.0f, exposure[k]);
  const float given[4] = {background_color[0], background_color[1], background_color[2], background_color[3]};
  nrf::overlay_background(given, rb->color_space, A.bg);
  A.render_space = rb->color_space;
  A.display_space = output_color_space;
  A.film = film_curve(rb->curve);
  RB_TRY((hipError_t)nrf::launch_overlay_image(A, image, image_data_type, (const float*)rb->srgb8, rb->surface, st));
  if (!stream) RB_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_rb_overlay_false_color(nrf_render_buffer* rb, int training_width, int training_height, int fov_axis, const void* error_map,
                               int map_width, int map_height, const void* average, float brightness, int viridis, void* stream) {
  if (!error_map || !average) return rb_fail(NRF_E_INVALID, "null argument");
  if (!overlay_size_valid(training_width) || !overlay_size_valid(training_height))
    return rb_fail(NRF_E_INVALID, "bad training resolution (1 .. 16384 per axis)");
  if (fov_axis != 0 && fov_axis != 1) return rb_fail(NRF_E_INVALID, "bad fov axis");
  if (map_width < 1 || map_width > nrf::ERROR_MAP_MAX || map_height < 1 || map_height > nrf::ERROR_MAP_MAX)
    return rb_fail(NRF_E_INVALID, "bad error map resolution (1 .. 512 per axis)");
  RB_READY();
  (void)n;
  if (!overlay_size_valid(rb->W) || !overlay_size_valid(rb->H)) return rb_fail(NRF_E_INVALID, "the surface is larger than 16384 on an axis");
  const nrf::OverlayFalseColor A{rb->W, rb->H, training_width, training_height, map_width, map_height, fov_axis, brightness, viridis ? 1 : 0};
  RB_TRY((hipError_t)nrf::launch_overlay_false_color(A, (const float*)error_map, (const float*)average, rb->surface, st));
  if (!stream) RB_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_rb_error_map(nrf_render_buffer* rb, const void* truth_f32x4, int map_width, int map_height, void* error_map, void* average,
                     void* stream) {
  if (!truth_f32x4 || !error_map || !average) return rb_fail(NRF_E_INVALID, "null argument");
  RB_READY();
  (void)n;
  if (!overlay_size_valid(rb->W) || !overlay_size_valid(rb->H)) return rb_fail(NRF_E_INVALID, "the surface is larger than 16384 on an axis");
  if (!nrf::error_map_axis_valid(rb->W, map_width) || !nrf::error_map_axis_valid(rb->H, map_height))
    return rb_fail(NRF_E_INVALID, "bad error map resolution (1 <= cells <= min(pixels, 512) per axis)");
  RB_TRY((hipError_t)nrf::launch_error_map(rb->W, rb->H, map_width, map_height, rb->surface, truth_f32x4, (float*)error_map, (float*)average, st));
  if (!stream) RB_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_rb_host_to_accumulate_buffer(nrf_render_buffer* rb, const uint8_t* rgb, int count) {
  void* stream = nullptr;
  RB_READY();
  if (!rgb || count != n) return rb_fail(NRF_E_INVALID, "size does not match the resolution");
  std::vector<float> v((size_t)n * 4);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < 3; ++j) v[(size_t)i * 4 + j] = float(rgb[(size_t)i * 3 + j]) / 255.0;
    v[(size_t)i * 4 + 3] = 1.0;
  }
  RB_TRY(hipMemcpyAsync(rb->accum, v.data(), v.size() * 4, hipMemcpyHostToDevice, st));
  RB_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

// ---- the upscaler: nrf_upscale_plan.h is the definition, nrf_kernels_upscale.hip the launch ----
int nrf_rb_enable_upscale(nrf_render_buffer* rb, int out_width, int out_height) {
  if (!rb) return rb_fail(NRF_E_INVALID, "null argument");
  if (!rb->frame) return rb_fail(NRF_E_STATE, "resize has not been called");
  if (!nrf::upscale_axis_valid(rb->W, out_width) || !nrf::upscale_axis_valid(rb->H, out_height))
    return rb_fail(NRF_E_INVALID, "bad upscale resolution (in <= out <= 8 * in and out <= 16384 per axis)");
  RB_TRY(hipSetDevice(rb->device));
  RB_TRY(hipDeviceSynchronize());
  void* plane = nullptr;
  const size_t bytes = (size_t)out_width * out_height * 16;
  RB_TRY(hipMalloc(&plane, bytes));
  hipError_t e = hipMemsetAsync(plane, 0, bytes, rb->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(rb->stream);
  if (e != hipSuccess) {
    (void)hipFree(plane);
    return rb_hip(e, "clearing the upscaled plane");
  }
  if (rb->upscaled) (void)hipFree(rb->upscaled);
  rb_free_history(rb);  // (the device is idle: synchronised above)
  rb->upscaled = plane;
  rb->OW = out_width;
  rb->OH = out_height;
  return NRF_OK;
}

int nrf_rb_disable_upscale(nrf_render_buffer* rb) {
  if (!rb) return rb_fail(NRF_E_INVALID, "null argument");
  if (rb->upscaled) {
    RB_TRY(hipSetDevice(rb->device));
    RB_TRY(hipDeviceSynchronize());
    (void)hipFree(rb->upscaled);
    rb_free_history(rb);
  }
  rb->upscaled = nullptr;
  rb->OW = rb->OH = 0;
  return NRF_OK;
}

int nrf_rb_set_upscale_sharpening(nrf_render_buffer* rb, float amount) {
  if (!rb) return rb_fail(NRF_E_INVALID, "null argument");
  if (!nrf::upscale_amount_valid(amount)) return rb_fail(NRF_E_INVALID, "bad sharpening amount (0 <= amount <= 2)");
  rb->sharpening = amount;
  return NRF_OK;
}

int nrf_rb_resolutions(nrf_render_buffer* rb, int in_wh[2], int out_wh[2]) {
  if (!rb) return rb_fail(NRF_E_INVALID, "null argument");
  if (in_wh) in_wh[0] = rb->W, in_wh[1] = rb->H;
  if (out_wh) out_wh[0] = rb->OW ? rb->OW : rb->W, out_wh[1] = rb->OW ? rb->OH : rb->H;
  return NRF_OK;
}

int nrf_rb_upscale(nrf_render_buffer* rb, void* rgba8, void* stream) {
  RB_READY();
  (void)n;
  if (!rb->upscaled) return rb_fail(NRF_E_STATE, "upscaling is not enabled");
  nrf::UpscalePlan P;
  if (!nrf::upscale_plan(rb->W, rb->H, rb->OW, rb->OH, rb->sharpening, P)) return rb_fail(NRF_E_STATE, "the resolutions do not fit");
  RB_TRY((hipError_t)nrf::launch_upscale(P, rb->surface, rb->upscaled, rgba8, st));
  if (!stream) RB_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_rb_upscaled(nrf_render_buffer* rb, void** plane) {
  if (!rb || !plane) return rb_fail(NRF_E_INVALID, "null argument");
  if (!rb->upscaled) return rb_fail(NRF_E_STATE, "upscaling is not enabled");
  *plane = rb->upscaled;
  return NRF_OK;
}

int nrf_rb_read_upscaled(nrf_render_buffer* rb, float* rgba) {
  if (!rb || !rgba) return rb_fail(NRF_E_INVALID, "null argument");
  if (!rb->upscaled) return rb_fail(NRF_E_STATE, "upscaling is not enabled");
  RB_TRY(hipSetDevice(rb->device));
  RB_TRY(hipDeviceSynchronize());
  RB_TRY(hipMemcpy(rgba, rb->upscaled, (size_t)rb->OW * rb->OH * 16, hipMemcpyDeviceToHost));
  return NRF_OK;
}

// ---- the temporal upscaler: nrf_temporal_plan.h is the definition, nrf_kernels_temporal.hip the launch ----
int nrf_rb_upscale_jitter(uint32_t index, float jitter[2]) {
  if (!jitter) return rb_fail(NRF_E_INVALID, "null argument");
  float j[2];
  nrf::temporal_jitter(index, j);
  jitter[0] = j[0], jitter[1] = j[1];
  return NRF_OK;
}

int nrf_rb_set_upscale_history(nrf_render_buffer* rb, float max_history) {
  if (!rb) return rb_fail(NRF_E_INVALID, "null argument");
  if (!nrf::temporal_history_valid(max_history)) return rb_fail(NRF_E_INVALID, "bad history length (1 <= max_history <= 256)");
  rb->max_history = max_history;
  return NRF_OK;
}

int nrf_rb_upscale_temporal(nrf_render_buffer* rb, const nrf_upscale_temporal* t, void* rgba8, void* stream) {
  RB_READY();
  (void)n;
  if (!rb->upscaled) return rb_fail(NRF_E_STATE, "upscaling is not enabled");
  if (!t) return rb_fail(NRF_E_INVALID, "null argument");
  if ((t->flags & ~(uint32_t)(NRF_UPSCALE_T_RESET | NRF_UPSCALE_T_RECTIFY)) || t->reserved != 0)
    return rb_fail(NRF_E_INVALID, "unknown flag or reserved field set");
  if (!nrf::temporal_jitter_valid(t->jitter[0]) || !nrf::temporal_jitter_valid(t->jitter[1]))
    return rb_fail(NRF_E_INVALID, "bad jitter (finite, within [-0.5, 0.5] per axis)");
  const size_t texels = (size_t)rb->OW * rb->OH;
  if (!rb->history[0]) {  // the first call: the four planes, zero-filled; all or none
    void* planes[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4 && e == hipSuccess; ++k) {
      const size_t bytes = texels * (k < 2 ? 16 : 4);
      e = hipMalloc(&planes[k], bytes);
      if (e == hipSuccess) e = hipMemsetAsync(planes[k], 0, bytes, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      for (void* p : planes) if (p) (void)hipFree(p);
      return rb_hip(e, "allocating the history planes");
    }
    rb->history[0] = planes[0], rb->history[1] = planes[1], rb->weight[0] = planes[2], rb->weight[1] = planes[3];
    rb->latest = 0;
    rb->n_frames = 0;
  }
  uint32_t flags = t->flags;
  if (rb->n_frames == 0) flags |= NRF_UPSCALE_T_RESET;  // nothing to blend with yet
  nrf::TemporalPlan T;
  if (!nrf::temporal_plan(rb->W, rb->H, rb->OW, rb->OH, rb->sharpening, t->jitter[0], t->jitter[1], rb->max_history, flags, T))
    return rb_fail(NRF_E_STATE, "the resolutions do not fit");
  const int prev = rb->latest, next = 1 - rb->latest;
  RB_TRY((hipError_t)nrf::launch_temporal(T, rb->surface, t->motion, rb->history[prev], rb->weight[prev], rb->history[next], rb->weight[next],
                                          rb->upscaled, rgba8, st));
  rb->latest = next;
  if (rb->n_frames != UINT32_MAX) ++rb->n_frames;
  if (!stream) RB_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_rb_upscale_history(nrf_render_buffer* rb, void** history, void** weight, uint32_t* n_frames) {
  if (!rb) return rb_fail(NRF_E_INVALID, "null argument");
  if (!rb->upscaled) return rb_fail(NRF_E_STATE, "upscaling is not enabled");
  if (history) *history = rb->history[rb->latest];
  if (weight) *weight = rb->weight[rb->latest];
  if (n_frames) *n_frames = rb->n_frames;
  return NRF_OK;
}

int nrf_rb_read_upscale_history(nrf_render_buffer* rb, float* rgba, float* weight) {
  if (!rb) return rb_fail(NRF_E_INVALID, "null argument");
  if (!rb->upscaled) return rb_fail(NRF_E_STATE, "upscaling is not enabled");
  if (!rb->history[0] || rb->n_frames == 0) return rb_fail(NRF_E_STATE, "no history yet (call nrf_rb_upscale_temporal)");
  RB_TRY(hipSetDevice(rb->device));
  RB_TRY(hipDeviceSynchronize());
  const size_t texels = (size_t)rb->OW * rb->OH;
  if (rgba) RB_TRY(hipMemcpy(rgba, rb->history[rb->latest], texels * 16, hipMemcpyDeviceToHost));
  if (weight) RB_TRY(hipMemcpy(weight, rb->weight[rb->latest], texels * 4, hipMemcpyDeviceToHost));
  return NRF_OK;
}

int nrf_rb_read(nrf_render_buffer* rb, float* accumulate_rgba, float* surface_rgba) {
  void* stream = nullptr;
  RB_READY();
  RB_TRY(hipDeviceSynchronize());
  if (accumulate_rgba) RB_TRY(hipMemcpy(accumulate_rgba, rb->accum, (size_t)n * 16, hipMemcpyDeviceToHost));
  if (surface_rgba) RB_TRY(hipMemcpy(surface_rgba, rb->surface, (size_t)n * 16, hipMemcpyDeviceToHost));
  (void)st;
  return NRF_OK;
}

}  // extern "C"
