// testbed.cpp -- mirror of the reference's `testbed` main (src/main.cu:131-206) without the
// GLFW/Vulkan/DLSS presentation part: load a snapshot, render ONE frame with the hard-coded camera
// and pose, print "Process time", write image.png / deep.png.
//   usage: testbed [snapshot.msgpack] [width height] [out_prefix] [transforms.json]
// With a transforms.json (NeRF-synthetic / instant-ngp camera path) every frame of the path is rendered as well, in
// batches of 32 views per launch, and written to <out_prefix>path_NNNN.rgb.
//   options (anywhere): --save_mesh FILE.obj | FILE.ply [--mesh_res N] [--mesh_iso X] -- the iso-surface of the density on an N^3 lattice
//   over the model's aabb (NerfRender::extract_mesh; defaults 128 and 2.5), written as a Wavefront OBJ with vertex normals or, for a
//   name that ends in .ply, as a binary PLY with vertex normals and colours (NerfRender::mesh_attributes, save_ply)
//   [--mesh_min_triangles N] [--mesh_largest] -- between extraction and attributes the mesh is filtered on the device by connected
//   component (NerfRender::mesh_components, filter_mesh): components with fewer than N triangles are dropped, --mesh_largest keeps only
//   the component with the most triangles
//   [--mesh_refine N] -- after the filter and before the attributes every vertex is moved along its lattice edge onto the iso value of
//   the density network, N (0 .. 16) bisections and a secant step on the device (NerfRender::refine_mesh)
//   [--mesh_simplify K] -- after the filter and the refinement and before the attributes the mesh is simplified on the device by vertex
//   clustering on blocks of K^3 lattice points, K = 1 .. 256 (NerfRender::simplify_mesh)
//   [--mesh_texture R [--mesh_texture_width W]] -- with FILE.obj: after the filter, the refinement and the simplification, and in place
//   of the attributes, the colours of the network are baked on the device into a per-triangle texture atlas of R (2 .. 256) texels along
//   a triangle's legs and W (default 4096) texels width (NerfRender::bake_mesh_texture), and the mesh is written as FILE.obj with
//   FILE.mtl and FILE.png next to it (save_obj_textured)
//   [--upscale S [--upscale_sharpening A]] -- where the reference hands the frame to DLSS at twice the resolution and writes dlss.png
//   (main.cu:171-206): after tonemapped.png the same render buffer upscales its surface on the device to round(W S) x round(H S),
//   1 <= S <= 8 (the reference's fixed value is 2), sharpened by A (0 .. 2, default 0, the value the reference sets), and upscaled.png is
//   written (RenderBuffer::enable_upscale, upscale: a deterministic spatial filter, not DLSS)
//   [--upscale_temporal N] -- with --upscale: N frames (1 .. 256) of the same view go through the temporal upscaler instead, the way the
//   reference drives DLSS: frame k is rendered with the sub-pixel jitter of RenderBuffer::upscale_jitter(k) (frame 0 without, as a
//   reset), developed alone into the surface, and accumulated at the output resolution (RenderBuffer::upscale_temporal); upscaled.png
//   is the presented plane after the last frame
//   [--overlay_image FILE.ppm [--overlay_alpha A]] -- an 8-bit binary PPM (P6, maxval 255) of the frame's size is uploaded as Byte texels
//   with alpha 255 and blended with weight A (default 0.5) over the developed frame on the device before tonemapped.png is written
//   (RenderBuffer::overlay_image: the photograph next to the render)
//   [--compare FILE.ppm] -- the same kind of file is uploaded as a float4 truth plane (v / 255, alpha 1); the per-cell mean squared error
//   of the developed frame against it is reduced on the device at min(128, W) x min(128, H) cells (RenderBuffer::error_map), the average
//   and -10 log10(average) are printed, and the frame under the viridis false colours of that map is written as error.png
//   (RenderBuffer::overlay_false_color)
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "nerf_render.h"
#include "png_lite.h"
#include "render_buffer.h"

constexpr size_t PATH_BATCH_VIEWS = 32;  // frames of a camera path rendered (and held) per launch

using namespace ngp;

// A stream and a pair of events of the HIP runtime that libnerfhip.so has loaded, looked up by name: this directory compiles
// without HIP headers.  elapsed_ms() is the device time of what was enqueued on stream() between start() and stop().
class DeviceTimer {
 public:
  DeviceTimer() {
    create_stream = sym<int (*)(void**)>("hipStreamCreate");
    destroy_stream = sym<int (*)(void*)>("hipStreamDestroy");
    create_event = sym<int (*)(void**)>("hipEventCreate");
    destroy_event = sym<int (*)(void*)>("hipEventDestroy");
    record = sym<int (*)(void*, void*)>("hipEventRecord");
    synchronize = sym<int (*)(void*)>("hipEventSynchronize");
    elapsed = sym<int (*)(float*, void*, void*)>("hipEventElapsedTime");
    ok(create_stream(&m_stream));
    ok(create_event(&m_begin));
    ok(create_event(&m_end));
  }
  ~DeviceTimer() {
    if (m_begin) destroy_event(m_begin);
    if (m_end) destroy_event(m_end);
    if (m_stream) destroy_stream(m_stream);
  }
  DeviceTimer(const DeviceTimer&) = delete;
  DeviceTimer& operator=(const DeviceTimer&) = delete;
  void* stream() const { return m_stream; }
  void start() { ok(record(m_begin, m_stream)); }
  float stop() {
    float ms = 0.f;
    ok(record(m_end, m_stream));
    ok(synchronize(m_end));
    ok(elapsed(&ms, m_begin, m_end));
    return ms;
  }

 private:
  template <class F>
  static F sym(const char* name) {
    void* p = dlsym(RTLD_DEFAULT, name);
    if (!p) throw std::runtime_error{std::string("the HIP runtime has no ") + name};
    return reinterpret_cast<F>(p);
  }
  static void ok(int rc) {
    if (rc != 0) throw std::runtime_error{"HIP runtime error " + std::to_string(rc) + " while timing"};
  }
  int (*create_stream)(void**) = nullptr;
  int (*destroy_stream)(void*) = nullptr;
  int (*create_event)(void**) = nullptr;
  int (*destroy_event)(void*) = nullptr;
  int (*record)(void*, void*) = nullptr;
  int (*synchronize)(void*) = nullptr;
  int (*elapsed)(float*, void*, void*) = nullptr;
  void *m_stream = nullptr, *m_begin = nullptr, *m_end = nullptr;
};

// Device memory of the HIP runtime that libnerfhip.so has loaded, looked up by name like the timer's calls
class DeviceBuffer {
 public:
  explicit DeviceBuffer(size_t bytes) : m_bytes(bytes) {
    malloc_ = sym<int (*)(void**, size_t)>("hipMalloc");
    free_ = sym<int (*)(void*)>("hipFree");
    memcpy_ = sym<int (*)(void*, const void*, size_t, int)>("hipMemcpy");
    ok(malloc_(&m_ptr, bytes));
  }
  ~DeviceBuffer() {
    if (m_ptr) free_(m_ptr);
  }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  void* ptr() const { return m_ptr; }
  void upload(const void* host) { ok(memcpy_(m_ptr, host, m_bytes, 1)); }    // hipMemcpyHostToDevice
  void download(void* host) const { ok(memcpy_(host, m_ptr, m_bytes, 2)); }  // hipMemcpyDeviceToHost

 private:
  template <class F>
  static F sym(const char* name) {
    void* p = dlsym(RTLD_DEFAULT, name);
    if (!p) throw std::runtime_error{std::string("the HIP runtime has no ") + name};
    return reinterpret_cast<F>(p);
  }
  static void ok(int rc) {
    if (rc != 0) throw std::runtime_error{"HIP runtime error " + std::to_string(rc) + " on a device buffer"};
  }
  int (*malloc_)(void**, size_t) = nullptr;
  int (*free_)(void*) = nullptr;
  int (*memcpy_)(void*, const void*, size_t, int) = nullptr;
  void* m_ptr = nullptr;
  size_t m_bytes = 0;
};

// An 8-bit binary PPM (P6) of exactly W x H pixels: the rgb bytes.  Refused: another magic, a size that is not the frame's, a maxval
// other than 255, a file that ends before the last pixel
static std::vector<unsigned char> read_ppm(const std::string& path, int W, int H) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error{"cannot open " + path};
  char magic[3] = {0, 0, 0};
  int w = 0, h = 0, maxval = 0;
  const bool header = std::fscanf(f, "%2s %d %d %d", magic, &w, &h, &maxval) == 4 && std::string(magic) == "P6" && std::fgetc(f) != EOF;
  std::vector<unsigned char> rgb;
  if (header && w == W && h == H && maxval == 255) {
    rgb.resize((size_t)W * H * 3);
    if (std::fread(rgb.data(), 1, rgb.size(), f) != rgb.size()) rgb.clear();
  }
  std::fclose(f);
  if (!header) throw std::runtime_error{path + " is not a binary PPM (P6)"};
  if (w != W || h != H) throw std::runtime_error{path + " is " + std::to_string(w) + " x " + std::to_string(h) + ", the frame is " + std::to_string(W) + " x " + std::to_string(H)};
  if (maxval != 255) throw std::runtime_error{path + " has maxval " + std::to_string(maxval) + ", not 255"};
  if (rgb.empty()) throw std::runtime_error{path + " ends before its last pixel"};
  return rgb;
}

static void write_surface_png(const std::string& path, int W, int H, const std::vector<float>& rgba) {
  std::vector<unsigned char> out((size_t)W * H * 3);
  for (size_t i = 0; i < (size_t)W * H; ++i)
    for (int j = 0; j < 3; ++j) {
      const float v = rgba[i * 4 + j] * 255;
      out[i * 3 + j] = (unsigned char)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
    }
  pnglite::write(path.c_str(), W, H, 3, out.data());
}

int main(int argc, char** argv) {
  std::cout << "Hello, Metavese!" << std::endl;
  // the options, taken out of argv: what remains are the positional arguments above
  std::string mesh_path;
  int mesh_res = 128;
  float mesh_iso = 2.5f;  // (instant-ngp's default mesh threshold)
  unsigned long long mesh_min_triangles = 0;
  bool mesh_largest = false;
  int mesh_refine = -1;  // (off)
  int mesh_simplify = 0;  // (off)
  int mesh_texture = 0, mesh_texture_width = 4096;  // (off)
  float upscale = 0.0f, upscale_sharpening = 0.0f;  // (off)
  int upscale_temporal = 0;                          // (off)
  std::string overlay_path, compare_path;            // (off)
  float overlay_alpha = 0.5f;
  {
    int kept = 1;
    for (int i = 1; i < argc; ++i) {
      const std::string a = argv[i];
      if ((a == "--save_mesh" || a == "--mesh_res" || a == "--mesh_iso" || a == "--mesh_min_triangles" || a == "--mesh_refine" ||
           a == "--mesh_simplify" || a == "--mesh_texture" || a == "--mesh_texture_width" || a == "--upscale" || a == "--upscale_sharpening" ||
           a == "--upscale_temporal" || a == "--overlay_image" || a == "--overlay_alpha" || a == "--compare") &&
          i + 1 < argc) {
        if (a == "--save_mesh") mesh_path = argv[++i];
        else if (a == "--overlay_image") overlay_path = argv[++i];
        else if (a == "--overlay_alpha") overlay_alpha = (float)std::atof(argv[++i]);
        else if (a == "--compare") compare_path = argv[++i];
        else if (a == "--upscale") upscale = (float)std::atof(argv[++i]);
        else if (a == "--upscale_sharpening") upscale_sharpening = (float)std::atof(argv[++i]);
        else if (a == "--upscale_temporal") upscale_temporal = std::atoi(argv[++i]);
        else if (a == "--mesh_res") mesh_res = std::atoi(argv[++i]);
        else if (a == "--mesh_refine") mesh_refine = std::atoi(argv[++i]);
        else if (a == "--mesh_simplify") mesh_simplify = std::atoi(argv[++i]);
        else if (a == "--mesh_texture") mesh_texture = std::atoi(argv[++i]);
        else if (a == "--mesh_texture_width") mesh_texture_width = std::atoi(argv[++i]);
        else if (a == "--mesh_min_triangles") mesh_min_triangles = std::strtoull(argv[++i], nullptr, 10);
        else mesh_iso = (float)std::atof(argv[++i]);
      } else if (a == "--mesh_largest") {
        mesh_largest = true;
      } else {
        argv[kept++] = argv[i];
      }
    }
    argc = kept;
  }
  try {
    const int W = argc > 3 ? std::atoi(argv[2]) : 4000 / 8, H = argc > 3 ? std::atoi(argv[3]) : 4000 / 8;
    const std::string prefix = argc > 4 ? argv[4] : "./";
    // the pictures of --overlay_image and --compare, read before anything is loaded or rendered: a file that does not fit ends the run here
    std::vector<unsigned char> overlay_rgb, compare_rgb;
    if (!overlay_path.empty()) overlay_rgb = read_ppm(overlay_path, W, H);
    if (!compare_path.empty()) compare_rgb = read_ppm(compare_path, W, H);
    NerfRender* render = new NerfRender();
    const std::string config_path = argc > 1 ? argv[1] : "freality.msgpack";
    render->reload_network_from_file(config_path);  // Init Model
    const float s = (float)W / 500.0f;
    Camera cam = {3550.115f / 8 * s, 3554.515f / 8 * s, 3010.45f / 8 * s, 1996.027f / 8 * s};
    Matrix4f pos;
    const float p[16] = {-0.5575427361517304f, -0.11682263918046752f, 0.8218871992959822f, 3.9673954052389253f,
                         0.8300327085486383f,  -0.094966079921629f,   0.5495699649760266f, 2.667431152445114f,
                         0.013849191732089516f, 0.9886020001326434f,  0.14991425965987268f, 0.45955395816033995f,
                         0.0f, 0.0f, 0.0f, 1.0f};
    for (int i = 0; i < 16; ++i) pos.m[i] = p[i];
    render->set_resolution(Vector2i(W, H));
    const auto t0 = std::chrono::steady_clock::now();
    Image img = render->render_frame(cam, pos);
    const auto t1 = std::chrono::steady_clock::now();
    std::printf("Process time : %f s / frame\n", std::chrono::duration<double>(t1 - t0).count());
    const nrf_stats st = render->last_stats();
    std::printf("samples %llu  device time %.3f ms\n", (unsigned long long)st.n_samples, st.render_ms);
    pnglite::write((prefix + "deep.png").c_str(), img.W, img.H, 1, img.depth);
    pnglite::write((prefix + "image.png").c_str(), img.W, img.H, 3, img.rgb);
    // presentation chain of main.cu:87-129,171-206 without DLSS: u8 image -> accumulate buffer -> tonemap (sRGB)
    {
      RenderBuffer rb;
      rb.resize(Vector2i(img.W, img.H));
      rb.reset_accumulation();
      rb.host_to_accumulate_buffer(img.rgb, img.W * img.H);
      const float bg[4] = {0.f, 0.f, 0.f, 1.f};
      rb.tonemap(0.0f, bg, EColorSpace::SRGB);
      if (!overlay_path.empty()) {
        // the photograph over the developed frame, on the device: Byte texels (sRGB, alpha 255) through the same tonemap as the frame
        const std::vector<unsigned char>& rgb = overlay_rgb;
        std::vector<uint32_t> texels((size_t)img.W * img.H);
        for (size_t i = 0; i < texels.size(); ++i)
          texels[i] = (uint32_t)rgb[i * 3] | (uint32_t)rgb[i * 3 + 1] << 8 | (uint32_t)rgb[i * 3 + 2] << 16 | 0xFF000000u;
        DeviceBuffer image(texels.size() * sizeof(uint32_t));
        image.upload(texels.data());
        const float exposure[3] = {0.f, 0.f, 0.f}, center[2] = {0.5f, 0.5f};
        rb.overlay_image(overlay_alpha, exposure, bg, EColorSpace::SRGB, image.ptr(), EImageDataType::Byte, Vector2i(img.W, img.H), 0, 1.0f, center);
        std::printf("overlay: %s over the frame, alpha %g\n", overlay_path.c_str(), overlay_alpha);
      }
      write_surface_png(prefix + "tonemapped.png", img.W, img.H, rb.surface_host());
      if (upscale != 0.0f) {
        // main.cu:171-206 hands the frame to DLSS at out_resolution = 2 x in_resolution and writes dlss.png; here the surface just
        // developed goes through the upscaler on the device, on a stream of this program's so that a pair of events times the launch
        const Vector2i out_res((int)std::lround((double)img.W * upscale), (int)std::lround((double)img.H * upscale));
        rb.enable_upscale(out_res);
        rb.set_upscale_sharpening(upscale_sharpening);
        DeviceTimer timer;
        const Vector2i in = rb.in_resolution(), got = rb.out_resolution();
        if (upscale_temporal > 0) {
          // the same view N times, each frame through a camera moved by that frame's sub-pixel jitter and developed alone into the
          // surface (the chain above), then folded into the history at the output resolution; the last launch is the one timed
          if (upscale_temporal > 256) throw std::runtime_error{"--upscale_temporal takes 1 .. 256 frames"};
          float ms = 0.f;
          for (int k = 0; k < upscale_temporal; ++k) {
            float jitter[2] = {0.f, 0.f};
            if (k > 0) RenderBuffer::upscale_jitter((uint32_t)k, jitter);
            const Camera jittered = {cam.fl_x, cam.fl_y, cam.cx - jitter[0], cam.cy - jitter[1]};
            const Image frame = k == 0 ? img : render->render_frame(jittered, pos);
            rb.reset_accumulation();
            rb.host_to_accumulate_buffer(frame.rgb, frame.W * frame.H);
            rb.tonemap(0.0f, bg, EColorSpace::SRGB);
            timer.start();
            rb.upscale_temporal(jitter, nullptr, k == 0, false, nullptr, timer.stream());
            ms = timer.stop();
          }
          std::printf("upscale: %d x %d -> %d x %d, sharpening %g, temporal over %u frames, device time %.3f ms\n", in[0], in[1], got[0], got[1],
                      upscale_sharpening, rb.upscale_frames(), ms);
        } else {
          timer.start();
          rb.upscale(nullptr, timer.stream());
          const float ms = timer.stop();
          std::printf("upscale: %d x %d -> %d x %d, sharpening %g, device time %.3f ms\n", in[0], in[1], got[0], got[1], upscale_sharpening, ms);
        }
        const std::vector<float> up = rb.upscaled_host();
        std::vector<unsigned char> up8((size_t)got[0] * got[1] * 3);
        for (size_t i = 0; i < (size_t)got[0] * got[1]; ++i)
          for (int j = 0; j < 3; ++j) {
            const float v = up[i * 4 + j] * 255;
            up8[i * 3 + j] = (unsigned char)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
          }
        pnglite::write((prefix + "upscaled.png").c_str(), got[0], got[1], 3, up8.data());
      }
      if (!compare_path.empty()) {
        // where the developed frame is wrong: the file as the truth plane, the error map and its average on the device, then the frame
        // under the map's false colours (last: it changes the surface)
        const std::vector<unsigned char>& rgb = compare_rgb;
        std::vector<float> truth((size_t)img.W * img.H * 4);
        for (size_t i = 0; i < (size_t)img.W * img.H; ++i) {
          for (int j = 0; j < 3; ++j) truth[i * 4 + j] = (float)rgb[i * 3 + j] / 255.0f;
          truth[i * 4 + 3] = 1.0f;
        }
        const Vector2i cells(std::min(128, img.W), std::min(128, img.H));
        DeviceBuffer plane(truth.size() * sizeof(float)), map((size_t)cells[0] * cells[1] * sizeof(float)), average(sizeof(float));
        plane.upload(truth.data());
        rb.error_map(plane.ptr(), cells, (float*)map.ptr(), (float*)average.ptr());
        float mse = 0.f;
        average.download(&mse);
        std::printf("compare: %d x %d cells, average %.9g, %.4f dB\n", cells[0], cells[1], mse, -10.0 * std::log10((double)mse));
        rb.overlay_false_color(Vector2i(img.W, img.H), false, 0, nullptr, (const float*)map.ptr(), cells, (const float*)average.ptr(), 1.0f, true);
        write_surface_png(prefix + "error.png", img.W, img.H, rb.surface_host());
      }
    }
    FILE* f = std::fopen((prefix + "image.rgb").c_str(), "wb");  // raw copy for the parity test
    if (f) { std::fwrite(img.rgb, 1, (size_t)img.W * img.H * 3, f); std::fclose(f); }
    if (argc > 5) {
      std::vector<Camera> cams;
      std::vector<Matrix4f> poses;
      load_camera_path(argv[5], W, H, cams, poses);
      const auto p0 = std::chrono::steady_clock::now();
      size_t done = 0;
      for (size_t first = 0; first < cams.size(); first += PATH_BATCH_VIEWS) {
        const size_t n = std::min(cams.size() - first, PATH_BATCH_VIEWS);
        const std::vector<Image> imgs = render->render_frames(std::vector<Camera>(cams.begin() + first, cams.begin() + first + n),
                                                              std::vector<Matrix4f>(poses.begin() + first, poses.begin() + first + n));
        for (size_t i = 0; i < n; ++i, ++done) {
          char name[64];
          std::snprintf(name, sizeof(name), "path_%04zu.rgb", first + i);
          FILE* pf = std::fopen((prefix + name).c_str(), "wb");
          if (pf) { std::fwrite(imgs[i].rgb, 1, (size_t)W * H * 3, pf); std::fclose(pf); }
        }
      }
      const auto p1 = std::chrono::steady_clock::now();
      std::printf("camera path: %zu frames, %f s / frame\n", done, std::chrono::duration<double>(p1 - p0).count() / (double)(done ? done : 1));
    }
    if (!mesh_path.empty()) {
      // a cube of mesh_res^3 points over the model's aabb [-bound, bound]^3 (the density is 0 outside it, so the surface is closed
      // wherever the object does not touch the box)
      const float b = render->model_desc().bound;
      const uint32_t n = (uint32_t)std::max(2, mesh_res);
      const float origin[3] = {-b, -b, -b}, step = 2.0f * b / (float)(n - 1), cell[3] = {step, step, step};
      const uint32_t dims[3] = {n, n, n};
      const auto m0 = std::chrono::steady_clock::now();
      NerfRender::Mesh mesh = render->extract_mesh(origin, cell, dims, mesh_iso);
      const auto m1 = std::chrono::steady_clock::now();
      std::printf("mesh: %u^3 lattice at iso %g: %zu vertices, %zu triangles, %f s\n", n, mesh_iso, mesh.vertices.size() / 3,
                  mesh.triangles.size() / 3, std::chrono::duration<double>(m1 - m0).count());
      if (mesh_min_triangles || mesh_largest) {
        // floaters off, on the device, before the attributes: fewer vertices for the seven network passes each of them costs
        const size_t nv0 = mesh.vertices.size() / 3, nt0 = mesh.triangles.size() / 3;
        const auto f0 = std::chrono::steady_clock::now();
        const NerfRender::MeshComponents parts = render->mesh_components();
        mesh = render->filter_mesh(mesh_min_triangles, mesh_largest);
        const auto f1 = std::chrono::steady_clock::now();
        // the keep rule on the table's rows (ascending label: the first row with the most triangles wins a tie)
        const size_t rows = parts.table.size() / 3;
        size_t largest = 0, kept = 0;
        for (size_t r = 1; r < rows; ++r)
          if (parts.table[3 * r + 2] > parts.table[3 * largest + 2]) largest = r;
        for (size_t r = 0; r < rows; ++r) kept += parts.table[3 * r + 2] >= mesh_min_triangles && (!mesh_largest || r == largest);
        std::printf("mesh filter: %zu components, %zu kept, vertices %zu -> %zu, triangles %zu -> %zu, %f s\n", rows, kept, nv0,
                    mesh.vertices.size() / 3, nt0, mesh.triangles.size() / 3, std::chrono::duration<double>(f1 - f0).count());
      }
      if (mesh_refine >= 0) {
        // onto the iso-surface, on the device, after the filter (fewer vertices) and before the attributes (they are taken at the positions)
        const auto r0 = std::chrono::steady_clock::now();
        NerfRender::MeshRefinement refined = render->refine_mesh((uint32_t)mesh_refine);
        const auto r1 = std::chrono::steady_clock::now();
        std::printf("mesh refine: %d steps, %zu vertices, %llu unbracketed, %f s\n", mesh_refine, refined.vertices.size() / 3,
                    (unsigned long long)refined.unbracketed, std::chrono::duration<double>(r1 - r0).count());
        mesh.vertices = std::move(refined.vertices);
        mesh.vertices_dev = refined.vertices_dev;
      }
      if (mesh_simplify != 0) {
        // down to a triangle budget, on the device, after the refinement (the representatives are vertices of the mesh: they stay on the
        // iso-surface) and before the attributes (fewer vertices for the seven network passes each of them costs)
        const size_t nv0 = mesh.vertices.size() / 3, nt0 = mesh.triangles.size() / 3;
        const auto s0 = std::chrono::steady_clock::now();
        NerfRender::SimplifiedMesh simplified = render->simplify_mesh((uint32_t)mesh_simplify);
        const auto s1 = std::chrono::steady_clock::now();
        std::printf("mesh simplify: factor %d, vertices %zu -> %zu, triangles %zu -> %zu, %f s\n", mesh_simplify, nv0, simplified.vertices.size() / 3,
                    nt0, simplified.triangles.size() / 3, std::chrono::duration<double>(s1 - s0).count());
        mesh.vertices = std::move(simplified.vertices);
        mesh.triangles = std::move(simplified.triangles);
        mesh.vertices_dev = simplified.vertices_dev;
      }
      const bool ply = mesh_path.size() >= 4 && mesh_path.compare(mesh_path.size() - 4, 4, ".ply") == 0;
      if (mesh_texture != 0 && !ply) {
        // the appearance at a resolution of its own, on the device: one network pass per texel, looked at head-on
        const auto t0 = std::chrono::steady_clock::now();
        const NerfRender::MeshTexture tex = render->bake_mesh_texture((uint32_t)mesh_texture, (uint32_t)mesh_texture_width);
        const auto t1 = std::chrono::steady_clock::now();
        std::printf("mesh texture: res %u, atlas %u x %u, %zu triangles, %llu texels refused, %f s\n", tex.res, tex.width, tex.height,
                    tex.uvs.size() / 6, (unsigned long long)tex.refused, std::chrono::duration<double>(t1 - t0).count());
        if (!NerfRender::save_obj_textured(mesh_path, mesh.vertices, mesh.triangles, tex.uvs, tex.rgba8, tex.width, tex.height))
          throw std::runtime_error{"cannot write " + mesh_path};
      } else if (ply) {
        // normals and colours in one launch at the device vertices (a vertex within the step of the box's faces gets zeros)
        const auto a0 = std::chrono::steady_clock::now();
        const NerfRender::MeshAttributes attr = render->mesh_attributes(b / 128.0f);
        const auto a1 = std::chrono::steady_clock::now();
        std::printf("mesh attributes: %zu vertices, %f s\n", attr.sigmas.size(), std::chrono::duration<double>(a1 - a0).count());
        if (!NerfRender::save_ply(mesh_path, mesh.vertices, mesh.triangles, attr.normals, attr.colors)) throw std::runtime_error{"cannot write " + mesh_path};
      } else {
        // OBJ, vertex normals: nrf_density_gradient takes the device vertices as they are; its records need n float4 of device memory,
        // which an n x 1 render buffer's accumulate plane is
        std::vector<float> normals;
        if (!mesh.vertices.empty()) {
          RenderBuffer records;
          records.resize(Vector2i((int)(mesh.vertices.size() / 3), 1));
          render->density_gradient(mesh.vertices_dev, (uint32_t)(mesh.vertices.size() / 3), b / 128.0f, records.accumulate_buffer());
          normals = NerfRender::normals_from_gradients(records.accumulate_buffer_host());
        }
        if (!NerfRender::save_obj(mesh_path, mesh.vertices, mesh.triangles, normals)) throw std::runtime_error{"cannot write " + mesh_path};
      }
    }
    delete render;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
