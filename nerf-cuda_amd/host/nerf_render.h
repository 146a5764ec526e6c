// nerf_render.h -- C++ host mirror of the reference's renderer class on the C ABI.
//
// Same names, argument meaning and error behaviour as ngp::NerfRender
// (reference include/nerf-cuda/nerf_render.h:29-50), ngp::Camera and ngp::Image
// (include/nerf-cuda/common.h:68-89).  Third-party parameter types are replaced
// by small own equivalents: Eigen::Vector2i -> ngp::Vector2i, Eigen::Matrix4f ->
// ngp::Matrix4f (row-major, operator()(row, col)), nlohmann::json -> mpk::Value,
// filesystem::path -> std::string.  Everything device-side happens behind
// include/nerfhip.h; this file contains no HIP.
#pragma once
#include <string>
#include <vector>

#include "../../include/nerfhip.h"
#include "msgpack_lite.h"

namespace ngp {

struct Camera {  // reference common.h:68-74
  float fl_x, fl_y, cx, cy;
};

struct Image {  // reference common.h:76-89; pointers are owned by NerfRender (pinned host memory the GPU's copy engine
                // fills), valid until the second next render call (the reference: until the next render_frame)
  int W, H;
  unsigned char* rgb;    // W * H * 3, row-major
  unsigned char* depth;  // W * H
  Image(int w, int h, unsigned char* in_rgb, unsigned char* in_depth) : W(w), H(h), rgb(in_rgb), depth(in_depth) {}
};

struct Vector2i {
  int v[2];
  Vector2i(int x = 0, int y = 0) : v{x, y} {}
  int& operator[](int i) { return v[i]; }
  int operator[](int i) const { return v[i]; }
};

struct Matrix4f {  // row-major 4x4, camera-to-world in the NeRF/Blender convention
  float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float& operator()(int r, int c) { return m[4 * r + c]; }
  float operator()(int r, int c) const { return m[4 * r + c]; }
};

class NerfRender {
 public:
  // The reference fixes the device count with the NGPU macro (common.h:91); here it is a
  // constructor argument (or the NERF_NGPU environment variable; NERF_DEVICES="0,1,..." names the
  // devices, repeats allowed).  The devices form an nrf_group: member i renders the tile strips with
  // strip_id % n == i, the shards travel device-to-device to the first member, which untiles
  // (the reference: one thread per device, D2H copies, host de-interleave, nerf_render.cu:252-362).
  // n_gpus < 0: host-only instance that can load and inspect snapshots but not render.
  explicit NerfRender(int n_gpus = 0);
  // the same over an explicit device list (e.g. {3}: a single-device renderer on GPU 3, as a render_server worker)
  explicit NerfRender(const std::vector<int>& devices);
  ~NerfRender();
  NerfRender(const NerfRender&) = delete;
  NerfRender& operator=(const NerfRender&) = delete;

  void reload_network_from_file(const std::string& network_config_path);
  mpk::Value load_network_config(const std::string& network_config_path);
  void reset_network();
  void set_resolution(Vector2i resolution);
  Image render_frame(Camera cam, Matrix4f pos);
  // Batched form (addition): all views in one launch per NRF_MAX_VIEWS cameras (nrf_render_views); every
  // returned Image equals render_frame of that camera.  The images stay valid until the next render call.
  std::vector<Image> render_frames(const std::vector<Camera>& cams, const std::vector<Matrix4f>& poses);
  // Pipelined form of render_frames (addition): submit_frames starts the render + the copy to host memory and returns
  // a ticket at once; wait_frames blocks until that batch is in host memory.  Two batches may be in flight, so the
  // copy (and whatever the caller does with the images) of batch k overlaps the render of batch k + 1; the images of a
  // ticket stay valid until the second next submit_frames.  rgb_only: Image::depth is nullptr, its plane is not copied.
  int submit_frames(const std::vector<Camera>& cams, const std::vector<Matrix4f>& poses, bool rgb_only = false);
  std::vector<Image> wait_frames(int ticket);
  float last_wait_render_ms() const { return m_last_wait_render_ms; }  // device time of the batch wait_frames returned last
  // device ray buffers of the reference are internal to the fused kernel; this fills host copies
  void generate_rays(Camera cam, Matrix4f pos, int threadid);
  // Frame from caller-supplied rays (addition; nrf_render_rays): rays_o / rays_d are DEVICE pointers, fp32 [rays_per_view][3] in the
  // space and layout generate_rays produces (ngp units, row-major pixels of the set_resolution frame); pixels beyond
  // rays_per_view and rays the guard refuses are background.  Single-device renderers only (device groups are out of its
  // scope).  The Image is host memory of this object, valid until the next render_rays.
  Image render_rays(const void* rays_o, const void* rays_d, uint64_t rays_per_view);
  // ... between per-ray limits of t and over a per-ray background (nrf_render_rays_clipped): t_min / t_max are DEVICE fp32
  // [rays_per_view] in units of t along the (not normalised) direction, background DEVICE fp32 [rays_per_view][3]; nullptr each:
  // no limit / the renderer's background.  What a rasteriser passes to mix the NeRF into its scene: its G-buffer's hit distance
  // as t_max, its shaded colour as background.  The Image's depth is the normalised one: the metric depth plane
  // (NRF_RAYS_DEPTH_T) is a float plane an 8-bit Image cannot hold, and is reachable through the C call only.
  // So is the density-only mode for shadow and occlusion rays (NRF_RAYS_DENSITY_ONLY): it renders float planes only.
  Image render_rays(const void* rays_o, const void* rays_d, uint64_t rays_per_view, const void* t_min, const void* t_max,
                    const void* background);
  // nrf_ray_hits (nerfhip.h): where each of n rays (device fp32 [n][3] origins and directions, n <= width * height of set_resolution;
  // optional device fp32 [n] limits of t) first reaches the weight sum `opacity` -- picking, collision, the origins of shadow rays.
  // Returns [n][4] records followed by [n] depths as host floats: a hit is (t of the crossing sample, its dt, the weight sum before it,
  // the weight sum after it >= opacity), a miss (0, 0, 0, the final weight sum < opacity); the depth is the sum of w * t as composited.
  // Single device only, as render_rays.
  std::vector<float> ray_hits(const void* rays_o, const void* rays_d, uint64_t n, float opacity, const void* t_min = nullptr,
                              const void* t_max = nullptr);
  // nrf_density / nrf_density_gradient (nerfhip.h): sigma of the density network alone at n points (device fp32 [n][3]) into device
  // float [n], and (g_x, g_y, g_z, sigma) by central differences of step h into device float4 [n].  A point with a tap coordinate
  // that is not finite or outside [-bound, bound] yields zeros.  Synchronous; single device only, as render_rays.
  void density(const void* xyz, uint32_t n, void* sigma_dev);
  void density_gradient(const void* xyz, uint32_t n, float h, void* out_dev);
  // nrf_ray_hits followed by nrf_hit_gradients on its frame: for each of the n rays that reaches `opacity`, pos (device float4
  // [width * height]) = (x, y, z, tq) with tq = t - frac * dt on the ray and out (likewise) = the gradient record there; zeros for
  // every other pixel.  The records themselves stay readable as after ray_hits (nrf_read_f32).
  void hit_gradients(const void* rays_o, const void* rays_d, uint64_t n, float opacity, float frac, float h, void* pos_dev, void* out_dev,
                     const void* t_min = nullptr, const void* t_max = nullptr);
  // surface normals of host copies of such records ([m][4]): -g / |g|, zero where |g| == 0 -> [m][3]
  static std::vector<float> normals_from_gradients(const std::vector<float>& records);
  // nrf_extract_mesh (nerfhip.h): the iso-surface sigma == iso of the density network on the lattice of dims points per axis at
  // origin + index * cell, by marching tetrahedra on the device -> host vertices [n][3] and triangles [m][3] (counter-clockwise seen
  // from outside).  vertices_dev is the device copy ([n][3], owned by the context until the next extract_mesh): density_gradient
  // takes it as it is, and normals_from_gradients of a host copy of its records are the vertex normals.  Synchronous; single device.
  struct Mesh {
    std::vector<float> vertices;
    std::vector<uint32_t> triangles;
    const void* vertices_dev = nullptr;
  };
  Mesh extract_mesh(const float origin[3], const float cell[3], const uint32_t dims[3], float iso);
  // nrf_mesh_components (nerfhip.h): the connected components of the last extract_mesh / filter_mesh, labelled on the device -> host
  // labels [n] (the smallest vertex id of each vertex's component) and table [c][3] = (label, vertices, triangles) in ascending label;
  // rounds = the hook + compress rounds the labelling took.  Synchronous; single device.
  struct MeshComponents {
    std::vector<uint32_t> labels, table;
    uint32_t rounds = 0;
  };
  MeshComponents mesh_components();
  // nrf_filter_mesh (nerfhip.h): keeps the components with at least min_triangles triangles -- with keep_largest only the one with the
  // most triangles, a tie going to the smaller label -- and makes the result the context's mesh (mesh_attributes then sees it) -> the
  // filtered mesh as extract_mesh returns one.  Synchronous; single device.
  Mesh filter_mesh(uint64_t min_triangles, bool keep_largest);
  // nrf_refine_mesh (nerfhip.h): every vertex of the context's mesh moves along its lattice edge onto the iso value of the density
  // network, n_steps (0 .. 16) bisections and one secant step, in one launch on the device -> the refined host vertices [n][3] (the
  // triangles do not change; vertices_dev is the same buffer, rewritten in place) and the number of vertices left as they were because
  // their edge does not bracket iso.  After filter_mesh and before mesh_attributes is the cheap order.  Synchronous; single device.
  struct MeshRefinement {
    std::vector<float> vertices;
    uint64_t unbracketed = 0;
    const void* vertices_dev = nullptr;
  };
  MeshRefinement refine_mesh(uint32_t n_steps);
  // nrf_simplify_mesh (nerfhip.h): vertex clustering on the extraction's lattice, on the device -- the vertices whose lattice points
  // share a block of factor^3 points (factor 1 .. 256) merge into the one nearest the block's centre, collapsed triangles and vertices
  // nothing names any more are dropped, and the result is the context's mesh (filter_mesh, refine_mesh and mesh_attributes then see it)
  // -> the simplified mesh as extract_mesh returns one, with sources [n] (the old id of every vertex, ascending) and vertex_map
  // [vertices before] (the new id of every old vertex's representative, or 0xffffffff).  After filter_mesh and refine_mesh and before
  // mesh_attributes is the intended order.  Synchronous; single device.
  struct SimplifiedMesh : Mesh {
    std::vector<uint32_t> sources, vertex_map;
  };
  SimplifiedMesh simplify_mesh(uint32_t factor);
  // Wavefront OBJ: "v x y z" per vertex, "vn x y z" per vertex when normals ([n][3]) has one per vertex, faces 1-based ("f a//a b//b c//c"
  // with normals, "f a b c" without).  Returns false when the file cannot be written.
  static bool save_obj(const std::string& path, const std::vector<float>& vertices, const std::vector<uint32_t>& triangles,
                       const std::vector<float>& normals = {});
  // nrf_bake_mesh_texture (nerfhip.h): the colours of the full network on a per-triangle texture atlas of the current mesh, on the
  // device -- res texels along a triangle's legs (2 .. 256), two triangles per cell of (res + 2) x (res + 1) texels, width / (res + 2)
  // cells per atlas row -> host copies: texels [height][width][4] = (r, g, b, sigma), rgba8 [height][width] (alpha 255 where a
  // triangle's texel was evaluated, 0 elsewhere), uvs [n_triangles][3][2] (v grows with the atlas row) and the count of texels the
  // guard zeroed.  The mesh is only read; after filter_mesh, refine_mesh and simplify_mesh is the intended place.  Synchronous; single
  // device.
  struct MeshTexture {
    uint32_t width = 0, height = 0, res = 0;
    uint64_t refused = 0;
    std::vector<float> texels, uvs;
    std::vector<uint32_t> rgba8;
  };
  MeshTexture bake_mesh_texture(uint32_t res, uint32_t width);
  // Wavefront OBJ with a texture: `path` ("v", three "vt u (1 - v)" per triangle, "f a/3t+1 b/3t+2 c/3t+3", 1-based), next to it
  // <stem>.mtl (one material whose map_Kd names the image) and <stem>.png (the atlas's rgb, 8 bits, first row on top).  uvs is
  // [n_triangles][3][2], rgba8 [height][width].  Returns false when the sizes disagree or a file cannot be written.
  static bool save_obj_textured(const std::string& path, const std::vector<float>& vertices, const std::vector<uint32_t>& triangles,
                                const std::vector<float>& uvs, const std::vector<uint32_t>& rgba8, uint32_t width, uint32_t height);
  // nrf_mesh_attributes (nerfhip.h): unit normals and colours at the vertices of the last extract_mesh, in one launch on the device
  // -> host normals [n][3] (outward, -g / |g|; zeros where the gradient is degenerate), colours [n][3] (the network's rgb, looked at
  // along -normal), sigmas [n] and |g| [n].  h is the step of the central differences; a vertex within h of the box's faces gets
  // zeros throughout.  Synchronous; single device.
  struct MeshAttributes {
    std::vector<float> normals, colors, sigmas, lengths;
  };
  MeshAttributes mesh_attributes(float h);
  // Binary little-endian PLY: per vertex "x y z nx ny nz" as float and "red green blue" as uchar -- a colour byte is the library's
  // 8-bit rule (nerfhip.h: (unsigned char)(255.0 * x), saturating, NaN -> 0) --, faces as "list uchar int vertex_indices".  normals and
  // colors are [n][3], one per vertex.  Returns false when they are not, or when the file cannot be written.
  static bool save_ply(const std::string& path, const std::vector<float>& vertices, const std::vector<uint32_t>& triangles,
                       const std::vector<float>& normals, const std::vector<float>& colors);
  // the density grid from the network (nerf_render.cu:388-429, dead and incomplete in the reference; completed in
  // nrf_generate_density_grid); reload_network_from_file calls it for a snapshot that carries no density grid
  void generate_density_grid();
  // Reads the reference's snapshot format (nerf_render.cu:431-473) and, in addition, instant-ngp's own layout
  // (`snapshot.nerf`, `params_binary`, Morton-ordered `density_grid_binary`: see nerf_render.cpp load_ngp_snapshot).
  void load_snapshot(const std::string& filepath_string);

  // additions (the reference has no accessors)
  // Device memory a model may spend on gather copies of its hash grid (nrf_model_desc.gather_copy_budget_mb: 0 = the library's
  // default, a sixteenth of the device's memory; 1 = none); takes effect at the next load_snapshot / reload_network_from_file
  void set_gather_copy_budget_mb(uint32_t mb) { m_gather_copy_budget_mb = mb; }
  int n_gpus() const { return (int)m_ctx.size(); }
  const nrf_model_desc& model_desc() const { return m_desc; }
  nrf_stats last_stats(int gpu = 0) const;
  const std::vector<float>& rays_o() const { return m_rays_o; }
  const std::vector<float>& rays_d() const { return m_rays_d; }

 private:
  void check(int rc, const char* what) const;
  void load_ngp_snapshot(const mpk::Value& config);
  float m_ngp_per_level_scale = 0.0f;  // instant-ngp snapshots: per_level_scale derived from aabb_scale (0: not one)
  bool m_ngp_rgb_sigmoid = false;      //   ... and instant-ngp's logistic colour activation
  nrf_group* m_group = nullptr;
  std::vector<nrf_context*> m_ctx;  // the group's members (owned by the group)
  mpk::Value m_network_config;
  std::string m_network_config_path;
  nrf_model_desc m_desc{};
  uint32_t m_gather_copy_budget_mb = 0;
  size_t m_mesh_vertices = 0;  // of the context's current mesh (extract_mesh, filter_mesh)
  bool m_have_snapshot = false, m_have_network = false;
  std::vector<float> m_params, m_density_grid;
  Vector2i resolution;
  float m_last_wait_render_ms = 0.f;
  std::vector<float> m_rays_o, m_rays_d;
  std::vector<unsigned char> m_rays_rgb, m_rays_depth;  // render_rays' Image
};

// Camera path from a NeRF-synthetic / instant-ngp `transforms.json` (intrinsics scaled to width x height; 0 = the file's w / h)
void load_camera_path(const std::string& transforms_json, int width, int height, std::vector<Camera>& cams, std::vector<Matrix4f>& poses);

}  // namespace ngp
