// nrf_api.hip -- the C ABI of include/nerfhip.h on top of the gfx950 kernels.
//
// Host-side mirror of what ngp::NerfRender does around its kernels
// (R/src/nerf_render.cu): model upload (load_snapshot + reset_network +
// NerfNetwork::deserialize), buffer allocation (set_resolution) and one
// kernel launch per frame (render_frame).  No CPU compute path exists here:
// without a gfx950 device nrf_create fails.

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "nrf_device.h"
#include "nrf_frame_plan.h"
#include "nrf_generic.h"
#include "nrf_grid_plan.h"
#include "nrf_launch.h"
#include "nrf_meshcc_plan.h"
#include "nrf_refine_plan.h"
#include "nrf_simplify_plan.h"
#include "nrf_model_plan.h"
#include "nrf_points_plan.h"
#include "nrf_temporal_plan.h"

using namespace nrf;

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int hip_fail(hipError_t e, const char* what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return NRF_E_HIP;
}
#define HIP_TRY(expr)                            \
  do {                                           \
    hipError_t _e = (expr);                      \
    if (_e != hipSuccess) return hip_fail(_e, #expr); \
  } while (0)

// R/include/nerf-cuda/render_utils.h:68-77
void nerf_matrix_to_ngp(const float p[16], float s, float R[9], float org[3]) {
  const int rows[3] = {1, 2, 0};
  for (int r = 0; r < 3; ++r) {
    const float* src = p + 4 * rows[r];
    R[3 * r + 0] = src[0];
    R[3 * r + 1] = -src[1];
    R[3 * r + 2] = -src[2];
    org[r] = src[3] * s + 0.0f;
  }
}

}  // namespace

struct nrf_context {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool model_loaded = false;
  nrf_model_desc desc{};
  nrf_level_table lv{};
  DevModel dm{};
  void* d_grid = nullptr;
  void* d_occ = nullptr;
  void* d_wfrag = nullptr;
  void* d_lv = nullptr;
  void* d_coarse = nullptr;
  void* d_dilated = nullptr;
  void* d_ctab = nullptr;
  void* d_gen = nullptr;
  void* d_wfrag_gen = nullptr;  // wide models: generic-layout fragments for the stage entry points
  GridFit fit{};                // what plan_grid made of the current density grid (fit.rays_persistent: nrf_render_rays runs the persistent RAYS instance)
  size_t table_words[4] = {0, 0, 0, 0};  // words of d_occ, d_coarse, d_ctab, d_dilated
  int own_net = NET_HOT;        // the loaded model's own instance (plan_model): plan_grid checks for every grid whether it fits
  void* d_wfrag_hot = nullptr;  // fragments of the model's own register-resident instance when it is not the stage one
  GenModel gen{};  // host copy of the generic instance's description (valid unless dm.stage == NET_HOT)
  size_t wfrag_bytes = 0, wfrag_gen_bytes = 0, wfrag_hot_bytes = 0;  // bytes of d_wfrag, d_wfrag_gen, d_wfrag_hot (nrf_debug_model_readout)
  std::vector<float> host_grid;  // the float density grid the march tables were built from
  bool grid_missing = false;     // loaded without a density grid and none generated yet
  bool allow_persistent = true;  // NRF_PERSISTENT=0 keeps the one-workgroup-per-strip render_kernel (A/B runs)
  bool allow_gather_plan = true; // NRF_GATHER_PLAN=0: the hot instance selects every gather step's form at run time (GATHER_RUNTIME; A/B runs)
  bool centre_out = true;        // NRF_CENTRE_OUT=0: the persistent kernel's queue in row order
  bool allow_gen_wlds = true;    // NRF_GEN_WLDS=0: the generic instance's weight fragments are never staged in LDS
  bool allow_width_instances = true;  // NRF_WIDTH_INSTANCES=0: 16 / 32 / 128-neuron models render in the generic instance (A/B runs)
  int queue_classes = 0;         // NRF_QUEUE_CLASSES=1..8: work queues of the persistent kernel (default: one per XCD)
  int n_cus = 256;
  nrf_options opt{};
  int W = 0, H = 0;
  int n_local_tiles = 0;
  int max_views = 1;    // views the context's own frame buffers hold (nrf_set_max_views)
  int last_views = 1;
  size_t n_out_px = 0;  // pixels of ONE view in the frame buffers (= the view stride)
  size_t n_alloc_px = 0;
  void* d_rgba = nullptr;
  void* d_depth = nullptr;
  void* d_plan = nullptr;      // CALL_RING plan buffers (plan_price_kernel / plan_sort_kernel: the queue order of a launch), PLAN_BYTES each
  int plan_max_pos = 1 << 14;  // launches of up to this many strips are planned (NRF_PLAN_MAX_POS; 0: never) -- one or two 1080p views
  void* d_counters = nullptr;  // CALL_RING slots of statistics counters + work queues, one per render call (call_slot)
  int call_index = 0;          // ring position of the last render call
  int quad_levels = -1;        // NRF_QUAD_LEVELS=n: only the first n levels (whole steps of four) may get a cell-major quad copy (0: none; A/B runs)
  int quad_budget_mb = -1;     // NRF_QUAD_BUDGET_MB=m overrides nrf_model_desc.gather_copy_budget_mb (A/B runs, render_server deployments)
  uint64_t table_bytes = 0, table_ref_bytes = 0;  // device bytes of the grid table with / without the quad copies
  uint32_t gather_addresses = 0;  // lane addresses one sample sends into the texture path with the loaded model (nrf_stats)
  bool allow_gen_fast_grid = true;  // NRF_GEN_FAST_GRID=0: the generic instance always encodes with gen_level (A/B runs)
  int march_ff = 1;            // NRF_MARCH_FF=0: no barrier fast-forward ahead of t_skip (A/B runs, equality tests)
  int tail_split = 1;          // NRF_TAIL_SPLIT=0: no tail splitting in the persistent kernel (A/B runs)
  // The barrier fast-forward's step tables (nrf_step_plan.h), one per (min_near, dt_gamma, bound, H) a call has rendered with: built
  // and uploaded once into a buffer of its own, never rewritten (a launch in flight may still read it), freed with the context.
  struct StepTable {
    uint32_t key[4];
    float* d = nullptr;
    int n = 0;
  };
  std::vector<StepTable> step_tables;
  bool allow_step_table = true;              // NRF_STEP_TABLE=0: every launch gets a null table and steps (A/B runs, equality tests)
  int step_table_cap = STEP_TABLE_CAPACITY;  // NRF_STEP_TABLE_CAP=n: tables of n entries (tests: targets beyond the table at small shapes)
  void* d_rgb8 = nullptr;
  void* d_depth8 = nullptr;
  void* bound_rgba = nullptr;  // caller-owned targets (nrf_bind_output)
  void* bound_depth = nullptr;
  void* bound_rgbd8 = nullptr;  // caller-owned packed 8-bit target (nrf_bind_output_rgbd8)
  void* bound_rgb8 = nullptr;   // caller-owned 8-bit planar targets (nrf_bind_output_u8)
  void* bound_depth8 = nullptr;
  // host frames (nrf_submit_host_u8): HOST_SLOTS x {device 8-bit planes the kernel writes, pinned host planes the copy
  // engine fills}, so that the copy of one call overlaps the render of the next
  struct HostSlot {
    void* d_buf = nullptr;     // device: rgb [views][px][3] | depth [views][px]
    uint8_t* h_buf = nullptr;  // pinned host, same layout
    size_t views = 0, px = 0;  // capacity
    hipEvent_t done = nullptr, t0 = nullptr, t1 = nullptr;  // done: the call's last copy; t0 / t1: around its render launches
    hipEvent_t grp[2] = {nullptr, nullptr};                 // the two copy groups a progressive call keeps in flight (progressive_copies)
    std::vector<int> row_lo, row_hi;  // per view: the rows of the pinned planes that do not hold the background value ...
    std::vector<int> col_lo, col_hi;  // ... and, inside those rows, the columns
    int bg = -1;               // the 8-bit background value the other rows hold (-1: nothing filled yet)
    int n_views = 0, W = 0, H = 0;
    bool with_depth = true, pending = false;
    uint64_t copied = 0;
    std::vector<int> rows;     // this call: per view the rows [lo, hi) and the columns [x0, x1) of its region of interest (what is copied)
    // progress reporting (FrameParams::prog_*): the kernel flags finished strip rows, nrf_wait_host_u8 copies them meanwhile
    unsigned* d_done = nullptr;   // device [views][tiles_y]
    unsigned* h_flags = nullptr;  // pinned host [views][tiles_y]
    size_t prog_entries = 0;
    unsigned epoch = 0;
    bool progressive = false, copies_issued = false;
  } hs[2];
  int hs_next = 0;
  hipStream_t copy_stream = nullptr;
  bool host_merge = true;        // NRF_HOST_MERGE=0: every ready band is copied by itself, at once (A/B runs)
  bool host_progressive = true;  // NRF_HOST_PROGRESSIVE=0: every copy of a host frame waits for the end of its render (A/B runs)
  bool host_cols = true;         // NRF_HOST_COLS=0: a host frame that is copied after its render travels as whole rows (A/B runs)
  bool host_skip_outside = true; // NRF_HOST_SKIP_OUTSIDE=0: the kernel writes the background rows of a host frame as well (A/B runs)
  void* last_rgba = nullptr;
  void* last_depth = nullptr;
  int march_budget = 256;  // NRF_MARCH_BUDGET overrides (tuning only; the image does not depend on it)
  bool sample_cap_forced = false;  // NRF_SAMPLE_CAP was given: it holds for every launch (else launches of one or two views queue 8)
  int sample_cap = 2;      // per-round sample queue of a ray by its transmittance (FrameParams::sample_cap); NRF_SAMPLE_CAP=0 / 1: A/B runs
  bool rendered = false;
  hipStream_t last_stream = nullptr;
  // nrf_extract_mesh: the last mesh and the polygoniser's workspace, grown as needed (capacities in bytes)
  struct MeshBuffers {
    void *sigma = nullptr, *codes = nullptr, *vbase = nullptr, *tbase = nullptr, *partials = nullptr, *vertices = nullptr, *triangles = nullptr;
    size_t cap_sigma = 0, cap_codes = 0, cap_vbase = 0, cap_tbase = 0, cap_partials = 0, cap_vertices = 0, cap_triangles = 0;
    uint32_t* totals = nullptr;  // device: n_vertices, n_triangles, the emit pass's flag, nrf_refine_mesh's count of unbracketed vertices
    uint64_t n_vertices = 0, n_triangles = 0;
    bool have = false;
    // nrf_mesh_attributes: float4 [n_vertices] each, of the mesh above (have_attr falls with every nrf_extract_mesh)
    void *normals = nullptr, *colors = nullptr;
    size_t cap_normals = 0, cap_colors = 0;
    bool have_attr = false;
    // nrf_mesh_components / nrf_filter_mesh: the labelling and the table of the mesh above (have_parts falls with every
    // nrf_extract_mesh, nrf_filter_mesh and nrf_simplify_mesh), the second vertex / triangle buffers the filter scatters into and then
    // swaps in, and
    // cc_words (device): the largest component's key (64 bits), the hook's changed flag, the scatter's flag, a scan's two totals
    void *labels = nullptr, *rows = nullptr, *components = nullptr, *vertices2 = nullptr, *triangles2 = nullptr;
    size_t cap_labels = 0, cap_rows = 0, cap_components = 0, cap_vertices2 = 0, cap_triangles2 = 0;
    uint32_t* cc_words = nullptr;
    uint64_t n_components = 0;
    uint32_t n_rounds = 0;
    bool have_parts = false;
    void* sigma_used = nullptr;  // nrf_mesh.sigma of the extraction
    // nrf_refine_mesh: the edge word of every vertex of the mesh above (written by nrf_extract_mesh, carried by nrf_filter_mesh into
    // edges2, which is then swapped in), the lattice and the iso of the extraction, and the bracket records of the last refinement
    // (have_brackets falls with every nrf_extract_mesh, nrf_filter_mesh and nrf_simplify_mesh)
    void *edges = nullptr, *edges2 = nullptr, *brackets = nullptr;
    size_t cap_edges = 0, cap_edges2 = 0, cap_brackets = 0;
    MeshLattice lattice{};
    float iso = 0.f;
    bool have_brackets = false;
    // nrf_simplify_mesh: the dense key table, the used / survive flags, and the records of the last simplification (have_simplify
    // falls with every nrf_extract_mesh and nrf_filter_mesh); n_vertices_before = the elements of vertex_map; it scatters into
    // vertices2 / triangles2 / edges2 and swaps them in, as the filter does
    void *skeys = nullptr, *sused = nullptr, *ssurvive = nullptr, *sources = nullptr, *vertex_map = nullptr;
    size_t cap_skeys = 0, cap_sused = 0, cap_ssurvive = 0, cap_sources = 0, cap_vertex_map = 0;
    uint64_t n_vertices_before = 0;
    bool have_simplify = false;
    // nrf_bake_mesh_texture: the atlas planes and the UVs of the mesh above, the counter of refused texels (device) and the layout and
    // count of the last bake (have_texture falls with every nrf_extract_mesh, nrf_filter_mesh, nrf_refine_mesh and nrf_simplify_mesh)
    void *texels = nullptr, *rgba8 = nullptr, *uvs = nullptr, *bake_count = nullptr;
    size_t cap_texels = 0, cap_rgba8 = 0, cap_uvs = 0, cap_bake_count = 0;
    BakeLayout texture{};
    bool have_texture = false;
  } mesh;
};

namespace {

int set_device(nrf_context* c) {
  HIP_TRY(hipSetDevice(c->device));
  return NRF_OK;
}

void free_model(nrf_context* c) {
  if (c->d_grid) (void)hipFree(c->d_grid);
  if (c->d_occ) (void)hipFree(c->d_occ);
  if (c->d_wfrag) (void)hipFree(c->d_wfrag);
  if (c->d_lv) (void)hipFree(c->d_lv);
  if (c->d_coarse) (void)hipFree(c->d_coarse);
  if (c->d_ctab) (void)hipFree(c->d_ctab);
  if (c->d_dilated) (void)hipFree(c->d_dilated);
  if (c->d_gen) (void)hipFree(c->d_gen);
  if (c->d_wfrag_gen) (void)hipFree(c->d_wfrag_gen);
  if (c->d_wfrag_hot) (void)hipFree(c->d_wfrag_hot);
  c->d_wfrag_gen = c->d_wfrag_hot = nullptr;
  c->d_grid = c->d_occ = c->d_wfrag = c->d_lv = c->d_coarse = c->d_ctab = c->d_dilated = c->d_gen = nullptr;
  c->model_loaded = false;
}

constexpr int CALL_RING = 16;  // render calls of one context that may be in flight on different streams
constexpr size_t CALL_SLOT_BYTES = COUNTER_BYTES + 128 + 65536;  // statistics | work queues | the diagnostic build's per-wave stamps
constexpr int HOST_SLOTS = 2;
// Cell-major quad copies of grid levels (nrf_load_model; nrf_device.h level_gather_quad): which levels get one by default.
constexpr uint32_t QUAD_BUDGET_MB_DEFAULT = 8192;  // base.json's grid: levels 0..7 take 95 MB, levels 8..11 4.5 GB (levels 12..15: 216 GB, never copied);
                                                   // an instant-ngp grid at aabb_scale 32: levels 0..3 2.4 MB, levels 4..7 9.2 GB
inline char* call_slot(const nrf_context* c, int index) { return (char*)c->d_counters + (size_t)(index % CALL_RING) * CALL_SLOT_BYTES; }

void free_host_slots(nrf_context* c) {
  for (auto& h : c->hs) {
    if (h.d_buf) (void)hipFree(h.d_buf);
    if (h.h_buf) (void)hipHostFree(h.h_buf);
    if (h.d_done) (void)hipFree(h.d_done);
    if (h.h_flags) (void)hipHostFree(h.h_flags);
    h.d_buf = nullptr;
    h.h_buf = nullptr;
    h.d_done = h.h_flags = nullptr;
    h.views = h.px = h.prog_entries = 0;
    h.bg = -1;
    h.pending = false;
  }
}

void free_frame(nrf_context* c) {
  if (c->d_rgba) (void)hipFree(c->d_rgba);
  if (c->d_depth) (void)hipFree(c->d_depth);
  if (c->d_rgb8) (void)hipFree(c->d_rgb8);
  if (c->d_depth8) (void)hipFree(c->d_depth8);
  c->d_rgba = c->d_depth = c->d_rgb8 = c->d_depth8 = nullptr;
  c->n_out_px = 0;
  c->rendered = false;
}

void free_mesh(nrf_context* c) {
  auto& m = c->mesh;
  for (void* q : {m.sigma, m.codes, m.vbase, m.tbase, m.partials, m.vertices, m.triangles, m.normals, m.colors, (void*)m.totals,
                  m.labels, m.rows, m.components, m.vertices2, m.triangles2, (void*)m.cc_words, m.edges, m.edges2, m.brackets,
                  m.skeys, m.sused, m.ssurvive, m.sources, m.vertex_map, m.texels, m.rgba8, m.uvs, m.bake_count})
    if (q) (void)hipFree(q);
  m = nrf_context::MeshBuffers{};
}

// a buffer of the mesh extraction holds at least `need` bytes afterwards (its contents are not kept)
int grow_mesh_buffer(void** p, size_t& cap, uint64_t need) {
  if (need <= cap) return NRF_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  cap = 0;
  HIP_TRY(hipMalloc(p, (size_t)need));
  cap = (size_t)need;
  return NRF_OK;
}

// the shard layout (tile-major [n_tiles][64]) instead of the row-major frame: every multi-shard render, and a single shard on request
bool tiled_layout(const nrf_context* c) { return c->opt.shard_count > 1 || c->opt.tile_major != 0; }

int alloc_frame(nrf_context* c) {
  if (c->W <= 0 || c->H <= 0) return NRF_OK;
  const bool tiled = tiled_layout(c);
  c->n_local_tiles = local_tiles(c->W, c->H, c->opt.shard_index, c->opt.shard_count);
  const size_t per_view = tiled ? (size_t)tiles_per_shard(c->W, c->H, c->opt.shard_count) * 64 : (size_t)c->W * c->H;
  const size_t need = per_view * (size_t)c->max_views;
  if (per_view == c->n_out_px && need == c->n_alloc_px && c->d_rgba) return NRF_OK;
  HIP_TRY(hipDeviceSynchronize());
  free_frame(c);
  HIP_TRY(hipMalloc(&c->d_rgba, need * 16));
  HIP_TRY(hipMalloc(&c->d_depth, need * 4));
  HIP_TRY(hipMemsetAsync(c->d_rgba, 0, need * 16, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_depth, 0, need * 4, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->n_out_px = per_view;
  c->n_alloc_px = need;
  return NRF_OK;
}

int fill_frame_params(nrf_context* c, const float cam[4], const float pose[16], FrameParams& P) {
  std::memset(&P, 0, sizeof(P));
  nerf_matrix_to_ngp(pose, c->desc.scale, P.R, P.org);
  for (int i = 0; i < 4; ++i) P.cam[i] = cam[i];
  P.W = c->W;
  P.H = c->H;
  P.tiles_x = tiles_of(c->W);
  P.tiles_y = tiles_of(c->H);
  P.shard_index = c->opt.shard_index;
  P.shard_count = c->opt.shard_count;
  P.n_local_tiles = c->n_local_tiles;
  P.tile_major = tiled_layout(c);
  P.bg_color = c->opt.bg_color;
  P.min_near = c->opt.min_near;
  P.dt_gamma = c->opt.dt_gamma;
  P.density_scale = c->opt.density_scale;
  P.max_steps = c->opt.max_steps;
  P.march_budget = c->march_budget;
  P.sample_cap = c->sample_cap;
  P.centre_out = c->centre_out ? 1 : 0;
  P.out_mode = c->bound_rgbd8 ? OUT_RGBD8 : (c->bound_rgb8 ? OUT_U8 : OUT_F32);
  P.skip_outside = 0;
  P.prog_done = P.prog_flags = nullptr;
  P.prog_epoch = 0;
  P.tail_split = c->tail_split;
  P.perturb = c->opt.perturb;
  P.march_ff = c->opt.perturb ? 0 : c->march_ff;  // (the fast-forward replays a chain that starts at `near`: a shifted chain keeps its trips)
  P.fast_interp = c->opt.fast_interp ? 1 : 0;
  P.queue_classes = c->queue_classes;
  return NRF_OK;
}

// The step table of a call's options and the loaded model (nrf_step_plan.h): where launch_render hands it to the persistent
// kernel.  Cached per context under the bits of its four inputs; a new key is built on the host and uploaded once.  tab stays
// null when the switch is off or the inputs have no table: the kernel steps.
constexpr size_t STEP_TABLES_MAX = 64;  // distinct option sets a context keeps tables for; beyond that all are dropped and rebuilt
int step_table_for(nrf_context* c, const FrameParams& P, const float*& tab, int& n) {
  tab = nullptr;
  n = 0;
#if NRF_STEP_TABLE
  if (!c->allow_step_table) return NRF_OK;
  const uint32_t key[4] = {step_bits(P.min_near), step_bits(P.dt_gamma), step_bits(c->dm.bound), c->dm.H};
  for (const auto& s : c->step_tables)
    if (std::memcmp(s.key, key, sizeof(key)) == 0) {
      tab = s.d;
      n = s.n;
      return NRF_OK;
    }
  if (c->step_tables.size() >= STEP_TABLES_MAX) {
    HIP_TRY(hipDeviceSynchronize());  // nothing may still be reading the tables that go
    for (auto& s : c->step_tables) if (s.d) (void)hipFree(s.d);
    c->step_tables.clear();
  }
  std::vector<float> members((size_t)STEP_TABLE_CAPACITY);
  nrf_context::StepTable s;
  std::memcpy(s.key, key, sizeof(key));
  s.n = step_table(P.min_near, P.dt_gamma, c->dm.bound, c->dm.H, c->step_table_cap, members.data());
  if (s.n > 0) {
    HIP_TRY(hipMalloc((void**)&s.d, (size_t)s.n * 4));
    HIP_TRY(hipMemcpy(s.d, members.data(), (size_t)s.n * 4, hipMemcpyHostToDevice));
  }
  c->step_tables.push_back(s);  // (n == 0: these inputs have no table, remembered as well)
  tab = s.d;
  n = s.n;
#endif
  return NRF_OK;
}

// The grid side of the plan (nrf_grid_plan.h), decided without a device like plan_model (nrf_debug_grid_plan:
// tests/test_grid_plan_cpu.py): the march tables of a density grid, which of them are staged in LDS, and the workgroup that
// renders the frames beside them -- own / stage / gen_wave_bytes: plan_model's; gen_frag_bytes: DevModel's.
struct GridPlan {
  GridTables tables;
  GridFit fit;
};
GridPlan plan_grid(const nrf_model_desc& d, int own, int stage, uint32_t gen_wave_bytes, uint32_t gen_frag_bytes, bool allow_persistent,
                   bool allow_gen_wlds, const float* density_grid, float mean_density) {
  GridPlan g;
  g.tables = build_march_tables(d.density_grid_size, d.cascade, d.bound, d.aabb, density_grid, mean_density);
  const int form = march_form(d.density_grid_size, d.cascade, d.bound);
  auto candidate = [&](int net) {
    FitCandidate k{net, {render_persist_waves(net, form), 0}, {0u, 0u}, net == NET_GENERIC, net == NET_HOT};
    if (net == NET_GENERIC && k.waves[0] != 8) k.waves[1] = 8;
    for (int s = 0; s < 2; ++s) k.lds_bytes[s] = k.waves[s] ? (uint32_t)render_persistent_lds_bytes(net, k.waves[s], gen_wave_bytes) : 0u;
    return k;
  };
  FitInputs in{};
  in.coarse_words = g.tables.coarse.size();
  in.ctab_floats = g.tables.ctab.size();
  in.dilated_words = g.tables.dilated.size();
  in.own = candidate(own);
  in.stage = candidate(stage);
  in.stage_generic = stage == NET_GENERIC;
  in.stage_wide = stage == NET_WIDE;
  in.allow_persistent = allow_persistent;
  in.allow_gen_wlds = allow_gen_wlds;
  in.table_budget = (uint32_t)render_lds_table_max_bytes();
  in.strip_fixed_bytes = (uint32_t)render_strip_lds_fixed_bytes(stage, gen_wave_bytes);
  in.weight_area_bytes = (uint32_t)render_weight_area_bytes();
  in.staged_weight_bytes = (uint32_t)render_staged_weight_bytes(gen_frag_bytes);
  g.fit = fit_grid(in);
  return g;
}

// the plan's part of DevModel (the table pointers are the caller's)
void apply_grid_plan(DevModel& M, const GridPlan& g) {
  for (int i = 0; i < 6; ++i) M.occ_box[i] = g.tables.occ_box[i];
  M.coarse_shift = g.tables.coarse_shift;
  M.dilated_level_words = g.tables.dilated_level_words;
  M.lds_coarse_words = g.fit.lds_coarse_words;
  M.lds_ctab_floats = g.fit.lds_ctab_floats;
  M.lds_dilated_words = g.fit.persistent ? g.fit.lds_dilated_persist : g.fit.lds_dilated_strip;
  M.net = (uint32_t)g.fit.net;
  M.persistent = g.fit.persistent;
  M.persist_waves = g.fit.persist_waves;
  M.gen_weights_lds = g.fit.gen_weights_lds;
}

// Plans the march tables of a density grid (plan_grid) and uploads them.  Called by nrf_load_model with the snapshot's grid and
// by nrf_generate_density_grid with the one evaluated from the network.  Needs c->desc, c->dm.stage / gen_wave_bytes /
// gen_frag_bytes and c->own_net.
int set_density_grid(nrf_context* c, const float* density_grid, float mean_density) {
  HIP_TRY(hipDeviceSynchronize());  // nothing may still be marching on the old tables
  for (void** q : {&c->d_occ, &c->d_coarse, &c->d_ctab, &c->d_dilated}) {
    if (*q) (void)hipFree(*q);
    *q = nullptr;
  }
  DevModel& M = c->dm;
  const GridPlan g = plan_grid(c->desc, c->own_net, (int)M.stage, M.gen_wave_bytes, M.gen_frag_bytes, c->allow_persistent, c->allow_gen_wlds,
                               density_grid, mean_density);
  const GridTables& T = g.tables;
  auto upload = [&](void** dst, const void* src, size_t words) -> hipError_t {  // (a table the grid does not have stays null)
    if (words == 0) return hipSuccess;
    hipError_t e = hipMalloc(dst, words * 4);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(*dst, src, words * 4, hipMemcpyHostToDevice, c->stream);
  };
  const size_t n_words[4] = {T.occ.size(), T.coarse.size(), T.ctab.size(), T.dilated.size()};
  HIP_TRY(upload(&c->d_occ, T.occ.data(), n_words[0]));
  HIP_TRY(upload(&c->d_coarse, T.coarse.data(), n_words[1]));
  HIP_TRY(upload(&c->d_ctab, T.ctab.data(), n_words[2]));
  HIP_TRY(upload(&c->d_dilated, T.dilated.data(), n_words[3]));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipDeviceSynchronize());
  M.occ_bits = (const uint32_t*)c->d_occ;
  M.occ_coarse = (const uint32_t*)c->d_coarse;
  M.cell_bound = (const float*)c->d_ctab;
  M.occ_dilated = (const uint32_t*)c->d_dilated;
  M.n_cus = (uint32_t)c->n_cus;
  apply_grid_plan(M, g);
  c->fit = g.fit;
  std::copy(n_words, n_words + 4, c->table_words);
  c->desc.mean_density = mean_density;
  const uint64_t Hh = c->desc.density_grid_size;
  c->host_grid.assign(density_grid, density_grid + Hh * Hh * Hh * c->desc.cascade);
  return NRF_OK;
}

int need_model(nrf_context* c) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!c->model_loaded) return fail(NRF_E_STATE, "no model loaded (call nrf_load_model first)");
  return set_device(c);
}

}  // namespace

extern "C" {

const char* nrf_last_error(void) { return g_err.c_str(); }
void nrf_set_last_error_(const char* msg) { g_err = msg ? msg : ""; }  // used by nrf_renderbuffer.hip
int nrf_abi_version(void) { return NRF_ABI_VERSION; }

void nrf_default_options(nrf_options* o) {
  if (!o) return;
  o->bg_color = 1.0f;
  o->min_near = 0.2f;
  o->dt_gamma = 1.0f / 128.0f;
  o->max_steps = 1024;
  o->density_scale = 1.0f;
  o->perturb = 0;
  o->shard_index = 0;
  o->shard_count = 1;
  o->fast_interp = 0;
  o->tile_major = 0;
}

int nrf_level_table_compute(const nrf_model_desc* d, nrf_level_table* t) {
  if (!d || !t) return fail(NRF_E_INVALID, "null argument");
  const char* why = "";
  const int rc = compute_level_table(*d, *t, why);
  return rc ? fail(rc, why) : NRF_OK;
}

int nrf_expected_n_params(const nrf_model_desc* d, uint64_t* n) {
  if (!d || !n) return fail(NRF_E_INVALID, "null argument");
  nrf_level_table t;
  const char* why = "";
  int rc = compute_level_table(*d, t, why);
  if (!rc) rc = expected_params(*d, t, *n, why);
  return rc ? fail(rc, why) : NRF_OK;
}

int nrf_default_per_level_scale(float bound, uint32_t base_resolution, uint32_t n_levels, float* out) {
  if (!out || n_levels < 2 || base_resolution == 0) return fail(NRF_E_INVALID, "bad argument");
  const float desired_resolution = 2048.0f;  // R/src/nerf_render.cu:154-165
  *out = std::exp(std::log(desired_resolution * bound / (float)base_resolution) / (float)(n_levels - 1));
  return NRF_OK;
}

int nrf_tiles_per_shard(int width, int height, int shard_count, int* n) {
  if (!n || width <= 0 || height <= 0 || shard_count <= 0) return fail(NRF_E_INVALID, "bad argument");
  *n = tiles_per_shard(width, height, shard_count);
  return NRF_OK;
}

int nrf_create(int device, nrf_context** out) {
  if (!out) return fail(NRF_E_INVALID, "null argument");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(NRF_E_NODEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= count) return fail(NRF_E_NODEVICE, "device index out of range");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(NRF_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  nrf_context* c = new nrf_context;
  c->device = device;
  nrf_default_options(&c->opt);
  if (const char* e = std::getenv("NRF_MARCH_BUDGET")) {
    const int b = std::atoi(e);
    if (b >= 1 && b <= 4096) c->march_budget = b;
  }
  if (const char* e = std::getenv("NRF_SAMPLE_CAP")) { c->sample_cap = std::atoi(e); c->sample_cap_forced = true; }
  if (const char* e = std::getenv("NRF_PERSISTENT")) c->allow_persistent = std::atoi(e) != 0;
  if (const char* e = std::getenv("NRF_STEP_TABLE")) c->allow_step_table = std::atoi(e) != 0;
  if (const char* e = std::getenv("NRF_STEP_TABLE_CAP")) c->step_table_cap = std::max(2, std::min(std::atoi(e), (int)STEP_TABLE_CAPACITY));
  if (const char* e = std::getenv("NRF_GATHER_PLAN")) c->allow_gather_plan = std::atoi(e) != 0;
  if (const char* e = std::getenv("NRF_CENTRE_OUT")) c->centre_out = std::atoi(e) != 0;
  if (const char* e = std::getenv("NRF_GEN_WLDS")) c->allow_gen_wlds = std::atoi(e) != 0;
  if (const char* e = std::getenv("NRF_WIDTH_INSTANCES")) c->allow_width_instances = std::atoi(e) != 0;
  if (const char* e = std::getenv("NRF_QUEUE_CLASSES")) c->queue_classes = std::atoi(e);
  c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&c->ev0));
  HIP_TRY(hipEventCreate(&c->ev1));
  if (const char* e = std::getenv("NRF_HOST_PROGRESSIVE")) c->host_progressive = std::atoi(e) != 0;
  if (const char* e = std::getenv("NRF_HOST_MERGE")) c->host_merge = std::atoi(e) != 0;
  if (const char* e = std::getenv("NRF_HOST_SKIP_OUTSIDE")) c->host_skip_outside = std::atoi(e) != 0;
  if (const char* e = std::getenv("NRF_HOST_COLS")) c->host_cols = std::atoi(e) != 0;
  // The copy stream gets a hardware queue of its own.  HIP maps streams onto a few hardware queues (4 by default) and a
  // device-to-host copy issued while a render is resident on a queue it shares does not start before that render has
  // ended (scripts/copy_overlap_probe.py: a 133 MB copy issued 2 ms into a 14 ms render ended 2.3 ms after the render's
  // END; on a queue of its own it ran beside the render and ended 4.5 ms after its start).  Streams of another priority
  // come from another pool of hardware queues, whatever GPU_MAX_HW_QUEUES says.
  {
    int prio_lo = 0, prio_hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    HIP_TRY(hipStreamCreateWithPriority(&c->copy_stream, hipStreamNonBlocking, prio_hi));
  }
  for (auto& h : c->hs) {
    HIP_TRY(hipEventCreateWithFlags(&h.done, hipEventDisableTiming));
    for (hipEvent_t& g : h.grp) HIP_TRY(hipEventCreateWithFlags(&g, hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&h.t0));
    HIP_TRY(hipEventCreate(&h.t1));
  }
  if (const char* e = std::getenv("NRF_TAIL_SPLIT")) c->tail_split = std::atoi(e) != 0 ? 1 : 0;
  if (const char* e = std::getenv("NRF_MARCH_FF")) c->march_ff = std::atoi(e) != 0 ? 1 : 0;
  if (const char* e = std::getenv("NRF_GEN_FAST_GRID")) c->allow_gen_fast_grid = std::atoi(e) != 0;
  if (const char* e = std::getenv("NRF_QUAD_LEVELS")) c->quad_levels = std::atoi(e);
  if (const char* e = std::getenv("NRF_QUAD_BUDGET_MB")) c->quad_budget_mb = std::max(0, std::atoi(e));
  HIP_TRY(hipMalloc(&c->d_counters, CALL_RING * CALL_SLOT_BYTES));
  HIP_TRY(hipMemset(c->d_counters, 0, CALL_RING * CALL_SLOT_BYTES));
  if (const char* e = std::getenv("NRF_PLAN_MAX_POS")) c->plan_max_pos = std::max(0, std::min(std::atoi(e), (int)PLAN_CAP));
  HIP_TRY(hipMalloc(&c->d_plan, CALL_RING * PLAN_BYTES));
  HIP_TRY(hipMemset(c->d_plan, 0, CALL_RING * PLAN_BYTES));
  *out = c;
  return NRF_OK;
}

int nrf_destroy(nrf_context* c) {
  if (!c) return NRF_OK;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  free_model(c);
  free_frame(c);
  free_host_slots(c);
  free_mesh(c);
  for (auto& s : c->step_tables) if (s.d) (void)hipFree(s.d);
  for (auto& h : c->hs) {
    if (h.done) (void)hipEventDestroy(h.done);
    for (hipEvent_t g : h.grp) if (g) (void)hipEventDestroy(g);
    if (h.t0) (void)hipEventDestroy(h.t0);
    if (h.t1) (void)hipEventDestroy(h.t1);
  }
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  if (c->d_counters) (void)hipFree(c->d_counters);
  if (c->d_plan) (void)hipFree(c->d_plan);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return NRF_OK;
}

int nrf_load_model(nrf_context* c, const nrf_model_desc* d) {
  if (!c || !d || !d->params) return fail(NRF_E_INVALID, "null argument");
  if (d->abi_version != NRF_ABI_VERSION) return fail(NRF_E_INVALID, "abi_version mismatch");
  int rc = set_device(c);
  if (rc) return rc;
  {
    nrf_level_table lv;
    const char* why = "";
    rc = validate_model(*d, lv, why);
    if (rc) return fail(rc, why);
  }
  HIP_TRY(hipDeviceSynchronize());  // nothing may still be reading the old model
  free_model(c);
  // the budget of the quad copies: a sixteenth of the device's memory (MI355X: 18 GB), and no more than half of what is free --
  // QUAD_BUDGET_MB_DEFAULT when the device does not say; nrf_model_desc.gather_copy_budget_mb and NRF_QUAD_BUDGET_MB override it
  uint64_t budget_mb = QUAD_BUDGET_MB_DEFAULT;
  {
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess) budget_mb = std::min<uint64_t>((uint64_t)mem_total >> 24, (uint64_t)mem_free >> 21);
    else (void)hipGetLastError();
  }
  if (d->gather_copy_budget_mb) budget_mb = d->gather_copy_budget_mb;
  if (c->quad_budget_mb >= 0) budget_mb = (uint64_t)c->quad_budget_mb;
  ModelPlan p = plan_model(*d, c->allow_width_instances, budget_mb, c->quad_levels < 0 ? 4 : std::min(c->quad_levels, 16) / 4, c->allow_gather_plan);
  if (p.rc) return fail(p.rc, p.why);
  const ModelImage im = build_model_image(*d, p, c->allow_gen_fast_grid);
  // Uploads go through the context's own stream and the device is drained afterwards: the
  // render stream is non-blocking, so a NULL-stream hipMemcpy gives no ordering against it
  // (seen on MI355X as a few stale table entries in the first frame after a reload).
  auto upload = [&](void** dst, const void* src, size_t bytes) -> hipError_t {
    hipError_t e = hipMalloc(dst, bytes);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, c->stream);
  };
  if (hipMalloc(&c->d_grid, p.table_bytes) != hipSuccess) {  // no room for the copies: the reference-order table alone
    (void)hipGetLastError();
    c->d_grid = nullptr;
    p = drop_quads(p);
    HIP_TRY(hipMalloc(&c->d_grid, p.table_bytes));
  }
  HIP_TRY(hipMemcpyAsync(c->d_grid, im.grid16.data(), im.grid16.size() * 2, hipMemcpyHostToDevice, c->stream));
  for (uint32_t l = 0; l < d->n_levels; ++l) {  // the quad copies, from the table just uploaded (same stream)
    if (!((p.quad_mask >> l) & 1u)) continue;
    const LevelParams& Lv = p.lp[l];
    const uint64_t q_bytes = ((p.quad_far >> (l >> 2)) & 1u) ? (uint64_t)Lv.q_off_b << 4 : (uint64_t)Lv.q_off_b;
    HIP_TRY(launch_build_quads((const char*)c->d_grid + (size_t)Lv.offset * 4, Lv.res, Lv.size, Lv.mode == LV_HASH_POW2,
                               (char*)c->d_grid + q_bytes, c->stream));
  }
  HIP_TRY(upload(&c->d_wfrag, im.frags.data(), im.frags.size() * 2));
  if (p.stage != NET_HOT) HIP_TRY(upload(&c->d_gen, &im.gen, sizeof(im.gen)));
  if (p.stage == NET_WIDE) HIP_TRY(upload(&c->d_wfrag_gen, im.frags_gen.data(), im.frags_gen.size() * 2));
  if (p.own != p.stage) HIP_TRY(upload(&c->d_wfrag_hot, im.frags_hot.data(), im.frags_hot.size() * 2));
  HIP_TRY(upload(&c->d_lv, p.lp, sizeof(p.lp)));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipDeviceSynchronize());

  c->desc = *d;
  c->desc.params = nullptr;
  c->desc.density_grid = nullptr;
  c->lv = p.lv;
  DevModel& M = c->dm;
  fill_dev_model(M, *d, p);
  M.grid = (const uint32_t*)c->d_grid;
  M.wfrag = (const uint4*)c->d_wfrag;
  M.lv = (const LevelParams*)c->d_lv;
  M.gen = (const GenModel*)c->d_gen;
  M.wfrag_hot = (const uint4*)c->d_wfrag_hot;
  c->table_bytes = p.table_bytes;
  c->table_ref_bytes = p.table_ref_bytes;
  c->gather_addresses = 0;
  for (uint32_t l = 0; l < d->n_levels; ++l) c->gather_addresses += ((p.quad_mask >> l) & 1u) ? 2u : (d->interpolation == NRF_INTERP_NEAREST ? 1u : 8u);
  c->own_net = p.own;
  c->gen = im.gen;
  c->wfrag_bytes = im.frags.size() * 2;
  c->wfrag_gen_bytes = im.frags_gen.size() * 2;
  c->wfrag_hot_bytes = im.frags_hot.size() * 2;
  // the density grid of the snapshot (nerf_render.cu:447-466) -- or none yet: nrf_generate_density_grid evaluates it
  // from the network (NerfRender::generate_density_grid); until then the model cannot be rendered
  if (d->density_grid) {
    rc = set_density_grid(c, d->density_grid, d->mean_density);
    if (rc) { free_model(c); return rc; }
    c->grid_missing = false;
  } else {
    std::vector<float> empty((size_t)d->density_grid_size * d->density_grid_size * d->density_grid_size * d->cascade, 0.0f);
    rc = set_density_grid(c, empty.data(), d->mean_density);
    if (rc) { free_model(c); return rc; }
    c->grid_missing = true;
  }
  c->model_loaded = true;
  // the code objects of the render kernel's families are loaded here, not by the first frame (once per process and device)
  // (group members and server workers load models concurrently: one flag per device, taken under a lock)
  static std::once_flag preloaded[64];
  if (c->device >= 0 && c->device < 64) std::call_once(preloaded[c->device], [] { preload_kernels(true); });
  return NRF_OK;
}

// NerfRender::generate_density_grid (R/src/nerf_render.cu:388-429; dead and incomplete in the reference: the density
// query is commented out at :415).  What it sets out to do (torch-ngp's update_extra_state, which it restates), made
// whole: for every cascade the density at every cell's position (init_xyzs + dd_scale, perturbation off), scaled by
// 0.001691, folded into a grid that starts at 1/64 with g = max(g * decay, value), n_iterations times; mean_density =
// mean of max(g, 0).  The march tables are rebuilt from the result.
int nrf_generate_density_grid(nrf_context* c, int n_iterations, float decay, float* mean_density_out) {
  int rc = need_model(c);
  if (rc) return rc;
  if (n_iterations < 1 || !(decay > 0.0f) || !(decay <= 1.0f)) return fail(NRF_E_INVALID, "n_iterations >= 1 and 0 < decay <= 1 required");
  const uint32_t H = c->desc.density_grid_size, C = c->desc.cascade;
  const uint64_t n = (uint64_t)H * H * H;
  if (n >= (1ull << 31)) return fail(NRF_E_UNSUPPORTED, "density grid too large");
  void* buf = nullptr;  // xyz [n][3] | dir [n][3] | rgb [n][3] | sigma [n] | grid [n]
  HIP_TRY(hipMalloc(&buf, n * 11 * sizeof(float)));
  float* d_xyz = (float*)buf;
  float* d_dir = d_xyz + 3 * n;
  float* d_rgb = d_dir + 3 * n;
  float* d_sigma = d_rgb + 3 * n;
  float* d_cell = d_sigma + n;
  std::vector<float> grid((size_t)n * C);
  hipError_t e = hipSuccess;
  for (uint32_t cas = 0; cas < C && e == hipSuccess; ++cas) {
    const float bound = (float)(1u << cas) < c->desc.bound ? (float)(1u << cas) : c->desc.bound;  // nerf_render.cu:409
    const float half_grid_size = bound / (float)H;
    e = launch_density_positions(H, bound - half_grid_size, d_xyz, d_dir, c->stream);
    if (e == hipSuccess) e = launch_network(c->dm, d_xyz, d_dir, (uint32_t)n, d_sigma, d_rgb, c->stream);
    if (e == hipSuccess) e = launch_density_update(d_sigma, (uint32_t)n, decay, n_iterations, d_cell, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(grid.data() + (size_t)cas * n, d_cell, n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  (void)hipFree(buf);
  if (e != hipSuccess) return hip_fail(e, "nrf_generate_density_grid");
  double sum = 0.0;  // sequential, in cell order: the same number on every run (and in the oracle)
  for (float g : grid) sum += g > 0.0f ? (double)g : 0.0;
  const float mean = (float)(sum / (double)grid.size());
  rc = set_density_grid(c, grid.data(), mean);
  if (rc) return rc;
  c->grid_missing = false;
  if (mean_density_out) *mean_density_out = mean;
  return NRF_OK;
}

int nrf_read_density_grid(nrf_context* c, float* grid, uint64_t n, float* mean_density) {
  int rc = need_model(c);
  if (rc) return rc;
  if (grid) {
    if (n != c->host_grid.size()) return fail(NRF_E_INVALID, "n must be cascade * H^3");
    std::memcpy(grid, c->host_grid.data(), c->host_grid.size() * sizeof(float));
  }
  if (mean_density) *mean_density = c->desc.mean_density;
  return NRF_OK;
}

int nrf_set_resolution(nrf_context* c, int width, int height) {
  if (!c || width <= 0 || height <= 0) return fail(NRF_E_INVALID, "bad resolution");
  int rc = set_device(c);
  if (rc) return rc;
  c->W = width;
  c->H = height;
  return alloc_frame(c);
}

int nrf_set_options(nrf_context* c, const nrf_options* o) {
  if (!c || !o) return fail(NRF_E_INVALID, "null argument");
  if (o->shard_count < 1 || o->shard_index < 0 || o->shard_index >= o->shard_count)
    return fail(NRF_E_INVALID, "bad shard");
  if (o->perturb < 0) return fail(NRF_E_INVALID, "perturb must be >= 0 (0: off, the reference's m_perturb = false; > 0: the seed, render_utils.h:550)");
  if (o->max_steps < 1) return fail(NRF_E_INVALID, "max_steps must be >= 1");
  int rc = set_device(c);
  if (rc) return rc;
  c->opt = *o;
  return alloc_frame(c);
}

int nrf_set_max_views(nrf_context* c, int max_views) {
  if (!c || max_views < 1) return fail(NRF_E_INVALID, "max_views must be >= 1");
  int rc = set_device(c);
  if (rc) return rc;
  c->max_views = max_views;
  return alloc_frame(c);
}

}  // extern "C"

namespace {
// One launch per NRF_MAX_VIEWS cameras; all launches of a call go to the same stream back to back.  Every call takes the
// next slot of the context's ring of statistics counters + work queues (cleared on the call's own stream), so calls of
// one context that overlap on different streams never share a queue.
// rows_out (optional): per view the rows [lo, hi) and the columns [x0, x1) (whole tiles) its region of interest covers.
// (MAX_CAMERA_DISTANCE, and the guard of caller-supplied rays beside it: nrf_device.h)
struct ProgressArgs {
  unsigned* done;   // device [n_views][tiles_y], zeroed on the stream before the launches
  unsigned* flags;  // pinned host [n_views][tiles_y]
  unsigned epoch;
};
// rays (nrf_render_rays): the views' rays come from the caller's arrays -- cams / poses are null, every view's region of interest
// is its whole frame, and the launch is neither planned (there is no camera to price strips from) nor a host frame.
struct RayArgs {
  const float *o, *d;  // device [n_views][per_view][3]
  uint64_t per_view;
  // nrf_render_rays_clipped (nullptr / 0: nrf_render_rays): per-ray limits of t [n_views][per_view], per-ray background [..][3], nrf_rays.flags
  const float *t_min = nullptr, *t_max = nullptr, *background = nullptr;
  uint32_t flags = 0;
  float hit_opacity = 0.f;  // nrf_ray_hits: > 0 = the launch is a hit launch with this threshold (0: every other call)
};
// The model as the RAYS instances see it: the persistent form for the hot shape only (GridFit::rays_persistent); the per-strip
// kernel borrows the weight area for the dilated table, so it is given what fits there (GridFit::lds_dilated_strip)
DevModel rays_model(const nrf_context* c) {
  DevModel m = c->dm;
  if (!c->fit.rays_persistent) {
    m.persistent = 0;
    m.net = m.stage;
    m.lds_dilated_words = c->fit.lds_dilated_strip;
  }
  return m;
}
int render_views_impl(nrf_context* c, int n_views, const float* cams, const float* poses, hipStream_t st, void* rgba, void* depth,
                      size_t stride_px, int out_mode, int skip_outside, int* rows_out, const ProgressArgs* prog = nullptr,
                      const RayArgs* rays = nullptr) {
  FrameParams P;
  static const float unit_cam[4] = {1.f, 1.f, 0.f, 0.f};
  static const float unit_pose[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  fill_frame_params(c, rays ? unit_cam : cams, rays ? unit_pose : poses, P);
  if (rays) P.fast_interp = 0;
  const DevModel dm = rays ? rays_model(c) : c->dm;
  P.out_mode = out_mode;
  P.skip_outside = skip_outside;
  if (drops_sample_cap(c->n_local_tiles, n_views, (int)dm.n_cus, dm.persist_waves, c->sample_cap_forced)) P.sample_cap = 0;  // (nrf_frame_plan.h)
  c->call_index = (c->call_index + 1) % CALL_RING;
  char* counters = call_slot(c, c->call_index);
  unsigned* plan = (c->plan_max_pos > 0 && prog == nullptr && rays == nullptr) ? (unsigned*)((char*)c->d_plan + (size_t)c->call_index * PLAN_BYTES) : nullptr;
  const float* step_tab = nullptr;
  int step_n = 0;
  if (P.march_ff != 0) {  // (the fast-forward is the table's only reader)
    const int rc = step_table_for(c, P, step_tab, step_n);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(c->ev0, st));  // (render_ms covers the clearing of the call's counters and the planning of its queues)
  const int per_launch = views_per_launch(P.tiles_x, P.tiles_y, MAX_VIEWS);  // NRF_MAX_VIEWS, fewer for frames beyond 8K
  const size_t px_bytes_a = out_mode == OUT_U8 ? 3 : 16, px_bytes_b = out_mode == OUT_U8 ? 1 : 4;
  for (int first = 0; first < n_views; first += per_launch) {
    ViewBatch VB;
    std::memset(&VB, 0, sizeof(VB));
    VB.n_views = n_views - first < per_launch ? n_views - first : per_launch;
    VB.view_stride_px = stride_px;
    for (int v = 0; rays && v < VB.n_views; ++v) {  // (R, org, cam stay zero: no RAYS instance reads them)
      VB.v[v].roi[0] = VB.v[v].roi[1] = 0;
      VB.v[v].roi[2] = c->W - 1;
      VB.v[v].roi[3] = c->H - 1;
    }
    if (rays) {
      P.rays_o = rays->o + 3 * (size_t)first * rays->per_view;
      P.rays_d = rays->d + 3 * (size_t)first * rays->per_view;
      P.rays_per_view = (unsigned)rays->per_view;
      P.ray_tmin = rays->t_min ? rays->t_min + (size_t)first * rays->per_view : nullptr;
      P.ray_tmax = rays->t_max ? rays->t_max + (size_t)first * rays->per_view : nullptr;
      P.ray_bg = rays->background ? rays->background + 3 * (size_t)first * rays->per_view : nullptr;
      P.ray_flags = rays->flags;
      if (rays->hit_opacity > 0.f) {  // nrf_ray_hits: the RAYS_HIT instances; no background takes part, a pixel nobody renders is zero
        P.ray_flags = RAY_FLAG_HIT | RAY_FLAG_DEPTH_T;
        P.hit_opacity = rays->hit_opacity;
        P.hit_exp = hit_cap_exponent(rays->hit_opacity);  // (nrf_frame_plan.h)
        P.bg_color = 0.f;
      }
    }
    for (int v = 0; !rays && v < VB.n_views; ++v) {
      nerf_matrix_to_ngp(poses + 16 * (size_t)(first + v), c->desc.scale, VB.v[v].R, VB.v[v].org);
      for (int i = 0; i < 4; ++i) VB.v[v].cam[i] = cams[4 * (size_t)(first + v) + i];
      view_roi(VB.v[v].R, VB.v[v].org, VB.v[v].cam, c->dm.occ_box, c->W, c->H, VB.v[v].roi);
      far_camera_roi(VB.v[v].org, MAX_CAMERA_DISTANCE, VB.v[v].roi);
      if (rows_out) {  // {row lo, row hi, column lo, column hi} per view
        int* ro = rows_out + 4 * (size_t)(first + v);
        roi_rows(VB.v[v].roi, c->H, ro[0], ro[1]);
        roi_cols(VB.v[v].roi, c->W, ro[2], ro[3]);
      }
    }
    if (prog) {  // (the kernel indexes its progress arrays by the launch's own view numbers)
      P.prog_done = prog->done + (size_t)first * P.tiles_y;
      P.prog_flags = prog->flags + (size_t)first * P.tiles_y;
      P.prog_epoch = (int)prog->epoch;
    }
    HIP_TRY(launch_render(dm, P, VB, rgba ? (char*)rgba + (size_t)first * stride_px * px_bytes_a : nullptr,
                          (char*)depth + (size_t)first * stride_px * px_bytes_b, counters, st, first == 0, plan,
                          (unsigned)c->plan_max_pos, step_tab, step_n));
  }
  c->last_views = n_views;
  HIP_TRY(hipEventRecord(c->ev1, st));
  c->last_stream = st;
  c->rendered = true;
  return NRF_OK;
}

int check_renderable(nrf_context* c, const float* cams, const float* poses, int n_views) {
  int rc = need_model(c);
  if (rc) return rc;
  if (!cams || !poses) return fail(NRF_E_INVALID, "null argument");
  if (n_views < 1) return fail(NRF_E_INVALID, "n_views must be >= 1");
  if (c->W <= 0 || !c->d_rgba) return fail(NRF_E_STATE, "set_resolution has not been called");
  if (c->grid_missing)
    return fail(NRF_E_STATE, "the model was loaded without a density grid: call nrf_generate_density_grid first");
  return NRF_OK;
}
}  // namespace

extern "C" {

// nrf_render_views and nrf_render_rays behind their argument checks (rays == nullptr: cameras)
static int render_frames(nrf_context* c, int n_views, const float* cams, const float* poses, const RayArgs* rays, void* stream, nrf_frame* out) {
  int rc = NRF_OK;
  const bool bound = c->bound_rgba || c->bound_rgbd8 || c->bound_rgb8;
  if (!bound && n_views > c->max_views)
    return fail(NRF_E_STATE, "more views than the context's buffers hold: call nrf_set_max_views or nrf_bind_output");
  if (c->bound_rgb8 && tiled_layout(c))
    return fail(NRF_E_STATE, "8-bit planar output (nrf_bind_output_u8) needs a single-shard (row-major) frame");
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  void* rgba = c->bound_rgba ? c->bound_rgba : c->d_rgba;
  void* depth = c->bound_depth ? c->bound_depth : c->d_depth;
  int mode = OUT_F32;
  if (c->bound_rgbd8) {  // 4 bytes per pixel where the depth plane would be (store_pixel)
    rgba = nullptr;
    depth = c->bound_rgbd8;
    mode = OUT_RGBD8;
  } else if (c->bound_rgb8) {
    rgba = c->bound_rgb8;
    depth = c->bound_depth8;
    mode = OUT_U8;
  }
  rc = render_views_impl(c, n_views, cams, poses, st, rgba, depth, c->n_out_px, mode, 0, nullptr, nullptr, rays);
  if (rc) return rc;
  const bool floats = mode == OUT_F32;
  c->last_rgba = floats ? rgba : nullptr;  // (an 8-bit frame in a bound buffer is the caller's to read)
  c->last_depth = floats ? depth : nullptr;
  if (!stream) HIP_TRY(hipStreamSynchronize(st));
  if (out) {
    out->width = c->W;
    out->height = c->H;
    out->n_tiles = c->n_local_tiles;
    out->rgba = floats ? rgba : nullptr;
    out->depth = floats ? depth : nullptr;
    out->tile_major = tiled_layout(c);
    out->n_views = n_views;
    out->view_stride_px = (int64_t)c->n_out_px;
  }
  return NRF_OK;
}

int nrf_render_views(nrf_context* c, int n_views, const float* cams, const float* poses, void* stream, nrf_frame* out) {
  int rc = check_renderable(c, cams, poses, n_views);
  if (rc) return rc;
  return render_frames(c, n_views, cams, poses, nullptr, stream, out);
}

int nrf_render_rays_clipped(nrf_context* c, int n_views, const nrf_rays* r, void* stream, nrf_frame* out) {
  static const float none[16] = {};  // (check_renderable's null test is for cameras)
  int rc = check_renderable(c, none, none, n_views);
  if (rc) return rc;
  if (!r || !r->rays_o || !r->rays_d) return fail(NRF_E_INVALID, "null argument");
  if (r->reserved != 0 || (r->flags & ~(uint32_t)(NRF_RAYS_DEPTH_T | NRF_RAYS_DENSITY_ONLY)) != 0)
    return fail(NRF_E_INVALID, "nrf_rays: reserved must be 0 and flags may hold NRF_RAYS_DEPTH_T and NRF_RAYS_DENSITY_ONLY only");
  if (r->rays_per_view < 1 || r->rays_per_view > (uint64_t)c->W * (uint64_t)c->H)
    return fail(NRF_E_INVALID, "rays_per_view must be 1 .. width * height of nrf_set_resolution");
  if (c->opt.perturb > 0) return fail(NRF_E_UNSUPPORTED, "nrf_render_rays has no perturb instances (nrf_options.perturb must be 0)");
  if ((r->flags & NRF_RAYS_DEPTH_T) && (c->bound_rgbd8 || c->bound_rgb8))
    return fail(NRF_E_UNSUPPORTED, "NRF_RAYS_DEPTH_T needs a float depth plane: an 8-bit output is bound");
  if ((r->flags & NRF_RAYS_DENSITY_ONLY) && (c->bound_rgbd8 || c->bound_rgb8))
    return fail(NRF_E_UNSUPPORTED, "NRF_RAYS_DENSITY_ONLY needs float planes: an 8-bit output is bound");
  RayArgs rays{(const float*)r->rays_o, (const float*)r->rays_d, r->rays_per_view};
  rays.t_min = (const float*)r->t_min;
  rays.t_max = (const float*)r->t_max;
  rays.background = (const float*)r->background;
  rays.flags = r->flags;
  return render_frames(c, n_views, nullptr, nullptr, &rays, stream, out);
}

int nrf_ray_hits(nrf_context* c, int n_views, const nrf_rays* r, float opacity, void* stream, nrf_frame* out) {
  static const float none[16] = {};
  int rc = check_renderable(c, none, none, n_views);
  if (rc) return rc;
  if (!r || !r->rays_o || !r->rays_d) return fail(NRF_E_INVALID, "null argument");
  if (r->reserved != 0 || r->flags != 0 || r->background != nullptr)
    return fail(NRF_E_INVALID, "nrf_ray_hits: nrf_rays.flags and reserved must be 0 and background NULL");
  if (!(opacity > 0.0f && opacity <= 1.0f)) return fail(NRF_E_INVALID, "nrf_ray_hits: opacity must be in (0, 1]");  // (NaN fails both)
  if (r->rays_per_view < 1 || r->rays_per_view > (uint64_t)c->W * (uint64_t)c->H)
    return fail(NRF_E_INVALID, "rays_per_view must be 1 .. width * height of nrf_set_resolution");
  if (c->opt.perturb > 0) return fail(NRF_E_UNSUPPORTED, "nrf_render_rays has no perturb instances (nrf_options.perturb must be 0)");
  if (c->bound_rgbd8 || c->bound_rgb8) return fail(NRF_E_UNSUPPORTED, "nrf_ray_hits needs float planes: an 8-bit output is bound");
  RayArgs rays{(const float*)r->rays_o, (const float*)r->rays_d, r->rays_per_view};
  rays.t_min = (const float*)r->t_min;
  rays.t_max = (const float*)r->t_max;
  rays.hit_opacity = opacity;
  return render_frames(c, n_views, nullptr, nullptr, &rays, stream, out);
}

int nrf_render_rays(nrf_context* c, int n_views, const void* rays_o, const void* rays_d, uint64_t rays_per_view, void* stream,
                    nrf_frame* out) {
  nrf_rays r;  // no limits, the scalar background, normalised depth
  std::memset(&r, 0, sizeof(r));
  r.rays_o = rays_o;
  r.rays_d = rays_d;
  r.rays_per_view = rays_per_view;
  return nrf_render_rays_clipped(c, n_views, &r, stream, out);
}

// ---- host frames: the reference's render_frame ends in HOST memory (R/src/nerf_render.cu:345-359: D2H of the float
// planes, then a single-threaded quantise / de-interleave loop per GPU).  Here the kernel writes the 8-bit Image itself
// (OUT_U8), the rows of the view's region of interest travel by one asynchronous copy per plane into pinned memory the
// context owns, and the rows outside it -- background by construction -- are filled by the calling thread while the GPU
// renders (only those that held something else: a camera that moves a little costs a few rows).  Two slots: the copy of
// one call overlaps the render of the next.
namespace {
// copies the rows [lo, hi) of view v of a host-frame slot (both planes) on the context's copy stream; x0 < x1: only the
// columns [x0, x1) of those rows (a pitched copy: scripts/copy2d_probe.py measured 46.5 GB/s for 80 % of a 1080p frame's width
// against 49.1 GB/s for whole rows -- 0.85 of the time)
int copy_rows(nrf_context* c, nrf_context::HostSlot& h, int v, int lo, int hi, int x0 = 0, int x1 = 0) {
  if (hi <= lo) return NRF_OK;
  const RowCopy k = row_copy(h.W, h.px, h.views, v, lo, hi, x0, x1);
  const uint8_t* d_buf = (const uint8_t*)h.d_buf;
  for (const PlaneCopy* p : {&k.rgb, &k.depth}) {
    if (p == &k.depth && !h.with_depth) break;
    if (k.pitched) HIP_TRY(hipMemcpy2DAsync(h.h_buf + p->off, p->pitch, d_buf + p->off, p->pitch, p->width, p->rows, hipMemcpyDeviceToHost, c->copy_stream));
    else HIP_TRY(hipMemcpyAsync(h.h_buf + p->off, d_buf + p->off, p->width, hipMemcpyDeviceToHost, c->copy_stream));
    h.copied += p->bytes();
  }
  return NRF_OK;
}

// The copies of a progressive call, issued by the waiting thread while the render is still running: a band of strip rows
// goes to the copy engine as soon as the kernel has flagged all of its rows (the bytes are in memory by then: write-through
// stores, acknowledged before the row was counted -- nrf_render.h tile_written); whatever is left when the kernel's end
// event fires is copied then.  The loop ends with the kernel at the latest: it cannot wait for a flag that never comes.
int progressive_copies(nrf_context* c, nrf_context::HostSlot& h) {
  std::vector<Band> bands = plan_bands(h.W, h.with_depth, h.n_views, h.rows.data());  // (nrf_frame_plan.h)
  const int tiles_y = tiles_of(h.H);
  // A copy costs the engine ~12 us before its first byte moves (a 550 KB band: 34 us for 10 us of link time), and the rows of
  // a frame rendered alone complete within the last tenth of its render: band by band the copies ran for 0.3 ms after the
  // kernel's end.  So ready bands are issued in GROUPS: adjacent ones merged into one copy per plane, at most two groups in
  // flight -- while the engine is busy the ready bands collect, and what completes together leaves as one copy.
  size_t remaining = bands.size();
  bool kernel_done = false;
  unsigned spins = 0;
  static const bool debug = std::getenv("NRF_HOST_DEBUG") != nullptr;
  std::vector<hipEvent_t> dbg_events;
  const auto t_begin = std::chrono::steady_clock::now();
  auto since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
  std::vector<char> ready(bands.size(), 0);
  size_t n_ready = 0;     // ready, not yet issued
  int in_flight = 0;      // groups whose event has not been seen done (oldest: grp[(grp_next + 2 - in_flight) % 2])
  int grp_next = 0;
  const int max_groups = c->host_merge ? 2 : 1 << 30;
  while (remaining) {
    if (!kernel_done) {
      for (size_t i = 0; i < bands.size(); ++i) {
        const Band& b = bands[i];
        if (b.view < 0 || ready[i]) continue;
        bool ok = true;
        const unsigned* f = h.h_flags + (size_t)b.view * tiles_y;
        for (int r = b.s0; r < b.s1 && ok; ++r) ok = __atomic_load_n(f + r, __ATOMIC_ACQUIRE) == h.epoch;
        if (ok) { ready[i] = 1; ++n_ready; }
      }
    } else if (n_ready < remaining) {
      for (size_t i = 0; i < bands.size(); ++i) if (bands[i].view >= 0 && !ready[i]) { ready[i] = 1; ++n_ready; }
    }
    while (in_flight > 0 && c->host_merge) {
      const hipError_t e = hipEventQuery(h.grp[(grp_next + 2 - in_flight) % 2]);
      if (e == hipSuccess) --in_flight;
      else if (e == hipErrorNotReady) break;
      else return hip_fail(e, "hipEventQuery");
    }
    if (n_ready && in_flight < max_groups) {
      for (size_t i = 0; i < bands.size();) {
        if (bands[i].view < 0 || !ready[i]) { ++i; continue; }
        size_t j = i;  // [i, j]: ready bands of one view whose rows follow each other
        while (c->host_merge && j + 1 < bands.size() && bands[j + 1].view == bands[i].view && ready[j + 1] && bands[j + 1].s0 == bands[j].s1) ++j;
        if (debug) std::fprintf(stderr, "[host frame] +%.3f ms: view %d rows %d..%d (%zu band(s))%s\n", since(), bands[i].view, bands[i].lo, bands[j].hi, j - i + 1, kernel_done ? " (kernel done)" : "");
        hipEvent_t d0 = nullptr, d1 = nullptr;
        if (debug) { (void)hipEventCreate(&d0); (void)hipEventCreate(&d1); (void)hipEventRecord(d0, c->copy_stream); }
        int rc = copy_rows(c, h, bands[i].view, bands[i].lo, bands[j].hi);
        if (rc) return rc;
        if (debug) { (void)hipEventRecord(d1, c->copy_stream); dbg_events.push_back(d0); dbg_events.push_back(d1); }
        for (size_t k = i; k <= j; ++k) { bands[k].view = -1; ready[k] = 0; --remaining; --n_ready; }
        i = j + 1;
      }
      if (c->host_merge && remaining) {
        HIP_TRY(hipEventRecord(h.grp[grp_next], c->copy_stream));
        grp_next ^= 1;
        ++in_flight;
      }
      continue;
    }
    if (!remaining) break;
    if (!kernel_done && (++spins & 31u) == 0u) {
      const hipError_t e = hipEventQuery(h.t1);
      if (e == hipSuccess) kernel_done = true;
      else if (e != hipErrorNotReady) return hip_fail(e, "hipEventQuery");
    } else {
      __builtin_ia32_pause();
    }
  }
  HIP_TRY(hipEventRecord(h.done, c->copy_stream));
  h.copies_issued = true;
  if (debug) {  // when the copy engine really moved each band, relative to the start of the render
    (void)hipEventSynchronize(h.done);
    for (size_t i = 0; i + 1 < dbg_events.size(); i += 2) {
      float a = 0.f, b = 0.f;
      (void)hipEventElapsedTime(&a, h.t0, dbg_events[i]);
      (void)hipEventElapsedTime(&b, h.t0, dbg_events[i + 1]);
      std::fprintf(stderr, "[host frame] copy %zu ran %.3f .. %.3f ms after the render's start\n", i / 2, a, b);
      (void)hipEventDestroy(dbg_events[i]);
      (void)hipEventDestroy(dbg_events[i + 1]);
    }
  }
  return NRF_OK;
}
}  // namespace

int nrf_submit_host_u8(nrf_context* c, int n_views, const float* cams, const float* poses, int flags, int* ticket) {
  int rc = check_renderable(c, cams, poses, n_views);
  if (rc) return rc;
  if (!ticket) return fail(NRF_E_INVALID, "null argument");
  if (tiled_layout(c)) return fail(NRF_E_STATE, "host frames need a single-shard (row-major) frame");
  const int si = c->hs_next;
  nrf_context::HostSlot& h = c->hs[si];
  // the slot's previous frames are overwritten (nerfhip.h: valid until the second next submit); a call nobody waited for
  // has no copy in flight -- its render precedes this one on the context's stream
  if (h.pending && h.copies_issued) HIP_TRY(hipEventSynchronize(h.done));
  h.pending = false;
  const size_t px = (size_t)c->W * c->H;
  const int tiles_y = tiles_of(c->H);
  // keyed on the frame's GEOMETRY, not its pixel count: 1920x1080 -> 1080x1920 keeps W * H but changes the row bookkeeping
  // (row_lo / row_hi / bg describe byte ranges of the old width) and the number of strip rows (d_done / h_flags entries)
  if (h.px != px || h.W != c->W || h.H != c->H || h.views < (size_t)n_views) {
    HIP_TRY(hipDeviceSynchronize());
    for (void* q : {h.d_buf, (void*)h.d_done}) if (q) (void)hipFree(q);
    for (void* q : {(void*)h.h_buf, (void*)h.h_flags}) if (q) (void)hipHostFree(q);
    h.d_buf = nullptr;
    h.h_buf = nullptr;
    h.d_done = h.h_flags = nullptr;
    h.views = std::max((size_t)n_views, (size_t)c->max_views);
    h.px = px;
    h.prog_entries = h.views * (size_t)tiles_y;
    void* hp = nullptr;
    HIP_TRY(hipHostMalloc(&hp, h.views * px * 4, hipHostMallocPortable));
    h.h_buf = (uint8_t*)hp;
    HIP_TRY(hipMalloc(&h.d_buf, h.views * px * 4));
    HIP_TRY(hipMalloc((void**)&h.d_done, h.prog_entries * 4));
    HIP_TRY(hipHostMalloc(&hp, h.prog_entries * 4, hipHostMallocPortable | hipHostMallocMapped));
    h.h_flags = (unsigned*)hp;
    std::memset(h.h_flags, 0, h.prog_entries * 4);
    h.epoch = 0;
    h.row_lo.assign(h.views, 0);
    h.row_hi.assign(h.views, c->H);  // unknown content: everything counts as "not background"
    h.col_lo.assign(h.views, 0);
    h.col_hi.assign(h.views, c->W);
    h.bg = -1;
  }
  h.W = c->W;
  h.H = c->H;
  h.n_views = n_views;
  h.with_depth = !(flags & NRF_HOST_RGB_ONLY);
  h.copied = 0;
  h.copies_issued = false;
  // progress reporting needs the persistent form of the kernel (launch_render's choice for this model)
  // ... and a frame rendered alone, whose launch is planned, copies after its render (nrf_frame_plan.h)
  h.progressive = host_frame_progressive(c->host_progressive && c->dm.persistent && c->dm.lds_coarse_words > 0, n_views, c->W, tiles_y, c->plan_max_pos);
  const size_t depth_off = h.views * px * 3;  // depth planes follow the rgb planes of ALL views the slot holds
  h.rows.assign((size_t)4 * n_views, 0);
  ProgressArgs prog{h.d_done, h.h_flags, 0u};
  if (h.progressive) {
    prog.epoch = ++h.epoch;
    HIP_TRY(hipMemsetAsync(h.d_done, 0, (size_t)n_views * tiles_y * 4, c->stream));
  }
  HIP_TRY(hipEventRecord(h.t0, c->stream));
  rc = render_views_impl(c, n_views, cams, poses, c->stream, h.d_buf, (uint8_t*)h.d_buf + depth_off, px, OUT_U8, c->host_skip_outside ? 1 : 0, h.rows.data(),
                         h.progressive ? &prog : nullptr);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(h.t1, c->stream));
  c->last_rgba = c->last_depth = nullptr;
  if (!h.progressive) {  // every copy after the render's end
    HIP_TRY(hipStreamWaitEvent(c->copy_stream, h.t1, 0));
    for (int v = 0; v < n_views; ++v) {
      // (the copies of a call that is not progressive start after the render: only the region's columns travel.  Progressive
      //  copies run BESIDE the render, where a pitched copy the runtime chose to move with a blit kernel would find no compute
      //  unit free -- they keep whole rows)
      rc = copy_rows(c, h, v, h.rows[4 * v], h.rows[4 * v + 1], c->host_cols ? h.rows[4 * v + 2] : 0, c->host_cols ? h.rows[4 * v + 3] : 0);
      if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(h.done, c->copy_stream));
    h.copies_issued = true;
  }
  // while the GPU works: the pixels outside the regions of interest.  The pinned planes hold the background value except in
  // the rectangle the copies of earlier calls have written (row_lo / row_hi x col_lo / col_hi), so only that rectangle's
  // difference to the new one is filled.
  {
    const int bg = host_quant_u8(c->opt.bg_color);
    const bool all = h.bg != bg;
    const size_t Wb = (size_t)c->W;
    auto fill = [&](int v, int r0, int r1, int c0, int c1) {
      if (c0 == 0 && c1 == c->W) {
        std::memset(h.h_buf + ((size_t)v * px + (size_t)r0 * Wb) * 3, bg, (size_t)(r1 - r0) * Wb * 3);
        std::memset(h.h_buf + depth_off + (size_t)v * px + (size_t)r0 * Wb, 0, (size_t)(r1 - r0) * Wb);  // depth of a missed ray: 0
        return;
      }
      for (int r = r0; r < r1; ++r) {
        std::memset(h.h_buf + ((size_t)v * px + (size_t)r * Wb + (size_t)c0) * 3, bg, (size_t)(c1 - c0) * 3);
        std::memset(h.h_buf + depth_off + (size_t)v * px + (size_t)r * Wb + (size_t)c0, 0, (size_t)(c1 - c0));
      }
    };
    const bool use_cols = c->host_cols && !h.progressive;  // (what this call's copies write: the region's columns, or whole rows)
    for (int v = 0; v < (int)h.views; ++v) {
      if (v < n_views) {
        const FillPlan F = fill_rects({h.row_lo[v], h.row_hi[v], h.col_lo[v], h.col_hi[v]}, all, c->W, c->H, &h.rows[4 * v], use_cols);
        for (int i = 0; i < F.n; ++i) fill(v, F.rects[i].r0, F.rects[i].r1, F.rects[i].c0, F.rects[i].c1);
        h.row_lo[v] = F.now.r0;
        h.row_hi[v] = F.now.r1;
        h.col_lo[v] = F.now.c0;
        h.col_hi[v] = F.now.c1;
      } else if (all) {  // (not part of this call: stays as it is, counted as unknown)
        h.row_lo[v] = 0;
        h.row_hi[v] = c->H;
        h.col_lo[v] = 0;
        h.col_hi[v] = c->W;
      }
    }
    h.bg = bg;
  }
  h.pending = true;
  c->hs_next = (si + 1) % HOST_SLOTS;
  *ticket = si;
  return NRF_OK;
}

int nrf_wait_host_u8(nrf_context* c, int ticket, nrf_host_frame* out) {
  if (!c || ticket < 0 || ticket >= HOST_SLOTS) return fail(NRF_E_INVALID, "bad ticket");
  nrf_context::HostSlot& h = c->hs[ticket];
  if (!h.h_buf || h.n_views < 1) return fail(NRF_E_STATE, "nothing was submitted with this ticket");
  int rc = set_device(c);
  if (rc) return rc;
  if (h.pending) {
    if (!h.copies_issued) {
      rc = progressive_copies(c, h);
      if (rc) return rc;
    }
    // the last copy is a few tens of microseconds away: poll before blocking
    hipError_t e = hipErrorNotReady;
    for (int i = 0; i < 4000 && e == hipErrorNotReady; ++i) e = hipEventQuery(h.done);
    if (e == hipErrorNotReady) e = hipEventSynchronize(h.done);
    if (e != hipSuccess) return hip_fail(e, "waiting for the host frame's copies");
  }
  h.pending = false;
  if (out) {
    out->width = h.W;
    out->height = h.H;
    out->n_views = h.n_views;
    out->rgb = h.h_buf;
    out->depth = h.with_depth ? h.h_buf + h.views * h.px * 3 : nullptr;
    out->view_stride_px = (int64_t)h.px;
    out->render_ms = 0.f;
    out->copied_bytes = h.copied;
    (void)hipEventElapsedTime(&out->render_ms, h.t0, h.t1);
  }
  return NRF_OK;
}

int nrf_render_host_u8(nrf_context* c, int n_views, const float* cams, const float* poses, int flags, nrf_host_frame* out) {
  int ticket = -1;
  int rc = nrf_submit_host_u8(c, n_views, cams, poses, flags, &ticket);
  if (rc) return rc;
  return nrf_wait_host_u8(c, ticket, out);
}

int nrf_render_batch(nrf_context* c, int n_views, const float* cams, const float* poses, void* stream, nrf_frame* out) {
  return nrf_render_views(c, n_views, cams, poses, stream, out);
}

int nrf_render(nrf_context* c, const float cam[4], const float pose[16], void* stream, nrf_frame* out) {
  if (!cam || !pose) return fail(NRF_E_INVALID, "null argument");
  return nrf_render_views(c, 1, cam, pose, stream, out);
}

// Diagnostic (not part of include/nerfhip.h): raw counters of the last render; slots 2..6 are
// only filled by the NRF_PHASE_TIMING build (make prof).
int nrf_debug_counters(nrf_context* c, unsigned long long out[16]) {
  if (!c || !out) return fail(NRF_E_INVALID, "null argument");
  HIP_TRY(hipEventSynchronize(c->ev1));
  unsigned long long raw[COUNTER_SLOTS * 16];
  HIP_TRY(hipMemcpy(raw, call_slot(c, c->call_index), COUNTER_BYTES, hipMemcpyDeviceToHost));
  for (int i = 0; i < 16; ++i) {
    out[i] = 0;
    for (int sl = 0; sl < COUNTER_SLOTS; ++sl) out[i] = i == 14 ? std::max(out[i], raw[sl * 16 + i]) : out[i] + raw[sl * 16 + i];  // 14: a maximum
  }
  return NRF_OK;
}

// Diagnostic (not part of include/nerfhip.h): which kernel instance renders the loaded model (DevModel::net) -- 0 register-resident,
// 1 generic, 2 wide, 3 the register-resident instance of another width (16 / 32 / 128 neurons) or depth, 4 its wide form for SH
// degree 5..8, 5 a GRID instance (base.json's MLPs behind another grid: F = 2 with fewer than 16 levels, F = 4 / 8, Smoothstep);
// + 16 when the persistent form is used (tests assert that a model runs where it is meant to).
extern "C" int nrf_debug_instance(nrf_context* c) {
  if (!c || !c->model_loaded) return -1;
  const int net = (int)c->dm.net;
  const int code = net == NET_HOT ? 0 : net == NET_GENERIC ? 1 : net == NET_WIDE ? 2 : net == NET_WIDE_SH ? 4 : net_grid_f(net) ? 5 : 3;
  return code + (c->dm.persistent ? 16 : 0);
}

// Diagnostic (not part of include/nerfhip.h): which RAYS instance nrf_render_rays launches for the loaded model -- the stage code of
// nrf_debug_instance (0 register-resident, 1 generic, 2 wide), + 16 for the persistent form (the hot shape whose tables fit)
extern "C" int nrf_debug_rays_instance(nrf_context* c) {
  if (!c || !c->model_loaded) return -1;
  if (c->fit.rays_persistent) return 16;
  const int st = (int)c->dm.stage;
  return st == NET_GENERIC ? 1 : st == NET_WIDE ? 2 : 0;
}

// Diagnostic (not part of include/nerfhip.h): the guard of caller-supplied rays (ray_valid, nrf_device.h) on the host -- the same
// function the RAYS instances apply per ray; 1 = the ray is rendered, 0 = its pixel is the background
extern "C" int nrf_debug_ray_valid(const float o[3], const float d[3]) {
  if (!o || !d) return 0;
  return ray_valid(o, d) ? 1 : 0;
}

// Diagnostic (not part of include/nerfhip.h): plan_model of a descriptor without a device, at an explicit quad-copy budget (MiB) --
// out = {own instance, stage instance, quad_mask, quad_far, waves of the own instance's persistent workgroup, its LDS bytes
// without the march tables}; returns nrf_load_model's status for the descriptor (tests/test_instance_plan_cpu.py)
extern "C" int nrf_debug_plan(const nrf_model_desc* d, int allow_own, uint64_t budget_mb, uint32_t out[6]) {
  if (!d || !d->params || !out) return fail(NRF_E_INVALID, "null argument");
  const ModelPlan p = plan_model(*d, allow_own != 0, budget_mb, 4);
  if (p.rc) return fail(p.rc, p.why);
  const int waves = render_persist_waves(p.own, march_form(d->density_grid_size, d->cascade, d->bound));
  const uint32_t v[6] = {(uint32_t)p.own, (uint32_t)p.stage, p.quad_mask, p.quad_far, (uint32_t)waves,
                         (uint32_t)render_persistent_lds_bytes(p.own, waves, p.gen_wave_bytes)};
  std::memcpy(out, v, sizeof(v));
  return NRF_OK;
}

// Diagnostic (not part of include/nerfhip.h): the gather plan plan_model chooses for a descriptor at that budget -- out = {plan
// (0 = GATHER_RUNTIME), the four steps' forms (0 mixed, 1 dense, 2 hashed, 3 near quad, 4 far quad; of the static plan or, under
// GATHER_RUNTIME, what the kernel selects at run time)}.  budget_mb = 0 is the default budget, as in nrf_model_desc.gather_copy_budget_mb
// (QUAD_BUDGET_MB_DEFAULT: no device to ask).  NRF_GATHER_PLAN=0 in the environment forces GATHER_RUNTIME as it does for a context
// (tests/test_gather_plan_cpu.py)
extern "C" int nrf_debug_gather_plan(const nrf_model_desc* d, int allow_own, uint64_t budget_mb, uint32_t out[5]) {
  if (!d || !d->params || !out) return fail(NRF_E_INVALID, "null argument");
  const char* e = std::getenv("NRF_GATHER_PLAN");
  const ModelPlan p = plan_model(*d, allow_own != 0, budget_mb ? budget_mb : (uint64_t)QUAD_BUDGET_MB_DEFAULT, 4, !(e && std::atoi(e) == 0));
  if (p.rc) return fail(p.rc, p.why);
  out[0] = p.gather_plan;
  for (int jl = 0; jl < 4; ++jl)
    out[1 + jl] = ((p.quad_mask >> (4 * jl)) & 1u) ? (((p.quad_far >> jl) & 1u) ? GFORM_QUAD_FAR : GFORM_QUAD) : ((p.uni_modes >> (2 * jl)) & 3u);
  return NRF_OK;
}

// Diagnostic (not part of include/nerfhip.h): the gather plan the context's loaded model launches with (DevModel::gather_plan, made
// from the copies the device really granted and the context's NRF_GATHER_PLAN) -- a static plan's id or 0 = GATHER_RUNTIME; -1
// without a model.  The persistent hot kernel alone reads it: nrf_debug_instance tells whether that kernel runs
extern "C" long long nrf_debug_context_gather_plan(nrf_context* c) {
  if (!c || !c->model_loaded) return -1;
  return (long long)c->dm.gather_plan;
}

// Diagnostic (not part of include/nerfhip.h): the LDS schedule (nrf_launch.h) of the persistent hot instance compiled for gather
// plan `plan` and march form `form` -- out = {1 if it reads its levels from the staged compact blocks, the depth of its weight
// fragment prefetch}; {0, 0} for GATHER_RUNTIME, which every other instance is compiled with (tests/test_lds_schedule_cpu.py)
extern "C" int nrf_debug_lds_schedule(uint32_t plan, int form, uint32_t out[2]) {
  if (!out) return fail(NRF_E_INVALID, "null argument");
  if (plan != GATHER_RUNTIME && plan != GATHER_QQFH && plan != GATHER_QQHH && plan != GATHER_DMHH) return fail(NRF_E_INVALID, "not a gather plan");
  if (form != MARCH_FORM_GENERIC && form != MARCH_FORM_UNIT && form != MARCH_FORM_POW2) return fail(NRF_E_INVALID, "not a march form");
  out[0] = plan_levels(plan) ? 1u : 0u;
  out[1] = (uint32_t)plan_frag_depth(plan, form);
  return NRF_OK;
}

// Diagnostic (not part of include/nerfhip.h): the march side of the instance choice for a grid of side H with `cascade` cascades and
// that bound -- out = {march_form (nrf_launch.h: 0 generic, 1 unit, 2 power of two), 1 if the grid has the coarse occupancy
// level the march tables in LDS -- and with them the persistent kernel -- need (march_coarse_shift)} (tests/test_plan_matrix_cpu.py)
extern "C" int nrf_debug_march_form(uint32_t H, uint32_t cascade, float bound, uint32_t out[2]) {
  if (!out || H == 0 || cascade == 0 || !(bound > 0.0f)) return fail(NRF_E_INVALID, "bad argument");
  out[0] = (uint32_t)march_form(H, cascade, bound);
  out[1] = march_coarse_shift(H) ? 1u : 0u;
  return NRF_OK;
}

// Diagnostic (not part of include/nerfhip.h): the step plan (nrf_step_plan.h) without a device -- step_table of the four inputs
// into table[capacity] (capacity <= 1024; *n_out = its entries), then step_land of every (starts[i], targets[i]) on that table
// into landed[i] -- of min(targets[i], far) when far is finite, as the fast-forward functions clamp their barrier to the ray's
// far (an unclamped +inf target has no answer: the loop never ends once t + dt == t).  lds[0..2] (null: skipped) = a launch's LDS bytes without the table, the table's entries and a compute unit's
// LDS: lds[3] = step_table_lds_offset of them.  tests/test_step_table_cpu.py.
extern "C" int nrf_debug_step_table(float min_near, float dt_gamma, float bound, uint32_t H, int capacity, float* table, int* n_out,
                                    int n_targets, const float* starts, const float* targets, float far, float* landed, int32_t* lds) {
  if (!table || !n_out || capacity < 0 || capacity > STEP_TABLE_CAPACITY || n_targets < 0 || (n_targets > 0 && (!starts || !targets || !landed)))
    return fail(NRF_E_INVALID, "bad argument");
  const int n = step_table(min_near, dt_gamma, bound, H, capacity, table);
  *n_out = n;
  const float dt_min = step_dt_min(), dt_max = step_dt_max(bound, H);
  for (int i = 0; i < n_targets; ++i)
    landed[i] = step_land(n > 0 ? table : nullptr, n, starts[i], far <= 3.402823466e+38f ? fminf(targets[i], far) : targets[i], dt_gamma, dt_min, dt_max);
  if (lds) lds[3] = step_table_lds_offset((uint32_t)lds[0], lds[1], (uint32_t)lds[2]);
  return NRF_OK;
}

// Diagnostic (not part of include/nerfhip.h): what a render call of this context would hand the persistent kernel under its current
// options -- out[0] = entries of the step table (0: none), out[1] = its byte offset in the workgroup's LDS (-1: not staged -- no
// table, it does not fit, or the model has no persistent form), out[2] = the launch's LDS bytes with it.  tests/test_step_table_gpu.py.
extern "C" int nrf_debug_step_table_launch(nrf_context* c, int32_t out[3]) {
  int rc = need_model(c);
  if (rc) return rc;
  if (!out) return fail(NRF_E_INVALID, "null argument");
  FrameParams P;
  std::memset(&P, 0, sizeof(P));
  P.min_near = c->opt.min_near;
  P.dt_gamma = c->opt.dt_gamma;
  const float* tab = nullptr;
  int n = 0;
  if (!c->opt.perturb && c->march_ff) {
    rc = step_table_for(c, P, tab, n);
    if (rc) return rc;
  }
  const int lds = c->dm.persistent ? render_persistent_launch_lds_bytes(c->dm) : 0;
  out[0] = n;
  out[1] = c->dm.persistent && tab != nullptr ? step_table_lds_offset((uint32_t)lds, n, CU_LDS_BYTES) : -1;
  out[2] = out[1] >= 0 ? out[1] + 4 * n : lds;
  return NRF_OK;
}

// the 17 values nrf_debug_grid_plan and nrf_debug_grid_readout share: the fit, the tables' geometry and their lengths in words
static void grid_plan_values(const DevModel& M, const GridFit& f, const size_t n_words[4], uint32_t out[17]) {
  const uint32_t v[17] = {M.net, M.stage, M.persistent, M.persist_waves, M.gen_weights_lds, M.lds_coarse_words, M.lds_ctab_floats, f.lds_dilated_strip,
                          f.lds_dilated_persist, M.coarse_shift, M.dilated_level_words, f.rays_persistent ? 1u : 0u,
                          M.persistent ? (uint32_t)render_persistent_launch_lds_bytes(M) : 0u,  // (what launch_render asks for)
                          (uint32_t)n_words[0], (uint32_t)n_words[1], (uint32_t)n_words[2], (uint32_t)n_words[3]};
  std::memcpy(out, v, sizeof(v));
}

// Diagnostic (not part of include/nerfhip.h): plan_model, then plan_grid, of a descriptor without a device -- grid: [C * H^3] floats
// (null: the descriptor's), flags: bit 0 allow_own (NRF_WIDTH_INSTANCES), bit 1 allow_persistent (NRF_PERSISTENT), bit 2 allow_gen_wlds
// (NRF_GEN_WLDS); reads no environment.  out = {net, stage, persistent, persist_waves, gen_weights_lds, lds_coarse_words, lds_ctab_floats,
// the dilated words staged by the per-strip and by the persistent form, coarse_shift, dilated_level_words, rays_persistent, the LDS
// bytes launch_render asks for (from a DevModel the plan was applied to, as set_density_grid does), words of occ / coarse / ctab /
// dilated, visibility_walk, GridFit::persistent_lds_bytes}; box = occ_box; the tables are copied to the buffers that are given
// (tests/test_grid_plan_cpu.py)
extern "C" int nrf_debug_grid_plan(const nrf_model_desc* d, const float* grid, float mean_density, uint32_t flags, uint32_t out[19], float box[6],
                                   uint32_t* occ, uint32_t* coarse, float* ctab, uint32_t* dilated) {
  if (!d || !d->params || !out || !box || (!grid && !d->density_grid)) return fail(NRF_E_INVALID, "null argument");
  const ModelPlan p = plan_model(*d, (flags & 1u) != 0, QUAD_BUDGET_MB_DEFAULT, 4);
  if (p.rc) return fail(p.rc, p.why);
  DevModel M;
  fill_dev_model(M, *d, p);
  const GridPlan g = plan_grid(*d, p.own, p.stage, M.gen_wave_bytes, M.gen_frag_bytes, (flags & 2u) != 0, (flags & 4u) != 0,
                               grid ? grid : d->density_grid, mean_density);
  apply_grid_plan(M, g);
  const GridTables& T = g.tables;
  const size_t n_words[4] = {T.occ.size(), T.coarse.size(), T.ctab.size(), T.dilated.size()};
  grid_plan_values(M, g.fit, n_words, out);
  out[17] = T.visibility_walk ? 1u : 0u;
  out[18] = g.fit.persistent_lds_bytes;
  std::memcpy(box, T.occ_box, sizeof(T.occ_box));
  if (occ) std::memcpy(occ, T.occ.data(), T.occ.size() * 4);
  if (coarse) std::memcpy(coarse, T.coarse.data(), T.coarse.size() * 4);
  if (ctab) std::memcpy(ctab, T.ctab.data(), T.ctab.size() * 4);
  if (dilated) std::memcpy(dilated, T.dilated.data(), T.dilated.size() * 4);
  return NRF_OK;
}

// Diagnostic (not part of include/nerfhip.h): the frame plan (nrf_frame_plan.h) of one render call, without a context or a device.
// in = {W, H, shard_index, shard_count, n_views, n_cus, persist_waves, queue_classes, plan_max_pos, plan_cap, dilated bytes, flags,
// the previous rectangle of the fill {row lo, row hi, column lo, column hi}, RENDER_WAVES}; flags: 1 sample cap forced, 2 depth
// plane, 4 host_cols, 8 the context and model allow progressive copies, 16 the launch has a plan buffer and a dilated table, 32 the
// fill's background changed, 64 one launch of up to NRF_MAX_VIEWS views whatever views_per_launch says (the refusal), 128 a host
// frame: bands, copies and fills follow.  fin = {model scale, background, occupied box[6]}; rois (optional): the views' regions
// [n_views][4] instead of cams [n_views][4] / poses [n_views][16].  out = 24 values {tiles_x, tiles_y, strips per row, strips,
// local tiles, tiles per shard, views per launch, all_tail, sample cap dropped, progressive, views of the first launch, q_total,
// n_classes, class_cols, workgroups, blocks_per_view, refused, planned, n_pos, copied bytes, bands, fill rectangles, filled
// bytes, the quantised background}, per view {roi[4], row lo, row hi, column lo, column hi}, per view of the first launch
// {k_lo, k_hi, q_begin, q_rows, q_row0}; a host frame: per band {view, lo, hi, s0, s1}, per view {pitched, rgb off, pitch,
// width, rows, depth off, pitch, width, rows}, per view {n, 4 x {r0, r1, c0, c1}, the new rectangle} (tests/test_frame_plan_cpu.py)
extern "C" int nrf_debug_frame_plan(const int32_t in[17], const float fin[8], const float* cams, const float* poses, const int32_t* rois,
                                    int64_t* out, int64_t cap, int64_t* n_out) {
  if (!in || !fin || !out || !n_out || (!rois && (!cams || !poses))) return fail(NRF_E_INVALID, "null argument");
  const int W = in[0], H = in[1], idx = in[2], N = in[3], n_views = in[4], n_cus = in[5], waves = in[6], flags = in[11];
  if (W < 1 || H < 1 || N < 1 || idx < 0 || idx >= N || n_views < 1 || n_cus < 1 || waves < 1 || in[16] < 1) return fail(NRF_E_INVALID, "bad argument");
  const bool host = (flags & 128) != 0, with_depth = (flags & 2) != 0;
  std::vector<int64_t> o(24, 0);
  const int tiles_x = tiles_of(W), tiles_y = tiles_of(H), n_local = local_tiles(W, H, idx, N);
  const int per_launch = views_per_launch(tiles_x, tiles_y, MAX_VIEWS);
  const int launch_views = std::min(n_views, (flags & 64) ? MAX_VIEWS : per_launch);
  const bool progressive = host_frame_progressive((flags & 8) != 0, n_views, W, tiles_y, in[8]);
  std::vector<int> roi((size_t)4 * n_views), rows((size_t)4 * n_views);
  for (int v = 0; v < n_views; ++v) {
    int* r = &roi[4 * (size_t)v];
    if (rois) std::memcpy(r, rois + 4 * (size_t)v, 4 * sizeof(int));
    else {
      float R[9], org[3];
      nerf_matrix_to_ngp(poses + 16 * (size_t)v, fin[0], R, org);
      view_roi(R, org, cams + 4 * (size_t)v, fin + 2, W, H, r);
      far_camera_roi(org, MAX_CAMERA_DISTANCE, r);
    }
    int* ro = &rows[4 * (size_t)v];
    roi_rows(r, H, ro[0], ro[1]);
    roi_cols(r, W, ro[2], ro[3]);
    o.insert(o.end(), r, r + 4);
    o.insert(o.end(), ro, ro + 4);
  }
  std::vector<ViewQueue> vq((size_t)launch_views);
  const QueuePlan Q = plan_queues({tiles_x, tiles_y, idx, N, n_local, in[7], n_cus, waves, in[16]}, launch_views, roi.data(), vq.data());
  for (const ViewQueue& q : vq) o.insert(o.end(), {q.k_lo, q.k_hi, q.q_begin, q.q_rows, q.q_row0});
  int64_t copied = 0, n_bands = 0, n_fill = 0, filled = 0;
  if (host) {
    auto put = [&](const PlaneCopy& p, bool on) { o.insert(o.end(), {on ? (int64_t)p.off : 0, on ? (int64_t)p.pitch : 0, on ? (int64_t)p.width : 0, on ? (int64_t)p.rows : 0}); };
    const std::vector<Band> bands = progressive ? plan_bands(W, with_depth, n_views, rows.data()) : std::vector<Band>();
    n_bands = (int64_t)bands.size();
    const size_t px = (size_t)W * H;
    for (const Band& b : bands) {
      o.insert(o.end(), {b.view, b.lo, b.hi, b.s0, b.s1});
      const RowCopy k = row_copy(W, px, (size_t)n_views, b.view, b.lo, b.hi, 0, 0);
      copied += (int64_t)(k.rgb.bytes() + (with_depth ? k.depth.bytes() : 0));
    }
    const bool use_cols = (flags & 4) && !progressive;
    for (int v = 0; v < n_views; ++v) {
      const int* ro = &rows[4 * (size_t)v];
      const bool on = !progressive && ro[1] > ro[0];
      const RowCopy k = on ? row_copy(W, px, (size_t)n_views, v, ro[0], ro[1], use_cols ? ro[2] : 0, use_cols ? ro[3] : 0) : RowCopy{};
      o.push_back(k.pitched ? 1 : 0);
      put(k.rgb, on);
      put(k.depth, on && with_depth);
      if (on) copied += (int64_t)(k.rgb.bytes() + (with_depth ? k.depth.bytes() : 0));
    }
    for (int v = 0; v < n_views; ++v) {
      const FillPlan F = fill_rects({in[12], in[13], in[14], in[15]}, (flags & 32) != 0, W, H, &rows[4 * (size_t)v], use_cols);
      o.push_back(F.n);
      for (int i = 0; i < 4; ++i) {
        const Rect r = i < F.n ? F.rects[i] : Rect{0, 0, 0, 0};
        o.insert(o.end(), {r.r0, r.r1, r.c0, r.c1});
        filled += 4LL * (r.r1 - r.r0) * (r.c1 - r.c0);  // (rgb + depth bytes)
      }
      o.insert(o.end(), {F.now.r0, F.now.r1, F.now.c0, F.now.c1});
      n_fill += F.n;
    }
  }
  const int64_t head[24] = {tiles_x, tiles_y, strips_per_row(tiles_x), total_strips(W, H), n_local, tiles_per_shard(W, H, N), per_launch,
                            call_is_all_tail(n_local, n_views, n_cus, (unsigned)waves), drops_sample_cap(n_local, n_views, n_cus, (unsigned)waves, (flags & 1) != 0),
                            progressive, launch_views, Q.q_total, Q.n_classes, Q.class_cols, Q.workgroups, Q.blocks_per_view, Q.refused,
                            launch_is_planned((flags & 16) != 0, Q.n_pos, in[9], in[10]), Q.n_pos, copied, n_bands, n_fill, filled, host_quant_u8(fin[1])};
  std::copy(head, head + 24, o.begin());
  *n_out = (int64_t)o.size();
  if ((int64_t)o.size() > cap) return fail(NRF_E_INVALID, "the output buffer is too small");
  std::copy(o.begin(), o.end(), out);
  return NRF_OK;
}

// Diagnostic (not part of include/nerfhip.h): FrameParams::hit_exp of an nrf_ray_hits call with this threshold (hit_cap_exponent,
// nrf_frame_plan.h), without a context or a device (tests/test_ray_hits_cpu.py)
extern "C" int nrf_debug_hit_cap_exponent(float opacity) { return hit_cap_exponent(opacity); }

// Diagnostic (not part of include/nerfhip.h): the same 17 values of the loaded context, its occ_box, and its four device tables
// copied to the buffers that are given (tests/test_grid_plan_gpu.py)
extern "C" int nrf_debug_grid_readout(nrf_context* c, uint32_t out[17], float box[6], uint32_t* occ, uint32_t* coarse, float* ctab,
                                      uint32_t* dilated) {
  if (!c || !c->model_loaded || !out || !box) return fail(NRF_E_INVALID, "bad argument");
  grid_plan_values(c->dm, c->fit, c->table_words, out);
  std::memcpy(box, c->dm.occ_box, sizeof(c->dm.occ_box));
  void* dst[4] = {occ, coarse, ctab, dilated};
  const void* src[4] = {c->d_occ, c->d_coarse, c->d_ctab, c->d_dilated};
  for (int i = 0; i < 4; ++i)
    if (dst[i] && c->table_words[i]) HIP_TRY(hipMemcpy(dst[i], src[i], c->table_words[i] * 4, hipMemcpyDeviceToHost));
  return NRF_OK;
}

// The parts of a model's image nrf_debug_model_image and nrf_debug_model_readout share (`which`): 0 frags, 1 frags_gen, 2 frags_hot,
// 3 the GenModel bytes, 4 grid16 (the reference-order table), 5 the 16 LevelParams, 6 the plan's part of DevModel as 12 words --
// {net, stage, quad_mask, quad_far, uni_modes, gather_plan, grid_bytes, gen_wave_bytes, gen_frag_bytes, depth_xd, depth_xr, dir_w}
enum : int { PART_FRAGS = 0, PART_FRAGS_GEN, PART_FRAGS_HOT, PART_GEN, PART_GRID16, PART_LEVELS, PART_PLAN, N_PARTS };
static void plan_words(const DevModel& M, uint32_t own, uint32_t out[12]) {
  const uint32_t v[12] = {own, M.stage, M.quad_mask, M.quad_far, M.uni_modes, M.gather_plan, M.grid_bytes, M.gen_wave_bytes, M.gen_frag_bytes,
                          M.depth_xd, M.depth_xr, M.dir_w};
  std::memcpy(out, v, sizeof(v));
}

// Diagnostic (not part of include/nerfhip.h): one part of what nrf_load_model would upload for a descriptor, without a device --
// plan_model at an explicit quad-copy budget (MiB; 0: QUAD_BUDGET_MB_DEFAULT, as in nrf_debug_gather_plan), then build_model_image and
// fill_dev_model.  flags: bit 0 drop_quads first (the device had no room for the copies), bit 1 no step may have copies
// (NRF_QUAD_LEVELS=0), bit 2 NRF_GEN_FAST_GRID=0; reads no environment.  Copies min(length, cap) bytes of part `which` to buf and
// returns the part's length in *n (tests/test_model_image_cpu.py)
extern "C" int nrf_debug_model_image(const nrf_model_desc* d, int allow_own, uint64_t budget_mb, uint32_t flags, int which, void* buf, uint64_t cap,
                                     uint64_t* n) {
  if (!d || !d->params || !n || which < 0 || which >= N_PARTS || (cap && !buf)) return fail(NRF_E_INVALID, "bad argument");
  ModelPlan p = plan_model(*d, allow_own != 0, budget_mb ? budget_mb : (uint64_t)QUAD_BUDGET_MB_DEFAULT, (flags & 2u) ? 0 : 4);
  if (p.rc) return fail(p.rc, p.why);
  if (flags & 1u) p = drop_quads(p);
  const ModelImage im = build_model_image(*d, p, (flags & 4u) == 0);
  DevModel M;
  fill_dev_model(M, *d, p);
  uint32_t words[12];
  plan_words(M, (uint32_t)p.own, words);
  const void* src[N_PARTS] = {im.frags.data(), im.frags_gen.data(), im.frags_hot.data(), &im.gen, im.grid16.data(), p.lp, words};
  const uint64_t len[N_PARTS] = {im.frags.size() * 2, im.frags_gen.size() * 2, im.frags_hot.size() * 2, p.stage != NET_HOT ? sizeof(GenModel) : 0,
                                 im.grid16.size() * 2, sizeof(p.lp), sizeof(words)};
  *n = len[which];
  if (cap && *n) std::memcpy(buf, src[which], (size_t)std::min<uint64_t>(cap, *n));
  return NRF_OK;
}

// Diagnostic (not part of include/nerfhip.h): the same parts of the loaded context, copied back from the device (d_wfrag, d_wfrag_gen,
// d_wfrag_hot, d_gen, the reference-order part of d_grid, d_lv; the plan's words from its DevModel) (tests/test_model_image_gpu.py)
extern "C" int nrf_debug_model_readout(nrf_context* c, int which, void* buf, uint64_t cap, uint64_t* n) {
  if (!c || !c->model_loaded || !n || which < 0 || which >= N_PARTS || (cap && !buf)) return fail(NRF_E_INVALID, "bad argument");
  int rc = set_device(c);
  if (rc) return rc;
  uint32_t words[12];
  plan_words(c->dm, (uint32_t)c->own_net, words);
  const void* src[N_PARTS] = {c->d_wfrag, c->d_wfrag_gen, c->d_wfrag_hot, c->d_gen, c->d_grid, c->d_lv, words};
  const uint64_t len[N_PARTS] = {c->wfrag_bytes, c->wfrag_gen_bytes, c->wfrag_hot_bytes, c->d_gen ? sizeof(GenModel) : 0, c->table_ref_bytes,
                                 16 * sizeof(LevelParams), sizeof(words)};
  *n = len[which];
  const size_t bytes = (size_t)std::min<uint64_t>(cap, *n);
  if (bytes && which == PART_PLAN) std::memcpy(buf, words, bytes);
  else if (bytes) HIP_TRY(hipMemcpy(buf, src[which], bytes, hipMemcpyDeviceToHost));
  return NRF_OK;
}

// Diagnostic build: entry / exit stamps (s_memtime) of the persistent kernel's waves, 2 x n values.
extern "C" int nrf_debug_wave_times(nrf_context* c, unsigned long long* out, int n_waves) {
  if (!c || !out || n_waves < 1 || n_waves > 4096) return fail(NRF_E_INVALID, "bad argument");
  HIP_TRY(hipEventSynchronize(c->ev1));
  HIP_TRY(hipMemcpy(out, call_slot(c, c->call_index) + COUNTER_BYTES + 128, (size_t)n_waves * 16, hipMemcpyDeviceToHost));
  return NRF_OK;
}

int nrf_render_async(nrf_context* c, const float cam[4], const float pose[16], nrf_frame* out) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  return nrf_render(c, cam, pose, (void*)c->stream, out);
}

int nrf_sync(nrf_context* c) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  int rc = set_device(c);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->last_stream && c->last_stream != c->stream) HIP_TRY(hipStreamSynchronize(c->last_stream));
  return NRF_OK;
}

int nrf_bind_output(nrf_context* c, void* rgba, void* depth) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if ((rgba == nullptr) != (depth == nullptr)) return fail(NRF_E_INVALID, "bind both planes or neither");
  c->bound_rgba = rgba;
  c->bound_depth = depth;
  c->bound_rgbd8 = nullptr;
  c->bound_rgb8 = c->bound_depth8 = nullptr;
  return NRF_OK;
}

int nrf_bind_output_rgbd8(nrf_context* c, void* rgbd8) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  c->bound_rgbd8 = rgbd8;
  if (rgbd8) c->bound_rgba = c->bound_depth = c->bound_rgb8 = c->bound_depth8 = nullptr;
  return NRF_OK;
}

int nrf_bind_output_u8(nrf_context* c, void* rgb8, void* depth8) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if ((rgb8 == nullptr) != (depth8 == nullptr)) return fail(NRF_E_INVALID, "bind both planes or neither");
  if (((uintptr_t)rgb8 | (uintptr_t)depth8) & 3u) return fail(NRF_E_INVALID, "8-bit planes must be 4-byte aligned");
  c->bound_rgb8 = rgb8;
  c->bound_depth8 = depth8;
  if (rgb8) c->bound_rgba = c->bound_depth = c->bound_rgbd8 = nullptr;
  return NRF_OK;
}

int nrf_get_stats(nrf_context* c, nrf_stats* s) {
  if (!c || !s) return fail(NRF_E_INVALID, "null argument");
  if (!c->rendered) return fail(NRF_E_STATE, "nothing rendered yet");
  int rc = set_device(c);
  if (rc) return rc;
  HIP_TRY(hipEventSynchronize(c->ev1));
  unsigned long long raw[COUNTER_SLOTS * 16], cnt[6] = {0, 0, 0, 0, 0, 0};
  HIP_TRY(hipMemcpy(raw, call_slot(c, c->call_index), COUNTER_BYTES, hipMemcpyDeviceToHost));
  for (int sl = 0; sl < COUNTER_SLOTS; ++sl) {
    cnt[0] += raw[sl * 16];
    cnt[1] += raw[sl * 16 + 1];
    cnt[2] += raw[sl * 16 + 11];
    cnt[3] += raw[sl * 16 + 7];
    cnt[4] += raw[sl * 16 + 12];
    cnt[5] += raw[sl * 16 + 13];
  }
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  s->n_rays = (uint64_t)c->n_local_tiles * 64;
  s->n_samples = cnt[0];
  s->n_rounds = cnt[1];
  s->n_network_evals = cnt[2];
  s->n_composited = cnt[3];
  s->render_ms = ms;
  s->shader_clock_mhz = 0.f;
  s->gather_addresses_per_sample = c->gather_addresses;
  s->grid_device_bytes = c->table_bytes;
#ifndef NRF_PHASE_TIMING  // (a diagnostic build keeps other quantities in these two counters)
  if (cnt[5] > 0) s->shader_clock_mhz = (float)((double)cnt[4] / (double)cnt[5] * 100.0);
#endif
  return NRF_OK;
}

int nrf_read_view_f32(nrf_context* c, int view, float* rgba, float* depth) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!c->rendered) return fail(NRF_E_STATE, "nothing rendered yet");
  if (!c->last_rgba) return fail(NRF_E_STATE, "the last render went to a packed 8-bit buffer (nrf_bind_output_rgbd8): it is the caller's to read");
  if (tiled_layout(c)) return fail(NRF_E_STATE, "nrf_read_f32 needs a single-shard (row-major) frame");
  if (view < 0 || view >= c->last_views) return fail(NRF_E_INVALID, "view index out of range");
  int rc = set_device(c);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->last_stream));
  const size_t n = (size_t)c->W * c->H;
  if (rgba) HIP_TRY(hipMemcpy(rgba, (const char*)c->last_rgba + (size_t)view * c->n_out_px * 16, n * 16, hipMemcpyDeviceToHost));
  if (depth) HIP_TRY(hipMemcpy(depth, (const char*)c->last_depth + (size_t)view * c->n_out_px * 4, n * 4, hipMemcpyDeviceToHost));
  return NRF_OK;
}

int nrf_read_f32(nrf_context* c, float* rgba, float* depth) { return nrf_read_view_f32(c, 0, rgba, depth); }

int nrf_read_shard_f32(nrf_context* c, float* rgba, float* depth) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!c->rendered) return fail(NRF_E_STATE, "nothing rendered yet");
  if (!c->last_rgba) return fail(NRF_E_STATE, "the last render went to a packed 8-bit buffer (nrf_bind_output_rgbd8): it is the caller's to read");
  int rc = set_device(c);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->last_stream));
  const size_t n = tiled_layout(c) ? (size_t)c->n_local_tiles * 64 : (size_t)c->W * c->H;
  if (rgba) HIP_TRY(hipMemcpy(rgba, c->last_rgba, n * 16, hipMemcpyDeviceToHost));
  if (depth) HIP_TRY(hipMemcpy(depth, c->last_depth, n * 4, hipMemcpyDeviceToHost));
  return NRF_OK;
}

int nrf_read_view_u8(nrf_context* c, int view, uint8_t* rgb, uint8_t* depth) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!c->rendered) return fail(NRF_E_STATE, "nothing rendered yet");
  if (!c->last_rgba) return fail(NRF_E_STATE, "the last render went to a packed 8-bit buffer (nrf_bind_output_rgbd8): it is the caller's to read");
  if (tiled_layout(c)) return fail(NRF_E_STATE, "nrf_read_u8 needs a single-shard (row-major) frame");
  if (view < 0 || view >= c->last_views) return fail(NRF_E_INVALID, "view index out of range");
  int rc = set_device(c);
  if (rc) return rc;
  const size_t n = (size_t)c->W * c->H;
  if (!c->d_rgb8) {
    HIP_TRY(hipMalloc(&c->d_rgb8, n * 3));
    HIP_TRY(hipMalloc(&c->d_depth8, n));
  }
  hipStream_t st = c->last_stream;
  HIP_TRY(launch_quantize((const char*)c->last_rgba + (size_t)view * c->n_out_px * 16,
                          (const char*)c->last_depth + (size_t)view * c->n_out_px * 4, (int)n, c->d_rgb8, c->d_depth8, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (rgb) HIP_TRY(hipMemcpy(rgb, c->d_rgb8, n * 3, hipMemcpyDeviceToHost));
  if (depth) HIP_TRY(hipMemcpy(depth, c->d_depth8, n, hipMemcpyDeviceToHost));
  return NRF_OK;
}

int nrf_read_u8(nrf_context* c, uint8_t* rgb, uint8_t* depth) { return nrf_read_view_u8(c, 0, rgb, depth); }

int nrf_quantize_rgbd8(nrf_context* c, const void* rgba, const void* depth, uint64_t n_px, void* out_u32, void* stream) {
  if (!c || !rgba || !depth || !out_u32) return fail(NRF_E_INVALID, "null argument");
  int rc = set_device(c);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_quantize_rgbd8(rgba, depth, n_px, out_u32, st));
  if (!stream) HIP_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_quantize_u8(nrf_context* c, const void* rgba, const void* depth, uint64_t n_px, void* rgb8, void* depth8, void* stream) {
  if (!c || !rgba || !depth || !rgb8 || !depth8) return fail(NRF_E_INVALID, "null argument");
  if (n_px >= (1ull << 31)) return fail(NRF_E_INVALID, "n_px must be below 2^31");
  int rc = set_device(c);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_quantize(rgba, depth, (int)n_px, rgb8, depth8, st));
  if (!stream) HIP_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_untile_views_u8(nrf_context* c, const void* gathered_rgbd8, int shard_count, int tiles_per_shard, int n_views, void* rgb8,
                        void* depth8, void* stream) {
  if (!c || !gathered_rgbd8 || !rgb8 || !depth8 || shard_count < 1 || tiles_per_shard < 1 || n_views < 1)
    return fail(NRF_E_INVALID, "bad argument");
  if (c->W <= 0) return fail(NRF_E_STATE, "set_resolution has not been called");
  if (((uintptr_t)gathered_rgbd8 & 15u) || ((c->W & 3) == 0 && (((uintptr_t)rgb8 | (uintptr_t)depth8) & 3u)))
    return fail(NRF_E_INVALID, "the gathered shards must be 16-byte aligned, the 8-bit planes 4-byte aligned (widths that are multiples of 4)");
  int rc = set_device(c);
  if (rc) return rc;
  if (tiles_per_shard != nrf::tiles_per_shard(c->W, c->H, shard_count)) return fail(NRF_E_INVALID, "tiles_per_shard does not match the resolution");
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_untile_rgbd8_u8(gathered_rgbd8, shard_count, tiles_per_shard, c->W, c->H, n_views, rgb8, depth8, st));
  if (!stream) HIP_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_untile_views(nrf_context* c, const void* gathered, int shard_count, int tiles_per_shard, int channels, int n_views,
                     void* out, void* stream) {
  if (!c || !gathered || !out || shard_count < 1 || tiles_per_shard < 1 || channels < 1 || n_views < 1)
    return fail(NRF_E_INVALID, "bad argument");
  if (c->W <= 0) return fail(NRF_E_STATE, "set_resolution has not been called");
  int rc = set_device(c);
  if (rc) return rc;
  if (tiles_per_shard != nrf::tiles_per_shard(c->W, c->H, shard_count)) return fail(NRF_E_INVALID, "tiles_per_shard does not match the resolution");
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_untile(gathered, shard_count, tiles_per_shard, channels, c->W, c->H, n_views, out, st));
  if (!stream) HIP_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_untile(nrf_context* c, const void* gathered, int shard_count, int tiles_per_shard, int channels, void* out,
               void* stream) {
  return nrf_untile_views(c, gathered, shard_count, tiles_per_shard, channels, 1, out, stream);
}

// ---- stage entry points ----
#define STAGE_PROLOGUE()                                         \
  int rc = need_model(c);                                        \
  if (rc) return rc;                                             \
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;

#define STAGE_EPILOGUE() \
  if (!stream) HIP_TRY(hipStreamSynchronize(st)); \
  return NRF_OK;

int nrf_encode_grid(nrf_context* c, const void* pos01, uint32_t n, void* out, void* stream) {
  STAGE_PROLOGUE();
  if (n && (!pos01 || !out)) return fail(NRF_E_INVALID, "null argument");
  HIP_TRY(launch_encode_grid(c->dm, pos01, n, out, st, c->opt.fast_interp != 0));
  STAGE_EPILOGUE();
}

// A wide model's rows (direction encodings of 32..80 values) go through the generic stage kernels: same arithmetic,
// generic-layout fragments; the fused kernel and nrf_network run the wide instance itself.
static DevModel stage_model(const nrf_context* c) {
  DevModel m = c->dm;
  if (m.stage == NET_WIDE) {
    m.stage = NET_GENERIC;
    m.wfrag = (const uint4*)c->d_wfrag_gen;
  }
  return m;
}

int nrf_encode_dir(nrf_context* c, const void* dir01, uint32_t n, void* out, void* stream) {
  STAGE_PROLOGUE();
  if (n && (!dir01 || !out)) return fail(NRF_E_INVALID, "null argument");
  HIP_TRY(launch_encode_dir(stage_model(c), dir01, n, out, st));
  STAGE_EPILOGUE();
}

int nrf_mlp_forward_repeat(nrf_context* c, const void* feat, const void* dirfeat, uint32_t n, void* out, uint32_t repeat,
                           void* stream) {
  STAGE_PROLOGUE();
  if (n && (!feat || !dirfeat || !out)) return fail(NRF_E_INVALID, "null argument");
  if (repeat < 1) return fail(NRF_E_INVALID, "repeat must be >= 1");
  const DevModel m = stage_model(c);
  // the hot stage reads a lane's 16 bytes of its feature row and 8 of its direction row in one load each and writes a row's four
  // halves in one 8-byte store; the generic stage reads halves and writes the same 8-byte rows
  const uintptr_t in_mask = m.stage == NET_GENERIC ? 1u : 15u, dir_mask = m.stage == NET_GENERIC ? 1u : 7u;
  if (n && (((uintptr_t)feat & in_mask) || ((uintptr_t)dirfeat & dir_mask) || ((uintptr_t)out & 7u)))
    return fail(NRF_E_INVALID, "feat must be 16-byte aligned, dirfeat and out 8-byte aligned (generic stage: feat and dirfeat 2-byte aligned)");
  HIP_TRY(launch_mlp_forward(m, feat, dirfeat, n, out, repeat, st));
  STAGE_EPILOGUE();
}

int nrf_mlp_forward(nrf_context* c, const void* feat, const void* dirfeat, uint32_t n, void* out, void* stream) {
  return nrf_mlp_forward_repeat(c, feat, dirfeat, n, out, 1, stream);
}

int nrf_network(nrf_context* c, const void* xyz, const void* dir, uint32_t n, void* sigma, void* rgb, void* stream) {
  STAGE_PROLOGUE();
  if (n && (!xyz || !dir || !sigma || !rgb)) return fail(NRF_E_INVALID, "null argument");
  HIP_TRY(launch_network(c->dm, xyz, dir, n, sigma, rgb, st));
  STAGE_EPILOGUE();
}

// Point queries (nrf_kernels_points.hip; the arithmetic is nrf_points_plan.h): the stream rules of nrf_network, no slot of the
// 16-call ring, no statistics, nothing of the context's frame buffers is written.
int nrf_density(nrf_context* c, const void* xyz, uint32_t n, void* sigma, void* stream) {
  STAGE_PROLOGUE();
  if (n && (!xyz || !sigma)) return fail(NRF_E_INVALID, "null argument");
  PointsArgs A;
  A.xyz = (const float*)xyz;
  A.n = n;
  A.bound = c->desc.bound;
  A.sigma = (float*)sigma;
  HIP_TRY(launch_points(c->dm, POINTS_VALUE, A, st));
  STAGE_EPILOGUE();
}

int nrf_density_gradient(nrf_context* c, const void* xyz, uint32_t n, float h, void* out, void* stream) {
  STAGE_PROLOGUE();
  if (n && (!xyz || !out)) return fail(NRF_E_INVALID, "null argument");
  if (!points_step_valid(h, c->desc.bound)) return fail(NRF_E_INVALID, "nrf_density_gradient: h must be finite, > 0 and <= bound");
  PointsArgs A;
  A.xyz = (const float*)xyz;
  A.n = n;
  A.bound = c->desc.bound;
  A.h = h;
  A.inv2h = points_inv2h(h);
  A.out = (float*)out;
  HIP_TRY(launch_points(c->dm, POINTS_GRADIENT, A, st));
  STAGE_EPILOGUE();
}

int nrf_hit_gradients(nrf_context* c, const nrf_frame* hits, const nrf_rays* rays, float opacity, float frac, float h, void* pos,
                      void* out, void* stream) {
  STAGE_PROLOGUE();
  if (!hits || !rays || !rays->rays_o || !rays->rays_d || !pos || !out) return fail(NRF_E_INVALID, "null argument");
  if (!hits->rgba) return fail(NRF_E_INVALID, "nrf_hit_gradients: the hit frame has no rgba plane");
  if (!points_step_valid(h, c->desc.bound)) return fail(NRF_E_INVALID, "nrf_hit_gradients: h must be finite, > 0 and <= bound");
  if (!points_frac_valid(frac)) return fail(NRF_E_INVALID, "nrf_hit_gradients: frac must be in [0, 1]");  // (NaN fails both)
  if (!points_opacity_valid(opacity)) return fail(NRF_E_INVALID, "nrf_hit_gradients: opacity must be in (0, 1]");
  if (hits->tile_major) return fail(NRF_E_UNSUPPORTED, "nrf_hit_gradients needs a row-major hit frame (one shard, tile_major 0)");
  if (hits->n_views < 1 || hits->view_stride_px < 1 || (uint64_t)hits->n_views * (uint64_t)hits->view_stride_px > 0xffffffffull)
    return fail(NRF_E_INVALID, "nrf_hit_gradients: the hit frame's n_views * view_stride_px must be 1 .. 2^32 - 1");
  if (rays->rays_per_view < 1 || rays->rays_per_view > (uint64_t)hits->view_stride_px)
    return fail(NRF_E_INVALID, "nrf_hit_gradients: rays_per_view must be 1 .. the hit frame's view_stride_px");
  PointsArgs A;
  A.hits = (const float*)hits->rgba;
  A.rays_o = (const float*)rays->rays_o;
  A.rays_d = (const float*)rays->rays_d;
  A.n = (uint32_t)((uint64_t)hits->n_views * (uint64_t)hits->view_stride_px);
  A.stride_px = (uint32_t)hits->view_stride_px;
  A.per_view = (uint32_t)rays->rays_per_view;
  A.bound = c->desc.bound;
  A.h = h;
  A.inv2h = points_inv2h(h);
  A.opacity = opacity;
  A.frac = frac;
  A.out = (float*)out;
  A.pos = (float*)pos;
  HIP_TRY(launch_points(c->dm, POINTS_HIT_GRADIENT, A, st));
  STAGE_EPILOGUE();
}

// Mesh extraction (nrf_kernels_points.hip: the lattice mode; nrf_kernels_mesh.hip: the polygoniser; the arithmetic and the refusals
// are nrf_mesh_plan.h's).  Like the point queries: no slot of the 16-call ring, no statistics, no frame buffer.
static const char* lattice_refusal(const nrf_lattice* l, MeshLattice& L) {
  if (!l) return "null lattice";
  if (l->reserved != 0) return "nrf_lattice: reserved must be 0";
  if (!mesh_lattice_valid(l->origin, l->cell, l->dims))
    return "nrf_lattice: every dimension >= 2, at most 2^27 points, finite cells > 0 and a finite origin";
  for (int k = 0; k < 3; ++k) L.origin[k] = l->origin[k], L.cell[k] = l->cell[k], L.dims[k] = l->dims[k];
  return nullptr;
}

static hipError_t launch_lattice_sigma(const nrf_context* c, const MeshLattice& L, float* sigma, hipStream_t st) {
  return launch_points_lattice(c->dm, L, c->desc.bound, sigma, st);
}

int nrf_density_lattice(nrf_context* c, const nrf_lattice* lattice, void* sigma, void* stream) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  MeshLattice L;
  if (const char* why = lattice_refusal(lattice, L)) return fail(NRF_E_INVALID, why);
  if (!sigma) return fail(NRF_E_INVALID, "null argument");
  STAGE_PROLOGUE();
  HIP_TRY(launch_lattice_sigma(c, L, (float*)sigma, st));
  STAGE_EPILOGUE();
}

int nrf_extract_mesh(nrf_context* c, const nrf_lattice* lattice, float iso, const void* sigma, void* stream, nrf_mesh* out) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  MeshLattice L;
  if (const char* why = lattice_refusal(lattice, L)) return fail(NRF_E_INVALID, why);
  if (!out) return fail(NRF_E_INVALID, "null argument");
  if (!mesh_iso_valid(iso)) return fail(NRF_E_INVALID, "nrf_extract_mesh: iso must be finite");
  if (!sigma && !c->model_loaded) return fail(NRF_E_STATE, "no model loaded and no sigma given");
  int rc = set_device(c);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  auto& m = c->mesh;
  m.have = false;
  m.have_attr = false;
  m.have_texture = false;
  m.have_parts = false;
  m.have_brackets = false;
  m.have_simplify = false;
  const uint64_t n = mesh_points(L);
  if ((rc = grow_mesh_buffer(&m.codes, m.cap_codes, n * 4))) return rc;
  if ((rc = grow_mesh_buffer(&m.vbase, m.cap_vbase, n * 4))) return rc;
  if ((rc = grow_mesh_buffer(&m.tbase, m.cap_tbase, n * 4))) return rc;
  if ((rc = grow_mesh_buffer(&m.partials, m.cap_partials, (uint64_t)mesh_scan_tiles((uint32_t)n) * 8))) return rc;
  if (!m.totals) HIP_TRY(hipMalloc((void**)&m.totals, 16));
  const float* s = (const float*)sigma;
  if (!s) {
    if ((rc = grow_mesh_buffer(&m.sigma, m.cap_sigma, mesh_sigma_bytes(n)))) return rc;
    HIP_TRY(launch_lattice_sigma(c, L, (float*)m.sigma, st));
    s = (const float*)m.sigma;
  }
  // count and scan; the sizes reach the host; emit into buffers of exactly checked sizes; the flag reaches the host
  uint32_t host[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemsetAsync(m.totals, 0, 16, st));
  HIP_TRY(launch_mesh_count(L, s, iso, (uint32_t*)m.codes, (uint32_t*)m.vbase, (uint32_t*)m.tbase, m.partials, m.totals, st));
  HIP_TRY(hipMemcpyAsync(host, m.totals, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint32_t nv = host[0], nt = host[1];
  if ((rc = grow_mesh_buffer(&m.vertices, m.cap_vertices, mesh_vertex_bytes(nv)))) return rc;
  if ((rc = grow_mesh_buffer(&m.triangles, m.cap_triangles, mesh_triangle_bytes(nt)))) return rc;
  HIP_TRY(launch_mesh_emit(L, s, iso, (const uint32_t*)m.codes, (const uint32_t*)m.vbase, (const uint32_t*)m.tbase, nv, nt, (float*)m.vertices,
                           (uint32_t*)m.triangles, m.totals + 2, st));
  // the edge words, while codes and vbase are the extraction's (nrf_mesh_components reuses them)
  if ((rc = grow_mesh_buffer(&m.edges, m.cap_edges, refine_edge_bytes(nv)))) return rc;
  HIP_TRY(launch_mesh_edges(L, (const uint32_t*)m.codes, (const uint32_t*)m.vbase, nv, (uint32_t*)m.edges, m.totals + 2, st));
  HIP_TRY(hipMemcpyAsync(host, m.totals, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (host[2]) return fail(NRF_E_HIP, "nrf_extract_mesh: the count and the emit pass disagree (the sigmas changed during the call); writes were dropped");
  m.n_vertices = nv;
  m.n_triangles = nt;
  m.have = true;
  m.sigma_used = const_cast<float*>(s);
  m.lattice = L;
  m.iso = iso;
  out->n_vertices = nv;
  out->n_triangles = nt;
  out->vertices = nv ? m.vertices : nullptr;
  out->triangles = nt ? m.triangles : nullptr;
  out->sigma = m.sigma_used;
  return NRF_OK;
}

int nrf_read_mesh(nrf_context* c, float* vertices, uint32_t* triangles) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!c->mesh.have) return fail(NRF_E_STATE, "no mesh extracted yet (call nrf_extract_mesh first)");
  int rc = set_device(c);
  if (rc) return rc;
  const auto& m = c->mesh;
  if (vertices && m.n_vertices) HIP_TRY(hipMemcpy(vertices, m.vertices, (size_t)mesh_vertex_bytes(m.n_vertices), hipMemcpyDeviceToHost));
  if (triangles && m.n_triangles) HIP_TRY(hipMemcpy(triangles, m.triangles, (size_t)mesh_triangle_bytes(m.n_triangles), hipMemcpyDeviceToHost));
  return NRF_OK;
}

// Connected components and the filter by component size (nrf_kernels_meshcc.hip; the definition is nrf_meshcc_plan.h's).  Like the
// extraction: no slot of the 16-call ring, no statistics, no frame buffer, and no model.
namespace {
// the scan workspace of the extraction, for n code words (its contents are the extraction's no longer)
int grow_mesh_scan(nrf_context* c, uint64_t n) {
  auto& m = c->mesh;
  int rc;
  if ((rc = grow_mesh_buffer(&m.codes, m.cap_codes, n * 4))) return rc;
  if ((rc = grow_mesh_buffer(&m.vbase, m.cap_vbase, n * 4))) return rc;
  if ((rc = grow_mesh_buffer(&m.tbase, m.cap_tbase, n * 4))) return rc;
  if ((rc = grow_mesh_buffer(&m.partials, m.cap_partials, (uint64_t)mesh_scan_tiles((uint32_t)n) * 8))) return rc;
  if (!m.cc_words) HIP_TRY(hipMalloc((void**)&m.cc_words, 32));
  return NRF_OK;
}

MeshccArgs meshcc_args(const nrf_context* c) {
  const auto& m = c->mesh;
  MeshccArgs A;
  A.n_vertices = (uint32_t)m.n_vertices;
  A.n_triangles = (uint32_t)m.n_triangles;
  A.triangles = (const uint32_t*)m.triangles;
  A.labels = (uint32_t*)m.labels;
  A.rows = (uint32_t*)m.rows;
  A.components = (uint32_t*)m.components;
  A.n_components = (uint32_t)m.n_components;
  A.best = (unsigned long long*)m.cc_words;
  return A;
}

// labels, rows and the table of the current mesh; returns after completion
int label_mesh(nrf_context* c, hipStream_t st) {
  auto& m = c->mesh;
  m.have_parts = false;
  m.n_components = 0;
  m.n_rounds = 0;
  const uint64_t nv = m.n_vertices, nt = m.n_triangles;
  if (!nv) {
    m.have_parts = true;
    return NRF_OK;
  }
  int rc;
  if ((rc = grow_mesh_scan(c, nv > nt ? nv : nt))) return rc;
  if ((rc = grow_mesh_buffer(&m.labels, m.cap_labels, nv * 4))) return rc;
  if ((rc = grow_mesh_buffer(&m.rows, m.cap_rows, nv * 4))) return rc;
  MeshccArgs A = meshcc_args(c);
  HIP_TRY(launch_meshcc_init(A, st));
  // hook + compress until a hook lowered nothing: the flag (4 bytes) reaches the host after every round.  A changing round removes a
  // root, so n_vertices + 1 rounds are the most a mesh can take (nrf_kernels_meshcc.hip)
  uint32_t rounds = 0;
  for (;;) {
    uint32_t changed = 0;
    HIP_TRY(hipMemsetAsync(m.cc_words + 2, 0, 4, st));
    HIP_TRY(launch_meshcc_round(A, m.cc_words + 2, st));
    HIP_TRY(hipMemcpyAsync(&changed, m.cc_words + 2, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ++rounds;
    if (!changed) break;
    if (rounds > nv) return fail(NRF_E_HIP, "nrf_mesh_components: the labelling did not settle within n_vertices + 1 rounds");
  }
  // root flags -> rows (the vertex channel of the mesh scan; its triangle channel is all zeros) and the number of components
  uint32_t totals[2] = {0, 0};
  HIP_TRY(launch_meshcc_roots(A, (uint32_t*)m.codes, st));
  HIP_TRY(launch_mesh_scan((const uint32_t*)m.codes, (uint32_t)nv, (uint32_t*)m.rows, (uint32_t*)m.tbase, m.partials, m.cc_words + 4, st));
  HIP_TRY(hipMemcpyAsync(totals, m.cc_words + 4, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint64_t nc = totals[0];
  if (!nc || nc > nv) return fail(NRF_E_HIP, "nrf_mesh_components: the root count is out of range");
  if ((rc = grow_mesh_buffer(&m.components, m.cap_components, nc * 12))) return rc;
  HIP_TRY(hipMemsetAsync(m.components, 0, (size_t)nc * 12, st));
  HIP_TRY(hipMemsetAsync(m.cc_words, 0, 8, st));
  m.n_components = nc;
  A = meshcc_args(c);
  HIP_TRY(launch_meshcc_table(A, st));
  HIP_TRY(hipStreamSynchronize(st));
  m.n_rounds = rounds;
  m.have_parts = true;
  return NRF_OK;
}
}  // namespace

int nrf_mesh_components(nrf_context* c, void* stream, nrf_mesh_parts* out) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!out) return fail(NRF_E_INVALID, "null argument");
  if (!c->mesh.have) return fail(NRF_E_STATE, "no mesh extracted yet (call nrf_extract_mesh first)");
  int rc = set_device(c);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  if ((rc = label_mesh(c, st))) {
    c->mesh.have_parts = false;
    return rc;
  }
  const auto& m = c->mesh;
  out->n_components = m.n_components;
  out->labels = m.n_vertices ? m.labels : nullptr;
  out->components = m.n_components ? m.components : nullptr;
  out->n_rounds = m.n_rounds;
  out->reserved = 0;
  return NRF_OK;
}

int nrf_read_mesh_components(nrf_context* c, uint32_t* labels, uint32_t* components) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!c->mesh.have || !c->mesh.have_parts)
    return fail(NRF_E_STATE, "no components of the current mesh (call nrf_mesh_components after nrf_extract_mesh or nrf_filter_mesh)");
  int rc = set_device(c);
  if (rc) return rc;
  const auto& m = c->mesh;
  if (labels && m.n_vertices) HIP_TRY(hipMemcpy(labels, m.labels, (size_t)m.n_vertices * 4, hipMemcpyDeviceToHost));
  if (components && m.n_components) HIP_TRY(hipMemcpy(components, m.components, (size_t)m.n_components * 12, hipMemcpyDeviceToHost));
  return NRF_OK;
}

int nrf_filter_mesh(nrf_context* c, uint64_t min_triangles, uint32_t flags, void* stream, nrf_mesh* out) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!out) return fail(NRF_E_INVALID, "null argument");
  if (!meshcc_flags_valid(flags)) return fail(NRF_E_INVALID, "nrf_filter_mesh: unknown flag bit");
  auto& m = c->mesh;
  if (!m.have) return fail(NRF_E_STATE, "no mesh extracted yet (call nrf_extract_mesh first)");
  int rc = set_device(c);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  if (!m.have_parts && (rc = label_mesh(c, st))) {
    m.have_parts = false;
    return rc;
  }
  uint32_t kept[2] = {0, 0};
  if (m.n_vertices) {
    const uint64_t nv = m.n_vertices, nt = m.n_triangles, n = nv > nt ? nv : nt;
    const MeshccArgs A = meshcc_args(c);
    // keep flags; the two prefix sums; the kept sizes reach the host; scatter into second buffers of exactly checked sizes; the flag
    // reaches the host; then the second buffers ARE the mesh
    HIP_TRY(launch_meshcc_keep(A, min_triangles, flags, (uint32_t*)m.codes, st));
    HIP_TRY(launch_mesh_scan((const uint32_t*)m.codes, (uint32_t)n, (uint32_t*)m.vbase, (uint32_t*)m.tbase, m.partials, m.cc_words + 4, st));
    HIP_TRY(hipMemsetAsync(m.cc_words + 3, 0, 4, st));
    HIP_TRY(hipMemcpyAsync(kept, m.cc_words + 4, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (kept[0] > nv || kept[1] > nt) return fail(NRF_E_HIP, "nrf_filter_mesh: the kept counts exceed the mesh");
    if ((rc = grow_mesh_buffer(&m.vertices2, m.cap_vertices2, mesh_vertex_bytes(kept[0])))) return rc;
    if ((rc = grow_mesh_buffer(&m.triangles2, m.cap_triangles2, mesh_triangle_bytes(kept[1])))) return rc;
    if ((rc = grow_mesh_buffer(&m.edges2, m.cap_edges2, refine_edge_bytes(kept[0])))) return rc;
    uint32_t dropped = 0;
    HIP_TRY(launch_meshcc_scatter(A, (const float*)m.vertices, (const uint32_t*)m.codes, (const uint32_t*)m.vbase, (const uint32_t*)m.tbase, kept[0],
                                  kept[1], (float*)m.vertices2, (uint32_t*)m.triangles2, m.cc_words + 3, st, (const uint32_t*)m.edges,
                                  kept[0] ? (uint32_t*)m.edges2 : nullptr));
    HIP_TRY(hipMemcpyAsync(&dropped, m.cc_words + 3, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (dropped) return fail(NRF_E_HIP, "nrf_filter_mesh: the scan and the scatter pass disagree (the mesh changed during the call); writes were dropped");
    std::swap(m.vertices, m.vertices2);
    std::swap(m.cap_vertices, m.cap_vertices2);
    std::swap(m.triangles, m.triangles2);
    std::swap(m.cap_triangles, m.cap_triangles2);
    std::swap(m.edges, m.edges2);
    std::swap(m.cap_edges, m.cap_edges2);
    m.n_vertices = kept[0];
    m.n_triangles = kept[1];
  }
  m.have_parts = false;
  m.have_attr = false;
  m.have_texture = false;
  m.have_brackets = false;
  m.have_simplify = false;
  out->n_vertices = m.n_vertices;
  out->n_triangles = m.n_triangles;
  out->vertices = m.n_vertices ? m.vertices : nullptr;
  out->triangles = m.n_triangles ? m.triangles : nullptr;
  out->sigma = m.sigma_used;
  return NRF_OK;
}

// Point attributes (nrf_kernels_attr.hip; the arithmetic is nrf_attr_plan.h on top of nrf_points_plan.h): the stream rules of
// nrf_network, no slot of the 16-call ring, no statistics, nothing of the context's frame buffers is written.
static hipError_t launch_attributes(const nrf_context* c, const void* xyz, const void* dir, uint32_t n, float h, void* normal, void* color,
                                    hipStream_t st) {
  AttrArgs A;
  A.xyz = (const float*)xyz;
  A.dir = (const float*)dir;
  A.n = n;
  A.bound = c->desc.bound;
  A.h = h;
  A.inv2h = points_inv2h(h);
  A.normal = (float*)normal;
  A.color = (float*)color;
  return launch_attr(c->dm, A, st);
}

int nrf_point_attributes(nrf_context* c, const void* xyz, const void* dir, uint32_t n, float h, void* normal, void* color, void* stream) {
  STAGE_PROLOGUE();
  if (n && (!xyz || !normal || !color)) return fail(NRF_E_INVALID, "null argument");
  if (!points_step_valid(h, c->desc.bound)) return fail(NRF_E_INVALID, "nrf_point_attributes: h must be finite, > 0 and <= bound");
  HIP_TRY(launch_attributes(c, xyz, dir, n, h, normal, color, st));
  STAGE_EPILOGUE();
}

int nrf_mesh_attributes(nrf_context* c, float h, void* stream, nrf_mesh_attr* out) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!out) return fail(NRF_E_INVALID, "null argument");
  STAGE_PROLOGUE();  // (a mesh made from a caller's lattice on a context without a model has no network to ask: NRF_E_STATE)
  auto& m = c->mesh;
  if (!m.have) return fail(NRF_E_STATE, "no mesh extracted yet (call nrf_extract_mesh first)");
  if (!points_step_valid(h, c->desc.bound)) return fail(NRF_E_INVALID, "nrf_mesh_attributes: h must be finite, > 0 and <= bound");
  m.have_attr = false;
  const uint64_t nv = m.n_vertices;
  if (nv) {
    if ((rc = grow_mesh_buffer(&m.normals, m.cap_normals, nv * 16))) return rc;
    if ((rc = grow_mesh_buffer(&m.colors, m.cap_colors, nv * 16))) return rc;
    HIP_TRY(launch_attributes(c, m.vertices, nullptr, (uint32_t)nv, h, m.normals, m.colors, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  m.have_attr = true;
  out->n_vertices = nv;
  out->normals = nv ? m.normals : nullptr;
  out->colors = nv ? m.colors : nullptr;
  return NRF_OK;
}

int nrf_read_mesh_attributes(nrf_context* c, float* normals, float* colors) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!c->mesh.have || !c->mesh.have_attr) return fail(NRF_E_STATE, "no attributes of the current mesh (call nrf_mesh_attributes after nrf_extract_mesh)");
  int rc = set_device(c);
  if (rc) return rc;
  const auto& m = c->mesh;
  if (normals && m.n_vertices) HIP_TRY(hipMemcpy(normals, m.normals, (size_t)m.n_vertices * 16, hipMemcpyDeviceToHost));
  if (colors && m.n_vertices) HIP_TRY(hipMemcpy(colors, m.colors, (size_t)m.n_vertices * 16, hipMemcpyDeviceToHost));
  return NRF_OK;
}

// Mesh refinement (nrf_kernels_refine.hip; the definition is nrf_refine_plan.h's).  Like the extraction: no slot of the 16-call ring,
// no statistics, no frame buffer; it returns after completion, because the count of unbracketed vertices has to reach the host.
int nrf_refine_mesh(nrf_context* c, uint32_t n_steps, void* stream, nrf_mesh_refine* out) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!out) return fail(NRF_E_INVALID, "null argument");
  if (!refine_steps_valid(n_steps)) return fail(NRF_E_INVALID, "nrf_refine_mesh: n_steps must be 0 .. 16");
  STAGE_PROLOGUE();  // (a mesh made from a caller's lattice on a context without a model has no network to ask: NRF_E_STATE)
  auto& m = c->mesh;
  if (!m.have) return fail(NRF_E_STATE, "no mesh extracted yet (call nrf_extract_mesh first)");
  m.have_brackets = false;
  m.have_attr = false;
  m.have_texture = false;
  const uint64_t nv = m.n_vertices;
  uint32_t open = 0;
  if (nv) {
    if ((rc = grow_mesh_buffer(&m.brackets, m.cap_brackets, refine_bracket_bytes(nv)))) return rc;
    RefineArgs A;
    A.L = m.lattice;
    A.iso = m.iso;
    A.bound = c->desc.bound;
    A.n = (uint32_t)nv;
    A.n_steps = n_steps;
    A.edges = (const uint32_t*)m.edges;
    A.vertices = (float*)m.vertices;
    A.brackets = (float*)m.brackets;
    A.n_unbracketed = m.totals + 3;
    HIP_TRY(hipMemsetAsync(m.totals + 3, 0, 4, st));
    HIP_TRY(launch_refine(c->dm, A, st));
    HIP_TRY(hipMemcpyAsync(&open, m.totals + 3, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  m.have_brackets = true;
  out->n_vertices = nv;
  out->n_unbracketed = open;
  out->vertices = nv ? m.vertices : nullptr;
  out->edges = nv ? m.edges : nullptr;
  out->brackets = nv ? m.brackets : nullptr;
  out->n_steps = n_steps;
  out->reserved = 0;
  return NRF_OK;
}

int nrf_read_mesh_refinement(nrf_context* c, uint32_t* edges, float* brackets) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!c->mesh.have) return fail(NRF_E_STATE, "no mesh extracted yet (call nrf_extract_mesh first)");
  if (brackets && !c->mesh.have_brackets)
    return fail(NRF_E_STATE, "no brackets of the current mesh (call nrf_refine_mesh after nrf_extract_mesh or nrf_filter_mesh)");
  int rc = set_device(c);
  if (rc) return rc;
  const auto& m = c->mesh;
  if (edges && m.n_vertices) HIP_TRY(hipMemcpy(edges, m.edges, (size_t)refine_edge_bytes(m.n_vertices), hipMemcpyDeviceToHost));
  if (brackets && m.n_vertices) HIP_TRY(hipMemcpy(brackets, m.brackets, (size_t)refine_bracket_bytes(m.n_vertices), hipMemcpyDeviceToHost));
  return NRF_OK;
}

// Mesh simplification by vertex clustering (nrf_kernels_simplify.hip; the definition is nrf_simplify_plan.h's).  Like the filter: no
// slot of the 16-call ring, no statistics, no frame buffer, and no model; it returns after completion, because the sizes have to
// reach the host.
int nrf_simplify_mesh(nrf_context* c, uint32_t factor, void* stream, nrf_mesh_simplify* out) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!out) return fail(NRF_E_INVALID, "null argument");
  if (!simplify_factor_valid(factor)) return fail(NRF_E_INVALID, "nrf_simplify_mesh: factor must be 1 .. 256");
  auto& m = c->mesh;
  if (!m.have) return fail(NRF_E_STATE, "no mesh extracted yet (call nrf_extract_mesh first)");
  int rc = set_device(c);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  const uint64_t nv = m.n_vertices, nt = m.n_triangles, n = nv > nt ? nv : nt;
  uint32_t kept[2] = {0, 0};
  m.have_simplify = false;
  if (nv) {
    SimplifyArgs A;
    A.L = m.lattice;
    A.factor = factor;
    A.n_clusters = simplify_clusters(m.lattice, factor);
    A.n_vertices = (uint32_t)nv;
    A.n_triangles = (uint32_t)nt;
    if ((rc = grow_mesh_scan(c, n))) return rc;
    if ((rc = grow_mesh_buffer(&m.skeys, m.cap_skeys, simplify_key_bytes(A.n_clusters)))) return rc;
    if ((rc = grow_mesh_buffer(&m.sused, m.cap_sused, nv * 4))) return rc;
    if ((rc = grow_mesh_buffer(&m.ssurvive, m.cap_ssurvive, nt * 4))) return rc;
    if ((rc = grow_mesh_buffer(&m.vertex_map, m.cap_vertex_map, nv * 4))) return rc;
    A.vertices = (const float*)m.vertices;
    A.edges = (const uint32_t*)m.edges;
    A.triangles = (const uint32_t*)m.triangles;
    A.keys = (unsigned long long*)m.skeys;
    // the key table filled with ones, used[] with zeros; keys, flags and the two prefix sums; the kept sizes reach the host; scatter into
    // second buffers of exactly checked sizes; the flag reaches the host; then the second buffers ARE the mesh
    HIP_TRY(hipMemsetAsync(m.skeys, 0xff, (size_t)simplify_key_bytes(A.n_clusters), st));
    HIP_TRY(hipMemsetAsync(m.sused, 0, (size_t)nv * 4, st));
    HIP_TRY(launch_simplify_mark(A, (uint32_t*)m.sused, (uint32_t*)m.ssurvive, (uint32_t*)m.codes, st));
    HIP_TRY(launch_mesh_scan((const uint32_t*)m.codes, (uint32_t)n, (uint32_t*)m.vbase, (uint32_t*)m.tbase, m.partials, m.cc_words + 4, st));
    HIP_TRY(hipMemsetAsync(m.cc_words + 3, 0, 4, st));
    HIP_TRY(hipMemcpyAsync(kept, m.cc_words + 4, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (kept[0] > nv || kept[1] > nt) return fail(NRF_E_HIP, "nrf_simplify_mesh: the kept counts exceed the mesh");
    if ((rc = grow_mesh_buffer(&m.vertices2, m.cap_vertices2, mesh_vertex_bytes(kept[0])))) return rc;
    if ((rc = grow_mesh_buffer(&m.triangles2, m.cap_triangles2, mesh_triangle_bytes(kept[1])))) return rc;
    if ((rc = grow_mesh_buffer(&m.edges2, m.cap_edges2, refine_edge_bytes(kept[0])))) return rc;
    if ((rc = grow_mesh_buffer(&m.sources, m.cap_sources, (uint64_t)kept[0] * 4))) return rc;
    uint32_t dropped = 0;
    HIP_TRY(launch_simplify_scatter(A, (const uint32_t*)m.codes, (const uint32_t*)m.vbase, (const uint32_t*)m.tbase, kept[0], kept[1],
                                    (float*)m.vertices2, (uint32_t*)m.edges2, (uint32_t*)m.sources, (uint32_t*)m.vertex_map,
                                    (uint32_t*)m.triangles2, m.cc_words + 3, st));
    HIP_TRY(hipMemcpyAsync(&dropped, m.cc_words + 3, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (dropped)
      return fail(NRF_E_HIP, "nrf_simplify_mesh: the scan and the scatter pass disagree (the mesh changed during the call); writes were dropped");
    std::swap(m.vertices, m.vertices2);
    std::swap(m.cap_vertices, m.cap_vertices2);
    std::swap(m.triangles, m.triangles2);
    std::swap(m.cap_triangles, m.cap_triangles2);
    std::swap(m.edges, m.edges2);
    std::swap(m.cap_edges, m.cap_edges2);
    m.n_vertices = kept[0];
    m.n_triangles = kept[1];
  }
  m.n_vertices_before = nv;
  m.have_simplify = true;
  m.have_parts = false;
  m.have_attr = false;
  m.have_texture = false;
  m.have_brackets = false;
  out->n_vertices = m.n_vertices;
  out->n_triangles = m.n_triangles;
  out->n_vertices_before = nv;
  out->n_triangles_before = nt;
  out->vertices = m.n_vertices ? m.vertices : nullptr;
  out->triangles = m.n_triangles ? m.triangles : nullptr;
  out->edges = m.n_vertices ? m.edges : nullptr;
  out->sources = m.n_vertices ? m.sources : nullptr;
  out->vertex_map = nv ? m.vertex_map : nullptr;
  out->factor = factor;
  out->reserved = 0;
  return NRF_OK;
}

int nrf_read_mesh_simplification(nrf_context* c, uint32_t* sources, uint32_t* vertex_map) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!c->mesh.have || !c->mesh.have_simplify)
    return fail(NRF_E_STATE, "no simplification of the current mesh (call nrf_simplify_mesh after nrf_extract_mesh or nrf_filter_mesh)");
  int rc = set_device(c);
  if (rc) return rc;
  const auto& m = c->mesh;
  if (sources && m.n_vertices) HIP_TRY(hipMemcpy(sources, m.sources, (size_t)m.n_vertices * 4, hipMemcpyDeviceToHost));
  if (vertex_map && m.n_vertices_before) HIP_TRY(hipMemcpy(vertex_map, m.vertex_map, (size_t)m.n_vertices_before * 4, hipMemcpyDeviceToHost));
  return NRF_OK;
}

// The mesh texture (nrf_kernels_bake.hip; the definition is nrf_bake_plan.h's).  Like the attributes: no slot of the 16-call ring, no
// statistics, no frame buffer, and the mesh is only read; it returns after completion, because the count of refused texels has to
// reach the host.
static std::string bake_limit_message(const char* who, uint64_t n_triangles, uint32_t res, uint32_t width) {
  const uint32_t fit = bake_smallest_width(n_triangles, res);
  std::string msg = std::string(who) + ": the atlas of " + std::to_string(n_triangles) + " triangles at res " + std::to_string(res) + " and width " +
                    std::to_string(width) + " would be " + std::to_string(bake_height64(n_triangles, res, width)) +
                    " texels high (limits: height 16384, width * height 2^26); ";
  msg += fit ? "the smallest width that fits is " + std::to_string(fit) : std::string("no width fits at this res");
  return msg;
}

int nrf_mesh_texture_size(uint64_t n_triangles, uint32_t res, uint32_t width, uint32_t* height) {
  if (!height) return fail(NRF_E_INVALID, "null argument");
  if (!bake_params_valid(res, width)) return fail(NRF_E_INVALID, "nrf_mesh_texture_size: res must be 2 .. 256 and width res + 2 .. 16384");
  BakeLayout B;
  if (!bake_layout(n_triangles, res, width, B)) return fail(NRF_E_INVALID, bake_limit_message("nrf_mesh_texture_size", n_triangles, res, width));
  *height = B.height;
  return NRF_OK;
}

int nrf_bake_mesh_texture(nrf_context* c, uint32_t res, uint32_t width, void* stream, nrf_mesh_texture* out) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!out) return fail(NRF_E_INVALID, "null argument");
  if (!bake_params_valid(res, width)) return fail(NRF_E_INVALID, "nrf_bake_mesh_texture: res must be 2 .. 256 and width res + 2 .. 16384");
  STAGE_PROLOGUE();  // (a mesh made from a caller's lattice on a context without a model has no network to ask: NRF_E_STATE)
  auto& m = c->mesh;
  if (!m.have) return fail(NRF_E_STATE, "no mesh extracted yet (call nrf_extract_mesh first)");
  const uint64_t nt = m.n_triangles;
  BakeLayout B;
  if (!bake_layout(nt, res, width, B)) return fail(NRF_E_INVALID, bake_limit_message("nrf_bake_mesh_texture", nt, res, width));
  m.have_texture = false;
  uint32_t refused = 0;
  if (nt) {
    if ((rc = grow_mesh_buffer(&m.texels, m.cap_texels, bake_texel_bytes(B)))) return rc;
    if ((rc = grow_mesh_buffer(&m.rgba8, m.cap_rgba8, bake_rgba8_bytes(B)))) return rc;
    if ((rc = grow_mesh_buffer(&m.uvs, m.cap_uvs, bake_uv_bytes(nt)))) return rc;
    if ((rc = grow_mesh_buffer(&m.bake_count, m.cap_bake_count, 4))) return rc;
    BakeArgs A;
    A.B = B;
    A.n_vertices = (uint32_t)m.n_vertices;
    A.bound = c->desc.bound;
    A.vertices = (const float*)m.vertices;
    A.triangles = (const uint32_t*)m.triangles;
    A.texels = (float*)m.texels;
    A.rgba8 = (uint32_t*)m.rgba8;
    A.n_refused = (uint32_t*)m.bake_count;
    // both planes and the counter cleared; the texels; the UVs; the count reaches the host
    HIP_TRY(hipMemsetAsync(m.texels, 0, (size_t)bake_texel_bytes(B), st));
    HIP_TRY(hipMemsetAsync(m.rgba8, 0, (size_t)bake_rgba8_bytes(B), st));
    HIP_TRY(hipMemsetAsync(m.bake_count, 0, 4, st));
    HIP_TRY(launch_bake(c->dm, A, st));
    HIP_TRY(launch_bake_uvs(B, (float*)m.uvs, st));
    HIP_TRY(hipMemcpyAsync(&refused, m.bake_count, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  m.texture = B;
  m.have_texture = true;
  out->width = B.width;
  out->height = B.height;
  out->res = B.res;
  out->cols = B.cols;
  out->n_triangles = nt;
  out->n_refused = refused;
  out->texels = nt ? m.texels : nullptr;
  out->rgba8 = nt ? m.rgba8 : nullptr;
  out->uvs = nt ? m.uvs : nullptr;
  return NRF_OK;
}

int nrf_read_mesh_texture(nrf_context* c, float* texels, uint32_t* rgba8, float* uvs) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!c->mesh.have || !c->mesh.have_texture)
    return fail(NRF_E_STATE, "no texture of the current mesh (call nrf_bake_mesh_texture after the last call that changed the mesh)");
  int rc = set_device(c);
  if (rc) return rc;
  const auto& m = c->mesh;
  const BakeLayout& B = m.texture;
  if (!B.n_triangles) return NRF_OK;
  if (texels) HIP_TRY(hipMemcpy(texels, m.texels, (size_t)bake_texel_bytes(B), hipMemcpyDeviceToHost));
  if (rgba8) HIP_TRY(hipMemcpy(rgba8, m.rgba8, (size_t)bake_rgba8_bytes(B), hipMemcpyDeviceToHost));
  if (uvs) HIP_TRY(hipMemcpy(uvs, m.uvs, (size_t)bake_uv_bytes(B.n_triangles), hipMemcpyDeviceToHost));
  return NRF_OK;
}

int nrf_generate_rays(nrf_context* c, const float cam[4], const float pose[16], void* rays_o, void* rays_d, void* nears,
                      void* fars, void* stream) {
  STAGE_PROLOGUE();
  if (!cam || !pose) return fail(NRF_E_INVALID, "null argument");
  if (c->W <= 0) return fail(NRF_E_STATE, "set_resolution has not been called");
  FrameParams P;
  fill_frame_params(c, cam, pose, P);
  HIP_TRY(launch_generate_rays(c->dm, P, rays_o, rays_d, nears, fars, st));
  STAGE_EPILOGUE();
}

int nrf_generate_rays_host(nrf_context* c, const float cam[4], const float pose[16], float* rays_o, float* rays_d,
                           float* nears, float* fars) {
  int rc = need_model(c);
  if (rc) return rc;
  if (c->W <= 0) return fail(NRF_E_STATE, "set_resolution has not been called");
  const size_t n = (size_t)c->W * c->H;
  void* buf = nullptr;
  HIP_TRY(hipMalloc(&buf, n * 8 * sizeof(float)));
  float* d_o = (float*)buf;
  float* d_d = d_o + 3 * n;
  float* d_n = d_d + 3 * n;
  float* d_f = d_n + n;
  rc = nrf_generate_rays(c, cam, pose, d_o, d_d, d_n, d_f, nullptr);
  hipError_t e = hipSuccess;
  if (!rc && rays_o) e = hipMemcpy(rays_o, d_o, n * 12, hipMemcpyDeviceToHost);
  if (!rc && e == hipSuccess && rays_d) e = hipMemcpy(rays_d, d_d, n * 12, hipMemcpyDeviceToHost);
  if (!rc && e == hipSuccess && nears) e = hipMemcpy(nears, d_n, n * 4, hipMemcpyDeviceToHost);
  if (!rc && e == hipSuccess && fars) e = hipMemcpy(fars, d_f, n * 4, hipMemcpyDeviceToHost);
  (void)hipFree(buf);
  if (rc) return rc;
  if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
  return NRF_OK;
}

// The motion vectors of a static scene (nrf_temporal_plan.h: motion_vector; nrf_kernels_temporal.hip: motion_kernel).  Both poses go
// through motion_camera (nerf_matrix_to_ngp's operations) with the loaded model's scale, as nrf_render's do (1 while no model is loaded).  No model is needed, no slot
// of the calls in flight is taken and the statistics are left alone.
int nrf_motion_vectors(nrf_context* c, const nrf_motion* m, void* motion_f32x2, void* stream) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  if (!m || !motion_f32x2 || !m->rays_o || !m->rays_d || !m->rgba || !m->depth_t) return fail(NRF_E_INVALID, "null argument");
  if (m->reserved != 0) return fail(NRF_E_INVALID, "reserved field set");
  MotionPlan M;
  if (!motion_plan(m->width, m->height, m->out_width, m->out_height, m->min_alpha, M))
    return fail(NRF_E_INVALID, "bad resolutions (in <= out <= 8 * in and out <= 16384 per axis) or min_alpha not in (0, 1]");
  int rc = set_device(c);
  if (rc) return rc;
  const float scale = c->model_loaded ? c->desc.scale : 1.0f;
  motion_camera(m->pose, scale, m->cam, M.cur);
  motion_camera(m->prev_pose, scale, m->prev_cam, M.prev);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY((hipError_t)launch_motion(M, m->rays_o, m->rays_d, m->rgba, m->depth_t, motion_f32x2, st));
  if (!stream) HIP_TRY(hipStreamSynchronize(st));
  return NRF_OK;
}

int nrf_march(nrf_context* c, const void* rays_o, const void* rays_d, const void* rays_t, const void* fars, uint32_t n,
              uint32_t n_step, void* xyzs, void* dirs, void* deltas, void* stream) {
  STAGE_PROLOGUE();
  if (n_step < 1 || n_step > 8) return fail(NRF_E_INVALID, "n_step must be 1..8");
  if (n && (!rays_o || !rays_d || !rays_t || !fars || !xyzs || !dirs || !deltas)) return fail(NRF_E_INVALID, "null argument");
  HIP_TRY(launch_march(c->dm, c->opt.dt_gamma, rays_o, rays_d, rays_t, fars, n, n_step, xyzs, dirs, deltas, st, (uint32_t)c->opt.perturb));
  STAGE_EPILOGUE();
}

int nrf_composite(nrf_context* c, const void* sigmas, const void* rgbs, const void* deltas, uint32_t n, uint32_t n_step,
                  void* rays_t, void* state, void* stream) {
  if (!c) return fail(NRF_E_INVALID, "null context");
  int rc = set_device(c);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  if (n_step < 1 || n_step > 8) return fail(NRF_E_INVALID, "n_step must be 1..8");
  if (n && (!sigmas || !rgbs || !deltas || !rays_t || !state)) return fail(NRF_E_INVALID, "null argument");
  HIP_TRY(launch_composite(sigmas, rgbs, deltas, n, n_step, rays_t, state, st));
  STAGE_EPILOGUE();
}

}  // extern "C"
