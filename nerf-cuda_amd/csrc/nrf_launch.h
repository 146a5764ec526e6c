// nrf_launch.h -- host-callable launchers implemented in nrf_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "nrf_bake_plan.h"  // BakeLayout
#include "nrf_grid_plan.h"  // persistent_lds_total: the sum plan_grid and launch_render share
#include "nrf_mesh_plan.h"  // MeshLattice

namespace nrf {
// Instances of the render kernel (nrf_render.h), one id for host and device code.  DevModel::net renders the frames;
// DevModel::stage (NET_HOT, NET_WIDE or NET_GENERIC) runs the stage entry points, the per-strip kernel and the density-grid
// generation, and renders the frames when the model's own instance does not fit (nrf_model_plan.h plan_model, nrf_api.hip plan_grid).
// NET_W16 / NET_W32 / NET_W128: the register-resident instance for the other widths of tcnn's FullyFusedMLP (persistent kernel only)
// NET_WIDE_SH: the wide form for SphericalHarmonics of degree 5..8 (32..64 direction values): the entries beyond the first sixteen
// are computed once per ray into an LDS row (not per sample in-lane as for Frequency) -- persistent kernel only
// NET_DEPTH: 64 neurons with other numbers of hidden layers than base.json's 1 + 2 (mlp_tiles_depth) -- persistent kernel only
// NET_ACT (round 6): the same with hidden activations other than ReLU (Squareplus, Softplus, Sigmoid, Exponential, None: activate_native
// on the fp32 accumulators) -- 12 waves per workgroup: the activation sequences need the registers
// NET_GRID1 / 2 / 4 / 8: base.json's MLPs behind another grid -- F = 1, F = 2 with fewer than 16 levels, F = 4 / 8 with up to 32
// features in all, Linear, Smoothstep or Nearest (grid_features) -- persistent kernel only
enum : int { NET_HOT = 0, NET_GENERIC = 1, NET_WIDE = 2, NET_W16 = 3, NET_W32 = 4, NET_W128 = 5, NET_WIDE_SH = 6, NET_DEPTH = 7,
             NET_GRID2 = 8, NET_GRID4 = 9, NET_GRID8 = 10, NET_GRID1 = 11, NET_ACT = 12 };
__host__ __device__ constexpr int net_grid_f(int net) {
  return net == NET_GRID2 ? 2 : (net == NET_GRID4 ? 4 : (net == NET_GRID8 ? 8 : (net == NET_GRID1 ? 1 : 0)));
}
__host__ __device__ constexpr int net_width(int net) { return net == NET_W16 ? 16 : (net == NET_W32 ? 32 : (net == NET_W128 ? 128 : 64)); }

// Gather plan: the form of each of a sample's four gather steps (levels 4 jl .. 4 jl + 3) as a COMPILE-TIME parameter of the hot
// path.  GATHER_RUNTIME (the default of every template) selects each step's form at run time from DevModel::quad_mask / quad_far /
// uni_modes (gather_step); a static plan names the four forms, so that the tile program has no control flow between a sample's
// loads -- behind the run-time diamonds the compiler drains the memory counter in front of every step but the first
// (profiles/r07/gather_plan_listing.txt).  Static plans exist for the NET_HOT persistent kernel only (nrf_kernels_hot_*.hip);
// plan_model (nrf_model_plan.h: gather_plan_of) picks one when the model's steps have exactly its forms.
enum : uint32_t { GFORM_MIXED = 0, GFORM_DENSE = 1, GFORM_HASHED = 2, GFORM_QUAD = 3, GFORM_QUAD_FAR = 4 };  // (0..2: uni_modes' values)
__host__ __device__ constexpr uint32_t gather_plan(uint32_t f0, uint32_t f1, uint32_t f2, uint32_t f3) {
  return 0x10000u | f0 | (f1 << 4) | (f2 << 8) | (f3 << 12);
}
__host__ __device__ constexpr uint32_t gather_form(uint32_t plan, int jl) { return (plan >> (4 * jl)) & 15u; }
constexpr uint32_t GATHER_RUNTIME = 0;
constexpr uint32_t GATHER_QQFH = gather_plan(GFORM_QUAD, GFORM_QUAD, GFORM_QUAD_FAR, GFORM_HASHED);  // base.json's grid, default copy budget
constexpr uint32_t GATHER_QQHH = gather_plan(GFORM_QUAD, GFORM_QUAD, GFORM_HASHED, GFORM_HASHED);    // near copies only (about 100 .. 256 MB)
constexpr uint32_t GATHER_DMHH = gather_plan(GFORM_DENSE, GFORM_MIXED, GFORM_HASHED, GFORM_HASHED);  // no copies
// the plan of a model's steps: one of the three static plans when `own` is NET_HOT and the forms match, else GATHER_RUNTIME
inline uint32_t gather_plan_of(int own, uint32_t n_levels, uint32_t uni_modes, uint32_t quad_mask, uint32_t quad_far) {
  if (own != NET_HOT || n_levels != 16) return GATHER_RUNTIME;
  uint32_t f[4];
  for (int jl = 0; jl < 4; ++jl)
    f[jl] = ((quad_mask >> (4 * jl)) & 1u) ? (((quad_far >> jl) & 1u) ? GFORM_QUAD_FAR : GFORM_QUAD) : ((uni_modes >> (2 * jl)) & 3u);
  const uint32_t plan = gather_plan(f[0], f[1], f[2], f[3]);
  return plan == GATHER_QQFH || plan == GATHER_QQHH || plan == GATHER_DMHH ? plan : GATHER_RUNTIME;
}

struct DevModel;
struct FrameParams;
struct ViewBatch;

// one launch for VB.n_views (<= MAX_VIEWS) cameras; blocks_per_view is filled in by the launcher
// the persistent kernel's work-queue counters follow the statistics counters (counters + COUNTER_BYTES); queues_are_zero:
// the caller has just cleared them together with the statistics
constexpr int RENDER_QUEUE_BYTES = 8 * 4;
constexpr int WIDE_GENERIC_MARCH_WAVES = 8;  // waves of the persistent workgroup of NET_WIDE with the generic march (nrf_render.h persist_waves)
hipError_t launch_render(const DevModel& M, const FrameParams& P, const ViewBatch& VB, void* rgba, void* depth, void* counters,
                         hipStream_t st, bool first_launch, unsigned* plan = nullptr, unsigned plan_cap = 0,
                         const float* step_tab = nullptr, int step_n = 0);  // the launch's step table (device; nrf_step_plan.h), null: none
// a call's plan buffer (plan_price_kernel / plan_sort_kernel): 4 header words + a price and an order entry per queue position
constexpr unsigned PLAN_CAP = 60u * 1024u;  // queue positions (strips) of a launch that may be planned (its last workgroup keeps a byte per position in LDS)
constexpr size_t PLAN_BYTES = (4 + 2 * (size_t)PLAN_CAP) * 4;
// Builds the cell-major quad copy of one level of an F = 2 grid (nrf_device.h level_gather_quad) on the device: table = the level's
// entries in the reference order, quads = res * res * (res + 1) 16-byte entries.
hipError_t launch_build_quads(const void* table, uint32_t res, uint32_t size, bool hashed, void* quads, hipStream_t st);
hipError_t launch_encode_grid(const DevModel& M, const void* pos01, uint32_t n, void* out, hipStream_t st, bool fast_interp = false);
hipError_t launch_encode_dir(const DevModel& M, const void* dir01, uint32_t n, void* out, hipStream_t st);
hipError_t launch_mlp_forward(const DevModel& M, const void* feat, const void* dirfeat, uint32_t n, void* out, uint32_t repeat,
                              hipStream_t st);
hipError_t launch_network(const DevModel& M, const void* xyz, const void* dir, uint32_t n, void* sigma, void* rgb, hipStream_t st);
// Point queries (nrf_kernels_points.hip, arithmetic: nrf_points_plan.h): sigma of the density network alone at points
// (POINTS_VALUE), its central differences (POINTS_GRADIENT), the same at the hits of an nrf_ray_hits frame (POINTS_HIT_GRADIENT).
// Launch sizes and LDS are launch_network's for the model's stage instance.
struct PointsArgs {
  const float* xyz = nullptr;     // VALUE / GRADIENT: [n][3]
  const float* hits = nullptr;    // HIT_GRADIENT: the frame's records [n][4], n = n_views * stride_px pixels
  const float* rays_o = nullptr;  // HIT_GRADIENT: [n_views][per_view][3]
  const float* rays_d = nullptr;
  uint32_t n = 0;
  uint32_t stride_px = 1, per_view = 0;  // HIT_GRADIENT: pixel i is pixel i % stride_px of view i / stride_px; it has a ray if that is < per_view
  float bound = 0.f, h = 0.f, inv2h = 0.f, opacity = 0.f, frac = 0.f;
  float* sigma = nullptr;  // VALUE: [n]
  float* out = nullptr;    // GRADIENT / HIT_GRADIENT: [n][4] = (g_x, g_y, g_z, sigma)
  float* pos = nullptr;    // HIT_GRADIENT: [n][4] = (x, y, z, tq)
};
hipError_t launch_points(const DevModel& M, int mode, const PointsArgs& A, hipStream_t st);
// POINTS_VALUE at the mesh_points(L) points of a lattice (points_lattice_kernel): sigma [nx][ny][nz]; no position array is read
hipError_t launch_points_lattice(const DevModel& M, const MeshLattice& L, float bound, float* sigma, hipStream_t st);
// Point attributes (nrf_kernels_attr.hip, arithmetic: nrf_attr_plan.h on top of nrf_points_plan.h): the unit normal of the density
// and the colour of the full network at points, seven network passes per chunk in one launch.  dir == nullptr: a point is looked at
// along d = -n.  Launch sizes and LDS are launch_network's for the model's stage instance.
struct AttrArgs {
  const float* xyz = nullptr;  // [n][3]
  const float* dir = nullptr;  // [n][3] or nullptr
  uint32_t n = 0;
  float bound = 0.f, h = 0.f, inv2h = 0.f;
  float* normal = nullptr;  // [n][4] = (n_x, n_y, n_z, sigma)
  float* color = nullptr;   // [n][4] = (r, g, b, |g|)
};
hipError_t launch_attr(const DevModel& M, const AttrArgs& A, hipStream_t st);
// Mesh extraction (nrf_kernels_mesh.hip, arithmetic: nrf_mesh_plan.h) on a lattice of n = mesh_points(L) sigmas:
//   launch_mesh_count  codes[n] (mesh_count_point), then vbase[n] / tbase[n] = the exclusive prefix sums of the codes' vertex and
//                      triangle counts and totals[0 .. 1] = the sums; partials: mesh_scan_tiles(n) uint2 of workspace
//   launch_mesh_emit   vertices [n_vertices][3] and triangles [n_triangles][3] at the scanned offsets; *flag is set to 1 when a write
//                      was dropped because it would have fallen outside those counts
constexpr uint32_t MESH_SCAN_TILE = 2048;  // lattice points per workgroup of the scan: 256 lanes x 8
inline uint32_t mesh_scan_tiles(uint32_t n) { return (n + MESH_SCAN_TILE - 1) / MESH_SCAN_TILE; }
hipError_t launch_mesh_count(const MeshLattice& L, const float* sigma, float iso, uint32_t* codes, uint32_t* vbase, uint32_t* tbase,
                             void* partials, uint32_t* totals, hipStream_t st);
hipError_t launch_mesh_emit(const MeshLattice& L, const float* sigma, float iso, const uint32_t* codes, const uint32_t* vbase,
                            const uint32_t* tbase, uint32_t n_vertices, uint32_t n_triangles, float* vertices, uint32_t* triangles,
                            uint32_t* flag, hipStream_t st);
//   launch_mesh_scan   the scan of launch_mesh_count by itself, over any n > 0 code words: vbase[n] / tbase[n] = the exclusive prefix
//                      sums of mesh_code_vertices / mesh_code_triangles of the codes, totals[0 .. 1] = the sums
hipError_t launch_mesh_scan(const uint32_t* codes, uint32_t n, uint32_t* vbase, uint32_t* tbase, void* partials, uint32_t* totals,
                            hipStream_t st);
//   launch_mesh_edges  edges [n_vertices] = the edge word (p << 3) | m of every vertex (nrf_refine_plan.h), from the codes and vbase of
//                      launch_mesh_count while they are valid; *flag as launch_mesh_emit has it
hipError_t launch_mesh_edges(const MeshLattice& L, const uint32_t* codes, const uint32_t* vbase, uint32_t n_vertices, uint32_t* edges,
                             uint32_t* flag, hipStream_t st);
// Mesh refinement (nrf_kernels_refine.hip, arithmetic: nrf_refine_plan.h): every vertex moves along the lattice edge its edge word names
// onto the iso value of the density network, n_steps bisections and a secant step, n_steps + 2 network passes per chunk in one launch.
// Launch sizes and LDS are launch_points' for the model's stage instance.
struct RefineArgs {
  MeshLattice L;                      // the lattice and the iso of the extraction
  float iso = 0.f, bound = 0.f;
  uint32_t n = 0, n_steps = 0;
  const uint32_t* edges = nullptr;    // [n]
  float* vertices = nullptr;          // [n][3], rewritten in place where the edge brackets iso
  float* brackets = nullptr;          // [n][4] = (lo, hi, s_lo, s_hi)
  uint32_t* n_unbracketed = nullptr;  // += the vertices left as they were (zeroed by the caller)
};
hipError_t launch_refine(const DevModel& M, const RefineArgs& A, hipStream_t st);
// Connected components and the filter by component size of an indexed mesh (nrf_kernels_meshcc.hip, definition: nrf_meshcc_plan.h);
// n_vertices > 0.  Every launch is a streaming pass that needs nothing another workgroup writes during it.
//   launch_meshcc_init      parent[v] = v
//   launch_meshcc_round     hook over the triangles (*changed = 1 when an atomic minimum lowered a parent), then compress over the vertices
//   launch_meshcc_roots     codes[v] = a scan code word whose vertex channel is 1 where parent[v] == v (launch_mesh_scan makes the rows of it)
//   launch_meshcc_table     components [n_components][3] (zeroed by the caller) = (label, n_vertices, n_triangles) by integer atomic adds,
//                           then *best = the maximum of meshcc_key over the rows (zeroed by the caller)
//   launch_meshcc_keep      codes[i], i < max(n_vertices, n_triangles): the keep flags of vertex i and triangle i as a scan code word
//   launch_meshcc_scatter   the kept vertices and the remapped kept triangles into second buffers of kept_vertices / kept_triangles
//                           elements; *flag is set to 1 when a write was dropped because it would have fallen outside those counts.
//                           edges / edges_out (both or neither): the kept vertices' edge words travel with them (nrf_refine_plan.h)
struct MeshccArgs {
  uint32_t n_vertices = 0, n_triangles = 0;
  const uint32_t* triangles = nullptr;  // [n_triangles][3]
  uint32_t* labels = nullptr;           // [n_vertices]: parent[] while the labelling runs, label[] after it
  uint32_t* rows = nullptr;             // [n_vertices]: the number of roots below v
  uint32_t* components = nullptr;       // [n_components][3]
  uint32_t n_components = 0;
  unsigned long long* best = nullptr;
};
hipError_t launch_meshcc_init(const MeshccArgs& A, hipStream_t st);
hipError_t launch_meshcc_round(const MeshccArgs& A, uint32_t* changed, hipStream_t st);
hipError_t launch_meshcc_roots(const MeshccArgs& A, uint32_t* codes, hipStream_t st);
hipError_t launch_meshcc_table(const MeshccArgs& A, hipStream_t st);
hipError_t launch_meshcc_keep(const MeshccArgs& A, uint64_t min_triangles, uint32_t flags, uint32_t* codes, hipStream_t st);
hipError_t launch_meshcc_scatter(const MeshccArgs& A, const float* vertices, const uint32_t* codes, const uint32_t* vnew, const uint32_t* tnew,
                                 uint32_t kept_vertices, uint32_t kept_triangles, float* vertices_out, uint32_t* triangles_out, uint32_t* flag,
                                 hipStream_t st, const uint32_t* edges = nullptr, uint32_t* edges_out = nullptr);
// Simplification of an indexed mesh by vertex clustering on the extraction's lattice (nrf_kernels_simplify.hip, definition:
// nrf_simplify_plan.h); n_vertices > 0.  Every launch is a streaming pass that needs nothing another workgroup writes during it.
//   launch_simplify_mark     the key pass (one 64-bit atomic minimum per vertex into keys, which the caller has filled with ones), the
//                            triangle pass (survive[t], and used[rep] = 1 for a survivor; used zeroed by the caller) and
//                            codes[i], i < max(n_vertices, n_triangles): used[i] and survive[i] as a scan code word
//   launch_simplify_scatter  kept vertices, their edge words and sources, vertex_map [n_vertices] and the remapped surviving triangles
//                            into second buffers of kept_vertices / kept_triangles elements; *flag is set to 1 when a write was dropped
//                            because it would have fallen outside those counts
struct SimplifyArgs {
  MeshLattice L;                         // the lattice of the extraction
  uint32_t factor = 0, n_clusters = 0;   // n_clusters = simplify_clusters(L, factor)
  uint32_t n_vertices = 0, n_triangles = 0;
  const float* vertices = nullptr;       // [n_vertices][3]
  const uint32_t* edges = nullptr;       // [n_vertices]
  const uint32_t* triangles = nullptr;   // [n_triangles][3]
  unsigned long long* keys = nullptr;    // [n_clusters]
};
hipError_t launch_simplify_mark(const SimplifyArgs& A, uint32_t* used, uint32_t* survive, uint32_t* codes, hipStream_t st);
hipError_t launch_simplify_scatter(const SimplifyArgs& A, const uint32_t* codes, const uint32_t* vnew, const uint32_t* tnew, uint32_t kept_vertices,
                                   uint32_t kept_triangles, float* vertices_out, uint32_t* edges_out, uint32_t* sources, uint32_t* vertex_map,
                                   uint32_t* triangles_out, uint32_t* flag, hipStream_t st);
// The mesh texture (nrf_kernels_bake.hip, definition: nrf_bake_plan.h): every texel of every pair's cell is one work item, a lane makes
// its position and its direction itself from its triangle's three vertices, ONE full network pass per chunk of 64 texels.  Launch
// sizes and LDS are launch_network's for the model's stage instance.  The caller has cleared texels and rgba8 on the same stream:
// the kernel writes accepted texels only.  launch_bake_uvs: one thread per triangle.
struct BakeArgs {
  BakeLayout B;
  uint32_t n_vertices = 0;
  float bound = 0.f;
  const float* vertices = nullptr;      // [n_vertices][3]
  const uint32_t* triangles = nullptr;  // [B.n_triangles][3]
  float* texels = nullptr;              // [B.height][B.width][4] = (r, g, b, sigma)
  uint32_t* rgba8 = nullptr;            // [B.height][B.width]
  uint32_t* n_refused = nullptr;        // += the owned texels the guard refused
};
hipError_t launch_bake(const DevModel& M, const BakeArgs& A, hipStream_t st);
hipError_t launch_bake_uvs(const BakeLayout& B, float* uvs, hipStream_t st);
hipError_t launch_density_positions(uint32_t H, float k, void* xyz, void* dir, hipStream_t st);
hipError_t launch_density_update(const void* sigma, uint32_t n, float decay, int n_iterations, void* grid, hipStream_t st);
hipError_t launch_generate_rays(const DevModel& M, const FrameParams& P, void* rays_o, void* rays_d, void* nears, void* fars,
                                hipStream_t st);
hipError_t launch_march(const DevModel& M, float dt_gamma, const void* rays_o, const void* rays_d, const void* rays_t,
                        const void* fars, uint32_t n, uint32_t n_step, void* xyzs, void* dirs, void* deltas, hipStream_t st,
                        uint32_t perturb = 0);
hipError_t launch_composite(const void* sigmas, const void* rgbs, const void* deltas, uint32_t n, uint32_t n_step, void* rays_t,
                            void* state, hipStream_t st);
hipError_t launch_untile(const void* gathered, int shard_count, int tiles_per_shard, int C, int W, int H, int n_views, void* out,
                         hipStream_t st);
hipError_t launch_untile_rgbd8_u8(const void* gathered, int shard_count, int tiles_per_shard, int W, int H, int n_views, void* rgb8,
                                  void* depth8, hipStream_t st);
hipError_t launch_quantize_rgbd8(const void* rgba, const void* depth, uint64_t n, void* out, hipStream_t st);
hipError_t launch_quantize(const void* rgba, const void* depth, int n, void* rgb8, void* depth8, hipStream_t st);
// The march form of a model and the waves of its persistent workgroup: ONE rule, read by plan_grid (nrf_api.hip; it sizes the
// workgroup's LDS and decides whether the model fits the persistent kernel) and by launch_render (which picks the kernel
// instance); the launch macros refuse a workgroup size other than their instance's.
enum : int { MARCH_FORM_GENERIC = 0, MARCH_FORM_UNIT = 1, MARCH_FORM_POW2 = 2 };
inline int march_form(uint32_t H, uint32_t cascade, float bound) {
  const bool pow2_h = H != 0 && (H & (H - 1)) == 0;
  int eb = 0;
  if (pow2_h && cascade == 1 && bound >= 1.0f) return MARCH_FORM_UNIT;                                  // one cascade with mip_bound == 1
  if (pow2_h && cascade > 1 && bound >= 1.0f && frexpf(bound, &eb) == 0.5f) return MARCH_FORM_POW2;    // several, power-of-two bound
  return MARCH_FORM_GENERIC;
}
// LDS schedule of the static-plan instances (round 8; NRF_LDS_PARAMS / NRF_LDS_FRAG_DEPTH may be overridden for A/B builds):
//   PLAN_LEVELS  the kernel stages, in the level table's region, a compact 32-byte block per level laid out for the form its
//                plan names (nrf_render.h: stage_plan_level) instead of LevelParams: what a lane needs of a level is ONE aligned 16-byte LDS
//                read (two for the mixed form), and a tile's four reads go out together ahead of its first gather load
//   FRAG_DEPTH   mlp_tiles reads weight fragment f + FRAG_DEPTH before the MFMAs of fragment f issue (nrf_device.h)
#ifndef NRF_LDS_PARAMS
#define NRF_LDS_PARAMS 1
#endif
#ifndef NRF_LDS_FRAG_DEPTH
#define NRF_LDS_FRAG_DEPTH 2
#endif
#ifndef NRF_LDS_FRAG_DEPTH_GENERIC
#define NRF_LDS_FRAG_DEPTH_GENERIC (NRF_LDS_FRAG_DEPTH > 1 ? 1 : NRF_LDS_FRAG_DEPTH)  // MARCH_GENERIC has no registers for two
#endif
// Pair gather of the static-plan instances (round 13; NRF_PAIR_GATHER=0 is the tile-major pass everywhere, for A/B builds): a
// pass of two full tiles gathers both tiles step by step (nrf_render.h: pair_features) -- positions and level blocks read once
// per pass, pair_window (tile, step) units in flight -- instead of tile 0's four steps, then tile 1's.  Four units are two
// steps of both tiles (128 VGPRs under GATHER_QQFH, no scratch); MARCH_GENERIC has the registers for three (four: 12 bytes of
// scratch under GATHER_QQFH).
#ifndef NRF_PAIR_GATHER
#define NRF_PAIR_GATHER 1
#endif
__host__ __device__ constexpr bool plan_levels(uint32_t gp) { return gp != GATHER_RUNTIME && NRF_LDS_PARAMS != 0; }
__host__ __device__ constexpr int pair_window(uint32_t gp, int march) {  // 0: tile-major
  return !plan_levels(gp) || NRF_PAIR_GATHER == 0 ? 0 : (march == MARCH_FORM_GENERIC ? 3 : 4);
}
__host__ __device__ constexpr int plan_frag_depth(uint32_t gp, int march) {
  return gp == GATHER_RUNTIME ? 0 : (march == MARCH_FORM_GENERIC ? NRF_LDS_FRAG_DEPTH_GENERIC : NRF_LDS_FRAG_DEPTH);
}
// waves of the persistent workgroup of instance `net` with that march form (NET_GENERIC may also run with 8: plan_grid
// tries 12 first), and its LDS bytes without the march tables (gen_wave_bytes: the generic instance's per-wave rows)
int render_persist_waves(int net, int form);
int render_persistent_lds_bytes(int net, int waves, uint32_t gen_wave_bytes);
// loads the code objects of the render kernel's instance families now instead of at their first launch
void preload_kernels(bool all);
// The LDS figures plan_grid (nrf_api.hip) fits the march tables with; launch_render sizes its launches from the same functions.
int render_lds_table_max_bytes();  // coarse + cell-boundary tables beyond this stay in global memory
int render_strip_lds_fixed_bytes(int stage, uint32_t gen_wave_bytes);  // LDS of the per-strip render_kernel of that stage instance without the march tables
int render_weight_area_bytes();    // the per-strip kernel's weight area: it holds the dilated table during ray setup
int render_staged_weight_bytes(uint32_t gen_frag_bytes);  // generic instance, persistent kernel: its weight fragments staged in LDS
int render_persistent_launch_lds_bytes(const DevModel& M);  // LDS of the persistent launch of a model plan_grid found one for
}  // namespace nrf
