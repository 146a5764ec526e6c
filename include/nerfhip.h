/*
 * nerfhip.h -- C ABI of the MI355X-native NeRF render hot path.
 *
 * This is the drop-in boundary.  The reference
 * (metaverse3d2022/Nerf-Cuda) has no FFI layer: its boundary is the C++ class
 * ngp::NerfRender (include/nerf-cuda/nerf_render.h:29-50) calling CUDA kernels
 * and tiny-cuda-nn objects directly.  Every entry point below names the
 * reference interface it replaces; the C++ class that mirrors ngp::NerfRender
 * on top of this header lives in nerf-cuda_amd/host/nerf_render.h.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures: device memory is passed as
 *     void* (a HIP device pointer), streams as void* (hipStream_t, NULL = the
 *     context's own stream).
 *   - every function returns an int status: 0 = NRF_OK, otherwise an
 *     NRF_E_* code; nrf_last_error() returns a thread-local message.
 *     No C++ exception crosses this boundary.
 *   - one context per device; a context is used by one thread at a time.  Render calls of one context may overlap
 *     on different streams: every call takes its own statistics counters and work queues from a ring of 16, so at
 *     most 16 render calls of a context may be in flight; nrf_get_stats reports the last call.
 *   - there is NO CPU fallback: if the HIP runtime finds no gfx950 device,
 *     nrf_create fails with NRF_E_NODEVICE.
 */
#ifndef NERFHIP_H_
#define NERFHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRF_ABI_VERSION 7
#define NRF_MAX_VIEWS 128 /* cameras one launch of the fused kernel takes (nrf_render_views) */

/* ---- status codes ------------------------------------------------------ */
enum {
  NRF_OK = 0,
  NRF_E_INVALID = 1,     /* bad argument / null pointer / bad shape          */
  NRF_E_UNSUPPORTED = 2, /* config the HIP path does not implement           */
  NRF_E_NODEVICE = 3,    /* no usable gfx950 device                          */
  NRF_E_HIP = 4,         /* a HIP runtime call failed                        */
  NRF_E_STATE = 5,       /* call order violated (e.g. render before load)    */
  NRF_E_PARAMS = 6       /* parameter count / density grid size mismatch:
                            reference nerf_network.h:425-427,
                            nerf_render.cu:467-469                           */
};

/* ---- enums mirrored from the reference's JSON vocabulary ---------------- */
/* tcnn activation names, T/src/network.cu:41-60 */
enum {
  NRF_ACT_NONE = 0,
  NRF_ACT_RELU = 1,
  NRF_ACT_EXPONENTIAL = 2,
  NRF_ACT_SIGMOID = 3,
  NRF_ACT_SQUAREPLUS = 4,
  NRF_ACT_SOFTPLUS = 5,
  NRF_ACT_SINE = 6
};
/* direction encodings, T/src/encoding.cu:97-117 */
enum {
  NRF_DIR_SH = 0,        /* SphericalHarmonics, degree 1..8                     */
  NRF_DIR_FREQUENCY = 1, /* Frequency, n_frequencies 1..18 (tcnn's default: 12)  */
  NRF_DIR_IDENTITY = 2
};
/* hash-grid flavours, T/include/tiny-cuda-nn/encodings/grid.h:1366-1367 */
enum { NRF_GRID_HASH = 0, NRF_GRID_DENSE = 1, NRF_GRID_TILED = 2 };
/* grid interpolation, T/include/tiny-cuda-nn/encodings/grid.h:1383 ("interpolation": Nearest | Linear | Smoothstep),
 * kernel_grid :196-232 */
enum { NRF_INTERP_LINEAR = 0, NRF_INTERP_NEAREST = 1, NRF_INTERP_SMOOTHSTEP = 2 };

/* ---- model description ---------------------------------------------------
 * Replaces: NerfRender::load_snapshot + reset_network + NerfNetwork ctor +
 * NerfNetwork::deserialize (nerf_render.cu:431-473,111-184;
 * nerf_network.h:95-144,424-443).  The caller has already parsed the
 * msgpack snapshot; all pointers are HOST pointers and are copied.           */
typedef struct nrf_model_desc {
  uint32_t abi_version; /* = NRF_ABI_VERSION */

  /* "encoding" block (position hash grid, 3-D input) */
  uint32_t grid_type;             /* NRF_GRID_*                               */
  uint32_t n_levels;              /* L, <= 16                                 */
  uint32_t n_features_per_level;  /* F in {1, 2, 4, 8} (grid.h:1403-1411)     */
  uint32_t log2_hashmap_size;     /* log2 T                                   */
  uint32_t base_resolution;       /* Nmin                                     */
  float per_level_scale;          /* b (already derived, nerf_render.cu:158)  */
  uint32_t interpolation;         /* NRF_INTERP_*                             */

  /* "network" (density MLP) and "rgb_network" blocks: FullyFusedMLP widths 16/32/64/128, any number of hidden
   * layers >= 1 (T/src/fully_fused_mlp.cu:636-687, 700-725).  L = 16, F = 2, 64 neurons, 1 + 2 hidden layers, a
   * 16-wide direction encoding, ReLU / None / Exponential activations (the reference's base.json) run in the
   * register-resident instance of the fused kernel; every other combination in its generic instance.           */
  uint32_t n_neurons;
  uint32_t density_hidden_layers;  /* n_hidden_layers of "network"            */
  uint32_t density_activation;     /* hidden activation                       */
  uint32_t density_output_activation;
  uint32_t density_n_output;       /* 1..16, padded to 16 rows (nerf_network.h:120-122) */
  uint32_t sigma_activation;       /* nerf_network.h:125, default Exponential */
  uint32_t rgb_hidden_layers;
  uint32_t rgb_activation;
  uint32_t rgb_output_activation;

  /* "dir_encoding" block (Composite{SH|Frequency|Identity on 3 dims}) */
  uint32_t dir_encoding;  /* NRF_DIR_*                                        */
  uint32_t sh_degree;     /* for NRF_DIR_SH                                   */
  uint32_t n_frequencies; /* for NRF_DIR_FREQUENCY                            */

  /* "snapshot" block, nerf_render.cu:441-453 */
  float aabb[6];
  float bound;
  float scale;
  uint32_t cascade;           /* C */
  uint32_t density_grid_size; /* H */
  float mean_density;

  /* fp32 parameters in the reference order (nerf_network.h:273-291):
   * density MLP | rgb MLP | hash grid | (dir encoding: none).
   * Each MLP: first [n_neurons x in] | hidden [n_neurons x n_neurons]... |
   * last [16 x n_neurons], row-major [out][in], no biases.                   */
  const float* params;
  uint64_t n_params;
  /* float density grid [C*H*H*H], index level*H^3 + x*H^2 + y*H + z; NULL (n = 0): the snapshot carries
   * none -- nrf_generate_density_grid evaluates one from the network before the first render              */
  const float* density_grid;
  uint64_t n_density_grid;
  /* (ABI 6) Device memory the library may spend on GATHER COPIES of the hash grid, in MB; 0 = the default: a sixteenth of the
   * device's memory (MI355X: 18 GB), at most half of what is free; 1 = none.  For the base.json grid shape (L = 16, F = 2, Linear) the render kernel
   * reads a level's eight trilinear corners as two aligned 16-byte "quads" from a cell-major copy of the level (every entry
   * copied, on the device, from the index grid.h:100-117 names: the same bits) instead of eight 4-byte table entries -- a
   * quarter of the gather addresses.  Copies are made four levels at a time, in level order, while they fit: levels 0..7 of
   * base.json's grid take 95 MB, levels 8..11 another 4.5 GB (MI355X, 1080p: 11.7 -> 10.7 -> 10.1 ms per 16 views).  The table
   * the reference defines is kept beside them.  The environment variable NRF_QUAD_BUDGET_MB overrides this field.         */
  uint32_t gather_copy_budget_mb;
} nrf_model_desc;

/* Level geometry derived on the host exactly as the reference does
 * (grid.h:899-931 ctor, grid.h:186-190 kernel).                              */
typedef struct nrf_level_table {
  uint32_t n_levels;
  uint32_t offset[17];     /* in entries (F values each); offset[L] = total   */
  uint32_t resolution[16]; /* grid_resolution = ceil(scale)+1                 */
  float scale[16];         /* exp2f(l*log2f(b))*Nmin - 1                      */
} nrf_level_table;

/* Render parameters.  The reference keeps these as private members without
 * setters (nerf_render.h:55-78); defaults here equal those members.          */
typedef struct nrf_options {
  float bg_color;      /* 1      m_bg_color (int in the reference)            */
  float min_near;      /* 0.2    m_min_near                                   */
  float dt_gamma;      /* 1/128  m_dt_gamma                                   */
  int32_t max_steps;   /* 1024   m_max_infer_steps                            */
  float density_scale; /* 1      m_density_scale                              */
  int32_t perturb;     /* 0      m_perturb.  > 0: the seed of kernel_march_rays' perturb branch (render_utils.h:550,
                          585-589: t += MIN_STEPSIZE() * pcg32(n, perturb).next_float() ahead of every march call) -- in
                          nrf_march n = the ray's place in the call; in rendered frames n = the ray's pixel and every sample's
                          search is a call (the per-ray loop), in instances of the per-strip kernel (slower than the default
                          path: the reference never takes this branch, m_perturb = false).  < 0: NRF_E_INVALID            */
  /* Sharding of one frame over ranks: the frame is cut into 8x8-pixel tiles
   * and those into strips of 4 horizontally adjacent tiles (32x8 pixels, one
   * workgroup); strip id = ty*ceil(ceil(W/8)/4) + tx/4, and strip id %
   * shard_count == shard_index belongs to this context, as local strip
   * id / shard_count (local tile = 4*local strip + tx%4).  Replaces the pixel
   * interleave p = NGPU*tid + gpu of render_utils.h:37.                      */
  int32_t shard_index; /* 0 */
  int32_t shard_count; /* 1 */
  /* Opt-in (default 0), NOT the reference's arithmetic: the trilinear interpolation of the hash grid accumulates
   * (half)(w * h + acc) with one rounding per corner (v_fma_mixlo/hi_f16) instead of the reference's three (grid.h:258-260:
   * fp32 product, cast to fp16, fp16 sum) -- half the vector instructions of the kernel's most expensive loop.  Features
   * differ from the bit-exact path by an ulp of a partial sum now and then (more accurate, not identical: within 4 x 2^-11
   * for table entries of magnitude 0.5); frames within the 2/255 the parity tests allow.  Measured gain: under 1 % -- the
   * kernel is co-limited by its gather path (DESIGN.md "What binds the kernel").  Honoured by the register-resident instance of the fused kernel in its persistent form and by
   * nrf_encode_grid; other instances render with the exact arithmetic.                                              */
  int32_t fast_interp; /* 0 */
  /* 1: a single shard (shard_count == 1) is rendered in the shard layout as well -- tile-major [n_tiles][64], what
   * nrf_untile* takes -- instead of the row-major frame.  What a one-rank rehearsal of the multi-GPU exchange renders
   * (bench.py --force-dist: render -> RCCL gather -> untile with shard_count 1); host frames and nrf_read_* need 0.  */
  int32_t tile_major;  /* 0 */
} nrf_options;

/* One rendered frame (device memory owned by the context, valid until the
 * next nrf_render on the same context).  Replaces ngp::Image
 * (common.h:75-89) plus the float buffers image/depth/weight_sum
 * (nerf_render.cu:200-202).                                                  */
typedef struct nrf_frame {
  int32_t width, height;
  int32_t n_tiles;      /* tiles rendered by this shard (4 per strip, including
                           out-of-image padding tiles of a ragged strip)      */
  void* rgba;           /* device float [n_px][4]; rgb after background blend
                           (render_utils.h:259-261), a = weight_sum           */
  void* depth;          /* device float [n_px] (render_utils.h:262-263)       */
  /* layout: shard_count==1 (and nrf_options.tile_major == 0) -> row-major
   * [H][W]; otherwise tile-major [n_tiles][64] in ascending tile id, see
   * nrf_untile.                                                              */
  int32_t tile_major;
  /* batched renders (nrf_render_views): view i lives at rgba + i*view_stride_px
   * pixels (depth likewise); n_views == 1 for nrf_render                      */
  int32_t n_views;
  int64_t view_stride_px;
} nrf_frame;

typedef struct nrf_stats {
  uint64_t n_rays;      /* rays generated by this shard                       */
  uint64_t n_samples;   /* march-emitted samples evaluated by the network     */
  uint64_t n_rounds;    /* sum over wave tiles of march/eval/composite rounds */
  uint64_t n_network_evals; /* network evaluations including the padding of the
                           16-sample MFMA tiles (>= n_samples)                 */
  float render_ms;      /* device time of the last nrf_render (hipEvents)     */
  uint64_t n_composited; /* samples that entered a ray's compositing sum: what the reference's own per-ray schedule emits
                           (n_samples also counts the samples a ray queues behind its terminating one; how many those are
                           depends on how rays are batched into rounds, this count does not)                           */
  float shader_clock_mhz; /* the core clock the last launch of the persistent render kernel ran at, measured in the launch:
                           d(s_memtime) / d(s_memrealtime) x 100 MHz between the entry and the exit of one wave per workgroup,
                           summed over the workgroups; 0 when the last render did not run that kernel                    */
  uint32_t gather_addresses_per_sample; /* (ABI 6) lane addresses one evaluated sample sends into the texture path with the loaded
                           model: 8 per level (the corners of grid.h:236-262), 2 for a level that is gathered from its cell-major quad
                           copy (two aligned 16-byte entries), 1 per level with Nearest interpolation                              */
  uint64_t grid_device_bytes; /* (ABI 6) device memory of the loaded model's hash grid: the reference-order table + its gather copies
                           (nrf_model_desc.gather_copy_budget_mb)                                                                  */
} nrf_stats;

typedef struct nrf_context nrf_context;

/* ---- lifecycle ----------------------------------------------------------- */
const char* nrf_last_error(void);
int nrf_abi_version(void);
/* NerfRender::NerfRender(), nerf_render.cu:46-57 (per-GPU stream creation)   */
int nrf_create(int device, nrf_context** out);
int nrf_destroy(nrf_context* ctx);
void nrf_default_options(nrf_options* o);

/* host-only helper: level geometry + parameter count for a description.
 * n_params check of nerf_network.h:425.                                      */
int nrf_level_table_compute(const nrf_model_desc* d, nrf_level_table* t);
int nrf_expected_n_params(const nrf_model_desc* d, uint64_t* n);
/* host-only: the reference's automatic per_level_scale, nerf_render.cu:158-165:
 * fp32 exp(log(2048*bound/base_resolution)/(n_levels-1)).                    */
int nrf_default_per_level_scale(float bound, uint32_t base_resolution, uint32_t n_levels,
                                float* out);

/* load_snapshot + reset_network + deserialize                                */
int nrf_load_model(nrf_context* ctx, const nrf_model_desc* d);
/* NerfRender::generate_density_grid, nerf_render.cu:388-429 (dead and incomplete in the reference: its density
 * query is commented out at :415).  Completed as its origin (torch-ngp's update_extra_state) defines it: for every
 * cascade, the density network at every cell position (init_xyzs / dd_scale, render_utils.h:79-108; no random
 * perturbation), scaled by 0.001691, folded into a grid that starts at 1/64 by g = max(g * decay, value)
 * (dg_update, render_utils.h:120-128) n_iterations times; mean_density = mean(max(g, 0)).  Replaces the model's
 * density grid and rebuilds the occupancy structures of the march.  nrf_read_density_grid returns the float grid
 * [cascade * H^3] the march currently uses (snapshot's or generated) and its mean_density.                        */
int nrf_generate_density_grid(nrf_context* ctx, int n_iterations, float decay, float* mean_density);
int nrf_read_density_grid(nrf_context* ctx, float* grid, uint64_t n, float* mean_density);
/* NerfRender::set_resolution, nerf_render.cu:186-236 (idempotent here)       */
int nrf_set_resolution(nrf_context* ctx, int width, int height);
int nrf_set_options(nrf_context* ctx, const nrf_options* o);

/* ---- the hot path -------------------------------------------------------- */
/* NerfRender::render_frame, nerf_render.cu:238-367.
 * cam = {fl_x, fl_y, cx, cy} (common.h:68-74); pose = row-major 4x4
 * camera-to-world in the NeRF/Blender convention (converted with
 * nerf_matrix_to_ngp, render_utils.h:68-77).  Asynchronous on `stream`
 * unless stream==NULL, in which case the call returns after completion.
 * A camera more than 4096 units (the reference's ngp units: 0.33 x the pose's
 * translation + 0.5) from the origin renders as background: out there t + dt
 * stops changing t in fp32, and the march of render_utils.h:593-653 -- the
 * reference's as well as this one -- would never end.                         */
int nrf_render(nrf_context* ctx, const float cam[4], const float pose[16],
               void* stream, nrf_frame* out);
/* Batched multi-view render: n_views cameras (cams [n][4], poses [n][16], same
 * model / resolution / shard) in ONE launch per NRF_MAX_VIEWS views: the tiles
 * of view v+1 take the wave slots the few long tiles at the end of view v leave
 * idle (the kernel is persistent -- one workgroup per compute unit pulls tile
 * strips of all views from work queues -- so every launch ends with the same
 * short tail whatever its size, and nothing else runs on the device while it
 * is resident: see INTEGRATION.md).  This is the path for a render_server with many concurrent camera
 * requests (the reference serves them one render_frame at a time,
 * render_server.cu:86-101) and for multi-GPU shards, which are too small to
 * fill a GPU alone.  Every view is bit-identical to an nrf_render of that
 * camera.  The context's own buffers hold nrf_set_max_views views (default 1);
 * bound buffers (nrf_bind_output) must hold n_views * view_stride_px pixels.  */
int nrf_set_max_views(nrf_context* ctx, int max_views);
int nrf_render_views(nrf_context* ctx, int n_views, const float* cams, const float* poses,
                     void* stream, nrf_frame* out);
/* SURVEY.md 8(b) lists this entry point as nrf_render_batch: same function.   */
int nrf_render_batch(nrf_context* ctx, int n_views, const float* cams, const float* poses,
                     void* stream, nrf_frame* out);
/* (ABI 7) Frames from caller-supplied rays -- whatever a pinhole cannot describe: lens distortion, fisheye, panoramas,
 * orthographic views, per-eye offsets, the secondary rays of a renderer that mixes a NeRF into its scene.
 * rays_o, rays_d: device fp32 [n_views][rays_per_view][3], in the space and layout nrf_generate_rays writes (ngp units,
 * row-major pixels).  The frame is the W x H of nrf_set_resolution: pixel (px, py) of view v takes ray
 * v * rays_per_view + py * W + px; 1 <= rays_per_view <= W * H, and a pixel whose ray number is >= rays_per_view has
 * no ray and is the background (rgb = bg_color, alpha 0, depth 0) -- a list of N rays is a W x ceil(N / W) frame.
 * Everything after ray generation is nrf_render's: near / far against the aabb with min_near, the occupied-box clip
 * and the visibility walk, march, network, compositing, the get_image_and_depth epilogue; the rays nrf_generate_rays
 * writes for a camera render that camera's nrf_render frame bit for bit.  Directions are used as given, NOT normalised:
 * depth and step sizes are in units of t along d, as in the reference.
 * Ray guard (in the kernel, per ray): a ray with a non-finite component, with |o| > 4096 (see nrf_render) or with |d|^2
 * outside [0.25, 4] is not marched; its pixel is the background.  Zero components of d are legal.
 * Honoured: bg_color, min_near, dt_gamma, max_steps, density_scale, shard_* (every rank is given the same arrays and reads
 * the rays of its own strips), tile_major; bound outputs; nrf_set_max_views; stream / sync rules and the 16 calls in
 * flight; nrf_get_stats; nrf_read_*.  perturb > 0: NRF_E_UNSUPPORTED.  fast_interp is ignored: the ray instances of the
 * fused kernel render with the exact arithmetic.  The arrays must stay valid until the call has completed.          */
int nrf_render_rays(nrf_context* ctx, int n_views, const void* rays_o, const void* rays_d,
                    uint64_t rays_per_view, void* stream, nrf_frame* out);
/* (ABI 7, addition) nrf_render_rays between per-ray limits of t, over a per-ray background: what a renderer needs to mix a
 * NeRF into a scene of its own -- a ray stops at the depth of the geometry it hits (t_max), may start behind a portal or a
 * near clip surface (t_min), and is composited over what lies behind it (background: the shaded geometry).
 * rays_o, rays_d, rays_per_view: as nrf_render_rays.  t_min, t_max: device fp32 [n_views][rays_per_view], background: device
 * fp32 [n_views][rays_per_view][3]; view v's entries start at v * rays_per_view in every array; NULL each: no limit / the
 * scalar bg_color.  With all three NULL and flags 0 this IS nrf_render_rays (which calls it so), bit for bit.
 * Limits.  A ray the guard accepts gets near, far as in nrf_render_rays (the aabb, min_near), then
 *     if (t_min > near) near = t_min;   if (t_max < far) far = t_max;
 * in exactly this form: a NaN limit is no limit, +-inf is legal.  Everything downstream uses the clamped pair -- the march,
 * and the depth normalisation of get_image_and_depth, (depth - near) / (far - near); the frame is what the reference's
 * per-ray loop yields with those two numbers replaced.  A ray with near >= far after the clamp is the background: alpha 0,
 * depth 0.  t is in units along d, which is NOT normalised (as in nrf_render_rays): for a hit at distance s along the ray
 * pass t = s / |d|.
 * Background.  A pixel whose ray has an entry is rgb[k] = c[k] + (1 - weight_sum) * background[ray][k] -- the two roundings
 * of the scalar epilogue; so is the pixel of a ray the guard refuses or whose interval is empty (it shows its own entry).  A
 * pixel without a ray (ray number >= rays_per_view) keeps the scalar bg_color.
 * flags: NRF_RAYS_DEPTH_T -- the depth plane holds the accumulated sum of w * t as composited (kernel_composite_rays'
 * state[1]; divide by alpha for the expected hit distance) instead of its normalised form; 0 for a ray without samples.
 * With an 8-bit output bound (nrf_bind_output_rgbd8 / _u8) the flag is NRF_E_UNSUPPORTED.  reserved != 0 or an unknown flag:
 * NRF_E_INVALID.  Everything else -- options, perturb, shards, views, bound outputs, streams, the calls in flight, stats,
 * the ray guard -- is as nrf_render_rays has it; all arrays must stay valid until the call has completed.
 * flags: NRF_RAYS_DENSITY_ONLY (ABI 7, addition; may be combined with NRF_RAYS_DEPTH_T) -- shadow and occlusion rays: how much
 * light gets through and where, not what colour the volume has.  The density network alone is evaluated per sample; the
 * direction encoding and the colour network are not.  Everything else is this call's, unchanged: the ray guard, near / far and
 * the clamp, the march, its termination (T < 1e-4, max_steps, far) and density_scale, views, shards and tile_major, bound float
 * outputs, streams and the 16 calls in flight, stats.  nrf_frame.rgba[..][3] (weight_sum), the depth plane and nrf_stats'
 * n_rays / n_composited are bit-identical to the same call without the flag.  rgb of a pixel that has a ray is
 *     rgb[k] = (1 - weight_sum) * b[k]      (fp32: the subtraction rounded, then the product rounded)
 * with b the ray's entry of background, or the scalar bg_color when background is NULL -- the epilogue above with c = 0.  A ray
 * the guard refuses or whose interval is empty after the clamp has alpha 0, depth 0 and rgb = its background entry; a pixel
 * without a ray keeps bg_color, alpha 0, depth 0.  Use: pass the unshadowed radiance of the light as background and the distance
 * to the light over |d| as t_max; rgb is the radiance that arrives, alpha the opacity in between.  With an 8-bit output bound
 * (nrf_bind_output_rgbd8 / _u8) the flag is NRF_E_UNSUPPORTED.  The value is 4: bit 1 (value 2) stays unassigned and is, like
 * every other unknown bit, NRF_E_INVALID.  nrf_render_rays and the pinhole entry points have no such mode.          */
enum { NRF_RAYS_DEPTH_T = 1, NRF_RAYS_DENSITY_ONLY = 4 }; /* nrf_rays.flags */
typedef struct nrf_rays {
  const void* rays_o;
  const void* rays_d;
  uint64_t rays_per_view;
  const void* t_min;
  const void* t_max;
  const void* background;
  uint32_t flags;
  uint32_t reserved; /* = 0 */
} nrf_rays;
int nrf_render_rays_clipped(nrf_context* ctx, int n_views, const nrf_rays* rays, void* stream, nrf_frame* out);
/* (ABI 7, addition) Ray hits: where a caller's ray reaches an opacity threshold -- picking, collision and placement, range
 * sensors, the origins of the shadow rays NRF_RAYS_DENSITY_ONLY serves.  A ray is processed exactly as nrf_render_rays_clipped
 * with NRF_RAYS_DENSITY_ONLY processes it -- the guard, near / far and the clamp by t_min / t_max, the march, the density network,
 * density_scale, and per sample  alpha,  T = 1 - ws,  w = alpha * T,  ws += w,  dep += w * t  -- with one more termination: after a
 * sample's update, ws >= opacity (an fp32 compare on the updated ws) ends the ray; that sample counts as composited.  The
 * ordinary terminations (T < 1e-4, t >= far, max_steps) stay.  The crossing sample is the first whose updated ws reaches opacity.
 *                 hit                                          miss (never reached opacity)   no ray / refused / empty interval
 *   rgba[..][0]   t of the crossing sample as composited: the   0                              0
 *                 end of its interval, what dep += w * t uses
 *   rgba[..][1]   the crossing sample's dt                      0                              0
 *   rgba[..][2]   ws before the crossing sample (< opacity)     0                              0
 *   rgba[..][3]   ws after it (>= opacity)                      the final ws (< opacity)       0
 *   depth         the sum of w * t up to and including the      that sum over the whole ray    0
 *                 crossing sample (NRF_RAYS_DEPTH_T semantics)
 * A hit is recognised by rgba[..][3] >= opacity.  bg_color and backgrounds play no part.  Refinement: if density is constant inside
 * the crossing sample, the exact crossing distance is
 *     t* = t - dt + dt * ln((1 - a0) / (1 - opacity)) / ln((1 - a0) / (1 - a1)),    a0 = rgba[..][2], a1 = rgba[..][3];
 * the kernel does not compute it.
 * rays->rays_o, rays_d, rays_per_view, t_min, t_max: as nrf_render_rays_clipped.  rays->background must be NULL, rays->flags and
 * rays->reserved 0, and 0 < opacity <= 1 (NaN is invalid): NRF_E_INVALID otherwise.  An 8-bit output bound (nrf_bind_output_rgbd8 /
 * _u8): NRF_E_UNSUPPORTED, nothing is written.  perturb > 0: NRF_E_UNSUPPORTED.  fast_interp is ignored.  Everything else is as in
 * nrf_render_rays_clipped: views, shards and tile_major, bound float outputs, nrf_set_max_views, stream rules, the 16 calls in
 * flight, nrf_get_stats (a ray that stops at the threshold stops marching: n_composited counts what it composited), nrf_read_*. */
int nrf_ray_hits(nrf_context* ctx, int n_views, const nrf_rays* rays, float opacity, void* stream, nrf_frame* out);
/* Binds caller-owned device buffers (e.g. a render buffer's RGBA plane or a
 * torch tensor) as the target of subsequent nrf_render calls: rgba float
 * [n_px][4], depth float [n_px], n_px as nrf_frame describes.  NULL, NULL
 * returns to the context's own buffers.  Replaces the host round trip
 * render_frame -> host_to_accumulate_buffer of main.cu:87-129.               */
int nrf_bind_output(nrf_context* ctx, void* rgba, void* depth);
/* Binds a caller-owned device buffer of packed 8-bit pixels -- the reference's output format
 * (unsigned char)(255.0 * x) of r, g, b and depth (nerf_render.cu:352-359) as r | g << 8 | b << 16 | depth << 24,
 * uint32 [n_views * view_stride_px], same pixel order as the float planes (tile-major for a shard) -- as the
 * target of subsequent renders: the kernel writes these 4 bytes per pixel instead of the 20 of the float planes,
 * bit-identical to nrf_quantize_rgbd8 of them.  The frame is then the caller's to read (nrf_read_* return
 * NRF_E_STATE, nrf_frame::rgba / depth are NULL); NULL returns to the float planes.  What a rank of a multi-GPU
 * step binds: its shard goes onto the wire as rendered.                                                    */
int nrf_bind_output_rgbd8(nrf_context* ctx, void* rgbd8);
/* Binds caller-owned device (or device-visible pinned host) buffers in the layout of the reference's host Image
 * (common.h:75-89, filled by nerf_render.cu:352-359): rgb u8 [n_views * view_stride_px][3], depth u8
 * [n_views * view_stride_px], row-major, single-shard frames only; both 4-byte aligned.  The kernel writes these
 * 4 bytes per pixel itself -- bit-identical to nrf_read_u8 of the float planes -- as whole dwords assembled inside
 * the tile's wavefront.  nrf_read_* return NRF_E_STATE; NULL, NULL returns to the float planes.               */
int nrf_bind_output_u8(nrf_context* ctx, void* rgb8, void* depth8);
/* nrf_render on the context's own stream WITHOUT waiting for it (the way the
 * reference overlaps its NGPU devices, nerf_render.cu:252-362); nrf_sync waits. */
int nrf_render_async(nrf_context* ctx, const float cam[4], const float pose[16], nrf_frame* out);
int nrf_sync(nrf_context* ctx);
/* ---- host frames: NerfRender::render_frame's result is HOST memory (nerf_render.cu:345-359: D2H of the float planes and
 * a single-threaded quantise / de-interleave loop per GPU; Image, common.h:75-89).  nrf_submit_host_u8 renders n_views
 * cameras into 8-bit planes (the kernel writes the Image's bytes itself), has the copy engine move the rows of every
 * view's region of interest into pinned host memory owned by the context, and fills the remaining rows -- background by
 * construction -- from the calling thread while the GPU renders.  It returns at once; nrf_wait_host_u8 blocks until the
 * frames of that ticket are in host memory.  Two slots: the copy of one call overlaps the render of the next, and the
 * pointers of a ticket stay valid until the SECOND next nrf_submit_host_u8 on the context (that call waits for the
 * slot's copy, not for its reader).  NRF_HOST_RGB_ONLY: depth is not copied (nrf_host_frame::depth = NULL) -- what a
 * render_server needs.  Bytes identical to nrf_render + nrf_read_u8.  Single-shard frames only.                      */
enum { NRF_HOST_RGB_ONLY = 1 };
typedef struct nrf_host_frame {
  int32_t width, height, n_views;
  const uint8_t* rgb;      /* pinned host: view v at rgb + v * view_stride_px * 3, [H][W][3] */
  const uint8_t* depth;    /* pinned host: view v at depth + v * view_stride_px, [H][W]; NULL with NRF_HOST_RGB_ONLY */
  int64_t view_stride_px;
  float render_ms;         /* device time of this call's render launches (events on their stream) */
  uint64_t copied_bytes;   /* what the copy engine moved for this call (the rows of the regions of interest) */
} nrf_host_frame;
int nrf_submit_host_u8(nrf_context* ctx, int n_views, const float* cams, const float* poses, int flags, int* ticket);
int nrf_wait_host_u8(nrf_context* ctx, int ticket, nrf_host_frame* out);
/* submit + wait: one NerfRender::render_frame(s) call of the reference                                               */
int nrf_render_host_u8(nrf_context* ctx, int n_views, const float* cams, const float* poses, int flags, nrf_host_frame* out);
/* Host copy + quantisation, nerf_render.cu:345-359 (saturating, row-major), of a frame rendered into float planes
 * (a quantise launch + two blocking copies per view: the after-the-fact path; nrf_render_host_u8 is the fast one). */
int nrf_read_u8(nrf_context* ctx, uint8_t* rgb, uint8_t* depth);
/* The same quantisation on the device for any float frame / shard / batch of
 * n_px pixels: out[i] = r | g << 8 | b << 16 | depth << 24.  Four bytes per
 * pixel instead of twenty is what a multi-GPU gather should carry when the
 * consumer wants the reference's 8-bit Image (common.h:75-89); 4-byte pixels go
 * through nrf_untile(_views) with channels = 1.                               */
int nrf_quantize_rgbd8(nrf_context* ctx, const void* rgba, const void* depth, uint64_t n_px,
                       void* out_u32, void* stream);
/* The same quantisation into the planar layout of the reference's Image: rgb u8 [n_px][3], depth u8 [n_px] (device). */
int nrf_quantize_u8(nrf_context* ctx, const void* rgba, const void* depth, uint64_t n_px, void* rgb8, void* depth8,
                    void* stream);
/* Host copy of the float buffers (row-major; single-shard frames only).      */
int nrf_read_f32(nrf_context* ctx, float* rgba, float* depth);
/* nrf_read_f32 / nrf_read_u8 for view `view` of the last nrf_render_views.    */
int nrf_read_view_f32(nrf_context* ctx, int view, float* rgba, float* depth);
int nrf_read_view_u8(nrf_context* ctx, int view, uint8_t* rgb, uint8_t* depth);
/* Host copy of this context's shard as rendered: rgba [n_tiles*64][4], depth
 * [n_tiles*64] (tile-major when shard_count > 1, else the row-major frame).  */
int nrf_read_shard_f32(nrf_context* ctx, float* rgba, float* depth);
/* Rearranges gathered tile-major shards ([shard][n_tiles_max][64][C] floats,
 * as produced by a gather of every rank's nrf_frame buffer) into a
 * row-major [H][W][C] image on the device.  Replaces the de-interleave loop
 * nerf_render.cu:352-359.                                                    */
int nrf_untile(nrf_context* ctx, const void* gathered, int shard_count,
               int tiles_per_shard, int channels, void* out_rowmajor,
               void* stream);
/* Same for gathered batches of nrf_render_views: [shard][view][n_tiles_max][64][C]
 * -> [view][H][W][C].                                                         */
int nrf_untile_views(nrf_context* ctx, const void* gathered, int shard_count,
                     int tiles_per_shard, int channels, int n_views,
                     void* out_rowmajor, void* stream);
/* Gathered PACKED shards ([shard][view][n_tiles_max][64] uint32 r | g << 8 | b << 16 | depth << 24, as rendered with
 * nrf_bind_output_rgbd8) -> the planar layout of the reference's Image: rgb u8 [view][H][W][3], depth u8 [view][H][W]
 * (device or device-visible pinned host memory; the shards 16-byte aligned, the planes 4-byte aligned when the width is a multiple of 4).  The de-interleave + quantise loop of
 * nerf_render.cu:352-359 for a device group, on the device.                                                    */
int nrf_untile_views_u8(nrf_context* ctx, const void* gathered_rgbd8, int shard_count, int tiles_per_shard, int n_views,
                        void* rgb8, void* depth8, void* stream);
int nrf_tiles_per_shard(int width, int height, int shard_count, int* n);
int nrf_get_stats(nrf_context* ctx, nrf_stats* s);

/* ---- device groups: several GPUs driven by one process ---------------------
 * The reference's NGPU threads + D2H gather + host de-interleave loop
 * (nerf_render.cu:252-362, common.h:91) as one object: every member renders
 * its strips of every view, ships the shard device-to-device to devices[0]
 * (xGMI peer copies) and devices[0] untiles.  devices == NULL means 0..n-1; a
 * device may be listed more than once.  The frames of nrf_group_render_views
 * are row-major float planes on devices[0] (nrf_frame, view_stride_px = W*H),
 * bit-identical to nrf_render_views on a single context.  The one-process-per-
 * GPU form (torch.distributed / RCCL gather) is bench.py.                      */
typedef struct nrf_group nrf_group;
int nrf_group_create(int n_devices, const int* devices, nrf_group** out);
int nrf_group_destroy(nrf_group* grp);
/* The transport of the one exchange step (the reference: cudaMemcpyAsync D2H of every GPU's planes into one host buffer,
 * nerf_render.cu:345-359).  NRF_GATHER_PEER_COPY (default): hipMemcpyPeerAsync per member.  NRF_GATHER_RCCL: one RCCL
 * communicator per member (ncclCommInitAll) and one group of ncclSend / ncclRecv to devices[0] per call -- a direct gather
 * over the point-to-point xGMI links; needs distinct devices (NRF_E_UNSUPPORTED otherwise) and librccl, which is opened
 * on this call (a process that never asks never loads it).  In this mode a ONE-member group runs the whole exchange too
 * (tile-major shard, send to self, untile).  Frames are the same bits either way.  May be called between renders; it
 * reallocates the group's buffers, so host-frame pointers handed out earlier become invalid and a ticket that has not been
 * waited for makes it return NRF_E_STATE.  The environment variable NRF_GROUP_GATHER=rccl|peer sets it at nrf_group_create. */
enum { NRF_GATHER_PEER_COPY = 0, NRF_GATHER_RCCL = 1 };
int nrf_group_set_gather(nrf_group* grp, int mode);
/* rccl_version: ncclGetVersion() of the opened library in RCCL mode (e.g. 22703), else 0 */
int nrf_group_get_gather(const nrf_group* grp, int* mode, int* rccl_version);
int nrf_group_size(const nrf_group* grp);
/* member i's context (owned by the group): stage entry points, per-device statistics */
nrf_context* nrf_group_member(nrf_group* grp, int index);
int nrf_group_load_model(nrf_group* grp, const nrf_model_desc* d);
int nrf_group_set_options(nrf_group* grp, const nrf_options* o); /* shard_* are set by the group */
int nrf_group_set_resolution(nrf_group* grp, int width, int height);
int nrf_group_render_views(nrf_group* grp, int n_views, const float* cams, const float* poses,
                           nrf_frame* out);
int nrf_group_read_view_f32(nrf_group* grp, int view, float* rgba, float* depth);
int nrf_group_read_view_u8(nrf_group* grp, int view, uint8_t* rgb, uint8_t* depth);
/* Host frames of a group (see nrf_submit_host_u8): the members render packed 8-bit shards, devices[0] untiles them
 * into the Image layout and ONE copy per call brings all views to pinned host memory; same ticket rules.          */
int nrf_group_submit_host_u8(nrf_group* grp, int n_views, const float* cams, const float* poses, int flags, int* ticket);
int nrf_group_wait_host_u8(nrf_group* grp, int ticket, nrf_host_frame* out);
int nrf_group_render_host_u8(nrf_group* grp, int n_views, const float* cams, const float* poses, int flags, nrf_host_frame* out);
int nrf_group_get_stats(nrf_group* grp, nrf_stats* s); /* sums; render_ms = slowest member */

/* ---- stage entry points (unit parity against the oracle) -----------------
 * All pointers are DEVICE pointers, n = number of samples / rays.            */
/* kernel_grid<half,3,F>, grid.h:139-268.  pos01 [n][3] in [0,1];
 * out fp16 [n][next_multiple(L*F, 16)] (padding columns are 0, grid.h:959-969) */
int nrf_encode_grid(nrf_context* ctx, const void* pos01, uint32_t n, void* out_f16,
                    void* stream);
/* kernel_sh / frequency_encoding / identity.  dir01 [n][3] in [0,1];
 * out fp16 [n][next_multiple(raw width, 16)]: 16 for SH <= 4, 64 for SH 8,
 * 80 for Frequency with 12 frequencies                                       */
int nrf_encode_dir(nrf_context* ctx, const void* dir01, uint32_t n, void* out_f16,
                   void* stream);
/* kernel_mlp_fused x2 + extract_density (nerf_network.h:148-196) on
 * pre-encoded inputs: feat fp16 [n][feature width], dirfeat fp16 [n][dir
 * width] (the widths of nrf_encode_grid / nrf_encode_dir: 32 and 16 for the
 * base configuration) -> out fp16 [n][4] = (r,g,b,sigma).
 * Alignment: feat_f16 16 bytes, dirfeat_f16 and out_f16 8 bytes (the base
 * configuration's kernel reads a row in 16- and 8-byte pieces and writes a
 * row in one 8-byte store; models that go through the generic stage need
 * 2 bytes for the two inputs and 8 for out_f16).  Anything else is refused
 * with NRF_E_INVALID before a kernel is launched.                            */
int nrf_mlp_forward(nrf_context* ctx, const void* feat_f16, const void* dirfeat_f16,
                    uint32_t n, void* out_f16, void* stream);
/* Measurement aid: the same call, every chunk of samples evaluated `repeat`
 * times from registers (identical output): repeat >> 1 gives the rate of the
 * MFMA chain with its fp32 -> fp16 re-packing, without the HBM stream.       */
int nrf_mlp_forward_repeat(nrf_context* ctx, const void* feat_f16, const void* dirfeat_f16,
                           uint32_t n, void* out_f16, uint32_t repeat, void* stream);
/* Whole network on raw march output (world-space xyz in [-bound,bound], unit
 * dirs), including the two affine maps nerf_render.cu:311-314 and
 * decompose (render_utils.h:308-334): -> sigma f32 [n], rgb f32 [n][3]       */
int nrf_network(nrf_context* ctx, const void* xyz, const void* dir, uint32_t n,
                void* sigma_f32, void* rgb_f32, void* stream);
/* (ABI 7, additions) Density and its gradient at points and at ray hits: what a renderer with geometry of its own needs to light a
 * hit of nrf_ray_hits, to offset its shadow ray and to respond to a collision -- which way the surface faces there.
 * xyz: device fp32 [n][3] in the space nrf_network takes (nrf_march's output; o + t d of the rays of nrf_generate_rays /
 * nrf_render_rays).  sigma is nrf_network's sigma bit for bit, from the density network alone: no directions, density_scale is
 * not applied, options play no part.  The surface normal is -g / |g|; the kernel does not normalise (no sqrt, no division).
 * Every operation below is ONE fp32 rounding (no contraction), so a host can replay it:
 *   taps      for axis k:  xp = x_k + h,  xm = x_k - h;  a tap is the point with that one coordinate replaced.  Seven taps: the
 *             centre, then +x, -x, +y, -y, +z, -z.
 *   gradient  g_k = (s(xp) - s(xm)) * inv2h,  inv2h = 1.0f / (h + h) computed once on the host.
 *   guard     a point is evaluated if and only if every coordinate of every tap is finite and within [-bound, bound]
 *             (nrf_model_desc.bound); otherwise ALL its outputs are 0 and none of its taps is gathered.  nrf_density has the centre
 *             tap only: |x_k| <= bound.  Exact: no clamping, no one-sided stencil.
 * nrf_density:           sigma_f32 = device float [n].
 * nrf_density_gradient:  out_f32x4 = device float4 [n] = (g_x, g_y, g_z, sigma at the point).
 * nrf_hit_gradients:     the same at the hits of an nrf_ray_hits frame, without a round trip through the caller.  Pixel p of view v
 *   of hits->rgba is a record (t, dt, ws0, ws1) and belongs to ray v * rays_per_view + p.  It is a hit if p < rays_per_view &&
 *   ws1 >= opacity (the fp32 compare of nrf_ray_hits).  For a hit:  tq = t - frac * dt,  x_k = o_k + tq * d_k;  pos = (x, y, z, tq),
 *   out = the gradient record at x under the same guard.  Every other pixel is zeros in both planes.  frac in [0, 1]: 1 is the start
 *   of the crossing sample's interval, 0 its end, 0.5 the middle (for the refined t* of nrf_ray_hits compute positions yourself and
 *   call nrf_density_gradient).  pos_f32x4 and out_f32x4 hold hits->n_views * hits->view_stride_px float4 each, in the frame's own
 *   pixel order.  Of `rays` only rays_o, rays_d and rays_per_view (1 .. view_stride_px) are read.
 * NRF_E_INVALID: a NULL pointer with n > 0; h not finite, <= 0 or > bound; frac outside [0, 1] or NaN; opacity outside (0, 1];
 * hits->rgba == NULL.  NRF_E_UNSUPPORTED: a tile-major hit frame (shards, nrf_options.tile_major).  NRF_E_STATE: no model loaded.
 * n == 0: NRF_OK, nothing done.  Stream and synchronisation rules are nrf_network's; the calls take no slot of the 16 calls in
 * flight, leave nrf_get_stats untouched and write none of the context's frame buffers. */
int nrf_density(nrf_context* ctx, const void* xyz, uint32_t n, void* sigma_f32, void* stream);
int nrf_density_gradient(nrf_context* ctx, const void* xyz, uint32_t n, float h, void* out_f32x4, void* stream);
int nrf_hit_gradients(nrf_context* ctx, const nrf_frame* hits, const nrf_rays* rays, float opacity, float frac, float h,
                      void* pos_f32x4, void* out_f32x4, void* stream);
/* (ABI 7, addition) Mesh extraction: the object itself -- a collision proxy, a shadow caster for a rasteriser, a preview or export
 * mesh -- instead of answers per ray or per point.  The density network is evaluated on a lattice whose positions the kernel makes
 * itself (no position upload), and the iso-surface is polygonised on the device by marching tetrahedra on the Kuhn split of each
 * cell (six tetrahedra around the main diagonal): no ambiguous faces, so where the surface does not reach the lattice's boundary it is
 * a closed, consistently oriented 2-manifold.  Every fp32 operation below is ONE rounding (no contraction), so a host can replay it:
 *   lattice    dims = (nx, ny, nz), each >= 2; point (i, j, k) has the linear index p = (i * ny + j) * nz + k (z innermost) and the
 *              position x_c = origin_c + (float)index_c * cell_c (the product is rounded, then the sum).
 *   inside     sigma[p] >= iso (fp32 compare; NaN is outside).
 *   vertices   point p owns edge m = 1 .. 7 to q = (i + (m & 1), j + ((m >> 1) & 1), k + ((m >> 2) & 1)) where q is in the lattice.
 *              The edge crosses iff inside(p) != inside(q) and then carries one vertex: d = s_q - s_p, u = (iso - s_p) / d,
 *              u = 0.5 unless 0 <= u <= 1 (infinite sigmas, NaN), v_c = x_p,c + u * (x_q,c - x_p,c).  Vertices are numbered in order
 *              of p, then m.
 *   triangles  the cell with min corner p (i < nx - 1, j < ny - 1, k < nz - 1) has the tetrahedra c0 = p, c1 = c0 + e_a, c2 = c1 + e_b,
 *              c3 = p + (1, 1, 1) for (a, b, c) = xyz, xzy, yxz, yzx, zxy, zyx.  One corner L unlike the others r0 < r1 < r2: the
 *              triangle (L-r0, L-r1, L-r2); two inside A < B, two outside C < D: (AC, AD, BD) and (AC, BD, BC); the last two indices
 *              swapped where needed so that (b - a) x (c - a) points from inside to outside (counter-clockwise seen from outside).
 *              Triangles are numbered in order of p, then tetrahedron, then as listed.  (csrc/nrf_mesh_plan.h is this text as code.)
 * nrf_density_lattice: sigma_f32 = device float [nx][ny][nz], bit-identical to nrf_density on those positions: 0 where a coordinate is
 *   outside [-bound, bound] (a lattice may stick out of the box).  Stream and synchronisation rules are nrf_density's.
 * nrf_extract_mesh: sigma_f32 == NULL evaluates the lattice into a buffer of the context; otherwise it polygonises the caller's device
 *   array float [nx][ny][nz] and needs no model.  The work is enqueued on `stream` (NULL: the context's) and the call returns after
 *   it has completed: the sizes have to reach the host.  out->vertices (device float [n_vertices][3]) and out->triangles (device
 *   uint32 [n_triangles][3]) are owned by the context, grow as needed and stay valid until the next nrf_extract_mesh or nrf_destroy;
 *   out->sigma is the lattice that was used (the caller's pointer, or the context's buffer).  An empty surface is NRF_OK with zero
 *   counts.  The vertex layout is [n][3] on purpose: nrf_density_gradient takes out->vertices as it is (n = n_vertices), and
 *   -g / |g| of its records is the vertex normal.
 * nrf_read_mesh: host copies of the last mesh (float [n_vertices][3], uint32 [n_triangles][3]); either may be NULL.
 * NRF_E_INVALID: a NULL lattice or out (nrf_density_lattice: sigma_f32); a dimension below 2; nx * ny * nz > 2^27; a cell that is not
 * finite or <= 0; a non-finite origin; a non-finite iso; reserved != 0.  NRF_E_STATE: no model loaded and no sigma given
 * (nrf_read_mesh: no mesh extracted yet).  NRF_E_HIP with a message: the sigmas changed between the count and the emit pass (every
 * write is checked against the counted sizes).  A refused call writes nothing.  The calls take no slot of the 16 calls in flight, leave
 * nrf_get_stats untouched and write none of the context's frame buffers. */
typedef struct nrf_lattice {
  float origin[3];  /* position of point (0, 0, 0)                           */
  float cell[3];    /* spacing per axis, > 0                                 */
  uint32_t dims[3]; /* points per axis, >= 2                                 */
  uint32_t reserved; /* 0                                                    */
} nrf_lattice;
typedef struct nrf_mesh {
  uint64_t n_vertices, n_triangles;
  void* vertices;  /* device float [n_vertices][3]                           */
  void* triangles; /* device uint32 [n_triangles][3]                         */
  void* sigma;     /* device float [nx][ny][nz]                              */
} nrf_mesh;
int nrf_density_lattice(nrf_context* ctx, const nrf_lattice* lattice, void* sigma_f32, void* stream);
int nrf_extract_mesh(nrf_context* ctx, const nrf_lattice* lattice, float iso, const void* sigma_f32, void* stream, nrf_mesh* out);
int nrf_read_mesh(nrf_context* ctx, float* vertices, uint32_t* triangles);
/* (ABI 7, addition) Unit normals and colours at points and at mesh vertices: what an exported mesh needs besides positions and
 * triangles, and what a rasteriser needs to draw the proxy it has just extracted -- in one launch, without a round trip through the
 * caller.  Seven network passes per point: the six off-centre taps of nrf_density_gradient through the density network alone, then the
 * centre through both networks, looked at along a direction the kernel forms itself.  The gradient record (g_x, g_y, g_z) is
 * nrf_density_gradient's, bit for bit: the same taps, the same guard, the same inv2h.  Every operation below is ONE fp32 rounding (no
 * contraction), the square root and the division the correctly rounded IEEE ones, so a host can replay it:
 *   l2   = (g_x * g_x + g_y * g_y) + g_z * g_z          three products, two sums, in this order
 *   ok   = l2 is finite && l2 >= 2^-60                   (false for NaN; the floor makes the result independent of the denormal mode)
 *   len  = ok ? sqrt(l2) : 0
 *   d_k  = ok ? g_k / len : 0                            the direction of a viewer's ray that meets the surface head-on, from outside
 *   n_k  = -d_k                                          exact: the outward normal -g / |g|.  A degenerate point (ok false) has
 *                                                        n = d = (+0, +0, +0), not -0
 *   direction  the network is given u_k = 0.5f * v_k (rounded), then + 0.5f (rounded), as nrf_network forms it, with v = d (dir == NULL)
 *              or v = the caller's direction: not normalised, not checked.  A direction never becomes an address.
 *   guard      nrf_density_gradient's: a point is evaluated if and only if every coordinate of every one of its seven taps is finite and
 *              within [-bound, bound]; otherwise BOTH its records are zeros and none of its taps is gathered.
 * nrf_point_attributes: xyz = device fp32 [n][3], as nrf_density_gradient takes it (nrf_mesh.vertices goes in as it is); dir = device
 *   fp32 [n][3] or NULL.  normal_f32x4 = device float4 [n] = (n_x, n_y, n_z, sigma at the point); color_f32x4 = device float4 [n] =
 *   (r, g, b, len).  sigma and rgb are those of nrf_network at (x, v), bit for bit.  With a given direction the six taps still run: the
 *   normal is reported all the same.  A degenerate point has n = 0, len = 0 and, with dir == NULL, the direction (0, 0, 0); its sigma and
 *   its colour are still evaluated: a flat region has a colour too.
 * nrf_mesh_attributes: the same at the vertices of the context's last nrf_extract_mesh, with dir == NULL, into two buffers owned by the
 *   context (device float4 [n_vertices] each): they grow as needed and stay valid until the next nrf_extract_mesh, nrf_mesh_attributes
 *   or nrf_destroy.  The work is enqueued on `stream` (NULL: the context's) and the call returns after it has completed, as
 *   nrf_extract_mesh does.  A vertex whose stencil leaves [-bound, bound] gets zeros in both records: on a lattice that spans the whole
 *   box (testbed's) those are the vertices within h of a face.  An empty mesh is NRF_OK with n_vertices = 0.
 * nrf_read_mesh_attributes: host copies of the last attributes (float [n_vertices][4] each); either may be NULL.
 * An exported colour byte is the library's 8-bit rule of nrf_read_u8: (unsigned char)(255.0 * x), saturating, NaN -> 0.
 * NRF_E_INVALID: a NULL xyz, normal or colour pointer with n > 0 (nrf_mesh_attributes: out); h not finite, <= 0 or > bound.  NRF_E_STATE:
 * no model loaded (also for a mesh made from a caller's lattice on a context without a model: there is no network to ask); no mesh
 * extracted yet; nrf_read_mesh_attributes: no attributes of the current mesh -- a new nrf_extract_mesh invalidates them.  n == 0: NRF_OK,
 * nothing done.  Stream and synchronisation rules of nrf_point_attributes are nrf_network's.  A refused call writes nothing.  The calls
 * take no slot of the 16 calls in flight, leave nrf_get_stats untouched and write none of the context's frame buffers.
 * (csrc/nrf_attr_plan.h is this text as code.) */
typedef struct nrf_mesh_attr {
  uint64_t n_vertices;
  void* normals; /* device float4 [n_vertices] = (n_x, n_y, n_z, sigma)      */
  void* colors;  /* device float4 [n_vertices] = (r, g, b, len)              */
} nrf_mesh_attr;
int nrf_point_attributes(nrf_context* ctx, const void* xyz, const void* dir, uint32_t n, float h, void* normal_f32x4, void* color_f32x4,
                         void* stream);
int nrf_mesh_attributes(nrf_context* ctx, float h, void* stream, nrf_mesh_attr* out);
int nrf_read_mesh_attributes(nrf_context* ctx, float* normals_f32x4, float* colors_f32x4);
/* (ABI 7, addition) Connected components and floater removal: an iso-surface of a trained density is never one surface -- it is the
 * object plus small closed blobs around it and, on a lattice that spans the whole box, open sheets at the faces.  These calls label
 * the components of the context's current mesh on the device, report a small table of them and filter the mesh in place by component
 * size, so that "the object" never travels to the host and back before it gets its attributes.  Integers and copied float bits only:
 *   connected  two vertices of the current mesh are connected if a triangle names both; components are the classes of the transitive
 *              closure.  A vertex that no triangle names is a component of its own with 0 triangles (nrf_extract_mesh never makes one).
 *   label      label[v] = the smallest vertex id in v's component; hence label[v] <= v and label[label[v]] == label[v], and the result
 *              does not depend on the order in which anything ran.
 *   table      one row per component in ascending label: label, n_vertices, n_triangles.  A triangle belongs to the component of its
 *              vertices.  The counts are integer sums and exact.
 *   keep       a component is kept iff n_triangles >= min_triangles; with NRF_MESH_KEEP_LARGEST it must in addition be the component
 *              with the most triangles, a tie going to the smaller label.  With the flag set and min_triangles above the largest count
 *              nothing is kept.
 *   filtered   a vertex is kept iff its component is, a triangle likewise.  Kept vertices keep their float bits and their relative
 *              order: the new id of a vertex is the number of kept vertices with a smaller old id.  Kept triangles keep their relative
 *              order and the order of their three indices, each index remapped.  (csrc/nrf_meshcc_plan.h is this text as code.)
 * nrf_mesh_components: labels and table of the current mesh, in buffers owned by the context that grow as needed and stay valid until
 *   the next nrf_extract_mesh, nrf_filter_mesh, nrf_mesh_components or nrf_destroy.  n_rounds reports how many hook + compress rounds
 *   the labelling took, the final round that changed nothing included.  An empty mesh is NRF_OK with n_components == 0.
 * nrf_read_mesh_components: host copies of the current labelling: uint32 [n_vertices] and uint32 [n_components][3]; either may be NULL.
 * nrf_filter_mesh: the context's mesh BECOMES the filtered mesh -- nrf_read_mesh, nrf_mesh_attributes and nrf_point_attributes on
 *   out->vertices all see it; out->sigma is the extraction's, unchanged; earlier vertices / triangles pointers are invalid.  It labels
 *   the mesh itself when no current labelling exists.  Keeping everything leaves the mesh bit for bit as it was; keeping nothing is
 *   NRF_OK with zero counts.  It invalidates the labelling and the attributes of the mesh it replaced: nrf_read_mesh_components and
 *   nrf_read_mesh_attributes return NRF_E_STATE until asked again -- attributes after filtering is the intended order: fewer vertices,
 *   seven network passes each.
 * The work is enqueued on `stream` (NULL: the context's) and the calls return after it has completed, as nrf_extract_mesh does: sizes
 * and the labelling's convergence flag have to reach the host.  No model is needed.  NRF_E_INVALID: a NULL out; an unknown flag bit.
 * NRF_E_STATE: no mesh extracted yet; nrf_read_mesh_components: no current labelling.  NRF_E_HIP with a message: the mesh changed
 * between the scan and the scatter pass of the filter (every write is checked against the counted sizes).  A refused call writes
 * nothing.  The calls take no slot of the 16 calls in flight, leave nrf_get_stats untouched and write none of the context's frame
 * buffers. */
typedef struct nrf_mesh_parts {
  uint64_t n_components;
  void* labels;        /* device uint32 [n_vertices]: label of each vertex of the current mesh                 */
  void* components;    /* device uint32 [n_components][3] = label, n_vertices, n_triangles; ascending label    */
  uint32_t n_rounds;   /* hook + compress rounds the labelling took, the final round that changed nothing included */
  uint32_t reserved;   /* written as 0 */
} nrf_mesh_parts;
enum { NRF_MESH_KEEP_LARGEST = 1 };  /* nrf_filter_mesh flags */
int nrf_mesh_components(nrf_context* ctx, void* stream, nrf_mesh_parts* out);
int nrf_read_mesh_components(nrf_context* ctx, uint32_t* labels, uint32_t* components);
int nrf_filter_mesh(nrf_context* ctx, uint64_t min_triangles, uint32_t flags, void* stream, nrf_mesh* out);
/* (ABI 7, addition) Mesh refinement: nrf_extract_mesh places a vertex by LINEAR interpolation of sigma between two lattice points, and
 * sigma -- the exponential of a network output -- changes by large factors across one cell, so every vertex sits towards the outside
 * lattice point (the terraces of a NeRF mesh).  A crossing edge has one endpoint inside and one outside: it brackets the iso value, and
 * bisection along it converges whatever the density does in between.  nrf_refine_mesh does that on the device, in one launch with
 * n_steps + 2 passes of the density network per vertex, between the extraction (or the filter) and the attributes:
 *   edge word  nrf_extract_mesh records for every vertex w = (p << 3) | m: the lattice point p (< 2^27) that owns its edge and the edge
 *              m = 1 .. 7; nrf_filter_mesh carries the words with the vertices it keeps.  xp = the position of p, xq = the position of
 *              the point edge m runs to (origin + (float)index * cell, as above), e_c = xq_c - xp_c, and
 *              point(u)_c = xp_c + u * e_c (the product rounded, then the sum: the form of the extraction's vertex).
 *   s(x)       nrf_density at x, bit for bit: 0 where a coordinate is outside [-bound, bound] or not finite.
 *   ends       s0 = s(xp), s1 = s(xq); in0 = s0 >= iso, in1 = s1 >= iso, with the lattice and the iso of the last nrf_extract_mesh.
 *              in0 == in1: the vertex is UNBRACKETED -- it keeps its bits and its bracket record is (0, 1, s0, s1).  This happens only
 *              where a caller's lattice disagrees with the network, or with NaN.
 *   bisect     lo = 0, hi = 1, slo = s0, shi = s1; n_steps times: um = 0.5f * (lo + hi), sm = s(point(um)); if (sm >= iso) == in0 then
 *              (lo, slo) = (um, sm), else (hi, shi) = (um, sm).
 *   finish     one secant step in the final bracket: d = shi - slo; r = (iso - slo) / d; if (!(r >= 0 && r <= 1)) r = 0.5;
 *              u = lo + r * (hi - lo); the vertex becomes point(u) and its bracket record (lo, hi, slo, shi).  Every operation is one
 *              fp32 rounding.  (csrc/nrf_refine_plan.h is this text as code.)
 *   With n_steps == 0 this is the extraction's interpolation on the network's own sigmas: a mesh extracted from the context's own
 *   lattice (sigma_f32 == NULL) is left bit for bit as it was.  hi - lo == 2^-n_steps for every bracketed vertex.
 * nrf_refine_mesh: the vertices of the context's current mesh are rewritten in place; the result depends on the edge words and not on
 *   the current positions, so calling it twice with the same n_steps gives the same bits.  The buffers are owned by the context, grow
 *   as needed and stay valid until the next nrf_extract_mesh, nrf_filter_mesh, nrf_refine_mesh or nrf_destroy.  Triangles, and a current
 *   labelling of nrf_mesh_components, stay valid: topology does not change.  The attributes of the mesh are invalidated:
 *   nrf_read_mesh_attributes returns NRF_E_STATE until nrf_mesh_attributes is asked again -- extract, filter, refine, attributes is the
 *   cheap order.  An empty mesh is NRF_OK with zero counts.
 * nrf_read_mesh_refinement: host copies of the current mesh's edge words (uint32 [n_vertices], readable after any extraction or
 *   filter) and of the last refinement's bracket records (float [n_vertices][4], readable only after a refinement of the current
 *   mesh); either may be NULL.
 * The work is enqueued on `stream` (NULL: the context's) and nrf_refine_mesh returns after it has completed, as nrf_extract_mesh does:
 * n_unbracketed has to reach the host.  NRF_E_INVALID: a NULL out; n_steps > 16 (the midpoints are exact up to there).  NRF_E_STATE: no
 * model loaded (also for a mesh made from a caller's lattice on a context without a model); no mesh extracted yet;
 * nrf_read_mesh_refinement with a brackets pointer: no refinement of the current mesh.  A refused call writes nothing.  The calls take
 * no slot of the 16 calls in flight, leave nrf_get_stats untouched and write none of the context's frame buffers. */
typedef struct nrf_mesh_refine {
  uint64_t n_vertices;
  uint64_t n_unbracketed; /* vertices left as they were (in0 == in1) */
  void* vertices;         /* the mesh's vertex buffer, refined in place */
  void* edges;            /* device uint32 [n_vertices] = (p << 3) | m */
  void* brackets;         /* device float4 [n_vertices] = (lo, hi, s_lo, s_hi) */
  uint32_t n_steps;
  uint32_t reserved;      /* written as 0 */
} nrf_mesh_refine;
int nrf_refine_mesh(nrf_context* ctx, uint32_t n_steps, void* stream, nrf_mesh_refine* out);
int nrf_read_mesh_refinement(nrf_context* ctx, uint32_t* edges, float* brackets_f32x4);
/* (ABI 7, addition) Mesh simplification: marching tetrahedra emits about twice the triangles of the cube table, many of them slivers,
 * and a collision proxy, a shadow caster or a preview mesh has a triangle budget.  A coarser lattice loses exactly the thin parts the
 * refinement was written to place, so nrf_simplify_mesh decimates the context's current mesh where it lives, by vertex clustering on
 * the lattice of the last nrf_extract_mesh.  Its representatives are vertices of the mesh itself, so every vertex of the result is an
 * old vertex with its float bits and its edge word -- still on the iso-surface after a refinement, and nrf_refine_mesh afterwards still
 * works.  No model is needed.  Integers and copied float bits, but for the nine fp32 operations of the key:
 *   cluster    the owner point of vertex v is p = word >> 3 = (i * ny + j) * nz + k of its edge word (above).  Its block is
 *              b_c = index_c / factor (integer division) of nb_c = (dims_c - 1) / factor + 1 blocks per axis, and its cluster
 *              cid = (b_x * nb_y + b_y) * nb_z + b_z.  factor = 1 .. 256; factor 1 already merges the up to seven vertices one point owns.
 *   key        the block's centre cc_c = origin_c + (float)((2 * b_c + 1) * factor) * (0.5f * cell_c) (the integer converted to fp32, the
 *              half cell, the product, the sum: one rounding each); d_c = v_c - cc_c with v the vertex's CURRENT position;
 *              d2 = (d_x * d_x + d_y * d_y) + d_z * d_z, three products and two sums in this order, one rounding each;
 *              hi = d2 < +inf ? bits(d2) : 0x7f800000 (NaN and inf rank last; d2 >= +0, so the bits order as the values do);
 *              key = (uint64)hi << 32 | v.
 *   rep        rep(v) = the low word of the minimum key over the vertices of v's cluster: the vertex nearest its block's centre, a tie
 *              going to the smaller id.  A minimum does not depend on the order in which anything ran.
 *   triangles  (a, b, c) maps to (rep a, rep b, rep c) in that order and survives iff the three are pairwise different; a triangle that
 *              names a vertex >= n_vertices is dropped.  Survivors keep their relative order.  Duplicate and mutually opposite
 *              triangles are KEPT, on purpose: the vertex map commutes with the boundary operator, so a closed mesh stays closed as a
 *              chain -- every directed edge occurs as often as its opposite -- and its signed volume keeps a meaning.
 *   vertices   a vertex is kept iff it is a representative and a surviving triangle names it.  Its new id is the number of kept
 *              vertices with a smaller old id; its float bits and its edge word are copied.  The result has no unreferenced vertex.
 *   records    sources[new] = old id, ascending.  vertex_map[old v] = the new id of rep(v), or 0xffffffff where rep(v) was not kept.
 *              (csrc/nrf_simplify_plan.h is this text as code.)
 * nrf_simplify_mesh: the context's mesh BECOMES the simplified mesh, as with nrf_filter_mesh -- nrf_read_mesh, nrf_mesh_components,
 *   nrf_filter_mesh, nrf_refine_mesh, nrf_mesh_attributes and nrf_read_mesh_refinement's edge words all see it; earlier vertices /
 *   triangles / edges pointers are invalid.  It invalidates the labelling, the attributes and the bracket records of the mesh it
 *   replaced: their read calls return NRF_E_STATE until asked again.  sources and vertex_map stay valid until the next nrf_extract_mesh,
 *   nrf_filter_mesh, nrf_simplify_mesh or nrf_destroy.  An empty mesh, or a result with nothing left, is NRF_OK with zero counts.
 *   Memory: a dense key table of 8 bytes per cluster -- 16 MB for a 256^3 lattice at factor 2, 128 MB at factor 1 -- and 4 bytes per
 *   vertex and per triangle of flags, owned by the context and kept for the next call.
 * nrf_read_mesh_simplification: host copies of the last simplification's records: uint32 [n_vertices] and uint32 [n_vertices_before];
 *   either may be NULL.
 * The work is enqueued on `stream` (NULL: the context's) and nrf_simplify_mesh returns after it has completed, as nrf_filter_mesh does:
 * the sizes have to reach the host.  NRF_E_INVALID: a NULL out; factor 0 or > 256.  NRF_E_STATE: no mesh extracted yet;
 * nrf_read_mesh_simplification: no simplification of the current mesh.  NRF_E_HIP with a message: a scatter write fell outside the
 * counted sizes (every write is checked, as in the filter).  A refused call writes nothing.  The calls take no slot of the 16 calls in
 * flight, leave nrf_get_stats untouched and write none of the context's frame buffers. */
typedef struct nrf_mesh_simplify {
  uint64_t n_vertices, n_triangles;               /* after */
  uint64_t n_vertices_before, n_triangles_before;
  void* vertices;    /* device float [n_vertices][3]: the context's mesh */
  void* triangles;   /* device uint32 [n_triangles][3] */
  void* edges;       /* device uint32 [n_vertices]: the kept vertices' edge words */
  void* sources;     /* device uint32 [n_vertices] */
  void* vertex_map;  /* device uint32 [n_vertices_before] */
  uint32_t factor;
  uint32_t reserved; /* written as 0 */
} nrf_mesh_simplify;
int nrf_simplify_mesh(nrf_context* ctx, uint32_t factor, void* stream, nrf_mesh_simplify* out);
int nrf_read_mesh_simplification(nrf_context* ctx, uint32_t* sources, uint32_t* vertex_map);
/* (ABI 7, addition) The mesh texture: the colours of the full network baked into a per-triangle texture atlas of the context's current
 * mesh, so that the resolution of its appearance is chosen independently of its triangle budget (one colour per vertex is all
 * nrf_mesh_attributes hands out, and nrf_simplify_mesh lowers the vertex count).  A lane of the kernel makes its texel's position and
 * direction itself; nothing but the counters leaves the device.  All integer arithmetic is exact; every fp32 operation is ONE rounding
 * (no contraction), the division and the square root the correctly rounded IEEE ones, so a host can replay it:
 *   parameters res = r texels along a triangle's legs, 2 <= r <= 256; width = the atlas width in texels, r + 2 <= width <= 16384.
 *   cells      triangles are paired: pair q = t >> 1 owns a cell of (r + 2) x (r + 1) texels.  cols = width / (r + 2) (integer
 *              division), rows = ceil(n_pairs / cols), height = rows * (r + 1); pair q's cell origin is (x0, y0) = ((q % cols) * (r + 2),
 *              (q / cols) * (r + 1)).  height <= 16384 and width * height <= 2^26; an empty mesh has height 0.
 *   ownership  a cell texel (i', j'), 0 <= i' <= r + 1, 0 <= j' <= r, belongs to the even triangle 2q with (i, j) = (i', j') if
 *              i' + j' <= r, and otherwise to the odd triangle 2q + 1 with (i, j) = (r + 1 - i', r - j').  Each half holds
 *              (r + 1)(r + 2) / 2 texels and the two tile the cell exactly.  The corners of a triangle (a, b, c) sit at the texel centres
 *              (i, j) = (0, 0), (r - 1, 0), (0, r - 1); the texels with i + j = r, and (r, 0) and (0, r), lie one step outside the
 *              hypotenuse and are evaluated at the extrapolated position in the triangle's plane: a bilinear fetch anywhere inside the
 *              triangle reads texels of the same triangle only.
 *   position   of texel (i, j) of triangle (a, b, c) with the mesh's CURRENT vertex positions va, vb, vc: s = (float)i / (float)(r - 1),
 *              t = (float)j / (float)(r - 1), e1_k = vb_k - va_k, e2_k = vc_k - va_k, x_k = (va_k + s * e1_k) + t * e2_k: the products are
 *              rounded, then the sums, in this order.
 *   direction  n_x = e1_y * e2_z - e1_z * e2_y and cyclically: two rounded products and one rounded difference -- the outward face
 *              normal by the extraction's orientation rule.  d = the unit direction of (-n_x, -n_y, -n_z) as nrf_point_attributes forms
 *              one from a gradient (above; the negations are exact): the head-on viewing direction.  A degenerate triangle (l2 not finite
 *              or < 2^-60) has d = (0, 0, 0) and is still coloured.  The network is given 0.5f * d_k (rounded), then + 0.5f (rounded).
 *   guard      a texel is evaluated if and only if its triangle exists (t < n_triangles), names only vertices < n_vertices, and every
 *              x_k is finite with |x_k| <= bound (the one-tap guard of nrf_density).  A refused texel is zeros in every plane and nothing
 *              of it is gathered.  An index is checked before it becomes an address.
 *   texel      (r, g, b, sigma) = nrf_network at (x, d), bit for bit.  rgba8 = u8(r) | u8(g) << 8 | u8(b) << 16 | 255 << 24 with the
 *              8-bit rule of nrf_read_u8 ((unsigned char)(255.0 * x), saturating, NaN -> 0).  An atlas texel that no triangle owns or
 *              whose texel was refused -- the right margin, the cells after the last pair, the odd half of the last cell when
 *              n_triangles is odd -- is zeros in both planes: rgba8's alpha is the coverage mask.
 *   uvs        float [n_triangles][3][2].  A corner at atlas texel (px, py) has u = ((float)px + 0.5f) / (float)width and
 *              v = ((float)py + 0.5f) / (float)height (v grows with the atlas row).  Even triangle, corners a, b, c: (x0, y0),
 *              (x0 + r - 1, y0), (x0, y0 + r - 1); odd: (x0 + r + 1, y0 + r), (x0 + 2, y0 + r), (x0 + r + 1, y0 + 1).
 * nrf_mesh_texture_size: the height of the atlas of n_triangles at (res, width); host only, no context.
 * nrf_bake_mesh_texture: bakes the context's current mesh -- after nrf_filter_mesh, nrf_refine_mesh and nrf_simplify_mesh is the intended
 *   place -- into three buffers owned by the context; they grow as needed and stay valid until the next nrf_extract_mesh,
 *   nrf_filter_mesh, nrf_refine_mesh, nrf_simplify_mesh, nrf_bake_mesh_texture or nrf_destroy.  Each of the first four invalidates the
 *   texture: nrf_read_mesh_texture returns NRF_E_STATE until the mesh is baked again.  The mesh itself, its labelling, its attributes and
 *   its refinement records are untouched.  n_refused counts the texels of existing triangles that the guard zeroed.  The work is enqueued
 *   on `stream` (NULL: the context's) and the call returns after it has completed: n_refused has to reach the host.  An empty mesh is
 *   NRF_OK with height 0 and NULL pointers.
 * nrf_read_mesh_texture: host copies of the last bake: float [height][width][4], uint32 [height][width], float [n_triangles][3][2];
 *   each may be NULL.
 * NRF_E_INVALID: a NULL out (nrf_mesh_texture_size: height); res or width out of range; an atlas beyond the height or texel limits --
 * the message names the smallest width that would fit, or says that none does.  NRF_E_STATE: no model loaded (also for a mesh made from
 * a caller's lattice on a context without a model: there is no network to ask); no mesh extracted yet; nrf_read_mesh_texture: no texture
 * of the current mesh.  A refused call writes nothing.  The calls take no slot of the 16 calls in flight, leave nrf_get_stats untouched
 * and write none of the context's frame buffers.
 * (csrc/nrf_bake_plan.h is this text as code.) */
typedef struct nrf_mesh_texture {
  uint32_t width, height, res, cols;
  uint64_t n_triangles;
  uint64_t n_refused; /* owned texels the guard zeroed */
  void* texels;       /* device float4 [height][width] = (r, g, b, sigma) */
  void* rgba8;        /* device uint32 [height][width] */
  void* uvs;          /* device float [n_triangles][3][2] */
} nrf_mesh_texture;
int nrf_mesh_texture_size(uint64_t n_triangles, uint32_t res, uint32_t width, uint32_t* height); /* host only */
int nrf_bake_mesh_texture(nrf_context* ctx, uint32_t res, uint32_t width, void* stream, nrf_mesh_texture* out);
int nrf_read_mesh_texture(nrf_context* ctx, float* texels_f32x4, uint32_t* rgba8, float* uvs); /* each may be NULL */
/* set_rays_o/d + kernel_near_far_from_aabb for every pixel (row-major):
 * rays_o [n][3], rays_d [n][3], nears [n], fars [n]                          */
int nrf_generate_rays(nrf_context* ctx, const float cam[4], const float pose[16],
                      void* rays_o, void* rays_d, void* nears, void* fars,
                      void* stream);
/* Same with HOST output arrays (any may be NULL); NerfRender::generate_rays
 * (nerf_render.cu:369-386) for callers that hold no device memory.           */
int nrf_generate_rays_host(nrf_context* ctx, const float cam[4], const float pose[16],
                           float* rays_o, float* rays_d, float* nears, float* fars);
/* kernel_march_rays (render_utils.h:524-655) for n rays with explicit start
 * t: xyzs [n][n_step][3], dirs likewise, deltas [n][n_step][2]; unused slots
 * are zero-filled (DESIGN.md deviation D-1).                                 */
int nrf_march(nrf_context* ctx, const void* rays_o, const void* rays_d,
              const void* rays_t, const void* fars, uint32_t n, uint32_t n_step,
              void* xyzs, void* dirs, void* deltas, void* stream);
/* kernel_composite_rays (render_utils.h:658-751): state [n][5] =
 * (weight_sum, depth, r, g, b) updated in place; rays_t in/out               */
int nrf_composite(nrf_context* ctx, const void* sigmas, const void* rgbs,
                  const void* deltas, uint32_t n, uint32_t n_step, void* rays_t,
                  void* state, void* stream);

/* ---- render buffer (presentation chain) -----------------------------------
 * Replaces ngp::CudaRenderBuffer (include/nerf-cuda/render_buffer.h:160-315,
 * src/render_buffer.cu:224-259 accumulate_kernel, :261-342 tonemap,
 * :529-556 tonemap_kernel, :590-627).  The frame buffer is RGBA fp32 + depth
 * on the device: bind it as the render target with
 * nrf_bind_output(ctx, rgba, depth) and the kernel composites straight into
 * it (the reference goes through host u8, main.cu:87-129).  The GL / CUDA-surface
 * parts of the reference class are out of scope; the tonemapped result goes
 * to a plain RGBA fp32 "surface" buffer, and the class's three overlays
 * (depth, image, false colour) blend over it (below).  Where the
 * reference class has DLSS, nrf_rb_enable_upscale / nrf_rb_upscale (below)
 * upscale that surface on the device.                                        */
enum { NRF_CS_LINEAR = 0, NRF_CS_SRGB = 1, NRF_CS_VISPOSNEG = 2 };          /* EColorSpace, common.h:93-97     */
enum { NRF_TM_IDENTITY = 0, NRF_TM_ACES = 1, NRF_TM_HABLE = 2, NRF_TM_REINHARD = 3 }; /* ETonemapCurve :100-105 */
typedef struct nrf_render_buffer nrf_render_buffer;
int nrf_rb_create(int device, nrf_render_buffer** out);
int nrf_rb_destroy(nrf_render_buffer* rb);
int nrf_rb_resize(nrf_render_buffer* rb, int width, int height);           /* resize(), zero-fills           */
int nrf_rb_reset_accumulation(nrf_render_buffer* rb);                      /* m_spp = 0                      */
int nrf_rb_spp(nrf_render_buffer* rb, uint32_t* spp);
int nrf_rb_set_color_space(nrf_render_buffer* rb, int color_space);        /* m_color_space                  */
int nrf_rb_set_tonemap_curve(nrf_render_buffer* rb, int curve);            /* m_tonemap_curve                */
/* device pointers: frame RGBA [h][w][4], depth [h][w], accumulate RGBA, surface RGBA (tonemap output) */
int nrf_rb_buffers(nrf_render_buffer* rb, void** frame, void** depth, void** accumulate, void** surface);
int nrf_rb_clear_frame(nrf_render_buffer* rb, void* stream);               /* clear_frame()                  */
int nrf_rb_accumulate(nrf_render_buffer* rb, float exposure, void* stream);/* accumulate(): running mean     */
int nrf_rb_tonemap(nrf_render_buffer* rb, float exposure, const float background_color[4],
                   int output_color_space, void* stream);                  /* tonemap()                      */
/* accumulate() + tonemap() of the reference's per-frame sequence (main.cu:87-129, render_buffer.cu:590-627) as ONE pass over
 * the planes: reads the frame (and the mean so far, unless this is the first sample), writes the new mean and the developed
 * surface -- 64 B per pixel instead of 96 for the two calls; the planes hold the same bits as after nrf_rb_accumulate +
 * nrf_rb_tonemap.  rgba8 (optional, device, uint32 [h][w]): the surface as 8-bit r | g << 8 | b << 16 | a << 24 (saturating,
 * NaN -> 0: the library's 8-bit rule), what a display or an encoder takes; NULL: not written.                       */
int nrf_rb_present(nrf_render_buffer* rb, float exposure, const float background_color[4],
                   int output_color_space, void* rgba8, void* stream);
/* host_to_accumulate_buffer(): rgb u8 [n][3] -> accumulate RGBA = rgb/255, a = 1 (render_buffer.h:231-241) */
/* overlay_depth() (render_buffer.cu:431-477, 690-714): turbo-coloured depth (device float plane of
 * image_width x image_height, e.g. nrf_frame.depth) blended over the surface with weight alpha.     */
int nrf_rb_overlay_depth(nrf_render_buffer* rb, float alpha, const void* depth, float depth_scale,
                         int image_width, int image_height, int fov_axis, float zoom,
                         const float screen_center[2], void* stream);
int nrf_rb_host_to_accumulate_buffer(nrf_render_buffer* rb, const uint8_t* rgb, int n);
int nrf_rb_read(nrf_render_buffer* rb, float* accumulate_rgba, float* surface_rgba);  /* host copies (either may be NULL) */
/* (ABI 7, addition) The image overlay, the false-colour overlay and the error map: the two remaining public methods of the reference's
 * CudaRenderBuffer (overlay_image, render_buffer.cu:341-411, 656-688; overlay_false_color, :479-527, 716-733) and the producer of what the
 * second one reads.  Every fp32 operation is ONE rounding (no contraction), every integer operation exact, in the order of the
 * reference's source text; the one transcendental function is the power inside the sRGB pair.  W x H is the surface.
 *   pixel mapping   (nrf_rb_overlay_depth's) surface pixel (x, y) -> (srcx, srcy) of an iw x ih image:
 *                   scale = (float)(fov_axis == 0 ? iw : ih) / (float)(fov_axis == 0 ? W : H);
 *                   fx = (float)x + 0.5f; fx -= (float)W * 0.5f; fx /= zoom; fx += screen_center[0] * (float)W; fy likewise with H and
 *                   screen_center[1]; u = (fx - (float)W * 0.5f) * scale + (float)iw * 0.5f; v likewise; srcx = (int)floorf(u),
 *                   srcy = (int)floorf(v), where the conversion saturates and a NaN gives an index outside the image.
 *   image texels    image_data_type is the reference's EImageDataType.  NRF_IMG_BYTE: uint32 texels r | g << 8 | b << 16 | a << 24, sRGB
 *                   with straight alpha.  The texel 0x00FF00FF gives (-1, -1, -1, -1); otherwise a = (float)b3 * (1.0f / 255.0f) and
 *                   channel = T[b] * a with T[b] = srgb_to_linear((float)b * (1.0f / 255.0f)), b = 0 .. 255, a table the library makes
 *                   ONCE on the host with libm (nrf_rb_srgb8_table returns it) -- the one deliberate difference from evaluating the
 *                   power per pixel on the device: a Byte image is bit-exact against a CPU compile of the reference.  NRF_IMG_HALF:
 *                   four fp16 values per texel, widened exactly.  NRF_IMG_FLOAT: four fp32 values.  Premultiplied linear values both.
 *   nrf_rb_overlay_image, per surface pixel: val = the texel at (srcx, srcy), zeros when that lies outside the image.  Render colour
 *                   space sRGB: rgb = linear_to_srgb(rgb / w) * w for w > 0, else 0; otherwise the background colour (given as sRGB) is
 *                   decoded on the host once per call, as nrf_rb_tonemap does.  weight = (1 - w) * bg.w; rgb += bg.rgb * weight;
 *                   w += weight.  Then the reference's five-argument tonemap: srgb_to_linear if the render space is sRGB, times
 *                   powf(2, exposure[k]) per channel (made on the host), the buffer's film curve (the curves' max(x, 0) is fmaxf), and
 *                   linear_to_srgb if output_color_space is sRGB.  surface = color * alpha + surface * (1.f - alpha), all four channels.
 *   nrf_rb_overlay_false_color, per surface pixel: error_map_scale = brightness / (0.0000001f + average[0]);
 *                   scale = (float)(fov_axis == 0 ? tw : th) / (float)(fov_axis == 0 ? W : H) with tw x th the training resolution;
 *                   u = ((float)x + 0.5f - (float)W * 0.5f) * scale + (float)tw * 0.5f, v likewise;
 *                   srcx = (int)floorf(u * (float)map_width / fmaxf(1.f, (float)tw)), srcy likewise (the same conversion).  A pixel
 *                   outside the map is left untouched.  err = map[srcy][srcx] * error_map_scale; with viridis err *= 1.f / (1.f + err).
 *                   c = colormap_viridis(err) -- c0 + x (c1 + x (c2 + x (c3 + x (c4 + x (c5 + x c6))))) per channel on x clamped to
 *                   [0, 1] -- or colormap_turbo(err), nrf_rb_overlay_depth's.  grey = r * 0.2126f + g * 0.7152f + b * 0.0722f, summed
 *                   left to right; rgb = grey * sat(c) with sat clamping to [0, 1] and NaN -> 0; alpha untouched.  (The reference's
 *                   to_srgb argument is dead in its kernel and is not part of this call.)
 *   nrf_rb_error_map (this library's definition: the reference fills its map while training): the surface S against a truth plane G,
 *                   both float4 [H][W], into a map float [map_height][map_width] with 1 <= map_width <= min(W, 512),
 *                   1 <= map_height <= min(H, 512), and its average, one float.  Cell cx covers columns x0(cx) .. x0(cx + 1) - 1 with
 *                   x0(c) = (c * W + map_width - 1) / map_width in integers, rows likewise: every cell holds at least one pixel.  Per
 *                   pixel e = (((dr * dr) + (dg * dg)) + (db * db)) / 3.0f with d = S - G; alpha is ignored.  A cell is reduced in a
 *                   fixed order: with its pixels row-major as k = 0, 1, ..., v[l] (l = 0 .. 63) adds e_k for k = l (mod 64) in
 *                   ascending k onto 0.0f; then for s = 32, 16, ..., 1 and l < s, v[l] = v[l] + v[l + s]; the cell's value is
 *                   v[0] / (float)count.  The average is the same scheme over the cells in row-major order:
 *                   average[0] = v[0] / (float)(map_width * map_height).  NaNs propagate.  The average is the MEAN OF THE CELL MEANS: it
 *                   equals the image's mean squared error only when map_width divides W and map_height divides H.
 * image, error_map, average and truth_f32x4 are device pointers; error_map and average of nrf_rb_error_map may be handed to
 * nrf_rb_overlay_false_color as they are, on the same stream.  Stream rules are nrf_rb_overlay_depth's (NULL: the buffer's stream, and
 * the call returns after the work has completed).  NRF_E_STATE before a resize.  NRF_E_INVALID, with nothing written: a NULL pointer, an
 * unknown data type or colour space, a fov_axis other than 0 or 1, an image, training or surface size <= 0 or above 16384 on an axis, map
 * sizes outside 1 .. 512 (nrf_rb_error_map: outside the bounds above), a zoom that is zero or not finite, a screen_center that is not
 * finite.  nrf_rb_srgb8_table is host only and needs no device.
 * (csrc/nrf_overlay_plan.h is this text as code.) */
enum { NRF_IMG_BYTE = 1, NRF_IMG_HALF = 2, NRF_IMG_FLOAT = 3 };              /* EImageDataType, common.h */
int nrf_rb_srgb8_table(float table[256]);                                   /* host only */
int nrf_rb_overlay_image(nrf_render_buffer* rb, float alpha, const float exposure[3], const float background_color[4],
                         int output_color_space, const void* image, int image_data_type, int image_width, int image_height,
                         int fov_axis, float zoom, const float screen_center[2], void* stream);
int nrf_rb_overlay_false_color(nrf_render_buffer* rb, int training_width, int training_height, int fov_axis,
                               const void* error_map, int map_width, int map_height, const void* average,
                               float brightness, int viridis, void* stream);
int nrf_rb_error_map(nrf_render_buffer* rb, const void* truth_f32x4, int map_width, int map_height,
                     void* error_map, void* average, void* stream);
/* (ABI 7, addition) The upscaler: the developed surface at the render resolution -> a plane at an output resolution, on the device, in ONE
 * kernel launch -- bicubic (Catmull-Rom) reconstruction with a de-ringing clamp, then a clamped unsharp mask.  It stands where the
 * reference's render buffer has DLSS (enable_dlss / set_dlss_sharpening / in_resolution / out_resolution, dlss.png of main.cu:171-206) and
 * is NOT DLSS: purely spatial, one frame in, no motion vectors, no depth, no history, no learned filter.  What it is instead is
 * deterministic: every fp32 operation is ONE rounding (no contraction), every integer operation exact, no transcendental function, so a
 * host can replay it bit for bit:
 *   planes     the source plane P is [IH][IW] float4 (the surface), the target plane [OH][OW] float4.
 *   geometry   per axis: r = (float)I / (float)O, computed once on the host.  For output index X: s = ((float)X + 0.5f) * r - 0.5f -- the
 *              sum is rounded, then the product, then the difference; i = (int)floorf(s), f = s - (float)i (exact, 0 <= f < 1).  The tap
 *              indices are i - 1, i, i + 1, i + 2, each clamped to [0, I - 1] as integers.
 *   weights    of t = f, every operation as parenthesised: w0 = t * (-0.5f + t * (1.0f - 0.5f * t)),
 *              w1 = 1.0f + (t * t) * (-2.5f + 1.5f * t), w2 = t * (0.5f + t * (2.0f - 1.5f * t)), w3 = (t * t) * (-0.5f + 0.5f * t).
 *   stage 1    reconstruction, per channel, all four channels: for each of the four tap rows j,
 *              h_j = ((wx0 * p0 + wx1 * p1) + wx2 * p2) + wx3 * p3; then v = ((wy0 * h_0 + wy1 * h_1) + wy2 * h_2) + wy3 * h_3.
 *              De-ringing: lo and hi are the fminf / fmaxf over the four inner texels (columns i, i + 1 and rows i, i + 1, with the
 *              clamped indices), taken as f(f(p11, p12), f(p21, p22)) row by row; U = fminf(fmaxf(v, lo), hi).
 *   stage 2    sharpening, on the plane U at the output resolution, channels r, g, b (alpha is U's alpha): n, s, w, e are the four
 *              neighbours of c = U[Y][X] with indices clamped to the plane; blur = ((n + s) + (w + e)) * 0.25f, d = c - blur,
 *              x = c + amount * d, out = fminf(fmaxf(x, min(c, n, s, w, e)), max(c, n, s, w, e)), the minima and maxima nested fminf /
 *              fmaxf from the left.
 *   packed     rgba8 = u8(r) | u8(g) << 8 | u8(b) << 16 | u8(a) << 24 of out with the library's 8-bit rule ((unsigned char)(255.0 * x),
 *              saturating, NaN -> 0).
 *   it follows at equal resolutions and amount 0 the output equals the surface as values; amount 0 makes stage 2 the identity bit for
 *              bit; a constant plane stays constant bit for bit at any ratio and amount; a 1 x 1 plane upscales to copies of its texel;
 *              every output channel lies within the minimum and maximum of that channel over the source.
 * nrf_rb_enable_upscale: needs a resized buffer (else NRF_E_STATE); in <= out <= 8 * in and out <= 16384 per axis (else NRF_E_INVALID and
 *   nothing changes); the two axes may have different ratios and the ratios need not be integers.  Allocates the upscaled plane,
 *   zero-filled; calling it again replaces the output resolution.  While it is enabled nrf_rb_resize checks the new size against the output
 *   resolution under the same rule before anything is freed: a size that does not fit is NRF_E_INVALID and leaves the buffer as it was.
 * nrf_rb_disable_upscale: frees the plane.  nrf_rb_upscale, nrf_rb_upscaled and nrf_rb_read_upscaled return NRF_E_STATE then, as they do
 *   before an enable; nrf_rb_resolutions reports out == in while disabled (either array may be NULL).
 * nrf_rb_set_upscale_sharpening: 0 <= amount <= 2 (NaN: NRF_E_INVALID); the default is 0, the value the reference's testbed sets.
 * nrf_rb_upscale: reads the surface as the last nrf_rb_tonemap, nrf_rb_present or nrf_rb_overlay_depth left it and writes the upscaled
 *   plane; with rgba8 != NULL also device uint32 [out_h][out_w] of the same pixels.  Stream rules are nrf_rb_present's (NULL: the
 *   buffer's stream, and the call returns after the work has completed).  Surface, accumulate plane and spp are untouched.
 * (csrc/nrf_upscale_plan.h is this text as code.) */
int nrf_rb_enable_upscale(nrf_render_buffer* rb, int out_width, int out_height);  /* enable_dlss(out_res) */
int nrf_rb_disable_upscale(nrf_render_buffer* rb);                                /* disable_dlss()       */
int nrf_rb_set_upscale_sharpening(nrf_render_buffer* rb, float amount);           /* set_dlss_sharpening  */
int nrf_rb_resolutions(nrf_render_buffer* rb, int in_wh[2], int out_wh[2]);       /* in_/out_resolution() */
int nrf_rb_upscale(nrf_render_buffer* rb, void* rgba8, void* stream);
int nrf_rb_upscaled(nrf_render_buffer* rb, void** plane);     /* device float4 [out_h][out_w] */
int nrf_rb_read_upscaled(nrf_render_buffer* rb, float* rgba); /* host copy [out_h][out_w][4]  */
/* (ABI 7, addition) The temporal upscaler: an accumulator at the output resolution over a sequence of jittered frames at the render
 * resolution -- how the reference drives DLSS (a per-frame sub-pixel jitter, a reset flag on sample 0, depth and motion vectors;
 * render_buffer.cu:636-653, main.cu:53-85).  A NeRF is a static scene, so every motion vector follows from the two cameras and the depth
 * the renderer has (the motion vectors, below).  Still no learned filter, and moving scene content is not handled.  Like the
 * spatial upscaler it is defined operation by operation: every fp32 operation is ONE rounding, division is the correctly rounded IEEE
 * one, integer arithmetic is exact, no transcendental function.
 *   planes     P [IH][IW] float4 is the surface.  The history colour H [OH][OW] float4 (never sharpened) and the history weight Wt
 *              [OH][OW] float exist twice, previous and current, swapped after each call.  The presented plane is the upscaled plane.
 *   jitter     j = (jx, jy), each finite and in [-0.5, 0.5]: the sample of render pixel (x, y) was taken at (x + 0.5 + jx, y + 0.5 + jy)
 *              in render pixels.  A pinhole frame gets that by rendering with cam = (fl_x, fl_y, cx - jx, cy - jy).
 *   source     per axis: s = the spatial upscaler's s - j (one more rounded subtraction), i = (int)floorf(s), f = s - (float)i (rounded: it
 *              may reach 1).  Taps and weights as in the spatial upscaler, of i and f.
 *   current    C = stage 1 of the spatial upscaler (de-ringing included) at this s.  With j = (0, 0) it is its U bit for bit.
 *   weight     per axis: n = clamp((int)floorf(s + 0.5f), 0, I - 1), d = (s - (float)n) * o with o = (float)O / (float)I from the host;
 *              a = dx * dx + dy * dy, b = fmaxf(1.0f - a, 0.0f), wc = fmaxf(b * b, 0.015625f).
 *   history    motion is a float2 [IH][IW] plane in OUTPUT pixels, or NULL; the vector m of output pixel (X, Y) is the entry of render
 *              pixel (nx, ny) above; q = ((float)X + mx, (float)Y + my).  motion NULL or m exactly (0, 0): Hq and Wq are the previous
 *              planes' texels at (X, Y), no arithmetic.  Otherwise, if m is finite and -0.5 <= q_c <= (float)O_c - 0.5f on both axes: Hq is
 *              stage 1 (de-ringing included) on the previous H at base (int)floorf(q_c) and fraction q_c - floorf(q_c), indices clamped
 *              to the plane; Wq is the previous Wt at clamp((int)floorf(q_c + 0.5f), 0, O_c - 1).  In every other case Wq = 0.
 *              NRF_UPSCALE_T_RESET makes Wq = 0 everywhere and reads no history.
 *   rectify    only with NRF_UPSCALE_T_RECTIFY and only where history is blended: per channel Hq = fminf(fmaxf(Hq, lo), hi); lo / hi are
 *              fminf / fmaxf nested from the left over the 3 x 3 render texels around (nx, ny) in row-major order, indices clamped.
 *              From a static camera it costs several dB, because it cuts off exactly the detail between samples: it is for moving cameras.
 *   blend      wh = fminf(Wq, max_history).  wh > 0: tot = wh + wc, alpha = wc / tot, H' = Hq + alpha * (C - Hq) per channel (all four),
 *              Wt' = tot.  Otherwise (reset, no history, NaN): H' = C, Wt' = wc.
 *   presented  stage 2 of the spatial upscaler (the buffer's sharpening amount) on the plane H', and the packed pixel if asked.
 *   sequence   jitter_k = (halton2(k + 1) - 0.5f, halton3(k + 1) - 0.5f) with the reference's recurrence: f = 1, r = 0; while i > 0:
 *              f = f / base, r = r + f * (float)(i % base), i /= base.  (The reference keeps this Halton variant commented out beside its
 *              scrambled Sobol sequence; that one needs the reference's direction tables and is not restated.)
 *   motion     of a render pixel: each of the two cameras is a pose in ngp form (rotation R and centre c, exactly as the render call
 *              converts a pose, with the loaded model's scale; 1 while none is loaded) and cam = (fl_x, fl_y, cx, cy).  For a point x:
 *              v = x - c, p_k = (R[0][k] * v_0 + R[1][k] * v_1) + R[2][k] * v_2; p_z not finite or <= 0: invalid; else
 *              u = (p_x / p_z) * fl_x + cx, w = (p_y / p_z) * fl_y + cy.  x = o + t * d (the product rounded, then the sum) with
 *              t = depth / alpha where alpha >= min_alpha and t is finite and > 0; otherwise the pixel is at infinity: v = d for both
 *              cameras.  m = ((u_prev - u_cur) * ox, (w_prev - w_cur) * oy); either projection invalid or the ray not finite:
 *              m = (+inf, +inf), which the fetch above reads as no history.  Both projections go through the unjittered cameras.
 * The jitter call is host only.  The history length is 1 <= max_history <= 256 (NaN: NRF_E_INVALID), default 64.
 * The temporal call needs an enabled upscale (else NRF_E_STATE).  The four history planes are allocated, zero-filled, by the first call
 *   and freed by nrf_rb_disable_upscale; nrf_rb_enable_upscale and nrf_rb_resize drop them, and the next call then behaves as a reset with
 *   n_frames restarting at 0, as the first call ever does whatever the flag says.  NRF_E_INVALID with nothing written: a jitter that is not
 *   finite or outside [-0.5, 0.5], an unknown flag, reserved != 0.  Stream rules are nrf_rb_upscale's.  nrf_rb_upscale between two temporal
 *   calls overwrites the presented plane only.  A buffer that never makes the temporal call allocates nothing for it.
 * The history calls return the planes the last temporal call wrote (device pointers, NULL before the first; the host copy returns
 *   NRF_E_STATE then) and the number of calls since the history began.
 * The motion call takes the row-major planes of a NRF_RAYS_DEPTH_T ray frame (rgba for alpha, depth_t for the sum of w t) and the rays
 *   that made it (the jittered ones will do), writes float2 [height][width]; it needs no model, takes no slot of the calls in flight and
 *   leaves the statistics alone.  NRF_E_INVALID: NULL pointers, resolutions outside in <= out <= 8 * in, out <= 16384, a min_alpha that is
 *   not in (0, 1], reserved != 0.
 * (csrc/nrf_temporal_plan.h is this text as code.) */
enum { NRF_UPSCALE_T_RESET = 1, NRF_UPSCALE_T_RECTIFY = 2 };
typedef struct nrf_upscale_temporal {
  const void* motion;   /* device float2 [in_h][in_w] in output pixels, or NULL */
  float jitter[2];
  uint32_t flags;       /* NRF_UPSCALE_T_* */
  uint32_t reserved;    /* 0 */
} nrf_upscale_temporal;
int nrf_rb_upscale_jitter(uint32_t index, float jitter[2]);                 /* host only */
int nrf_rb_set_upscale_history(nrf_render_buffer* rb, float max_history);   /* 1..256, default 64; NaN invalid */
int nrf_rb_upscale_temporal(nrf_render_buffer* rb, const nrf_upscale_temporal* t, void* rgba8, void* stream);
int nrf_rb_upscale_history(nrf_render_buffer* rb, void** history, void** weight, uint32_t* n_frames);
int nrf_rb_read_upscale_history(nrf_render_buffer* rb, float* rgba, float* weight);
typedef struct nrf_motion {
  const void* rays_o;   /* device float [height][width][3] */
  const void* rays_d;   /* device float [height][width][3] */
  const void* rgba;     /* device float4 [height][width]: alpha in w */
  const void* depth_t;  /* device float [height][width]: the sum of w t */
  int32_t width, height, out_width, out_height;
  float min_alpha;
  float cam[4], pose[16], prev_cam[4], prev_pose[16];
  uint32_t reserved;    /* 0 */
} nrf_motion;
int nrf_motion_vectors(nrf_context* ctx, const nrf_motion* m, void* motion_f32x2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERFHIP_H_ */
