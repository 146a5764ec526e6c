// nrf_model_plan.h -- the model side of the host's plan, without a device: no call of the HIP runtime (hipcc's host pass builds it:
// the level table, the fragments and the generic description are the device headers' types).  plan_model decides what a model
// descriptor makes of the device side, build_model_image makes the bytes every render instance reads; nrf_api.hip's
// nrf_load_model uploads them.  nrf_debug_model_image returns them (tests/test_model_image_cpu.py), host/model_plan_asan.cpp
// runs them under the sanitizers.  A refusal comes back as a code and its text (`why`): nrf_api.hip hands both to nrf_last_error.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "nrf_device.h"
#include "nrf_generic.h"
#include "nrf_launch.h"

namespace nrf {

inline int refuse(const char*& why, int code, const char* msg) {
  why = msg;
  return code;
}

inline uint32_t next_multiple(uint32_t v, uint32_t d) { return (v + d - 1) / d * d; }

// T/include/tiny-cuda-nn/encodings/grid.h:899-931 (ctor) and :186-190 (kernel): the level geometry is
// computed once, on the host, with libm's exp2f/log2f, and handed to every kernel as constants.
inline int compute_level_table(const nrf_model_desc& d, nrf_level_table& t, const char*& why) {
  if (d.n_levels == 0 || d.n_levels > 16) return refuse(why, NRF_E_UNSUPPORTED, "n_levels must be 1..16");
  if (d.log2_hashmap_size > 31) return refuse(why, NRF_E_INVALID, "log2_hashmap_size must be <= 31");
  std::memset(&t, 0, sizeof(t));
  t.n_levels = d.n_levels;
  const float log2_pls = std::log2(d.per_level_scale);
  uint32_t offset = 0;
  for (uint32_t i = 0; i < d.n_levels; ++i) {
    const float scale = exp2f((float)i * log2_pls) * (float)d.base_resolution - 1.0f;
    const uint32_t res = (uint32_t)ceilf(scale) + 1;
    const uint32_t max_params = std::numeric_limits<uint32_t>::max() / 2;
    uint32_t params = powf((float)res, 3.0f) > (float)max_params ? max_params : res * res * res;
    params = next_multiple(params, 8u);
    if (d.grid_type == NRF_GRID_TILED) {
      const uint32_t b3 = d.base_resolution * d.base_resolution * d.base_resolution;
      params = params < b3 ? params : b3;
    } else if (d.grid_type == NRF_GRID_HASH) {
      const uint32_t T = 1u << d.log2_hashmap_size;
      params = params < T ? params : T;
    } else if (d.grid_type != NRF_GRID_DENSE) {
      return refuse(why, NRF_E_INVALID, "GridEncoding: invalid grid type");
    }
    t.offset[i] = offset;
    t.resolution[i] = res;
    t.scale[i] = scale;
    offset += params;
  }
  t.offset[d.n_levels] = offset;
  return NRF_OK;
}

inline uint32_t dir_raw_width(const nrf_model_desc& d) {
  switch (d.dir_encoding) {
    case NRF_DIR_SH: return d.sh_degree * d.sh_degree;
    case NRF_DIR_FREQUENCY: return 6 * d.n_frequencies;
    case NRF_DIR_IDENTITY: return 3;
    default: return 0;
  }
}

// n_params of NerfNetwork (nerf_network.h:273-291): density MLP | rgb MLP | grid | dir enc (0)
inline int expected_params(const nrf_model_desc& d, const nrf_level_table& t, uint64_t& n, const char*& why) {
  const uint32_t raw = dir_raw_width(d);
  if (raw == 0) return refuse(why, NRF_E_UNSUPPORTED, "unknown dir encoding");
  const uint64_t Wn = d.n_neurons;
  const uint64_t feat = next_multiple(d.n_levels * d.n_features_per_level, 16u);
  const uint64_t rgb_in = next_multiple(next_multiple(raw, 16u) + 16u, 16u);
  if (d.density_hidden_layers < 1 || d.rgb_hidden_layers < 1)
    return refuse(why, NRF_E_INVALID, "FullyFusedMLP requires at least 1 hidden layer (3 layers in total).");  // fully_fused_mlp.cu:653-655
  auto mlp = [&](uint64_t in, uint64_t hidden) { return in * Wn + (hidden - 1) * Wn * Wn + Wn * 16; };
  n = mlp(feat, d.density_hidden_layers) + mlp(rgb_in, d.rgb_hidden_layers) +
      (uint64_t)t.offset[d.n_levels] * d.n_features_per_level;
  return NRF_OK;
}

// fp16 weight fragments for v_mfma_f32_16x16x32_f16 (see nrf_device.h mlp_tiles):
// fragment f, lane l, element j  =  W[16m + (l&15)][kmap(l>>4, j)], zero where kmap names a column beyond the matrix's width `in`
template <class KMap>
inline void put_fragment(std::vector<_Float16>& frags, int f, const _Float16* Wm, int in, int m, KMap kmap) {
  for (int l = 0; l < 64; ++l)
    for (int j = 0; j < 8; ++j) {
      const int k = kmap(l >> 4, j);
      frags[((size_t)f * 64 + l) * 8 + j] = k < in ? Wm[(size_t)(16 * m + (l & 15)) * in + k] : (_Float16)0.0f;
    }
}
// The K maps (g = l >> 4: the lane group).
// First density layer: lane group g holds, in this order, the features of the levels {g, 4 + g, ...} it encodes (F features per level) --
//   F = 2: kmap(g, j) = 2 (4 (j >> 1) + g) + (j & 1)     F = 4: 4 (4 (j >> 2) + g) + (j & 3)     F = 8: 8 g + j     F = 1: 4 j + g (j < 4)
// -- F = 2 is base.json's (levels g, 4+g, 8+g, 12+g); F = 1: level 4 j + g, the lane's upper four are zero columns
inline auto kmap_levels(int F) {
  return [F](int g, int j) {
    if (F == 1) return j < 4 ? 4 * j + g : (1 << 20);
    return F == 2 ? 2 * (4 * (j >> 1) + g) + (j & 1) : (F == 4 ? 4 * (4 * (j >> 2) + g) + (j & 3) : 8 * g + j);
  };
}
// natural order, K step s: column 32 s + 8 g + j (FRAG_D0_NATURAL, FRAG_R0X)
inline auto kmap_natural(int s) {
  return [s](int g, int j) { return 32 * s + 8 * g + j; };
}
// first rgb layer: [density out | dir enc]
inline int kmap_rgb_in(int g, int j) { return j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4); }
// hidden -> next, K step s: a D fragment re-used in-lane as B
inline auto kmap_hidden(int s) {
  return [s](int g, int j) { return 16 * (2 * s + (j >> 2)) + 4 * g + (j & 3); };
}

// The 1 + 2-layer layouts (nrf_device.h MlpShape<W>): D0 [W][feat_w] | D1 [16][W] | R0 [W][rgb_in] | R1 [W][W] | R2 [16][W],
// MT = W / 16 row tiles, KS = ceil(W / 32) K steps; columns beyond a matrix's width are zero (W = 16: the upper half of the one step).
//   hot (W = 64, feat_w = 32, F = 2): the FRAG_* order, fragments 0 .. N_FRAGS - 1
//   width (W = 16 / 32 / 128, feat_w = rgb_in = 32, F = 2): the same order; at W = 64 it IS the hot layout
//   GRID instances (nrf_render.h grid_features; W = 64): the hot layout with the first density layer's K order of a grid of F
//     features per level, feat_w = its padded width (16 or 32); zero columns where the grid has no level (k >= feat_w, or a padded
//     feature of feat_w itself); at F = 2 and feat_w = 32 it IS the hot layout
//   wide_tail (W = 64; R0 [64][rgb_in]: 32 for a 16-wide direction encoding, up to 96): N_FRAGS_WIDE_ALL fragments -- behind the hot
//     ones FRAG_D0_NATURAL (the stage entry points' first density layer) and FRAG_R0X (the wide instance: the columns beyond the
//     first 32, natural order; zero beyond rgb_in)
inline std::vector<_Float16> pack_fragments(const _Float16* w16, int Wd, int feat_w, int F, int rgb_in, bool wide_tail) {
  const int MT = Wd / 16, KS = (Wd + 31) / 32;
  const int fD1 = MT, fR0 = MT + KS, fR1 = 2 * MT + KS, fR2 = 2 * MT + KS + MT * KS, n = 2 * MT + 2 * KS + MT * KS;
  std::vector<_Float16> frags((size_t)(wide_tail ? N_FRAGS_WIDE_ALL : n) * 64 * 8, (_Float16)0.0f);
  const _Float16* D0 = w16;                          // [W][feat_w]
  const _Float16* D1 = D0 + (size_t)Wd * feat_w;     // [16][W]
  const _Float16* R0 = D1 + (size_t)16 * Wd;         // [W][rgb_in]
  const _Float16* R1 = R0 + (size_t)Wd * rgb_in;     // [W][W]
  const _Float16* R2 = R1 + (size_t)Wd * Wd;         // [16][W]
  for (int m = 0; m < MT; ++m) put_fragment(frags, m, D0, feat_w, m, kmap_levels(F));
  for (int s = 0; s < KS; ++s) put_fragment(frags, fD1 + s, D1, Wd, 0, kmap_hidden(s));
  for (int m = 0; m < MT; ++m) put_fragment(frags, fR0 + m, R0, rgb_in, m, kmap_rgb_in);
  for (int m = 0; m < MT; ++m)
    for (int s = 0; s < KS; ++s) put_fragment(frags, fR1 + KS * m + s, R1, Wd, m, kmap_hidden(s));
  for (int s = 0; s < KS; ++s) put_fragment(frags, fR2 + s, R2, Wd, 0, kmap_hidden(s));
  if (wide_tail) {
    for (int m = 0; m < MT; ++m) put_fragment(frags, FRAG_D0_NATURAL + m, D0, feat_w, m, kmap_natural(0));
    for (int s = 1; s < RK_WIDE; ++s)
      for (int m = 0; m < MT; ++m) put_fragment(frags, FRAG_R0X + 4 * (s - 1) + m, R0, rgb_in, m, kmap_natural(s));
  }
  return frags;
}

// DEPTH instance (nrf_device.h DF_*, mlp_tiles_depth): 64 neurons, nd / nr hidden layers in the density / rgb MLP.  Parameter order
// (tcnn): D0 [64][32] | (nd - 1) x [64][64] | D1 [16][64] | R0 [64][32] | (nr - 1) x [64][64] | R2 [16][64].  DEPTH_FRAGS fragments,
// unused ones zero.
inline std::vector<_Float16> pack_fragments_depth(const _Float16* w16, int nd, int nr) {
  std::vector<_Float16> frags((size_t)DEPTH_FRAGS * 64 * 8, (_Float16)0.0f);
  const int xd = nd - 1, xr = nr - 1;
  const _Float16* D0 = w16;
  const _Float16* DW = D0 + 64 * 32;
  const _Float16* D1 = DW + (size_t)xd * 64 * 64;
  const _Float16* R0 = D1 + 16 * 64;
  const _Float16* RW = R0 + 64 * 32;
  const _Float16* R2 = RW + (size_t)xr * 64 * 64;
  for (int m = 0; m < 4; ++m) put_fragment(frags, DF_D0 + m, D0, 32, m, kmap_levels(2));
  for (int s = 0; s < 2; ++s) put_fragment(frags, DF_D1 + s, D1, 64, 0, kmap_hidden(s));
  for (int m = 0; m < 4; ++m) put_fragment(frags, DF_R0 + m, R0, 32, m, kmap_rgb_in);
  for (int s = 0; s < 2; ++s) put_fragment(frags, DF_R2 + s, R2, 64, 0, kmap_hidden(s));
  for (int e = 0; e < xd + xr; ++e) {
    const _Float16* Wm = e < xd ? DW + (size_t)e * 64 * 64 : RW + (size_t)(e - xd) * 64 * 64;
    for (int m = 0; m < 4; ++m)
      for (int s = 0; s < 2; ++s) put_fragment(frags, DF_WW + 8 * e + 2 * m + s, Wm, 64, m, kmap_hidden(s));
  }
  return frags;
}

// Generic instance (nrf_generic.h gen_layer): fragment (m, s) of a layer W[N][K], lane l, element j =
// W[16 m + (l & 15)][32 s + 8 (l >> 4) + j]  (natural K order), zero beyond K.
inline void pack_generic_layer(const _Float16* Wm, uint32_t N, uint32_t K, std::vector<_Float16>& frags) {
  const uint32_t n_tiles = N / 16, k_steps = (K + 31) / 32;
  for (uint32_t m = 0; m < n_tiles; ++m)
    for (uint32_t s = 0; s < k_steps; ++s)
      for (uint32_t l = 0; l < 64; ++l)
        for (uint32_t j = 0; j < 8; ++j) {
          const uint32_t k = 32 * s + 8 * (l >> 4) + j;
          frags.push_back(k < K ? Wm[(size_t)(16 * m + (l & 15)) * K + k] : (_Float16)0.0f);
        }
}

// The matmuls of the two MLPs in parameter order (fully_fused_mlp.cu:636-687): each MLP first [W x in] | hidden [W x W] ... | last
// [16 x W]; act: the activation behind the layer.  The generic instance's fragments and their byte count both walk this list.
struct LayerDim { uint32_t N, K, act; };
inline std::vector<LayerDim> gen_layers(const nrf_model_desc& d, const GenModel& G) {
  std::vector<LayerDim> layers;
  auto add_mlp = [&](uint32_t in, uint32_t hidden, uint32_t act, uint32_t out_act) {
    layers.push_back({G.width, in, act});
    for (uint32_t i = 1; i < hidden; ++i) layers.push_back({G.width, G.width, act});
    layers.push_back({16u, G.width, out_act});
  };
  add_mlp(G.feat_w, d.density_hidden_layers, d.density_activation, d.density_output_activation);
  add_mlp(G.rgb_in, d.rgb_hidden_layers, d.rgb_activation, d.rgb_output_activation);
  return layers;
}
// bytes of the generic instance's weight fragments: pack_generic_layer's 1 KiB per 16 x 32 tile of every layer of the two MLPs
inline uint32_t generic_frag_bytes(const nrf_model_desc& d, const GenModel& G) {
  uint32_t tiles = 0;
  for (const LayerDim& ly : gen_layers(d, G)) tiles += (ly.N / 16) * ((ly.K + 31) / 32);
  return 1024u * tiles;
}

// The descriptor checks of nrf_load_model that come before the old model is released: what the reference's vocabulary allows
// (T/.../grid.h:1403-1411, T/src/fully_fused_mlp.cu:700-725, 653-655; spherical_harmonics.h:394-412); anything outside is
// refused loudly, never emulated on the CPU
inline int validate_model(const nrf_model_desc& d, nrf_level_table& lv, const char*& why) {
  if (d.abi_version != NRF_ABI_VERSION) return refuse(why, NRF_E_INVALID, "abi_version mismatch");
  const uint32_t F = d.n_features_per_level;
  if (F != 1 && F != 2 && F != 4 && F != 8) return refuse(why, NRF_E_INVALID, "GridEncoding: n_features_per_level must be 1, 2, 4, or 8.");
  if (d.interpolation > NRF_INTERP_SMOOTHSTEP) return refuse(why, NRF_E_INVALID, "Invalid interpolation type");
  if (d.n_neurons != 16 && d.n_neurons != 32 && d.n_neurons != 64 && d.n_neurons != 128)
    return refuse(why, NRF_E_INVALID, "FullyFusedMLP: n_neurons must be 16, 32, 64 or 128");
  if (d.density_hidden_layers < 1 || d.rgb_hidden_layers < 1)
    return refuse(why, NRF_E_INVALID, "FullyFusedMLP requires at least 1 hidden layer (3 layers in total).");
  if (d.density_hidden_layers + d.rgb_hidden_layers + 2 > (uint32_t)GEN_MAX_LAYERS)
    return refuse(why, NRF_E_UNSUPPORTED, "HIP path: more than 24 layers in the two MLPs together");
  if (d.density_n_output < 1 || d.density_n_output > 16)  // wider outputs take tcnn's CUTLASS last layer (out of scope)
    return refuse(why, NRF_E_UNSUPPORTED, "HIP path: density n_output_dims must be 1..16");
  const uint32_t raw = dir_raw_width(d);
  if (d.dir_encoding == NRF_DIR_SH && (d.sh_degree < 1 || d.sh_degree > 8))
    return refuse(why, NRF_E_INVALID, "SphericalHarmonics: degree must be 1..8");
  if (raw == 0 || next_multiple(raw, 16u) > (uint32_t)GEN_MAX_DIR_W)
    return refuse(why, NRF_E_UNSUPPORTED, "HIP path: direction encoding must have 1..112 outputs (after padding to 16)");
  if (d.density_grid_size < 2 || d.density_grid_size >= (1u << 24) || d.cascade < 1)
    return refuse(why, NRF_E_INVALID, "bad density grid geometry");
  if (!(d.bound > 0.0f)) return refuse(why, NRF_E_INVALID, "bound must be positive");
  int rc = compute_level_table(d, lv, why);
  if (rc) return rc;
  uint64_t expect = 0;
  rc = expected_params(d, lv, expect, why);
  if (rc) return rc;
  if (d.n_params != expect)  // R/include/nerf-cuda/nerf_network.h:425-427
    return refuse(why, NRF_E_PARAMS, "Can't set params because number of parameters and model size do not match with each other.");
  const uint64_t Hh = d.density_grid_size;
  const uint64_t cells = Hh * Hh * Hh * d.cascade;
  if (d.density_grid && d.n_density_grid != cells)  // R/src/nerf_render.cu:467-469
    return refuse(why, NRF_E_PARAMS, "Incompatible number of grid cascades.");
  if (cells >= (1ull << 32)) return refuse(why, NRF_E_UNSUPPORTED, "density grid too large");
  return NRF_OK;
}

// What a model descriptor makes of the device side, decided without a device (nrf_debug_plan: tests/test_instance_plan_cpu.py).
struct ModelPlan {
  int rc;                    // NRF_OK, or the refusal ...
  const char* why;           // ... and its text
  nrf_level_table lv;
  LevelParams lp[16];        // the device's level table: index modes, entry offsets, byte constants, quad copies
  GenModel gen;              // the generic description without its layers (valid unless stage == NET_HOT)
  uint32_t gen_wave_bytes;   // LDS bytes per wave of its direction + activation rows (0 when stage == NET_HOT)
  uint32_t gen_frag_bytes;   // DevModel::gen_frag_bytes: bytes of the generic instance's weight fragments (0 unless stage == NET_GENERIC)
  bool generic_grid;         // a level of LV_GENERIC index arithmetic
  int own;                   // NET_*: the instance that renders the frames when its march tables fit (plan_grid)
  int stage;                 // NET_HOT, NET_WIDE or NET_GENERIC: the stage entry points, the per-strip kernel, the fallback
  uint32_t quad_mask, quad_far;  // DevModel::quad_mask / quad_far
  uint32_t uni_modes;        // DevModel::uni_modes
  bool static_gather;        // the hot instance may run under a static gather plan
  uint32_t gather_plan;      // DevModel::gather_plan: the static gather plan of the hot instance the steps' forms match, or GATHER_RUNTIME
  uint64_t table_ref_bytes;  // device bytes of the reference-order table
  uint64_t table_bytes;      // ... and of the quad copies behind it
};

// 2 bits per unrolled step jl of the fused kernel (DevModel::uni_modes): its existing levels are all dense (1) / all power-of-two hashed (2)
inline uint32_t uni_modes_of(const LevelParams* lp, uint32_t L) {
  uint32_t uni = 0;
  for (int jl = 0; jl < 4; ++jl) {
    bool all_dense = true, all_hash = true;
    for (int g = 0; g < 4; ++g) {
      if ((uint32_t)(4 * jl + g) >= L) continue;  // (a level the grid does not have: its lanes are masked, grid_features)
      all_dense = all_dense && lp[4 * jl + g].mode == LV_DENSE;
      all_hash = all_hash && lp[4 * jl + g].mode == LV_HASH_POW2;
    }
    uni |= (all_dense ? 1u : (all_hash ? 2u : 0u)) << (2 * jl);
  }
  return uni;
}

// budget_mb: bytes of quad copies allowed (MiB); max_quad_steps: unrolled steps (four levels each) that may have them;
// static_gather: the hot instance may run under a static gather plan (NRF_GATHER_PLAN=0: never)
inline ModelPlan plan_model(const nrf_model_desc& d, bool allow_own, uint64_t budget_mb, int max_quad_steps, bool static_gather = true) {
  ModelPlan p;
  std::memset(&p, 0, sizeof(p));
  p.why = "";
  p.static_gather = static_gather;
  p.rc = validate_model(d, p.lv, p.why);
  if (p.rc) return p;
  const nrf_level_table& lv = p.lv;
  const uint32_t F = d.n_features_per_level, L = d.n_levels, Wn = d.n_neurons;
  for (uint32_t l = 0; l < L; ++l) {
    LevelParams& Lv = p.lp[l];
    Lv.scale = lv.scale[l];
    Lv.res = lv.resolution[l];
    Lv.size = lv.offset[l + 1] - lv.offset[l];
    Lv.hashed = d.grid_type == NRF_GRID_HASH;
    // replay grid_index's stride loop (grid.h:106-114) in uint32 to classify the level
    uint32_t stride = 1, mult[3] = {0, 0, 0};  // mult: what grid_index multiplies x, y, z with (0: the term is skipped)
    int dims = 0;
    for (; dims < 3 && stride <= Lv.size; ++dims) {
      mult[dims] = stride;
      stride *= Lv.res;  // uint32, as in the reference: wraps for res^3 >= 2^32
    }
    const bool uses_hash = Lv.hashed && Lv.size < stride;
    const bool pow2_size = Lv.size >= 2 && (Lv.size & (Lv.size - 1)) == 0;
    if (uses_hash && pow2_size) Lv.mode = LV_HASH_POW2;
    else if (!uses_hash && dims == 3 && Lv.res >= 2 && (uint64_t)Lv.res * Lv.res * Lv.res <= Lv.size) Lv.mode = LV_DENSE;
    else if (!uses_hash && pow2_size && dims >= 1) Lv.mode = LV_ADD_POW2;  // (x + y * mult[1] + z * mult[2]) & (size - 1), see nrf_device.h
    else Lv.mode = LV_GENERIC;
    Lv.my_b = mult[1] << 2;  // (the hashed levels' constants replace these below)
    Lv.mz_b = mult[2] << 2;
    p.generic_grid = p.generic_grid || Lv.mode == LV_GENERIC;
  }
  // The instance: base.json's shape (F = 2 x 16 levels, Linear; 64 neurons, 1 + 2 hidden layers; a 16-wide direction encoding;
  // ReLU hidden, density output None, rgb output None or Sigmoid, sigma Exponential) is NET_HOT.  Each register-resident
  // instance relaxes one axis of it; everything else is the generic instance.
  GenModel& G = p.gen;
  G.F = F; G.interp = d.interpolation; G.n_levels = L; G.feat_raw = L * F; G.feat_w = next_multiple(G.feat_raw, 16u);
  G.feat_k = next_multiple(G.feat_w, 32u); G.width = Wn; G.dir_raw = dir_raw_width(d); G.dir_w = next_multiple(G.dir_raw, 16u);
  G.rgb_in = 16u + G.dir_w;
  G.n_dens = d.density_hidden_layers + 1; G.n_rgb = d.rgb_hidden_layers + 1;
  G.act_stride = std::max(G.feat_k, next_multiple(Wn, 32u)) + 8;  // +16 bytes: consecutive rows start 4 banks apart (ds_read_b128 of 16 rows: conflict-free)
  G.dir_stride = G.dir_w + 8;
  const uint32_t dir_w = G.dir_w;
  const bool grid_base = !p.generic_grid && F == 2 && L == 16 && d.interpolation == NRF_INTERP_LINEAR;
  const bool mlp_base = Wn == 64 && d.density_hidden_layers == 1 && d.rgb_hidden_layers == 2;
  const bool dir16 = dir_w == 16;
  const bool relu = d.density_activation == NRF_ACT_RELU && d.rgb_activation == NRF_ACT_RELU;
  auto native = [](uint32_t a) {  // (nrf_device.h activate_native; Sine keeps the generic instance)
    return a == NRF_ACT_RELU || a == NRF_ACT_NONE || a == NRF_ACT_EXPONENTIAL || a == NRF_ACT_SIGMOID || a == NRF_ACT_SQUAREPLUS || a == NRF_ACT_SOFTPLUS;
  };
  const bool acts_native = native(d.density_activation) && native(d.rgb_activation);
  const bool outputs_base = d.density_output_activation == NRF_ACT_NONE && d.sigma_activation == NRF_ACT_EXPONENTIAL &&
                            (d.rgb_output_activation == NRF_ACT_NONE || d.rgb_output_activation == NRF_ACT_SIGMOID);
  // a Frequency encoding of 32..80 values: NET_WIDE (the first rgb layer in RK_WIDE K steps); SH of degree 5..8: NET_WIDE_SH
  const bool freq_wide = dir_w > 16 && dir_w <= 16u * (2u * RK_WIDE - 1u) && d.dir_encoding == NRF_DIR_FREQUENCY;
  const bool sh_wide = dir_w > 16 && dir_w <= 64 && d.dir_encoding == NRF_DIR_SH;
  const uint32_t extra_layers = (d.density_hidden_layers - 1) + (d.rgb_hidden_layers - 1);
  int own = NET_GENERIC;
  if (!outputs_base) own = NET_GENERIC;
  else if (grid_base && mlp_base && relu && dir16) own = NET_HOT;
  else if (grid_base && mlp_base && relu && freq_wide) own = NET_WIDE;
  else if (!allow_own) own = NET_GENERIC;  // (NRF_WIDTH_INSTANCES=0: A/B runs)
  else if (grid_base && mlp_base && relu && sh_wide) own = NET_WIDE_SH;
  else if (grid_base && dir16 && relu && Wn != 64 && d.density_hidden_layers == 1 && d.rgb_hidden_layers == 2)
    own = Wn == 16 ? NET_W16 : (Wn == 32 ? NET_W32 : NET_W128);  // tcnn's other FullyFusedMLP widths
  else if (grid_base && dir16 && Wn == 64 && acts_native && extra_layers <= (uint32_t)DEPTH_MAX_WW)
    own = relu ? NET_DEPTH : NET_ACT;  // other numbers of hidden layers (runtime), hidden activations other than ReLU
  else if (!p.generic_grid && !grid_base && L * F <= 32 && mlp_base && dir16 && relu)
    own = F == 1 ? NET_GRID1 : (F == 2 ? NET_GRID2 : (F == 4 ? NET_GRID4 : NET_GRID8));  // another grid in front of base.json's MLPs
  p.own = own;
  p.stage = own == NET_HOT || own == NET_WIDE ? own : NET_GENERIC;
  p.gen_wave_bytes = p.stage != NET_HOT ? gen_dir_bytes(G) + gen_act_bytes(G) : 0u;
  p.gen_frag_bytes = p.stage == NET_GENERIC ? generic_frag_bytes(d, G) : 0u;
  if (p.stage == NET_GENERIC && render_strip_lds_fixed_bytes(NET_GENERIC, p.gen_wave_bytes) > (int)CU_LDS_BYTES) {
    p.rc = refuse(p.why, NRF_E_UNSUPPORTED, "HIP path: this network shape needs more LDS than a CU has");
    return p;
  }
  // Device copy of the table: the reference's entries level by level; a dense level is followed by
  // res^2 + res + 1 copies of its first entries so that x + y*res + z*res^2 (at most
  // size + res^2 + res when a +1 corner sits on the x = 1 / y = 1 / z = 1 face) needs no modulo.
  uint64_t entries = 0;
  for (uint32_t l = 0; l < L; ++l) {
    LevelParams& Lv = p.lp[l];
    if (Lv.mode == LV_HASH_POW2 || Lv.mode == LV_ADD_POW2)  // aligned to its own (power-of-two) size: `index & mask | offset` (level_gather)
      entries = (entries + Lv.size - 1) / Lv.size * Lv.size;
    Lv.offset = (uint32_t)entries;
    entries += Lv.size;
    if (Lv.mode == LV_DENSE) entries += (uint64_t)Lv.res * Lv.res + Lv.res + 1;
  }
  p.table_ref_bytes = entries * F * 2;
  if (p.table_ref_bytes >= (1ull << 32)) {  // level_gather addresses the table by 32-bit byte offsets
    p.rc = refuse(p.why, NRF_E_UNSUPPORTED, "hash tables of 4 GiB or more are not supported");
    return p;
  }
  // Cell-major quad copies (round 6; nrf_device.h level_gather_quad) behind the reference-order table, for the instances whose
  // network phase is network_from_lds with an F = 2 x 16 grid (the hot instance, its wide / width / depth forms): per cell
  // (x, y, z), x, y < res, z <= res, the four entries of the corners (x | x + 1, y | y + 1, z) as grid_index (grid.h:100-117)
  // names them.  The reference-order table stays: every other kernel (stage entry points, generic instance) reads it.
  // A step of the fused kernel (levels 4 jl .. 4 jl + 3, one per lane group) takes quads as a whole or not at all (steps that
  // mix the two forms run both instruction streams: measured no faster, profiles/r06/quad_sweep.txt); steps are granted in order
  // while their copies fit the budget (nrf_model_desc.gather_copy_budget_mb).  Copies that end beyond the 4 GiB a buffer
  // resource's byte offset reaches are FAR: addressed in 16-byte units from the table base (level_gather_quad_far).
  p.table_bytes = p.table_ref_bytes;
  if (own != NET_GENERIC && net_grid_f(own) == 0) {
    uint64_t budget = budget_mb << 20;
    uint64_t end_bytes = (p.table_ref_bytes + 15) & ~15ull;
    for (int jl = 0; jl < max_quad_steps; ++jl) {
      uint64_t step_bytes = 0;
      bool ok = true;
      for (int g = 0; g < 4; ++g) {
        const LevelParams& Lv = p.lp[4 * jl + g];
        ok = ok && (Lv.mode == LV_DENSE || Lv.mode == LV_HASH_POW2) && Lv.res >= 2 && Lv.res < 1024u;  // (res^2 << 4 < 2^24)
        step_bytes += (uint64_t)Lv.res * Lv.res * ((uint64_t)Lv.res + 1) * 16;
      }
      if (!ok || step_bytes > budget || end_bytes + step_bytes >= (1ull << 36)) continue;
      const bool far = end_bytes + step_bytes >= (1ull << 32);
      if (far && own == NET_WIDE) continue;  // (NET_WIDE is compiled without the far form: nrf_render.h network_from_lds)
      budget -= step_bytes;
      p.quad_mask |= 15u << (4 * jl);
      if (far) p.quad_far |= 1u << jl;
      for (int g = 0; g < 4; ++g) {
        LevelParams& Lv = p.lp[4 * jl + g];
        const uint32_t res = Lv.res;
        Lv.q_off_b = far ? (uint32_t)(end_bytes >> 4) : (uint32_t)end_bytes;
        Lv.q_my_b = far ? res : res << 4;
        Lv.q_mz_b = far ? res * res : (res * res) << 4;
        Lv.q_max = res - 1;
        end_bytes += (uint64_t)res * res * (res + 1) * 16;
      }
    }
    p.table_bytes = end_bytes;
  }
  // byte-offset constants of level_gather / level_gather_wide / level_gather_f1: an entry is 2 F bytes (the generic instance's
  // literal index arithmetic, gen_level, does not read them)
  const uint32_t sh_b = F == 8 ? 4u : (F == 4 ? 3u : (F == 1 ? 1u : 2u));
  for (LevelParams& Lv : p.lp) {
    const bool hashed_pow2 = Lv.mode == LV_HASH_POW2;
    Lv.off_b = Lv.offset << sh_b;
    if (hashed_pow2) {
      Lv.my_b = 2654435761u << sh_b;
      Lv.mz_b = 805459861u << sh_b;
    } else {  // the additive multipliers of the stride loop above (dense: res, res^2; LV_ADD_POW2: possibly wrapped / 0)
      Lv.my_b = (Lv.my_b >> 2) << sh_b;
      Lv.mz_b = (Lv.mz_b >> 2) << sh_b;
    }
    Lv.mask_b = (hashed_pow2 || Lv.mode == LV_ADD_POW2) ? ((Lv.size - 1) << sh_b) : 0xffffffffu;
  }
  p.uni_modes = uni_modes_of(p.lp, L);
  p.gather_plan = static_gather ? gather_plan_of(own, L, p.uni_modes, p.quad_mask, p.quad_far) : GATHER_RUNTIME;
  return p;
}

// The plan as it stands when the device had no room for the quad copies: the reference-order table alone, and the gather plan
// decided again (without the copies the plan's instance would read quads that do not exist)
inline ModelPlan drop_quads(ModelPlan p) {
  for (LevelParams& Lv : p.lp) Lv.q_off_b = Lv.q_my_b = Lv.q_mz_b = Lv.q_max = 0;
  p.quad_mask = p.quad_far = 0;
  p.table_bytes = p.table_ref_bytes;
  p.gather_plan = p.static_gather ? gather_plan_of(p.own, p.lv.n_levels, p.uni_modes, 0u, 0u) : GATHER_RUNTIME;
  return p;
}

// Everything nrf_load_model uploads beside the plan's level table (ModelPlan::lp: drop_quads may still change it), as host vectors
struct ModelImage {
  std::vector<_Float16> frags;      // DevModel::wfrag: the stage instance's fragments (hot / wide: the wide layout; generic: its layers')
  std::vector<_Float16> frags_gen;  // wide models: generic-layout fragments for the stage entry points
  std::vector<_Float16> frags_hot;  // DevModel::wfrag_hot: a register-resident own instance other than the stage one
  GenModel gen;                     // the generic description with fast_grid and layer[] (zero when stage == NET_HOT)
  std::vector<_Float16> grid16;     // the table at the plan's level offsets (padding zero), the dense levels' tails behind them
};

inline ModelImage build_model_image(const nrf_model_desc& d, const ModelPlan& p, bool allow_gen_fast_grid) {
  ModelImage im;
  // fp32 -> fp16 cast of every parameter (nerf_network.h:434-436), order: density MLP | rgb MLP | grid;
  // each MLP: first [W x in] | hidden [W x W] ... | last [16 x W] (fully_fused_mlp.cu:636-687)
  const uint32_t F = d.n_features_per_level, L = d.n_levels;
  const int feat_w = (int)p.gen.feat_w, rgb_in = (int)p.gen.rgb_in;
  const std::vector<LayerDim> layers = gen_layers(d, p.gen);
  size_t n_mlp = 0;
  for (const LayerDim& ly : layers) n_mlp += (size_t)ly.N * ly.K;
  std::vector<_Float16> w16(n_mlp);
  for (size_t i = 0; i < n_mlp; ++i) w16[i] = (_Float16)d.params[i];
  const float* gp = d.params + n_mlp;
  auto pack = [&](bool wide_tail) { return pack_fragments(w16.data(), net_width(p.own), feat_w, (int)F, rgb_in, wide_tail); };
  if (p.stage != NET_GENERIC) im.frags = pack(true);
  switch (p.own) {  // the fragments of a register-resident instance other than the stage one
    case NET_W16: case NET_W32: case NET_W128: case NET_GRID1: case NET_GRID2: case NET_GRID4: case NET_GRID8: im.frags_hot = pack(false); break;
    case NET_DEPTH: case NET_ACT: im.frags_hot = pack_fragments_depth(w16.data(), (int)d.density_hidden_layers, (int)d.rgb_hidden_layers); break;
    case NET_WIDE_SH: im.frags_hot = pack(true); break;  // the wide layout: first rgb layer in RK_WIDE K steps
    default: break;
  }
  // the generic description + fragments: the generic instance's model, and -- for a wide model -- what the stage
  // entry points nrf_encode_dir / nrf_mlp_forward run on (rows of the padded widths)
  GenModel& G = im.gen;
  std::memset(&G, 0, sizeof(G));
  if (p.stage != NET_HOT) {
    std::vector<_Float16>& fr = p.stage == NET_GENERIC ? im.frags : im.frags_gen;
    G = p.gen;
    // 1: F = 2 (level_gather); 4 / 8: that F (level_gather_wide); 0: gen_level's literal index arithmetic (F = 1, Nearest, odd sizes)
    G.fast_grid = (!p.generic_grid && (F == 2 || F == 4 || F == 8) && (d.interpolation == NRF_INTERP_LINEAR || d.interpolation == NRF_INTERP_SMOOTHSTEP) &&
                   allow_gen_fast_grid) ? (F == 2 ? 1u : F) : 0u;
    const _Float16* wp = w16.data();
    for (size_t i = 0; i < layers.size(); ++i) {
      G.layer[i].frag_off = (uint32_t)(fr.size() / (64 * 8));
      G.layer[i].k_steps = (layers[i].K + 31) / 32;
      G.layer[i].n_tiles = layers[i].N / 16;
      G.layer[i].act = layers[i].act;
      pack_generic_layer(wp, layers[i].N, layers[i].K, fr);
      wp += (size_t)layers[i].N * layers[i].K;
    }
  }
  // the table at the plan's level offsets (padding zero)
  im.grid16.assign(p.table_ref_bytes / 2, (_Float16)0.0f);
  for (uint32_t l = 0; l < L; ++l) {
    const LevelParams& Lv = p.lp[l];
    const float* src = gp + (size_t)p.lv.offset[l] * F;
    _Float16* dst = im.grid16.data() + (size_t)Lv.offset * F;
    const size_t n = (size_t)Lv.size * F + (Lv.mode == LV_DENSE ? ((size_t)Lv.res * Lv.res + Lv.res + 1) * F : 0);
    for (size_t i = 0; i < n; ++i) dst[i] = (_Float16)src[i % ((size_t)Lv.size * F)];
  }
  return im;
}

// Every field of DevModel that needs no device pointer (the pointers are nrf_load_model's; the grid side: apply_grid_plan)
inline void fill_dev_model(DevModel& M, const nrf_model_desc& d, const ModelPlan& p) {
  std::memset(&M, 0, sizeof(M));
  M.grid_bytes = (uint32_t)std::min<uint64_t>(p.table_bytes, 0xffffffffull);  // (far quad copies lie beyond: no resource reads them)
  for (int i = 0; i < 6; ++i) M.aabb[i] = d.aabb[i];
  M.bound = d.bound;
  M.rbound = 1.0f / d.bound;
  M.pos_w = (float)(1.0 / (2 * (double)d.bound));
  {
    int e;
    M.pos_w_pow2 = std::frexp(M.pos_w, &e) == 0.5f ? 1u : 0u;
  }
  M.cascade = d.cascade;
  M.H = d.density_grid_size;
  M.n_levels = d.n_levels;
  M.dir_encoding = d.dir_encoding;
  M.sh_degree = d.sh_degree;
  M.n_frequencies = d.n_frequencies;
  M.density_activation = d.density_activation;
  M.density_output_activation = d.density_output_activation;
  M.sigma_activation = d.sigma_activation;
  M.rgb_activation = d.rgb_activation;
  M.rgb_output_activation = d.rgb_output_activation;
  M.uni_modes = p.uni_modes;
  M.quad_mask = p.quad_mask;
  M.quad_far = p.quad_far;
  M.gather_plan = p.gather_plan;
  M.stage = (uint32_t)p.stage;
  M.net = (uint32_t)p.own;  // (plan_grid falls back to the stage instance when the own one does not fit)
  M.gen_wave_bytes = p.gen_wave_bytes;
  M.gen_frag_bytes = p.gen_frag_bytes;
  M.depth_xd = (p.own == NET_DEPTH || p.own == NET_ACT) ? d.density_hidden_layers - 1 : 0u;
  M.depth_xr = (p.own == NET_DEPTH || p.own == NET_ACT) ? d.rgb_hidden_layers - 1 : 0u;
  M.grid_smooth = d.interpolation == NRF_INTERP_SMOOTHSTEP ? 1u : 0u;
  M.grid_nearest = d.interpolation == NRF_INTERP_NEAREST ? 1u : 0u;
  M.dir_w = p.gen.dir_w;
}

}  // namespace nrf
