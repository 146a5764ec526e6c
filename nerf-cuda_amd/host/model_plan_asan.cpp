// Sanitizer driver of csrc/nrf_model_plan.h (make model_asan: AddressSanitizer + UBSan on hipcc's host pass, no libnerfhip.so, no
// device): plan_model, drop_quads, build_model_image and fill_dev_model over every shape of tests/test_instance_plan_cpu.py (as
// descriptor fields), log2 T = 4 and 12, quad budgets of 0, 1, 64 MiB and the default, with and without drop_quads; the parameters
// are a seeded LCG.  The sanitizers watch the packers' index arithmetic and the table copy (level offsets, the dense levels'
// wrap-around tails); the driver itself checks what needs no second implementation.
#include <cstdio>
#include <vector>

#include "../csrc/nrf_model_plan.h"

namespace nrf {
// (nrf_kernels.hip's, which this program does not link: any figure below a CU's LDS lets every shape through)
int render_strip_lds_fixed_bytes(int, uint32_t) { return 64 * 1024; }
}  // namespace nrf

using namespace nrf;

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED %s (line %d): %s\n", what, __LINE__, #cond); ++g_fail; } \
  } while (0)

struct Shape {
  const char* name;
  void (*set)(nrf_model_desc&);
};
#define SHAPE(name, body) {name, [](nrf_model_desc& d) { (void)d; body; }}
#define ACT(a) d.density_activation = d.rgb_activation = NRF_ACT_##a
static const Shape SHAPES[] = {
    SHAPE("base", ),
    SHAPE("freq12", d.dir_encoding = NRF_DIR_FREQUENCY; d.n_frequencies = 12),
    SHAPE("freq10", d.dir_encoding = NRF_DIR_FREQUENCY; d.n_frequencies = 10),
    SHAPE("freq4", d.dir_encoding = NRF_DIR_FREQUENCY; d.n_frequencies = 4),
    SHAPE("sh5", d.sh_degree = 5), SHAPE("sh6", d.sh_degree = 6), SHAPE("sh7", d.sh_degree = 7), SHAPE("sh8", d.sh_degree = 8),
    SHAPE("w32_h2_h3", d.n_neurons = 32; d.density_hidden_layers = 2; d.rgb_hidden_layers = 3),
    SHAPE("w128_h1_h1", d.n_neurons = 128; d.density_hidden_layers = 1; d.rgb_hidden_layers = 1),
    SHAPE("w16_h3_h4", d.n_neurons = 16; d.density_hidden_layers = 3; d.rgb_hidden_layers = 4),
    SHAPE("w64_h2_h2", d.density_hidden_layers = 2),
    SHAPE("F1_L16", d.n_features_per_level = 1),
    SHAPE("F4_L8", d.n_features_per_level = 4; d.n_levels = 8),
    SHAPE("F8_L16_w128", d.n_features_per_level = 8; d.n_neurons = 128),
    SHAPE("F2_L5", d.n_levels = 5),
    SHAPE("F2_L11_sh8_w32", d.n_levels = 11; d.sh_degree = 8; d.n_neurons = 32),
    SHAPE("nearest", d.interpolation = NRF_INTERP_NEAREST),
    SHAPE("smoothstep_F4", d.interpolation = NRF_INTERP_SMOOTHSTEP; d.n_features_per_level = 4; d.n_levels = 6),
    SHAPE("sigmoid_softplus", ACT(SOFTPLUS); d.rgb_output_activation = NRF_ACT_SIGMOID; d.sigma_activation = NRF_ACT_RELU; d.density_n_output = 1),
    SHAPE("act_squareplus", ACT(SQUAREPLUS)),
    SHAPE("act_softplus_h2_h1", ACT(SOFTPLUS); d.density_hidden_layers = 2; d.rgb_hidden_layers = 1),
    SHAPE("act_sigmoid", ACT(SIGMOID); d.rgb_output_activation = NRF_ACT_SIGMOID),
    SHAPE("act_none_h1_h3", ACT(NONE); d.rgb_hidden_layers = 3),
    SHAPE("act_sine", ACT(SINE)),
    SHAPE("g4_8", d.n_features_per_level = 4; d.n_levels = 8), SHAPE("g8_4", d.n_features_per_level = 8; d.n_levels = 4),
    SHAPE("g4_6s", d.n_features_per_level = 4; d.n_levels = 6; d.interpolation = NRF_INTERP_SMOOTHSTEP),
    SHAPE("g8_2", d.n_features_per_level = 8; d.n_levels = 2),
    SHAPE("g4_3s", d.n_features_per_level = 4; d.n_levels = 3; d.interpolation = NRF_INTERP_SMOOTHSTEP),
    SHAPE("g2_5", d.n_levels = 5), SHAPE("g2_11", d.n_levels = 11), SHAPE("g2_16s", d.interpolation = NRF_INTERP_SMOOTHSTEP), SHAPE("g2_8", d.n_levels = 8),
    SHAPE("g4_8_sig", d.n_features_per_level = 4; d.n_levels = 8; d.rgb_output_activation = NRF_ACT_SIGMOID),
    SHAPE("g2_16n", d.interpolation = NRF_INTERP_NEAREST),
    SHAPE("g4_8n", d.n_features_per_level = 4; d.n_levels = 8; d.interpolation = NRF_INTERP_NEAREST),
    SHAPE("g8_3n", d.n_features_per_level = 8; d.n_levels = 3; d.interpolation = NRF_INTERP_NEAREST),
    SHAPE("g2_7n", d.n_levels = 7; d.interpolation = NRF_INTERP_NEAREST),
    SHAPE("g1_16", d.n_features_per_level = 1),
    SHAPE("g1_9s", d.n_features_per_level = 1; d.n_levels = 9; d.interpolation = NRF_INTERP_SMOOTHSTEP),
    SHAPE("g1_13n", d.n_features_per_level = 1; d.n_levels = 13; d.interpolation = NRF_INTERP_NEAREST),
    SHAPE("g1_3", d.n_features_per_level = 1; d.n_levels = 3),
    SHAPE("w16", d.n_neurons = 16), SHAPE("w32", d.n_neurons = 32), SHAPE("w128", d.n_neurons = 128),
    SHAPE("d2_2", d.density_hidden_layers = 2; d.rgb_hidden_layers = 2), SHAPE("d1_1", d.density_hidden_layers = 1; d.rgb_hidden_layers = 1),
    SHAPE("d3_4", d.density_hidden_layers = 3; d.rgb_hidden_layers = 4), SHAPE("d1_3", d.density_hidden_layers = 1; d.rgb_hidden_layers = 3),
    SHAPE("d2_1", d.density_hidden_layers = 2; d.rgb_hidden_layers = 1),
    SHAPE("tiled", d.grid_type = NRF_GRID_TILED),  // (LV_ADD_POW2 levels)
};

int main() {
  const uint64_t QUAD_BUDGET_MB_DEFAULT = 8192;  // (nrf_api.hip)
  int runs = 0;
  char what[128];
  for (const Shape& shape : SHAPES)
    for (uint32_t log2_T : {4u, 12u})
      for (uint64_t budget_mb : {(uint64_t)0, (uint64_t)1, (uint64_t)64, QUAD_BUDGET_MB_DEFAULT})
        for (int drop = 0; drop < 2; ++drop) {
          std::snprintf(what, sizeof(what), "%s log2_T=%u budget=%llu drop=%d", shape.name, log2_T, (unsigned long long)budget_mb, drop);
          nrf_model_desc d{};  // base.json (synthetic.py base_config) with a table of 2^log2_T entries, H = 32
          d.abi_version = NRF_ABI_VERSION;
          d.grid_type = NRF_GRID_HASH; d.n_levels = 16; d.n_features_per_level = 2; d.log2_hashmap_size = log2_T; d.base_resolution = 16;
          d.interpolation = NRF_INTERP_LINEAR;
          d.n_neurons = 64; d.density_hidden_layers = 1; d.rgb_hidden_layers = 2; d.density_n_output = 16;
          d.density_activation = d.rgb_activation = NRF_ACT_RELU;
          d.density_output_activation = d.rgb_output_activation = NRF_ACT_NONE; d.sigma_activation = NRF_ACT_EXPONENTIAL;
          d.dir_encoding = NRF_DIR_SH; d.sh_degree = 4;
          for (int a = 0; a < 3; ++a) { d.aabb[a] = -1.0f; d.aabb[a + 3] = 1.0f; }
          d.bound = 1.0f; d.scale = 0.33f; d.cascade = 1; d.density_grid_size = 32; d.mean_density = 0.02f;
          shape.set(d);
          d.per_level_scale = d.n_levels > 1 ? std::exp(std::log(2048.0f * d.bound / (float)d.base_resolution) / (float)(d.n_levels - 1)) : 2.0f;
          const char* why = "";
          nrf_level_table lt;
          CHECK(compute_level_table(d, lt, why) == NRF_OK);
          uint64_t n_params = 0;
          CHECK(expected_params(d, lt, n_params, why) == NRF_OK);
          std::vector<float> params(n_params);
          uint32_t rng = 12345u + log2_T;
          for (float& v : params) { rng = rng * 1664525u + 1013904223u; v = ((float)(rng >> 8) / 8388608.0f - 1.0f) * 0.5f; }
          d.params = params.data();
          d.n_params = n_params;

          ModelPlan p = plan_model(d, true, budget_mb, 4);
          CHECK(p.rc == NRF_OK && p.why[0] == 0);
          if (p.rc) continue;
          if (drop) p = drop_quads(p);
          const ModelImage im = build_model_image(d, p, true);
          DevModel M;
          fill_dev_model(M, d, p);
          ++runs;
          // the fragment counts
          const size_t FRAG = 64 * 8;
          const int Wd = net_width(p.own), MT = Wd / 16, KS = (Wd + 31) / 32;
          if (p.stage != NET_GENERIC) CHECK(im.frags.size() == (size_t)N_FRAGS_WIDE_ALL * FRAG);
          else CHECK(im.frags.size() * 2 == generic_frag_bytes(d, p.gen) && M.gen_frag_bytes == im.frags.size() * 2);
          CHECK((p.stage == NET_WIDE) ? im.frags_gen.size() * 2 == generic_frag_bytes(d, p.gen) : im.frags_gen.empty());
          CHECK((p.stage == NET_HOT) == (im.gen.width == 0) && (p.stage == NET_GENERIC || M.gen_frag_bytes == 0));
          switch (p.own) {
            case NET_HOT: case NET_WIDE: case NET_GENERIC: CHECK(im.frags_hot.empty() && p.own == p.stage); break;
            case NET_WIDE_SH: CHECK(im.frags_hot.size() == (size_t)N_FRAGS_WIDE_ALL * FRAG); break;
            case NET_DEPTH: case NET_ACT: CHECK(im.frags_hot.size() == (size_t)DEPTH_FRAGS * FRAG); break;
            case NET_W16: case NET_W32: case NET_W128: CHECK(im.frags_hot.size() == (size_t)(2 * MT + 2 * KS + MT * KS) * FRAG); break;
            default: CHECK(net_grid_f(p.own) == (int)d.n_features_per_level && im.frags_hot.size() == (size_t)N_FRAGS * FRAG); break;
          }
          // the table: every level, with a dense level's tail, inside grid16; power-of-two levels aligned to their size
          const uint32_t F = d.n_features_per_level;
          CHECK(im.grid16.size() * 2 == p.table_ref_bytes);
          for (uint32_t l = 0; l < d.n_levels; ++l) {
            const LevelParams& Lv = p.lp[l];
            const uint64_t tail = Lv.mode == LV_DENSE ? (uint64_t)Lv.res * Lv.res + Lv.res + 1 : 0;
            CHECK(((uint64_t)Lv.offset + Lv.size + tail) * F <= im.grid16.size());
            if (Lv.mode == LV_HASH_POW2 || Lv.mode == LV_ADD_POW2) CHECK((Lv.size & (Lv.size - 1)) == 0 && Lv.offset % Lv.size == 0);
          }
          // the quad copies: none after drop_quads, and none that the budget does not cover
          uint64_t quad_bytes = 0;
          for (uint32_t l = 0; l < 16; ++l) {
            const LevelParams& Lv = p.lp[l];
            const bool has = ((p.quad_mask >> l) & 1u) != 0;
            CHECK(has == (Lv.q_off_b != 0) && has == (Lv.q_max != 0) && has == (Lv.q_my_b != 0) && has == (Lv.q_mz_b != 0));
            if (has) quad_bytes += (uint64_t)Lv.res * Lv.res * (Lv.res + 1) * 16;
          }
          CHECK(quad_bytes <= (budget_mb << 20) && p.table_bytes >= p.table_ref_bytes && p.table_bytes - p.table_ref_bytes < quad_bytes + 16);
          if (drop) CHECK(p.quad_mask == 0 && p.quad_far == 0 && p.table_bytes == p.table_ref_bytes && quad_bytes == 0);
          CHECK(M.quad_mask == p.quad_mask && M.gather_plan == p.gather_plan && M.grid_bytes == std::min<uint64_t>(p.table_bytes, 0xffffffffull));
          CHECK(p.gather_plan == gather_plan_of(p.own, d.n_levels, p.uni_modes, p.quad_mask, p.quad_far));
        }
  std::printf("model_plan_asan: %d images, %d failures\n", runs, g_fail);
  return g_fail ? 1 : 0;
}
