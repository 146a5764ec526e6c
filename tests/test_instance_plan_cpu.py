"""The host's model plan without a GPU (nrf_debug_plan, an undeclared diagnostic of libnerfhip.so): which kernel instance a
model descriptor gets (own: the one that renders its frames when its march tables fit beside the persistent workgroup;
stage: the one its stage entry points run, and the one frames fall back to), which levels get cell-major quad copies (and
which of those lie beyond 4 GiB), and the waves and LDS bytes (march tables not counted) of the persistent workgroup of
`own`.  The expectations are today's values: a change of any of them is a change of behaviour."""
import ctypes as C

import pytest

import models
import nerfhip as nh

# instance ids (csrc/nrf_launch.h)
HOT, GENERIC, WIDE, W16, W32, W128, WIDE_SH, DEPTH, GRID2, GRID4, GRID8, GRID1, ACT = range(13)
QUAD_BUDGET_MB_DEFAULT = 8192  # (csrc/nrf_api.hip)


def _plan(desc, allow_own=1, budget_mb=QUAD_BUDGET_MB_DEFAULT):
    lib = nh.load_library()
    lib.nrf_debug_plan.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.nrf_debug_plan.restype = C.c_int
    out = (C.c_uint32 * 6)()
    rc = lib.nrf_debug_plan(C.byref(desc), allow_own, budget_mb, out)
    return rc, tuple(out)


# the model shapes of tests/test_generic_gpu.py (SHAPES, GRID_SHAPES, the width / depth / SH shapes), log2 T = 12, H = 32
SHAPES = {
    "freq12": dict(dir_otype="Frequency", n_frequencies=12), "freq10": dict(dir_otype="Frequency", n_frequencies=10),
    "freq4": dict(dir_otype="Frequency", n_frequencies=4), "sh5": dict(sh_degree=5), "sh6": dict(sh_degree=6), "sh7": dict(sh_degree=7),
    "sh8": dict(sh_degree=8), "w32_h2_h3": dict(n_neurons=32, density_hidden_layers=2, rgb_hidden_layers=3),
    "w128_h1_h1": dict(n_neurons=128, density_hidden_layers=1, rgb_hidden_layers=1),
    "w16_h3_h4": dict(n_neurons=16, density_hidden_layers=3, rgb_hidden_layers=4), "w64_h2_h2": dict(density_hidden_layers=2),
    "F1_L16": dict(n_features_per_level=1), "F4_L8": dict(n_features_per_level=4, n_levels=8),
    "F8_L16_w128": dict(n_features_per_level=8, n_neurons=128), "F2_L5": dict(n_levels=5),
    "F2_L11_sh8_w32": dict(n_levels=11, sh_degree=8, n_neurons=32), "nearest": dict(interpolation="Nearest"),
    "smoothstep_F4": dict(interpolation="Smoothstep", n_features_per_level=4, n_levels=6),
    "sigmoid_softplus": dict(activation="Softplus", rgb_output_activation="Sigmoid", sigma_activation="ReLU", density_n_output=1),
    "act_squareplus": dict(activation="Squareplus"), "act_softplus_h2_h1": dict(activation="Softplus", density_hidden_layers=2, rgb_hidden_layers=1),
    "act_sigmoid": dict(activation="Sigmoid", rgb_output_activation="Sigmoid"), "act_none_h1_h3": dict(activation="None", rgb_hidden_layers=3),
    "act_sine": dict(activation="Sine"),
    "g4_8": dict(n_features_per_level=4, n_levels=8), "g8_4": dict(n_features_per_level=8, n_levels=4),
    "g4_6s": dict(n_features_per_level=4, n_levels=6, interpolation="Smoothstep"), "g8_2": dict(n_features_per_level=8, n_levels=2),
    "g4_3s": dict(n_features_per_level=4, n_levels=3, interpolation="Smoothstep"), "g2_5": dict(n_levels=5), "g2_11": dict(n_levels=11),
    "g2_16s": dict(interpolation="Smoothstep"), "g2_8": dict(n_levels=8), "g4_8_sig": dict(n_features_per_level=4, n_levels=8, rgb_output_activation="Sigmoid"),
    "g2_16n": dict(interpolation="Nearest"), "g4_8n": dict(n_features_per_level=4, n_levels=8, interpolation="Nearest"),
    "g8_3n": dict(n_features_per_level=8, n_levels=3, interpolation="Nearest"), "g2_7n": dict(n_levels=7, interpolation="Nearest"),
    "g1_16": dict(n_features_per_level=1), "g1_9s": dict(n_features_per_level=1, n_levels=9, interpolation="Smoothstep"),
    "g1_13n": dict(n_features_per_level=1, n_levels=13, interpolation="Nearest"), "g1_3": dict(n_features_per_level=1, n_levels=3),
    "w16": dict(n_neurons=16), "w32": dict(n_neurons=32), "w128": dict(n_neurons=128),
    "d2_2": dict(density_hidden_layers=2, rgb_hidden_layers=2), "d1_1": dict(density_hidden_layers=1, rgb_hidden_layers=1),
    "d3_4": dict(density_hidden_layers=3, rgb_hidden_layers=4), "d1_3": dict(density_hidden_layers=1, rgb_hidden_layers=3),
    "d2_1": dict(density_hidden_layers=2, rgb_hidden_layers=1),
    "base": dict(),
}
# what the generic instance's first workgroup (12 waves) needs beside its march tables: the fallback of every own instance
GEN_12 = (GENERIC, GENERIC, 0, 0, 12, 173672)
# shape -> (own, stage, quad_mask, quad_far, persist_waves, LDS bytes) with allow_own = 1, then with allow_own = 0
# (quads: the default budget; levels 8..11 of these tables end beyond 4 GiB)
QUADS, FAR = 0xFFF, 0b100
PLANS = {
    "freq12": ((WIDE, WIDE, 0xFF, 0, 12, 82536),) * 2,  # NET_WIDE has no far form: step 2 is refused
    "freq10": ((WIDE, WIDE, 0xFF, 0, 12, 82536),) * 2,
    "freq4": ((WIDE, WIDE, 0xFF, 0, 12, 82536),) * 2,
    "sh5": ((WIDE_SH, GENERIC, QUADS, FAR, 8, 132712), (GENERIC, GENERIC, 0, 0, 12, 185960)),
    "sh6": ((WIDE_SH, GENERIC, QUADS, FAR, 8, 132712), (GENERIC, GENERIC, 0, 0, 12, 198248)),
    "sh7": ((WIDE_SH, GENERIC, QUADS, FAR, 8, 132712), (GENERIC, GENERIC, 0, 0, 12, 210536)),
    "sh8": ((WIDE_SH, GENERIC, QUADS, FAR, 8, 132712), (GENERIC, GENERIC, 0, 0, 12, 210536)),
    "w32_h2_h3": ((GENERIC, GENERIC, 0, 0, 12, 124520),) * 2,
    "w128_h1_h1": ((GENERIC, GENERIC, 0, 0, 12, 271976),) * 2,
    "w16_h3_h4": ((GENERIC, GENERIC, 0, 0, 12, 124520),) * 2,
    "w64_h2_h2": ((DEPTH, GENERIC, QUADS, FAR, 16, 112232), GEN_12),
    "F1_L16": ((GRID1, GENERIC, 0, 0, 16, 79464), GEN_12),
    "F4_L8": ((GRID4, GENERIC, 0, 0, 16, 79464), GEN_12),
    "F8_L16_w128": ((GENERIC, GENERIC, 0, 0, 12, 271976),) * 2,
    "F2_L5": ((GRID2, GENERIC, 0, 0, 16, 79464), GEN_12),
    "F2_L11_sh8_w32": ((GENERIC, GENERIC, 0, 0, 12, 161384),) * 2,
    "nearest": ((GRID2, GENERIC, 0, 0, 16, 79464), GEN_12),
    "smoothstep_F4": ((GRID4, GENERIC, 0, 0, 16, 79464), GEN_12),
    "sigmoid_softplus": (GEN_12,) * 2,
    "act_squareplus": ((ACT, GENERIC, QUADS, FAR, 12, 97896), GEN_12),
    "act_softplus_h2_h1": ((ACT, GENERIC, QUADS, FAR, 12, 97896), GEN_12),
    "act_sigmoid": ((ACT, GENERIC, QUADS, FAR, 12, 97896), GEN_12),
    "act_none_h1_h3": ((ACT, GENERIC, QUADS, FAR, 12, 97896), GEN_12),
    "act_sine": (GEN_12,) * 2,  # (Sine keeps the generic instance)
    "g4_8": ((GRID4, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g8_4": ((GRID8, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g4_6s": ((GRID4, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g8_2": ((GRID8, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g4_3s": ((GRID4, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g2_5": ((GRID2, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g2_11": ((GRID2, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g2_16s": ((GRID2, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g2_8": ((GRID2, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g4_8_sig": ((GRID4, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g2_16n": ((GRID2, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g4_8n": ((GRID4, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g8_3n": ((GRID8, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g2_7n": ((GRID2, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g1_16": ((GRID1, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g1_9s": ((GRID1, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g1_13n": ((GRID1, GENERIC, 0, 0, 16, 79464), GEN_12),
    "g1_3": ((GRID1, GENERIC, 0, 0, 16, 79464), GEN_12),
    "w16": ((W16, GENERIC, QUADS, FAR, 16, 64104), (GENERIC, GENERIC, 0, 0, 12, 124520)),
    "w32": ((W32, GENERIC, QUADS, FAR, 16, 67176), (GENERIC, GENERIC, 0, 0, 12, 124520)),
    "w128": ((W128, GENERIC, QUADS, FAR, 12, 101992), (GENERIC, GENERIC, 0, 0, 12, 271976)),
    "d2_2": ((DEPTH, GENERIC, QUADS, FAR, 16, 112232), GEN_12),
    "d1_1": ((DEPTH, GENERIC, QUADS, FAR, 16, 112232), GEN_12),
    "d3_4": ((DEPTH, GENERIC, QUADS, FAR, 16, 112232), GEN_12),
    "d1_3": ((DEPTH, GENERIC, QUADS, FAR, 16, 112232), GEN_12),
    "d2_1": ((DEPTH, GENERIC, QUADS, FAR, 16, 112232), GEN_12),
    "base": ((HOT, HOT, QUADS, FAR, 16, 79464),) * 2,
}
# the register-resident instances the GPU tests run in the persistent kernel: their workgroup plus the march tables of an
# H = 32 grid (one cascade: coarse words, the cell-boundary table and the dilated words) fit a CU's 160 KiB
REGISTER_RESIDENT = {HOT, WIDE, W16, W32, W128, WIDE_SH, DEPTH, GRID2, GRID4, GRID8, GRID1, ACT}
TABLES_H32 = 4 * ((32 // 4) ** 3 // 32 + 33 + (32 // 4) ** 3 // 32)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_instance_of_each_shape(name):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **SHAPES[name])
    for allow_own, want in zip((1, 0), PLANS[name]):
        rc, got = _plan(desc, allow_own)
        assert rc == nh.NRF_OK and got == want, (name, allow_own, got)
        if allow_own == 0:
            assert got[0] == got[1]  # without its own instance a model renders in its stage instance
        if got[0] in REGISTER_RESIDENT:
            assert got[5] + TABLES_H32 <= 160 * 1024


@pytest.mark.parametrize("budget_mb, mask, far", [(0, 0, 0), (1, 0, 0), (100, 0xFF, 0), (QUAD_BUDGET_MB_DEFAULT, 0xFFF, 0b100)])
def test_base_json_quads_at_explicit_budgets(budget_mb, mask, far):
    """base.json (2^19 entries): levels 0..7 take 95 MB, levels 8..11 4.5 GB (the third step ends beyond 4 GiB: far copies),
    levels 12..15 are never copied.  At the default budget a sample gathers 12 x 2 + 4 x 8 = 56 addresses (the GPU tests'
    gather_addresses_per_sample)."""
    desc, keep, _ = models.build_model()
    for allow_own in (1, 0):
        rc, got = _plan(desc, allow_own, budget_mb)
        assert rc == nh.NRF_OK and got == (HOT, HOT, mask, far, 16, 79464)
    addresses = sum(2 if (mask >> level) & 1 else 8 for level in range(16))
    assert (budget_mb != QUAD_BUDGET_MB_DEFAULT) or addresses == 56


def test_wide_gets_no_far_copies_and_grid_or_generic_models_get_none():
    desc, keep, _ = models.build_model(dir_otype="Frequency", n_frequencies=12)
    assert _plan(desc, 1, 1 << 20) == (nh.NRF_OK, (WIDE, WIDE, 0xFF, 0, 12, 82536))
    for kw, own in ((dict(n_levels=8), GRID2), (dict(n_features_per_level=4, n_levels=8), GRID4), (dict(activation="Sine"), GENERIC),
                    (dict(n_neurons=32, density_hidden_layers=2), GENERIC)):
        desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **kw)
        for allow_own in (1, 0):
            rc, got = _plan(desc, allow_own, 1 << 20)
            assert rc == nh.NRF_OK and got[2:4] == (0, 0) and got[0] == (own if allow_own else GENERIC), (kw, got)


def test_tables_of_other_geometries():
    """Frequency-12 at base.json's table, the 2^22 table (LV_ADD_POW2 levels at its finest resolutions), instant-ngp's
    geometry at aabb_scale 32 (LV_ADD_POW2 levels, logistic colours): all keep their register-resident instance."""
    pls = nh.default_per_level_scale(32.0, 16, 16)
    cases = (
        (dict(dir_otype="Frequency", n_frequencies=12), ((WIDE, WIDE, 0xFF, 0, 12, 82536),) * 2),
        (dict(log2_hashmap_size=22, H=32), ((HOT, HOT, 0xFFF, 0b100, 16, 79464),) * 2),
        (dict(log2_hashmap_size=19, H=32, bound=16.0, cascade=5, per_level_scale=pls, rgb_output_activation="Sigmoid"),
         ((HOT, HOT, 0xF, 0, 16, 79464),) * 2),
        (dict(log2_hashmap_size=12, H=32, grid_type="Tiled"), ((HOT, HOT, 0, 0, 16, 79464),) * 2),
    )
    for kw, want in cases:
        desc, keep, _ = models.build_model(**kw)
        for allow_own, w in zip((1, 0), want):
            rc, got = _plan(desc, allow_own)
            assert rc == nh.NRF_OK and got == w, (kw, allow_own, got)
    # instant-ngp's levels 4..7 take 9.2 GB: granted by a budget of 18 GB (a sixteenth of an MI355X), as far copies
    desc, keep, _ = models.build_model(**cases[2][0])
    assert _plan(desc, 1, 18432) == (nh.NRF_OK, (HOT, HOT, 0xFF, 0b10, 16, 79464))


def test_wide_with_the_generic_march_runs_8_waves():
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=33, dir_otype="Frequency", n_frequencies=12)
    assert _plan(desc) == (nh.NRF_OK, (WIDE, WIDE, 0xFF, 0, 8, 65128))


@pytest.mark.parametrize("field, value, code", [("n_neurons", 48, nh.NRF_E_INVALID), ("n_features_per_level", 3, nh.NRF_E_INVALID),
                                                ("sh_degree", 9, nh.NRF_E_INVALID), ("density_n_output", 32, nh.NRF_E_UNSUPPORTED),
                                                ("n_params", 7, nh.NRF_E_PARAMS)])
def test_invalid_descriptors_keep_their_codes(field, value, code):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    setattr(desc, field, value)
    rc, _ = _plan(desc)
    assert rc == code
