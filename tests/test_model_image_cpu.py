"""The model side of the host's plan without a GPU (nrf_debug_model_image, an undeclared diagnostic of libnerfhip.so: plan_model,
build_model_image and fill_dev_model of csrc/nrf_model_plan.h): the bytes nrf_load_model uploads for a descriptor -- weight fragments,
the generic description, the fp16 table at the plan's level offsets, the level table.  Every part of every row is pinned to what the
commit before the header held on an MI355X (tests/golden/model_image_parent.json, tests/model_image_rows.py); the fragment layouts
are stated a second time here, in numpy, from the formulas of the header's comments."""
import ctypes as C
import zlib

import numpy as np
import pytest

import model_image_rows as R
import nerfhip as nh

HOT, GENERIC, WIDE, W16, W32, W128, WIDE_SH, DEPTH, GRID2, GRID4, GRID8, GRID1, ACT = range(13)  # (csrc/nrf_launch.h)
N_FRAGS, FRAG_D0_NATURAL, FRAG_R0X, N_FRAGS_WIDE_ALL, RK_WIDE = 20, 20, 24, 32, 3                # (csrc/nrf_device.h)
DF_D0, DF_D1, DF_R0, DF_R2, DF_WW, DEPTH_FRAGS = 0, 4, 6, 10, 12, 52
LV_DENSE, LV_HASH_POW2, LV_GENERIC, LV_ADD_POW2 = range(4)
LEVEL_WORDS = ("scale", "res", "offset", "size", "mode", "hashed", "off_b", "my_b", "mz_b", "mask_b", "q_off_b", "q_my_b", "q_mz_b", "q_max",
               "pad0", "pad1")
Q_WORDS = [LEVEL_WORDS.index(k) for k in ("q_off_b", "q_my_b", "q_mz_b", "q_max")]


@pytest.fixture(scope="module")
def golden():
    return R.golden()


_cache = {}


def _image(name):
    """(desc, parts) of a row, built once"""
    if name not in _cache:
        row = R.ROWS[name]
        desc, keep, budget = R.build(row)
        _cache[name] = (desc, keep, R.image(desc, budget, row["flags"]))
    return _cache[name][0], _cache[name][2]


def _plan(parts):
    return dict(zip(R.PLAN_WORDS, (int(v) for v in parts["plan"].view(np.uint32))))


def _levels(parts):
    return parts["levels"].view(np.uint32).reshape(16, 16)


@pytest.mark.parametrize("name", sorted(R.ROWS))
def test_row_is_the_parents(name, golden):
    """every part: length and crc32 of the recorded parent"""
    desc, parts = _image(name)
    got, want = R.record(parts), golden[name]
    if R.ROWS[name]["flags"] & R.DROP_QUADS:
        # (recorded at a budget that grants nothing -- model_image_rows.py: the one difference is the table's size, which drop_quads
        # sets to the reference-order table's and a plan without copies rounds up to the next 16 bytes)
        i = R.PLAN_WORDS.index("grid_bytes")
        assert got["plan"][i] == parts["grid16"].size and want["plan"][i] == (parts["grid16"].size + 15) // 16 * 16
        assert got["plan"][:i] + got["plan"][i + 1:] == want["plan"][:i] + want["plan"][i + 1:]
        assert got["len"] == want["len"] and got["crc32"][:-1] == want["crc32"][:-1]
    else:
        assert got == want


# --- the fragment layouts, a second time: fragment f, lane l, element j = W[16 m + (l & 15)][kmap(l >> 4, j)], zero beyond the width


def _kmap_levels(F):
    if F == 1:
        return lambda g, j: np.where(j < 4, 4 * j + g, 1 << 20)
    return {2: lambda g, j: 2 * (4 * (j >> 1) + g) + (j & 1), 4: lambda g, j: 4 * (4 * (j >> 2) + g) + (j & 3), 8: lambda g, j: 8 * g + j}[F]


def _kmap_natural(s):
    return lambda g, j: 32 * s + 8 * g + j


def _kmap_rgb_in(g, j):
    return np.where(j < 4, 4 * g + j, 16 + 4 * g + (j - 4))


def _kmap_hidden(s):
    return lambda g, j: 16 * (2 * s + (j >> 2)) + 4 * g + (j & 3)


def _fragment(Wm, m, kmap):
    l, j = np.arange(64)[:, None], np.arange(8)[None, :]
    k = kmap(l >> 4, j) + 0 * l
    return np.where(k < Wm.shape[1], Wm[16 * m + (l & 15), np.minimum(k, Wm.shape[1] - 1)], np.uint16(0)).astype(np.uint16)


def _matrices(desc, shapes):
    """the fp16 bits of the MLP parameters, cut into the matrices [N][K] of `shapes` in parameter order"""
    n = sum(a * b for a, b in shapes)
    w = np.ctypeslib.as_array(desc.params, (n,)).astype(np.float16).view(np.uint16)
    cuts = np.cumsum([0] + [a * b for a, b in shapes])
    return [w[cuts[i]:cuts[i + 1]].reshape(shapes[i]) for i in range(len(shapes))]


def _layout_1_2(desc, W, feat_w, F, rgb_in, wide_tail):
    """D0 [W][feat_w] | D1 [16][W] | R0 [W][rgb_in] | R1 [W][W] | R2 [16][W] in the MlpShape<W> order, the wide extras behind"""
    D0, D1, R0, R1, R2 = _matrices(desc, [(W, feat_w), (16, W), (W, rgb_in), (W, W), (16, W)])
    MT, KS = W // 16, (W + 31) // 32
    fr = [_fragment(D0, m, _kmap_levels(F)) for m in range(MT)] + [_fragment(D1, 0, _kmap_hidden(s)) for s in range(KS)]
    fr += [_fragment(R0, m, _kmap_rgb_in) for m in range(MT)] + [_fragment(R1, m, _kmap_hidden(s)) for m in range(MT) for s in range(KS)]
    fr += [_fragment(R2, 0, _kmap_hidden(s)) for s in range(KS)]
    assert len(fr) == 2 * MT + 2 * KS + MT * KS
    if wide_tail:
        assert W == 64 and len(fr) == N_FRAGS == FRAG_D0_NATURAL and FRAG_R0X == FRAG_D0_NATURAL + 4
        fr += [_fragment(D0, m, _kmap_natural(0)) for m in range(4)]
        fr += [_fragment(R0, m, _kmap_natural(s)) for s in range(1, RK_WIDE) for m in range(4)]
        assert len(fr) == N_FRAGS_WIDE_ALL
    return np.stack(fr)


def _layout_depth(desc, nd, nr):
    xd, xr = nd - 1, nr - 1
    mats = _matrices(desc, [(64, 32)] + [(64, 64)] * xd + [(16, 64), (64, 32)] + [(64, 64)] * xr + [(16, 64)])
    D0, DW, D1, R0, RW, R2 = mats[0], mats[1:1 + xd], mats[1 + xd], mats[2 + xd], mats[3 + xd:3 + xd + xr], mats[3 + xd + xr]
    fr = np.zeros((DEPTH_FRAGS, 64, 8), np.uint16)
    for m in range(4):
        fr[DF_D0 + m], fr[DF_R0 + m] = _fragment(D0, m, _kmap_levels(2)), _fragment(R0, m, _kmap_rgb_in)
    for s in range(2):
        fr[DF_D1 + s], fr[DF_R2 + s] = _fragment(D1, 0, _kmap_hidden(s)), _fragment(R2, 0, _kmap_hidden(s))
    for e, Wm in enumerate(DW + RW):
        for m in range(4):
            for s in range(2):
                fr[DF_WW + 8 * e + 2 * m + s] = _fragment(Wm, m, _kmap_hidden(s))
    return fr


def _layers(desc, feat_w, rgb_in):
    W = desc.n_neurons
    mlp = lambda k, hidden: [(W, k)] + [(W, W)] * (hidden - 1) + [(16, W)]
    return mlp(feat_w, desc.density_hidden_layers) + mlp(rgb_in, desc.rgb_hidden_layers)


def _layout_generic(desc, feat_w, rgb_in):
    """every layer of the two MLPs: fragment (m, s) in the natural K order"""
    shapes = _layers(desc, feat_w, rgb_in)
    return np.stack([_fragment(Wm, m, _kmap_natural(s)) for Wm in _matrices(desc, shapes) for m in range(Wm.shape[0] // 16)
                     for s in range((Wm.shape[1] + 31) // 32)])


@pytest.mark.parametrize("shape", sorted(R.SHAPES))
def test_fragments_are_the_formulas(shape):
    desc, parts = _image(shape)
    plan = _plan(parts)
    own, stage = plan["own"], plan["stage"]
    feat_w = (desc.n_levels * desc.n_features_per_level + 15) // 16 * 16
    rgb_in, F, W = 16 + plan["dir_w"], desc.n_features_per_level, desc.n_neurons
    frags = lambda k: parts[k].view(np.uint16).reshape(-1, 64, 8)
    if stage != GENERIC:  # the hot and the wide instance, and every stage entry point of theirs: the wide layout
        assert np.array_equal(frags("frags"), _layout_1_2(desc, 64, 32, 2, rgb_in, True))
    else:
        assert np.array_equal(frags("frags"), _layout_generic(desc, feat_w, rgb_in))
    if stage == WIDE:
        assert np.array_equal(frags("frags_gen"), _layout_generic(desc, feat_w, rgb_in))
    if own in (W16, W32, W128):
        assert np.array_equal(frags("frags_hot"), _layout_1_2(desc, W, 32, 2, 32, False))
    elif own in (DEPTH, ACT):
        assert np.array_equal(frags("frags_hot"), _layout_depth(desc, desc.density_hidden_layers, desc.rgb_hidden_layers))
    elif own == WIDE_SH:
        assert np.array_equal(frags("frags_hot"), _layout_1_2(desc, 64, 32, 2, rgb_in, True))
    elif own in (GRID1, GRID2, GRID4, GRID8):
        assert np.array_equal(frags("frags_hot"), _layout_1_2(desc, 64, feat_w, F, 32, False))
    else:
        assert own == stage and parts["frags_hot"].size == 0


def test_three_layouts_are_one_on_base_weights():
    """the width layout at W = 64 == the first N_FRAGS fragments of the hot layout == the grid layout at F = 2 with feat_w = 32"""
    desc, parts = _image("base")
    hot = parts["frags"].view(np.uint16).reshape(-1, 64, 8)
    width = _layout_1_2(desc, 64, 32, 2, 32, False)  # (MlpShape<64>)
    assert hot.shape[0] == N_FRAGS_WIDE_ALL and np.array_equal(hot[:N_FRAGS], width)
    # the library's own grid layout of these weights: an F = 2 x 16 Smoothstep grid renders in GRID2 with feat_w = 32
    sdesc, skeep, _ = R.models.build_model(log2_hashmap_size=12, H=32, interpolation="Smoothstep")
    assert sdesc.n_params == desc.n_params
    C.memmove(sdesc.params, desc.params, 4 * desc.n_params)
    grid = R.image(sdesc, R.QUAD_BUDGET_MB_DEFAULT)
    assert _plan(grid)["own"] == GRID2 and np.array_equal(grid["frags_hot"].view(np.uint16).reshape(-1, 64, 8), hot[:N_FRAGS])


@pytest.mark.parametrize("shape", ["base", "g4_8", "g1_3", "tiled"])
def test_grid16_is_the_cast_table_at_the_plans_offsets(shape):
    """fp16 casts of the reference's entries level by level; a dense level ends with res^2 + res + 1 of its leading entries again;
    a power-of-two level starts at a multiple of its size; everything between is zero"""
    desc, parts = _image(shape)
    F, L = desc.n_features_per_level, desc.n_levels
    lt = nh.level_table(desc)
    n_mlp = sum(a * b for a, b in _layers(desc, (L * F + 15) // 16 * 16, 16 + _plan(parts)["dir_w"]))
    table = np.ctypeslib.as_array(desc.params, (desc.n_params,))[n_mlp:].astype(np.float16).view(np.uint16)
    grid16, lv = parts["grid16"].view(np.uint16), _levels(parts)
    covered = np.zeros(grid16.size, bool)
    modes = set()
    for l in range(L):
        p = dict(zip(LEVEL_WORDS, (int(v) for v in lv[l])))
        size, res, modes = p["size"], p["res"], modes | {p["mode"]}
        assert size == lt.offset[l + 1] - lt.offset[l] and res == lt.resolution[l]
        src = table[lt.offset[l] * F:lt.offset[l + 1] * F]
        tail = (res * res + res + 1) if p["mode"] == LV_DENSE else 0
        assert tail <= size
        assert np.array_equal(grid16[p["offset"] * F:(p["offset"] + size) * F], src)
        assert np.array_equal(grid16[(p["offset"] + size) * F:(p["offset"] + size + tail) * F], src[:tail * F])
        if p["mode"] in (LV_HASH_POW2, LV_ADD_POW2):
            assert size & (size - 1) == 0 and p["offset"] % size == 0
        covered[p["offset"] * F:(p["offset"] + size + tail) * F] = True
    assert (p["offset"] + size + tail) * F == grid16.size and not grid16[~covered].any()
    assert LV_DENSE in modes and (LV_ADD_POW2 in modes) == (shape == "tiled")
    assert not lv[L:].view(np.uint32)[:, [1, 2, 3, 4]].any()  # levels the grid does not have


@pytest.mark.parametrize("shape", ["freq12", "sh8", "w32_h2_h3", "act_sine", "smoothstep_F4", "nearest", "g8_2"])
def test_gen_model_layers_are_running_tile_counts(shape):
    """GenModel: 16 words of geometry, then layer[24] = {frag_off, k_steps, n_tiles, act}; frag_off are the running tile counts, and
    they end at the fragment count of the generic fragments (gen_frag_bytes for a generic stage)"""
    desc, parts = _image(shape)
    plan = _plan(parts)
    gen = parts["gen"].view(np.uint32)
    layers = gen[-24 * 4:].reshape(24, 4)
    shapes = _layers(desc, (desc.n_levels * desc.n_features_per_level + 15) // 16 * 16, 16 + plan["dir_w"])
    tiles = [(n // 16) * ((k + 31) // 32) for n, k in shapes]
    assert [int(v) for v in layers[:len(shapes), 0]] == [sum(tiles[:i]) for i in range(len(shapes))]
    assert [(int(a), int(b)) for a, b in layers[:len(shapes), 1:3]] == [((k + 31) // 32, n // 16) for n, k in shapes]
    assert not layers[len(shapes):].any()
    frags = parts["frags" if plan["stage"] == GENERIC else "frags_gen"]
    assert frags.size == 1024 * sum(tiles) and plan["gen_frag_bytes"] == (frags.size if plan["stage"] == GENERIC else 0)


@pytest.mark.parametrize("shape", R.BUDGET_SHAPES)
def test_drop_quads_leaves_the_plan_of_a_budget_that_grants_nothing(shape):
    desc, plain = _image(shape)
    _, dropped = _image(shape + "-drop")
    a, b = _levels(plain), _levels(dropped)
    assert a[:, Q_WORDS].any() and not b[:, Q_WORDS].any()  # the LevelParams differ in q_* ...
    rest = [i for i in range(16) if i not in Q_WORDS]
    assert np.array_equal(a[:, rest], b[:, rest])            # ... and in nothing else
    for part in ("frags", "frags_gen", "frags_hot", "gen", "grid16"):
        assert np.array_equal(plain[part], dropped[part])
    p, q = _plan(plain), _plan(dropped)
    assert p["quad_mask"] == 0xFFF and (q["quad_mask"], q["quad_far"]) == (0, 0) and q["grid_bytes"] == dropped["grid16"].size
    assert {k: v for k, v in p.items() if k not in ("quad_mask", "quad_far", "gather_plan", "grid_bytes")} == \
           {k: v for k, v in q.items() if k not in ("quad_mask", "quad_far", "gather_plan", "grid_bytes")}
    # the gather plan is chosen again: nrf_debug_gather_plan's answer at a budget (1 MiB) that grants nothing
    fn = nh.load_library().nrf_debug_gather_plan
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint32)]
    out = (C.c_uint32 * 5)()
    assert fn(C.byref(desc), 1, 1, out) == nh.NRF_OK and R.quad_step_bytes(desc, 0) > 1 << 20
    assert out[0] == q["gather_plan"] and all(f in (0, 1, 2) for f in out[1:])
    _, nosteps = _image(shape + "-nosteps")
    assert np.array_equal(_levels(nosteps), b) and _plan(nosteps)["quad_mask"] == 0


def test_what_the_rows_are_there_for(golden):
    """Each branch the rows were chosen for is taken by the row chosen for it (in the RECORDED values: a row that stopped taking
    its branch would pin nothing)."""
    ln = lambda n: dict(zip(R.PARTS, golden[n]["len"]))
    plan = lambda n: dict(zip(R.PLAN_WORDS, golden[n]["plan"]))
    own = {"base": HOT, "freq12": WIDE, "sh8": WIDE_SH, "w16": W16, "w32": W32, "w128": W128, "d1_1": DEPTH, "d3_4": DEPTH, "act_squareplus": ACT,
           "g1_3": GRID1, "g2_5": GRID2, "g4_8": GRID4, "g8_2": GRID8, "w32_h2_h3": GENERIC, "act_sine": GENERIC, "smoothstep_F4": GRID4,
           "nearest": GRID2, "tiled": HOT}
    assert set(own) == set(R.SHAPES)
    for n, o in own.items():
        p, k = plan(n), ln(n)
        stage = o if o in (HOT, WIDE) else GENERIC
        assert (p["own"], p["stage"]) == (o, stage)
        assert (k["frags_gen"] != 0) == (n == "freq12")            # generic fragments beside the wide ones: the WIDE stage alone
        assert (k["frags_hot"] != 0) == (o != stage)               # an own instance other than the stage one brings its fragments
        assert (k["gen"] != 0) == (stage != HOT)
        assert k["frags"] == (N_FRAGS_WIDE_ALL * 1024 if stage != GENERIC else p["gen_frag_bytes"])
        if o != stage:
            assert k["frags_hot"] == 1024 * {W16: 5, W32: 8, W128: 56, DEPTH: DEPTH_FRAGS, ACT: DEPTH_FRAGS, WIDE_SH: N_FRAGS_WIDE_ALL}.get(o, N_FRAGS)
        assert (p["depth_xd"], p["depth_xr"]) == {"d3_4": (2, 3), "d1_1": (0, 0), "act_squareplus": (0, 1)}.get(n, (0, 0))
    assert DEPTH_FRAGS == DF_WW + 8 * 5 and plan("d3_4")["depth_xd"] + plan("d3_4")["depth_xr"] == 5  # all five extra layers
    # the quad copies: the F = 2 x 16 hash grids behind a register-resident network get them -- steps 0..2 at the default budget, the third
    # beyond 4 GiB (NET_WIDE has no far form), step 0 alone at the step-0 budget, none without steps or after drop_quads
    for n in ("base", "sh8", "w16", "w32", "w128", "d1_1", "d3_4", "act_squareplus"):
        assert (plan(n)["quad_mask"], plan(n)["quad_far"]) == (0xFFF, 0b100) and plan(n)["grid_bytes"] == 0xFFFFFFFF
        assert (plan(n + "-step0")["quad_mask"], plan(n + "-step0")["quad_far"]) == (0xF, 0)
    assert (plan("freq12")["quad_mask"], plan("freq12")["quad_far"]) == (0xFF, 0) and plan("freq12-step0")["quad_mask"] == 0xF
    for n in ("g1_3", "g2_5", "g4_8", "g8_2", "w32_h2_h3", "act_sine", "smoothstep_F4", "nearest", "tiled"):  # (tiled: LV_ADD_POW2 levels take none)
        assert plan(n)["quad_mask"] == plan(n + "-step0")["quad_mask"] == 0 and golden[n] == golden[n + "-step0"]
    for n in R.BUDGET_SHAPES:
        assert plan(n + "-nosteps")["quad_mask"] == plan(n + "-drop")["quad_mask"] == 0
        assert golden[n + "-nosteps"] == golden[n + "-drop"] and golden[n + "-drop"]["crc32"][:5] == golden[n]["crc32"][:5]
        assert golden[n + "-drop"]["crc32"][5] != golden[n]["crc32"][5] != golden[n + "-step0"]["crc32"][5]
    # fast_grid (word 11 of GenModel is not recorded by itself: the two rows' descriptions differ from their Linear F = 2 / F = 4 twins)
    assert golden["nearest"]["crc32"][3] != golden["act_sine"]["crc32"][3] and golden["smoothstep_F4"]["crc32"][3] != golden["g4_8"]["crc32"][3]


def test_fast_grid_of_the_generic_description():
    """GenModel::fast_grid: 1 for F = 2, F for 4 / 8 (Linear, Smoothstep), 0 for F = 1, Nearest and under NRF_GEN_FAST_GRID=0 -- the one
    word of the description that differs between a row and itself with the flag"""
    want = {"sh8": 1, "act_sine": 1, "w32_h2_h3": 1, "g2_5": 1, "g4_8": 4, "smoothstep_F4": 4, "g8_2": 8, "g1_3": 0, "nearest": 0}
    for shape, fast in want.items():
        desc, parts = _image(shape)
        off = R.image(desc, R.QUAD_BUDGET_MB_DEFAULT, R.NO_FAST_GRID)["gen"].view(np.uint32)
        on = parts["gen"].view(np.uint32)
        diff = np.flatnonzero(on != off)
        assert (diff.size == 1 and int(on[diff[0]]) == fast and int(off[diff[0]]) == 0) if fast else diff.size == 0, shape
