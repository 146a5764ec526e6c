"""Probe models: models whose rendered frame shows single encoding values exactly (helper of test_probe_cpu.py and
test_probe_gpu.py; no test in it).

A probe model is any model `models.build_model` makes with its MLP parameters and one table feature replaced:

  * every weight matrix is zero except for single routes of weight +1 / -1, each through its own neuron per layer (a seeded
    permutation: asymmetric), so that rgb[c] = act(s_c * v_c) for one chosen grid feature (through the density MLP into one of
    g[1..15], then through the rgb MLP) or one chosen direction-encoding value.  The sign sits on the route's first weight.
    Every sum has one non-zero product: the summation order of an MFMA cannot matter, every fp16 rounding is an identity;
  * all entries of one grid feature that no route shows (`info["sigma_feature"]`: feature 0 of level 0, or the next one when
    a route shows feature 0) are 1.0 and routed with weight 11 to g[0]: sigma = exp(11) at every sample, alpha == 1.0f with
    any exp, a ray ends at its first sample with weight exactly 1.

So for every ray that meets occupied space: pixel rgb == the fp16 value of the chosen features at the ray's first march
sample, bit for bit, and alpha == 1.  Hidden activation ReLU (rgb = relu(s v)) or None (rgb = s v); rgb output None.

LEGS lists what the GPU file renders and the CPU file proves its conditions for.  FOG_LEGS (at the end): the same models with a
thin density, whose frames show the compositor (test_fog_cpu.py, test_fog_gpu.py).  The "plan matrix" legs of both lists
(PLAN_CELLS) are the ones that run the hot instance under its three static gather plans in every march form: the legs built
on T12 never do (test_plan_matrix_cpu.py)."""
from __future__ import annotations

import numpy as np

import models
import nerfhip as nh
import synthetic as syn

# instance ids (csrc/nrf_launch.h), as in test_instance_plan_cpu.py
HOT, GENERIC, WIDE, W16, W32, W128, WIDE_SH, DEPTH, GRID2, GRID4, GRID8, GRID1, ACT = range(13)
# nrf_debug_instance's class of an instance
INSTANCE_CLASS = {HOT: 0, GENERIC: 1, WIDE: 2, W16: 3, W32: 3, W128: 3, DEPTH: 3, ACT: 3, WIDE_SH: 4, GRID1: 5, GRID2: 5, GRID4: 5, GRID8: 5}

FRAME_W, FRAME_H = 64, 48
SH_C0 = np.float16(0.28209479177387814)  # the degree-0 coefficient: the one direction value that is a constant by definition


def poses(n=2):
    """An orbit pose and a camera inside the volume (test_persistent_gpu._poses("inside", 1)[0]), which look in opposite
    directions: between them every direction value a reduced route set shows takes both signs.  n = 3 (the full legs): one more
    orbit pose, with which that holds for every spherical-harmonics coefficient up to degree 8; n = 4 (Nearest legs, whose
    coarse levels show one table entry per cell): another one, for 300 distinct cells of the coarsest level."""
    return [syn.orbit_pose(222.0, -25.0), syn.orbit_pose(0.0, 20.0, radius=0.4 / 0.33), syn.orbit_pose(90.0, -30.0),
            syn.orbit_pose(310.0, 40.0)][:n]


def random_density_grid(H, cascade, seed, occupied=0.03):
    """A seeded grid with 3 % of every cascade's cells occupied: first samples spread through the volume."""
    rng = np.random.default_rng(seed)
    return (rng.random(cascade * H ** 3) < occupied).astype(np.float32)


_BUILT = {}
NGP_AABB32 = "instant-ngp, aabb_scale 32"
BASE_PLS = "base.json: 2048 / 16 over 15 levels at bound 1"


def _build(build_kw):
    """models.build_model, once per shape (a leg loads several probe models of one shape; nothing of the result is written to)."""
    key = tuple(sorted(build_kw.items()))
    if key not in _BUILT:
        _BUILT.clear()  # (legs of one shape follow each other: one shape's arrays are enough to keep)
        _BUILT[key] = models.build_model(**resolve(build_kw))
    return _BUILT[key]


def resolve(build_kw):
    """build_model's keywords with instant-ngp's per_level_scale at aabb_scale 32 worked out (by the library: not at import)."""
    kw = dict(build_kw)
    if kw.get("per_level_scale") == NGP_AABB32:
        kw["per_level_scale"] = nh.default_per_level_scale(32.0, 16, 16)
    if kw.get("per_level_scale") == BASE_PLS:
        kw["per_level_scale"] = nh.default_per_level_scale(1.0, 16, 16)
    return kw


def probe_desc(build_kw, routes, density_grid=None, seed=0, sigma_weight=11.0):
    """routes: three of ("grid", feature index, sign) / ("dir", value index, sign), one per colour channel.
    density_grid: None (the synthetic object) or "random" (random_density_grid).  sigma_weight: the weight of the constant-1
    feature's route to g[0] (11: every ray ends at its first sample; 1 .. 4.5: a fog, see FOG_LEGS).  Returns (desc, keep, info)."""
    assert len(routes) == 3
    desc, keep, cfg = _build(build_kw)
    feat_raw, feat_w, width, dens_hidden, rgb_hidden, dir_raw, dir_w = shape = syn.network_shape(cfg)
    act = cfg["network"]["activation"]
    assert act in ("ReLU", "None") and cfg["rgb_network"]["activation"] == act and cfg["rgb_network"]["output_activation"] == "None"
    shown = {k for kind, k, _ in routes if kind == "grid"}
    sigma_feature = min(k for k in range(feat_raw) if k not in shown)
    rng = np.random.default_rng(seed)
    sh = cfg["dir_encoding"]["nested"][0]["otype"] == "SphericalHarmonics"
    dir_pad = dir_w - dir_raw if sh else 0  # the padding ones of a SphericalHarmonics encoding come first, any other's last

    def matrices(n_in, hidden):
        dims = [n_in] + [width] * hidden + [16]
        return [np.zeros((dims[i + 1], dims[i]), np.float32) for i in range(len(dims) - 1)]

    D, R = matrices(feat_w, dens_hidden), matrices(16 + dir_w, rgb_hidden)
    # a layer's routes run through different neurons: the first four of a seeded permutation (path 0: sigma)
    d_neurons = [rng.permutation(width)[:4] for _ in range(dens_hidden)]
    r_neurons = [rng.permutation(width)[:3] for _ in range(rgb_hidden)]
    g_slots = 1 + rng.permutation(15)[:3]  # the density outputs g[1..15] the grid routes pass through

    def chain(mats, neurons, path, col, row, first, last=1.0):
        """column `col` of the first matrix -> the path's neuron of every hidden layer -> row `row` of the last matrix"""
        for i, m in enumerate(mats):
            out = row if i == len(mats) - 1 else int(neurons[i][path])
            m[out, col] = (first if i == 0 else 1.0) * (last if i == len(mats) - 1 else 1.0)
            col = out

    chain(D, d_neurons, 0, sigma_feature, 0, 1.0, last=float(sigma_weight))
    for c, (kind, k, sign) in enumerate(routes):
        assert sign in (1, -1)
        if kind == "grid":
            assert 0 <= k < feat_raw
            chain(D, d_neurons, 1 + c, k, int(g_slots[c]), float(sign))
            chain(R, r_neurons, c, int(g_slots[c]), c, 1.0)
        else:
            assert kind == "dir" and 0 <= k < dir_raw
            chain(R, r_neurons, c, 16 + dir_pad + k, c, float(sign))
    mlp = np.concatenate([m.reshape(-1) for m in D + R])
    params = keep[0].copy()
    assert nh.expected_n_params(desc) == params.size
    params[:mlp.size] = mlp
    lt = nh.level_table(desc)
    F = int(desc.n_features_per_level)
    level, f = divmod(sigma_feature, F)
    table = params[mlp.size:].reshape(-1, F)
    assert table.shape[0] == int(lt.offset[desc.n_levels])
    table[int(lt.offset[level]):int(lt.offset[level + 1]), f] = 1.0
    grid = keep[1]
    if density_grid == "random":
        grid = random_density_grid(int(desc.density_grid_size), int(desc.cascade), 77)
        cfg = dict(cfg, snapshot=dict(cfg["snapshot"], mean_density=float(grid.mean())))
    else:
        assert density_grid is None
    desc2, keep2 = nh.desc_from_config(cfg, params, grid)
    info = dict(routes=list(routes), bound=float(desc2.bound), act=act, sigma_feature=sigma_feature, shape=shape, F=F,
                n_levels=int(desc2.n_levels), sigma_weight=float(sigma_weight), frequency=cfg["dir_encoding"]["nested"][0]["otype"] == "Frequency",
                sh=sh, dir_pad=dir_pad)
    return desc2, keep2, info


def pos01(xyz, bound):
    """World position -> [0, 1]: the one statement kernel (nrf_render.h sample_pos01) and oracle (network_one) share, in fp32:
    the product by float(1 / (2 bound)) rounded, then + 0.5 rounded -- two roundings.  Where 1 / (2 bound) is a power of two
    the product is exact and the kernel's single fma gives the same value; where it is not (bound 1.5: float(1 / 3)) the
    kernel takes the multiply-then-add branch, which is this statement.  expected_rgb's assertion judges it against the oracle."""
    w = np.float32(1.0 / (2.0 * float(bound)))
    return (w * np.asarray(xyz, np.float32)).astype(np.float32) + np.float32(0.5)


def dir01(d):
    return (np.float32(0.5) * np.asarray(d, np.float32)).astype(np.float32) + np.float32(0.5)


def expected_values(oracle, xyz, dirs, info, feat=None):
    """act(s * f16 encoding value) of the three routes at world positions / directions, float32 [n][3].  feat: grid features to
    show in place of the oracle's (test_plan_matrix_cpu.py: what a wrong gather would put there)."""
    if feat is None:
        feat = oracle.encode_grid(pos01(xyz, info["bound"])).view(np.float16).astype(np.float32)
    dirf = oracle.encode_dir(dir01(dirs)).view(np.float16).astype(np.float32)
    want = np.empty((len(feat), 3), np.float32)
    for c, (kind, k, sign) in enumerate(info["routes"]):
        v = np.float32(sign) * (feat[:, k] if kind == "grid" else dirf[:, info["dir_pad"] + k])
        want[:, c] = np.maximum(v, np.float32(0.0)) if info["act"] == "ReLU" else v
    return want


def first_samples(oracle, cam, pose, W, H, opts=None):
    """(hit [n], xyz [n][3], dirs [n][3], deltas [n][2]) of every ray's first march sample, rays in pixel order."""
    o, d, nr, fr = oracle.generate_rays(cam, pose, W, H, opts)
    xyz, dirs, deltas = oracle.march(o, d, nr, fr, 1, opts)
    hit = deltas[:, 0, 0] > 0
    xyz, dirs = np.where(hit[:, None], xyz[:, 0], np.float32(0.0)), np.where(hit[:, None], dirs[:, 0], np.float32(0.0))
    return hit, xyz.astype(np.float32), dirs.astype(np.float32), deltas[:, 0]


def expected_rgb(oracle, cam, pose, W, H, info, opts=None):
    """(hit_mask [H][W], want_rgb [H][W][3]; rays that miss: 0).  The oracle's whole network on the first samples must
    return the same values exactly: that checks this file's position map and routing against the oracle's."""
    hit, xyz, dirs, _ = first_samples(oracle, cam, pose, W, H, opts)
    want = expected_values(oracle, xyz, dirs, info)
    sigma, rgb = oracle.network(xyz, dirs)
    assert np.array_equal(rgb[hit], want[hit]) and np.all(sigma[hit] > 5e4)
    want[~hit] = 0.0
    return hit.reshape(H, W), want.reshape(H, W, 3)


# --------------------------------------------------------------------------- routes
def reduced_routes(n_levels, F, dir_raw, start=0):
    """Every grid level once, alternating feature 0 / 1 and the sign from level to level (F = 1: feature 0), then two
    direction values, the last raw one among them; in threes (one model each), the last model padded with further features."""
    r = [("grid", l * F + ((l + start) % 2 if F > 1 else 0), 1 if (l + start) % 2 == 0 else -1) for l in range(n_levels)]
    r += [("dir", dir_raw - 1, 1), ("dir", (1 + start) % max(dir_raw - 1, 1), -1)]
    k = 0
    while len(r) % 3:
        r.append(("grid", (n_levels * F - 1 - k) % (n_levels * F), 1 if k else -1))
        k += 1
    return [r[i:i + 3] for i in range(0, len(r), 3)]


def full_routes(feat_raw, dir_raw):
    """Every grid feature and every direction value in both signs."""
    r = [(kind, k, s) for kind, n in (("grid", feat_raw), ("dir", dir_raw)) for k in range(n) for s in (1, -1)]
    assert len(r) % 3 == 0
    return [r[i:i + 3] for i in range(0, len(r), 3)]


# --------------------------------------------------------------------------- legs
T12 = dict(log2_hashmap_size=12, H=32)
STRIP, PERSISTENT = {"NRF_PERSISTENT": "0"}, {"NRF_PERSISTENT": "1"}
# gather forms of the 16 x 2 instances: (environment, nrf_model_desc.gather_copy_budget_mb, lane addresses per sample).  "None" must
# be none for every geometry (a budget of 1 MB still grants step 0 of a base_resolution 8 grid): the environment's 0.
GATHER = {"none": ({"NRF_QUAD_BUDGET_MB": "0"}, 0, 128), "near": ({}, 256, 80), "far": ({}, 6000, 56)}
NO_GATHER_AXIS = {"-": ({}, 0, None)}

# The plan matrix: base.json's grid (2^19 entries, 16 levels, F = 2, base resolution 16) with per_level_scale pinned to its
# value at bound 1, so that the split between dense and hashed levels (0..4 dense) and with it the steps' forms do not move
# with the bound: without copies {dense, mixed, hashed, hashed}, with 256 MB {quad, quad, hashed, hashed}, with 6000 MB
# {quad, quad, far quad, hashed} -- the three static plans of the hot persistent kernel (csrc/nrf_launch.h), which no T12 model
# reaches without copies and no loader-scaled bound-4 model reaches at 256 MB.  x four march cells.  Everything restated
# here (plan ids, step forms, march forms, whether the march tables can live in LDS) is held to what the library reports by
# test_plan_matrix_cpu.py.
T19 = dict(log2_hashmap_size=19, H=32, per_level_scale=BASE_PLS)
GFORM_MIXED, GFORM_DENSE, GFORM_HASHED, GFORM_QUAD, GFORM_QUAD_FAR = range(5)  # step forms (csrc/nrf_launch.h); the tests' one copy
FORM_GENERIC, FORM_UNIT, FORM_POW2 = 0, 1, 2  # csrc/nrf_launch.h: MARCH_FORM_*
# plan -> (GATHER key, the four steps' forms)
PLANS = {
    "dmhh": ("none", (GFORM_DENSE, GFORM_MIXED, GFORM_HASHED, GFORM_HASHED)),
    "qqhh": ("near", (GFORM_QUAD, GFORM_QUAD, GFORM_HASHED, GFORM_HASHED)),
    "qqfh": ("far", (GFORM_QUAD, GFORM_QUAD, GFORM_QUAD_FAR, GFORM_HASHED)),
}
# cell -> (build_model keywords, march form, whether the grid has the coarse occupancy level the march tables in LDS need).
# generic_h: a grid side that is no multiple of 4 has no coarse level, so NO march table is staged in LDS and the model
# renders in the per-strip kernel, which selects the gather forms at run time: the cell holds the hot strip kernel to the
# references at this table size and reaches no static-plan instance.  generic_b is the cell that runs the three
# MARCH_GENERIC static-plan instances: 1 / (2 bound) is no power of two (pos01's two roundings), mip_bound = min(2^k, bound).
PLAN_CELLS = {
    "unit": (dict(H=32, cascade=1, bound=1.0), FORM_UNIT, True),
    "pow2": (dict(H=32, cascade=3, bound=4.0), FORM_POW2, True),
    "generic_h": (dict(H=30, cascade=1, bound=1.0), FORM_GENERIC, False),
    "generic_b": (dict(H=32, cascade=2, bound=1.5), FORM_GENERIC, True),
}
# what a cell's legs share, whatever their plan (one expectation serves a cell's three plans): (start of the route
# alternation, density grid of the probe legs, fog route set)
PLAN_CELL_MODELS = {"unit": (0, None, 21), "pow2": (1, "random", 22), "generic_h": (0, "random", 23), "generic_b": (1, None, 24)}


def plan_id(forms):
    """gather_plan() of csrc/nrf_launch.h"""
    return 0x10000 | forms[0] | forms[1] << 4 | forms[2] << 8 | forms[3] << 12


def plan_fields(plan, cell):
    """What a plan-matrix leg adds to a leg: the plan and forms nrf_debug_gather_plan must report, the march form, and whether
    the persistent kernel -- the static-plan instances' -- can run it."""
    kw, form, tables = PLAN_CELLS[cell]
    return dict(plan=plan, cell=cell, forms=PLANS[plan][1], plan_id=plan_id(PLANS[plan][1]), march_form=form, lds_tables=tables)


def plan_sched(cell):
    """The kernel that renders a cell's legs.  Their environment asks for the persistent kernel in every cell (NRF_PERSISTENT=1);
    the library gives it where the march tables fit LDS, the per-strip kernel where the grid has no coarse level."""
    return "persistent" if PLAN_CELLS[cell][2] else "strip"

# name -> (build_model keywords, own instance, stage instance, extra environment)
INSTANCES = {
    "hot": ({}, HOT, HOT, {}),
    "wide_freq12": (dict(dir_otype="Frequency", n_frequencies=12), WIDE, WIDE, {}),
    "widesh_5": (dict(sh_degree=5), WIDE_SH, GENERIC, {}),
    "widesh_8": (dict(sh_degree=8), WIDE_SH, GENERIC, {}),
    "w16": (dict(n_neurons=16), W16, GENERIC, {}),
    "w32": (dict(n_neurons=32), W32, GENERIC, {}),
    "w128": (dict(n_neurons=128), W128, GENERIC, {}),
    "depth_d2_2": (dict(density_hidden_layers=2, rgb_hidden_layers=2), DEPTH, GENERIC, {}),
    "depth_d3_4": (dict(density_hidden_layers=3, rgb_hidden_layers=4), DEPTH, GENERIC, {}),
    "depth_d1_1": (dict(density_hidden_layers=1, rgb_hidden_layers=1), DEPTH, GENERIC, {}),
    "act_none": (dict(activation="None"), ACT, GENERIC, {}),
    # GRID_SHAPES of test_generic_gpu.py
    "grid1_g1_16": (dict(n_features_per_level=1), GRID1, GENERIC, {}),
    "grid2_g2_11": (dict(n_levels=11), GRID2, GENERIC, {}),
    "grid4_g4_8": (dict(n_features_per_level=4, n_levels=8), GRID4, GENERIC, {}),
    "grid8_g8_4": (dict(n_features_per_level=8, n_levels=4), GRID8, GENERIC, {}),
    "grid4_g4_6s": (dict(n_features_per_level=4, n_levels=6, interpolation="Smoothstep"), GRID4, GENERIC, {}),
    "grid2_g2_16n": (dict(interpolation="Nearest"), GRID2, GENERIC, {}),
    "generic_w32_width_instances_off": (dict(n_neurons=32), GENERIC, GENERIC, {"NRF_WIDTH_INSTANCES": "0"}),
    "generic_w32_h2": (dict(n_neurons=32, density_hidden_layers=2), GENERIC, GENERIC, {}),
}
QUAD_INSTANCES = ("hot", "wide_freq12", "widesh_5", "widesh_8", "w16", "w32", "w128", "depth_d2_2", "depth_d3_4", "depth_d1_1", "act_none")
GEOMETRIES = {
    "base8": dict(base_resolution=8),
    "base12_pls1.3": dict(base_resolution=12, per_level_scale=1.3),
    "bound4_cascade3": dict(bound=4.0, cascade=3),
    "ngp_aabb32": dict(bound=16.0, cascade=5, per_level_scale=NGP_AABB32),
}
OPTIONS = ("perturb5", "u8", "views3", "shard1of3")


def _leg(name, kw, own, stage, env, gather, routes, grid, option=None, table=T12):
    genv, budget, addresses = dict(GATHER, **NO_GATHER_AXIS)[gather]
    return dict(id=name, build_kw=dict(table, **kw), own=own, stage=stage, env=dict(env, **genv), budget_mb=budget,
                addresses=addresses, routes=routes, density_grid=grid, option=option, full=False, n_poses=2)


def _legs():
    out, n = [], 0
    for name, (kw, own, stage, env) in INSTANCES.items():
        feat_raw, _, _, _, _, dir_raw, _ = syn.network_shape(syn.base_config(**kw))
        F = kw.get("n_features_per_level", 2)
        forms = ("none", "near", "far") if name in QUAD_INSTANCES else ("-",)
        for sched_name, sched in (("persistent", PERSISTENT), ("strip", STRIP)):
            for form in forms:
                if form == "far" and own == WIDE:
                    continue  # NET_WIDE has no far form
                n += 1  # the random grid in every other leg, another start of the alternation from leg to leg
                nearest = kw.get("interpolation") == "Nearest"  # (few cells of a coarse level lie on the object's surface: random grid)
                out.append(dict(_leg(f"{name}-{sched_name}-{form}" if form != "-" else f"{name}-{sched_name}", kw, own, stage,
                                     dict(env, **sched), form, reduced_routes(feat_raw // F, F, dir_raw, start=n % 2),
                                     "random" if n % 2 or nearest else None), n_poses=4 if nearest else 2))
    for gname, kw in GEOMETRIES.items():
        n += 1
        # (how many steps 256 MB hold depends on the geometry: the addresses follow from the plan)
        out.append(dict(_leg(f"hot-geometry-{gname}", kw, HOT, HOT, PERSISTENT, "near", reduced_routes(16, 2, 16, start=n % 2),
                             "random" if n % 2 else None), addresses=None))
    for opt in OPTIONS:
        n += 1
        out.append(_leg(f"hot-option-{opt}", {}, HOT, HOT, PERSISTENT, "near", reduced_routes(16, 2, 16, start=n % 2),
                        "random" if n % 2 else None, option=opt))
    for form in ("none", "far"):
        out.append(dict(_leg(f"hot-full-{form}", {}, HOT, HOT, PERSISTENT, form, full_routes(32, 16), "random" if form == "far" else None),
                        full=True, n_poses=3))
    # the plan matrix: the plan without copies (held to nothing before, and reduced_routes shows every level of its mixed
    # step in both signs) in every march cell; the two copy plans in the cells no exact reference reached
    # (cell by cell: a cell's plans render the same models, whose expectations are made once)
    for cell in PLAN_CELLS:
        for plan in ("dmhh", "qqhh", "qqfh") if cell in ("pow2", "generic_b") else ("dmhh",):
            start, grid, _ = PLAN_CELL_MODELS[cell]
            out.append(dict(_leg(f"plan-{plan}-{cell}", PLAN_CELLS[cell][0], HOT, HOT, PERSISTENT, PLANS[plan][0],
                                 reduced_routes(16, 2, 16, start=start), grid, table=T19), **plan_fields(plan, cell)))
    return out


LEGS = _legs()


def leg_options(leg):
    o = nh.default_options()
    if leg["option"] == "perturb5":
        o.perturb = 5
    return o


def leg_models(leg):
    """(desc, keep, info) of every model of a leg, one per three routes."""
    for i, routes in enumerate(leg["routes"]):
        yield probe_desc(leg["build_kw"], routes, leg["density_grid"], seed=1000 + i)


# --------------------------------------------------------------------------- fog legs
# A fog probe model: a sigma_weight of FOG_WEIGHTS in place of 11 -- sigma = fp16(exp(weight * ~1)) ~ 2.6 / 8.1 / 22 / 79 at every
# sample, still an exact fp16 value, the same bits in kernel and oracle; rays now run through many samples and end with alphas
# spread over (0, 1): the frame shows the compositor.  tests/fog_reference.py restates it in float64 with a derived bound;
# test_fog_cpu.py proves every condition below for every leg, test_fog_gpu.py holds the kernels to the bound.
#
# Every leg renders two models of the same routes and weight, one frame each:
#   the synthetic object from the camera inside the volume -- every ray hits, 100+ samples per ray, which leave the volume with
#     alpha < 1 in a thin fog and stop on the transmittance test in a thick one;
#   random_density_grid from an orbit pose -- short rays through scattered cells, final alphas all over (0, 1), rays that miss.
# (One grid alone cannot give a thick fog both: at sigma 90 the object is opaque but for chords of half a cell, and the
# scattered cells are too few for T to reach 1e-4.)  The strength legs render both poses with both grids.
# The weights are "about 1, 2, 3 and 4.5", moved to the nearest values for which exp(g0) of every g0 = fp16(weight * v), v within
# a few fp16 ulps of 1 (the interpolated constant wobbles), stays 3 * 2^-16 relative away from an fp16 rounding boundary: at
# 1, 3 and 4.5 themselves one of the sigmas sits within 2^-16 of a tie, where v_exp_f32 and libm may round apart
# (test_fog_cpu.py checks the values each leg really meets).  sigma ~ 2.6, 8.1, 21.9, 79.
FOG_WEIGHTS = W1, W2, W3, W4 = (0.96875, 2.09375, 3.0859375, 4.375)
FOG_FRAMES = ((None, 1), ("random", 0))  # (density grid, index into poses())
FOG_SWITCHES = {
    "cap0": {"NRF_SAMPLE_CAP": "0"}, "cap1": {"NRF_SAMPLE_CAP": "1"}, "cap2": {"NRF_SAMPLE_CAP": "2"},
    "tailsplit0": {"NRF_TAIL_SPLIT": "0"}, "marchff0": {"NRF_MARCH_FF": "0"}, "budget3": {"NRF_MARCH_BUDGET": "3"},
}
# name -> (nrf_options fields, sigma weight).  max_steps: around the 8-sample round and not a multiple of it; weight W2: a ray cut
# after 1 .. 37 samples ends with alpha 0.02 .. 0.9
FOG_OPTIONS = {
    "max_steps1": (dict(max_steps=1), W2), "max_steps7": (dict(max_steps=7), W2), "max_steps8": (dict(max_steps=8), W2),
    "max_steps9": (dict(max_steps=9), W2), "max_steps37": (dict(max_steps=37), W2),
    "density_scale0.37": (dict(density_scale=0.37), W4), "density_scale2": (dict(density_scale=2.0), W3),
    "bg0": (dict(bg_color=0.0), W2), "bg0.25": (dict(bg_color=0.25), W3),
    "min_near0.05": (dict(min_near=0.05), W3),
    "dt_gamma0": (dict(dt_gamma=0.0), W3), "dt_gamma1_32": (dict(dt_gamma=1.0 / 32.0), W2),
    "perturb5": (dict(perturb=5), W3),
}
# the "stageoption" legs: stage WIDE, and under stage GENERIC a width instance, a grid instance and the catch-all
FOG_STAGE_OPTION_INSTANCES = ("wide_freq12", "w32", "grid4_g4_8", "generic_w32_h2")
FOG_STAGE_OPTIONS = ("max_steps7", "max_steps9", "density_scale0.37", "density_scale2", "min_near0.05", "dt_gamma0")
FOG_LARGE = (333, 211)  # several strips per queue, and a tail that is split: a 64 x 48 frame is all tail


def fog_routes(L, F, dir_raw, n, frequency):
    """Two features of different fine levels (the upper half: their values change from sample to sample along a ray, so a
    sample left out moves the pixel), in both signs, and a third route: a coarse level, or in every other leg the last
    direction value (constant along a ray: the channel shows the weights alone).  No direction route where the encoding is
    Frequency (v_sin_f32 against sinf: not exact, see test_probe_gpu.py)."""
    half = L // 2

    def level(j):
        return half + (n + j) % (L - half)
    third = ("dir", dir_raw - 1, 1) if n % 2 and not frequency else ("grid", (n % half) * F, 1)
    return [("grid", level(0) * F + n % F, 1), ("grid", level(3) * F + (n + 1) % F, -1), third]


def _fog_leg(family, name, iname, sched, gather, weight, n, frames=FOG_FRAMES, geometry=None, opts_kw=None, option=None, env=None,
             same_as_plain=False, size=(FRAME_W, FRAME_H), table=T12, cell_kw=None):
    kw, own, stage, ienv = INSTANCES[iname]
    kw = dict(kw, **(GEOMETRIES[geometry] if geometry else {}), **(cell_kw or {}))
    feat_raw, _, _, _, _, dir_raw, _ = syn.network_shape(syn.base_config(**INSTANCES[iname][0]))
    F = kw.get("n_features_per_level", 2)
    routes = fog_routes(feat_raw // F, F, dir_raw, n, kw.get("dir_otype") == "Frequency")
    genv, budget, addresses = dict(GATHER, **NO_GATHER_AXIS)[gather]
    sched_env = PERSISTENT if sched == "persistent" else STRIP
    return dict(id=f"fog-{family}-{name}", family=family, instance=iname, sched=sched, gather=gather, build_kw=dict(table, **kw),
                own=own, stage=stage, env=dict(ienv, **sched_env, **genv, **(env or {})), plain_env=dict(ienv, **sched_env, **genv),
                budget_mb=budget, addresses=addresses if geometry is None else None, routes=routes,
                weight=float(weight), frames=tuple(frames), opts_kw=dict(opts_kw or {}), option=option, same_as_plain=same_as_plain,
                size=tuple(size))


def _fog_legs():
    out, n = [], 0
    for w, sigma in zip(FOG_WEIGHTS, ("2.6", "8", "22", "79")):  # every strength with both grids, from both poses
        n += 1
        out.append(_fog_leg("strength", f"sigma{sigma}", "hot", "persistent", "near", w, n,
                            frames=((None, 0), (None, 1), ("random", 0), ("random", 1))))
    for i, (iname, (kw, own, stage, env)) in enumerate(INSTANCES.items()):
        quad = iname in QUAD_INSTANCES
        forms = ("none", "near", "far") if iname == "hot" else ((("none", "near") if own == WIDE else ("none", "near", "far"))[i % (2 if own == WIDE else 3)],) if quad else ("-",)
        n += 1  # (both schedulers and every gather form of an instance render the same models: one restatement serves them)
        for sched in ("persistent", "strip"):
            for form in forms:
                out.append(_fog_leg("instance", f"{iname}-{sched}" + (f"-{form}" if form != "-" else ""), iname, sched, form,
                                    W3 if iname == "hot" else FOG_WEIGHTS[i % 4], n))
    for j, (oname, (opts_kw, w)) in enumerate(FOG_OPTIONS.items()):
        n += 1
        out.append(_fog_leg("option", oname, "hot", ("persistent", "strip")[j % 2], "near", w, n, opts_kw=opts_kw))
    for j, gname in enumerate(("bound4_cascade3", "ngp_aabb32")):
        n += 1
        out.append(_fog_leg("option", f"geometry-{gname}", "hot", ("persistent", "strip")[j % 2], "near", W3, n, geometry=gname))
    hot_n = 5  # the route set of the hot instance legs: the legs below must equal their frames bit for bit
    assert out[4]["instance"] == "hot" and out[4]["routes"] == _fog_leg("x", "x", "hot", "strip", "near", W3, hot_n)["routes"]
    for sched in ("persistent", "strip"):
        for sname, env in FOG_SWITCHES.items():
            if sched == "strip" and sname == "tailsplit0":
                continue  # (tail splitting is the persistent kernel's)
            out.append(_fog_leg("switch", f"{sname}-{sched}", "hot", sched, "near", W3, hot_n, env=env, same_as_plain=True))
        out.append(_fog_leg("output", f"rays-{sched}", "hot", sched, "near", W3, hot_n, option="rays", same_as_plain=True))
    for opt in ("views3", "shard1of3", "u8"):
        out.append(_fog_leg("output", opt, "hot", "persistent", "near", W3, hot_n, option=opt, same_as_plain=True))
    for sched in ("persistent", "strip"):
        out.append(_fog_leg("large", sched, "hot", sched, "near", W3, hot_n, size=FOG_LARGE))
    # the plan matrix: every plan in every march cell; in the cells with several cascades also max_steps 7 and 9 -- rounds that
    # are no multiple of 16 samples, passes of one tile and of two, where a weight-fragment prefetch of the wrong depth shows.
    # "u8planes": the frame once more into 8-bit planes (the OUT_U8 instances) == nrf_quantize_u8 of the float frame
    for cell, (cell_kw, _, _) in PLAN_CELLS.items():
        n_routes = PLAN_CELL_MODELS[cell][2]
        for max_steps in (None, 7, 9) if cell in ("pow2", "generic_b") else (None,):
            for plan, (gather, _) in PLANS.items():
                out.append(dict(_fog_leg("plan", f"{plan}-{cell}" + (f"-max_steps{max_steps}" if max_steps else ""), "hot", "persistent",
                                         gather, W3, n_routes, opts_kw=dict(max_steps=max_steps) if max_steps else None,
                                         option="u8planes" if max_steps is None and cell != "generic_h" else None, table=T19,
                                         cell_kw=cell_kw), sched=plan_sched(cell), **plan_fields(plan, cell)))
    # the options in the stages other than the hot one: the wide and the generic network pass apply density_scale in a line of their
    # own, and every option leg above is the hot instance's.  Each instance renders the models of its own "instance" legs (same route
    # set, same gather form); the scheduler alternates from option to option and from instance to instance, so that under the generic
    # stage every option meets both kernel forms.
    for i, iname in enumerate(FOG_STAGE_OPTION_INSTANCES):
        plain = next(leg for leg in out if leg["family"] == "instance" and leg["instance"] == iname)
        for k, oname in enumerate(FOG_STAGE_OPTIONS):
            opts_kw, w = FOG_OPTIONS[oname]
            leg = _fog_leg("stageoption", f"{iname}-{oname}", iname, ("persistent", "strip")[(i + k) % 2], plain["gather"], w,
                           hot_n + list(INSTANCES).index(iname), opts_kw=opts_kw)
            assert leg["routes"] == plain["routes"] and leg["stage"] != HOT
            out.append(leg)
    return out


FOG_LEGS = _fog_legs()


def fog_options(leg):
    o = nh.default_options()
    for k, v in leg["opts_kw"].items():
        setattr(o, k, v)
    return o


def fog_key(leg):
    """What a leg's restatement depends on: legs that differ in scheduler, gather form, switches or output path share it."""
    return (tuple(sorted(leg["build_kw"].items())), repr(leg["routes"]), leg["weight"], leg["frames"], tuple(sorted(leg["opts_kw"].items())),
            leg["size"])


def fog_models(leg):
    """(desc, keep, info, pose) of every frame of a leg."""
    all_poses = poses(2)
    for grid, p in leg["frames"]:
        desc, keep, info = probe_desc(leg["build_kw"], leg["routes"], grid, seed=3000, sigma_weight=leg["weight"])
        yield desc, keep, info, all_poses[p]
