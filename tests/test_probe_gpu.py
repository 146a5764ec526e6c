"""Probe models on the GPU: every instance of the render kernel must show single encoding values exactly.

A probe model (tests/probe_model.py) routes one grid feature or one direction value into each colour channel with weights
+-1 and ends every ray at its first sample with weight exactly 1, so for every ray that meets occupied space
    pixel rgb == act(s * fp16 encoding value at the ray's first march sample), bit for bit, and alpha == 1.
The expectation comes from the oracle's generate_rays + march(n_step = 1) + encode_grid / encode_dir alone: no MLP, no
compositor, no tolerance.  tests/test_probe_cpu.py proves on the CPU that the oracle itself has the property for every leg
below, that no leg passes vacuously (hit rays, distinct values, non-zero values, every level shown), and checks the oracle's
grid encoding against a float64 reference.

The one exception, for a stated arithmetic reason: the direction channels of the Frequency legs (NET_WIDE).  The kernel
evaluates the encoding with v_sin_f32 on arguments up to 2^11 pi, the oracle with libm's sinf (the reference itself uses
__sinf); those channels keep the bound test_generic_gpu.py states for that instruction, 4e-3 absolute.  Their grid channels,
and every channel of every other leg, are compared with array_equal.

The "plan-" legs (probe_model.PLANS x PLAN_CELLS: base.json's 2^19 table) are the ones that run the hot instance's static gather
plans; each asserts the plan and forms the library makes for its model before it renders (_assert_plan)."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # (before anything loads libnerfhip.so: the two then share torch's HIP runtime)
pytestmark = pytest.mark.gpu

import nerfhip as nh  # noqa: E402
import oracle_py as op  # noqa: E402
import probe_model as pm  # noqa: E402
import synthetic as syn  # noqa: E402

W, H = pm.FRAME_W, pm.FRAME_H
FREQUENCY_ATOL = 4e-3  # v_sin_f32 against sinf at 12 frequencies (test_generic_gpu.py)


def _context(env):
    """A context created with `env` in force (the library reads its switches at nrf_create), the environment restored."""
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return nh.NerfHip(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _plan(desc, allow_own, budget_mb):
    lib = nh.load_library()
    lib.nrf_debug_plan.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.nrf_debug_plan.restype = C.c_int
    out = (C.c_uint32 * 6)()
    assert lib.nrf_debug_plan(C.byref(desc), allow_own, budget_mb, out) == nh.NRF_OK
    return tuple(out)


def _instance(ctx):
    ctx.lib.nrf_debug_instance.argtypes = [C.c_void_p]
    return ctx.lib.nrf_debug_instance(ctx.h)


def _context_plan(ctx):
    """The gather plan the context's loaded model launches with (a static plan's id, 0: the run-time selection)"""
    fn = ctx.lib.nrf_debug_context_gather_plan
    fn.argtypes, fn.restype = [C.c_void_p], C.c_longlong
    return int(fn(ctx.h))


def _assert_plan(ctx, desc, leg):
    """A plan-matrix leg (pm.PLANS x pm.PLAN_CELLS), before it renders: the loaded model plans the static gather plan and the
    step forms meant, at the budget the context plans with, and the kernel that runs is the persistent one -- the static-plan
    instances' -- except in the cell whose grid has no coarse level: that one renders in the per-strip kernel."""
    fn = ctx.lib.nrf_debug_gather_plan
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint32)], C.c_int
    out = (C.c_uint32 * 5)()
    budget = int(leg["env"].get("NRF_QUAD_BUDGET_MB", leg["budget_mb"])) or 1  # (0 would ask for the default budget: 1 MB grants no copy)
    assert "NRF_GATHER_PLAN" not in os.environ and fn(C.byref(desc), 1, budget, out) == nh.NRF_OK
    assert (int(out[0]), tuple(out[1:])) == (leg["plan_id"], leg["forms"]), (leg["id"], hex(out[0]), tuple(out[1:]))
    assert _instance(ctx) == (16 if leg["lds_tables"] else 0), (leg["id"], _instance(ctx))
    assert _context_plan(ctx) == leg["plan_id"], (leg["id"], hex(_context_plan(ctx)))  # what the loaded context launches with


_EXPECTED = {}


def _expectations(leg):
    """Per model of the leg: per pose (hit, want rgb, the oracle's frame, depth and composited samples per ray).  Legs that differ in
    scheduler or gather form only share them."""
    key = (tuple(sorted(leg["build_kw"].items())), repr(leg["routes"]), leg["density_grid"], leg["option"], leg["n_poses"])
    if key not in _EXPECTED:
        opts, cam, out = pm.leg_options(leg), syn.default_camera(W, H), []
        for desc, keep, info in pm.leg_models(leg):
            o = op.Oracle(desc)
            frames = []
            for pose in pm.poses(leg["n_poses"]):
                hit, want = pm.expected_rgb(o, cam, pose, W, H, info, opts)
                wantf, wdepth, wst, counts, _ = o.render_rays(cam, pose, W, H, opts, schedule=op.SCHED_PER_RAY)
                assert int(counts.sum()) == wst.n_composited
                frames.append((hit, want, wantf, wdepth, counts))
            out.append(frames)
        if len(_EXPECTED) > 4:
            _EXPECTED.clear()
        _EXPECTED[key] = out
    return _EXPECTED[key]


def _check_frame(what, info, rgba, depth, expected, covered=None):
    """Every pixel (of `covered`) is compared: hit pixels for value and alpha 1, all others for background and alpha 0."""
    hit, want, wantf, wdepth, _ = expected
    covered = np.ones_like(hit) if covered is None else covered
    h, m = hit & covered, ~hit & covered
    assert h.sum() + m.sum() == covered.sum() and h.sum() > 0
    for c, (kind, k, sign) in enumerate(info["routes"]):
        got, exp = rgba[..., c][h], want[..., c][h]
        if kind == "dir" and info["frequency"]:
            assert np.abs(got - exp).max() <= FREQUENCY_ATOL, (what, c, float(np.abs(got - exp).max()))
        else:
            bad = got != exp
            assert not bad.any(), (what, f"channel {c} route {kind} {k} sign {sign}: {int(bad.sum())} of {bad.size} hit pixels differ, "
                                         f"worst |d| {float(np.abs(got - exp)[bad].max()):.3g}")
    assert np.all(rgba[..., 3][h] == 1.0), (what, "alpha of hit rays")
    assert np.all(rgba[..., 3][m] == 0.0), (what, "alpha of other rays")
    assert np.array_equal(rgba[m], wantf[m]), (what, "background")
    assert np.abs(depth[covered] - wdepth[covered]).max() <= 2.0 / 255.0, what


def _composited_close(got, want):
    return abs(int(got) - int(want)) <= 0.002 * want + 8  # (test_render_frame_matches_oracle's allowance for ties)


@pytest.mark.parametrize("leg", pm.LEGS, ids=[leg["id"] for leg in pm.LEGS])
def test_probe_frames_show_the_encoding_exactly(leg):
    # (a grid without the coarse level has no march tables in LDS: the per-strip kernel renders it, pm.PLAN_CELLS generic_h)
    persistent = leg["env"]["NRF_PERSISTENT"] == "1" and leg.get("lds_tables", True)
    runs = leg["own"] if persistent else leg["stage"]  # (instances other than the stage ones have the persistent form only)
    allow_own = int(leg["env"].get("NRF_WIDTH_INSTANCES", "1"))
    budget = int(leg["env"].get("NRF_QUAD_BUDGET_MB", leg["budget_mb"] or 8192))
    opts = pm.leg_options(leg)
    option = leg["option"]
    if option == "shard1of3":
        opts.shard_index, opts.shard_count = 1, 3
    cam, poses = syn.default_camera(W, H), pm.poses(leg["n_poses"])
    expectations = _expectations(leg)
    ctx = _context(leg["env"])
    try:
        ctx.set_options(opts)
        ctx.set_resolution(W, H)
        for i, (desc, keep, info) in enumerate(pm.leg_models(leg)):
            d = nh.ModelDesc.from_buffer_copy(desc)  # (the pointers stay `keep`'s)
            d.gather_copy_budget_mb = leg["budget_mb"]
            ctx.load_model(d)
            # the instance meant is the one that runs, reading the table in the form meant
            own, stage, mask, far, _, _ = _plan(d, allow_own, budget)
            assert (own, stage) == (leg["own"], leg["stage"])
            assert _instance(ctx) == pm.INSTANCE_CLASS[runs] + (16 if persistent else 0), (leg["id"], _instance(ctx))
            nearest = leg["build_kw"].get("interpolation") == "Nearest"
            addresses = sum(2 if (mask >> level) & 1 else (1 if nearest else 8) for level in range(info["n_levels"]))
            assert leg["addresses"] in (None, addresses)
            if leg["id"].endswith("-far") or leg.get("plan") == "qqfh":
                assert far != 0 and (mask >> 8) & 15 == 15  # levels 8..11 come from far copies
            if "plan" in leg:
                _assert_plan(ctx, d, leg)
            what = (leg["id"], i)
            if option == "views3":
                views = poses + [poses[0]]
                ctx.set_max_views(3)
                ctx.render_views(np.stack([cam] * 3), np.stack(views))
                st = ctx.stats()
                assert st.gather_addresses_per_sample == addresses
                for v in range(3):
                    rgba, depth = ctx.read_view_f32(v)
                    _check_frame(what + (v,), info, rgba, depth, expectations[i][v % 2])
                assert _composited_close(st.n_composited, sum(int(expectations[i][v % 2][4].sum()) for v in range(3)))
                continue
            for j, pose in enumerate(poses):
                f = ctx.render(cam, pose)
                st = ctx.stats()
                assert st.gather_addresses_per_sample == addresses, (leg["id"], st.gather_addresses_per_sample)
                if option == "shard1of3":
                    tps = nh.tiles_per_shard(W, H, 3)
                    part, dpart = np.empty((f.n_tiles * 64, 4), np.float32), np.empty(f.n_tiles * 64, np.float32)
                    nh._check(ctx.lib.nrf_read_shard_f32(ctx.h, part.ctypes.data, dpart.ctypes.data))
                    gathered = np.full((3, tps * 64, 5), np.nan, np.float32)
                    gathered[1, :f.n_tiles * 64, :4], gathered[1, :f.n_tiles * 64, 4] = part, dpart
                    frame = nh.untile_numpy(gathered, W, H)
                    covered = ~np.isnan(frame[..., 4])  # the shard's pixels: a third of the strips
                    assert 0.25 * W * H <= covered.sum() <= 0.45 * W * H
                    _check_frame(what + (j,), info, frame[..., :4], frame[..., 4], expectations[i][j], covered)
                    assert _composited_close(st.n_composited, int(expectations[i][j][4][covered].sum()))
                    continue
                rgba, depth = ctx.read_f32()
                _check_frame(what + (j,), info, rgba, depth, expectations[i][j])
                assert _composited_close(st.n_composited, int(expectations[i][j][4].sum())), (leg["id"], st.n_composited)
                if option == "u8":  # the packed 8-bit output of the kernel == the quantised float frame that was just checked
                    got = torch.full((H * W,), 0x07070707, dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()
                    ctx.bind_output_rgbd8(got.data_ptr())
                    ctx.render(cam, pose)
                    torch.cuda.synchronize()
                    ctx.bind_output_rgbd8(0)
                    rgb8, d8 = op.quantize_u8(rgba, depth)
                    packed = (rgb8[..., 0].astype(np.uint32) | rgb8[..., 1].astype(np.uint32) << 8 | rgb8[..., 2].astype(np.uint32) << 16 |
                              d8.astype(np.uint32) << 24)
                    assert np.array_equal(got.cpu().numpy().view(np.uint32).reshape(H, W), packed)
    finally:
        ctx.close()


# --------------------------------------------------------------------------- the stage kernels on chosen positions
def _chosen_positions(desc, rng, n_random):
    """World positions [n][3] at bound 1 (p01 = pm.pos01(xyz, 1): every position is built from the world coordinate, so the
    map reproduces the intended p01 bit for bit, which the caller checks).  Per level and several cells k (1, the middle, the
    last one a position reaches: res - 1 where the level's scale is whole, res - 2 otherwise) the smallest coordinate whose
    grid position fp32(fp32(p01 * scale) + 0.5f) reaches k (fraction 0, or the smallest one where no float gives k itself)
    and its predecessor among the multiples of 2^-24 (the largest fraction of cell k - 1); cell 0 from p01 = 0; the corners
    and face centres of the unit cube, 2^-24 and 1 - 2^-24; uniform ones."""
    lt = nh.level_table(desc)
    f32 = np.float32
    unit = [np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], f32),
            np.array([[0.5, 0.5, 0], [0.5, 0.5, 1], [0.5, 0, 0.5], [0.5, 1, 0.5], [0, 0.5, 0.5], [1, 0.5, 0.5],
                      [1 - 2 ** -24, 2 ** -24, 0.5], [2 ** -24, 0.5, 1 - 2 ** -24]], f32)]
    pos = [(f32(2.0) * a - f32(1.0)).astype(f32) for a in unit]  # (exact: the coordinates are 0, 1/2, 1, 2^-24, 1 - 2^-24)
    assert all(np.array_equal(pm.pos01(x, 1.0), a) for x, a in zip(pos, unit))
    n_boundaries = 0
    for level in range(int(desc.n_levels)):
        res, scale = int(lt.resolution[level]), f32(lt.scale[level])

        def g(x):
            return f32(f32(pm.pos01(f32(x), 1.0) * scale) + f32(0.5))
        last = int(g(1.0))
        assert res - 2 <= last <= res - 1 and g(-1.0) == 0.5  # (cell 0 starts at fraction one half)
        for k in (1, res // 2, last):
            lo, hi = -2 ** 24, 2 ** 24  # world coordinates i 2^-24: bisect for the smallest one with g >= k (g is monotone)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if g(mid * 2.0 ** -24) >= k else (mid, hi)
            x, y = f32(hi * 2.0 ** -24), f32(lo * 2.0 ** -24)
            assert -1 < y < x <= 1 and k <= g(x) < k + 2.0 ** -10 and k - 2.0 ** -10 < g(y) < k, (level, k, g(x), g(y))
            n_boundaries += 1
            pos.append(np.array([[x, -0.375, 0.375], [y, -0.375, 0.375], [0.25, x, y], [y, -0.75, x], [-1, y, x]], f32))
    assert n_boundaries == 3 * int(desc.n_levels)
    n_special = sum(len(a) for a in pos)
    return np.concatenate(pos + [rng.uniform(-1.0, 1.0, (n_random, 3)).astype(f32)]), n_special


STAGE_LEGS = [(name, form) for name in ("hot", "wide_freq12", "generic_w32_h2")
              for form in (("none", "near", "far") if name == "hot" else ("none", "near") if name == "wide_freq12" else ("-",))]


@pytest.mark.parametrize("name,form", STAGE_LEGS, ids=[f"{n}-{f}" for n, f in STAGE_LEGS])
def test_probe_network_stage_kernels_on_chosen_positions(name, form):
    """nrf_network (the three stage kernels: NET_HOT, NET_WIDE, NET_GENERIC) with probe models on chosen positions: cell
    boundaries of every level from both sides, the cube's corners and faces, 20 000 uniform ones.  rgb == act(s * encoding),
    array_equal (Frequency direction channels: see the module's docstring).  Every position is a world position at bound 1
    whose map to [0, 1] is the intended p01 by construction (_chosen_positions)."""
    kw, own, stage, env = pm.INSTANCES[name]
    genv, budget, addresses = dict(pm.GATHER, **pm.NO_GATHER_AXIS)[form]
    feat_raw, _, _, _, _, dir_raw, _ = syn.network_shape(syn.base_config(**kw))
    rng = np.random.default_rng(31)
    ctx = _context(dict(env, **genv))
    try:
        for i, routes in enumerate(pm.reduced_routes(feat_raw // 2, 2, dir_raw, start=len(form) % 2)):
            desc, keep, info = pm.probe_desc(dict(pm.T12, **kw), routes, None, seed=2000 + i)
            xyz, n_special = _chosen_positions(desc, rng, 20000)
            p01 = pm.pos01(xyz, 1.0)
            assert p01.min() == 0.0 and p01.max() == 1.0 and n_special > 15 * info["n_levels"]
            dirs = rng.normal(size=(len(xyz), 3)).astype(np.float32)
            dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            want = pm.expected_values(op.Oracle(desc), xyz, dirs, info)
            d = nh.ModelDesc.from_buffer_copy(desc)
            d.gather_copy_budget_mb = budget
            ctx.load_model(d)
            assert _plan(d, 1, int(genv.get("NRF_QUAD_BUDGET_MB", budget or 8192)))[1] == stage == own
            n = len(xyz)
            sig = torch.empty(n, dtype=torch.float32, device="cuda")
            rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            x_d, d_d = torch.from_numpy(xyz).cuda(), torch.from_numpy(dirs).cuda()
            torch.cuda.synchronize()
            ctx.network(x_d.data_ptr(), d_d.data_ptr(), n, sig.data_ptr(), rgb.data_ptr())
            got = rgb.cpu().numpy()
            assert np.all(sig.cpu().numpy() > 5e4)
            for c, (kind, k, sign) in enumerate(routes):
                if kind == "dir" and info["frequency"]:
                    assert np.abs(got[:, c] - want[:, c]).max() <= FREQUENCY_ATOL
                else:
                    bad = got[:, c] != want[:, c]
                    assert not bad.any(), (name, form, kind, k, sign, int(bad.sum()), float(np.abs(got[:, c] - want[:, c]).max()))
                assert len(np.unique(want[:, c])) >= 300 and (want[:, c] != 0).mean() >= 0.10
    finally:
        ctx.close()
