"""Dense probe models on the GPU: the two MLPs of every render instance, bit for bit.

A dense probe model (tests/dense_model.py) has dense weight matrices of +1 / -1 whose dot products are exact in fp32 in ANY
summation order on the samples tests/dense_reference.py certifies, and ends every ray at its first sample with weight
exactly 1.  So for every ray that meets occupied space at a certified sample
    pixel rgb == the rgb network's fp16 output at the ray's first march sample, bit for bit, and alpha == 1:
every fp16 store between the layers, the handoff of the density network's outputs, the weight repack and the padding columns
of the instance that rendered the frame are in that value.  The expectation is the float64 chain on the oracle's bit-exact
encodings; tests/test_dense_cpu.py proves on the CPU that the oracle equals it, that at least 0.85 of every frame's hit pixels
are certified, and that an fp16 accumulator, a skipped or truncating hidden store, a moved weight and a stale padding column
each change at least half of them.

What stays at a tolerance, for a stated reason: the uncertified hit pixels (1 .. 4 % of a frame, a direction value or hidden
activation next to zero: two fp32 summation orders may round apart) keep mlp_close's relative bound without its absolute
term, 4 * 2^-11 |want| plus one fp16 ulp of want; the sine / cosine columns of a Frequency model hold zero weights
(v_sin_f32 against sinf, tests/test_probe_gpu.py); sigma of the stage kernels == fp16(exp(g0)) to rtol 2e-3 (v_exp_f32).

The "dense-plan-" legs (dense_model._plan_leg) render base.json's 2^19 table under each static gather plan in every march cell:
the encodings read in the plan's forms in front of both MLPs, the plan asserted before the frame, the addresses after it."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")  # (before anything loads libnerfhip.so: the two then share torch's HIP runtime)
pytestmark = pytest.mark.gpu

import dense_model as dm  # noqa: E402
import dense_reference as dr  # noqa: E402
import nerfhip as nh  # noqa: E402
import oracle_py as op  # noqa: E402
import probe_model as pm  # noqa: E402
import synthetic as syn  # noqa: E402
from test_probe_gpu import _assert_plan, _composited_close, _context, _instance, _plan  # noqa: E402


def _fp16_ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)).astype(np.float16)).astype(np.float64)


_EXPECTED = {}


def _expectation(leg, seed, grid, p):
    """One frame's expectation: dense_model.expected_frame + the oracle's frame, depth and composited samples per ray.  Legs that
    differ in scheduler or output path share it."""
    key = dm.frame_key(leg, seed, grid, p)
    if key not in _EXPECTED:
        W, H = leg["size"]
        cam, pose = syn.default_camera(W, H), dm.poses()[p]
        desc, keep, info = dm.dense_desc(leg["build_kw"], seed, grid, leg["s"])
        o = op.Oracle(desc)
        e = dm.expected_frame(o, cam, pose, W, H, info)
        wantf, wdepth, wst, counts, _ = o.render_rays(cam, pose, W, H, None, schedule=op.SCHED_PER_RAY)
        assert np.array_equal(wantf[..., :3][e["certified"]], e["want"][e["certified"]])  # (the oracle is one fp32 order)
        assert np.all(np.isfinite(e["want"])) and int(counts.sum()) == wst.n_composited
        if len(_EXPECTED) > 6:
            _EXPECTED.clear()
        _EXPECTED[key] = dict(hit=e["hit"], certified=e["certified"], want=e["want"], wantf=wantf, wdepth=wdepth, counts=counts,
                              xyz=e["xyz"], dirs=e["dirs"])
    return _EXPECTED[key]


def _check_frame(what, rgba, depth, exp, covered=None):
    """Every pixel (of `covered`): certified hit pixels for the exact value, the other hit pixels within the summation-order
    bound, both for alpha 1; all others for background and alpha 0."""
    hit, cert, want = exp["hit"], exp["certified"], exp["want"]
    covered = np.ones_like(hit) if covered is None else covered
    c, u, m = cert & covered, hit & ~cert & covered, ~hit & covered
    assert c.sum() + u.sum() + m.sum() == covered.sum() and c.sum() > 0
    bad = (rgba[..., :3][c] != want[c]).any(axis=1)
    assert not bad.any(), (what, f"{int(bad.sum())} of {bad.size} certified hit pixels differ, worst |d| "
                                 f"{float(np.abs(rgba[..., :3][c] - want[c])[bad].max()):.3g}")
    w64 = want[u].astype(np.float64)
    assert np.all(np.abs(rgba[..., :3][u] - w64) <= 4 * 2.0 ** -11 * np.abs(w64) + _fp16_ulp(want[u])), (what, "uncertified hit pixels")
    assert np.all(rgba[..., 3][c | u] == 1.0), (what, "alpha of hit rays")
    assert np.all(rgba[..., 3][m] == 0.0), (what, "alpha of other rays")
    assert np.array_equal(rgba[m], exp["wantf"][m]), (what, "background")
    assert np.abs(depth[covered] - exp["wdepth"][covered]).max() <= 2.0 / 255.0, what


@pytest.mark.parametrize("leg", dm.DENSE_LEGS, ids=[leg["id"] for leg in dm.DENSE_LEGS])
def test_dense_frames_show_both_mlps_exactly(leg):
    persistent = leg["sched"] == "persistent"  # (what runs: pm.plan_sched for the plan-matrix legs)
    runs = leg["own"] if persistent else leg["stage"]  # (instances other than the stage ones have the persistent form only)
    allow_own = int(leg["env"].get("NRF_WIDTH_INSTANCES", "1"))
    budget = int(leg["env"].get("NRF_QUAD_BUDGET_MB", leg["budget_mb"] or 8192))
    W, H = leg["size"]
    opts, option = nh.default_options(), leg["option"]
    if option == "shard1of3":
        opts.shard_index, opts.shard_count = 1, 3
    cam, poses = syn.default_camera(W, H), dm.poses()
    ctx = _context(leg["env"])
    try:
        ctx.set_options(opts)
        ctx.set_resolution(W, H)
        for seed, grid, p in dm.leg_frames(leg):
            desc, keep, info = dm.dense_desc(leg["build_kw"], seed, grid, leg["s"])
            d = nh.ModelDesc.from_buffer_copy(desc)  # (the pointers stay `keep`'s)
            d.gather_copy_budget_mb = leg["budget_mb"]
            ctx.load_model(d)
            # the instance meant is the one that runs
            own, stage, mask, far, _, _ = _plan(d, allow_own, budget)
            assert (own, stage) == (leg["own"], leg["stage"])
            assert _instance(ctx) == pm.INSTANCE_CLASS[runs] + (16 if persistent else 0), (leg["id"], _instance(ctx))
            if "plan" in leg:  # the plan matrix: the static plan meant, read in the form meant
                _assert_plan(ctx, d, leg)
                assert (far != 0) == (leg["plan"] == "qqfh")
                assert sum(2 if (mask >> level) & 1 else 8 for level in range(16)) == leg["addresses"]
            exp, what = _expectation(leg, seed, grid, p), (leg["id"], seed, grid)
            if option == "views3":
                exps = [exp, _expectation(leg, seed, grid, 1 - p), exp]
                ctx.set_max_views(3)
                ctx.render_views(np.stack([cam] * 3), np.stack([poses[p], poses[1 - p], poses[p]]))
                st = ctx.stats()
                for v in range(3):
                    rgba, depth = ctx.read_view_f32(v)
                    _check_frame(what + (v,), rgba, depth, exps[v])
                assert _composited_close(st.n_composited, sum(int(e["counts"].sum()) for e in exps))
                continue
            f = ctx.render(cam, poses[p])
            st = ctx.stats()
            assert leg.get("addresses") in (None, st.gather_addresses_per_sample), (leg["id"], st.gather_addresses_per_sample)
            if option == "shard1of3":
                tps = nh.tiles_per_shard(W, H, 3)
                part, dpart = np.empty((f.n_tiles * 64, 4), np.float32), np.empty(f.n_tiles * 64, np.float32)
                nh._check(ctx.lib.nrf_read_shard_f32(ctx.h, part.ctypes.data, dpart.ctypes.data))
                gathered = np.full((3, tps * 64, 5), np.nan, np.float32)
                gathered[1, :f.n_tiles * 64, :4], gathered[1, :f.n_tiles * 64, 4] = part, dpart
                frame = nh.untile_numpy(gathered, W, H)
                covered = ~np.isnan(frame[..., 4])  # the shard's pixels: a third of the strips
                assert 0.25 * W * H <= covered.sum() <= 0.45 * W * H
                _check_frame(what, frame[..., :4], frame[..., 4], exp, covered)
                assert _composited_close(st.n_composited, int(exp["counts"][covered].sum()))
                continue
            rgba, depth = ctx.read_f32()
            _check_frame(what, rgba, depth, exp)
            assert _composited_close(st.n_composited, int(exp["counts"].sum())), (leg["id"], st.n_composited)
    finally:
        ctx.close()


# --------------------------------------------------------------------------- the stage kernels
STAGE_N = (1, 15, 16, 17, 63, 64, 65, 255, 4099)  # a single row, partly filled 16-row MFMA tiles, many blocks


def _crafted_inputs(info, n, seed):
    """(feat [n][feat_w], dirf [n][dir_w]) as float64 holding fp16 values: feat from fp16 values in [0.3, 0.9], dirf from multiples of
    2^-10 in [-1, 1]; the first rows: all 0.25, all 0.9, zeros, alternating signs in dirf.  The padding columns hold what the
    encodings put there (grid: 0, direction: 1) in every row."""
    feat_raw, feat_w, _, _, _, dir_raw, dir_w = info["shape"]
    rng = np.random.default_rng(seed)
    feat = rng.uniform(0.3, 0.9, (n, feat_w)).astype(np.float16).astype(np.float64)
    dirf = rng.integers(-1024, 1025, (n, dir_w)).astype(np.float64) / 1024.0
    edges = [(0.25, 0.25), (float(np.float16(0.9)), float(np.float16(0.9))), (0.0, 0.0), (0.5, 0.5 * np.resize([1.0, -1.0], dir_w))]
    for i, (fv, dv) in enumerate(edges[:n]):
        feat[i], dirf[i] = fv, dv
    feat[:, feat_raw:] = 0.0
    dirf[:, [c - 16 for c in info["pad_cols"]]] = 1.0
    return feat, dirf


def _as_device_halves(a):
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.float16)).view(np.int16)).cuda()


@pytest.mark.parametrize("name", list(pm.INSTANCES))
def test_dense_mlp_forward_on_crafted_inputs(name):
    """nrf_mlp_forward (the stage kernels: NET_HOT, NET_WIDE, and NET_GENERIC for every other shape) with a dense probe model on
    inputs every row of which is certified: rgb array_equal to the float64 chain, sigma == fp16(exp(g0)) to rtol 2e-3, for
    every n of STAGE_N in a call of its own; nrf_mlp_forward_repeat(3) returns the same bits."""
    kw, own, stage, env = pm.INSTANCES[name]
    desc, keep, info = dm.dense_desc(dict(pm.T12, **kw), dm.SEEDS_OF.get(name, dm.SEEDS)[0], None)
    ctx = _context(env)
    try:
        ctx.load_model(desc)
        assert _plan(desc, int(env.get("NRF_WIDTH_INSTANCES", "1")), 8192)[1] == stage
        for n in STAGE_N:
            feat, dirf = _crafted_inputs(info, n, 100 + n)
            c = dr.chain(info["D"], info["R"], info["act"], feat, dirf)
            assert c["certified"].all() and np.all(np.isfinite(c["rgb"])), (name, n)
            assert n < 15 or len(np.unique(c["rgb"])) > min(n, 300)
            want_sigma = np.exp(c["g"][:, 0].astype(np.float32)).astype(np.float16).astype(np.float32)
            assert np.all(np.isfinite(want_sigma))
            f_d, d_d = _as_device_halves(feat), _as_device_halves(dirf)
            out = torch.full((n, 4), float("nan"), dtype=torch.float16, device="cuda")
            torch.cuda.synchronize()
            ctx.mlp_forward(f_d.data_ptr(), d_d.data_ptr(), n, out.data_ptr())
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            bad = (got[:, :3].astype(np.float32) != c["rgb"]).any(axis=1)
            assert not bad.any(), (name, n, f"{int(bad.sum())} rows differ, the first: {np.flatnonzero(bad)[:8].tolist()}")
            np.testing.assert_allclose(got[:, 3].astype(np.float32), want_sigma, rtol=2e-3)
            if n == STAGE_N[-1]:
                again = torch.full((n, 4), float("nan"), dtype=torch.float16, device="cuda")
                torch.cuda.synchronize()
                ctx.mlp_forward_repeat(f_d.data_ptr(), d_d.data_ptr(), n, again.data_ptr(), 3)
                torch.cuda.synchronize()
                assert np.array_equal(again.cpu().numpy().view(np.uint16), got.view(np.uint16)), (name, "repeat")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["hot", "widesh_8", "generic_w32_h2"])
def test_dense_network_stage_kernels_on_first_samples(name):
    """nrf_network (encodings and both MLPs in one stage kernel) on the first samples of one frame: rgb array_equal to the
    float64 chain on every certified sample."""
    leg = next(leg for leg in dm.DENSE_LEGS if leg["instance"] == name and leg["option"] is None)
    seed, grid, p = dm.leg_frames(leg)[0]
    exp = _expectation(leg, seed, grid, p)
    desc, keep, info = dm.dense_desc(leg["build_kw"], seed, grid, leg["s"])
    hit, cert = exp["hit"].reshape(-1), exp["certified"].reshape(-1)
    xyz, dirs = np.ascontiguousarray(exp["xyz"][hit]), np.ascontiguousarray(exp["dirs"][hit])
    n = len(xyz)
    ctx = _context({})
    try:
        ctx.load_model(desc)
        assert _plan(desc, 1, 8192)[1] == leg["stage"]
        sig = torch.empty(n, dtype=torch.float32, device="cuda")
        rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        x_d, d_d = torch.from_numpy(xyz).cuda(), torch.from_numpy(dirs).cuda()
        torch.cuda.synchronize()
        ctx.network(x_d.data_ptr(), d_d.data_ptr(), n, sig.data_ptr(), rgb.data_ptr())
        torch.cuda.synchronize()
        got, want = rgb.cpu().numpy(), exp["want"].reshape(-1, 3)[hit]
        c = cert[hit]
        assert c.sum() >= 0.85 * n and n >= 500
        bad = (got[c] != want[c]).any(axis=1)
        assert not bad.any(), (name, f"{int(bad.sum())} of {bad.size} certified samples differ")
        w64 = want[~c].astype(np.float64)
        assert np.all(np.abs(got[~c] - w64) <= 4 * 2.0 ** -11 * np.abs(w64) + _fp16_ulp(want[~c]))
        assert np.all(sig.cpu().numpy() > 5e4)
    finally:
        ctx.close()
