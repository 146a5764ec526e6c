"""Fog probe models on the GPU: the compositing half of every render instance against a float64 restatement.

A fog probe model (tests/probe_model.py, FOG_LEGS) has per-sample rgb and sigma that are exact fp16 values, the same bits in
the kernel and in the oracle; rays run through 5 .. 150 samples and end with alphas spread over (0, 1).  The only arithmetic
in which a kernel may differ from tests/fog_reference.py's float64 chain is the fp32 compositing loop and its exp, so on
EVERY pixel rgba and depth must lie within the per-ray bound derived there (median 1e-6 .. 3e-5, largest 9e-5; the frame
tests allow 2/255 = 7.8e-3), pixels that miss are the background exactly, and stats().n_composited differs from the
oracle's count by no more than the number of rays with a transmittance inside the stop window.  Legs that change a switch,
the output path or the source of the rays also equal the plain leg's frame bit for bit.  tests/test_fog_cpu.py proves on
the CPU that the oracle itself satisfies all of it for every leg, that no sigma sits on an fp16 tie, that no leg passes
vacuously and that the bound sees a dropped sample, a stop threshold of 1e-3 and max_steps off by one.

Measured worst error / bound (rgba and depth) per leg family on an MI355X, the oracle's own ratio on the same legs in brackets:
    strength 0.56 (0.56), instance 0.41 (0.41), option 0.40 (0.40), switch 0.34 (0.34), output 0.34 (0.34), large 0.37 (0.37),
    stageoption 0.40 (0.40): the options under the wide and generic stages; leg by leg the two ratios are equal but under
    density_scale2 (0.19 .. 0.24 against the oracle's 0.18) and in generic_w32_h2 under max_steps 7 and 9 (0.18 against 0.16);
    chained nrf_composite: state 0.17, depth sum 0.22 (oracle 0.16 / 0.22).  `pytest -s` prints every frame's ratios.

The "fog-plan-" legs (probe_model.PLANS x PLAN_CELLS) run the hot instance's three static gather plans in every march cell, with
max_steps 7 and 9 in the cascaded ones, and render the frame once more into 8-bit planes (the OUT_U8 instances), which must
equal nrf_quantize_u8 of the float frame byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # (before anything loads libnerfhip.so: the two then share torch's HIP runtime)
pytestmark = pytest.mark.gpu

import fog_reference as fr  # noqa: E402
import nerfhip as nh  # noqa: E402
import oracle_py as op  # noqa: E402
import probe_model as pm  # noqa: E402
import synthetic as syn  # noqa: E402
from test_probe_gpu import _assert_plan  # noqa: E402


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


def _rays_instance(ctx):
    fn = ctx.lib.nrf_debug_rays_instance
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    return int(fn(ctx.h))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_EXPECTED = {}


def _expectations(leg):
    """Per frame of the leg: the float64 frame, its bounds, the stop-window rays and the oracle's per-ray counts.  Legs that
    differ in scheduler, gather form, switch or output path share them."""
    key = pm.fog_key(leg)
    if key not in _EXPECTED:
        W, H = leg["size"]
        opts, cam, out = pm.fog_options(leg), syn.default_camera(W, H), []
        for desc, keep, info, pose in pm.fog_models(leg):
            o = op.Oracle(desc)
            s, st, rgba, depth, b, db, window = fr.restate(o, info, cam, pose, W, H, opts)
            want, wdepth, wst, counts, _ = o.render_rays(cam, pose, W, H, opts, schedule=op.SCHED_PER_RAY)
            hit = st["count"].reshape(H, W) > 0
            oracle_ratio = max(float((np.abs(want - rgba).max(axis=2)[hit] / b[hit]).max()), float((np.abs(wdepth - depth)[hit] / db[hit]).max()))
            out.append(dict(rgba=rgba, depth=depth, b=b, db=db, window=window, hit=hit, counts=counts, oracle_ratio=oracle_ratio))
        if len(_EXPECTED) > 6:
            _EXPECTED.clear()
        _EXPECTED[key] = out
    return _EXPECTED[key]


def _check_frame(what, opts, rgba, depth, exp, covered=None):
    """Every pixel (of `covered`): hit pixels within the ray's bound of the float64 frame, all others the background exactly.
    Returns the worst error / bound."""
    hit = exp["hit"]
    covered = np.ones_like(hit) if covered is None else covered
    h, m = hit & covered, ~hit & covered
    assert h.sum() + m.sum() == covered.sum() and h.sum() > 0
    assert np.all(np.isfinite(rgba[covered])) and np.all(np.isfinite(depth[covered]))
    err, derr = np.abs(rgba - exp["rgba"]).max(axis=2), np.abs(depth - exp["depth"])
    ratio, dratio = float((err[h] / exp["b"][h]).max()), float((derr[h] / exp["db"][h]).max())
    print(f"fog-gpu {what}: worst error / bound rgba {ratio:.3f} depth {dratio:.3f} (oracle {exp['oracle_ratio']:.3f}); "
          f"worst error {float(err[h].max()):.2e}")
    bad = h & (err > exp["b"])
    assert not bad.any(), (what, f"{int(bad.sum())} of {int(h.sum())} hit pixels outside the bound, worst error / bound {ratio:.2f} at pixel "
                                 f"{np.unravel_index(np.argmax(np.where(h, err / np.where(exp['b'] > 0, exp['b'], np.inf), 0)), hit.shape)}")
    assert np.all(derr[h] <= exp["db"][h]), (what, "depth", dratio)
    bg = np.float32(opts.bg_color)
    assert np.all(rgba[m][:, :3] == bg) and np.all(rgba[m][:, 3] == 0.0) and np.all(depth[m] == 0.0), (what, "background")
    return max(ratio, dratio)


def _composited_close(what, st, exp_frames, covered=None):
    """n_composited within the number of stop-window rays of the oracle's count; n_samples >= n_composited."""
    want = sum(int(e["counts"][covered].sum()) if covered is not None else int(e["counts"].sum()) for e in exp_frames)
    slack = sum(int(e["window"][covered].sum()) if covered is not None else int(e["window"].sum()) for e in exp_frames)
    assert abs(int(st.n_composited) - want) <= slack, (what, int(st.n_composited), want, slack)
    assert st.n_samples >= st.n_composited > 0, what


def _load(ctx, leg, desc):
    d = nh.ModelDesc.from_buffer_copy(desc)  # (the pointers stay the caller's `keep`'s)
    d.gather_copy_budget_mb = leg["budget_mb"]
    ctx.load_model(d)
    return d


_PLAIN = {}


def _plain_frames(leg, extra_pose):
    """The frames (and the extra pose's, for the views leg) of the leg's models from a context without the leg's switch:
    [(rgba, depth, n_composited)] per model, [..] of the extra pose per model."""
    key = (pm.fog_key(leg), tuple(sorted(leg["plain_env"].items())))
    if key not in _PLAIN:
        W, H = leg["size"]
        cam = syn.default_camera(W, H)
        ctx = _context(leg["plain_env"])
        try:
            ctx.set_options(pm.fog_options(leg))
            ctx.set_resolution(W, H)
            out = []
            for desc, keep, info, pose in pm.fog_models(leg):
                _load(ctx, leg, desc)
                frames = []
                for p in (pose, extra_pose):
                    ctx.render(cam, p)
                    rgba, depth = ctx.read_f32()
                    frames.append((rgba.copy(), depth.copy(), int(ctx.stats().n_composited)))
                out.append(frames)
        finally:
            ctx.close()
        _PLAIN.clear()
        _PLAIN[key] = out
    return _PLAIN[key]


@pytest.mark.parametrize("leg", pm.FOG_LEGS, ids=[leg["id"] for leg in pm.FOG_LEGS])
def test_fog_frames_stay_within_the_compositing_bound(leg):
    persistent = leg["sched"] == "persistent"  # (what runs: pm.plan_sched for the plan-matrix legs)
    runs = leg["own"] if persistent else leg["stage"]  # (instances other than the stage ones have the persistent form only)
    allow_own = int(leg["env"].get("NRF_WIDTH_INSTANCES", "1"))
    budget = int(leg["env"].get("NRF_QUAD_BUDGET_MB", leg["budget_mb"] or 8192))
    W, H = leg["size"]
    opts, option = pm.fog_options(leg), leg["option"]
    if option == "shard1of3":
        opts.shard_index, opts.shard_count = 1, 3
    cam = syn.default_camera(W, H)
    extra_pose = pm.poses(3)[2]
    expectations = _expectations(leg)
    plain = _plain_frames(leg, extra_pose) if leg["same_as_plain"] else None
    worst = 0.0
    ctx = _context(leg["env"])
    try:
        ctx.set_options(opts)
        ctx.set_resolution(W, H)
        for i, (desc, keep, info, pose) in enumerate(pm.fog_models(leg)):
            d = _load(ctx, leg, desc)
            exp, what = expectations[i], f"{leg['id']} frame {i}"
            # the instance meant is the one that runs, reading the table in the form meant
            own, stage, mask, far, _, _ = _plan(d, allow_own, budget)
            assert (own, stage) == (leg["own"], leg["stage"])
            assert _instance(ctx) == pm.INSTANCE_CLASS[runs] + (16 if persistent else 0), (leg["id"], _instance(ctx))
            nearest = leg["build_kw"].get("interpolation") == "Nearest"
            addresses = sum(2 if (mask >> level) & 1 else (1 if nearest else 8) for level in range(info["n_levels"]))
            assert leg["addresses"] in (None, addresses)
            if leg["gather"] == "far":
                assert far != 0 and (mask >> 8) & 15 == 15  # levels 8..11 come from far copies
            if "plan" in leg:
                _assert_plan(ctx, d, leg)
            if option == "views3":
                ctx.set_max_views(3)
                ctx.render_views(np.stack([cam] * 3), np.stack([pose, extra_pose, pose]))
                st = ctx.stats()
                for v in range(3):
                    rgba, depth = ctx.read_view_f32(v)
                    if v != 1:
                        worst = max(worst, _check_frame(f"{what} view {v}", opts, rgba, depth, exp))
                    assert np.array_equal(_bits(rgba), _bits(plain[i][v % 2][0])) and np.array_equal(_bits(depth), _bits(plain[i][v % 2][1])), (what, v)
                assert st.n_composited == 2 * plain[i][0][2] + plain[i][1][2] and st.n_samples >= st.n_composited
                continue
            if option == "rays":
                assert _rays_instance(ctx) == (16 if persistent else 0)
                ro, rd = torch.empty((H * W, 3), device="cuda"), torch.empty((H * W, 3), device="cuda")
                torch.cuda.synchronize()
                ctx.generate_rays(cam, pose, ro.data_ptr(), rd.data_ptr(), 0, 0)
                f = ctx.render_rays(ro.data_ptr(), rd.data_ptr(), W * H)
            else:
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
                worst = max(worst, _check_frame(what, opts, np.nan_to_num(frame[..., :4]), np.nan_to_num(frame[..., 4]), exp, covered))
                _composited_close(what, st, [exp], covered)
                assert np.array_equal(_bits(frame[..., :4][covered]), _bits(plain[i][0][0][covered]))
                assert np.array_equal(_bits(frame[..., 4][covered]), _bits(plain[i][0][1][covered]))
                continue
            rgba, depth = ctx.read_f32()
            worst = max(worst, _check_frame(what, opts, rgba, depth, exp))
            _composited_close(what, st, [exp])
            if leg["same_as_plain"]:
                assert np.array_equal(_bits(rgba), _bits(plain[i][0][0])) and np.array_equal(_bits(depth), _bits(plain[i][0][1])), what
                assert st.n_composited == plain[i][0][2], what
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
            if option == "u8planes":  # the OUT_U8 instance of the same plan and march form: its bytes == nrf_quantize_u8 of the float frame
                n_px = W * H
                src, dsrc = torch.from_numpy(rgba.reshape(-1, 4)).cuda(), torch.from_numpy(depth.reshape(-1)).cuda()
                want8, wantd8 = torch.full((n_px, 3), 77, dtype=torch.uint8, device="cuda"), torch.full((n_px,), 78, dtype=torch.uint8, device="cuda")
                got8, gotd8 = torch.full((n_px, 3), 79, dtype=torch.uint8, device="cuda"), torch.full((n_px,), 80, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ctx.quantize_u8(src.data_ptr(), dsrc.data_ptr(), n_px, want8.data_ptr(), wantd8.data_ptr())
                ctx.bind_output_u8(got8.data_ptr(), gotd8.data_ptr())
                ctx.render(cam, pose)
                st8 = ctx.stats()
                torch.cuda.synchronize()
                ctx.bind_output_u8(0, 0)
                assert st8.n_composited == st.n_composited and st8.gather_addresses_per_sample == addresses, what
                assert np.array_equal(got8.cpu().numpy(), want8.cpu().numpy()) and np.array_equal(gotd8.cpu().numpy(), wantd8.cpu().numpy()), what
                assert len(np.unique(want8.cpu().numpy())) > 16  # (a picture: more byte values than a flat frame or a fill pattern holds)
    finally:
        ctx.close()
    print(f"fog-gpu-leg {leg['family']} {leg['id']}: worst error / bound {worst:.3f} (oracle {max(e['oracle_ratio'] for e in expectations):.3f})")


# --------------------------------------------------------------------------- the nrf_composite stage, chained
def test_composite_stage_chained_calls_against_the_float64_chain():
    """nrf_composite three times in a row, carrying `state` and `rays_t`, on inputs with sigma == 0, alpha == 1, zero-filled
    unused slots and rays that die in the first call -- against the float64 chain with its derived bound
    (fog_reference.check_chained_composite; test_fog_cpu.py holds the oracle's composite to the same)."""
    n, n_step = 6000, 8
    ctx = nh.NerfHip(0)

    def on_gpu(sig, col, dl, rays_t, state):
        ts = [torch.from_numpy(a).cuda() for a in (sig, col, dl, rays_t, state)]
        torch.cuda.synchronize()
        ctx.composite(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), n, n_step, ts[3].data_ptr(), ts[4].data_ptr())
        torch.cuda.synchronize()
        return ts[3].cpu().numpy(), ts[4].cpu().numpy()

    try:
        fr.check_chained_composite("kernel", on_gpu, n=n, calls=3, n_step=n_step)
    finally:
        ctx.close()
