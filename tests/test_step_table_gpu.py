"""The step table of the barrier fast-forward in the persistent kernel (csrc/nrf_step_plan.h, csrc/nrf_render.h): a frame rendered
with the table equals the frame rendered with NRF_STEP_TABLE=0 -- the stepping loop -- bit for bit, in rgba and depth, with equal
n_composited; and so does the frame of a table cut to 8 entries (NRF_STEP_TABLE_CAP=8), where every barrier lies beyond the table.

The models are fog probe models (tests/probe_model.py: exact fp16 values at every sample, a thin density -- a ray composites many
samples, and one that starts its march a member early or late moves every one of them) of the shapes the other GPU tests use,
plus the bench model.  Frames of 64 x 48 and 33 x 70.  The poses: a camera inside the aabb, where every ray starts at min_near
and is on the table, and the az 0 orbit pose at radius 4.0311, where part of the rays enter through an aabb face and keep the
loop (test_the_orbit_pose_mixes_rays_on_and_off_the_table holds that share to 0.1 .. 0.9 on the CPU oracle)."""
import ctypes as C
import functools

import numpy as np
import pytest

import models
import nerfhip as nh
import oracle_py as op
import probe_model as pm
import synthetic as syn
import test_render_rays_clip_gpu as clip
from test_render_rays_clip_gpu import _bits, _clipped, _context, _upload

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

SIZES = [(64, 48), (33, 70)]
INSIDE = syn.orbit_pose(0.0, 20.0, radius=0.4 / 0.33)
AZ0 = syn.orbit_pose(0.0, 30.0, radius=4.0311)
OFF = {"NRF_STEP_TABLE": "0"}
CAP8 = {"NRF_STEP_TABLE_CAP": "8"}
ROUTES = [("grid", 2, 1), ("grid", 9, -1), ("dir", 1, 1)]
T12 = dict(log2_hashmap_size=12, H=32)
# row -> (build_model keywords, nrf_options fields, environment, views, 8-bit output)
ROWS = {
    "default": (T12, {}, {}, 1, False),
    "min_near0.05": (T12, dict(min_near=0.05), {}, 1, False),
    "min_near0.5": (T12, dict(min_near=0.5), {}, 1, False),
    "dt_gamma0": (T12, dict(dt_gamma=0.0), {}, 1, False),
    "dt_gamma1/64": (T12, dict(dt_gamma=1.0 / 64), {}, 1, False),
    "march_ff_off": (T12, {}, {"NRF_MARCH_FF": "0"}, 1, False),
    "pow2-bound2-cascade2": (dict(T12, bound=2.0, cascade=2), {}, {}, 1, False),
    "h96": (dict(log2_hashmap_size=12, H=96), {}, {}, 1, False),
    "h64-bound1.5-cascade2": (dict(log2_hashmap_size=12, H=64, bound=1.5, cascade=2), {}, {}, 1, False),
    "views3": (T12, {}, {}, 3, False),
    "u8": (T12, {}, {}, 1, True),
}


@functools.lru_cache(maxsize=None)
def _model(key):
    desc, keep, _ = pm.probe_desc(dict(key), ROUTES, None, seed=5, sigma_weight=pm.W3)
    return desc, keep


def _poses(views):
    return [INSIDE, AZ0, syn.orbit_pose(90.0, 30.0)][:max(views, 2)]


def _launch_state(ctx):
    fn = ctx.lib.nrf_debug_step_table_launch
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 3)(-7, -7, -7)
    assert fn(ctx.h, out) == nh.NRF_OK
    return tuple(out)


def _frames(desc, W, H, env, opts, views, u8):
    """Every frame of a row under one environment: [(rgba bits, depth bits, n_composited)], and what the launches were handed"""
    ctx = _context(desc, W, H, dict(clip.PERSISTENT, **env), **opts)
    out = []
    try:
        state = _launch_state(ctx)
        cam = syn.default_camera(W, H)
        if u8:
            rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            d8 = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.bind_output_u8(rgb8.data_ptr(), d8.data_ptr())
        if views > 1:
            ctx.set_max_views(views)
            ctx.render_views(np.stack([cam] * views), np.stack(_poses(views)))
            for v in range(views):
                rgba, depth = ctx.read_view_f32(v)
                out.append((_bits(rgba), _bits(depth), int(ctx.stats().n_composited)))
        else:
            for pose in _poses(1):
                ctx.render(cam, pose)
                if u8:
                    torch.cuda.synchronize()
                    st = ctx.stats()
                    out.append((rgb8.cpu().numpy().copy(), d8.cpu().numpy().copy(), int(st.n_composited)))
                else:
                    rgba, depth = ctx.read_f32()
                    out.append((_bits(rgba), _bits(depth), int(ctx.stats().n_composited)))
    finally:
        ctx.close()
    return out, state


def _same_frames(a, b, what):
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), (what, "frame", i)
        assert x[2] == y[2] and x[2] > 0, (what, "n_composited", i, x[2], y[2])


def test_the_orbit_pose_mixes_rays_on_and_off_the_table():
    """The az 0 pose on the CPU oracle: of the rays that enter the aabb, the share whose near is min_near's bits"""
    desc, _ = _model(tuple(sorted(T12.items())))
    orc = op.Oracle(desc)
    mn = np.float32(nh.default_options().min_near)
    for (W, H) in SIZES:
        for pose, lo, hi in ((AZ0, 0.1, 0.9), (INSIDE, 1.0, 1.0)):
            o, d, near, far = orc.generate_rays(syn.default_camera(W, H), pose, W, H)
            enters = near < far
            share = float(np.mean(_bits(near[enters]) == _bits(mn)))
            print(f"{W}x{H}: {int(enters.sum())} rays enter the aabb, {share:.3f} of them start at min_near")
            assert enters.sum() > 0.5 * W * H and lo <= share <= hi, (W, H, share)


@gpu
@pytest.mark.parametrize("row", list(ROWS))
def test_the_table_changes_no_bit(row):
    build_kw, opts, env, views, u8 = ROWS[row]
    desc, keep = _model(tuple(sorted(build_kw.items())))
    W, H = SIZES[list(ROWS).index(row) % 2]
    on, s_on = _frames(desc, W, H, env, opts, views, u8)
    off, s_off = _frames(desc, W, H, dict(env, **OFF), opts, views, u8)
    cut, s_cut = _frames(desc, W, H, dict(env, **CAP8), opts, views, u8)
    ff = env.get("NRF_MARCH_FF") != "0"
    # the launches were handed what the row says: a staged table, none, a table of 8 entries
    assert (s_on[0] > 8 and s_on[1] > 0 and s_on[2] <= 160 * 1024) if ff else s_on[:2] == (0, -1), (row, s_on)
    assert s_off[:2] == (0, -1), (row, s_off)
    assert (s_cut[0] == 8 and s_cut[1] == s_on[1]) if ff else s_cut[:2] == (0, -1), (row, s_cut)
    _same_frames(on, off, (row, "table against loop"))
    _same_frames(cut, off, (row, "8 entries against loop"))
    if not u8:  # the frames show something: the fog covers part of every frame
        assert all(np.mean(f[0].view(np.float32).reshape(H, W, 4)[..., 3] > 0.05) > 0.05 for f in on), row


@gpu
def test_the_bench_model_at_a_small_frame():
    desc, keep, _ = models.build_model(log2_hashmap_size=19, H=128)
    W, H = 64, 48
    on, s_on = _frames(desc, W, H, {}, {}, 1, False)
    off, s_off = _frames(desc, W, H, OFF, {}, 1, False)
    assert s_on[0] > 8 and s_on[1] > 0 and s_off[:2] == (0, -1), (s_on, s_off)
    _same_frames(on, off, "bench model")


@gpu
@pytest.mark.parametrize("model", ["bound1", "pow2-bound2-cascade2"])
def test_caller_rays_with_half_of_them_on_the_table(model):
    """nrf_render_rays_clipped, its density-only mode and nrf_ray_hits on the inside camera's rays, all of which start at min_near:
    t_min = min_near for the even rays (no limit: they stay on the table), 1.37 min_near for the odd ones (their march starts off it)"""
    build_kw = T12 if model == "bound1" else ROWS[model][0]
    desc, keep = _model(tuple(sorted(build_kw.items())))
    W, H = SIZES[model != "bound1"]
    n = W * H
    mn = np.float32(nh.default_options().min_near)
    t_min = np.where(np.arange(n) % 2 == 0, mn, np.float32(1.37) * mn).astype(np.float32)
    got = {}
    for name, env in (("on", {}), ("off", OFF), ("cut", CAP8)):
        ctx = _context(desc, W, H, dict(clip.PERSISTENT, **env))
        try:
            assert clip._rays_instance(ctx) == 16
            o = torch.empty((n, 3), device="cuda")
            d = torch.empty((n, 3), device="cuda")
            torch.cuda.synchronize()
            ctx.generate_rays(syn.default_camera(W, H), INSIDE, o.data_ptr(), d.data_ptr(), 0, 0)
            tm = _upload(t_min)
            res = []
            for flags in (0, nh.NRF_RAYS_DENSITY_ONLY):
                rgba, depth, st = _clipped(ctx, o, d, n, t_min=tm, flags=flags)
                res.append((_bits(rgba), _bits(depth), int(st.n_composited)))
            ctx.ray_hits(o.data_ptr(), d.data_ptr(), n, 0.5, tm.data_ptr(), 0)
            rec, dep = ctx.read_f32()
            res.append((_bits(rec), _bits(dep), int(ctx.stats().n_composited)))
            got[name] = res
        finally:
            ctx.close()
    _same_frames(got["on"], got["off"], (model, "table against loop"))
    _same_frames(got["cut"], got["off"], (model, "8 entries against loop"))
    # the limit is one: the odd rays' frames differ from an unlimited call's somewhere
    alpha = got["on"][0][0].view(np.float32).reshape(-1, 4)[:, 3]
    assert np.mean(alpha > 0.05) > 0.3, model
