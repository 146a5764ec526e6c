"""The frame plan (csrc/nrf_frame_plan.h) on the device: what nrf_debug_frame_plan says of a call is what the call does.  The bytes
a host frame's copies move are the plan's, call by call, while the frames stay byte-equal to nrf_read_u8 of a fresh context; a
call of more views than one launch takes renders each view as a call of its own does; the shards of a frame that is no multiple
of a tile, untiled, are the single-shard frame bit for bit in both forms of the kernel."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_plan_rows as fr
import grid_plan_rows as gp
import models
import nerfhip as nh
import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def model():
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, H=32)
    return desc, keep, cfg


def _context(desc, env=None, shard=(0, 1)):
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = nh.NerfHip(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    ctx.load_model(desc)
    o = nh.default_options()
    o.shard_index, o.shard_count = shard
    ctx.set_options(o)
    return ctx


def _reference_u8(desc, W, H, cams, poses, opts=None):
    ctx = _context(desc)
    if opts is not None:
        ctx.set_options(opts)
    ctx.set_resolution(W, H)
    out = []
    for c, p in zip(cams, poses):
        ctx.render(c, p)
        out.append(ctx.read_u8())
    ctx.close()
    return out


def _predicted_bytes(ctx, desc, W, H, cams, poses, rgb_only, bg=1.0):
    """copied_bytes of nrf_debug_frame_plan for the call, from the loaded context's own occupied box"""
    ctx.lib.nrf_debug_instance.argtypes = [C.c_void_p]
    assert ctx.lib.nrf_debug_instance(ctx.h) >= 16  # the persistent kernel with its tables in LDS: progressive copies are possible
    _, box, _ = gp.readout(ctx)
    row = fr._row("call", W, H, cams=cams, poses=poses, box=tuple(float(v) for v in box), scale=float(desc.scale), bg=bg,
                  flags=fr.HOST | fr.COLS | fr.PROGRESSIVE | fr.HAVE_PLAN | (0 if rgb_only else fr.DEPTH))
    return fr.plan(row).head


def test_a_lone_frames_copied_bytes_are_the_plans(model):
    """the call sequence of test_region_of_interest_narrower_than_the_frame_travels_by_columns (tests/test_host_frames_gpu.py)"""
    desc, keep, cfg = model
    W, H = 640, 360
    seq = [(cam, pose) for name, w, h, cam, pose, box in fr.camera_rows() if name.startswith("shift-")]
    assert len(seq) == 9
    ctx = _context(desc)
    ctx.set_resolution(W, H)
    narrow = 0
    for bg, flags in ((1.0, 0), (0.25, 0), (0.25, nh.NRF_HOST_RGB_ONLY)):
        o = nh.default_options()
        o.bg_color = bg
        ctx.set_options(o)
        want = _reference_u8(desc, W, H, [c for c, _ in seq], [p for _, p in seq], o)
        for i, (cam, pose) in enumerate(seq):
            f = ctx.render_host_u8_raw(np.ascontiguousarray(cam, np.float32).reshape(1, 4), np.ascontiguousarray(pose, np.float32).reshape(1, 16), flags)
            rgb, depth = nh._host_frame_arrays(f, False)
            np.testing.assert_array_equal(rgb[0], want[i][0], err_msg=f"rgb, bg {bg}, flags {flags}, call {i}")
            if not flags:
                np.testing.assert_array_equal(depth[0], want[i][1], err_msg=f"depth, bg {bg}, call {i}")
            head = _predicted_bytes(ctx, desc, W, H, [cam], [pose], bool(flags), bg)
            assert head["progressive"] == 0 and int(f.copied_bytes) == head["copied_bytes"], (bg, flags, i, int(f.copied_bytes), head["copied_bytes"])
            narrow += 0 < head["copied_bytes"] < W * H * (3 if flags else 4) * 0.6
    assert narrow >= 6
    ctx.close()


@pytest.mark.parametrize("W,H,n_views", [(96, 56, 16), (480, 272, 3)])
def test_a_progressive_calls_copied_bytes_are_the_plans(model, W, H, n_views):
    desc, keep, cfg = model
    poses = [syn.orbit_pose(25.0 * i, 20 + (i % 3) * 10, radius=(4.0311 if i % 4 else 9.0)) for i in range(n_views)]
    cams = [syn.default_camera(W, H)] * n_views
    want = _reference_u8(desc, W, H, cams, poses)
    ctx = _context(desc)
    ctx.set_max_views(n_views)
    ctx.set_resolution(W, H)
    for rgb_only in (False, True):
        for rep in range(2):  # both slots
            f = ctx.render_host_u8_raw(np.ascontiguousarray(cams, np.float32), np.ascontiguousarray(poses, np.float32).reshape(-1, 16),
                                       nh.NRF_HOST_RGB_ONLY if rgb_only else 0)
            rgb, depth = nh._host_frame_arrays(f, False)
            for i in range(n_views):
                np.testing.assert_array_equal(rgb[i], want[i][0], err_msg=f"rgb view {i} pass {rep}")
                if not rgb_only:
                    np.testing.assert_array_equal(depth[i], want[i][1], err_msg=f"depth view {i} pass {rep}")
            head = _predicted_bytes(ctx, desc, W, H, cams, poses, rgb_only)
            assert head["progressive"] == 1 and head["n_bands"] >= 1
            assert int(f.copied_bytes) == head["copied_bytes"], (rgb_only, rep, int(f.copied_bytes), head["copied_bytes"])
    ctx.close()


def test_a_call_of_130_views_takes_two_launches_and_equals_single_renders(model):
    desc, keep, cfg = model
    W, H, n = 36, 20, nh.NRF_MAX_VIEWS + 2
    poses = [syn.orbit_pose(11.0 * i, 10.0 + 7.0 * (i % 5), radius=(4.0311 if i % 3 else 6.0)) for i in range(n)]
    cam = syn.default_camera(W, H)
    assert fr.plan(fr._row("call", W, H, rois=[fr.region("full", W, H)] * n)).head["launch_views"] == nh.NRF_MAX_VIEWS  # a second launch follows
    ctx = _context(desc)
    ctx.set_max_views(n)
    ctx.set_resolution(W, H)
    ctx.render_views(np.stack([cam] * n), np.stack(poses))
    batch = {v: ctx.read_view_f32(v) for v in (0, 127, 128, 129)}
    for v, (rgba, depth) in batch.items():
        ctx.render(cam, poses[v])
        one_rgba, one_depth = ctx.read_f32()
        assert one_rgba[..., 3].max() > 0  # the object is in the view
        assert np.array_equal(rgba.view(np.uint32), one_rgba.view(np.uint32)) and np.array_equal(depth.view(np.uint32), one_depth.view(np.uint32)), v
    ctx.close()


@pytest.mark.parametrize("env", [{"NRF_PERSISTENT": "1"}, {"NRF_PERSISTENT": "0"}])
def test_three_shards_of_101x77_untile_to_the_single_shard_frame(model, env):
    desc, keep, cfg = model
    W, H, world = 101, 77, 3
    cam, pose = syn.default_camera(W, H), syn.orbit_pose(30, 30)

    def render(shard):
        ctx = _context(desc, env, shard)
        ctx.set_resolution(W, H)
        n_px = nh.tiles_per_shard(W, H, world) * 64 if shard[1] > 1 else W * H
        rgba = torch.full((n_px, 4), 7.0, device="cuda")
        depth = torch.full((n_px, 1), 7.0, device="cuda")
        torch.cuda.synchronize()
        ctx.bind_output(rgba.data_ptr(), depth.data_ptr())
        ctx.render(cam, pose)
        out = rgba.cpu().numpy(), depth.cpu().numpy()
        ctx.close()
        return out

    whole, whole_depth = render((0, 1))
    shards = [render((i, world)) for i in range(world)]
    rgba = nh.untile_numpy(np.stack([s[0] for s in shards]), W, H)
    depth = nh.untile_numpy(np.stack([s[1] for s in shards]), W, H)
    assert whole.reshape(H, W, 4)[..., 3].max() > 0
    assert np.array_equal(rgba.view(np.uint32), whole.reshape(H, W, 4).view(np.uint32))
    assert np.array_equal(depth.view(np.uint32), whole_depth.reshape(H, W, 1).view(np.uint32))
