"""nrf_rb_upscale_temporal and nrf_motion_vectors on the GPU: the history colour, its weight, the presented plane and the packed dwords
against tests/temporal_replay.py of the read-back surfaces, bit for bit -- 96 x 64 spans 2 x 5 tiles of temporal_kernel (a tile is 62 x 14
output pixels), so apron and tile edges are covered, 53 x 41 covers ragged tiles --, all four kernel instances, both stream rules, every
state and return code, the motion vectors of rays from nrf_generate_rays, one end-to-end leg on a rendered NeRF frame, and
`testbed --upscale_temporal`."""
import ctypes as C

import numpy as np
import pytest

import nerfhip as nh
import temporal_replay as tr
import test_upscale_cpu as ucpu
import test_upscale_gpu as ugpu
import upscale_replay as ur
from test_temporal_cpu import CASES, RUNS, _frames, _motion_plane

pytestmark = pytest.mark.gpu
F = np.float32


def _device(array):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(array)).cuda()
    torch.cuda.synchronize()
    return t


def _step(rb, T, plane, jitter, flags, motion, pack, stream=None):
    """one nrf_rb_upscale_temporal of the presented `plane` against one step of the replay T, every plane bit for bit"""
    import torch
    surface = ugpu._present(rb, plane)
    ow, oh = T.ow, T.oh
    rgba8 = torch.full((oh, ow), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if pack else None
    dev_motion = _device(motion) if motion is not None else None
    torch.cuda.synchronize()
    rb.upscale_temporal(jitter, motion=dev_motion.data_ptr() if motion is not None else None, flags=flags,
                        rgba8=rgba8.data_ptr() if pack else None, stream=stream)
    if stream:
        torch.cuda.synchronize()
    want, packed = T.step(surface, jitter, motion, flags)
    shown = rb.read_upscaled()
    H, Wt = rb.read_upscale_history()
    for name, got, ref in (("H'", H, T.H), ("Wt'", Wt, T.Wt), ("presented", shown, want)):
        bad = np.nonzero(ur.bits(got) != ur.bits(ref))
        assert len(bad[0]) == 0, (surface.shape, (ow, oh), name, flags, len(bad[0]), [b[:5] for b in bad])
    if pack:
        assert np.array_equal(rgba8.cpu().numpy().view(np.uint32), packed), (surface.shape, (ow, oh), flags)
    assert rb.upscale_history()[2] == T.n_frames
    return shown


@pytest.mark.parametrize("case", CASES)
def test_the_temporal_upscale_is_the_replay_bit_for_bit(case):
    """three frames per run; the runs take the static and the motion instance, with and without the packed plane, the buffer's stream and
    a caller's"""
    import torch
    (iw, ih), (ow, oh) = case
    stream = torch.cuda.Stream()
    for k, (with_motion, flags) in enumerate(RUNS):
        amount, max_history = (0.0, 0.5, 2.0, 0.25)[k], (64.0, 1.0, 256.0, 2.5)[k]
        rb = nh.RenderBuffer(0)
        rb.resize(iw, ih)
        rb.enable_upscale(ow, oh)
        rb.set_upscale_sharpening(amount)
        rb.set_upscale_history(max_history)
        T = tr.Temporal(ow, oh, amount, max_history)
        for f, (plane, jitter, fl, motion) in enumerate(_frames(case, 700 + 31 * k + iw, with_motion, flags)):
            _step(rb, T, plane, jitter, fl, motion, pack=(k + f) % 2 == 0, stream=stream.cuda_stream if k % 2 else None)
        rb.close()


def test_a_frame_without_jitter_on_a_fresh_buffer_is_nrf_rb_upscale():
    (iw, ih), (ow, oh) = (48, 32), (96, 64)
    rb = nh.RenderBuffer(0)
    rb.resize(iw, ih)
    rb.enable_upscale(ow, oh)
    rb.set_upscale_sharpening(0.5)
    ugpu._present(rb, ucpu._plane(77, iw, ih))
    rb.upscale()
    spatial = rb.read_upscaled()
    ugpu._upload(rb.upscaled_ptr(), np.full((oh, ow, 4), np.nan, np.float32))
    rb.upscale_temporal((0.0, 0.0))
    assert np.array_equal(ur.bits(rb.read_upscaled()), ur.bits(spatial))
    # nrf_rb_upscale between two temporal calls overwrites the presented plane only
    H, Wt = rb.read_upscale_history()
    rb.upscale()
    H2, Wt2 = rb.read_upscale_history()
    assert np.array_equal(ur.bits(H), ur.bits(H2)) and np.array_equal(ur.bits(Wt), ur.bits(Wt2)) and rb.upscale_history()[2] == 1
    rb.close()


def _code(call, *args, **kw):
    with pytest.raises(nh.NerfHipError) as e:
        call(*args, **kw)
    return e.value.code


def test_states_and_errors():
    pytest.importorskip("torch")
    (iw, ih), (ow, oh) = (19, 11), (38, 22)
    rb = nh.RenderBuffer(0)
    rb.resize(iw, ih)
    for call in (lambda: rb.upscale_temporal((0.0, 0.0)), rb.upscale_history, rb.read_upscale_history):   # before an enable
        assert _code(call) == nh.NRF_E_STATE
    rb.enable_upscale(ow, oh)
    assert rb.upscale_history() == (None, None, 0)                                # nothing is allocated before the first call
    assert _code(rb.read_upscale_history) == nh.NRF_E_STATE
    for bad in (0.5, 256.5, -1.0, float("nan"), float("inf")):
        assert _code(rb.set_upscale_history, bad) == nh.NRF_E_INVALID, bad
    rb.set_upscale_history(1.0)
    rb.set_upscale_history(256.0)
    rb.set_upscale_history(64.0)
    T = tr.Temporal(ow, oh, 0.0)
    planes = [ucpu._plane(60 + k, iw, ih) for k in range(6)]
    _step(rb, T, planes[0], tr.jitter(0), tr.RECTIFY, None, pack=True)           # the first call ever is a reset whatever the flags say
    hist, weight, n = rb.upscale_history()
    assert hist and weight and n == 1
    before = (rb.read_upscaled(), *rb.read_upscale_history())
    # refused calls write nothing: jitter, flags, reserved
    for jitter in ((0.51, 0.0), (0.0, -0.5001), (float("nan"), 0.0), (0.0, float("inf"))):
        assert _code(rb.upscale_temporal, jitter) == nh.NRF_E_INVALID, jitter
    assert _code(rb.upscale_temporal, (0.0, 0.0), flags=4) == nh.NRF_E_INVALID
    assert _code(rb.upscale_temporal, (0.0, 0.0), reserved=1) == nh.NRF_E_INVALID
    assert nh.load_library().nrf_rb_upscale_temporal(rb.h, None, None, None) == nh.NRF_E_INVALID
    after = (rb.read_upscaled(), *rb.read_upscale_history())
    assert all(np.array_equal(ur.bits(a), ur.bits(b)) for a, b in zip(before, after)) and rb.upscale_history()[2] == 1
    _step(rb, T, planes[1], (0.5, -0.5), 0, None, pack=False)                     # the limits of the jitter are valid
    assert rb.upscale_history()[2] == 2 and rb.upscale_history()[0] != hist       # the planes were swapped
    # nrf_rb_resize drops the history: the next call is a reset and n_frames restarts
    rb.resize(iw + 1, ih)
    assert rb.upscale_history() == (None, None, 0)
    T = tr.Temporal(ow, oh, 0.0)
    _step(rb, T, ucpu._plane(70, iw + 1, ih), tr.jitter(3), 0, None, pack=False)
    _step(rb, T, ucpu._plane(71, iw + 1, ih), tr.jitter(4), 0, None, pack=False)
    assert rb.upscale_history()[2] == 2
    # nrf_rb_enable_upscale with another resolution drops it as well
    rb.enable_upscale(ow + 3, oh + 2)
    assert rb.upscale_history() == (None, None, 0)
    T = tr.Temporal(ow + 3, oh + 2, 0.0)
    _step(rb, T, ucpu._plane(72, iw + 1, ih), tr.jitter(5), 0, _motion_plane(1, iw + 1, ih, ow + 3, oh + 2), pack=True)
    rb.disable_upscale()                                                          # frees the history
    for call in (lambda: rb.upscale_temporal((0.0, 0.0)), rb.upscale_history, rb.read_upscale_history):
        assert _code(call) == nh.NRF_E_STATE
    rb.close()


def _model():
    import models
    return models.build_model(log2_hashmap_size=12, H=32)


def test_the_motion_vectors_are_the_replays():
    import torch
    import synthetic as syn
    desc, keep, cfg = _model()
    W, H, OW, OH = 40, 30, 53, 41
    ctx = nh.NerfHip(0)
    ctx.load_model(desc)
    ctx.set_resolution(W, H)
    cam, pose = np.asarray(syn.default_camera(W, H), np.float32), np.asarray(syn.orbit_pose(20.0, 30), np.float32)
    prev_cam, prev_pose = cam + F([0.5, -0.5, 0.3, 0.2]), np.asarray(syn.orbit_pose(23.0, 31), np.float32)
    o, d = torch.empty((H, W, 3), device="cuda"), torch.empty((H, W, 3), device="cuda")
    ctx.generate_rays(cam - F([0, 0, 0.25, -0.125]), pose, o.data_ptr(), d.data_ptr(), None, None)   # the rays of a jittered frame
    rng = np.random.default_rng(4)
    rgba = rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)
    depth = (rgba[..., 3] * rng.uniform(0.2, 2.0, (H, W))).astype(np.float32)
    rgba[0, :4, 3] = F([0.0, np.nan, 0.25, 1.0])
    depth[1, :4] = F([np.inf, np.nan, -1.0, 0.0])
    out = torch.full((H, W, 2), 7.0, device="cuda")
    dev_rgba, dev_depth = _device(rgba), _device(depth)
    args = (o.data_ptr(), d.data_ptr(), dev_rgba.data_ptr(), dev_depth.data_ptr(), W, H, OW, OH, cam, pose, prev_cam, prev_pose)
    for stream in (None, torch.cuda.Stream().cuda_stream):
        out.fill_(7.0)
        torch.cuda.synchronize()
        ctx.motion_vectors(*args, out.data_ptr(), min_alpha=0.5, stream=stream)
        torch.cuda.synchronize()
        want = tr.motion_vectors(o.cpu().numpy(), d.cpu().numpy(), rgba[..., 3], depth, OW, OH, 0.5, tr.camera(pose, desc.scale, cam),
                                 tr.camera(prev_pose, desc.scale, prev_cam))
        bad = np.nonzero(ur.bits(out.cpu().numpy()) != ur.bits(want))
        assert len(bad[0]) == 0, (len(bad[0]), [b[:5] for b in bad])
        assert np.isfinite(want).all() and np.abs(want).max() > 0.5
    # identical cameras: exactly zero
    ctx.motion_vectors(*args[:8], cam, pose, cam, pose, out.data_ptr())
    assert not out.cpu().numpy().any()
    # refused: NULL planes, resolutions, min_alpha, reserved -- nothing written
    out.fill_(7.0)
    torch.cuda.synchronize()
    for k in range(4):
        assert _code(ctx.motion_vectors, *[None if i == k else a for i, a in enumerate(args)], out.data_ptr()) == nh.NRF_E_INVALID
    assert _code(ctx.motion_vectors, *args, None) == nh.NRF_E_INVALID
    for ow, oh in ((W - 1, OH), (OW, 8 * H + 1), (16385, OH)):
        assert _code(ctx.motion_vectors, *args[:6], ow, oh, *args[8:], out.data_ptr()) == nh.NRF_E_INVALID
    for min_alpha in (0.0, -0.5, 1.5, float("nan")):
        assert _code(ctx.motion_vectors, *args, out.data_ptr(), min_alpha=min_alpha) == nh.NRF_E_INVALID
    assert _code(ctx.motion_vectors, *args, out.data_ptr(), reserved=1) == nh.NRF_E_INVALID
    assert (out.cpu().numpy() == 7.0).all()
    ctx.close()


def test_the_motion_vectors_past_one_grid_stride_pass():
    """motion_kernel's launch is capped at 2048 x 256 lanes: 1023 x 513 = 524 799 render pixels take a second, ragged trip (511 pixels,
    no multiple of 256).  Bit for bit against the replay; the odd alphas and depths of the test above sit in the first trip and again
    beyond pixel 524 288; 64 rows after the plane stay as they were."""
    import torch
    import synthetic as syn
    desc, keep, cfg = _model()
    W, H, OW, OH, GUARD = 1023, 513, 1300, 700, 64
    assert W * H > 2048 * 256 and (W * H) % 256 != 0
    ctx = nh.NerfHip(0)
    ctx.load_model(desc)
    ctx.set_resolution(W, H)
    cam, pose = np.asarray(syn.default_camera(W, H), np.float32), np.asarray(syn.orbit_pose(20.0, 30), np.float32)
    prev_cam, prev_pose = cam + F([0.5, -0.5, 0.3, 0.2]), np.asarray(syn.orbit_pose(23.0, 31), np.float32)
    o, d = torch.empty((H, W, 3), device="cuda"), torch.empty((H, W, 3), device="cuda")
    ctx.generate_rays(cam - F([0, 0, 0.25, -0.125]), pose, o.data_ptr(), d.data_ptr(), None, None)
    rng = np.random.default_rng(40)
    rgba = rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)
    depth = (rgba[..., 3] * rng.uniform(0.2, 2.0, (H, W))).astype(np.float32)
    for row, col in ((0, 0), (H - 1, 600)):
        assert row * W + col + 10 <= 2048 * 256 if row == 0 else row * W + col > 2048 * 256
        rgba[row, col:col + 4, 3] = F([0.0, np.nan, 0.25, 1.0])
        depth[row, col + 4:col + 8] = F([np.inf, np.nan, -1.0, 0.0])
        rgba[row, col + 8:col + 10, 3] = F([0.5, np.nextafter(F(0.5), F(0))])  # the two sides of min_alpha
    sentinel = F(-77.25)
    out = torch.full((H + GUARD, W, 2), float(sentinel), device="cuda")
    dev_rgba, dev_depth = _device(rgba), _device(depth)
    torch.cuda.synchronize()
    ctx.motion_vectors(o.data_ptr(), d.data_ptr(), dev_rgba.data_ptr(), dev_depth.data_ptr(), W, H, OW, OH, cam, pose, prev_cam, prev_pose,
                       out.data_ptr(), min_alpha=0.5)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = tr.motion_vectors(o.cpu().numpy(), d.cpu().numpy(), rgba[..., 3], depth, OW, OH, 0.5, tr.camera(pose, desc.scale, cam),
                             tr.camera(prev_pose, desc.scale, prev_cam))
    assert want.shape == (H, W, 2)
    bad = np.nonzero(ur.bits(got[:H]) != ur.bits(want))
    assert len(bad[0]) == 0, (len(bad[0]), [b[:5] for b in bad])
    assert np.all(ur.bits(got[H:]) == ur.bits(np.full(1, sentinel, np.float32))[0])
    assert not np.any(ur.bits(want) == ur.bits(np.full(1, sentinel, np.float32))[0])  # every pixel of the plane was written
    second = want.reshape(-1, 2)[2048 * 256:]
    assert len(second) == 511 and np.isfinite(second).all() and np.abs(second).max() > 0.5
    ctx.close()


def test_eight_jittered_frames_of_a_model_come_closer_to_the_full_resolution_render():
    """Render 48 x 32 with 8 jittered cameras, present, accumulate to 96 x 64: closer (PSNR) to a direct 96 x 64 render of the same view than
    nrf_rb_upscale of the unjittered frame is.  A relative condition; both values are printed."""
    import synthetic as syn
    pytest.importorskip("torch")
    desc, keep, cfg = _model()
    W, H = 48, 32
    cam, pose = np.asarray(syn.default_camera(W, H), np.float32), syn.orbit_pose(20.0, 30)
    ctx = nh.NerfHip(0)
    ctx.load_model(desc)

    def develop(rb, w, h, camera):
        ctx.set_resolution(w, h)
        frame_p, depth_p, _, _ = rb.buffers()
        ctx.bind_output(frame_p, depth_p)
        rb.clear_frame()
        ctx.render(camera, pose)
        rb.reset_accumulation()
        rb.present(0.0, [1, 1, 1, 1], nh.CS_SRGB)

    full = nh.RenderBuffer(0)
    full.resize(2 * W, 2 * H)
    full.set_tonemap_curve(nh.TM_ACES)
    develop(full, 2 * W, 2 * H, cam * F(2.0))
    truth = full.read()[1]
    assert truth.std() > 0.01                                                    # a picture, not a flat plane
    rb = nh.RenderBuffer(0)
    rb.resize(W, H)
    rb.set_tonemap_curve(nh.TM_ACES)
    rb.enable_upscale(2 * W, 2 * H)
    for k in range(8):
        j = (F(0), F(0)) if k == 0 else tr.jitter(k)
        develop(rb, W, H, cam - F([0, 0, j[0], j[1]]))
        if k == 0:
            rb.upscale()
            spatial = rb.read_upscaled()
        rb.upscale_temporal(j, reset=k == 0)
    temporal = rb.read_upscaled()
    assert rb.upscale_history()[2] == 8
    got, base = ucpu._psnr(temporal, truth), ucpu._psnr(spatial, truth)
    print(f"{W} x {H} -> {2 * W} x {2 * H} on a rendered model: temporal over 8 frames {got:.2f} dB, spatial {base:.2f} dB (+{got - base:.2f})")
    ctx.bind_output(None, None)
    ctx.close()
    rb.close()
    full.close()
    assert got > base, (got, base)


def test_testbed_accumulates_jittered_frames(tmp_path):
    """`testbed --upscale 2 --upscale_temporal 4` writes an upscaled.png of the output size that differs from the `--upscale 2` one"""
    import subprocess
    from pathlib import Path

    import synthetic as syn
    import test_mesh_texture_cpu as tcpu
    host = Path(nh.LIB_PATH).parent / "host"
    if not (host / "testbed").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, keep, cfg = _model()
    snap = tmp_path / "tiny.msgpack"
    syn.write_snapshot(snap, cfg, keep[0], keep[1])
    W, H = 60, 44
    pictures = []
    for name, extra in (("spatial", []), ("temporal", ["--upscale_temporal", "4"])):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([str(host / "testbed"), str(snap), str(W), str(H), str(out) + "/", "--upscale", "2", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr + r.stdout
        assert f"upscale: {W} x {H} -> {2 * W} x {2 * H}, sharpening 0" in r.stdout, r.stdout
        assert ("temporal over 4 frames" in r.stdout) == bool(extra), r.stdout
        pictures.append(tcpu.parse_png((out / "upscaled.png").read_bytes()))
    assert pictures[0].shape == pictures[1].shape == (2 * H, 2 * W, 3)
    assert not np.array_equal(pictures[0], pictures[1]) and pictures[1].std() > 1
    assert np.abs(pictures[0].astype(int) - pictures[1].astype(int)).mean() < 8   # the same view
