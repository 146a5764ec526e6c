"""nrf_rb_upscale on the GPU: the upscaled plane and the packed dwords against tests/upscale_replay.py of the read-back surface, bit for
bit -- every tile edge case of upscale_kernel (a tile is 62 x 14 output pixels, one workgroup per tile: a plane smaller than a tile,
partial tiles, exact multiples, several tiles per axis), the surface as nrf_rb_present and nrf_rb_overlay_depth leave it, every return
code of the calls, both stream rules, `testbed --upscale`, and one frame rendered by nrf_render into the buffer and upscaled."""
import ctypes as C

import numpy as np
import pytest

import nerfhip as nh
import upscale_replay as ur

pytestmark = pytest.mark.gpu
AMOUNTS = (0.0, 0.5, 2.0)
TILE_W, TILE_H = 62, 14  # UPS_TILE_W, UPS_TILE_H of nrf_kernels_upscale.hip


def _upload(dst, array):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(array)).cuda()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    torch.cuda.synchronize()
    assert hip.hipMemcpy(dst, t.data_ptr(), array.nbytes, 3) == 0
    torch.cuda.synchronize()


def _plane(seed, w, h):
    """random finite texels, some negative and some above 1"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 1.5, (h, w, 4)).astype(np.float32)
    p[rng.random((h, w, 4)) < 0.1] *= np.float32(3.0)
    p[0, 0, :2] = np.float32([-0.25, 1.75])
    return p


def _present(rb, plane):
    """the plane through the frame plane and nrf_rb_present (identity curve, linear, nothing behind it) -> the surface read back"""
    frame_p = rb.buffers()[0]
    _upload(frame_p, plane)
    rb.reset_accumulation()
    rb.present(0.0, [0.0, 0.0, 0.0, 0.0], nh.CS_LINEAR)
    return rb.read()[1]


def _hold(rb, surface, ow, oh, amount, stream=None):
    """one nrf_rb_upscale with the packed plane against the replay of `surface`, bit for bit"""
    import torch
    rgba8 = torch.full((oh, ow), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rb.set_upscale_sharpening(amount)
    rb.upscale(rgba8.data_ptr(), stream)
    if stream:
        torch.cuda.synchronize()
    got = rb.read_upscaled()
    want, packed = ur.upscale(surface, ow, oh, amount)
    bad = np.nonzero(np.any(ur.bits(got) != ur.bits(want), axis=2))
    assert len(bad[0]) == 0, (surface.shape, (ow, oh), amount, len(bad[0]), bad[0][:5], bad[1][:5])
    assert np.array_equal(rgba8.cpu().numpy().view(np.uint32), packed), (surface.shape, (ow, oh), amount)
    return got


# (source, target).  The issue's rows: ratio 2; ratio 2, wider than a tile; non-integer ratios; identity; ratio 4 (exactly two tiles
# high); a single texel (a plane smaller than a tile); ratio 8 on one axis (three tiles high, the last one partial).  Then the tiles:
# exact multiples of the tile on both axes; one pixel into the second tile on both axes; identity over 3 x 3 tiles, where a tile's
# source footprint is at its largest (68 x 20); a ratio just above 1 over 3 x 3 tiles
ROWS = [((19, 11), (38, 22)), ((45, 13), (90, 26)), ((23, 9), (37, 17)), ((33, 17), (33, 17)), ((13, 7), (52, 28)), ((1, 1), (4, 4)),
        ((5, 40), (40, 40)),
        ((62, 14), (2 * TILE_W, 2 * TILE_H)), ((21, 5), (TILE_W + 1, TILE_H + 1)), ((130, 31), (130, 31)), ((125, 29), (126, 30))]


@pytest.mark.parametrize("src,dst", ROWS)
def test_the_upscale_is_the_replay_of_the_surface_bit_for_bit(src, dst):
    pytest.importorskip("torch")
    rb = nh.RenderBuffer(0)
    rb.resize(*src)
    rb.enable_upscale(*dst)
    assert rb.resolutions() == (src, dst)
    assert not rb.read_upscaled().any()                          # zero-filled
    surface = _present(rb, _plane(src[0] * 100 + dst[1], *src))
    assert (surface < 0).any() and (surface > 1).any()
    for amount in AMOUNTS:
        _hold(rb, surface, dst[0], dst[1], amount)
    rb.upscale()                                                 # without the packed plane: the same float plane
    assert np.array_equal(ur.bits(rb.read_upscaled()), ur.bits(ur.upscale(surface, dst[0], dst[1], AMOUNTS[-1])[0]))
    rb.close()


def test_the_surface_is_read_as_an_overlay_left_it():
    import torch
    W, H, iw, ih = 45, 13, 40, 30
    rb = nh.RenderBuffer(0)
    rb.resize(W, H)
    rb.enable_upscale(90, 26)
    developed = _present(rb, _plane(5, W, H))
    depth = torch.from_numpy(np.random.default_rng(6).random((ih, iw), dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    rb.overlay_depth(0.35, depth.data_ptr(), 0.9, iw, ih, 1, 1.7, (0.42, 0.61))
    surface = rb.read()[1]
    assert not np.array_equal(surface, developed)
    got = _hold(rb, surface, 90, 26, 0.5)
    assert not np.array_equal(got, ur.upscale(developed, 90, 26, 0.5)[0])
    rb.close()


def _code(call, *args):
    with pytest.raises(nh.NerfHipError) as e:
        call(*args)
    return e.value.code


def test_states_and_errors():
    pytest.importorskip("torch")
    rb = nh.RenderBuffer(0)
    assert _code(rb.enable_upscale, 8, 8) == nh.NRF_E_STATE                      # needs a resized buffer
    W, H = 19, 11
    rb.resize(W, H)
    assert rb.resolutions() == ((W, H), (W, H))                                  # out == in while disabled
    for call in (rb.upscale, rb.upscaled_ptr, rb.read_upscaled):                 # before an enable
        assert _code(call) == nh.NRF_E_STATE
    rb.enable_upscale(38, 22)
    plane = rb.upscaled_ptr()
    assert plane and rb.resolutions() == ((W, H), (38, 22))
    # a bad output resolution changes nothing: below the source, beyond 8 x, beyond 16384 (8 x 2100 = 16800 would allow it)
    for ow, oh in [(18, 22), (38, 10), (8 * W + 1, 22), (38, 8 * H + 1), (0, 0), (-38, 22)]:
        assert _code(rb.enable_upscale, ow, oh) == nh.NRF_E_INVALID, (ow, oh)
        assert rb.resolutions() == ((W, H), (38, 22)) and rb.upscaled_ptr() == plane
    wide = nh.RenderBuffer(0)
    wide.resize(2100, 1)
    assert _code(wide.enable_upscale, 16385, 1) == nh.NRF_E_INVALID
    wide.enable_upscale(16384, 1)
    wide.close()
    # the amount
    for amount in (-0.25, 2.5, float("nan"), float("inf")):
        assert _code(rb.set_upscale_sharpening, amount) == nh.NRF_E_INVALID, amount
    # an upscale leaves the resolutions, spp, the surface and the accumulate plane alone
    surface = _present(rb, _plane(9, W, H))
    acc_before, sur_before = rb.read()
    assert rb.spp() == 1
    _hold(rb, surface, 38, 22, 0.5)
    acc_after, sur_after = rb.read()
    assert rb.spp() == 1 and rb.resolutions() == ((W, H), (38, 22))
    assert np.array_equal(ur.bits(acc_before), ur.bits(acc_after)) and np.array_equal(ur.bits(sur_before), ur.bits(sur_after))
    # a resize that does not fit the enabled output resolution: refused, and the buffer is as it was
    for w, h in [(39, 11), (19, 23), (4, 11), (19, 2)]:
        assert _code(rb.resize, w, h) == nh.NRF_E_INVALID, (w, h)
        assert rb.resolutions() == ((W, H), (38, 22)) and rb.spp() == 1
        assert np.array_equal(ur.bits(rb.read()[1]), ur.bits(sur_before))
    rb.resize(38, 22)                                                            # one that fits: out stays, everything is zero-filled
    assert rb.resolutions() == ((38, 22), (38, 22)) and rb.spp() == 0 and not rb.read_upscaled().any()
    rb.enable_upscale(40, 25)                                                    # again: replaces the output resolution
    assert rb.resolutions() == ((38, 22), (40, 25)) and rb.read_upscaled().shape == (25, 40, 4)
    rb.disable_upscale()
    assert rb.resolutions() == ((38, 22), (38, 22))
    for call in (rb.upscale, rb.upscaled_ptr, rb.read_upscaled):                 # after a disable
        assert _code(call) == nh.NRF_E_STATE
    rb.resize(200, 3)                                                            # as before the feature: any size
    assert rb.resolutions() == ((200, 3), (200, 3))
    rb.disable_upscale()                                                         # twice is fine
    rb.close()


def test_a_callers_stream_and_the_buffers_own_give_the_same_bits():
    import torch
    src, dst = (45, 13), (90, 26)
    rb = nh.RenderBuffer(0)
    rb.resize(*src)
    rb.enable_upscale(*dst)
    surface = _present(rb, _plane(21, *src))
    own = _hold(rb, surface, dst[0], dst[1], 0.5)
    _upload(rb.upscaled_ptr(), np.full((dst[1], dst[0], 4), np.nan, np.float32))
    stream = torch.cuda.Stream()
    theirs = _hold(rb, surface, dst[0], dst[1], 0.5, stream=stream.cuda_stream)
    assert np.array_equal(ur.bits(own), ur.bits(theirs))
    rb.close()


def test_testbed_writes_the_upscaled_picture(tmp_path):
    """`testbed --upscale S --upscale_sharpening A`: after tonemapped.png the same render buffer upscales its surface and upscaled.png
    is written -- the replay of that surface, quantised as testbed quantises; without the flag there is no such file"""
    import subprocess
    from pathlib import Path

    import models
    import synthetic as syn
    import test_mesh_texture_cpu as tcpu
    host = Path(nh.LIB_PATH).parent / "host"
    if not (host / "testbed").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, H=32)
    snap = tmp_path / "tiny.msgpack"
    syn.write_snapshot(snap, cfg, keep[0], keep[1])
    W, H, OW, OH = 60, 44, 90, 66
    r = subprocess.run([str(host / "testbed"), str(snap), str(W), str(H), str(tmp_path) + "/", "--upscale", "1.5", "--upscale_sharpening", "0.25"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert f"upscale: {W} x {H} -> {OW} x {OH}, sharpening 0.25, device time" in r.stdout, r.stdout
    got = tcpu.parse_png((tmp_path / "upscaled.png").read_bytes())
    assert got.shape == (OH, OW, 3)
    rb = nh.RenderBuffer(0)                                                      # testbed's chain: u8 image -> accumulate -> tonemap (sRGB)
    rb.resize(W, H)
    rb.host_to_accumulate_buffer(np.fromfile(tmp_path / "image.rgb", np.uint8))
    rb.tonemap(0.0, [0.0, 0.0, 0.0, 1.0], nh.CS_SRGB)
    want, _ = ur.upscale(rb.read()[1], OW, OH, 0.25)
    rb.close()
    scaled = want[:, :, :3] * np.float32(255)
    assert np.array_equal(got, np.clip(scaled, 0, 255).astype(np.uint8))
    assert got.std() > 1                                                         # a picture
    plain = tmp_path / "plain"
    plain.mkdir()
    r = subprocess.run([str(host / "testbed"), str(snap), str(W), str(H), str(plain) + "/"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "upscale" not in r.stdout
    assert (plain / "tonemapped.png").exists() and not (plain / "upscaled.png").exists()


def test_a_rendered_frame_is_upscaled_on_the_device():
    """nrf_render into the buffer's frame plane, nrf_rb_present, nrf_rb_upscale to twice the resolution: the replay of the surface"""
    import models
    import synthetic as syn
    pytest.importorskip("torch")
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, H=32)
    W, H = 48, 32
    ctx = nh.NerfHip(0)
    ctx.load_model(desc)
    ctx.set_resolution(W, H)
    rb = nh.RenderBuffer(0)
    rb.resize(W, H)
    rb.set_tonemap_curve(nh.TM_ACES)
    rb.enable_upscale(2 * W, 2 * H)
    frame_p, depth_p, _, _ = rb.buffers()
    ctx.bind_output(frame_p, depth_p)
    rb.clear_frame()
    ctx.render(syn.default_camera(W, H), syn.orbit_pose(20.0, 30))
    rb.present(0.0, [1, 1, 1, 1], nh.CS_SRGB)
    surface = rb.read()[1]
    assert surface.std() > 0.01                                                  # a picture, not a flat plane
    for amount in (0.0, 0.5):
        _hold(rb, surface, 2 * W, 2 * H, amount)
    ctx.bind_output(None, None)
    ctx.close()
    rb.close()
