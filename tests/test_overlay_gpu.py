"""nrf_rb_overlay_image / nrf_rb_overlay_false_color / nrf_rb_error_map on the GPU against tests/overlay_replay.py of the read-back
surface: the row families of tests/test_overlay_cpu.py through nh.RenderBuffer -- bit for bit wherever the device evaluates no power
(render space Linear or VisPosNeg, display Linear, integer exposures: all four curves, every image data type, Byte included thanks to
the table, both colour maps, the whole error map and its average), at tests/test_render_buffer.py::test_hip_matches_oracle's tolerances
(rtol 2e-5, atol 2e-6) through pow_positive and at the non-integer exposure, there on finite inputs in [0, 4] --, a surface of 257 x 3
(a second workgroup with a partial tail) and one of 1031 x 521 (more pixels than the 2048 x 256 lanes of the overlays' grid: the
grid-stride loop makes a second trip; its error map at 512 x 512 cells and as one cell of 537 151 pixels), the chains with present, the
upscaler and the device buffers of the error map, every return code, and `testbed --overlay_image / --compare`.

"Bit for bit" lets a NaN match any NaN (overlay_replay.same)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import nerfhip as nh
import overlay_replay as orp
import test_overlay_cpu as ocpu

pytestmark = pytest.mark.gpu
F = np.float32
RTOL, ATOL = 2e-5, 2e-6  # test_render_buffer.py::test_hip_matches_oracle's, for the surface
BIG = (1031, 521)        # > 2048 * 256 pixels


def dev(array):
    """a device copy (a torch tensor: keep it alive) of a numpy array of any 16-, 32-bit type"""
    import torch
    a = np.ascontiguousarray(array)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint16:
        a = a.view(np.int16)
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t


def host(t, dtype=np.float32):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)


def set_surface(rb, plane):
    t = dev(plane)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(rb.buffers()[3], t.data_ptr(), plane.nbytes, 3) == 0
    import torch
    torch.cuda.synchronize()


def finite(plane):
    """finite values in [0, 4]"""
    return np.clip(np.nan_to_num(np.asarray(plane, np.float32), nan=0.5, posinf=4.0, neginf=0.0), 0.0, 4.0).astype(np.float32)


def exact_row(rs, ds, exposure):
    return rs != nh.CS_SRGB and ds == nh.CS_LINEAR and all(float(e).is_integer() for e in np.atleast_1d(exposure))


def hold_image(rb, table, surface, image, ty, axis, zoom, center, alpha, rs, ds, curve, exposure, bg, stream=None):
    """one nrf_rb_overlay_image over `surface` against the replay; returns the surface read back"""
    exact = exact_row(rs, ds, exposure)
    if not exact:
        surface = finite(surface)
        if ty == nh.IMG_FLOAT:
            image = finite(image)
        elif ty == nh.IMG_HALF:
            image = finite(image.view(np.float16).astype(np.float32)).astype(np.float16).view(np.uint16)
    rb.set_color_space(rs)
    rb.set_tonemap_curve(curve)
    set_surface(rb, surface)
    t = dev(image)
    ih, iw = image.shape[:2]
    rb.overlay_image(alpha, exposure, bg, ds, t.data_ptr(), ty, iw, ih, axis, zoom, center, stream)
    if stream:
        import torch
        torch.cuda.synchronize()
    got = rb.read()[1]
    want = orp.overlay_image(surface, alpha, exposure, bg, rs, ds, curve, image, ty, table, axis, zoom, center)
    what = (surface.shape, (iw, ih), ty, axis, zoom, center, alpha, rs, ds, curve, exposure)
    if exact:
        bad = orp.mismatches(got, want)
        assert len(bad) == 0, (what, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    else:
        assert np.isfinite(want).all(), what
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=str(what))
    return got


@pytest.fixture(scope="module")
def table():
    pytest.importorskip("torch")  # (before the library is loaded: torch brings a HIP runtime of its own, and the first one loaded serves both)
    return nh.srgb8_table()


# ---------------------------------------------------------------- the image overlay
@pytest.mark.parametrize("ty", ocpu.TYPES)
@pytest.mark.parametrize("surf", ocpu.SURFACES)
def test_the_image_overlay_is_the_replay_of_the_surface(table, surf, ty):
    pytest.importorskip("torch")
    rows = [(k, r) for k, r in enumerate(ocpu._image_rows()) if r[0] == surf and r[2] == ty]
    assert len(rows) >= 90
    rb = nh.RenderBuffer(0)
    rb.resize(*surf)
    exact = 0
    for k, row in rows:
        _, img, _, axis, zoom, center, alpha, (rs, ds), curve, exposure = row
        s, im, bg = ocpu._image_inputs(k, row)
        hold_image(rb, table, s, im, ty, axis, zoom, center, alpha, rs, ds, curve, exposure, bg)
        exact += exact_row(rs, ds, exposure)
    assert exact >= 10 and exact < len(rows)
    rb.close()


@pytest.mark.parametrize("ty", ocpu.TYPES)
def test_the_image_overlay_on_a_second_workgroup_with_a_partial_tail(table, ty):
    pytest.importorskip("torch")
    W, H = 257, 3
    rb = nh.RenderBuffer(0)
    rb.resize(W, H)
    for k, (img, axis, zoom, center, (rs, ds), curve) in enumerate([((40, 23), 0, 1.0, (0.5, 0.5), (0, 0), 1), ((7, 5), 1, 0.5, (0.1, 0.9), (2, 0), 3),
                                                                   ((300, 2), 0, -1.0, (0.5, 0.5), (1, 1), 2), ((1, 1), 1, 3.0, (0.5, 0.5), (0, 1), 0)]):
        hold_image(rb, table, ocpu.surface_plane(7000 + k, W, H), ocpu.image_plane(7100 + k, img[0], img[1], ty), ty, axis, zoom, center, 0.25,
                   rs, ds, curve, (1.0, -1.0, 2.0), (0.9, 0.1, 0.3, 0.5))
    rb.close()


def test_the_overlays_grid_stride_loop_makes_a_second_trip(table):
    """1031 x 521 = 537 151 pixels on 2048 x 256 lanes: the image overlay (Byte, Reinhard, bit for bit) and the false colours"""
    pytest.importorskip("torch")
    W, H = BIG
    assert W * H > 2048 * 256
    rb = nh.RenderBuffer(0)
    rb.resize(W, H)
    s = ocpu.surface_plane(7200, W, H)
    hold_image(rb, table, s, ocpu.image_plane(7201, 640, 360, nh.IMG_BYTE), nh.IMG_BYTE, 1, 1.25, (0.45, 0.55), 0.25, nh.CS_LINEAR, nh.CS_LINEAR,
               nh.TM_REINHARD, (1.0, 0.0, -1.0), (0.25, 0.5, 1.0, 1.0))
    emap = np.random.default_rng(7202).uniform(0.0, 0.5, (16, 16)).astype(np.float32)
    hold_false_color(rb, s, W, H, 0, emap, 0.2, 1.0, 1)
    rb.close()


# ---------------------------------------------------------------- the false colours
def hold_false_color(rb, surface, tw, th, axis, emap, average, brightness, viridis, stream=None):
    set_surface(rb, surface)
    m, a = dev(emap), dev(F([average]))
    mh, mw = emap.shape
    rb.overlay_false_color(tw, th, axis, m.data_ptr(), mw, mh, a.data_ptr(), brightness, viridis, stream)
    if stream:
        import torch
        torch.cuda.synchronize()
    got = rb.read()[1]
    want = orp.overlay_false_color(surface, tw, th, axis, emap, average, brightness, viridis)
    bad = orp.mismatches(got, want)
    assert len(bad) == 0, (surface.shape, (tw, th), emap.shape, axis, average, brightness, viridis, len(bad), bad[:5])
    return got


@pytest.mark.parametrize("surf", ocpu.SURFACES + [(257, 3)])
def test_the_false_colours_are_the_replay_of_the_surface_bit_for_bit(surf):
    pytest.importorskip("torch")
    rb = nh.RenderBuffer(0)
    rb.resize(*surf)
    rows = [(k, r) for k, r in enumerate(ocpu._false_color_rows()) if r[0] == surf]
    if not rows:  # 257 x 3: both maps, both axes, a map wider than it is high
        rows = [(900 + k, (surf, (tw, th), (mw, mh), axis, viridis, [0.0, np.nan, 0.05, 0.3][k % 4], [0.0, 16.0, 1.0][k % 3]))
                for k, ((tw, th), (mw, mh), axis, viridis) in enumerate(itertools.product([(257, 3), (128, 1), (385, 4)], [(16, 16), (3, 2)], (0, 1), (0, 1)))]
    for k, row in rows:
        _, (tw, th), _, axis, viridis, average, brightness = row
        s, emap = ocpu._false_color_inputs(k, row)
        hold_false_color(rb, s, tw, th, axis, emap, average, brightness, viridis)
    rb.close()


# ---------------------------------------------------------------- the error map
def hold_error_map(rb, surface, truth, mw, mh, stream=None):
    import torch
    set_surface(rb, surface)
    g = dev(truth)
    m = torch.full((mh, mw), float("nan"), dtype=torch.float32, device="cuda")
    a = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rb.error_map(g.data_ptr(), mw, mh, m.data_ptr(), a.data_ptr(), stream)
    got, got_average = host(m), host(a)[0]
    want, want_average = orp.error_map(surface, truth, mw, mh)
    bad = orp.mismatches(got, want)
    assert len(bad) == 0, (surface.shape, mw, mh, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert orp.same(got_average, want_average), (surface.shape, mw, mh, got_average, want_average)
    return got, got_average, m, a


def test_the_error_map_is_the_replay_bit_for_bit():
    pytest.importorskip("torch")
    for s, g, mw, mh, what in ocpu._error_inputs():
        rb = nh.RenderBuffer(0)
        rb.resize(s.shape[1], s.shape[0])
        got, average, _, _ = hold_error_map(rb, s, g, mw, mh)
        if what == "one NaN":
            assert np.isnan(got).sum() == 1 and np.isnan(average)
        if what == "identical":
            assert not orp.bits(got).any() and orp.bits(average) == 0
        rb.close()


@pytest.mark.parametrize("cells", [(512, 512), (1, 1)])
def test_the_error_map_of_a_large_plane(cells):
    """1031 x 521 -> 512 x 512: cells of 2 or 3 by 1 or 2 pixels, 65 536 workgroups; -> 1 x 1: one wave over 537 151 pixels, 8 393 or 8 392
    additions per lane in a fixed order"""
    pytest.importorskip("torch")
    W, H = BIG
    rng = np.random.default_rng(7300)
    s, g = rng.uniform(0, 1, (H, W, 4)).astype(np.float32), rng.uniform(0, 1, (H, W, 4)).astype(np.float32)
    rb = nh.RenderBuffer(0)
    rb.resize(W, H)
    got, average, _, _ = hold_error_map(rb, s, g, *cells)
    mse = np.mean((s[..., :3].astype(np.float64) - g[..., :3]) ** 2)
    assert abs(float(average) - mse) <= 1e-3 * mse  # (the mean of the cell means of nearly equal cells; fp32 sums)
    rb.close()


# ---------------------------------------------------------------- chains
def test_present_then_the_image_overlay_then_the_upscaler_reads_the_overlaid_surface(table):
    import upscale_replay as ur
    pytest.importorskip("torch")
    W, H = 45, 13
    rb = nh.RenderBuffer(0)
    rb.resize(W, H)
    rb.enable_upscale(90, 26)
    rb.set_upscale_sharpening(0.5)
    frame = np.random.default_rng(7400).uniform(0, 1.5, (H, W, 4)).astype(np.float32)
    t = dev(frame)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(rb.buffers()[0], t.data_ptr(), frame.nbytes, 3) == 0
    rb.reset_accumulation()
    rb.set_tonemap_curve(nh.TM_ACES)
    rb.present(0.0, [0.0, 0.0, 0.0, 1.0], nh.CS_LINEAR)
    developed = rb.read()[1]
    image = finite(ocpu.image_plane(7401, 40, 23, nh.IMG_FLOAT)).astype(np.float16).view(np.uint16)
    im = dev(image)
    rb.overlay_image(0.35, (1.0, 0.0, -1.0), (0.2, 0.4, 0.6, 1.0), nh.CS_LINEAR, im.data_ptr(), nh.IMG_HALF, 40, 23, 1, 1.7, (0.42, 0.61))
    surface = rb.read()[1]
    want = orp.overlay_image(developed, 0.35, (1.0, 0.0, -1.0), (0.2, 0.4, 0.6, 1.0), nh.CS_LINEAR, nh.CS_LINEAR, nh.TM_ACES, image, nh.IMG_HALF, table,
                             1, 1.7, (0.42, 0.61))
    assert np.array_equal(orp.bits(surface), orp.bits(want)) and not np.array_equal(orp.bits(surface), orp.bits(developed))
    rb.upscale()
    assert np.array_equal(ur.bits(rb.read_upscaled()), ur.bits(ur.upscale(surface, 90, 26, 0.5)[0]))
    rb.close()


def test_the_error_maps_device_buffers_feed_the_false_colours_on_both_kinds_of_stream():
    import torch
    W, H, mw, mh = 45, 13, 9, 4
    rng = np.random.default_rng(7500)
    s, g = rng.uniform(0, 1, (H, W, 4)).astype(np.float32), rng.uniform(0, 1, (H, W, 4)).astype(np.float32)
    emap, average = orp.error_map(s, g, mw, mh)
    want = orp.overlay_false_color(s, W, H, 0, emap, average, 1.0, 1)
    results = []
    for stream in (None, torch.cuda.Stream()):
        rb = nh.RenderBuffer(0)
        rb.resize(W, H)
        handle = stream.cuda_stream if stream else None
        _, _, m, a = hold_error_map(rb, s, g, mw, mh, handle)    # (leaves the surface as uploaded)
        rb.overlay_false_color(W, H, 0, m.data_ptr(), mw, mh, a.data_ptr(), 1.0, True, handle)   # the device buffers as they are
        torch.cuda.synchronize()
        results.append(rb.read()[1])
        assert orp.same(results[-1], want)
        rb.close()
    assert np.array_equal(orp.bits(results[0]), orp.bits(results[1]))


def test_the_error_map_of_a_surface_against_itself_is_all_plus_zero():
    import torch
    W, H = 45, 13
    rb = nh.RenderBuffer(0)
    rb.resize(W, H)
    set_surface(rb, finite(ocpu.surface_plane(7600, W, H)))
    m = torch.full((5, 7), float("nan"), dtype=torch.float32, device="cuda")
    a = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rb.error_map(rb.buffers()[3], 7, 5, m.data_ptr(), a.data_ptr())
    assert not host(m, np.uint32).any() and not host(a, np.uint32).any()
    rb.close()


# ---------------------------------------------------------------- return codes
def test_every_refusal_leaves_the_surface_and_the_outputs_alone():
    import torch
    lib = nh.load_library()
    fp = lambda *v: (C.c_float * len(v))(*v)  # noqa: E731
    W, H = 19, 11
    image = dev(ocpu.image_plane(7700, 7, 5, nh.IMG_FLOAT))
    truth = dev(np.zeros((H, W, 4), np.float32))
    m = torch.full((16, 16), 7.0, dtype=torch.float32, device="cuda")
    a = torch.full((1,), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def image_call(rb, **o):
        p = dict(alpha=0.5, exposure=fp(0, 0, 0), bg=fp(0, 0, 0, 1), ds=0, image=image.data_ptr(), ty=nh.IMG_FLOAT, iw=7, ih=5, axis=0, zoom=1.0,
                 center=fp(0.5, 0.5))
        p.update(o)
        return lib.nrf_rb_overlay_image(rb.h, p["alpha"], p["exposure"], p["bg"], p["ds"], p["image"], p["ty"], p["iw"], p["ih"], p["axis"],
                                        p["zoom"], p["center"], None)

    def false_color_call(rb, **o):
        p = dict(tw=W, th=H, axis=0, map=m.data_ptr(), mw=16, mh=16, average=a.data_ptr())
        p.update(o)
        return lib.nrf_rb_overlay_false_color(rb.h, p["tw"], p["th"], p["axis"], p["map"], p["mw"], p["mh"], p["average"], 1.0, 1, None)

    def error_call(rb, **o):
        p = dict(truth=truth.data_ptr(), mw=5, mh=3, map=m.data_ptr(), average=a.data_ptr())
        p.update(o)
        return lib.nrf_rb_error_map(rb.h, p["truth"], p["mw"], p["mh"], p["map"], p["average"], None)

    fresh = nh.RenderBuffer(0)                                   # before a resize
    assert image_call(fresh) == nh.NRF_E_STATE and false_color_call(fresh) == nh.NRF_E_STATE and error_call(fresh) == nh.NRF_E_STATE
    fresh.close()
    rb = nh.RenderBuffer(0)
    rb.resize(W, H)
    before = finite(ocpu.surface_plane(7701, W, H))
    set_surface(rb, before)
    inf, nan = float("inf"), float("nan")
    refused = [(image_call, o) for o in (
        dict(exposure=None), dict(bg=None), dict(image=None), dict(center=None), dict(ty=0), dict(ty=4), dict(ds=-1), dict(ds=3), dict(axis=2),
        dict(axis=-1), dict(iw=0), dict(ih=-1), dict(iw=16385), dict(ih=16385), dict(zoom=0.0), dict(zoom=-0.0), dict(zoom=inf), dict(zoom=nan),
        dict(center=fp(nan, 0.5)), dict(center=fp(0.5, inf)))]
    refused += [(false_color_call, o) for o in (dict(map=None), dict(average=None), dict(tw=0), dict(th=-3), dict(tw=16385), dict(th=16385), dict(axis=2),
                                                dict(axis=-1), dict(mw=0), dict(mh=0), dict(mw=513), dict(mh=513))]
    refused += [(error_call, o) for o in (dict(truth=None), dict(map=None), dict(average=None), dict(mw=0), dict(mh=0), dict(mw=-1), dict(mw=W + 1),
                                          dict(mh=H + 1))]
    for call, o in refused:
        assert call(rb, **o) == nh.NRF_E_INVALID, (call.__name__, o)
        assert lib.nrf_last_error()
        assert np.array_equal(orp.bits(rb.read()[1]), orp.bits(before)), (call.__name__, o)
        assert np.all(host(m) == 7.0) and host(a)[0] == 7.0, (call.__name__, o)
    rb.close()
    wide = nh.RenderBuffer(0)                                    # 512 cells are the most on an axis, however wide the surface
    wide.resize(600, 1)
    row = torch.full((1, 600), 7.0, dtype=torch.float32, device="cuda")
    g = dev(np.ones((1, 600, 4), np.float32))
    torch.cuda.synchronize()
    assert error_call(wide, truth=g.data_ptr(), mw=513, mh=1, map=row.data_ptr()) == nh.NRF_E_INVALID and np.all(host(row) == 7.0)
    assert error_call(wide, truth=g.data_ptr(), mw=512, mh=1, map=row.data_ptr()) == nh.NRF_OK
    got = host(row)
    assert np.all(got[0, :512] == 1.0) and np.all(got[0, 512:] == 7.0) and host(a)[0] == 1.0   # (1 - 0)^2 * 3 / 3
    wide.close()
    # the calls as they should be: accepted
    rb = nh.RenderBuffer(0)
    rb.resize(W, H)
    assert image_call(rb) == nh.NRF_OK and error_call(rb) == nh.NRF_OK and false_color_call(rb, mw=5, mh=3) == nh.NRF_OK
    rb.close()


# ---------------------------------------------------------------- testbed
def test_testbed_overlays_a_picture_and_compares_with_it(tmp_path, table):
    """`testbed --overlay_image FILE.ppm --overlay_alpha A --compare FILE.ppm`: tonemapped.png is the frame under the picture, the printed
    average is nrf_rb_error_map's of that surface against the picture, error.png is written; a PPM that is short, of another size or of
    another maxval is refused"""
    import subprocess
    from pathlib import Path

    import models
    import synthetic as syn
    import test_mesh_texture_cpu as tcpu
    pytest.importorskip("torch")
    bin_dir = Path(nh.LIB_PATH).parent / "host"
    if not (bin_dir / "testbed").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, H=32)
    snap = tmp_path / "tiny.msgpack"
    syn.write_snapshot(snap, cfg, keep[0], keep[1])
    W, H = 60, 44
    photo = np.random.default_rng(7800).integers(0, 256, (H, W, 3), dtype=np.uint8)
    photo[:, : W // 2] = (np.linspace(0, 255, H)[:, None, None] * np.ones((1, W // 2, 3))).astype(np.uint8)
    ppm = tmp_path / "photo.ppm"
    ppm.write_bytes(f"P6\n{W} {H}\n255\n".encode() + photo.tobytes())
    base = [str(bin_dir / "testbed"), str(snap), str(W), str(H), str(tmp_path) + "/"]
    r = subprocess.run(base + ["--overlay_image", str(ppm), "--overlay_alpha", "0.25", "--compare", str(ppm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert f"overlay: {ppm} over the frame, alpha 0.25" in r.stdout, r.stdout
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("compare:"))
    words = line.replace(",", "").split()
    assert words[1:5] == [str(W), "x", str(H), "cells"] and words[5] == "average" and words[8] == "dB", line
    printed, decibel = F(words[6]), float(words[7])
    # testbed's chain through the library: u8 image -> accumulate -> tonemap (sRGB) -> the picture over it -> the error map
    rb = nh.RenderBuffer(0)
    rb.resize(W, H)
    rb.host_to_accumulate_buffer(np.fromfile(tmp_path / "image.rgb", np.uint8))
    bg = [0.0, 0.0, 0.0, 1.0]
    rb.tonemap(0.0, bg, nh.CS_SRGB)
    developed = rb.read()[1]
    texels = (photo[..., 0].astype(np.uint32) | photo[..., 1].astype(np.uint32) << 8 | photo[..., 2].astype(np.uint32) << 16 | np.uint32(0xFF000000))
    t = dev(texels)
    rb.overlay_image(0.25, 0.0, bg, nh.CS_SRGB, t.data_ptr(), nh.IMG_BYTE, W, H)
    surface = rb.read()[1]
    want = orp.overlay_image(developed, 0.25, 0.0, bg, nh.CS_LINEAR, nh.CS_SRGB, nh.TM_IDENTITY, texels, nh.IMG_BYTE, table)
    np.testing.assert_allclose(surface, want, rtol=RTOL, atol=ATOL)
    got = tcpu.parse_png((tmp_path / "tonemapped.png").read_bytes())
    assert got.shape == (H, W, 3)
    assert np.array_equal(got, np.clip(surface[:, :, :3] * F(255), 0, 255).astype(np.uint8))
    truth = np.concatenate([photo.astype(np.float32) / F(255.0), np.ones((H, W, 1), np.float32)], axis=2)
    _, average, m, a = hold_error_map(rb, surface, truth, W, H)
    assert orp.bits(printed) == orp.bits(average) and abs(decibel - (-10.0 * np.log10(float(average)))) < 1e-3, (line, average)
    rb.overlay_false_color(W, H, 0, m.data_ptr(), W, H, a.data_ptr(), 1.0, True)
    error = tcpu.parse_png((tmp_path / "error.png").read_bytes())
    assert error.shape == (H, W, 3) and error.std() > 1
    assert np.array_equal(error, np.clip(rb.read()[1][:, :, :3] * F(255), 0, 255).astype(np.uint8))
    rb.close()
    # without the options: neither line nor file
    plain = tmp_path / "plain"
    plain.mkdir()
    r = subprocess.run(base[:4] + [str(plain) + "/"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "overlay:" not in r.stdout and "compare:" not in r.stdout and not (plain / "error.png").exists()
    assert not np.array_equal(tcpu.parse_png((plain / "tonemapped.png").read_bytes()), got)
    # refused files
    for name, data, message in [("short.ppm", f"P6\n{W} {H}\n255\n".encode() + photo.tobytes()[:-1], "ends before its last pixel"),
                                ("size.ppm", f"P6\n{W + 1} {H}\n255\n".encode() + bytes((W + 1) * H * 3), "the frame is"),
                                ("deep.ppm", f"P6\n{W} {H}\n65535\n".encode() + bytes(W * H * 6), "maxval 65535"),
                                ("text.ppm", f"P3\n{W} {H}\n255\n".encode() + b"0 " * (W * H * 3), "not a binary PPM")]:
        (tmp_path / name).write_bytes(data)
        for option in ("--overlay_image", "--compare"):                  # (read before the model is loaded: no frame is rendered)
            r = subprocess.run(base + [option, str(tmp_path / name)], capture_output=True, text=True, timeout=120)
            assert r.returncode == 1 and message in r.stderr and "Process time" not in r.stdout, (name, option, r.stderr)
