"""The HIP render buffer against tests/golden/reference_render_buffer.npz: rows the REFERENCE's own kernels wrote
(R/src/render_buffer.cu compiled for the CPU; tests/golden/make_reference_render_buffer_golden.py).  Only the fixture is read:
neither a reference tree nor oracle/_ref/ is needed.  The generator module is imported for the row definitions alone.

The chain is per pixel, so the fixture's thinned pixels are laid out as a P x 5 plane: five copies, more than one block.

Bit for bit: every row with no power function on the device -- render space Linear or VisPosNeg, display Linear, integer
exposure (2^e is exact, every other operation an individually rounded fp32 add / multiply / divide / max on both sides) --, all
four curves on them, every overlay row and the colour map.  Rows through the device's `pow_positive` (sRGB on either side) take
the tolerances tests/test_render_buffer.py::test_hip_matches_oracle states: rtol 2e-6 / atol 1e-7 on the mean, rtol 2e-5 / atol
2e-6 on the surface; the non-integer exposure is held at the surface tolerance too (its gain is the host's libm on another
machine).  The NaN / -0 rows are held to the device rule of deviation D-11 (fmaxf / fminf), which is what the fixture records for
them.  A NaN's sign and payload are not compared.

What the library's calls cannot reach and so is not here: clamp_output_color (no call carries it; the reference sets it only with
DLSS) and sample_count 2^24 (the count is the number of calls made); both are held on the CPU, in the oracle."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import nerfhip as nh

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
G = np.load(GOLDEN / "reference_render_buffer.npz")
U32, F32 = np.uint32, np.float32
TILES = 5


def _generator():
    spec = importlib.util.spec_from_file_location("make_reference_render_buffer_golden", GOLDEN / "make_reference_render_buffer_golden.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


GEN = _generator()
TRIPLES = GEN.triples()
TM_ROWS = GEN.fixture_tonemap_rows()


_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipFree.argtypes = [C.c_void_p]
    return _hip


def upload(ptr, a):
    """host -> device, complete on return (the render buffer works on a stream of its own)"""
    a = np.ascontiguousarray(a, F32)
    assert hip().hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0
    assert hip().hipDeviceSynchronize() == 0


def tiled(px):
    return np.ascontiguousarray(np.broadcast_to(px[None], (TILES,) + px.shape))


def bits(a):
    a = np.array(a, F32)
    a[np.isnan(a)] = np.nan
    return a.view(U32)


def same_bits(got, want, what):
    """every tile of `got` has the bits of `want` (one NaN for all NaNs)"""
    want = tiled(np.ascontiguousarray(want, F32)) if got.ndim == want.ndim + 1 else want
    assert got.shape == want.shape, f"{what}: shapes {got.shape} != {want.shape}"
    diff = bits(got) != bits(want)
    if diff.any():
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} values differ in their bits; first at {at}: "
                             f"device {got[at]!r} ({got.view(U32)[at]:#010x}) reference {want[at]!r} ({want.view(U32)[at]:#010x})")


def close(got, want, rtol, atol, what):
    np.testing.assert_allclose(got, tiled(np.ascontiguousarray(want, F32)), rtol=rtol, atol=atol, err_msg=what)


def buffer(px, cs, curve=nh.TM_IDENTITY):
    rb = nh.RenderBuffer(0)
    rb.resize(len(px), TILES)
    rb.set_color_space(cs)
    rb.set_tonemap_curve(curve)
    return rb


def bit_exact_row(cs, ocs, exposure):
    return not GEN.has_device_power(cs, ocs) and float(exposure) == int(exposure)


# ------------------------------------------------------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("cs", [nh.CS_LINEAR, nh.CS_SRGB, nh.CS_VISPOSNEG])
def test_accumulate_against_the_references_kernel(cs):
    """nrf_rb_accumulate at sample counts 0 (over the cleared plane), 1, 2 and 255 on the crafted frame and mean planes: below 0,
    above 1, both zeros, denormals, +inf, NaN, the float on each side of 0.0031308, a VisPosNeg value that changes sign"""
    frame, accum = G["acc_frame"], G["acc_accum"]
    rb = buffer(frame, cs)
    frame_p, _, accum_p, _ = rb.buffers()
    upload(frame_p, tiled(frame))
    for k in (0, 1, 2, 255):
        while rb.spp() < k:
            rb.accumulate()
        upload(accum_p, tiled(accum if k else np.zeros_like(accum)))
        rb.accumulate()
        assert rb.spp() == k + 1
        got, _ = rb.read()
        what = f"accumulate cs {cs} sample_count {k}"
        if cs == nh.CS_SRGB:  # linear_to_srgb: the device's power
            close(got, G[f"acc/{cs}/{k}"], 2e-6, 1e-7, what)
        else:
            same_bits(got, G[f"acc/{cs}/{k}"], what)
    rb.close()


# --------------------------------------------------------------------------------------------------------------------- tonemap
def check_surface(got, want, cs, ocs, exposure, what):
    if bit_exact_row(cs, ocs, exposure):
        same_bits(got, want, what)
    else:
        close(got, want, 2e-5, 2e-6, what)


@pytest.mark.parametrize("cs,ocs,curve", TRIPLES)
def test_tonemap_against_the_references_kernel(cs, ocs, curve):
    """nrf_rb_tonemap on the crafted mean plane (alpha below 0, inside [0, 1] and above 1; colours negative, zero, near 1, around 50,
    the float on each side of both transfer thresholds) for one (colour space, display, curve) triple: the fixture's exposures and
    background alphas of that triple"""
    rows = [r for r in TM_ROWS if r[1:4] == (cs, ocs, curve)]
    assert len(rows) == (2 if GEN.has_device_power(cs, ocs) else 5)
    rb = buffer(G["tm_in"], cs, curve)
    upload(rb.buffers()[2], tiled(G["tm_in"]))
    for key, _, _, _, exposure, bg in rows:
        rb.tonemap(exposure, bg, ocs)
        _, got = rb.read()
        check_surface(got, G[key], cs, ocs, exposure, key)
    rb.close()


def test_the_fixture_covers_every_exposure_and_background_bit_for_bit():
    exact = [r for r in TM_ROWS if bit_exact_row(r[1], r[2], r[4])]
    assert {r[3] for r in exact} == {0, 1, 2, 3} and {r[1] for r in exact} == {nh.CS_LINEAR, nh.CS_VISPOSNEG}
    assert {r[4] for r in exact} == {-2.0, 0.0, 1.0, 3.0} and {r[5][3] for r in exact} == {0.0, 0.8, 1.0}
    assert {r[4] for r in TM_ROWS} == set(GEN.EXPOSURES) and {r[1:4] for r in TM_ROWS} == set(TRIPLES)


@pytest.mark.parametrize("ocs,curve", [(o, c) for o in (nh.CS_LINEAR, nh.CS_SRGB) for c in (0, 1, 2, 3)])
def test_present_against_the_references_kernels(ocs, curve):
    """nrf_rb_present as a first sample in the Linear colour space: the mean is the frame itself, (0 * 0 + x) / 1, so with the crafted
    plane as the frame the surface is the fixture's tonemap row and the mean plane the frame"""
    cs = nh.CS_LINEAR
    rows = [r for r in TM_ROWS if r[1:4] == (cs, ocs, curve)]
    rb = buffer(G["tm_in"], cs, curve)
    frame_p, _, accum_p, _ = rb.buffers()
    upload(frame_p, tiled(G["tm_in"]))
    for key, _, _, _, exposure, bg in rows:
        rb.reset_accumulation()
        upload(accum_p, np.full((TILES, len(G["tm_in"]), 4), np.nan, F32))  # ignored by a first sample
        rb.present(exposure, bg, ocs)
        mean, got = rb.read()
        same_bits(mean, G["tm_in"], key + ": the mean after one sample")
        check_surface(got, G[key], cs, ocs, exposure, key + " through present")
    rb.close()


@pytest.mark.parametrize("cs,ocs,curve", TRIPLES)
def test_deviation_d11_nan_and_negative_zero_follow_the_device_rule(cs, ocs, curve):
    """The NaN / -0 rows: the fixture holds the device rule's surface (fmaxf(x, 0) ahead of a curve: NaN and -0 give +0), which is the
    reference kernel's own outside the recorded D-11 positions"""
    want, mask = G[f"nan/{cs}{ocs}{curve}"], G[f"nan_mask/{cs}{ocs}{curve}"].astype(bool)
    assert mask.any() == (curve != nh.TM_IDENTITY) and not np.isnan(want[mask]).any()
    rb = buffer(G["nan_in"], cs, curve)
    upload(rb.buffers()[2], tiled(G["nan_in"]))
    rb.tonemap(GEN.NAN_EXPOSURE, GEN.NAN_BACKGROUNDS[0], ocs)
    _, got = rb.read()
    check_surface(got, want, cs, ocs, GEN.NAN_EXPOSURE, f"NaN rows cs {cs} ocs {ocs} curve {curve}")
    assert not np.isnan(got[:, mask]).any() and (np.isnan(got) == np.isnan(tiled(want))).all()
    rb.close()


# ------------------------------------------------------------------------------------------------------- turbo, overlay_depth
def overlay(before, depth, alpha, depth_scale, fov_axis, zoom, center):
    h, w = before.shape[:2]
    depth = np.ascontiguousarray(depth, F32)
    rb = nh.RenderBuffer(0)
    rb.resize(w, h)
    upload(rb.buffers()[3], before)
    d = C.c_void_p()
    assert hip().hipMalloc(C.byref(d), depth.nbytes) == 0
    try:
        upload(d, depth)
        rb.overlay_depth(alpha, d.value, depth_scale, depth.shape[1], depth.shape[0], fov_axis, zoom, center)
        _, after = rb.read()
    finally:
        hip().hipFree(d)
        rb.close()
    return after


def test_colormap_turbo_against_the_references():
    """colormap_turbo through nrf_rb_overlay_depth: a 1 x n surface over a 1 x n image at zoom 1 is the identity resampling, alpha 1
    over a zero surface leaves the colour; i / 4096 for every 8th i, and -3, 7, both zeros, a denormal, the infinities and NaN"""
    x = GEN.turbo_inputs()[GEN.TURBO_PICK]
    after = overlay(np.zeros((1, len(x), 4), F32), x.reshape(1, -1), 1.0, 1.0, 0, 1.0, (0.5, 0.5))
    assert (after[0, :, 3] == 1).all()
    same_bits(after[0, :, :3], G["turbo"], "colormap_turbo")


@pytest.mark.parametrize("name", list(GEN.OVERLAY_ROWS))
def test_overlay_depth_against_the_references_kernel(name):
    row = GEN.OVERLAY_ROWS[name]
    before = GEN.overlay_before(*GEN.OVERLAY_FIXTURE_SURFACE)
    after = overlay(before, G[f"ov_depth/{row['image']}"], row["alpha"], GEN.DEPTH_SCALE, row["fov_axis"], row["zoom"], row["center"])
    same_bits(after, G[f"ov/{name}"], f"overlay_depth {name}")
