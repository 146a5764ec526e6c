"""The CPU oracle's presentation chain against the reference's OWN render-buffer kernels, bit for bit.

oracle/ref_render_buffer.cpp compiles R/src/render_buffer.cu (accumulate_kernel, the two `tonemap` functions with the four film
curves, tonemap_kernel, colormap_turbo, overlay_depth_kernel) for the CPU, unchanged, behind stand-in headers (oracle/ref_shim/),
and launches every kernel with its call site's geometry; tests/ref_render_buffer_py.py binds it.  Every comparison is on uint32
views: both sides are CPU code with the same libm, no contraction and Eigen on its scalar path, so nothing takes a tolerance.  The
rows are tests/golden/make_reference_render_buffer_golden.py's: crafted values laid into 67 x 41 planes, not random planes alone.

One thing may differ, deviation D-11 (make_reference_render_buffer_golden.device_rule_tonemap states it): Eigen's host cwiseMax /
cwiseMin keep a NaN, and a -0 against +0, where the device's yield 0 or the bound.  Exactly the positions whose input to such a
call is NaN or -0 are left out of the comparison with the kernel and held to the device rule instead; a plane that holds neither
leaves nothing out, and none of the rows the tonemap test runs does.  A NaN's sign and payload are not compared anywhere: which
operand's NaN an instruction passes on is the compiler's choice of operand order.

Without a reference tree AND without the built library the module skips; with the tree and without the library it fails."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import nerfhip as nh
import oracle_py as op
import ref_kernels_py as rk
import ref_render_buffer_py as rr

U32 = np.uint32
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _library():
    rr.require()
    rk.require()


_cache = {}


def gen():
    if "gen" not in _cache:
        path = Path(__file__).resolve().parent / "golden" / "make_reference_render_buffer_golden.py"
        spec = importlib.util.spec_from_file_location("make_reference_render_buffer_golden", path)
        _cache["gen"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_cache["gen"])
    return _cache["gen"]


def cached(name):
    if name not in _cache:
        _cache[name] = getattr(gen(), name)()
    return _cache[name]


def bits(a):
    a = np.array(a, F32)
    a[np.isnan(a)] = np.nan  # one NaN
    return a.view(U32)


def same_bits(got, want, what, keep=None):
    """equal bits (one NaN for all NaNs) at every position, or at the positions of `keep`"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, f"{what}: shapes {got.shape} != {want.shape}"
    diff = bits(got) != bits(want)
    if keep is not None:
        diff &= keep
    if diff.any():
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} values differ in their bits; first at {at}: "
                             f"oracle {got[at]!r} ({got.view(U32)[at]:#010x}) reference {want[at]!r} ({want.view(U32)[at]:#010x})")


def oracle_accumulate(frame, accum, k, cs):
    return op.rb_accumulate(frame.reshape(-1, 4), accum.reshape(-1, 4), k, cs).reshape(frame.shape)


def oracle_tonemap(plane, exposure, bg, cs, ocs, curve, clamp):
    return op.rb_tonemap(plane.reshape(-1, 4), exposure, bg, cs, ocs, curve, clamp).reshape(plane.shape)


# ------------------------------------------------------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("cs", [nh.CS_LINEAR, nh.CS_SRGB, nh.CS_VISPOSNEG])
def test_accumulate(cs):
    """accumulate_kernel in every colour space at sample counts 0, 1, 2, 255 and 2^24 over the crafted planes (frame values below 0,
    above 1, both zeros, denormals, +inf, NaN, the float on each side of 0.0031308, against earlier means of both signs, inf and
    NaN), then chained: three samples folded one after another, each on the previous result."""
    g = gen()
    frame, accum = cached("accumulate_planes")
    assert frame.shape == (g.H, g.W, 4) and np.isnan(frame).any() and np.isinf(frame).any() and (frame < 0).any()
    for k in g.SAMPLE_COUNTS:
        want = rr.accumulate(frame, accum, k, cs)
        same_bits(oracle_accumulate(frame, accum, k, cs), want, f"accumulate cs {cs} sample_count {k}")
        if k == 16777216:  # k + 1 == k: the new sample still enters the numerator
            finite = np.isfinite(want) & np.isfinite(accum)
            assert (want[finite] != accum[finite]).any()
    zero = np.zeros_like(accum)
    same_bits(oracle_accumulate(frame, zero, 0, cs), rr.accumulate(frame, zero, 0, cs), f"accumulate cs {cs} first sample over a cleared plane")
    if cs == nh.CS_VISPOSNEG:  # the crafted running values change sign in both directions
        n = g.N_ACC_CRAFTED
        a0, a1 = accum.reshape(-1, 4)[n - 4:n], rr.accumulate(frame, accum, 1, cs).reshape(-1, 4)[n - 4:n]
        assert ((a0[:, 0] > 0) & (a1[:, 1] > 0) & (a1[:, 0] == 0)).any() and ((a0[:, 1] > 0) & (a1[:, 0] > 0) & (a1[:, 1] == 0)).any()
    got = want = zero
    rng = np.random.default_rng(61 + cs)
    for k in range(3):
        f = (rng.random(frame.shape, dtype=F32) * F32(1.75) - F32(0.25)).astype(F32)
        got, want = oracle_accumulate(f, got, k, cs), rr.accumulate(f, want, k, cs)
        same_bits(got, want, f"accumulate cs {cs} chained sample {k}")


# --------------------------------------------------------------------------------------------------------------------- tonemap
@pytest.mark.parametrize("cs", [nh.CS_LINEAR, nh.CS_SRGB, nh.CS_VISPOSNEG])
@pytest.mark.parametrize("ocs", [nh.CS_LINEAR, nh.CS_SRGB])
@pytest.mark.parametrize("curve", [nh.TM_IDENTITY, nh.TM_ACES, nh.TM_HABLE, nh.TM_REINHARD])
def test_tonemap(cs, ocs, curve):
    """tonemap_kernel for one (colour space, output colour space, curve) triple at five exposures, three background alphas and both
    values of clamp_output_color, over the crafted plane (alpha below 0, inside [0, 1] and above 1; colours negative, zero, near 1,
    around 50, and the float on each side of both transfer thresholds).  The plane holds no NaN: nothing is left out."""
    g = gen()
    plane = cached("tonemap_plane")
    for exposure in g.EXPOSURES:
        for bg in g.BACKGROUNDS:
            for clamp in (False, True):
                what = f"tonemap cs {cs} ocs {ocs} curve {curve} exposure {exposure} bg alpha {bg[3]} clamp {clamp}"
                want = rr.tonemap(plane, exposure, bg, cs, ocs, curve, clamp)
                assert not (want == 777.0).any(), "a texel was not written"
                same_bits(oracle_tonemap(plane, exposure, bg, cs, ocs, curve, clamp), want, what)
                dev, mask = g.device_rule_tonemap(rr, rk, plane, exposure, bg, cs, ocs, curve, clamp)
                assert not mask.any(), f"{what}: positions left out of a plane without NaN"
                same_bits(dev, want, what + ": the kernel against its own pieces")


def test_tonemap_thresholds_reach_the_transfer_function():
    """The crafted neighbours of 0.04045 arrive at srgb_to_linear as laid in wherever the background's weight is 0 (alpha 1, or a
    background alpha of 0): the two sides of the threshold take different branches, and the oracle agrees on both."""
    g = gen()
    plane = cached("tonemap_plane").reshape(-1, 4)
    at = [i for i in range(g.N_TM_CRAFTED) if plane[i, 3] == 1 and plane[i, 0] in (g.below(g.DECODE_AT), g.DECODE_AT, g.above(g.DECODE_AT))]
    assert len(at) == 3
    px = np.ascontiguousarray(plane[at]).reshape(1, 3, 4)
    out = rr.tonemap(px, 0.0, g.BACKGROUNDS[1], nh.CS_SRGB, nh.CS_LINEAR, nh.TM_IDENTITY, False)[0, :, 0]
    lo, mid, hi = (F32(v) for v in px[0, :, 0])
    assert out[0] == lo / F32(12.92) and out[1] == mid / F32(12.92) and out[2] != hi / F32(12.92)
    same_bits(out, rk.srgb_to_linear(px[0, :, 0]), "srgb_to_linear at the threshold")
    same_bits(oracle_tonemap(px, 0.0, g.BACKGROUNDS[1], nh.CS_SRGB, nh.CS_LINEAR, nh.TM_IDENTITY, False)[0, :, 0], out, "the oracle at the threshold")


@pytest.mark.parametrize("curve", [nh.TM_IDENTITY, nh.TM_ACES, nh.TM_HABLE, nh.TM_REINHARD])
def test_film_curve_and_tonemap_function(curve):
    """The two `tonemap` device functions on their own.  The film curve against the oracle's: a Linear -> Linear development of an
    opaque pixel at exposure 0 over a background of alpha 0 is the curve and nothing else.  The five-argument function against the
    oracle's development of the same opaque pixels, at every exposure; and, for the curves that do not mix channels, with a DIFFERENT
    exposure per channel, which the kernel never passes: channel c then is channel c of a development at exposure[c]."""
    g = gen()
    rgb = np.ascontiguousarray(cached("tonemap_plane")[..., :3]).reshape(-1, 3)
    opaque = np.concatenate([rgb, np.ones((len(rgb), 1), F32)], axis=1).reshape(1, -1, 4)
    develop = lambda e, cs, ocs: oracle_tonemap(opaque, e, g.BACKGROUNDS[0], cs, ocs, curve, False)[0, :, :3]
    same_bits(develop(0.0, nh.CS_LINEAR, nh.CS_LINEAR), rr.film_curve(rgb, curve), f"film curve {curve}")
    for cs in g.COLOR_SPACES:
        for ocs in g.DISPLAY_SPACES:
            for e in g.EXPOSURES:
                same_bits(develop(e, cs, ocs), rr.tonemap_color(rgb, e, curve, cs, ocs), f"tonemap(col, {e}, curve {curve}, cs {cs}, ocs {ocs})")
            if curve != nh.TM_REINHARD:
                per_channel = (-1.0, 0.6, 2.0)
                want = rr.tonemap_color(rgb, per_channel, curve, cs, ocs)
                for c, e in enumerate(per_channel):
                    same_bits(develop(e, cs, ocs)[:, c], want[:, c], f"tonemap(col, exposure[{c}] = {e}, curve {curve}, cs {cs}, ocs {ocs})")


# ------------------------------------------------------------------------------------------------------------ the NaN deviation
@pytest.mark.parametrize("curve", [nh.TM_IDENTITY, nh.TM_ACES, nh.TM_HABLE, nh.TM_REINHARD])
def test_deviation_d11_host_cwise_max_keeps_a_nan_and_a_negative_zero(curve):
    """Over the NaN plane, every colour space and display, both clamps and two backgrounds: outside the D-11 positions the oracle has
    the kernel's bits; at ALL positions it has the device rule's (fmaxf / fminf), built from the reference's own pieces; the
    positions are only those whose input to a cwiseMax / cwiseMin is NaN or -0 -- never a pixel that holds neither --, and where
    the kernel's CPU compile differs from the device rule there, it is by keeping the NaN or the -0 that the device would not."""
    g = gen()
    plane = cached("nan_plane")
    special = (np.isnan(plane) | g.negative_zero(plane)).any(axis=-1)
    assert special.sum() == 100
    kept_nan = kept_zero = 0
    for bg in g.NAN_BACKGROUNDS:
        for cs in g.COLOR_SPACES:
            for ocs in g.DISPLAY_SPACES:
                for clamp in (False, True):
                    what = f"NaN plane cs {cs} ocs {ocs} curve {curve} clamp {clamp} bg alpha {bg[3]}"
                    got = oracle_tonemap(plane, g.NAN_EXPOSURE, bg, cs, ocs, curve, clamp)
                    want = rr.tonemap(plane, g.NAN_EXPOSURE, bg, cs, ocs, curve, clamp)
                    dev, mask = g.device_rule_tonemap(rr, rk, plane, g.NAN_EXPOSURE, bg, cs, ocs, curve, clamp)
                    assert not mask[~special].any(), f"{what}: a pixel without NaN or -0 is left out"
                    assert mask.any() == (curve != nh.TM_IDENTITY or clamp), what
                    same_bits(got, want, what + " outside D-11", keep=~mask)
                    same_bits(dev, want, what + ": the kernel against its own pieces outside D-11", keep=~mask)
                    same_bits(got, dev, what + " against the device rule")
                    differs = bits(want) != bits(dev)
                    assert (np.isnan(want[differs]) | g.negative_zero(want[differs])).all() and not np.isnan(dev[mask]).any(), what
                    kept_nan, kept_zero = kept_nan + int(np.isnan(want[differs]).sum()), kept_zero + int(g.negative_zero(want[differs]).sum())
    assert kept_nan > 0 and (kept_zero > 0 or curve in (nh.TM_ACES, nh.TM_HABLE)), "the plane is meant to show both halves of the deviation"
    # the literal form, one pixel: max(NaN, 0) ahead of the curve
    if curve != nh.TM_IDENTITY:
        assert np.isnan(rr.film_curve(np.array([[np.nan, 0.5, 2.0]], F32), curve)[0, 0])
        opaque = np.array([[[np.nan, 0.5, 2.0, 1.0]]], F32)
        got = oracle_tonemap(opaque, 0.0, g.BACKGROUNDS[0], nh.CS_LINEAR, nh.CS_LINEAR, curve, False)[0, 0, :3]
        same_bits(got, rr.film_curve(np.array([[0.0, 0.5, 2.0]], F32), curve)[0], "fmaxf(NaN, 0) = 0 ahead of the curve")


# ----------------------------------------------------------------------------------------------------------------------- turbo
def oracle_turbo(x):
    """The oracle's colour map through its overlay: a 1 x n surface over a 1 x n image at zoom 1 is the identity resampling, and
    alpha 1 over a zero surface leaves colour * 1 + 0 * 0"""
    x = np.ascontiguousarray(x, F32).reshape(1, -1)
    out = op.rb_overlay_depth(np.zeros((1, x.size, 4), F32), 1.0, x, 1.0, 0, 1.0, (0.5, 0.5))
    assert (out[0, :, 3] == 1).all(), "every texel of the image is reached"
    return out[0, :, :3]


def test_colormap_turbo():
    """colormap_turbo at i / 4096, i = 0 .. 4096, and at -3, 7, both zeros, a denormal, the infinities and NaN (`__saturatef` is the
    stand-in's and sends NaN to 0, as the oracle does)"""
    x = gen().turbo_inputs()
    assert len(x) == 4105
    want = rr.colormap_turbo(x)
    same_bits(oracle_turbo(x), want, "colormap_turbo")
    same_bits(want[-1], want[0], "turbo(NaN) = turbo(0)")
    same_bits(want[4097], want[0], "turbo(-3) = turbo(0)")
    same_bits(want[4098], want[4096], "turbo(7) = turbo(1)")


# --------------------------------------------------------------------------------------------------------------- overlay_depth
@pytest.mark.parametrize("name", ["full", "blend-zoom-in", "zoom-out", "alpha0", "outside-axis0", "outside-axis1", "tall-image", "one-texel"])
@pytest.mark.parametrize("size", [(67, 41), (23, 17)])
def test_overlay_depth(name, size):
    """overlay_depth_kernel: the three parameter rows of test_overlay_depth_matches_oracle, alpha 0, a zoom and centre that push part
    of the surface outside the image on either fov_axis, a tall image and an image of one texel"""
    g = gen()
    row = g.OVERLAY_ROWS[name]
    depth, before = g.overlay_depth_image(row["image"]), g.overlay_before(*size)
    args = (row["alpha"], depth, g.DEPTH_SCALE, row["fov_axis"], row["zoom"], row["center"])
    want = rr.overlay_depth(before, *args)
    same_bits(op.rb_overlay_depth(before, *args), want, f"overlay_depth {name} on {size}")
    inside = rr.overlay_depth(np.zeros_like(before), 1.0, *args[1:])[..., 3] == 1  # alpha 1 over zero: 1 inside the image, 0 outside
    if name.startswith("outside"):
        assert inside.any() and not inside.all(), "the row is meant to push part of the surface outside the image"
    elif name == "full":
        assert inside.all()
    if row["alpha"] == 0:
        same_bits(want, before, "alpha 0 leaves the surface")


def test_overlay_rows_are_the_existing_gpu_rows():
    rows = list(gen().OVERLAY_ROWS.values())[:3]
    assert [(r["alpha"], r["fov_axis"], r["zoom"], r["center"]) for r in rows] == \
        [(1.0, 0, 1.0, (0.5, 0.5)), (0.35, 1, 1.7, (0.42, 0.61)), (0.5, 0, 0.6, (0.5, 0.5))]


# ------------------------------------------------------------------------------------------------------------ golden vectors
def test_golden_vectors_regenerate_to_the_committed_bytes(tmp_path):
    """tests/golden/reference_render_buffer.npz, regenerated from the library: the same members in the same order, every member's
    .npy bytes equal.  (Members are compared uncompressed: the deflate stream around them may differ between zlib builds.)"""
    g = gen()
    committed = Path(g.__file__).with_name("reference_render_buffer.npz")
    assert committed.stat().st_size <= 160753, "larger than the largest fixture that was here before it"
    out = tmp_path / "reference_render_buffer.npz"
    g.write(out)
    fresh, kept = g.read_members(out), g.read_members(committed)
    assert [n for n, _ in fresh] == [n for n, _ in kept]
    stale = [n for (n, a), (_, b) in zip(fresh, kept) if a != b]
    assert not stale, f"tests/golden/reference_render_buffer.npz is stale in {stale}: run tests/golden/make_reference_render_buffer_golden.py"
