#!/usr/bin/env python3
"""Generates tests/golden/reference_render_buffer.npz: outputs of the REFERENCE's own render-buffer kernels, compiled for the CPU.

Made by oracle/_ref/libref_render_buffer.so (oracle/ref_render_buffer.cpp: R/src/render_buffer.cu unchanged, behind stand-in
headers), not by the oracle: these are the rows tests/test_reference_render_buffer_gpu.py holds nrf_rb_accumulate, nrf_rb_tonemap,
nrf_rb_present and nrf_rb_overlay_depth to on a machine that has neither the reference tree nor that library.  Data only: inputs
that cannot be rebuilt from integers, and recorded results.

This module also DEFINES the rows of tests/test_reference_render_buffer_cpu.py: the planes (accumulate_planes, tonemap_plane,
nan_plane, turbo_inputs, overlay_inputs), the parameter lists, and `device_rule_tonemap`, the statement of deviation D-11.  The CPU
module runs every row on whole 67 x 41 planes; the fixture records a thinned set (ACC_PIXELS, TM_PIXELS, NAN_PIXELS of those planes --
the chain is per pixel --, every 8th turbo input, the overlays on a 23 x 17 surface) so that the file stays below the largest
fixture that was here before it.

  acc_frame, acc_accum [P][4]       the thinned accumulate planes
  acc/<cs>/<k> [P][4]               accumulate_kernel, colour space cs, sample_count k (k = 0 over a zeroed plane, as the call site clears it)
  tm_in [P][4]                      the thinned tonemap plane
  tm/<cs><ocs><curve>/<e>/<bg> [P][4]   tonemap_kernel without the output clamp (the library's calls have none); see fixture_tonemap_rows
  nan_in [P][4], nan/<cs><ocs><curve> [P][4], nan_mask/<cs><ocs><curve> [P][4]
                                    the NaN and -0 rows: the DEVICE-RULE result (equal to the kernel's outside the mask) and the D-11 positions
  turbo [521][3]                    colormap_turbo of turbo_inputs()[TURBO_PICK]
  ov_depth/<image>, ov/<row> [17][23][4]    overlay_depth_kernel over overlay_before(23, 17)

Run from the repo root, after `make -C oracle ref`:  python tests/golden/make_reference_render_buffer_golden.py
"""
import io
import sys
import zipfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "nerf-cuda_amd"), str(ROOT / "tests")]

F32 = np.float32
W, H = 67, 41  # tests/test_render_buffer.py's plane: a multiple of neither 16 nor 8, 5 x 6 blocks of the reference's launch
CS_LINEAR, CS_SRGB, CS_VISPOSNEG = 0, 1, 2
COLOR_SPACES, DISPLAY_SPACES, CURVES = (0, 1, 2), (0, 1), (0, 1, 2, 3)
TM_REINHARD = 3
EXPOSURES = (-2.0, 0.0, 1.0, 3.0, 0.6)
BACKGROUNDS = ((0.3, 0.6, 0.9, 0.0), (0.3, 0.6, 0.9, 0.8), (0.3, 0.6, 0.9, 1.0))
SAMPLE_COUNTS = (0, 1, 2, 255, 16777216)  # 2^24: k + 1 == k in fp32
assert F32(16777216) + F32(1) == F32(16777216)


def below(x):
    return np.nextafter(F32(x), F32(-np.inf))


def above(x):
    return np.nextafter(F32(x), F32(np.inf))


DENORMAL = F32(1e-40)
ENCODE_AT, DECODE_AT = F32(0.0031308), F32(0.04045)  # the thresholds of linear_to_srgb and srgb_to_linear


# ------------------------------------------------------------------------------------------------------------------ accumulate
def accumulate_planes():
    """(frame, accum) [H][W][4].  The first 104 pixels are every frame value of F against every earlier mean of A in channel 0, the
    other channels rotated through the same lists; four pixels whose VisPosNeg running value changes sign in either direction; the
    rest uniform in [-0.25, 1.5) (frame) and [0, 1.5) (mean)."""
    Fv = np.array([-0.75, 1.5, 0.0, -0.0, DENORMAL, -DENORMAL, np.inf, np.nan, below(ENCODE_AT), ENCODE_AT, above(ENCODE_AT), 0.25, 1.0], F32)
    Av = np.array([0.0, -0.0, 0.5, -0.5, 2.0, DENORMAL, np.inf, np.nan], F32)
    rng = np.random.default_rng(51)
    frame = rng.random((H * W, 4), dtype=F32) * F32(1.75) - F32(0.25)
    accum = rng.random((H * W, 4), dtype=F32) * F32(1.5)
    i = 0
    for k in range(len(Av)):
        for j in range(len(Fv)):
            frame[i] = [Fv[j], Fv[(j + 3) % len(Fv)], Fv[(j + 7) % len(Fv)], Fv[(j + 5) % len(Fv)]]
            accum[i] = [Av[k], Av[(k + 1) % len(Av)], Av[(k + 3) % len(Av)], Av[(k + 2) % len(Av)]]
            i += 1
    frame[i:i + 4] = [[0, 2, 0.1, 1], [2, 0, 0.1, 1], [0.25, 0.75, 0, 1], [0.75, 0.25, 0, 0]]
    accum[i:i + 4] = [[0.5, 0, 0.2, 1], [0, 0.5, 0.2, 1], [0.5, 0, 0, 0.5], [0, 0.5, 0, 0.5]]
    return frame.reshape(H, W, 4), accum.reshape(H, W, 4)


N_ACC_CRAFTED = 108
ACC_PIXELS = np.r_[0:104:2, 104:108, 108:126]  # every other crafted pixel, the sign changes, 18 random ones


# --------------------------------------------------------------------------------------------------------------------- tonemap
def tonemap_plane():
    """The accumulate plane that tonemap rows develop, [H][W][4].  The first 80 pixels are 16 colour values (negative, zero, the
    float on each side of both transfer thresholds, near 1, around 50) against 5 alphas (below 0, 0, inside, 1, above 1), the other two
    channels rotated through the list.  With alpha 1, or a background alpha of 0, the background's weight is 0 and the colour reaches
    srgb_to_linear as laid in -- the threshold neighbours stay neighbours.  The rest: colours in [-0.25, 1.5), alphas in [-0.2, 1.2)."""
    Cv = np.array([-0.5, -1e-3, 0.0, 1e-3, below(ENCODE_AT), ENCODE_AT, above(ENCODE_AT), below(DECODE_AT), DECODE_AT, above(DECODE_AT),
                   0.5, 0.999, 1.0, 1.001, 50.0, 47.5], F32)
    Al = np.array([-0.25, 0.0, 0.3, 1.0, 1.5], F32)
    rng = np.random.default_rng(52)
    p = rng.random((H * W, 4), dtype=F32) * F32(1.75) - F32(0.25)
    p[:, 3] = rng.random(H * W, dtype=F32) * F32(1.4) - F32(0.2)
    i = 0
    for a in Al:
        for j in range(len(Cv)):
            p[i] = [Cv[j], Cv[(j + 5) % len(Cv)], Cv[(j + 11) % len(Cv)], a]
            i += 1
    assert not np.isnan(p).any() and not negative_zero(p).any()  # those are nan_plane()'s: deviation D-11
    return p.reshape(H, W, 4)


N_TM_CRAFTED = 80
TM_PIXELS = np.r_[0:16, 16:32:2, 32:48:2, 48:64, 64:80:2, 80:88]  # alpha -0.25 and 1 whole, the others halved, 8 random: 64


def negative_zero(a):
    return (a == 0) & np.signbit(a)


def nan_plane():
    """tonemap_plane() with a NaN laid into pixels 200..279 -- by pixel in r, g, b, alpha, or all of rgb -- and a -0 into pixels
    280..299, in r, g or b under an alpha of 1.5: over a background of alpha 0 the weight (1 - 1.5) * 0 is -0 and the -0 reaches the
    curve and the clamp (-0 + -0); over any other background, or under another alpha, the sum is +0 or the background's colour"""
    p = tonemap_plane().reshape(-1, 4).copy()
    for i in range(200, 280):
        k = i % 5
        if k == 4:
            p[i, :3] = np.nan
        else:
            p[i, k] = np.nan
    for i in range(280, 300):
        p[i, i % 3], p[i, 3] = -0.0, 1.5
    return p.reshape(H, W, 4)


NAN_PIXELS = np.r_[196:216, 275:290, 298:302]  # clean pixels on both sides of the block
NAN_EXPOSURE, NAN_BACKGROUNDS = 1.0, (BACKGROUNDS[0], BACKGROUNDS[1])  # the fixture records the first


def device_rule_tonemap(rr, rk, plane, exposure, bg, cs, ocs, curve, clamp):
    """Deviation D-11.  Eigen's cwiseMax / cwiseMin -- the curves' `x.cwiseMax(0.f)` (R/src/render_buffer.cu:266), the output clamp
    (:552) -- are std::max / std::min in a host compile: `a < b ? b : a`, which KEEPS a NaN in `a` and keeps a -0 against +0.  On the
    device Eigen specialises them to fmaxf / fminf, which return the other operand for a NaN and order -0 below +0.  The library
    and the oracle follow the device.  Returns (expected, mask):

    expected  the device-rule surface, put together from the reference's own pieces: tonemap_kernel with the Identity curve and a
              Linear display gives the colour as it ENTERS the curve (and the final alpha); fmaxf(x, 0) there is `x > 0 ? x : +0`;
              then the reference's film curve, its linear_to_srgb, and the clamp as fminf(fmaxf(v, 0), 1).
    mask      where the reference's CPU compile cannot be compared: the elements whose input to a cwiseMax / cwiseMin is NaN or -0
              in the reference -- the curve's input, and with the clamp the kernel's own unclamped output.  Reinhard's luminance
              mixes the three channels, so there one NaN channel takes the pixel's other two with it (Y is NaN on the host and
              finite on the device).  A plane that holds neither a NaN nor a -0 has an empty mask."""
    fmax0 = lambda v: np.where(v > 0, v, F32(0)).astype(F32)
    pre = rr.tonemap(plane, exposure, bg, cs, CS_LINEAR, 0, False)
    rgb = pre[..., :3]
    nan_in = np.isnan(rgb)
    mask = np.zeros(pre.shape, bool)
    if curve != 0:
        mask[..., :3] = (nan_in.any(axis=-1, keepdims=True) if curve == TM_REINHARD else nan_in) | negative_zero(rgb)
        rgb = rr.film_curve(fmax0(rgb), curve).reshape(rgb.shape)
    if ocs == CS_SRGB:
        rgb = rk.linear_to_srgb(rgb)
    out = np.concatenate([rgb, pre[..., 3:]], axis=-1).astype(F32)
    if clamp:
        unclamped = rr.tonemap(plane, exposure, bg, cs, ocs, curve, False)
        mask |= np.isnan(unclamped) | negative_zero(unclamped)
        out = fmax0(out)
        out = np.where(out < 1, out, F32(1)).astype(F32)
    return out, mask


def triples():
    return [(cs, ocs, curve) for cs in COLOR_SPACES for ocs in DISPLAY_SPACES for curve in CURVES]


def has_device_power(cs, ocs):
    """whether the device evaluates a power function per pixel in this row (either transfer function)"""
    return cs == CS_SRGB or ocs == CS_SRGB


def fixture_tonemap_rows():
    """[(key, cs, ocs, curve, exposure, background)].  Rows with no power on the device take every exposure; the others one integer
    exposure and the non-integer one.  The background alphas rotate."""
    rows = []
    for t, (cs, ocs, curve) in enumerate(triples()):
        exposures = EXPOSURES if not has_device_power(cs, ocs) else (EXPOSURES[t % 4], EXPOSURES[4])
        for e, exposure in enumerate(exposures):
            b = (t + e) % 3
            rows.append((f"tm/{cs}{ocs}{curve}/e{exposure:g}/bg{b}", cs, ocs, curve, exposure, BACKGROUNDS[b]))
    return rows


# ----------------------------------------------------------------------------------------------------------------------- turbo
TURBO_SPECIAL = np.array([-3.0, 7.0, 0.0, -0.0, DENORMAL, np.inf, -np.inf, np.nan], F32)


def turbo_inputs():
    """i / 4096 for i = 0 .. 4096, then the values outside [0, 1], both zeros, a denormal, the infinities and NaN"""
    return np.concatenate([(np.arange(4097) / 4096.0).astype(F32), TURBO_SPECIAL])


TURBO_PICK = np.r_[0:4097:8, 4097:4105]


# --------------------------------------------------------------------------------------------------------------- overlay_depth
DEPTH_SCALE = 0.9
# the first three are the parameter rows of tests/test_render_buffer.py::test_overlay_depth_matches_oracle
OVERLAY_ROWS = {
    "full": dict(alpha=1.0, fov_axis=0, zoom=1.0, center=(0.5, 0.5), image="20x15"),
    "blend-zoom-in": dict(alpha=0.35, fov_axis=1, zoom=1.7, center=(0.42, 0.61), image="20x15"),
    "zoom-out": dict(alpha=0.5, fov_axis=0, zoom=0.6, center=(0.5, 0.5), image="20x15"),
    "alpha0": dict(alpha=0.0, fov_axis=0, zoom=1.3, center=(0.5, 0.5), image="20x15"),
    "outside-axis0": dict(alpha=0.8, fov_axis=0, zoom=0.45, center=(0.9, 0.2), image="20x15"),  # part of the surface misses the image
    "outside-axis1": dict(alpha=0.8, fov_axis=1, zoom=0.45, center=(0.1, 0.85), image="20x15"),
    "tall-image": dict(alpha=0.6, fov_axis=1, zoom=1.0, center=(0.5, 0.5), image="9x31"),
    "one-texel": dict(alpha=0.75, fov_axis=0, zoom=0.8, center=(0.5, 0.5), image="1x1"),
}
OVERLAY_IMAGES = {"20x15": (20, 15), "9x31": (9, 31), "1x1": (1, 1)}
OVERLAY_FIXTURE_SURFACE = (23, 17)  # 2 x 3 blocks of the reference's launch, two blocks of the library's


def overlay_before(w, h):
    """the surface before the overlay, from integers: multiples of 1/32 in [0, 1)"""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(4), indexing="ij")
    return (((x * 7 + y * 13 + c * 5) % 32) / 32.0).astype(F32)


def overlay_depth_image(name):
    """depth [ih][iw]: uniform in [-0.1, 1.2) -- with the scale 0.9 both ends saturate --, the first texels of the 20 x 15 image special"""
    iw, ih = OVERLAY_IMAGES[name]
    d = (np.random.default_rng(53 + iw).random((ih, iw), dtype=F32) * F32(1.3) - F32(0.1)).astype(F32)
    if name == "20x15":
        d[7, 8:14] = [np.nan, np.inf, -np.inf, -3.0, 7.0, DENORMAL]
    return d


# --------------------------------------------------------------------------------------------------------------------- fixture
def vectors():
    import ref_kernels_py as rk
    import ref_render_buffer_py as rr

    v = {}
    frame, accum = accumulate_planes()
    pick = lambda plane, idx: np.ascontiguousarray(plane.reshape(-1, 4)[idx])
    v["acc_frame"], v["acc_accum"] = pick(frame, ACC_PIXELS), pick(accum, ACC_PIXELS)
    for cs in COLOR_SPACES:
        for k in SAMPLE_COUNTS:
            v[f"acc/{cs}/{k}"] = pick(rr.accumulate(frame, accum if k else np.zeros_like(accum), k, cs), ACC_PIXELS)
    plane = tonemap_plane()
    v["tm_in"] = pick(plane, TM_PIXELS)
    for key, cs, ocs, curve, exposure, bg in fixture_tonemap_rows():
        v[key] = pick(rr.tonemap(plane, exposure, bg, cs, ocs, curve, False), TM_PIXELS)
    nans = nan_plane()
    v["nan_in"] = pick(nans, NAN_PIXELS)
    for cs, ocs, curve in triples():
        want, mask = device_rule_tonemap(rr, rk, nans, NAN_EXPOSURE, NAN_BACKGROUNDS[0], cs, ocs, curve, False)
        v[f"nan/{cs}{ocs}{curve}"], v[f"nan_mask/{cs}{ocs}{curve}"] = pick(want, NAN_PIXELS), pick(mask, NAN_PIXELS).astype(np.uint8)
    v["turbo"] = rr.colormap_turbo(turbo_inputs()[TURBO_PICK])
    for name in OVERLAY_IMAGES:
        v[f"ov_depth/{name}"] = overlay_depth_image(name)
    for name, row in OVERLAY_ROWS.items():
        v[f"ov/{name}"] = rr.overlay_depth(overlay_before(*OVERLAY_FIXTURE_SURFACE), row["alpha"], v[f"ov_depth/{row['image']}"], DEPTH_SCALE,
                                           row["fov_axis"], row["zoom"], row["center"])
    return v


def members(v):
    for name in sorted(v):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.ascontiguousarray(v[name]), version=(1, 0), allow_pickle=False)
        yield name + ".npy", buf.getvalue()


def write(path):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, data in members(vectors()):
            info = zipfile.ZipInfo(name, date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, data, compresslevel=9)


def read_members(path):
    with zipfile.ZipFile(path) as z:
        return [(i.filename, z.read(i)) for i in z.infolist()]


if __name__ == "__main__":
    target = Path(__file__).with_name("reference_render_buffer.npz")
    write(target)
    print(f"wrote {target.name}: {target.stat().st_size} bytes")
