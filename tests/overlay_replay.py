"""A numpy replay of csrc/nrf_overlay_plan.h -- TEST INFRASTRUCTURE ONLY: the render buffer's image overlay, false-colour overlay and
error map (nrf_rb_overlay_image, nrf_rb_overlay_false_color, nrf_rb_error_map) as include/nerfhip.h defines them, fp32 throughout,
every operation one rounding in the header's order, integer cell bounds, the lane and tree order of the reduction, the saturating
float-to-int conversion as a range test before the cast.

The power inside the sRGB pair is libm's, not numpy's: it is taken from the CPU oracle (oracle_py.rb_tonemap with exposure 0, the
identity curve and nothing behind an opaque plane is `x * 1.0f` after srgb_to_linear resp. linear_to_srgb); the branch without a power
is plain fp32 arithmetic and stays in numpy, which also keeps a -0.  2^exposure comes from the oracle the same way.  The Byte table is
the library's own (nerfhip.srgb8_table()), which tests/test_overlay_cpu.py holds to the reference.

Planes are float32 [H][W][4].  An image is uint32 [ih][iw] (IMG_BYTE), uint16 [ih][iw][4] of fp16 bit patterns (IMG_HALF) or float32
[ih][iw][4] (IMG_FLOAT)."""
from __future__ import annotations

import numpy as np

import oracle_py as op

F = np.float32
CS_LINEAR, CS_SRGB, CS_VISPOSNEG = 0, 1, 2
TM_IDENTITY, TM_ACES, TM_HABLE, TM_REINHARD = 0, 1, 2, 3
IMG_BYTE, IMG_HALF, IMG_FLOAT = 1, 2, 3
INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
MAGIC_TEXEL = 0x00FF00FF
_ERR = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """bit for bit, a NaN matching any NaN (which payload and sign an operation hands on is the machine's choice)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def mismatches(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.argwhere(~((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------- colour
def _through_oracle(v, render_space, display_space, exposure=0.0):
    v = np.ascontiguousarray(v, np.float32)
    flat = v.reshape(-1)
    pad = (-flat.size) % 3
    rgb = np.concatenate([flat, np.zeros(pad, np.float32)]).reshape(-1, 3)
    plane = np.concatenate([rgb, np.ones((len(rgb), 1), np.float32)], axis=1)
    out = op.rb_tonemap(plane, exposure, [0.0, 0.0, 0.0, 0.0], render_space, display_space, TM_IDENTITY)
    return out[:, :3].reshape(-1)[:flat.size].reshape(v.shape)


def decode_srgb(v):
    v = np.asarray(v, np.float32)
    with np.errstate(**_ERR):
        return np.where(v <= F(0.04045), v / F(12.92), _through_oracle(v, CS_SRGB, CS_LINEAR)).astype(np.float32)


def encode_srgb(v):
    v = np.asarray(v, np.float32)
    with np.errstate(**_ERR):
        return np.where(v < F(0.0031308), F(12.92) * v, _through_oracle(v, CS_LINEAR, CS_SRGB)).astype(np.float32)


def gain(exposure):
    """powf(2, exposure[k]) per channel, libm's"""
    e = np.broadcast_to(np.asarray(exposure, np.float32), (3,))
    return np.array([_through_oracle(np.ones(3, np.float32), CS_LINEAR, CS_LINEAR, float(x))[0] for x in e], np.float32)


def film_constants(curve):
    """(kind, n2, n1, n0, d2, d1, d0) of film_curve(), the products in fp32 from the left as the compiler folds them"""
    if curve == TM_ACES:
        return ("rational", F(0.6) * F(0.6) * F(2.51), F(0.6) * F(0.03), F(0.0), F(0.6) * F(0.6) * F(2.43), F(0.6) * F(0.59), F(0.14))
    if curve == TM_HABLE:
        A, B, C, D, E, Fc, white = F(0.15), F(0.50), F(0.10), F(0.20), F(0.02), F(0.30), F(11.2)
        n2, n1, n0 = A * Fc - A * E, C * B * Fc - B * E, F(0.0)
        d2, d1, d0 = A * Fc, B * Fc, D * Fc * Fc
        at_white_n = n2 * (white * white) + n1 * white + n0
        at_white_d = d2 * (white * white) + d1 * white + d0
        norm = at_white_d / at_white_n
        return ("rational", F(4.0) * n2 * norm, F(2.0) * n1 * norm, n0 * norm, F(4.0) * d2, F(2.0) * d1, d0)
    if curve == TM_REINHARD:
        return ("luma",) + (F(0.0),) * 6
    return ("none",) + (F(0.0),) * 6


def tonemap(c, exposure, curve, render_space, display_space):
    """the reference's five-argument tonemap on colours [..., 3] (develop_color)"""
    c = np.array(c, np.float32)
    g = gain(exposure)
    with np.errstate(**_ERR):
        if render_space == CS_SRGB:
            c = decode_srgb(c)
        c = c * g
        kind, n2, n1, n0, d2, d1, d0 = film_constants(curve)
        if kind != "none":
            c = np.where(c > 0, c, F(0.0)).astype(np.float32)  # the device's fmaxf(x, 0): a NaN and a -0 give +0
            if kind == "luma":
                scale = F(1.0) / ((F(0.2126) * c[..., 0] + (F(0.7152) * c[..., 1] + F(0.0722) * c[..., 2])) + F(1.0))
                c = c * scale[..., None]
            else:
                sq = c * c
                c = (sq * n2 + n1 * c + n0) / (d2 * sq + d1 * c + d0)
        if display_space == CS_SRGB:
            c = encode_srgb(c)
    return c.astype(np.float32)


def saturate(x):
    x = np.asarray(x, np.float32)
    return np.where(x > 0, np.where(x > 1, F(1.0), x), F(0.0)).astype(np.float32)


def colormap_turbo(x):
    kR4, kG4, kB4 = F([0.13572138, 4.61539260, -42.66032258, 132.13108234]), F([0.09140261, 2.19418839, 4.84296658, -14.18503333]), \
        F([0.10667330, 12.64194608, -60.58204836, 110.36276771])
    kR2, kG2, kB2 = F([-152.94239396, 59.28637943]), F([4.27729857, 2.82956604]), F([-89.90310912, 27.34824973])
    x = np.fmin(np.fmax(np.asarray(x, np.float32), F(0.0)), F(1.0))
    x = np.where(np.isnan(x), F(0.0), x).astype(np.float32)
    x2 = x * x
    x3 = x2 * x
    v20, v21 = x3 * x, x3 * x2
    one = np.ones_like(x)
    dot4 = lambda a: (a[0] * one + a[1] * x) + (a[2] * x2 + a[3] * x3)  # noqa: E731
    return np.stack([dot4(a4) + (v20 * a2[0] + v21 * a2[1]) for a4, a2 in ((kR4, kR2), (kG4, kG2), (kB4, kB2))], axis=-1).astype(np.float32)


_VIRIDIS = F([[0.2777273272234177, 0.005407344544966578, 0.3340998053353061],
              [0.1050930431085774, 1.404613529898575, 1.384590162594685],
              [-0.3308618287255563, 0.214847559468213, 0.09509516302823659],
              [-4.634230498983486, -5.799100973351585, -19.33244095627987],
              [6.228269936347081, 14.17993336680509, 56.69055260068105],
              [4.776384997670288, -13.74514537774601, -65.35303263337234],
              [-5.435455855934631, 4.645852612178535, 26.3124352495832]])


def colormap_viridis(x):
    x = saturate(x)[..., None]
    h = np.broadcast_to(_VIRIDIS[6], x.shape[:-1] + (3,)).astype(np.float32)
    for i in range(5, -1, -1):
        h = _VIRIDIS[i] + x * h
    return h.astype(np.float32)


# ---------------------------------------------------------------- the pixel mapping
def index(floored):
    """a floored coordinate as an index: saturating, a NaN outside every image"""
    f = np.asarray(floored, np.float32)
    out = np.full(f.shape, INT_MIN, np.int64)
    high = f >= F(2147483648.0)
    mid = (f >= F(-2147483648.0)) & ~high
    out[mid] = f[mid].astype(np.int64)
    out[high] = INT_MAX
    return out


def source(W, H, iw, ih, fov_axis, zoom, center):
    """(srcx, srcy), int64 [H][W] each: overlay_depth_kernel's mapping"""
    zoom, cx, cy = F(zoom), F(center[0]), F(center[1])
    with np.errstate(**_ERR):
        scale = F(iw if fov_axis == 0 else ih) / F(W if fov_axis == 0 else H)

        def axis(n, c, size):
            f = np.arange(n, dtype=np.float32) + F(0.5)
            f = f - F(n) * F(0.5)
            f = f / zoom
            f = f + c * F(n)
            u = (f - F(n) * F(0.5)) * scale + F(size) * F(0.5)
            return index(np.floor(u))

        sx, sy = axis(W, cx, iw), axis(H, cy, ih)
    return np.broadcast_to(sx[None, :], (H, W)), np.broadcast_to(sy[:, None], (H, W))


def inside(srcx, srcy, w, h):
    return ~((srcx >= w) | (srcy >= h) | (srcx < 0) | (srcy < 0))


# ---------------------------------------------------------------- read_rgba
def read_rgba(image, image_data_type, table):
    """every texel of an image as float32 [ih][iw][4]"""
    if image_data_type == IMG_BYTE:
        t = np.ascontiguousarray(image, np.uint32)
        b = [(t >> (8 * k)) & 0xFF for k in range(4)]
        a = b[3].astype(np.float32) * (F(1.0) / F(255.0))
        table = np.asarray(table, np.float32)
        out = np.stack([table[b[0]] * a, table[b[1]] * a, table[b[2]] * a, a], axis=-1).astype(np.float32)
        out[t == MAGIC_TEXEL] = F(-1.0)
        return out
    if image_data_type == IMG_HALF:
        return np.ascontiguousarray(image, np.uint16).view(np.float16).astype(np.float32)
    assert image_data_type == IMG_FLOAT
    return np.ascontiguousarray(image, np.float32)


# ---------------------------------------------------------------- the image overlay
def overlay_image(surface, alpha, exposure, background_color, render_space, display_space, curve, image, image_data_type, table,
                  fov_axis=0, zoom=1.0, center=(0.5, 0.5)):
    surface = np.ascontiguousarray(surface, np.float32)
    H, W = surface.shape[:2]
    texels = read_rgba(image, image_data_type, table)
    ih, iw = texels.shape[:2]
    srcx, srcy = source(W, H, iw, ih, fov_axis, zoom, center)
    ok = inside(srcx, srcy, iw, ih)
    val = np.zeros((H, W, 4), np.float32)
    val[ok] = texels[srcy[ok], srcx[ok]]
    bg = np.asarray(background_color, np.float32).reshape(4)
    alpha = F(alpha)
    with np.errstate(**_ERR):
        c, w = val[..., :3], val[..., 3]
        if render_space == CS_SRGB:
            wide = w[..., None]
            c = np.where(wide > 0, encode_srgb(c / wide) * wide, F(0.0)).astype(np.float32)
            bg_rgb = bg[:3]
        else:
            bg_rgb = decode_srgb(bg[:3])
        weight = (F(1.0) - w) * bg[3]
        c = c + bg_rgb * weight[..., None]
        w = w + weight
        c = tonemap(c, exposure, curve, render_space, display_space)
        color = np.concatenate([c, w[..., None]], axis=-1)
        out = color * alpha + surface * (F(1.0) - alpha)
    return out.astype(np.float32)


# ---------------------------------------------------------------- the false-colour overlay
def false_color_source(W, H, tw, th, mw, mh, fov_axis):
    with np.errstate(**_ERR):
        scale = F(tw if fov_axis == 0 else th) / F(W if fov_axis == 0 else H)

        def axis(n, t, m):
            u = (np.arange(n, dtype=np.float32) + F(0.5) - F(n) * F(0.5)) * scale + F(t) * F(0.5)
            return index(np.floor(u * F(m) / max(F(1.0), F(t))))

        sx, sy = axis(W, tw, mw), axis(H, th, mh)
    return np.broadcast_to(sx[None, :], (H, W)), np.broadcast_to(sy[:, None], (H, W))


def overlay_false_color(surface, training_width, training_height, fov_axis, error_map, average, brightness, viridis):
    surface = np.ascontiguousarray(surface, np.float32)
    error_map = np.ascontiguousarray(error_map, np.float32)
    H, W = surface.shape[:2]
    mh, mw = error_map.shape
    srcx, srcy = false_color_source(W, H, training_width, training_height, mw, mh, fov_axis)
    ok = inside(srcx, srcy, mw, mh)
    out = surface.copy()
    with np.errstate(**_ERR):
        error_map_scale = F(brightness) / (F(0.0000001) + F(average))
        err = error_map[srcy[ok], srcx[ok]] * error_map_scale
        if viridis:
            err = err * (F(1.0) / (F(1.0) + err))
        c = colormap_viridis(err) if viridis else colormap_turbo(err)
        color = surface[ok]
        grey = color[:, 0] * F(0.2126) + color[:, 1] * F(0.7152) + color[:, 2] * F(0.0722)
        rgb = grey[:, None] * saturate(c)
    out[ok] = np.concatenate([rgb, color[:, 3:4]], axis=-1)
    return out


# ---------------------------------------------------------------- the error map
def cell_begins(n, m):
    """x0(c) for c = 0 .. m"""
    return (np.arange(m + 1, dtype=np.int64) * n + m - 1) // m


def wave_sum(a):
    """the wave's order over the last axis: lane l adds elements l, l + 64, ... in ascending order onto 0, then the tree 32 .. 1"""
    a = np.ascontiguousarray(a, np.float32)
    count = a.shape[-1]
    v = np.zeros(a.shape[:-1] + (64,), np.float32)
    with np.errstate(**_ERR):
        for first in range(0, count, 64):
            seg = a[..., first:first + 64]
            n = seg.shape[-1]
            v[..., :n] = v[..., :n] + seg
        s = 32
        while s >= 1:
            v[..., :s] = v[..., :s] + v[..., s:2 * s]
            s //= 2
    return v[..., 0].copy()


def error_map(surface, truth, mw, mh):
    """(map float32 [mh][mw], average float32)"""
    S, G = np.ascontiguousarray(surface, np.float32), np.ascontiguousarray(truth, np.float32)
    H, W = S.shape[:2]
    assert 1 <= mw <= min(W, 512) and 1 <= mh <= min(H, 512)
    with np.errstate(**_ERR):
        d = S[..., :3] - G[..., :3]
        e = (((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])) / F(3.0)
    x0, y0 = cell_begins(W, mw), cell_begins(H, mh)
    cws, chs = np.diff(x0), np.diff(y0)
    assert cws.min() >= 1 and chs.min() >= 1 and x0[-1] == W and y0[-1] == H
    out = np.empty((mh, mw), np.float32)
    for cw in np.unique(cws):          # cells of one shape together: at most two widths and two heights
        cxs = np.nonzero(cws == cw)[0]
        cols = x0[cxs][:, None] + np.arange(cw)[None, :]
        for ch in np.unique(chs):
            cys = np.nonzero(chs == ch)[0]
            rows = y0[cys][:, None] + np.arange(ch)[None, :]
            block = e[rows[:, None, :, None], cols[None, :, None, :]]  # [cells down][cells across][ch][cw]: row-major inside a cell
            with np.errstate(**_ERR):
                out[np.ix_(cys, cxs)] = wave_sum(block.reshape(len(cys), len(cxs), int(ch * cw))) / F(int(ch * cw))
    with np.errstate(**_ERR):
        average = wave_sum(out.reshape(-1)) / F(mw * mh)
    return out, F(average)
