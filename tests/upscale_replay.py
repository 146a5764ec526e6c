"""The render buffer's upscaler (nrf_rb_upscale) replayed in numpy: the definition in include/nerfhip.h, float32 throughout, one rounding
per operation (numpy fuses nothing), np.fmin / np.fmax for the clamps.  host/upscale_plan_check.cpp (csrc/nrf_upscale_plan.h, the text
the kernel compiles) is held to it bit for bit by tests/test_upscale_cpu.py, and the GPU tests hold nrf_rb_upscale to it."""
import numpy as np

F = np.float32
RATIO_MAX, OUT_MAX, AMOUNT_MAX = 8, 16384, 2.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def axis_valid(n_in, n_out):
    return n_in > 0 and n_in <= n_out <= RATIO_MAX * n_in and n_out <= OUT_MAX


def geometry(n_in, n_out):
    """per output index: the tap base i (int64), the fraction f (float32) and the four clamped tap indices [n_out][4]"""
    r = F(n_in) / F(n_out)
    centre = np.arange(n_out).astype(np.float32) + F(0.5)
    scaled = centre * r
    s = scaled - F(0.5)
    fl = np.floor(s)
    i = fl.astype(np.int64)
    f = s - fl
    taps = np.clip(i[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return i, f, taps


def weights(t):
    """the Catmull-Rom weights [n][4] of the fractions t [n]"""
    t = np.asarray(t, np.float32)
    half, one, two = F(0.5), F(1.0), F(2.0)
    w0 = t * (-half + t * (one - half * t))
    w1 = one + (t * t) * (F(-2.5) + F(1.5) * t)
    w2 = t * (half + t * (two - F(1.5) * t))
    w3 = (t * t) * (-half + half * t)
    return np.stack([w0, w1, w2, w3], axis=1).astype(np.float32)


def _dot4(w, p0, p1, p2, p3):
    return ((w[0] * p0 + w[1] * p1) + w[2] * p2) + w[3] * p3


def reconstruct(plane, out_w, out_h):
    """stage 1: the plane U [out_h][out_w][4] of the source plane [in_h][in_w][4]"""
    P = np.ascontiguousarray(plane, np.float32)
    ih, iw = P.shape[:2]
    assert P.shape == (ih, iw, 4) and axis_valid(iw, out_w) and axis_valid(ih, out_h)
    _, fx, cx = geometry(iw, out_w)
    _, fy, cy = geometry(ih, out_h)
    wx = [w[None, :, None] for w in weights(fx).T]      # over the columns
    wy = [w[:, None, None] for w in weights(fy).T]      # over the rows
    with np.errstate(all="ignore"):
        tap = [[P[cy[:, j]][:, cx[:, a]] for a in range(4)] for j in range(4)]   # [out_h][out_w][4] each
        h = [_dot4(wx, *tap[j]) for j in range(4)]
        v = _dot4(wy, *h)
        lo = np.fmin(np.fmin(tap[1][1], tap[1][2]), np.fmin(tap[2][1], tap[2][2]))
        hi = np.fmax(np.fmax(tap[1][1], tap[1][2]), np.fmax(tap[2][1], tap[2][2]))
        return np.fmin(np.fmax(v, lo), hi).astype(np.float32)


def sharpen(U, amount):
    """stage 2: the clamped unsharp mask of r, g, b on the plane U; alpha is U's"""
    U = np.ascontiguousarray(U, np.float32)
    oh, ow = U.shape[:2]
    ys, xs = np.arange(oh), np.arange(ow)
    c = U
    n, s = U[np.clip(ys - 1, 0, oh - 1)], U[np.clip(ys + 1, 0, oh - 1)]
    w, e = U[:, np.clip(xs - 1, 0, ow - 1)], U[:, np.clip(xs + 1, 0, ow - 1)]
    with np.errstate(all="ignore"):
        blur = ((n + s) + (w + e)) * F(0.25)
        d = c - blur
        x = c + F(amount) * d
        lo = np.fmin(np.fmin(np.fmin(np.fmin(c, n), s), w), e)
        hi = np.fmax(np.fmax(np.fmax(np.fmax(c, n), s), w), e)
        out = np.fmin(np.fmax(x, lo), hi).astype(np.float32)
    out[:, :, 3] = U[:, :, 3]
    return out


def u8(v):
    """the library's 8-bit rule: (unsigned char)(255.0 * x) in double, saturating, NaN -> 0"""
    s = 255.0 * np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(s > 0.0, np.where(s >= 255.0, 255.0, np.floor(np.where(np.isfinite(s), s, 0.0))), 0.0).astype(np.uint32)


def rgba8(plane):
    q = u8(plane)
    return (q[..., 0] | q[..., 1] << np.uint32(8) | q[..., 2] << np.uint32(16) | q[..., 3] << np.uint32(24)).astype(np.uint32)


def upscale(plane, out_w, out_h, amount):
    """(float32 [out_h][out_w][4], uint32 [out_h][out_w]) of nrf_rb_upscale on the surface `plane` [in_h][in_w][4]"""
    assert 0.0 <= float(amount) <= AMOUNT_MAX
    out = sharpen(reconstruct(plane, out_w, out_h), amount)
    return out, rgba8(out)


def bilinear64(plane, out_w, out_h):
    """bilinear interpolation on the same geometry (pixel centres, clamped borders) in float64: what the reconstruction is measured against"""
    P = np.asarray(plane, np.float64)
    ih, iw = P.shape[:2]

    def axis(n_in, n_out):
        s = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
        i = np.floor(s).astype(np.int64)
        return np.clip(i, 0, n_in - 1), np.clip(i + 1, 0, n_in - 1), s - i

    x0, x1, fx = axis(iw, out_w)
    y0, y1, fy = axis(ih, out_h)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = P[y0][:, x0] * (1 - fx) + P[y0][:, x1] * fx
    bot = P[y1][:, x0] * (1 - fx) + P[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy
