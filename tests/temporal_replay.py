"""The render buffer's temporal upscaler (nrf_rb_upscale_temporal), its jitter sequence and the motion vectors of a static scene
(nrf_motion_vectors) replayed in numpy: the definition in include/nerfhip.h, float32 throughout, one rounding per operation (numpy fuses
nothing), np.fmin / np.fmax for the clamps.  It builds on tests/upscale_replay.py.  host/temporal_plan_check.cpp
(csrc/nrf_temporal_plan.h, the text the kernels compile) is held to it bit for bit by tests/test_temporal_cpu.py, and the GPU tests hold
the library to it."""
import numpy as np

import upscale_replay as ur

F = np.float32
RESET, RECTIFY = 1, 2
HISTORY_DEFAULT = 64.0
WEIGHT_FLOOR = F(0.015625)


def _axis(n_in, n_out, j):
    """per output index of one axis: the clamped taps [n_out][4], the weights [n_out][4], the nearest texel n and the scaled distance d"""
    r = F(n_in) / F(n_out)
    o = F(n_out) / F(n_in)
    centre = np.arange(n_out).astype(np.float32) + F(0.5)
    s = (centre * r - F(0.5)) - F(j)
    fl = np.floor(s)
    i = fl.astype(np.int64)
    f = s - fl
    taps = np.clip(i[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    n = np.clip(np.floor(s + F(0.5)).astype(np.int64), 0, n_in - 1)
    d = (s - n.astype(np.float32)) * o
    return taps, ur.weights(f), n, d.astype(np.float32)


def _reconstruct(P, cy, wy, cx, wx):
    """stage 1 of the spatial upscaler at per-pixel taps and weights: cy, cx [h][w][4] indices, wy, wx [h][w][4] weights -> [h][w][4]"""
    wxs = [wx[..., a, None] for a in range(4)]
    wys = [wy[..., a, None] for a in range(4)]
    with np.errstate(all="ignore"):
        tap = [[P[cy[..., j], cx[..., a]] for a in range(4)] for j in range(4)]
        h = [ur._dot4(wxs, *tap[j]) for j in range(4)]
        v = ur._dot4(wys, *h)
        lo = np.fmin(np.fmin(tap[1][1], tap[1][2]), np.fmin(tap[2][1], tap[2][2]))
        hi = np.fmax(np.fmax(tap[1][1], tap[1][2]), np.fmax(tap[2][1], tap[2][2]))
        return np.fmin(np.fmax(v, lo), hi).astype(np.float32)


def current(plane, out_w, out_h, jitter):
    """(C [out_h][out_w][4], wc [out_h][out_w], nx [out_w], ny [out_h]) of the surface `plane` sampled with `jitter`"""
    P = np.ascontiguousarray(plane, np.float32)
    ih, iw = P.shape[:2]
    assert P.shape == (ih, iw, 4) and ur.axis_valid(iw, out_w) and ur.axis_valid(ih, out_h)
    cx, wx, nx, dx = _axis(iw, out_w, jitter[0])
    cy, wy, ny, dy = _axis(ih, out_h, jitter[1])
    shape = (out_h, out_w, 4)
    C = _reconstruct(P, np.broadcast_to(cy[:, None, :], shape), np.broadcast_to(wy[:, None, :], shape),
                     np.broadcast_to(cx[None, :, :], shape), np.broadcast_to(wx[None, :, :], shape))
    with np.errstate(all="ignore"):
        a = (dx * dx)[None, :] + (dy * dy)[:, None]
        b = np.fmax(F(1.0) - a, F(0.0))
        wc = np.fmax(b * b, WEIGHT_FLOOR).astype(np.float32)
    return C, wc, nx, ny


def fetch_history(H, Wt, motion, nx, ny):
    """(Hq [oh][ow][4], Wq [oh][ow]) of the previous planes through the motion plane [ih][iw][2] (or None); Wq = 0 where there is none"""
    oh, ow = Wt.shape
    if motion is None:
        return H.copy(), Wt.copy()
    m = np.ascontiguousarray(motion, np.float32)[ny[:, None], nx[None, :]]       # [oh][ow][2]
    mx, my = m[..., 0], m[..., 1]
    static = (mx == 0) & (my == 0)
    with np.errstate(all="ignore"):
        qx = np.arange(ow).astype(np.float32)[None, :] + mx
        qy = np.arange(oh).astype(np.float32)[:, None] + my
        ok = np.isfinite(mx) & np.isfinite(my) & (qx >= F(-0.5)) & (qx <= F(ow) - F(0.5)) & (qy >= F(-0.5)) & (qy <= F(oh) - F(0.5)) & ~static
    qx, qy = np.where(ok, qx, F(0)), np.where(ok, qy, F(0))
    flx, fly = np.floor(qx), np.floor(qy)
    span = np.arange(-1, 3)
    tx = np.clip(flx.astype(np.int64)[..., None] + span, 0, ow - 1)
    ty = np.clip(fly.astype(np.int64)[..., None] + span, 0, oh - 1)
    vx = ur.weights((qx - flx).reshape(-1)).reshape(oh, ow, 4)
    vy = ur.weights((qy - fly).reshape(-1)).reshape(oh, ow, 4)
    Hr = _reconstruct(H, ty, vy, tx, vx)
    wx = np.clip(np.floor(qx + F(0.5)).astype(np.int64), 0, ow - 1)
    wy = np.clip(np.floor(qy + F(0.5)).astype(np.int64), 0, oh - 1)
    Wr = Wt[wy, wx]
    Hq = np.where(static[..., None], H, Hr)
    Wq = np.where(static, Wt, np.where(ok, Wr, F(0))).astype(np.float32)
    return Hq.astype(np.float32), Wq


def rectify(Hq, plane, nx, ny):
    P = np.ascontiguousarray(plane, np.float32)
    ih, iw = P.shape[:2]
    lo = hi = None
    for j in (-1, 0, 1):
        for a in (-1, 0, 1):
            t = P[np.clip(ny + j, 0, ih - 1)[:, None], np.clip(nx + a, 0, iw - 1)[None, :]]
            lo, hi = (t, t) if lo is None else (np.fmin(lo, t), np.fmax(hi, t))
    return np.fmin(np.fmax(Hq, lo), hi).astype(np.float32)


class Temporal:
    """the state of one buffer: step() is one nrf_rb_upscale_temporal"""

    def __init__(self, out_w, out_h, amount=0.0, max_history=HISTORY_DEFAULT):
        self.ow, self.oh, self.amount, self.max_history = out_w, out_h, amount, F(max_history)
        self.H = np.zeros((out_h, out_w, 4), np.float32)
        self.Wt = np.zeros((out_h, out_w), np.float32)
        self.n_frames = 0

    def step(self, plane, jitter=(0.0, 0.0), motion=None, flags=0):
        """-> (presented [oh][ow][4], rgba8 [oh][ow]); self.H, self.Wt are H' and Wt'"""
        assert all(np.isfinite(j) and -0.5 <= j <= 0.5 for j in jitter) and not flags & ~3
        C, wc, nx, ny = current(plane, self.ow, self.oh, jitter)
        if self.n_frames == 0 or flags & RESET:
            Hq, Wq = C, np.zeros_like(wc)
        else:
            Hq, Wq = fetch_history(self.H, self.Wt, motion, nx, ny)
        with np.errstate(all="ignore"):
            wh = np.fmin(Wq, self.max_history)
            use = wh > 0
            if flags & RECTIFY:
                Hq = rectify(Hq, plane, nx, ny)
            tot = wh + wc
            alpha = (wc / tot)[..., None]
            blended = Hq + alpha * (C - Hq)
        self.H = np.where(use[..., None], blended, C).astype(np.float32)
        self.Wt = np.where(use, tot, wc).astype(np.float32)
        self.n_frames += 1
        out = ur.sharpen(self.H, self.amount)
        return out, ur.rgba8(out)


def halton(index, base):
    f, r, i = F(1.0), F(0.0), int(index)
    while i > 0:
        f = f / F(base)
        r = r + f * F(i % base)
        i //= base
    return F(r)


def jitter(k):
    return (halton(k + 1, 2) - F(0.5), halton(k + 1, 3) - F(0.5))


def camera(pose, scale, cam):
    """(R [3][3], c [3], cam [4]) in ngp form, as nrf_render converts a pose"""
    p = np.asarray(pose, np.float32).reshape(4, 4)
    R, c = np.zeros((3, 3), np.float32), np.zeros(3, np.float32)
    for r, row in enumerate((1, 2, 0)):
        R[r] = [p[row, 0], -p[row, 1], -p[row, 2]]
        c[r] = p[row, 3] * F(scale) + F(0.0)
    return R, c, np.asarray(cam, np.float32)


def _project(K, v):
    R, _, cam = K
    with np.errstate(all="ignore"):
        p = [(R[0, k] * v[..., 0] + R[1, k] * v[..., 1]) + R[2, k] * v[..., 2] for k in range(3)]
        ok = np.isfinite(p[2]) & (p[2] > 0)
        u = (p[0] / p[2]) * cam[0] + cam[2]
        w = (p[1] / p[2]) * cam[1] + cam[3]
    return ok, u, w


def motion_vectors(rays_o, rays_d, alpha, depth, out_w, out_h, min_alpha, cur, prev):
    """float32 [h][w][2] of rays [h][w][3], alpha and depth [h][w]; cur / prev from camera()"""
    o, d = np.asarray(rays_o, np.float32), np.asarray(rays_d, np.float32)
    alpha, depth = np.asarray(alpha, np.float32), np.asarray(depth, np.float32)
    h, w = alpha.shape
    assert ur.axis_valid(w, out_w) and ur.axis_valid(h, out_h) and 0 < min_alpha <= 1
    ox, oy = F(out_w) / F(w), F(out_h) / F(h)
    with np.errstate(all="ignore"):
        t = depth / alpha
        near = (alpha >= F(min_alpha)) & np.isfinite(t) & (t > 0)
        x = o + t[..., None] * d
        vc = np.where(near[..., None], x - cur[1], d)
        vp = np.where(near[..., None], x - prev[1], d)
        okc, uc, wc = _project(cur, vc)
        okp, up, wp = _project(prev, vp)
        ok = okc & okp & np.all(np.isfinite(o), axis=-1) & np.all(np.isfinite(d), axis=-1)
        m = np.stack([(up - uc) * ox, (wp - wc) * oy], axis=-1)
    return np.where(ok[..., None], m, F(np.inf)).astype(np.float32)
