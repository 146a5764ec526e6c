"""The checker for nrf_render_rays_clipped: tests/rays_oracle.py's per-ray loop between per-ray limits of t, over a per-ray
background -- TEST INFRASTRUCTURE ONLY.

rays_oracle.render is run as it is (imported, not copied), with three changes made from outside:

    the clamp        rays_oracle.near_far is wrapped for the length of the call:  near = where(t_min > near, t_min, near),
                     far = where(t_max < far, t_max, far)  -- `if (t_min > near) near = t_min; if (t_max < far) far = t_max`, so a
                     NaN limit is no limit.  The loop's alive list (near < far), its march bound and its depth normalisation all
                     take the clamped pair, because they all take what near_far returned.
    the background   the loop runs with bg_color = 0, which makes its rgb planes the composited colour c exactly (c + 0); the
                     epilogue  rgb[k] = c[k] + (1 - weight_sum) * background[ray][k]  follows here, every operation rounded to fp32.
    the raw depth    the oracle handed to the loop is a proxy that forwards march / network / composite and keeps the state rows
                     composite returns: state[:, 1] (the accumulated sum of w * t) is returned beside the normalised depth.

With no limits and no background array this is rays_oracle.render bit for bit (tests/test_render_rays_clip_cpu.py)."""
from __future__ import annotations

import copy

import numpy as np

import nerfhip as nh
import rays_oracle as ro


def clamp(near, far, t_min=None, t_max=None):
    """The clamp of nrf_render_rays_clipped on fp32 arrays (None: no limit)."""
    near, far = np.asarray(near, np.float32), np.asarray(far, np.float32)
    with np.errstate(invalid="ignore"):
        if t_min is not None:
            t_min = np.asarray(t_min, np.float32).reshape(-1)
            near = np.where(t_min > near, t_min, near)
        if t_max is not None:
            t_max = np.asarray(t_max, np.float32).reshape(-1)
            far = np.where(t_max < far, t_max, far)
    return near.astype(np.float32), far.astype(np.float32)


def near_far(desc, rays_o, rays_d, min_near, t_min=None, t_max=None):
    """(near', far') per ray: rays_oracle.near_far, then the clamp."""
    near, far = ro.near_far([desc.aabb[i] for i in range(6)], rays_o, rays_d, min_near)
    return clamp(near, far, t_min, t_max)


class _StateKeeper:
    """The oracle as rays_oracle.render sees it, remembering every ray's last composited state."""

    def __init__(self, oracle, n):
        self._oracle = oracle
        self.state = np.zeros((n, 5), np.float32)
        self.alive = None  # set by the near_far wrapper: the loop's alive list starts as flatnonzero(near < far)

    def march(self, *a, **kw):
        return self._oracle.march(*a, **kw)

    def network(self, *a, **kw):
        return self._oracle.network(*a, **kw)

    def composite(self, sigmas, rgbs, deltas, rays_t, state):
        t_new, st_new = self._oracle.composite(sigmas, rgbs, deltas, rays_t, state)
        assert len(st_new) == len(self.alive)
        self.state[self.alive] = st_new
        self.alive = self.alive[t_new >= 0]  # (as the loop itself does)
        return t_new, st_new


def render(oracle, desc, rays_o, rays_d, opts=None, t_min=None, t_max=None, background=None):
    """rgba [n][4], normalised depth [n], samples, raw depth state[:, 1] [n] for n rays between their limits of t."""
    opts = opts or nh.default_options()
    n = len(np.asarray(rays_o).reshape(-1, 3))
    keeper = _StateKeeper(oracle, n)
    plain = ro.near_far

    def clamped(aabb, o, d, min_near):
        near, far = clamp(*plain(aabb, o, d, min_near), t_min, t_max)
        keeper.alive = np.flatnonzero(near < far)
        return near, far

    black = copy.copy(opts)
    black.bg_color = 0.0
    ro.near_far = clamped
    try:
        rgba, depth, n_samples = ro.render(keeper, desc, rays_o, rays_d, black)
    finally:
        ro.near_far = plain
    ws = rgba[:, 3]
    assert np.array_equal(ws.view(np.uint32), keeper.state[:, 0].view(np.uint32))
    if background is None:
        bg = np.full((n, 3), np.float32(opts.bg_color), np.float32)
    else:
        bg = np.ascontiguousarray(background, np.float32).reshape(n, 3)
    out = rgba.copy()
    T = (np.float32(1) - ws).astype(np.float32)
    for k in range(3):
        out[:, k] = rgba[:, k] + (T * bg[:, k]).astype(np.float32)
    return out, depth, n_samples, keeper.state[:, 1].copy()


def ramp(W, H, lo=0.7, span=0.9):
    """The limit the tests use: t(px) = lo + span * px / W along the columns, row-major [H * W]."""
    t = np.float32(lo) + np.float32(span) * np.arange(W, dtype=np.float32) / np.float32(W)
    return np.ascontiguousarray(np.broadcast_to(t.astype(np.float32), (H, W))).reshape(-1)
