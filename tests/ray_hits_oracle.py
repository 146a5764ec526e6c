"""The checker for nrf_ray_hits: tests/rays_oracle.py's per-ray loop, stopped at the first sample whose updated weight sum
reaches an opacity threshold -- TEST INFRASTRUCTURE ONLY.

rays_oracle.render is run as it is (imported, not copied) through a proxy in the style of rays_clip_oracle._StateKeeper.  The loop
calls composite with n_step = 1, so a call holds at most one sample per live ray (deltas[:, 0, 0] != 0: the march emitted one):

    the crossing sample   where the NEW state[:, 0] (the updated weight sum) is >= opacity, the proxy records
                          (tc, dt, old state[:, 0], new state[:, 0]) with tc = fp32(rays_t + deltas[:, 0, 1]) -- the t the sample is
                          composited at, the end of its interval -- and returns t_new = -1 for that ray, so the loop drops it
    the margin            per ray, the smallest |ws - opacity| over all its composited samples: a ray whose margin is large is
                          hit or missed whatever the last bits of the density are
    near / far            through the clamp of rays_clip_oracle

A ray that never reaches the threshold keeps (0, 0, 0, final weight sum); a ray that is never alive keeps zeros.  depth is
state[:, 1] as accumulated (NRF_RAYS_DEPTH_T semantics)."""
from __future__ import annotations

import numpy as np

import nerfhip as nh
import rays_clip_oracle as rco
import rays_oracle as ro


class _HitKeeper:
    """The oracle as rays_oracle.render sees it: stops a ray at its crossing sample and keeps its record."""

    def __init__(self, oracle, n, opacity):
        self._oracle = oracle
        self.opacity = np.float32(opacity)
        self.alive = None  # set by the near_far wrapper: the loop's alive list starts as flatnonzero(near < far)
        self.state = np.zeros((n, 5), np.float32)
        self.rec = np.zeros((n, 4), np.float32)
        self.hit = np.zeros(n, bool)
        self.margin = np.full(n, np.inf, np.float32)
        self.n_composited = 0

    def march(self, *a, **kw):
        return self._oracle.march(*a, **kw)

    def network(self, *a, **kw):
        return self._oracle.network(*a, **kw)

    def composite(self, sigmas, rgbs, deltas, rays_t, state):
        t_new, st_new = self._oracle.composite(sigmas, rgbs, deltas, rays_t, state)
        idx = self.alive
        assert len(st_new) == len(idx)
        found = deltas[:, 0, 0] != 0
        self.n_composited += int(found.sum())
        tc = (np.asarray(rays_t, np.float32) + deltas[:, 0, 1]).astype(np.float32)
        ws = st_new[:, 0]
        self.state[idx] = st_new
        self.margin[idx[found]] = np.minimum(self.margin[idx[found]], np.abs(ws - self.opacity)[found])
        h = found & (ws >= self.opacity)
        self.hit[idx[h]] = True
        self.rec[idx[h], 0] = tc[h]
        self.rec[idx[h], 1] = deltas[h, 0, 0]
        self.rec[idx[h], 2] = np.asarray(state, np.float32)[h, 0]
        t_new = np.where(h, np.float32(-1), t_new).astype(np.float32)
        self.alive = idx[t_new >= 0]  # (as the loop itself does)
        return t_new, st_new


class Hits:
    """records [n][4], depth [n] (the raw sum of w * t), hit [n] bool, margin [n], n_composited"""

    def __init__(self, keeper):
        self.records = keeper.rec
        self.records[:, 3] = keeper.state[:, 0]
        self.depth = keeper.state[:, 1].copy()
        self.hit = keeper.hit
        self.margin = keeper.margin
        self.n_composited = keeper.n_composited


def ray_hits(oracle, desc, rays_o, rays_d, opacity, opts=None, t_min=None, t_max=None) -> Hits:
    opts = opts or nh.default_options()
    n = len(np.asarray(rays_o).reshape(-1, 3))
    keeper = _HitKeeper(oracle, n, opacity)
    plain = ro.near_far

    def clamped(aabb, o, d, min_near):
        near, far = rco.clamp(*plain(aabb, o, d, min_near), t_min, t_max)
        keeper.alive = np.flatnonzero(near < far)
        return near, far

    ro.near_far = clamped
    try:
        _, _, n_samples = ro.render(keeper, desc, rays_o, rays_d, opts)
    finally:
        ro.near_far = plain
    assert n_samples == keeper.n_composited
    h = Hits(keeper)
    assert np.all(h.records[h.hit, 3] >= np.float32(opacity)) and np.all(h.records[~h.hit, 3] < np.float32(opacity))
    return h


def lowered(records, ulps=4):
    """fp32(t - dt) of the records, lowered by `ulps` ulps: a t_max just below the start of the crossing sample.  The march emits a
    sample when its start t_s < far and composites it at tc = fp32(t_s + dt), so fp32(tc - dt) is within about an ulp of t_s, and dt
    (>= 0.0034) is far larger than that: the limit cuts the crossing sample and keeps the one before it."""
    s = (records[:, 0] - records[:, 1]).astype(np.float32)
    for _ in range(ulps):
        s = np.nextafter(s, np.float32(-np.inf))
    return s.astype(np.float32)
