"""A float64 restatement of the compositor for frames of fog probe models (helper of test_fog_cpu.py, test_fog_gpu.py and the
chained nrf_composite test; numpy only, no test in it).

A fog probe model (probe_model.probe_desc with sigma_weight 1 .. 4.5) has per-sample rgb and sigma that are exact fp16 values,
the same bits in the kernel and in the oracle: the MLP sums have one non-zero product and the grid encoding is bit-exact.
What may differ between two fp32 implementations of a frame is the compositing chain and its exp alone.  This file states
that chain in float64 on the fp32 inputs, and the bound within which any fp32 evaluation of it must stay.

The samples of a ray: the oracle's march with n_step = 1, called again and again with rays_t += deltas[1] in fp32 -- what the
per-ray schedule does (march and deltas are pinned bit for bit elsewhere).  sigma from Oracle.network (times density_scale
in fp32), rgb from probe_model.expected_values, asserted equal to Oracle.network's rgb on every sample.

The rules (the reference's kernel_composite_rays and get_image_and_depth, as oracle/nerf_oracle.cpp states them), per ray:
    alpha = 1 - exp(-sigma dt);  T = 1 - ws;  w = alpha T;  ws += w;  t += deltas[1];  depth += w t;  rgb += w c
    after a sample with T < 1e-4 the ray ends; it ends after max_steps samples, and when its march finds no sample
    pixel = rgb + (1 - ws) bg;  alpha = ws;  depth = max(depth - near, 0) / (far - near)   (0 where far <= near)

The bound of a ray with N composited samples of transmittances T_i, c_max = max(1, |its values|, bg):
    2^-22 sum_i T_i c_max                    alpha of one sample: the rounding of the exp argument and one ulp of exp, on either
                                             side, stay below 2^-22 absolute; d(pixel)/d(alpha_i) <= T_i c_max
  + N 2^-23 c_max                            the fp32 products and running sums of a sample, and the epilogue
  + [min_i T_i <= 1.1e-4] 1.1e-4 a_max c_max the stop test falling the other way: T = 1 - ws carries the rounding of a sum near
                                             1, a relative error of ~1e-3 at the threshold; either verdict is then legitimate
                                             and costs one sample of weight T alpha.  a_max runs over the ray's composited
                                             samples AND the one behind them: when the float64 chain stops and an fp32 one
                                             goes on, that is the sample it adds.
Depth: the depth sum carries t, so its error is the bound (at c_max = 1) times the ray's largest t; the epilogue divides by
far - near and rounds twice (a value <= 1: 2 * 2^-24):  depth bound = bound_1 t_max / (far - near) + 2^-23."""
from __future__ import annotations

import numpy as np

import nerfhip as nh
import probe_model as pm

F32, F64 = np.float32, np.float64
STOP = 1e-4          # `T < 1e-4` (a double literal in the reference)
WINDOW = 1.1e-4      # transmittances up to here: the stop test of an fp32 chain may fall either way
T_FLOOR = 1e-8       # the march of the restatement goes on until the float64 transmittance is below this (so that a chain with
                     # a sample removed, or another threshold, still finds the samples it needs)


class RaySamples:
    """Every sample the rays of one frame can composite, padded to [R][N]: n [R] samples per ray, sigma / dt / t [R][N] fp32
    (t: rays_t after the sample), rgb [R][N][3] fp32, near / far [R]."""

    def __init__(self, near, far, n, sigma, dt, t, rgb, g0):
        self.near, self.far, self.n, self.sigma, self.dt, self.t, self.rgb, self.g0 = near, far, n, sigma, dt, t, rgb, g0


def density_output(oracle, xyz, info):
    """g[0] of the density MLP at world positions: fp16(sigma_weight * fp16 value of the constant-1 feature); sigma =
    fp16(exp(g[0]))."""
    feat = oracle.encode_grid(pm.pos01(xyz, info["bound"])).view(np.float16)[:, info["sigma_feature"]]
    return (F32(info["sigma_weight"]) * feat.astype(F32)).astype(np.float16)


def march_samples(oracle, info, rays_o, rays_d, nears, fars, opts=None):
    """The n_step = 1 loop over all rays at once.  Rays are served while they can still contribute: a sample was found, fewer
    than max_steps + 1 samples so far (one more than the cap: the off-by-one variant needs it), float64 T >= T_FLOOR."""
    opts = opts or nh.default_options()
    R = len(nears)
    nears, fars = np.asarray(nears, F32), np.asarray(fars, F32)
    t = nears.copy()
    alive = nears < fars
    T = np.ones(R)
    ds = F32(opts.density_scale)
    cols, it = [], 0
    while alive.any() and it < int(opts.max_steps) + 1:
        # (perturb: the random shift of a ray comes from its number, the row of the march call -- all rays are passed, the
        #  finished ones at their far end, where the march emits nothing)
        idx = np.arange(R) if opts.perturb else np.flatnonzero(alive)
        xyz, dirs, deltas = oracle.march(rays_o[idx], rays_d[idx], np.where(alive[idx], t[idx], fars[idx]), fars[idx], 1, opts)
        found = (deltas[:, 0, 0] > 0) & alive[idx]
        assert np.array_equal(found, deltas[:, 0, 0] > 0)
        fi = idx[found]
        x, d = xyz[found, 0], dirs[found, 0]
        sigma, rgb = oracle.network(x, d)
        want = pm.expected_values(oracle, x, d, info)
        assert np.array_equal(rgb, want), "Oracle.network's rgb != the routed encoding values"
        g0 = density_output(oracle, x, info)
        if opts.density_scale != 1.0:
            sigma = (ds * sigma).astype(F32)
        t[fi] = (t[fi] + deltas[found, 0, 1]).astype(F32)
        dt = deltas[found, 0, 0]
        cols.append((fi, sigma, dt, t[fi].copy(), rgb, g0))
        T[fi] *= np.exp(-(sigma.astype(F64) * dt.astype(F64)))
        alive[idx[~found]] = False
        alive[fi[T[fi] < T_FLOOR]] = False
        it += 1
    N = max(len(cols), 1)
    n = np.zeros(R, np.int64)
    sigma_a, dt_a, t_a = np.zeros((R, N), F32), np.zeros((R, N), F32), np.zeros((R, N), F32)
    rgb_a, g0_a = np.zeros((R, N, 3), F32), np.zeros((R, N), np.float16)
    for k, (fi, sigma, dt, tt, rgb, g0) in enumerate(cols):
        assert np.all(n[fi] == k)  # a ray's samples are consecutive iterations
        sigma_a[fi, k], dt_a[fi, k], t_a[fi, k], rgb_a[fi, k], g0_a[fi, k] = sigma, dt, tt, rgb, g0
        n[fi] = k + 1
    return RaySamples(nears, fars, n, sigma_a, dt_a, t_a, rgb_a, g0_a)


def composite(s: RaySamples, opts=None, stop=STOP, max_steps=None, drop=None):
    """The float64 chain over every ray.  drop [R]: the index of one sample each ray leaves out (-1: none).  Returns a dict of
    per-ray arrays: ws, rgb [R][3], dep (the depth sum), count, sum_T, min_T, a_max (composited samples), c_max, t_max,
    stopped (ended by the T test), capped (ended by max_steps with a further sample at hand), next (the index of the sample
    behind the last composited one)."""
    opts = opts or nh.default_options()
    cap = int(opts.max_steps) if max_steps is None else int(max_steps)
    R, N = s.sigma.shape
    alpha = -np.expm1(-(s.sigma.astype(F64) * s.dt.astype(F64)))
    z = np.zeros(R)
    st = dict(ws=z.copy(), rgb=np.zeros((R, 3)), dep=z.copy(), count=np.zeros(R, np.int64), sum_T=z.copy(), min_T=np.ones(R),
              a_max=z.copy(), c_max=np.full(R, max(1.0, abs(float(opts.bg_color)))), t_max=z.copy(), stopped=np.zeros(R, bool),
              capped=np.zeros(R, bool), next=np.zeros(R, np.int64))
    done = s.n == 0
    for k in range(N):
        here = ~done & (k < s.n)
        if drop is not None:
            here &= drop != k
        st["capped"] |= here & (st["count"] >= cap)
        done |= st["capped"]
        here &= ~done
        if not here.any():
            if done.all():
                break
            continue
        a, T = alpha[:, k], 1.0 - st["ws"]
        w = np.where(here, a * T, 0.0)
        st["ws"] += w
        st["dep"] += w * s.t[:, k].astype(F64)
        st["rgb"] += w[:, None] * s.rgb[:, k].astype(F64)
        st["count"] += here
        st["next"] = np.where(here, k + 1, st["next"])
        st["sum_T"] += np.where(here, T, 0.0)
        st["min_T"] = np.where(here, np.minimum(st["min_T"], T), st["min_T"])
        st["a_max"] = np.where(here, np.maximum(st["a_max"], a), st["a_max"])
        st["c_max"] = np.where(here, np.maximum(st["c_max"], np.abs(s.rgb[:, k]).max(axis=1)), st["c_max"])
        st["t_max"] = np.where(here, np.maximum(st["t_max"], s.t[:, k]), st["t_max"])
        stop_now = here & (T < stop)
        st["stopped"] |= stop_now
        done |= stop_now | (here & (k + 1 >= s.n))
    return st


def bounds(s: RaySamples, st):
    """(bound [R] of rgb and alpha, depth bound [R] of the normalised depth, window [R]: rays with a T_i inside the stop window,
    bound [R] of the depth sum itself).  The sample behind a ray's last one counts for a_max and t_max."""
    R, N = s.sigma.shape
    r, k = np.arange(R), np.minimum(st["next"], N - 1)
    has = st["next"] < s.n
    behind = np.where(has, -np.expm1(-(s.sigma[r, k].astype(F64) * s.dt[r, k].astype(F64))), 0.0)
    t_max = np.maximum(st["t_max"], np.where(has, s.t[r, k].astype(F64), 0.0))
    window = (st["count"] > 0) & (st["min_T"] <= WINDOW)
    unit = 2.0 ** -22 * st["sum_T"] + st["count"] * 2.0 ** -23 + window * WINDOW * np.maximum(st["a_max"], behind)
    span = s.far.astype(F64) - s.near.astype(F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        dbound = np.where(span > 0, unit * t_max / span, 0.0) + 2.0 ** -23
    return unit * st["c_max"], dbound, window, unit * t_max


def frame(s: RaySamples, st, opts=None):
    """get_image_and_depth on the chain's sums: (rgba [R][4], depth [R]) in float64."""
    opts = opts or nh.default_options()
    bg = float(F32(opts.bg_color))
    rgba = np.concatenate([st["rgb"] + ((1.0 - st["ws"]) * bg)[:, None], st["ws"][:, None]], axis=1)
    span = s.far.astype(F64) - s.near.astype(F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(span > 0, np.maximum(st["dep"] - s.near.astype(F64), 0.0) / span, 0.0)
    return rgba, depth


def restate(oracle, info, cam, pose, W, H, opts=None):
    """One camera frame: (samples, chain, rgba [H][W][4], depth [H][W], bound, depth bound, window [H][W])."""
    o, d, nr, fr = oracle.generate_rays(cam, pose, W, H, opts)
    s = march_samples(oracle, info, o, d, nr, fr, opts)
    st = composite(s, opts)
    rgba, depth = frame(s, st, opts)
    b, db, window, _ = bounds(s, st)
    return s, st, rgba.reshape(H, W, 4), depth.reshape(H, W), b.reshape(H, W), db.reshape(H, W), window.reshape(H, W)


# --------------------------------------------------------------------------- the composite stage, chained
def chain_inputs(n, calls, n_step, seed):
    """Samples of n rays over calls * n_step slots: a valid prefix per ray (0 .. all slots), zero-filled behind it.  sigma per
    ray thin, moderate, mixed or thick (up to 400), with exact zeros (alpha == 0) and, in a quarter of the rays, one sample with
    sigma dt = 600 (alpha == 1.0f with any exp) mixed in.  Returns (n_valid, sigma, dt, step, rgb, t0)."""
    rng = np.random.default_rng(seed)
    N = calls * n_step
    n_valid = rng.integers(0, N + 1, n)
    n_valid[:n // 8] = N                       # rays with every slot used
    n_valid[n // 8:n // 4] = rng.integers(0, n_step, n // 4 - n // 8)  # rays that die in the first call, some with no sample at all
    valid = np.arange(N)[None, :] < n_valid[:, None]
    kind = rng.integers(0, 5, (n, 1))          # per ray: 0 thin, 1 mixed, 2 thick, 3 mixed with one opaque sample, 4 moderate
    kind[:n // 16] = 0                         # (thin rays with every slot used: they live through all calls)
    kind[n // 16:n // 8] = 4                   # (moderate ones: the T test ends them in the last call)
    sigma = np.where(kind == 0, rng.uniform(0, 8, (n, N)), np.where(kind == 2, rng.uniform(0, 400, (n, N)),
                     np.where(kind == 4, rng.uniform(0, 25, (n, N)), rng.uniform(0, 60, (n, N)))))
    sigma[rng.random((n, N)) < 0.1] = 0.0
    opaque = (kind == 3) & (np.arange(N)[None, :] == rng.integers(0, N, (n, 1)))
    sigma[opaque] = 2.0e4
    dt = rng.uniform(0.0034, 0.0625, (n, N))
    dt[opaque] = 0.03
    step = dt * rng.uniform(1.0, 1.5, (n, N))   # deltas[1] = t - last_t: the step, or more where the march hopped over empty cells
    rgb = rng.uniform(-1.0, 1.0, (n, N, 3))
    sigma, dt, step, rgb = (np.where(valid, sigma, 0).astype(F32), np.where(valid, dt, 0).astype(F32), np.where(valid, step, 0).astype(F32),
                            np.where(valid[..., None], rgb, 0).astype(F32))
    return n_valid, sigma, dt, step, rgb, rng.uniform(0.2, 3.0, n).astype(F32)


def check_chained_composite(name, call, n=6000, calls=3, n_step=8, seed=11):
    """`call(sigmas [n][n_step], rgbs, deltas, rays_t, state) -> (rays_t, state)` -- a composite stage -- `calls` times in a row,
    carrying `state` and `rays_t` as the reference's round loop does (a ray whose rays_t came back negative is dead: its
    later slots are zero-filled, as a compacted ray is never passed again), against the float64 chain with its bound: ws and
    rgb within `bound`, the depth sum within bound * t_max.  rays_t of a ray that lives is the fp32 sum of its steps, bit for
    bit; a ray is dead where the chain ended, except where a transmittance lies in the stop window.  Returns the worst
    error / bound of the state and of the depth sum."""
    n_valid, sigma, dt, step, rgb, t0 = chain_inputs(n, calls, n_step, seed)
    N = calls * n_step
    t, run = np.empty((n, N), F32), t0.copy()
    for k in range(N):
        run = (run + step[:, k]).astype(F32)
        t[:, k] = run
    s = RaySamples(np.zeros(n, F32), np.ones(n, F32), n_valid.astype(np.int64), sigma, dt, t, rgb, None)
    st = composite(s)
    b, _, window, sum_bound = bounds(s, st)
    ended = st["stopped"] | (n_valid < N)  # by the T test, or at a zero slot
    hit = st["count"] > 0
    # the inputs hold what they are meant to hold
    assert st["stopped"].sum() > n // 10 and (~ended).sum() > n // 20 and (n_valid == 0).sum() > 0 and window.sum() > n // 10
    assert (hit & (st["count"] < n_step)).sum() > n // 20      # rays that die in the first call with samples composited
    assert (st["stopped"] & (st["count"] > 2 * n_step)).sum() > n // 50  # ... and rays the T test ends in the third
    valid = np.arange(N)[None, :] < n_valid[:, None]
    assert (valid & (sigma == 0)).sum() > n and (sigma * dt > 30).sum() > n // 20
    deltas = np.stack([dt, step], axis=2)
    rays_t, state = t0.copy(), np.zeros((n, 5), F32)
    for j in range(calls):
        sl = slice(j * n_step, (j + 1) * n_step)
        dead = rays_t < 0
        dl = np.where(dead[:, None, None], F32(0), deltas[:, sl])
        rays_t, state = call(np.ascontiguousarray(sigma[:, sl]), np.ascontiguousarray(rgb[:, sl]), np.ascontiguousarray(dl), rays_t, state)
        assert np.all(rays_t[dead] < 0), name
    err = np.maximum(np.abs(state[:, 0] - st["ws"]), np.abs(state[:, 2:5] - st["rgb"]).max(axis=1))
    derr = np.abs(state[:, 1] - st["dep"])
    ratio, dratio = float((err[hit] / b[hit]).max()), float((derr[hit] / sum_bound[hit]).max())
    print(f"chained composite, {name}: worst error / bound state {ratio:.3f} depth sum {dratio:.3f} ({int(hit.sum())} rays, {int(window.sum())} in the stop window)")
    assert np.all(err[hit] <= b[hit]), (name, ratio)
    assert np.all(derr[hit] <= sum_bound[hit]), (name, dratio)
    assert np.all(state[~hit] == 0), name
    dead = rays_t < 0
    assert np.array_equal(dead[~window], ended[~window]), name
    live = ~dead & ~ended
    assert live.sum() > n // 20 and np.array_equal(rays_t[live], t[live, N - 1]), name
    return ratio, dratio
