"""The arithmetic of nrf_density / nrf_density_gradient / nrf_hit_gradients replayed in numpy fp32 -- TEST INFRASTRUCTURE ONLY.

Every numpy operation on float32 arrays is one fp32 rounding, which is what the library's build (-ffp-contract=off
-fno-fast-math) makes of csrc/nrf_points_plan.h; tests/test_density_points_cpu.py holds this module to that header bit for bit
through host/points_plan_check.cpp, and the GPU tests hold the kernels to this module."""
from __future__ import annotations

import numpy as np

F = np.float32
N_TAPS = 7  # the centre, then +x, -x, +y, -y, +z, -z


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def bits(a):
    return f32(a).view(np.uint32)


def inv2h(h):
    h = F(h)
    with np.errstate(all="ignore"):
        return F(F(1.0) / F(h + h))


def taps(x, h):
    """[n][7][3]: tap 1 + 2 k replaces coordinate k by x_k + h, tap 2 + 2 k by x_k - h"""
    x = f32(x).reshape(-1, 3)
    h = F(h)
    t = np.repeat(x[:, None, :], N_TAPS, axis=1).copy()
    with np.errstate(all="ignore"):
        for k in range(3):
            t[:, 1 + 2 * k, k] = x[:, k] + h
            t[:, 2 + 2 * k, k] = x[:, k] - h
    return t


def guard(x, h, bound, n_taps=N_TAPS):
    """[n] bool: every coordinate of every tap is finite and within [-bound, bound] (n_taps = 1: the centre alone)"""
    t = taps(x, h)[:, :n_taps]
    with np.errstate(all="ignore"):
        return np.all(np.abs(t) <= F(bound), axis=(1, 2))  # (false for NaN; false for inf, the bound being finite)


def gradient(sigma7, h):
    """sigma7 [n][7] (the taps' sigmas in tap order) -> records [n][4] = (g_x, g_y, g_z, sigma at the centre)"""
    s = f32(sigma7).reshape(-1, N_TAPS)
    w = inv2h(h)
    out = np.empty((len(s), 4), np.float32)
    with np.errstate(all="ignore"):
        for k in range(3):
            d = (s[:, 1 + 2 * k] - s[:, 2 + 2 * k]).astype(np.float32)
            out[:, k] = (d * w).astype(np.float32)
    out[:, 3] = s[:, 0]
    return out


def hit_position(o, d, t, dt, frac):
    """[n][4] = (x, y, z, tq): tq = t - frac * dt, x_k = o_k + tq * d_k"""
    o, d = f32(o).reshape(-1, 3), f32(d).reshape(-1, 3)
    t, dt = f32(t).reshape(-1), f32(dt).reshape(-1)
    with np.errstate(all="ignore"):
        back = (F(frac) * dt).astype(np.float32)
        tq = (t - back).astype(np.float32)
        step = (tq[:, None] * d).astype(np.float32)
        x = (o + step).astype(np.float32)
    return np.concatenate([x, tq[:, None]], axis=1).astype(np.float32)


def is_hit(records, rays_per_view, opacity):
    """[px] bool for one view's records [px][4]: pixel p is a hit if p < rays_per_view and ws1 >= opacity (fp32 compare)"""
    rec = f32(records).reshape(-1, 4)
    return (np.arange(len(rec)) < rays_per_view) & (rec[:, 3] >= F(opacity))


def facing_shares(records, dirs):
    """(share with |g| > 0, share whose surface faces the ray) of gradient records [n][4] at points reached along dirs [n][3].
    The normal is n = -g / |g| (towards falling density); it faces the ray when it points back along it: dot(n, -d) > 0, that is
    dot(g, d) > 0 -- the density rises along the ray where it enters a surface."""
    g = f32(records).reshape(-1, 4)[:, :3].astype(np.float64)
    d = f32(dirs).reshape(-1, 3).astype(np.float64)
    if len(g) == 0:
        return 0.0, 0.0
    return float(np.mean(np.sum(g * g, axis=1) > 0)), float(np.mean(np.sum(g * d, axis=1) > 0))


def blob_model(log2_hashmap_size=12, H=32, radius=0.6, peak=7.0):
    """A model whose DENSITY has a shape: the synthetic models' tables are noise (their scene lives in the occupancy grid alone), so
    the gradient of their sigma says nothing about a surface.  Here every table entry is zero except level 0 (dense: 16^3 entries,
    the vertices of the outermost layer wrap onto each other and carry zeros), whose two features carry the trilinear field s(v) = max(0, radius - |world(v)|) along one fixed direction of
    feature space.  With ReLU layers and the positive density row of synthetic.mlp_weights, log sigma = K s for a K > 0: a ball
    whose density falls off radially; the occupancy grid is all ones.  `peak` is log sigma at the centre.
    Returns (desc, keep, cfg) like models.build_model."""
    import models
    import nerfhip as nh
    import oracle_py as op
    desc0, keep0, cfg = models.build_model(log2_hashmap_size=log2_hashmap_size, H=H)
    params = np.array(keep0[0], np.float32).copy()
    grid = np.ones_like(np.array(keep0[1], np.float32))  # every cell occupied: the rays see the ball, not the Lego-like shape
    lt = nh.level_table(desc0)
    Fdim = int(desc0.n_features_per_level)
    n_grid = int(lt.offset[desc0.n_levels]) * Fdim
    base = len(params) - n_grid
    res = int(lt.resolution[0])
    assert res ** 3 == int(lt.offset[1]) - int(lt.offset[0]), "level 0 must be dense"
    orc = op.Oracle(desc0)
    v = np.arange(res + 1)
    world = ((v - 0.5) / np.float64(lt.scale[0]) - 0.5) * 2.0 * float(desc0.bound)
    params[base:] = 0.0
    field = {}
    for x in v:
        for y in v:
            for z in v:
                s = max(0.0, radius - float(np.sqrt(world[x] ** 2 + world[y] ** 2 + world[z] ** 2)))
                i = int(lt.offset[0]) + orc.grid_index(0, int(x), int(y), int(z))
                assert field.get(i, s) == s, "wrapped vertices must agree"
                field[i] = s
    idx = np.fromiter(field.keys(), np.int64)
    val = np.fromiter(field.values(), np.float64)
    # K from the network itself: log sigma at the centre with unit amplitude, then the amplitude that gives `peak` there
    def log_sigma_centre(amp):
        p = params.copy()
        p[base + Fdim * idx] = (amp * val).astype(np.float32)
        p[base + Fdim * idx + 1] = (amp * val).astype(np.float32)
        d, k = nh.desc_from_config(cfg, p, grid)
        s, _ = op.Oracle(d).network(np.zeros((1, 3), np.float32), np.float32([[0, 0, 1]]))
        return float(np.log(s[0])), p, d, k
    l1 = log_sigma_centre(1.0)[0]
    assert l1 > 0
    _, p, desc, keep = log_sigma_centre(peak / l1)
    return desc, keep, cfg
