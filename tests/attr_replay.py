"""The arithmetic of nrf_point_attributes / nrf_mesh_attributes replayed in numpy fp32 -- TEST INFRASTRUCTURE ONLY.

From a gradient record (g_x, g_y, g_z) of nrf_density_gradient to the unit direction d = g / |g|, the outward normal n = -d and the
length, and the library's 8-bit rule of an exported colour (include/nerfhip.h).  Every numpy operation on float32 arrays is one fp32
rounding and numpy's float32 sqrt and division are the correctly rounded IEEE ones, which is what the library's build
(-ffp-contract=off -fno-fast-math) makes of csrc/nrf_attr_plan.h; tests/test_point_attributes_cpu.py holds this module to that header
bit for bit through host/attr_plan_check.cpp, and the GPU tests hold the kernels to this module.  It shares no code with the header."""
from __future__ import annotations

import numpy as np

F = np.float32
L2_FLOOR = F(2.0 ** -60)
NORM_BOUND = 8.0 * 2.0 ** -24  # | |n|^2 - 1 | of a non-degenerate normal, evaluated in float64 (derived in test_point_attributes_cpu.py)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def bits(a):
    return f32(a).view(np.uint32)


def direction(g):
    """g [n][3] -> (normal [n][3], length [n], d [n][3], ok [n]): l2 = (gx gx + gy gy) + gz gz; ok = l2 finite and >= 2^-60;
    len = sqrt(l2); d = g / len; n = -d; a degenerate row is all positive zeros"""
    g = f32(g).reshape(-1, 3)
    with np.errstate(all="ignore"):
        xx = (g[:, 0] * g[:, 0]).astype(np.float32)
        yy = (g[:, 1] * g[:, 1]).astype(np.float32)
        zz = (g[:, 2] * g[:, 2]).astype(np.float32)
        xy = (xx + yy).astype(np.float32)
        l2 = (xy + zz).astype(np.float32)
        ok = np.isfinite(l2) & (l2 >= L2_FLOOR)
        length = np.where(ok, np.sqrt(np.where(ok, l2, F(1))).astype(np.float32), F(0)).astype(np.float32)
        safe = np.where(ok, length, F(1)).astype(np.float32)
        d = np.where(ok[:, None], (g / safe[:, None]).astype(np.float32), F(0)).astype(np.float32)
        n = np.where(ok[:, None], -d, F(0)).astype(np.float32)
    return n, length, d, ok


def dir01(d):
    """what the network is given for a direction: 0.5 d (rounded), then + 0.5 (rounded)"""
    d = f32(d)
    with np.errstate(all="ignore"):
        u = (F(0.5) * d).astype(np.float32)
        return (u + F(0.5)).astype(np.float32)


def color_u8(x):
    """the library's 8-bit rule: (unsigned char)(255.0 * x) with the product in double, saturating, NaN -> 0"""
    with np.errstate(all="ignore"):
        s = 255.0 * f32(x).astype(np.float64)
        pos = s > 0.0  # (false for NaN)
        return np.where(pos, np.floor(np.minimum(np.where(pos, s, 0.0), 255.0)), 0.0).astype(np.uint8)


def records(gradient_records):
    """gradient records [n][4] = (g_x, g_y, g_z, sigma) -> (normal records [n][4] = (n, sigma), length [n], d [n][3], ok [n])"""
    rec = f32(gradient_records).reshape(-1, 4)
    n, length, d, ok = direction(rec[:, :3])
    return np.concatenate([n, rec[:, 3:4]], axis=1).astype(np.float32), length, d, ok


def norm_error(normals):
    """| |n|^2 - 1 | in float64"""
    n = f32(normals).reshape(-1, 3).astype(np.float64)
    return np.abs(np.sum(n * n, axis=1) - 1.0)
