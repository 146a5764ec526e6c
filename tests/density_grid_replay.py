"""nrf_generate_density_grid restated in numpy -- TEST INFRASTRUCTURE ONLY.

The generator (csrc/nrf_api.hip) evaluates, per cascade, the density network at one position per cell (density_positions_kernel),
folds 0.001691 * sigma into a grid that starts at 1/64 (density_update_kernel) and takes the mean of max(g, 0) on the host.  Every
step is a chain of single fp32 roundings (the build uses -ffp-contract=off), restated here operation by operation, so a test can
hold the generated grid to `update(sigma of nrf_network at positions(...))` bit for bit: tests/test_density_grid_gpu.py does that,
tests/test_density_grid_cpu.py holds this file to the oracle's nrfo_density_grid and -- `march_cell`, the march's own cell lookup
(render_utils.h:609-614 as the oracle states it) -- the positions to what they are for: the centre of cell i of cascade c is looked
up by the march as cell i of cascade c.  That last check is the one a cell order or axis mistake shared by kernel and oracle
cannot pass.

ROWS: the models the GPU tests generate a grid for (the geometries of tests/rays_forms.py plus the power-of-two ones of side 32)."""
from __future__ import annotations

import numpy as np

import rays_forms as rf

F = np.float32
SCALE = F(0.001691)      # dd_scale's constant (nerf_render.cu:417)
START = F(1.0) / F(64)   # the grid's initial value (nerf_render.cu:393)
CHUNK = 65536            # points per replay call to nrf_network: one trip of network_kernel (262 144 points)

# name: model kwargs of models.build_model(log2_hashmap_size=12, **kw)
HOT_ROWS = {
    "h32": dict(H=32),
    "h32-b4-c3": dict(H=32, bound=4.0, cascade=3),
    "h32-b2-c2": dict(H=32, bound=2.0, cascade=2),
    "h30": rf.kwargs("h30"),
    "h30-b4-c3": rf.kwargs("h30-b4-c3"),
    "h64-b1.5-c2": rf.kwargs("h64-b1.5-c2"),
    "h48-b3-c3": rf.kwargs("h48-b3-c3"),
    "h32-b0.5": dict(H=32, bound=0.5),
}
OTHER_ROWS = {
    "wide-h32": dict(H=32, **rf.FREQ12), "wide-h30": rf.kwargs("wide-h30"),
    "sine-h32": dict(H=32, **rf.SINE), "sine-h30": rf.kwargs("sine-h30"),
    "f4-h32": dict(H=32, n_neurons=32, n_features_per_level=4, n_levels=8),
}
TRIPS_ROW = {"h96": rf.kwargs("h96")}  # 884 736 cells: two ragged trips of the generator's two kernels, four of the network
ROWS = {**HOT_ROWS, **OTHER_ROWS, **TRIPS_ROW}
BASE = "h32"


def geometry(kw):
    """(H, bound, cascade) of a row's kwargs"""
    return int(kw.get("H", 128)), float(kw.get("bound", 1.0)), int(kw.get("cascade", 1))


def cascade_bound(bound, cascade_index):
    """min(2^c, bound) as nrf_generate_density_grid takes it (nerf_render.cu:409), fp32"""
    p = F(1 << cascade_index)
    return p if p < F(bound) else F(bound)


def positions(H, bound, cascade_index):
    """fp32 [H^3][3]: the position the generator evaluates for every cell of one cascade, x slowest, z fastest (init_xyzs,
    render_utils.h:91-108, scaled by bound_c - bound_c / H); every operation rounded on its own"""
    step = F(2) / F(H - 1)
    v = (step * np.arange(H, dtype=np.uint32).astype(F)).astype(F)
    v = (F(-1) + v).astype(F)
    b = cascade_bound(bound, cascade_index)
    k = F(b - F(b / F(H)))
    c = (k * v).astype(F)
    xyz = np.empty((H, H, H, 3), F)
    xyz[..., 0] = c[:, None, None]
    xyz[..., 1] = c[None, :, None]
    xyz[..., 2] = c[None, None, :]
    return xyz.reshape(-1, 3)


def directions(n):
    """the constant direction (0, 0, 1) of the generator's network call"""
    d = np.zeros((n, 3), F)
    d[:, 2] = 1
    return d


def update(sigma, n_iterations, decay):
    """dd_scale + dg_update (render_utils.h:120-128): g = max(g * decay, 0.001691 * sigma) while g >= 0, n_iterations times from
    1/64; Inf and NaN follow the comparisons literally"""
    sigma = np.ascontiguousarray(sigma, F)
    decay = F(decay)
    with np.errstate(all="ignore"):
        tmp = (SCALE * sigma).astype(F)
        g = np.full(sigma.shape, START, F)
        for _ in range(int(n_iterations)):
            gd = (g * decay).astype(F)
            g = np.where(g >= 0, np.where(gd > tmp, gd, tmp), g).astype(F)
    return g


def mean(grid):
    """mean of max(g, 0): the float64 sum taken sequentially in cell order, divided by the cell count, rounded to fp32"""
    g = np.ascontiguousarray(grid, F).reshape(-1)
    with np.errstate(all="ignore"):
        terms = np.where(g > 0, g.astype(np.float64), 0.0)
        total = np.add.accumulate(terms)[-1]  # (np.sum adds pairwise)
        return F(total / np.float64(g.size))


def march_cell(xyz, H, mip_bound):
    """The march's lookup of a position (the oracle's march, oracle/nerf_oracle.cpp: `0.5 * (x * mip_rbound + 1) * H` is double
    arithmetic on a float operand, narrowed to float, clamped to [0, H-1], truncated): (cell index nx H^2 + ny H + nz,
    fractional parts [n][3] of the promoted products)"""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    r = F(1) / F(mip_bound)
    t = ((xyz * r).astype(F) + F(1)).astype(F)
    p = 0.5 * t.astype(np.float64) * np.float64(H)
    n3 = np.clip(p.astype(F), F(0), F(H - 1)).astype(np.int64)
    return (n3[:, 0] * H + n3[:, 1]) * H + n3[:, 2], p - np.floor(p)
