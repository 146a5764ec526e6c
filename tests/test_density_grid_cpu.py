"""tests/density_grid_replay.py, the numpy restatement of nrf_generate_density_grid, without a GPU: held to the oracle's
nrfo_density_grid bit for bit (the restatement tests/test_generic_gpu.py already trusts), its positions held to the march's own cell
lookup (the generator evaluates the centre of the cell the march will read), and dg_update at its edges.  Here, too, the factor of
the infinite-sigma model of tests/test_density_grid_gpu.py is chosen."""
import ctypes as C

import numpy as np
import pytest

import density_grid_replay as dr
import models
import nerfhip as nh
import oracle_py as op

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _replayed(o, H, bound, cascade, n_iterations, decay):
    cells = []
    for c in range(cascade):
        xyz = dr.positions(H, bound, c)
        sigma, _ = o.network(xyz, dr.directions(len(xyz)))
        cells.append(dr.update(sigma, n_iterations, decay))
    grid = np.concatenate(cells)
    return grid, dr.mean(grid)


@pytest.mark.parametrize("kw", [dict(), dict(bound=1.5, cascade=2), dict(bound=0.5)], ids=["base", "b1.5-c2", "b0.5"])
@pytest.mark.parametrize("args", [(16, 0.95), (3, 0.5)])
def test_replay_is_the_oracles_density_grid(kw, args):
    H = 16
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, H=H, **kw)
    d0, k0 = nh.desc_from_config(cfg, keep[0])  # no grid
    o = op.Oracle(d0)
    want, wmean = o.density_grid(int(desc.cascade) * H ** 3, *args)
    got, mean = _replayed(o, H, float(desc.bound), int(desc.cascade), *args)
    assert np.array_equal(_bits(got), _bits(want))
    assert _bits(mean) == _bits(F(wmean))
    assert len(np.unique(got)) > 100 and want.min() < 0.01 < want.max()  # a grid on both sides of the occupancy threshold


@pytest.mark.parametrize("row", list(dr.ROWS))
def test_positions_are_the_centres_of_the_cells_the_march_reads(row):
    """march_cell(positions(...)) of cell i is i, in every cascade, and the promoted product lies half a cell past the cell's
    lower face: an order or axis mistake shared by kernel and oracle cannot pass this"""
    H, bound, cascade = dr.geometry(dr.ROWS[row])
    for c in range(cascade):
        cell, frac = dr.march_cell(dr.positions(H, bound, c), H, dr.cascade_bound(bound, c))
        assert np.array_equal(cell, np.arange(H ** 3)), (row, c)
        assert frac.min() >= 0.49 and frac.max() <= 0.51, (row, c, frac.min(), frac.max())
    # cell order: x slowest, z fastest; the positions grow with the index on every axis and are symmetric about 0
    p = dr.positions(H, bound, 0).reshape(H, H, H, 3)
    assert np.all(np.diff(p[:, 0, 0, 0]) > 0) and np.all(np.diff(p[0, :, 0, 1]) > 0) and np.all(np.diff(p[0, 0, :, 2]) > 0)
    assert np.all(p[:, 0, 0, 1] == p[0, 0, 0, 1]) and np.all(p[0, 0, :, 0] == p[0, 0, 0, 0])
    assert np.abs(p).max() < dr.cascade_bound(bound, 0)


def test_the_march_lookup_tells_a_swapped_axis():
    """(the anchor has teeth: positions with x and z exchanged do not land in their own cells)"""
    H = 8
    xyz = dr.positions(H, 1.0, 0)
    cell, _ = dr.march_cell(xyz[:, ::-1], H, 1.0)
    assert (cell != np.arange(H ** 3)).mean() > 0.8


def _update_scalar(sigma, n_iterations, decay):
    """density_update_kernel, literally, on numpy fp32 scalars"""
    with np.errstate(all="ignore"):
        tmp = F(F(0.001691) * F(sigma))
        g = F(1.0) / F(64)
        for _ in range(n_iterations):
            if g >= 0:
                gd = F(g * F(decay))
                g = gd if gd > tmp else tmp
    return F(g)


def _floor(n_iterations, decay):
    g = F(1.0) / F(64)
    for _ in range(n_iterations):
        g = F(g * F(decay))
    return g


@pytest.mark.parametrize("n_iterations,decay", [(16, 0.95), (1, 0.95), (16, 1.0), (3, 0.5), (1, 1.0)])
def test_update_edges(n_iterations, decay):
    floor = _floor(n_iterations, decay)
    assert floor == F(1 / 64) if decay == 1.0 else floor < F(1 / 64)
    at = floor / dr.SCALE  # sigma whose scaled value is about the floor
    sigma = np.array([0.0, -3.0, at * F(0.5), np.nextafter(at, F(0)), at, np.nextafter(at, F(np.inf)), at * F(1.5),
                      F(1 / 64) / dr.SCALE, F(1 / 64) / dr.SCALE * F(2), 1e4, 3e38, np.inf, -np.inf, np.nan], F)
    got = dr.update(sigma, n_iterations, decay)
    want = np.array([_update_scalar(s, n_iterations, decay) for s in sigma], F)
    assert np.array_equal(_bits(got), _bits(want))
    with np.errstate(all="ignore"):
        tmp = (dr.SCALE * sigma).astype(F)
    # closed forms: below the floor the decayed start value survives, above it the scaled sigma does
    below, above = tmp < floor, tmp > floor
    assert np.array_equal(_bits(got[below]), _bits(np.full(below.sum(), floor, F)))
    assert np.array_equal(_bits(got[above]), _bits(tmp[above]))
    assert below.sum() >= 4 and above.sum() >= 5
    assert got[11] == np.inf and np.isnan(got[13]) and got[12] == floor
    assert dr.mean(got) == np.inf
    finite = np.where(np.isfinite(got), got, F(0))
    assert _bits(dr.mean(np.where(np.isinf(got), F(0), got))) == _bits(dr.mean(finite))  # the NaN cell counts as 0


def test_mean_is_the_sequential_float64_sum():
    rng = np.random.default_rng(2)
    g = (rng.random(100003) * 10.0 ** rng.integers(-6, 3, 100003)).astype(F)
    g[::7] = -g[::7]
    total = 0.0
    for v in g.tolist():
        total += v if v > 0 else 0.0
    assert _bits(dr.mean(g)) == _bits(F(total / g.size))
    assert dr.mean(np.array([np.nan, 1.0, -2.0, 3.0], F)) == F(1.0)


# ---------------------------------------------------------------- the infinite-sigma model
def infinite_model(factor, H=32):
    """The base shape loaded without a grid, the density output layer's row for g0 (params[64 * 32 : 64 * 32 + 64], synthetic.py)
    scaled by `factor`, a power of two: sigma = exp(g0) overflows to +inf where g0 grew past 88.7.  (desc, keepalive)"""
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, H=H)
    params = np.array(keep[0], F)
    params[64 * 32:64 * 32 + 64] *= F(factor)
    return nh.desc_from_config(cfg, params)


INFINITE_FACTOR = 4.0  # (the oracle at H = 16: 2 gives 2.9 % of +inf cells, 4 gives 78.6 %, 8 gives 99.8 %)


def test_the_infinite_sigma_factor_gives_a_mixed_grid():
    """chosen here, on the CPU: the oracle's grid at H = 16 holds +inf in between 5 % and 95 % of its cells, the rest finite"""
    d0, k0 = infinite_model(INFINITE_FACTOR, H=16)
    grid, mean = op.Oracle(d0).density_grid(16 ** 3)
    share = float(np.isinf(grid).mean())
    print(f"share of +inf cells at factor {INFINITE_FACTOR}: {share:.3f}")
    assert 0.05 <= share <= 0.95
    assert not np.isnan(grid).any() and grid[np.isinf(grid)].min() > 0 and mean == np.inf
