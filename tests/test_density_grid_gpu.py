"""nrf_generate_density_grid on the GPU, every cell held to nrf_network's bits.

The generator launches density_positions_kernel, the stage's network_kernel and density_update_kernel per cascade, takes the mean on
the host and rebuilds every march table.  Positions and updates are single fp32 roundings and the network call is nrf_network's own
launcher, so the generated grid must equal `update(nrf_network's sigma at positions(...))` of tests/density_grid_replay.py in every
bit and the mean must equal `mean(...)` (tests/test_density_grid_cpu.py holds that replay to the oracle and the positions to the
march's own cell lookup).  Every replay call to nrf_network stays within one trip of its kernel (65 536 points), so a mistake in the
generator's own second trips -- the H = 96 leg: 884 736 cells, two ragged trips of the generator's two kernels, four of the network
-- cannot be shared by the reference.  Models: the 2^12 table, loaded WITHOUT a grid; rows: density_grid_replay.ROWS.
Every test here needs the GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import density_grid_replay as dr
import grid_plan_rows as R
import models
import nerfhip as nh
import synthetic as syn
from test_density_grid_cpu import INFINITE_FACTOR, infinite_model

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
STAGE = {"hot": 0, "generic": 1, "wide": 2}  # DevModel::stage (csrc/nrf_launch.h NET_HOT / NET_GENERIC / NET_WIDE)
ROW_STAGE = {**{r: "hot" for r in (*dr.HOT_ROWS, *dr.TRIPS_ROW)}, "wide-h32": "wide", "wide-h30": "wide", "sine-h32": "generic",
             "sine-h30": "generic", "f4-h32": "generic"}
W, H_PX = 64, 48
CAM, POSE = syn.default_camera(W, H_PX), syn.orbit_pose(40, 25)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _word(x):
    """the bits of a number as fp32"""
    return int(np.array([x], F).view(np.uint32)[0])


def _upload(a):
    t = torch.from_numpy(np.ascontiguousarray(a, F)).cuda()
    torch.cuda.synchronize()
    return t


@functools.lru_cache(maxsize=None)
def _model(row):
    """(descriptor without a grid, its keepalive, config, the descriptor with the synthetic grid, its keepalive), built once"""
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, **dr.ROWS[row])
    d0, k0 = nh.desc_from_config(cfg, keep[0])
    assert d0.n_density_grid == 0 and not d0.density_grid
    return d0, k0, cfg, desc, keep


def _with_grid(cfg, params, grid, mean):
    """the same parameters with `grid` and `mean` as the snapshot's"""
    cfg2 = dict(cfg)
    cfg2["snapshot"] = dict(cfg["snapshot"], mean_density=float(mean))
    return nh.desc_from_config(cfg2, params, grid)


def _network_sigma(ctx, xyz):
    """nrf_network's sigma at xyz with the generator's direction, in calls of at most one trip of network_kernel"""
    out = np.empty(len(xyz), F)
    for a in range(0, len(xyz), dr.CHUNK):
        x = xyz[a:a + dr.CHUNK]
        tx, td = _upload(x), _upload(dr.directions(len(x)))
        s, rgb = torch.full((len(x),), 7.0, device="cuda"), torch.empty((len(x), 3), device="cuda")
        torch.cuda.synchronize()
        ctx.network(tx.data_ptr(), td.data_ptr(), len(x), s.data_ptr(), rgb.data_ptr())
        out[a:a + len(x)] = s.cpu().numpy()
    return out


def _sigmas_of(ctx, desc):
    H, bound, cascade = int(desc.density_grid_size), float(desc.bound), int(desc.cascade)
    sig = np.concatenate([_network_sigma(ctx, dr.positions(H, bound, c)) for c in range(cascade)])
    sig.setflags(write=False)
    return sig


@functools.lru_cache(maxsize=None)
def _sigmas(row):
    """The replayed sigmas of a row, all cascades, computed once on a context of their own and shared (read-only)"""
    d0 = _model(row)[0]
    ctx = nh.NerfHip(0)
    try:
        ctx.load_model(d0)
        assert R.readout(ctx)[0]["stage"] == STAGE[ROW_STAGE[row]], row
        return _sigmas_of(ctx, d0)
    finally:
        ctx.close()


def _want(row, n_iterations=16, decay=0.95):
    grid = dr.update(_sigmas(row), n_iterations, decay)
    return grid, dr.mean(grid)


def _same_grid(got, want, H, what):
    gb, wb = _bits(got), _bits(want)
    assert gb.shape == wb.shape, what
    bad = np.flatnonzero(gb != wb)
    if bad.size:
        i = int(bad[0])
        c, r = divmod(i, H ** 3)
        pytest.fail(f"{what}: {bad.size} of {gb.size} cells differ; the first: cascade {c}, cell {r} = ({r // (H * H)}, {r // H % H}, {r % H}), "
                    f"generated {int(gb[i]):#010x}, replayed {int(wb[i]):#010x}")


def _same_mean(got, want, what):
    assert _word(got) == _word(want), f"{what}: mean generated {_word(got):#010x}, replayed {_word(want):#010x}"


def _generated(row, n_iterations=16, decay=0.95):
    """A fresh context with the row's model after nrf_generate_density_grid: (ctx, grid, mean); the caller closes ctx"""
    d0 = _model(row)[0]
    ctx = nh.NerfHip(0)
    ctx.load_model(d0)
    mean = ctx.generate_density_grid(n_iterations, decay)
    grid, mean2 = ctx.read_density_grid(int(d0.cascade) * int(d0.density_grid_size) ** 3)
    assert _word(mean) == _word(mean2)
    return ctx, grid, mean


def _frame(ctx, cam=CAM, pose=POSE):
    ctx.set_options(nh.default_options())
    ctx.set_resolution(W, H_PX)
    ctx.render(cam, pose)
    return ctx.read_f32()


def _same_readout(a, b, what):
    fa, ba, ta = R.readout(a)
    fb, bb, tb = R.readout(b)
    assert fa == fb, what
    assert np.array_equal(_bits(ba), _bits(bb)), what
    for x, y in zip(ta, tb):
        assert x.size == y.size and np.array_equal(x.view(np.uint32), y.view(np.uint32)), what


def _occupancy_words(grid, mean):
    """build_march_tables' bitfield: bit i = grid[i] > min(0.01, mean), plus the padding word"""
    with np.errstate(invalid="ignore"):
        bits = grid > np.fmin(F(0.01), F(mean))
    words = np.zeros((bits.size + 31) // 32 + 1, np.uint32)
    packed = np.packbits(bits, bitorder="little")
    words.view(np.uint8)[:packed.size] = packed
    return words


# ---------------------------------------------------------------- a. values
@pytest.mark.parametrize("row", [*dr.HOT_ROWS, *dr.OTHER_ROWS])
def test_generated_grid_is_the_replay_of_nrf_network(row):
    d0 = _model(row)[0]
    Hg = int(d0.density_grid_size)
    want, wmean = _want(row)
    ctx, grid, mean = _generated(row)
    try:
        _same_grid(grid, want, Hg, row)
        _same_mean(mean, wmean, row)
        assert np.isfinite(grid).all() and len(np.unique(grid)) > 100 and grid.min() < 0.01 < grid.max(), row  # a grid worth comparing
        occ = R.readout(ctx)[2][0]
        assert np.array_equal(occ, _occupancy_words(grid, mean)), row
    finally:
        ctx.close()


# ---------------------------------------------------------------- b. second trips
def test_second_trips_of_the_generators_kernels():
    row = "h96"
    d0 = _model(row)[0]
    Hg = int(d0.density_grid_size)
    assert Hg ** 3 > 524288  # the launch cap of density_positions_kernel and density_update_kernel: 2048 blocks of 256 threads
    assert Hg ** 3 > 3 * 262144 and Hg ** 3 % 262144 != 0 and Hg ** 3 % 524288 != 0  # four trips of the network, every last one ragged
    want, wmean = _want(row)
    ctx, grid, mean = _generated(row)
    try:
        _same_grid(grid, want, Hg, row)
        _same_mean(mean, wmean, row)
        assert len(np.unique(grid[524288:])) > 100  # the second trip holds a grid worth comparing, too
    finally:
        ctx.close()


# ---------------------------------------------------------------- c. arguments
@pytest.mark.parametrize("n_iterations,decay", [(1, 0.95), (16, 1.0), (3, 0.5)])
def test_other_arguments_go_against_the_replay(n_iterations, decay):
    want, wmean = _want(dr.BASE, n_iterations, decay)
    ctx, grid, mean = _generated(dr.BASE, n_iterations, decay)
    try:
        _same_grid(grid, want, 32, (n_iterations, decay))
        _same_mean(mean, wmean, (n_iterations, decay))
        assert not np.array_equal(_bits(grid), _bits(_want(dr.BASE)[0]))  # the arguments moved the grid
    finally:
        ctx.close()


def test_refused_arguments_leave_grid_and_mean_untouched():
    ctx, grid, mean = _generated(dr.BASE)
    assert F(1.0000001) > F(1.0)  # (above 1 in fp32, too)
    try:
        for n_iterations, decay in ((0, 0.95), (16, 0.0), (16, 1.0000001), (16, float("nan")), (-1, 0.95), (16, -0.5)):
            with pytest.raises(nh.NerfHipError) as e:
                ctx.generate_density_grid(n_iterations, decay)
            assert e.value.code == nh.NRF_E_INVALID, (n_iterations, decay)
            g2, m2 = ctx.read_density_grid(grid.size)
            assert np.array_equal(_bits(g2), _bits(grid)) and _word(m2) == _word(mean), (n_iterations, decay)
        occ = R.readout(ctx)[2][0]
        assert np.array_equal(occ, _occupancy_words(grid, mean))
    finally:
        ctx.close()


def test_a_context_without_a_model_is_refused():
    ctx = nh.NerfHip(0)
    try:
        with pytest.raises(nh.NerfHipError) as e:
            ctx.generate_density_grid(16, 0.95)
        assert e.value.code == nh.NRF_E_STATE
    finally:
        ctx.close()


# ---------------------------------------------------------------- d. consumers
@pytest.mark.parametrize("row", [dr.BASE, "h30-b4-c3", "wide-h30", "sine-h32"])
def test_consumers_of_a_generated_grid(row):
    d0, k0, cfg, desc, keep = _model(row)
    ctx, grid, mean = _generated(row)
    twin = nh.NerfHip(0)
    try:
        d2, k2 = _with_grid(cfg, keep[0], grid, mean)
        twin.load_model(d2)
        _same_readout(ctx, twin, row)
        got, want = _frame(ctx), _frame(twin)
        assert ctx.stats().n_samples > 0 and twin.stats().n_samples > 0, row
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1])), row
        assert got[0][..., 3].max() > 0.5, row  # the object is in view
        # generating twice gives the same bits
        m2 = ctx.generate_density_grid(16, 0.95)
        g2, _ = ctx.read_density_grid(grid.size)
        assert np.array_equal(_bits(g2), _bits(grid)) and _word(m2) == _word(mean), row
        _same_readout(ctx, twin, row)
        # a model that has a grid, loaded afterwards, keeps its own
        ctx.load_model(desc)
        g3, m3 = ctx.read_density_grid(grid.size)
        assert np.array_equal(_bits(g3), _bits(keep[1])) and _word(m3) == _word(desc.mean_density), row
        assert np.array_equal(R.readout(ctx)[2][0], _occupancy_words(keep[1], desc.mean_density)), row
    finally:
        twin.close()
        ctx.close()


# ---------------------------------------------------------------- e. groups
def test_every_group_member_generates_the_single_contexts_grid():
    d0 = _model(dr.BASE)[0]
    ctx, grid, mean = _generated(dr.BASE)
    g = nh.NerfGroup([0, 0])
    try:
        g.load_model(d0)
        gmean = g.generate_density_grid(16, 0.95)
        assert _word(gmean) == _word(mean)
        assert g.lib.nrf_group_size(g.h) == 2
        for i in range(2):
            member = C.c_void_p(g.lib.nrf_group_member(g.h, i))
            got, m = np.empty(grid.size, F), C.c_float()
            nh._check(g.lib.nrf_read_density_grid(member, got.ctypes.data, got.size, C.byref(m)))
            _same_grid(got, grid, 32, f"member {i}")
            _same_mean(m.value, mean, f"member {i}")
        poses = [POSE, syn.orbit_pose(200, 10)]
        g.set_options(nh.default_options())
        g.set_resolution(W, H_PX)
        g.render_views(np.stack([CAM, CAM]), np.stack(poses))
        for v, pose in enumerate(poses):
            want = _frame(ctx, CAM, pose)
            got = g.read_view_f32(v)
            assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1])), v
            assert want[0][..., 3].max() > 0.5
    finally:
        g.close()
        ctx.close()


# ---------------------------------------------------------------- f. infinite sigmas
def test_infinite_sigmas_give_infinite_cells_and_an_infinite_mean():
    """A density row scaled until exp(g0) overflows in most cells (the factor: tests/test_density_grid_cpu.py): the cell is +inf
    (0.001691 * inf, kept by every comparison of the update), the mean of max(g, 0) is +inf as include/nerfhip.h defines it, the
    occupancy threshold min(0.01, mean) is 0.01, and the frame stays finite: the march reads occupancy bits only."""
    d0, k0 = infinite_model(INFINITE_FACTOR)
    cfg = _model(dr.BASE)[2]
    ctx, twin = nh.NerfHip(0), nh.NerfHip(0)
    try:
        ctx.load_model(d0)
        want = dr.update(_sigmas_of(ctx, d0), 16, 0.95)
        share = float(np.isinf(want).mean())
        assert 0.01 <= share <= 0.99, share  # the condition of this leg: cells of both kinds
        assert not np.isnan(want).any()
        mean = ctx.generate_density_grid(16, 0.95)
        grid, mean2 = ctx.read_density_grid(32 ** 3)
        _same_grid(grid, want, 32, "infinite sigmas")
        assert mean == np.inf and mean2 == np.inf and dr.mean(want) == np.inf
        # occupancy: cell > min(0.01, mean), in the device's table and in the plan of this grid
        got, box, tables = R.readout(ctx)
        assert np.array_equal(tables[0], _occupancy_words(grid, mean))
        assert (grid[np.isinf(grid)] > 0).all()
        d2, k2 = _with_grid(cfg, k0[0], grid, mean)
        plan, pbox, ptables = R.plan(d2, grid, mean, R.ALL)
        assert np.array_equal(_bits(box), _bits(pbox))
        for t, p in zip(tables, ptables):
            assert t.size == p.size and np.array_equal(t.view(np.uint32), p.view(np.uint32))
        rgba, depth = _frame(ctx)
        assert np.isfinite(rgba).all() and np.isfinite(depth).all()
        assert rgba[..., 3].min() >= 0.0 and rgba[..., 3].max() <= 1.0 and rgba[..., 3].max() > 0.5
        twin.load_model(d2)
        _same_readout(ctx, twin, "infinite sigmas")
        trgba, tdepth = _frame(twin)
        assert np.array_equal(_bits(rgba), _bits(trgba)) and np.array_equal(_bits(depth), _bits(tdepth))
    finally:
        twin.close()
        ctx.close()
