"""The step plan of the barrier fast-forward (csrc/nrf_step_plan.h) without a GPU, through nrf_debug_step_table.

  * step_table is the march's recurrence t_{k+1} = t_k + clamp(t_k * dt_gamma, dt_min, dt_max), every operation rounded to fp32 on
    its own: every entry equals the numpy float32 recurrence as bits, the members strictly increase, and the table ends where the
    header says (the first member beyond min_near + 2 sqrt(3) bound plus one step, or 1024 entries);
  * step_land returns the bits of `while (t < tb) t += dt(t)`: 10^5 seeded targets per row against the recurrence continued in numpy
    -- every member and its two fp32 neighbours, targets at or below the start, targets beyond the last member, NaN, -inf and the
    NONE value; +inf under the clamp to a finite far the fast-forward functions apply (the loop itself never returns from +inf);
  * a table truncated to 8 entries gives the same bits as the full one;
  * a start one ulp off table[0] takes the loop and equals it.

The rows are every combination the kernels' options meet: min_near {0.05, 0.2, 0.5} x dt_gamma {0, 1/256, 1/128, 1/64, 0.01} x
bound {0.5, 1, 2, 16} x H {64, 96, 128}.  (0.01 is the one dt_gamma that is no power of two: with the others the product t * dt_gamma
is exact, and a product fused into the add would round the same.)

Sensitivity, checked by hand on scratch builds: with `m <= tb` for `m < tb` in step_land's lower bound
test_step_land_equals_the_loop fails (a target equal to a member lands one member late); with step_next computing
fmaf(t, dt_gamma, t) where the clamp does not bind, test_the_table_is_the_recurrence fails on the dt_gamma 0.01 rows."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import nerfhip as nh

F = np.float32
MIN_NEAR = [0.05, 0.2, 0.5]
DT_GAMMA = [0.0, 1.0 / 256, 1.0 / 128, 1.0 / 64, 0.01]
BOUND = [0.5, 1.0, 2.0, 16.0]
GRID = [64, 96, 128]
ROWS = list(itertools.product(MIN_NEAR, DT_GAMMA, BOUND, GRID))
CAPACITY = 1024
NONE = F(-3.402823466e+38)  # barrier_before's "no plane" (csrc/nrf_device.h)
N_TARGETS = 100_000
TAIL = 64  # members of the recurrence kept beyond the table: where targets beyond the last member land


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _consts(bound, H):
    dt_min = F(F(F(2) * F(1.7320508075688772)) / F(1024))
    dt_max = F(F(F(2) * F(bound)) / F(H))
    return dt_min, dt_max


def _recurrence(start, dt_gamma, bound, H, stop):
    """The members from `start` on, each operation a numpy float32 one; stop(members) -> True ends it"""
    dt_min, dt_max = _consts(bound, H)
    g = F(dt_gamma)
    out = [F(start)]
    while not stop(out):
        t = out[-1]
        p = F(t * g)
        dt = min(dt_max, max(dt_min, p))
        out.append(F(t + dt))
    return np.array(out, F)


@functools.lru_cache(maxsize=None)
def _expected(row, capacity=CAPACITY):
    """(the table the header must build for the row, the recurrence continued TAIL members beyond it)"""
    min_near, dt_gamma, bound, H = row
    reach = F(F(min_near) + F(F(F(2) * F(1.7320508075688772)) * F(bound)))

    def table_ends(m):
        return len(m) == capacity or (len(m) >= 2 and m[-2] > reach)

    table = _recurrence(min_near, dt_gamma, bound, H, table_ends)
    full = _recurrence(table[-1], dt_gamma, bound, H, lambda m: len(m) == TAIL + 1)
    full = np.concatenate([table, full[1:]])
    for a in (table, full):
        a.setflags(write=False)
    return table, full


def _call(row, starts, targets, capacity=CAPACITY, far=np.inf):
    """nrf_debug_step_table: (the table, step_land of every (start, target) on it)"""
    lib = nh.load_library()
    fn = lib.nrf_debug_step_table
    fp = C.POINTER(C.c_float)
    fn.restype = C.c_int
    fn.argtypes = [C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_int, fp, C.POINTER(C.c_int), C.c_int, fp, fp, C.c_float, fp,
                   C.POINTER(C.c_int32)]
    min_near, dt_gamma, bound, H = row
    starts = np.ascontiguousarray(np.broadcast_to(np.asarray(starts, F), np.shape(targets)), F)
    targets = np.ascontiguousarray(targets, F)
    table = np.full(max(capacity, 1), np.nan, F)
    landed = np.full(len(targets), np.nan, F)
    n = C.c_int(-1)
    rc = fn(min_near, dt_gamma, bound, H, capacity, table.ctypes.data_as(fp), C.byref(n), len(targets), starts.ctypes.data_as(fp),
            targets.ctypes.data_as(fp), far, landed.ctypes.data_as(fp), None)
    assert rc == nh.NRF_OK, row
    return table[:n.value], landed


def _loop(members, start, targets):
    """What `while (t < tb) t += dt(t)` returns from `start` = members[0]: the first member that is not below the target, the start
    itself where !(start < tb).  Every finite target must lie at or below members[-1]."""
    targets = np.asarray(targets, F)
    steps = np.less(F(start), targets)  # (False for NaN)
    assert np.all(targets[steps] <= members[-1])
    idx = np.searchsorted(members, np.where(steps, targets, F(start)), side="left")
    return np.where(steps, members[np.minimum(idx, len(members) - 1)], F(start)).astype(F)


def _targets(row, members, n_table, seed, n_total=N_TARGETS, with_inf=False):
    """Seeded targets of a row: every member of the table and its two fp32 neighbours, targets at or below the start, beyond the
    last member (within the recurrence's tail), NaN, -inf and NONE (and +inf), the rest uniform over the table's span"""
    rng = np.random.default_rng(seed)
    tab = members[:n_table]
    start, last, top = tab[0], tab[-1], members[-2]
    near = [tab, np.nextafter(tab, F(-np.inf)), np.nextafter(tab, F(np.inf))]
    below = np.array([start, np.nextafter(start, F(-np.inf)), 0.0, -0.0, -1.0, -start, start * F(0.5)], F)
    beyond = rng.uniform(last, top, 2000).astype(F)
    special = [np.nan, -np.inf, NONE] + ([np.inf] if with_inf else [])
    fixed = np.concatenate([*near, below, beyond, np.array(special, F)])
    rest = rng.uniform(float(start) - 0.1, float(last), max(0, n_total - len(fixed))).astype(F)
    t = np.concatenate([fixed, rest])
    return t[rng.permutation(len(t))]


@pytest.mark.parametrize("row", ROWS)
def test_the_table_is_the_recurrence(row):
    want, _ = _expected(row)
    got, _ = _call(row, [], np.zeros(0, F))
    assert len(got) == len(want), (row, len(got), len(want))
    assert np.array_equal(_bits(got), _bits(want)), (row, int(np.argmax(_bits(got) != _bits(want))))
    assert np.all(np.diff(got.astype(np.float64)) > 0), row
    assert _bits(got[:1])[0] == _bits(F(row[0])), row
    if row[1] == 0.0:  # the constant-dt_min sequence
        dt_min, _ = _consts(row[2], row[3])
        k = np.arange(1, min(len(got), 16))
        assert np.all(np.abs(got[k].astype(np.float64) - (float(F(row[0])) + k * float(dt_min))) < 1e-5), row


def test_the_rows_reach_every_regime():
    """Tables that end at the reach and tables the capacity cuts; steps of dt_min, of t * dt_gamma and of dt_max"""
    lengths = {row: len(_expected(row)[0]) for row in ROWS}
    assert any(n == CAPACITY for n in lengths.values()) and any(n < CAPACITY for n in lengths.values())
    seen = set()
    for row in ROWS:
        tab = _expected(row)[0]
        dt_min, dt_max = _consts(row[2], row[3])
        p = (tab[:-1] * F(row[1])).astype(F)
        seen |= {"min"} if np.any(p < dt_min) else set()
        seen |= {"max"} if np.any(p > dt_max) else set()
        seen |= {"gamma"} if np.any((p > dt_min) & (p < dt_max)) else set()
    assert seen == {"min", "max", "gamma"}


@pytest.mark.parametrize("row", ROWS)
def test_step_land_equals_the_loop(row):
    table, members = _expected(row)
    targets = _targets(row, members, len(table), seed=ROWS.index(row))
    assert len(targets) == N_TARGETS
    got_table, got = _call(row, table[0], targets)
    want = _loop(members, table[0], targets)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (row, targets[bad][:4], got[bad][:4], want[bad][:4])
    # what the targets held: members themselves, targets that move nothing, targets beyond the table
    assert np.isin(table, targets).all() and np.sum(~np.less(table[0], targets)) > 100 and np.sum(targets > table[-1]) > 1000
    assert np.sum(_bits(got) == _bits(table[0])) > 100 and np.sum(got > table[-1]) > 1000


@pytest.mark.parametrize("row", ROWS[::7])
def test_step_land_under_a_finite_far(row):
    """tb = min(barrier, far) in both fast-forward functions: +inf, and NaN, land where far does (fminf returns the other operand)"""
    table, members = _expected(row)
    for far in (F(0.5) * (members[len(table) + 20] + members[len(table) + 21]), F(0.5) * (table[len(table) // 2] + table[len(table) // 2 + 1])):
        targets = _targets(row, members, len(table), seed=1000 + ROWS.index(row), n_total=20_000, with_inf=True)
        _, got = _call(row, table[0], targets, far=float(far))
        want = _loop(members, table[0], np.fmin(targets, far))
        assert np.array_equal(_bits(got), _bits(want)), (row, far)
        assert _bits(got[np.isposinf(targets)])[0] == _bits(_loop(members, table[0], [far]))[0]


@pytest.mark.parametrize("row", ROWS)
def test_truncation_changes_nothing(row):
    table, members = _expected(row)
    targets = _targets(row, members, len(table), seed=2000 + ROWS.index(row), n_total=0)
    full_table, full = _call(row, table[0], targets)
    short_table, short = _call(row, table[0], targets, capacity=8)
    assert len(short_table) == 8 and np.array_equal(_bits(short_table), _bits(table[:8])), row
    assert np.array_equal(_bits(short), _bits(full)), row
    assert np.sum(targets > short_table[-1]) > 2000  # (the loop from the last member ran)


@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("side", [-1, 1])
def test_off_table_starts_fall_back_to_the_loop(row, side):
    table, members = _expected(row)
    start = np.nextafter(table[0], F(side * np.inf))
    own = _recurrence(start, row[1], row[2], row[3], lambda m: m[-1] > members[-1])
    targets = _targets(row, members, len(table), seed=3000 + ROWS.index(row), n_total=5000)
    _, got = _call(row, start, targets)
    want = _loop(own, start, targets)
    assert np.array_equal(_bits(got), _bits(want)), (row, side)
    moved = np.less(start, targets)
    assert moved.sum() > 4000 and not np.isin(got[moved], table).all()  # (its members are its own, not the table's)


def test_inputs_without_a_table():
    """dt_max below dt_min (the median of three is no clamp), a capacity below two entries: no table, step_land is the loop"""
    row = (0.2, 1.0 / 256, 0.5, 512)
    tab, landed = _call(row, [0.2, 0.2], np.array([0.1, np.nan], F))
    assert len(tab) == 0 and np.array_equal(_bits(landed), _bits(np.array([0.2, 0.2], F)))
    tab, _ = _call(ROWS[0], [], np.zeros(0, F), capacity=1)
    assert len(tab) == 0


def test_the_table_has_the_lowest_priority_in_lds():
    """step_table_lds_offset: behind the launch's bytes, 16-byte aligned, only if the whole table fits the compute unit"""
    lib = nh.load_library()
    fp = C.POINTER(C.c_float)
    fn = lib.nrf_debug_step_table
    fn.restype = C.c_int
    fn.argtypes = [C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_int, fp, C.POINTER(C.c_int), C.c_int, fp, fp, C.c_float, fp,
                   C.POINTER(C.c_int32)]
    cu = 160 * 1024
    for lds, n, want in ((1000, 600, 1008), (cu - 4096, 1024, cu - 4096), (cu - 4095, 1024, -1), (cu - 4080, 1020, cu - 4080), (cu, 1, -1),
                         (5000, 0, -1)):
        table = np.zeros(8, F)
        cnt = C.c_int(0)
        io = (C.c_int32 * 4)(lds, n, cu, 7)
        assert fn(0.2, 0.0, 1.0, 128, 8, table.ctypes.data_as(fp), C.byref(cnt), 0, None, None, np.inf, None, io) == nh.NRF_OK
        assert io[3] == want, (lds, n, io[3], want)
