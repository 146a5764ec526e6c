"""The grid side of a loaded context on the GPU (nrf_debug_grid_readout, an undeclared diagnostic: DevModel's grid fields, the fit
the context keeps, its four device tables copied back) equals the plan made without a device (nrf_debug_grid_plan) and what the
commit before plan_grid had in its context on an MI355X (tests/golden/grid_plan_parent.json; rows: tests/grid_plan_rows.py)."""
import os
import zlib

import numpy as np
import pytest

import grid_plan_rows as R
import nerfhip as nh

pytestmark = pytest.mark.gpu


def _context(flags):
    """A context with the flags' environment in force at its creation (nrf_create reads it)."""
    env = R.env_of(flags)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return nh.NerfHip(0)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _check(ctx, desc, grid, mean, flags, want):
    got, box, tables = R.readout(ctx)
    plan, pbox, ptables = R.plan(desc, grid, mean, flags)
    assert got == {k: plan[k] for k in R.FIELDS}
    assert np.array_equal(box.view(np.uint32), pbox.view(np.uint32))
    for t, p in zip(tables, ptables):
        assert t.size == p.size and np.array_equal(t.view(np.uint32), p.view(np.uint32))
    assert R.record(got, box, tables) == {k: want[k] for k in ("fields", "box_bits", "crc32")}


@pytest.mark.parametrize("name", R.GPU_ROWS)
def test_loaded_context_has_the_plan(name):
    row = R.ROWS[name]
    desc, keep, grid = R.build(row)
    ctx = _context(row["flags"])
    try:
        ctx.load_model(desc)
        _check(ctx, desc, grid, row["mean"], row["flags"], R.golden()[name])
    finally:
        ctx.close()


def test_generated_grid_is_planned_like_a_loaded_one():
    """a model loaded without a grid, then nrf_generate_density_grid: the plan of what nrf_read_density_grid returns"""
    row = R.ROWS["h32-unit"]
    desc, keep, _ = R.build(row, with_grid=False)
    ctx = _context(R.ALL)
    try:
        ctx.load_model(desc)
        ctx.generate_density_grid()
        grid, mean = ctx.read_density_grid(row["H"] ** 3)
        want = R.golden()[R.GENERATED]
        assert zlib.crc32(grid.tobytes()) == want["grid_crc32"] and mean == want["mean"]
        _check(ctx, desc, grid, mean, R.ALL, want)
    finally:
        ctx.close()
