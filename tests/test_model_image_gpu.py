"""The model image of a loaded context on the GPU (nrf_debug_model_readout, an undeclared diagnostic: d_wfrag, d_wfrag_gen, d_wfrag_hot,
d_gen, d_lv and the reference-order part of d_grid copied back, the plan's words of its DevModel) equals the image made without a
device (nrf_debug_model_image) and what the commit before csrc/nrf_model_plan.h held in its context on an MI355X
(tests/golden/model_image_parent.json; rows: tests/model_image_rows.py).  No frame is rendered; the quad copies themselves are built
by a device kernel and are not read back."""
import numpy as np
import pytest

import model_image_rows as R
import nerfhip as nh

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", R.GPU_ROWS)
def test_loaded_context_holds_the_image(name):
    row = R.ROWS[name]
    desc, keep, budget = R.build(row)  # (the descriptor carries the budget: gather_copy_budget_mb)
    ctx = nh.NerfHip(0)
    try:
        ctx.load_model(desc)
        got = R.readout(ctx)
    finally:
        ctx.close()
    want = R.image(desc, budget, row["flags"])
    for part in R.PARTS:
        assert got[part].size == want[part].size and np.array_equal(got[part], want[part]), part
    assert R.record(got) == R.golden()[name]
