"""The LDS schedule of the static-plan hot instances changes no bit (csrc/nrf_launch.h: plan_levels, plan_frag_depth): level
parameters read from the staged compact blocks in one go, weight fragments read one or two ahead of their MFMAs, against the same
library's run-time selection (NRF_GATHER_PLAN=0: the kernel as it was before either), in a fresh context each.  Float planes,
depth and composited samples must be identical.  The shapes are the smallest at which a misplaced read could show: one 8 x 8 tile
(rounds of 1-16 samples: one-tile passes only), 40 x 24 pixels with max_steps 1, 7 and 9 (sample counts that are no multiple of
16, odd tile counts), one launch of three views (per-round sample cap on, tail splitting), and the 8-bit output instances once;
three budgets, so that all three plans run."""
import ctypes as C
import os

import numpy as np
import pytest

import models
import nerfhip as nh
import probe_model as pm
import synthetic as syn
from test_gather_plan_cpu import GATHER_RUNTIME, gather_plan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _context(env):
    saved = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return nh.NerfHip(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# (width, height, views, max_steps or None for the default, 8-bit output)
CASES = [(8, 8, 1, None, False), (40, 24, 1, 1, False), (40, 24, 1, 7, False), (40, 24, 1, 9, False), (40, 24, 1, None, False),
         (40, 24, 3, None, False), (40, 24, 3, None, True)]


def _frames(desc, env, instance, plan):
    """[(planes..., n_composited)] of CASES, and the gather addresses per sample (which tells the steps' forms); `instance`:
    what nrf_debug_instance must say renders the model (16: the hot instance's persistent kernel, 0: its per-strip kernel);
    `plan`: the gather plan the context must launch with (nrf_debug_context_gather_plan)"""
    ctx = _context(env)
    out = []
    try:
        ctx.load_model(desc)
        ctx.lib.nrf_debug_instance.argtypes = [C.c_void_p]
        assert ctx.lib.nrf_debug_instance(ctx.h) == instance, (env, ctx.lib.nrf_debug_instance(ctx.h))
        ctx.lib.nrf_debug_context_gather_plan.argtypes, ctx.lib.nrf_debug_context_gather_plan.restype = [C.c_void_p], C.c_longlong
        assert ctx.lib.nrf_debug_context_gather_plan(ctx.h) == plan, (env, hex(ctx.lib.nrf_debug_context_gather_plan(ctx.h)))
        for W, H, n, max_steps, u8 in CASES:
            ctx.set_resolution(W, H)
            o = nh.default_options()
            if max_steps is not None:
                o.max_steps = max_steps
            ctx.set_options(o)
            poses = [syn.orbit_pose(40.0 + 70.0 * i, (25.0, -10.0, 50.0)[i]) for i in range(n)]
            cams = np.stack([syn.default_camera(W, H)] * n)
            if u8:
                a = torch.full((n, H, W, 3), 77, dtype=torch.uint8, device="cuda")
                b = torch.full((n, H, W), 78, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ctx.bind_output_u8(a.data_ptr(), b.data_ptr())
            else:
                a = torch.full((n, W * H, 4), 7.0, device="cuda")
                b = torch.full((n, W * H), 7.0, device="cuda")
                torch.cuda.synchronize()
                ctx.bind_output(a.data_ptr(), b.data_ptr())
            ctx.render_views(cams, np.stack(poses))
            st = ctx.stats()
            assert st.n_composited > 0
            out.append((a.cpu().numpy(), b.cpu().numpy(), int(st.n_composited)))
            addrs = int(st.gather_addresses_per_sample)
            if u8:
                ctx.bind_output_u8(0, 0)
            else:
                ctx.bind_output(0, 0)
    finally:
        ctx.close()
    return out, addrs


_MODELS = {}


def _model(cell, act):
    """base.json's grid in one of the four march cells of the plan matrix (probe_model.PLAN_CELLS), rgb output None or Sigmoid; the
    unit cell with no output activation is the model this file has always rendered.  Kept: a module's legs share them."""
    if (cell, act) not in _MODELS:
        kw = dict(pm.resolve(dict(pm.T19, **pm.PLAN_CELLS[cell][0])), rgb_output_activation=act)
        if (cell, act) == ("unit", "None"):
            kw = dict(log2_hashmap_size=19, H=32)
        _MODELS[(cell, act)] = models.build_model(**kw)
    return _MODELS[(cell, act)]


# NRF_QUAD_BUDGET_MB: 0 = no copies {dense, mixed, hashed, hashed}; 95 = levels 0..7 {quad, quad, hashed, hashed}; unset = the
# default budget {quad, quad, quad-far, hashed} -- 128 / 80 / 56 lane addresses per sample.
# The model: every march cell, so that the MARCH_UNIT, MARCH_POW2 and MARCH_GENERIC instances of each plan run (generic_h renders
# in the per-strip kernel, which has no static plan: the switch must change nothing there either), and rgb output Sigmoid --
# v_exp_f32 against libm leaves it no exact reference: equality with the run-time selection is its check.
@pytest.mark.parametrize("act", ["None", "Sigmoid"])
@pytest.mark.parametrize("cell", list(pm.PLAN_CELLS))
@pytest.mark.parametrize("budget, addrs, plan", [("0", 128, "dmhh"), ("95", 80, "qqhh"), (None, 56, "qqfh")])
def test_lds_schedule_changes_no_bit(cell, act, budget, addrs, plan):
    desc, keep, _ = _model(cell, act)
    # the plan each context makes, before anything renders: the static one, and the run-time selection of the same forms
    forms = pm.PLANS[plan][1]
    gp_budget = 1 if budget == "0" else int(budget or 0)  # (nrf_debug_gather_plan: 0 is the default budget, 1 MB grants no copy)
    assert gather_plan(desc, 1, gp_budget, env="1") == (nh.NRF_OK, pm.plan_id(forms), forms)
    assert gather_plan(desc, 1, gp_budget, env="0") == (nh.NRF_OK, GATHER_RUNTIME, forms)
    instance = 16 if pm.plan_sched(cell) == "persistent" else 0  # the persistent kernel, but for the grid without a coarse level
    new, new_addrs = _frames(desc, {"NRF_QUAD_BUDGET_MB": budget, "NRF_GATHER_PLAN": "1"}, instance, pm.plan_id(forms))
    old, old_addrs = _frames(desc, {"NRF_QUAD_BUDGET_MB": budget, "NRF_GATHER_PLAN": "0"}, instance, GATHER_RUNTIME)
    assert new_addrs == addrs and old_addrs == addrs, (new_addrs, old_addrs)
    for case, (a_n, b_n, comp_n), (a_o, b_o, comp_o) in zip(CASES, new, old):
        if case[4]:
            np.testing.assert_array_equal(a_n, a_o, err_msg=str(case))
            np.testing.assert_array_equal(b_n, b_o, err_msg=str(case))
        else:
            assert not np.any(a_n == 7.0) and not np.any(b_n == 7.0), case  # every pixel was written
            np.testing.assert_array_equal(a_n.view(np.uint32), a_o.view(np.uint32), err_msg=str(case))
            np.testing.assert_array_equal(b_n.view(np.uint32), b_o.view(np.uint32), err_msg=str(case))
        assert comp_n == comp_o, case
