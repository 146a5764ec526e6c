"""The pair gather of the static-plan hot instances changes no bit (csrc/nrf_launch.h: pair_gather; csrc/nrf_render.h:
pair_features): a pass of two full tiles gathers both tiles step by step, against the same library's run-time selection
(NRF_GATHER_PLAN=0: the tile-major kernel the static plans were held to), in a fresh context each.  Float planes, depth and
composited samples must be identical, and every pixel written.  The shapes are the smallest at which a step-major pass could go
wrong: one 8 x 8 tile (a first round of 64 samples -- two passes of two full tiles --, later rounds whose sample counts walk down
through a partly filled second tile, which keeps the tile-major pass, and a one-tile pass right behind a two-tile one), 16 x 8
(two tiles per strip), 40 x 24 pixels with max_steps 1, 7, 9 and the default (sample counts that are no multiple of 16 or 32),
one launch of three views (per-round sample cap on, tail splitting: a helper wave runs the same pass), and the 8-bit output
instance once; three budgets, so that all three plans run, in every march cell."""
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
CASES = [(8, 8, 1, None, False), (16, 8, 1, None, False), (40, 24, 1, 1, False), (40, 24, 1, 7, False), (40, 24, 1, 9, False),
         (40, 24, 1, None, False), (40, 24, 3, None, False), (40, 24, 3, None, True)]
POISON = 7.0


def _frames(desc, env, instance, plan):
    """[(colour plane, depth plane, n_composited)] of CASES; `instance`: what nrf_debug_instance must say renders the model (16:
    the hot instance's persistent kernel, 0: its per-strip kernel); `plan`: the gather plan the context must launch with"""
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
                a = torch.full((n, W * H, 4), POISON, device="cuda")
                b = torch.full((n, W * H), POISON, device="cuda")
                torch.cuda.synchronize()
                ctx.bind_output(a.data_ptr(), b.data_ptr())
            ctx.render_views(cams, np.stack(poses))
            st = ctx.stats()
            assert st.n_composited > 0
            out.append((a.cpu().numpy(), b.cpu().numpy(), int(st.n_composited)))
            if u8:
                ctx.bind_output_u8(0, 0)
            else:
                ctx.bind_output(0, 0)
    finally:
        ctx.close()
    return out


_MODELS = {}


def _model(cell):
    """base.json's grid in one of the four march cells of the plan matrix (probe_model.PLAN_CELLS).  Kept: a cell's legs share it."""
    if cell not in _MODELS:
        _MODELS[cell] = models.build_model(**pm.resolve(dict(pm.T19, **pm.PLAN_CELLS[cell][0])))
    return _MODELS[cell]


# NRF_QUAD_BUDGET_MB: 0 = no copies {dense, mixed, hashed, hashed}; 95 = levels 0..7 {quad, quad, hashed, hashed}; unset = the
# default budget {quad, quad, quad-far, hashed}.  generic_h renders in the per-strip kernel, which has no static plan: the switch
# must change nothing there either.
@pytest.mark.parametrize("cell", list(pm.PLAN_CELLS))
@pytest.mark.parametrize("budget, plan", [("0", "dmhh"), ("95", "qqhh"), (None, "qqfh")])
def test_pair_gather_changes_no_bit(cell, budget, plan):
    desc, _, _ = _model(cell)
    forms = pm.PLANS[plan][1]
    gp_budget = 1 if budget == "0" else int(budget or 0)  # (nrf_debug_gather_plan: 0 is the default budget, 1 MB grants no copy)
    assert gather_plan(desc, 1, gp_budget, env="1") == (nh.NRF_OK, pm.plan_id(forms), forms)
    assert gather_plan(desc, 1, gp_budget, env="0") == (nh.NRF_OK, GATHER_RUNTIME, forms)
    instance = 16 if pm.plan_sched(cell) == "persistent" else 0
    new = _frames(desc, {"NRF_QUAD_BUDGET_MB": budget, "NRF_GATHER_PLAN": "1"}, instance, pm.plan_id(forms))
    old = _frames(desc, {"NRF_QUAD_BUDGET_MB": budget, "NRF_GATHER_PLAN": "0"}, instance, GATHER_RUNTIME)
    for case, (a_n, b_n, comp_n), (a_o, b_o, comp_o) in zip(CASES, new, old):
        if case[4]:
            np.testing.assert_array_equal(a_n, a_o, err_msg=str(case))
            np.testing.assert_array_equal(b_n, b_o, err_msg=str(case))
        else:
            assert not np.any(a_n == POISON) and not np.any(b_n == POISON), case  # every pixel was written
            np.testing.assert_array_equal(a_n.view(np.uint32), a_o.view(np.uint32), err_msg=str(case))
            np.testing.assert_array_equal(b_n.view(np.uint32), b_o.view(np.uint32), err_msg=str(case))
        assert comp_n == comp_o, case
