"""The LDS schedule of the static-plan hot instances changes no bit (csrc/nrf_launch.h: plan_levels, plan_frag_depth): level
parameters read from the staged compact blocks in one go, weight fragments read one or two ahead of their MFMAs, against the same
library's run-time selection (NRF_GATHER_PLAN=0: the kernel as it was before either), in a fresh context each.  Float planes,
depth and composited samples must be identical.  The shapes are the smallest at which a misplaced read could show: one 8 x 8 tile
(rounds of 1-16 samples: one-tile passes only), 40 x 24 pixels with max_steps 1, 7 and 9 (sample counts that are no multiple of
16, odd tile counts), one launch of three views (per-round sample cap on, tail splitting), and the 8-bit output instances once;
three budgets, so that all three plans run."""
import os

import numpy as np
import pytest

import models
import nerfhip as nh
import synthetic as syn

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


def _frames(desc, env):
    """[(planes..., n_composited)] of CASES, and the gather addresses per sample (which tells the steps' forms)"""
    ctx = _context(env)
    out = []
    try:
        ctx.load_model(desc)
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


@pytest.fixture(scope="module")
def base_19():
    return models.build_model(log2_hashmap_size=19, H=32)


# NRF_QUAD_BUDGET_MB: 0 = no copies {dense, mixed, hashed, hashed}; 95 = levels 0..7 {quad, quad, hashed, hashed}; unset = the
# default budget {quad, quad, quad-far, hashed} -- 128 / 80 / 56 lane addresses per sample
@pytest.mark.parametrize("budget, addrs", [("0", 128), ("95", 80), (None, 56)])
def test_lds_schedule_changes_no_bit(base_19, budget, addrs):
    desc, keep, _ = base_19
    new, new_addrs = _frames(desc, {"NRF_QUAD_BUDGET_MB": budget, "NRF_GATHER_PLAN": "1"})
    old, old_addrs = _frames(desc, {"NRF_QUAD_BUDGET_MB": budget, "NRF_GATHER_PLAN": "0"})
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
