"""Static gather plans change no bit: the hot instance's persistent kernel under a static plan (the form of each of a sample's
four gather steps fixed at compile time: csrc/nrf_launch.h) against the same kernel selecting the forms at run time
(NRF_GATHER_PLAN=0 at context creation), for the three budgets that reach the three plans -- float planes, depth, composited
samples and the lane addresses a sample gathers must be identical.  One view, and one launch of three views (which switches the
per-round sample cap on); launches this small are all tail, so the tail-splitting copy of the tile program runs as well."""
import os

import numpy as np
import pytest

import models
import nerfhip as nh
import synthetic as syn
from test_gather_plan_cpu import DMHH, GATHER_RUNTIME, QQFH, QQHH, gather_plan, plan_id

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H = 96, 64


def _context(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return nh.NerfHip(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _frames(desc, budget_mb, env):
    """[(rgba, depth, n_composited, gather addresses per sample)] of one view and of one launch of three views"""
    d = nh.ModelDesc.from_buffer_copy(desc)  # (the pointers stay the caller's)
    d.gather_copy_budget_mb = budget_mb
    ctx = _context(env)
    out = []
    try:
        ctx.load_model(d)
        ctx.set_resolution(W, H)
        for n in (1, 3):
            poses = [syn.orbit_pose(40.0 + 70.0 * i, (25.0, -10.0, 50.0)[i]) for i in range(n)]
            rgba = torch.full((n, W * H, 4), 7.0, device="cuda")
            depth = torch.full((n, W * H), 7.0, device="cuda")
            torch.cuda.synchronize()
            ctx.bind_output(rgba.data_ptr(), depth.data_ptr())
            ctx.render_views(np.stack([syn.default_camera(W, H)] * n), np.stack(poses))
            st = ctx.stats()
            assert st.n_composited > 0
            out.append((rgba.cpu().numpy(), depth.cpu().numpy(), int(st.n_composited), int(st.gather_addresses_per_sample)))
    finally:
        ctx.close()
    return out


def _same(a, b, what):
    for (rgba_a, depth_a, comp_a, addr_a), (rgba_b, depth_b, comp_b, addr_b), views in zip(a, b, (1, 3)):
        assert not np.any(rgba_a == 7.0) and not np.any(depth_a == 7.0), (what, views)  # every pixel was written
        np.testing.assert_array_equal(rgba_a.view(np.uint32), rgba_b.view(np.uint32), err_msg=f"{what}, {views} view(s)")
        np.testing.assert_array_equal(depth_a.view(np.uint32), depth_b.view(np.uint32), err_msg=f"{what}, {views} view(s)")
        assert comp_a == comp_b and addr_a == addr_b, (what, views)


@pytest.fixture(scope="module")
def base_19():
    return models.build_model(log2_hashmap_size=19, H=32)


# (explicit budgets: the default one depends on the device's free memory; the far plan needs the copies to pass 4 GiB)
@pytest.mark.parametrize("budget_mb, forms, addrs", [(1, DMHH, 128), (256, QQHH, 80), (6000, QQFH, 56)])
def test_static_plan_changes_no_bit(base_19, budget_mb, forms, addrs):
    desc, keep, _ = base_19
    assert gather_plan(desc, 1, budget_mb) == (nh.NRF_OK, plan_id(forms), forms)  # this budget runs this plan's instances
    static = _frames(desc, budget_mb, {"NRF_GATHER_PLAN": "1"})
    runtime = _frames(desc, budget_mb, {"NRF_GATHER_PLAN": "0"})
    assert static[0][3] == addrs, static[0][3]
    _same(static, runtime, f"budget {budget_mb} MB")


def test_run_time_plan_against_the_per_strip_kernel():
    """log2 T = 12 without copies (step 0 mixed) has no static plan: the persistent kernel runs GATHER_RUNTIME with the switch on or
    off, and equals the per-strip kernel (NRF_PERSISTENT=0) as before."""
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    assert gather_plan(desc, 1, 1)[1] == GATHER_RUNTIME
    on = _frames(desc, 1, {"NRF_GATHER_PLAN": "1"})
    off = _frames(desc, 1, {"NRF_GATHER_PLAN": "0"})
    strip = _frames(desc, 1, {"NRF_PERSISTENT": "0"})
    assert on[0][3] == 128
    _same(on, off, "log2 T = 12, switch")
    _same(on, strip, "log2 T = 12, per-strip kernel")
