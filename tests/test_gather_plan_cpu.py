"""The gather plan the host's GPU-free model plan chooses (nrf_debug_gather_plan, an undeclared diagnostic of libnerfhip.so next
to nrf_debug_plan): the hot instance's persistent kernel exists under three static plans -- the form of each of a sample's four
gather steps fixed at compile time -- and every model whose steps have other forms, every other instance, and every model under
NRF_GATHER_PLAN=0 keeps the run-time selection (GATHER_RUNTIME)."""
import ctypes as C
import os

import pytest

import models
import nerfhip as nh
from probe_model import GFORM_DENSE as DENSE, GFORM_HASHED as HASHED, GFORM_MIXED as MIXED, GFORM_QUAD as QUAD, GFORM_QUAD_FAR as QUAD_FAR  # step forms
from probe_model import plan_id  # noqa: F401  (gather_plan() of csrc/nrf_launch.h)

GATHER_RUNTIME = 0


QQFH = (QUAD, QUAD, QUAD_FAR, HASHED)
QQHH = (QUAD, QUAD, HASHED, HASHED)
DMHH = (DENSE, MIXED, HASHED, HASHED)


def gather_plan(desc, allow_own=1, budget_mb=0, env=None):
    """(status, plan, the four steps' forms); env: NRF_GATHER_PLAN's value while the plan is made"""
    lib = nh.load_library()
    lib.nrf_debug_gather_plan.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.nrf_debug_gather_plan.restype = C.c_int
    out = (C.c_uint32 * 5)()
    saved = os.environ.get("NRF_GATHER_PLAN")
    if env is not None:
        os.environ["NRF_GATHER_PLAN"] = env
    else:
        os.environ.pop("NRF_GATHER_PLAN", None)
    try:
        rc = lib.nrf_debug_gather_plan(C.byref(desc), allow_own, budget_mb, out)
    finally:
        if saved is None:
            os.environ.pop("NRF_GATHER_PLAN", None)
        else:
            os.environ["NRF_GATHER_PLAN"] = saved
    return rc, int(out[0]), tuple(out[1:])


# budgets of tests/test_instance_plan_cpu.py: 0 = the default (8192 MB: levels 0..11 copied, 8..11 beyond 4 GiB), 100 MB (levels
# 0..7), 1 MB (no copies)
@pytest.mark.parametrize("budget_mb, forms", [(0, QQFH), (8192, QQFH), (100, QQHH), (1, DMHH)])
def test_base_json_selects_a_static_plan_at_each_budget(budget_mb, forms):
    desc, keep, _ = models.build_model()
    for allow_own in (1, 0):
        assert gather_plan(desc, allow_own, budget_mb) == (nh.NRF_OK, plan_id(forms), forms)
        assert gather_plan(desc, allow_own, budget_mb, env="1") == (nh.NRF_OK, plan_id(forms), forms)
        assert gather_plan(desc, allow_own, budget_mb, env="0") == (nh.NRF_OK, GATHER_RUNTIME, forms)  # (the forms are the model's)


def test_the_three_plans_are_distinct():
    assert len({plan_id(QQFH), plan_id(QQHH), plan_id(DMHH), GATHER_RUNTIME}) == 4


def test_another_dense_hashed_split_keeps_the_run_time_selection():
    """log2 T = 12: only level 0 is dense, so without copies step 0 is mixed and step 1 hashed -- no static plan has these forms.
    (A step gathered from quad copies has the quad form whatever its levels' index modes are: with copies of levels 0..7 the same
    table runs {quad, quad, hashed, hashed}.)"""
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    forms = (MIXED, HASHED, HASHED, HASHED)
    assert gather_plan(desc, 1, 1) == (nh.NRF_OK, GATHER_RUNTIME, forms)
    assert gather_plan(desc, 1, 1, env="0") == (nh.NRF_OK, GATHER_RUNTIME, forms)
    assert gather_plan(desc, 1, 100) == (nh.NRF_OK, plan_id(QQHH), QQHH)
    assert gather_plan(desc, 1, 100, env="0") == (nh.NRF_OK, GATHER_RUNTIME, QQHH)


@pytest.mark.parametrize("kw", [dict(dir_otype="Frequency", n_frequencies=12),           # NET_WIDE
                                dict(n_levels=8), dict(n_features_per_level=4, n_levels=8),  # GRID models
                                dict(activation="Sine"), dict(n_neurons=32, density_hidden_layers=2),  # the generic instance
                                dict(n_neurons=32), dict(density_hidden_layers=2)],           # width / depth instances
                         ids=["wide", "grid2", "grid4", "sine", "generic", "w32", "depth"])
@pytest.mark.parametrize("log2T", [12, 19])
def test_other_instances_keep_the_run_time_selection(kw, log2T):
    """(at log2 T = 19 the wide / width / depth instances' steps have exactly a static plan's forms: the plans are NET_HOT's alone)"""
    desc, keep, _ = models.build_model(log2_hashmap_size=log2T, H=32, **kw)
    for allow_own in (1, 0):
        for budget_mb in (0, 100, 1):
            for env in (None, "0"):
                rc, plan, _ = gather_plan(desc, allow_own, budget_mb, env=env)
                assert rc == nh.NRF_OK and plan == GATHER_RUNTIME, (kw, allow_own, budget_mb, env)


def test_debug_plan_is_unchanged_by_the_switch():
    """nrf_debug_plan's six outputs (tests/test_instance_plan_cpu.py) do not depend on NRF_GATHER_PLAN"""
    lib = nh.load_library()
    lib.nrf_debug_plan.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.nrf_debug_plan.restype = C.c_int
    desc, keep, _ = models.build_model()
    got = []
    for env in (None, "0"):
        saved = os.environ.get("NRF_GATHER_PLAN")
        if env is not None:
            os.environ["NRF_GATHER_PLAN"] = env
        try:
            out = (C.c_uint32 * 6)()
            assert lib.nrf_debug_plan(C.byref(desc), 1, 8192, out) == nh.NRF_OK
            got.append(tuple(out))
        finally:
            if saved is None:
                os.environ.pop("NRF_GATHER_PLAN", None)
            else:
                os.environ["NRF_GATHER_PLAN"] = saved
    assert got[0] == got[1] == (0, 0, 0xFFF, 0b100, 16, 79464)
