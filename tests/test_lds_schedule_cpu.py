"""LDS schedule of the static-plan hot instances (csrc/nrf_launch.h: plan_levels, plan_frag_depth).

The counting function of scripts/lds_wait_listing.py on hand-written listings -- an exposed LDS wait is an `s_waitcnt lgkmcnt(N)`
whose youngest retired operation is a ds_read issued at most 8 instructions earlier, the counter modelled in order with
scalar-memory loads counted and emptied at labels -- and the host's view of which instances are compiled with the schedule
(nrf_debug_lds_schedule, an undeclared diagnostic next to nrf_debug_gather_plan): the three static plans, nothing else."""
import ctypes as C
import importlib.util
from pathlib import Path

import pytest

import models
import nerfhip as nh
from test_gather_plan_cpu import DMHH, GATHER_RUNTIME, QQFH, QQHH, gather_plan, plan_id

_spec = importlib.util.spec_from_file_location("lds_wait_listing", Path(__file__).resolve().parents[1] / "scripts" / "lds_wait_listing.py")
lwl = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lwl)


def _listing(body):
    return [ln for ln in body.strip("\n").splitlines()]


def test_a_wait_right_behind_its_read_is_exposed():
    lines = _listing("""
	ds_read_b128 v[0:3], v9
	v_add_u32_e32 v8, 1, v8
	s_waitcnt lgkmcnt(0)
	v_mfma_f32_16x16x32_f16 v[4:7], v[0:3], v[10:13], 0
""")
    assert lwl.exposed_lds_waits(lines) == [3]


def test_a_read_more_than_eight_instructions_back_is_covered():
    far = "\tds_read_b128 v[0:3], v9\n" + "\tv_add_u32_e32 v8, 1, v8\n" * 8 + "\ts_waitcnt lgkmcnt(0)\n"
    near = "\tds_read_b128 v[0:3], v9\n" + "\tv_add_u32_e32 v8, 1, v8\n" * 7 + "\ts_waitcnt lgkmcnt(0)\n"
    assert lwl.exposed_lds_waits(far.splitlines()) == []      # the wait is the ninth instruction behind the read
    assert lwl.exposed_lds_waits(near.splitlines()) == [9]    # the eighth


def test_a_counted_wait_retires_the_older_read_only():
    # lgkmcnt(1) leaves the second read in flight: what it retires is the first one, twelve instructions back -- covered; the
    # lgkmcnt(0) behind it retires the second read, three instructions back -- exposed
    lines = _listing("\tds_read_b128 v[0:3], v9\n" + "\tv_add_u32_e32 v8, 1, v8\n" * 10 + """
	ds_read_b128 v[4:7], v9 offset:1024
	s_waitcnt lgkmcnt(1)
	v_mfma_f32_16x16x32_f16 v[20:23], v[0:3], v[10:13], 0
	s_waitcnt lgkmcnt(0)
	v_mfma_f32_16x16x32_f16 v[24:27], v[4:7], v[10:13], 0
""")
    assert lwl.exposed_lds_waits(lines) == [15]
    # the same pair back to back: the counted wait retires a read one instruction old
    pair = _listing("""
	ds_read_b128 v[0:3], v9
	ds_read_b128 v[4:7], v9 offset:1024
	s_waitcnt lgkmcnt(1)
	s_waitcnt lgkmcnt(0)
""")
    assert lwl.exposed_lds_waits(pair) == [3, 4]


def test_a_scalar_load_in_between_is_counted():
    # the youngest operation the wait retires is the scalar load, not the read: not an LDS wait
    lines = _listing("""
	ds_read_b128 v[0:3], v9
	s_load_dword s50, s[0:1], 0xac
	s_waitcnt lgkmcnt(0)
""")
    assert lwl.exposed_lds_waits(lines) == []
    # ... and it holds a place in the counter: lgkmcnt(1) retires the read and leaves the scalar load
    lines = _listing("""
	ds_read_b128 v[0:3], v9
	s_load_dword s50, s[0:1], 0xac
	s_waitcnt lgkmcnt(1)
""")
    assert lwl.exposed_lds_waits(lines) == [3]
    # an LDS write is counted as well, and is not a read
    lines = _listing("""
	ds_read_b32 v0, v9
	ds_write_b32 v9, v1
	s_waitcnt vmcnt(0) lgkmcnt(0)
""")
    assert lwl.exposed_lds_waits(lines) == []


def test_a_label_empties_the_counter():
    lines = _listing("""
	ds_read_b128 v[0:3], v9
.LBB0_2:                                ; %bb
	s_waitcnt lgkmcnt(0)
	v_mfma_f32_16x16x32_f16 v[4:7], v[0:3], v[10:13], 0
""")
    assert lwl.exposed_lds_waits(lines) == []


def test_directives_comments_and_vector_memory_waits_do_not_count():
    lines = _listing("""
	.p2align 8
	; a comment
	ds_read_b32 v0, v9
	; sched_barrier mask(0x00000676)
	s_waitcnt vmcnt(3)
	buffer_load_dword v1, v2, s[4:7], 0 offen
	s_waitcnt lgkmcnt(0)                    ; three instructions behind the read
""")
    assert lwl.exposed_lds_waits(lines) == [4]


def test_functions_and_the_pass_trace():
    text = """
	.text
_ZN3nrf1aEv:
	s_nop 0
.Lfunc_end0:
_ZN3nrf1bEv:
	ds_read_b128 v[14:17], v9
	s_waitcnt lgkmcnt(0)
	buffer_load_dwordx4 v[0:3], v8, s[4:7], 0 offen
	s_waitcnt vmcnt(0)
	ds_read_b128 v[4:7], v9
	s_waitcnt lgkmcnt(0)
	v_mfma_f32_16x16x32_f16 v[20:23], v[4:7], v[0:3], 0
	s_endpgm
.Lfunc_end1:
"""
    fs = lwl.functions(text)
    assert list(fs) == ["_ZN3nrf1aEv", "_ZN3nrf1bEv"]
    assert list(lwl.functions(text, "nrf::b")) == ["_ZN3nrf1bEv"]
    trace, inside = lwl.network_pass(fs["_ZN3nrf1bEv"])
    assert (trace, inside) == ("d[l0]!L[v0]d[l0]!M", 2)
    assert lwl.network_pass(fs["_ZN3nrf1aEv"]) == ("", 0)


# ---- which instances are compiled with the schedule

from probe_model import FORM_GENERIC, FORM_POW2, FORM_UNIT  # noqa: E402  (csrc/nrf_launch.h: MARCH_FORM_*)


def lds_schedule(plan, form):
    lib = nh.load_library()
    lib.nrf_debug_lds_schedule.argtypes = [C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]
    lib.nrf_debug_lds_schedule.restype = C.c_int
    out = (C.c_uint32 * 2)(7, 7)
    rc = lib.nrf_debug_lds_schedule(plan, form, out)
    return rc, tuple(out)


@pytest.mark.parametrize("forms", [QQFH, QQHH, DMHH])
def test_every_static_plan_instance_has_the_schedule(forms):
    # compact level blocks in all of them; two fragments ahead, one in the MARCH_GENERIC instances (no registers for two)
    assert lds_schedule(plan_id(forms), FORM_UNIT) == (nh.NRF_OK, (1, 2))
    assert lds_schedule(plan_id(forms), FORM_POW2) == (nh.NRF_OK, (1, 2))
    assert lds_schedule(plan_id(forms), FORM_GENERIC) == (nh.NRF_OK, (1, 1))


def test_the_run_time_selection_has_none():
    for form in (FORM_GENERIC, FORM_UNIT, FORM_POW2):
        assert lds_schedule(GATHER_RUNTIME, form) == (nh.NRF_OK, (0, 0))
    assert lds_schedule(plan_id((3, 3, 3, 3)), FORM_UNIT)[0] != nh.NRF_OK  # not a plan an instance exists for
    assert lds_schedule(plan_id(QQFH), 3)[0] != nh.NRF_OK


@pytest.mark.parametrize("budget_mb, forms", [(0, QQFH), (100, QQHH), (1, DMHH)])
def test_base_json_reaches_the_schedule_and_the_switch_leaves_it(budget_mb, forms):
    desc, keep, _ = models.build_model()
    rc, plan, _ = gather_plan(desc, 1, budget_mb)
    assert rc == nh.NRF_OK and plan == plan_id(forms)
    assert lds_schedule(plan, FORM_UNIT) == (nh.NRF_OK, (1, 2))
    rc, plan, _ = gather_plan(desc, 1, budget_mb, env="0")  # NRF_GATHER_PLAN=0: the parent's kernel
    assert rc == nh.NRF_OK and lds_schedule(plan, FORM_UNIT) == (nh.NRF_OK, (0, 0))


@pytest.mark.parametrize("kw", [dict(dir_otype="Frequency", n_frequencies=12), dict(n_levels=8), dict(activation="Sine"),
                                dict(n_neurons=32), dict(density_hidden_layers=2), dict(log2_hashmap_size=12)],
                         ids=["wide", "grid2", "generic", "w32", "depth", "log2T12"])
def test_other_instances_do_not(kw):
    desc, keep, _ = models.build_model(**{"log2_hashmap_size": 19, "H": 32, **kw})
    rc, plan, _ = gather_plan(desc, 1, 1)
    assert rc == nh.NRF_OK and plan == GATHER_RUNTIME
    assert lds_schedule(plan, FORM_UNIT) == (nh.NRF_OK, (0, 0))
