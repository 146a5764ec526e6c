"""The geometries the RAYS instances are tested at beyond H = 32 -- TEST INFRASTRUCTURE ONLY.

nrf_kernels_rays.hip instantiates 16 kernels: the persistent hot one for {UNIT, POW2, GENERIC} x {float, 8-bit planes}, and per
strip the hot and the wide stage for {UNIT, POW2, GENERIC with the march tables in LDS, GENERIC with the tables in global memory}
and the generic stage for {tables in LDS, tables in global memory}.  Which one renders a model follows from its grid alone:

    march form      march_form(H, cascade, bound) of csrc/nrf_launch.h: UNIT and POW2 need a power-of-two grid side and a power-of-two
                    bound >= 1; everything else is GENERIC
    coarse level    a grid side that is a multiple of 4 has the coarse occupancy level; without it the march tables stay in global
                    memory, and there is no persistent form

ROWS holds one model per combination the tests of H = 32 do not reach, with what nrf_debug_march_form and
nrf_debug_rays_instance must say of it and the figures of the ramp scene on the checker (tests/rays_clip_oracle.py, a 64 x 48
frame from orbit_pose(30, 30)): tests/test_render_rays_forms_cpu.py holds the table to the library and the figures to their
floors, tests/test_render_rays_forms_gpu.py renders the rows.

    hit          share of pixels with alpha > 0.5 in the unlimited frame
    partly       share with 0.05 < a < a_full - 0.05 under the ramp
    fully        share with a == 0 where a_full > 0.5
    untouched    share of hit pixels (a_full > 0) whose rgba bits equal the unlimited frame's
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import models
import nerfhip as nh
import oracle_py as op
import rays_clip_oracle as rco
import rays_oracle as ro
import synthetic as syn

GENERIC, UNIT, POW2 = 0, 1, 2  # march_form (csrc/nrf_launch.h)
HOT, GEN, WIDE = 0, 1, 2       # the stage code of nrf_debug_rays_instance; + 16: the persistent form
FREQ12 = dict(dir_otype="Frequency", n_frequencies=12)
SINE = dict(activation="Sine")

# name: (model kwargs, stage, (march form, coarse level), checker figures: hit, t_max partly / fully / untouched, t_min partly)
ROWS = {
    "h96":         (dict(H=96), HOT, (GENERIC, 1), (.436, .045, .254, .081, .048)),
    "h64-b1.5-c2": (dict(H=64, bound=1.5, cascade=2), HOT, (GENERIC, 1), (.467, .048, .273, .105, .046)),
    "h128-b0.75":  (dict(H=128, bound=0.75), HOT, (GENERIC, 1), (.417, .049, .246, .078, .051)),
    "h48-b3-c3":   (dict(H=48, bound=3.0, cascade=3), HOT, (GENERIC, 1), (.502, .064, .284, .103, .060)),
    "h30":         (dict(H=30), HOT, (GENERIC, 0), (.529, .064, .276, .107, .049)),
    "h30-b4-c3":   (dict(H=30, bound=4.0, cascade=3), HOT, (GENERIC, 0), (.527, .058, .274, .090, .052)),
    "wide-pow2":   (dict(H=32, bound=4.0, cascade=3, **FREQ12), WIDE, (POW2, 1), (.542, .060, .275, .130, .065)),
    "wide-h96":    (dict(H=96, **FREQ12), WIDE, (GENERIC, 1), (.436, .045, .254, .081, .048)),
    "wide-h30":    (dict(H=30, **FREQ12), WIDE, (GENERIC, 0), (.529, .064, .276, .107, .049)),
    "sine-h30":    (dict(H=30, **SINE), GEN, (GENERIC, 0), (.245, .123, .105, .043, .151)),
    "sine-h96":    (dict(H=96, **SINE), GEN, (GENERIC, 1), (.159, .069, .074, .049, .106)),
}
HOT_ROWS = [r for r, v in ROWS.items() if v[1] == HOT]
WIDE_ROWS = [r for r, v in ROWS.items() if v[1] == WIDE]
SINE_ROWS = [r for r, v in ROWS.items() if v[1] == GEN]
# the three fast-forward functions under the GENERIC form: one cascade at bound 1, several cascades, one cascade below bound 1
FF_ROWS = ["h96", "h64-b1.5-c2", "h128-b0.75", "h48-b3-c3"]
NO_COARSE_ROWS = ["h30", "h30-b4-c3"]

STRIP = {"NRF_PERSISTENT": "0"}
PERSISTENT = {"NRF_PERSISTENT": "1"}
SCHED = {"persistent": PERSISTENT, "strip": STRIP}
RW, RH = 64, 48  # the ramp scene's frame


def kwargs(row):
    return dict(ROWS[row][0])


@functools.lru_cache(maxsize=None)
def build(row):
    """models.build_model of a row at the 2^12 table, built once: (desc, keep, cfg)"""
    return models.build_model(log2_hashmap_size=12, **kwargs(row))


def coarse(row):
    return ROWS[row][2][1] == 1


def schedules(row):
    """The schedules that exist for a row: a hot row without the coarse level has no persistent form, the wide and generic
    stages render rays per strip whatever NRF_PERSISTENT says."""
    if ROWS[row][1] != HOT:
        return ["strip"]
    return ["persistent", "strip"] if coarse(row) else ["strip"]


def expected_instance(row, env):
    """nrf_debug_rays_instance of a context created for the row under the environment `env`"""
    stage = ROWS[row][1]
    if stage != HOT:
        return stage
    return 16 if coarse(row) and (env or {}).get("NRF_PERSISTENT") == "1" else 0


def hot_cases(rows=None):
    """(row, schedule) over the hot rows, every schedule that exists"""
    return [(r, s) for r in (rows or HOT_ROWS) for s in schedules(r)]


def march_form(H, cascade, bound):
    """nrf_debug_march_form: (march form, 1 if the grid has the coarse occupancy level)"""
    lib = nh.load_library()
    lib.nrf_debug_march_form.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.POINTER(C.c_uint32)]
    lib.nrf_debug_march_form.restype = C.c_int
    out = (C.c_uint32 * 2)(7, 7)
    assert lib.nrf_debug_march_form(H, cascade, bound, out) == nh.NRF_OK
    return int(out[0]), int(out[1])


_cache = {}


def scene(row):
    """The ramp scene of a row on the oracle, computed once and shared: desc, keep, the oracle, the orbit camera's rays, the
    unlimited frame (rgba, depth, samples) of tests/rays_oracle.py."""
    if ("scene", row) not in _cache:
        desc, keep, _ = build(row)
        orc = op.Oracle(desc)
        o, d, _, _ = orc.generate_rays(syn.default_camera(RW, RH), syn.orbit_pose(30, 30), RW, RH)
        full = ro.render(orc, desc, o, d)
        for a in (o, d, *full[:2]):
            a.setflags(write=False)
        _cache[("scene", row)] = (desc, keep, orc, o, d, full)
    return _cache[("scene", row)]


def checked(row, kind):
    """The checker's frame of the ramp as `kind` ("t_max" / "t_min"), computed once and shared (read-only): desc, rays, the
    unlimited frame, the limit, (rgba, depth, samples, raw depth), (near', far')."""
    desc, keep, orc, o, d, full = scene(row)
    if (row, kind) not in _cache:
        t = rco.ramp(RW, RH)
        res = rco.render(orc, desc, o, d, **{kind: t})
        nf = rco.near_far(desc, o, d, nh.default_options().min_near, **{kind: t})
        for a in (*res[:2], res[3], *nf, t):
            a.setflags(write=False)
        _cache[(row, kind)] = (t, res, nf)
    return (desc, o, d, full) + _cache[(row, kind)]


def ramp_figures(row):
    """hit, t_max partly / fully / untouched, t_min partly, and the sample counts (unlimited, t_max, t_min) of a row's scene"""
    full = scene(row)[5]
    a_full = full[0][:, 3]
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    rgba, _, n, _ = checked(row, "t_max")[5]
    a = rgba[:, 3]
    partly = float(np.mean((a > 0.05) & (a < a_full - 0.05)))
    fully = float(np.mean((a == 0) & (a_full > 0.5)))
    untouched = float(np.mean(np.all(bits(rgba) == bits(full[0]), axis=1) & (a_full > 0)))
    rgba2, _, n2, _ = checked(row, "t_min")[5]
    a2 = rgba2[:, 3]
    partly_min = float(np.mean((a2 > 0.05) & (a2 < a_full - 0.05)))
    return (float(np.mean(a_full > 0.5)), partly, fully, untouched, partly_min), (full[2], n, n2)
