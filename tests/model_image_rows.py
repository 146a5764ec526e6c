"""The rows of tests/test_model_image_cpu.py and test_model_image_gpu.py: a model shape (log2 T = 12, H = 32, weights from
build_model's seeded generator), a quad-copy budget and the flags of nrf_debug_model_image.

tests/golden/model_image_parent.json holds, per row, the byte length and crc32 of each part as the commit BEFORE csrc/nrf_model_plan.h
existed had it on an MI355X: a scratch program (not committed) compiled that commit's nrf_api.hip as its translation unit, loaded
each row's model with that commit's nrf_load_model and copied d_wfrag, d_wfrag_gen, d_wfrag_hot, d_gen, d_lv and the first
table_ref_bytes of d_grid back with hipMemcpy, with lengths from that commit's own constants (N_FRAGS_WIDE_ALL, MlpShape<W>::N,
DEPTH_FRAGS, N_FRAGS, DevModel::gen_frag_bytes, generic_frag_bytes); the plan's words are fields of its DevModel.  Nothing the new
header computes was written into the file.  The budgets were given to that commit as nrf_model_desc.gather_copy_budget_mb, "nosteps"
as NRF_QUAD_LEVELS=0.  A device that has no room for the copies cannot be arranged, so a "drop" row is recorded at
NRF_QUAD_BUDGET_MB=0: that commit's fallback zeroed the q_* fields, quad_mask and quad_far and chose the gather plan again, which is
what a budget that grants nothing leaves -- all parts are equal but one word, DevModel::grid_bytes: without copies the plan rounds the
table up to the 16 bytes a quad copy would start at, the fallback allocated table_ref_bytes (test_model_image_cpu.py states it)."""
import ctypes as C
import json
import zlib
from pathlib import Path

import numpy as np

import models
import nerfhip as nh

GOLDEN = Path(__file__).resolve().parent / "golden" / "model_image_parent.json"
PARTS = ("frags", "frags_gen", "frags_hot", "gen", "grid16", "levels", "plan")  # `which` of nrf_debug_model_image / nrf_debug_model_readout
PLAN_WORDS = ("own", "stage", "quad_mask", "quad_far", "uni_modes", "gather_plan", "grid_bytes", "gen_wave_bytes", "gen_frag_bytes", "depth_xd",
              "depth_xr", "dir_w")
DROP_QUADS, NO_STEPS, NO_FAST_GRID = 1, 2, 4  # flags of nrf_debug_model_image
QUAD_BUDGET_MB_DEFAULT = 8192  # (csrc/nrf_api.hip)

SHAPES = {  # one per code path of build_model_image (the names of tests/test_instance_plan_cpu.py SHAPES)
    "base": dict(),                                                                          # hot
    "freq12": dict(dir_otype="Frequency", n_frequencies=12),                                 # wide; stage = WIDE: frags_gen exists
    "sh8": dict(sh_degree=8),                                                                # WIDE_SH: frags_hot in the wide layout behind a generic stage
    "w16": dict(n_neurons=16), "w32": dict(n_neurons=32), "w128": dict(n_neurons=128),       # width
    "d1_1": dict(density_hidden_layers=1, rgb_hidden_layers=1),                              # depth
    "d3_4": dict(density_hidden_layers=3, rgb_hidden_layers=4),                              # ... with all five extra layers
    "act_squareplus": dict(activation="Squareplus"),                                         # ACT
    "g1_3": dict(n_features_per_level=1, n_levels=3),                                        # grid, F = 1: the zero upper columns
    "g2_5": dict(n_levels=5), "g4_8": dict(n_features_per_level=4, n_levels=8), "g8_2": dict(n_features_per_level=8, n_levels=2),
    "w32_h2_h3": dict(n_neurons=32, density_hidden_layers=2, rgb_hidden_layers=3),           # generic
    "act_sine": dict(activation="Sine"),                                                     # ... an activation no register-resident instance has
    "smoothstep_F4": dict(interpolation="Smoothstep", n_features_per_level=4, n_levels=6),   # fast_grid 4
    "nearest": dict(interpolation="Nearest"),                                                # fast_grid 0
    "tiled": dict(grid_type="Tiled"),                                                        # base with LV_ADD_POW2 levels (4096 entries, no hash)
}
BUDGET_SHAPES = ("base", "d3_4", "w16")  # ... at every budget


def _row(shape, budget="default", flags=0):
    return dict(shape=shape, budget=budget, flags=flags)


ROWS = {}
for _s in SHAPES:
    ROWS[_s] = _row(_s)
    ROWS[_s + "-step0"] = _row(_s, "step0")
for _s in BUDGET_SHAPES:
    ROWS[_s + "-nosteps"] = _row(_s, flags=NO_STEPS)
    ROWS[_s + "-drop"] = _row(_s, flags=DROP_QUADS)
# the far quad copies of a default-budget row take several GiB of device memory: one such row, the rest at the step-0 budget
GPU_ROWS = ("base",) + tuple(s + "-step0" for s in SHAPES)


def quad_step_bytes(desc, jl):
    """bytes of the cell-major quad copies of step jl (levels 4 jl .. 4 jl + 3): res^2 (res + 1) cells of 16 bytes per level"""
    lt = nh.level_table(desc)
    return sum(16 * int(lt.resolution[l]) ** 2 * (int(lt.resolution[l]) + 1) for l in range(4 * jl, 4 * jl + 4))


def step0_budget_mb(desc):
    """the smallest budget (MiB) that grants step 0, and no other step; 1 for a grid of fewer than 16 levels, which gets no copies at all"""
    if desc.n_levels < 16:
        return 1
    need = quad_step_bytes(desc, 0)
    mb = -(-need // (1 << 20))
    assert (mb << 20) >= need > ((mb - 1) << 20) and quad_step_bytes(desc, 1) > (mb << 20) - need
    return mb


def build(row):
    """(desc, keepalive, budget_mb): the row's descriptor and its budget in MiB, which the descriptor carries as gather_copy_budget_mb"""
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **SHAPES[row["shape"]])
    budget = QUAD_BUDGET_MB_DEFAULT if row["budget"] == "default" else step0_budget_mb(desc)
    desc.gather_copy_budget_mb = budget
    return desc, keep, budget


assert step0_budget_mb(build(ROWS["base"])[0]) == 2  # levels 0..3 (res 16, 23, 31, 43): 2.0 MB; levels 4..7 take 93 MB


def _read(call):
    n = C.c_uint64(0)
    rc = call(None, 0, C.byref(n))
    assert rc == nh.NRF_OK, (rc, nh.load_library().nrf_last_error())
    buf = np.zeros(max(n.value, 1), np.uint8)
    rc = call(buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
    assert rc == nh.NRF_OK and n.value <= buf.size, rc
    return buf[:n.value]


def image(desc, budget_mb, flags=0, allow_own=1, lib=None):
    """nrf_debug_model_image: {part: uint8 array}"""
    fn = (lib or nh.load_library()).nrf_debug_model_image
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    return {part: _read(lambda buf, cap, n: fn(C.byref(desc), allow_own, budget_mb, flags, which, buf, cap, n)) for which, part in enumerate(PARTS)}


def readout(ctx):
    """nrf_debug_model_readout of a loaded context: {part: uint8 array read back from the device}"""
    fn = ctx.lib.nrf_debug_model_readout
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    return {part: _read(lambda buf, cap, n: fn(ctx.h, which, buf, cap, n)) for which, part in enumerate(PARTS)}


def record(parts):
    """a golden entry"""
    return {"len": [int(parts[k].size) for k in PARTS], "crc32": [zlib.crc32(parts[k].tobytes()) for k in PARTS],
            "plan": [int(v) for v in parts["plan"].view(np.uint32)]}


def golden():
    return json.loads(GOLDEN.read_text())
