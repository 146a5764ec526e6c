"""The plan matrix on the CPU (no GPU): the legs of tests/probe_model.py (PLANS x PLAN_CELLS) and tests/dense_model.py that hold the
hot instance's static gather plans -- GATHER_DMHH, GATHER_QQHH, GATHER_QQFH, each compiled for three march forms and two output
modes, 18 instantiations of the persistent kernel -- to the exact references of test_probe_gpu.py, test_fog_gpu.py and
test_dense_gpu.py.

(1) Every leg reaches the instance it names, by what the library reports without a device: nrf_debug_gather_plan returns the
    leg's plan and step forms, nrf_debug_march_form (march_form of csrc/nrf_launch.h and whether the grid has the coarse level
    the march tables in LDS, and with them the persistent kernel, need) the leg's march form, nrf_debug_lds_schedule the compact
    level blocks and the prefetch depth of that instance (2; 1 in the MARCH_GENERIC ones), nrf_debug_plan own = stage = NET_HOT.
    Over the family the set of (plan, march form, output mode) is all 18.
    The cell `generic_h` (a grid side of 30) reaches none of them: a side that is no multiple of 4 has no coarse level, the
    march tables are not in LDS, the model renders in the per-strip kernel, which selects the forms at run time.  Its legs
    hold that kernel at this table size; the MARCH_GENERIC static-plan instances are `generic_b`'s.
(2) The legs that looked like static-plan coverage before are not: the T12 legs without copies and the loader-scaled geometry
    legs at 256 MB plan GATHER_RUNTIME.
(3) The new legs can fail: mistakes of the kind the static-plan code could make, restated on the oracle's encodings and fed to
    the probe and dense expectations, change at least half of the hit (probe) or certified (dense) pixels of a frame:
      a level of step 1 read with its neighbour's block; a hashed level masked with the dense mask 0xffffffff; a tile's last
      level (step 3) interpolated from the previous sample's values.
    A far level clamped at res instead of res - 1 CANNOT be seen, by any frame: the clamp is the identity for positions in
    [0, 1] at either value (floor(scale + 0.5) <= res - 1: level_gather_quad_far's comment).  The test asserts that per far
    level in the kernel's own fp32 arithmetic at p01 = 1, the largest position any sample can have (the cell is monotone in
    it), and on the first samples of the far legs' frames.  It guards the address of a load that has no range check, not a value.

Measured (64 x 48 frames): certified share of the dense legs 0.993 .. 0.997 (unit 0.996 / 0.994, pow2 0.997 / 0.993, generic_h
0.996 / 0.995, generic_b 0.997 / 0.995: inside pose / orbit pose); share of pixels a mutation changes, best frame of a leg:
probe -- neighbour's block 0.95 .. 0.99, dense mask (levels 7 and 8) 0.75 .. 0.82, previous sample 0.98 .. 0.99; dense -- 1.00 each.
`pytest -s` prints every leg's figures."""
import ctypes as C

import numpy as np
import pytest

import dense_model as dm
import dense_reference as dr
import models
import nerfhip as nh
import oracle_py as op
import probe_model as pm
import synthetic as syn
from test_gather_plan_cpu import GATHER_RUNTIME, gather_plan
from test_lds_schedule_cpu import lds_schedule
from test_probe_cpu import PRIMES, plan

W, H = pm.FRAME_W, pm.FRAME_H
OUT_F32, OUT_U8 = "float planes", "8-bit planes"


def march_form(desc):
    """(march form, 1 if the grid has the coarse level of the march tables in LDS) of the descriptor's grid, from the library"""
    lib = nh.load_library()
    lib.nrf_debug_march_form.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.POINTER(C.c_uint32)]
    lib.nrf_debug_march_form.restype = C.c_int
    out = (C.c_uint32 * 2)(7, 7)
    assert lib.nrf_debug_march_form(desc.density_grid_size, desc.cascade, desc.bound, out) == nh.NRF_OK
    return int(out[0]), int(out[1])


def family():
    """(kind, leg) of every plan-matrix leg of the three GPU files"""
    return ([("probe", leg) for leg in pm.LEGS if "plan" in leg] + [("fog", leg) for leg in pm.FOG_LEGS if "plan" in leg] +
            [("dense", leg) for leg in dm.DENSE_LEGS if "plan" in leg])


_MODELS = {}


def cell_model(build_kw):
    """models.build_model of a leg's shape (four shapes in all: kept)"""
    key = tuple(sorted(build_kw.items()))
    if key not in _MODELS:
        _MODELS[key] = models.build_model(**pm.resolve(build_kw))
    return _MODELS[key]


def budgets(leg):
    """(budget for nrf_debug_gather_plan, where 0 means the default: 1 MB grants this grid no copy either, which the caller
    checks; budget for nrf_debug_plan: what a context created with the leg's environment plans with)"""
    b = int(leg["env"].get("NRF_QUAD_BUDGET_MB", leg["budget_mb"] or 8192))
    return (b or 1), b


FAMILY = family()


@pytest.mark.parametrize("kind,leg", FAMILY, ids=[leg["id"] for _, leg in FAMILY])
def test_leg_reaches_the_instance_it_names(kind, leg):
    desc, keep, cfg = cell_model(leg["build_kw"])
    assert desc.log2_hashmap_size == 19 and desc.n_levels == 16 and desc.n_features_per_level == 2 and desc.base_resolution == 16
    assert abs(desc.per_level_scale - nh.default_per_level_scale(1.0, 16, 16)) < 1e-7
    gp_budget, plan_budget = budgets(leg)
    assert (nh.NRF_OK, leg["plan_id"], leg["forms"]) == gather_plan(desc, 1, gp_budget), leg["id"]
    assert (nh.NRF_OK, GATHER_RUNTIME, leg["forms"]) == gather_plan(desc, 1, gp_budget, env="0")  # (what NRF_GATHER_PLAN=0 compares with)
    own, stage, mask, far, _, _ = plan(desc, 1, plan_budget)
    assert (own, stage) == (pm.HOT, pm.HOT)
    if plan_budget == 0:
        assert plan(desc, 1, gp_budget)[2:4] == (0, 0) == (mask, far)  # (1 MB and no budget: the same plan)
    assert sum(2 if (mask >> level) & 1 else 8 for level in range(16)) == leg["addresses"] == {"dmhh": 128, "qqhh": 80, "qqfh": 56}[leg["plan"]]
    assert (far != 0) == (leg["plan"] == "qqfh")
    form, tables = march_form(desc)
    assert (form, bool(tables)) == (leg["march_form"], leg["lds_tables"]) == pm.PLAN_CELLS[leg["cell"]][1:], leg["id"]
    assert lds_schedule(leg["plan_id"], form) == (nh.NRF_OK, (1, 1 if form == pm.FORM_GENERIC else 2))
    assert leg["env"]["NRF_PERSISTENT"] == "1" and "NRF_GATHER_PLAN" not in leg["env"]
    if kind != "probe":
        assert leg["size"][0] <= W and leg["size"][1] <= H
        assert leg["sched"] == pm.plan_sched(leg["cell"]) == ("persistent" if tables else "strip")  # (what the GPU file expects to run)


def test_the_family_reaches_all_18_instances():
    """(plan, march form, output mode) over the legs the persistent kernel can run; the march form is the library's."""
    reached = {"probe": set(), "fog": set(), "dense": set()}
    for kind, leg in FAMILY:
        desc, _, _ = cell_model(leg["build_kw"])
        form, tables = march_form(desc)
        if not tables:
            assert leg["cell"] == "generic_h"
            continue  # the per-strip kernel: run-time selection
        _, plan_id, _ = gather_plan(desc, 1, budgets(leg)[0])
        reached[kind].add((plan_id, form, OUT_F32))
        if leg.get("option") == "u8planes":
            assert kind == "fog"
            reached[kind].add((plan_id, form, OUT_U8))
    plans = [pm.plan_id(forms) for _, forms in pm.PLANS.values()]
    forms = (pm.FORM_GENERIC, pm.FORM_UNIT, pm.FORM_POW2)
    every = {(p, f, o) for p in plans for f in forms for o in (OUT_F32, OUT_U8)}
    assert len(every) == 18 and reached["fog"] == every                       # compositing: fp64 bound; 8-bit: byte equality
    assert reached["dense"] == {c for c in every if c[2] == OUT_F32}           # encodings + MLPs: certified-exact
    dmhh = pm.plan_id(pm.PLANS["dmhh"][1])
    assert reached["probe"] == {(p, f, OUT_F32) for p in plans for f in forms if p == dmhh or f != pm.FORM_UNIT}  # encodings: bit-exact
    # the fog legs with a cap on the samples: the cells with several cascades, every plan, 7 and 9
    capped = {(leg["plan"], leg["cell"], leg["opts_kw"]["max_steps"]) for kind, leg in FAMILY if kind == "fog" and leg["opts_kw"]}
    assert capped == {(p, c, m) for p in pm.PLANS for c in ("pow2", "generic_b") for m in (7, 9)}


def test_the_legs_before_ran_the_run_time_selection():
    """What looked like static-plan coverage: the T12 legs without copies plan {mixed, hashed, hashed, hashed}, the geometry legs
    (per_level_scale from the loader: 1.5157 at bound 4) at their 256 MB {quad, hashed, hashed, hashed} -- GATHER_RUNTIME both."""
    for legs, ids in ((pm.LEGS, ("hot-geometry-bound4_cascade3", "hot-geometry-ngp_aabb32", "hot-persistent-none")),
                      (pm.FOG_LEGS, ("fog-option-geometry-bound4_cascade3", "fog-option-geometry-ngp_aabb32", "fog-instance-hot-persistent-none"))):
        for leg_id in ids:
            leg = next(leg for leg in legs if leg["id"] == leg_id)
            desc, _, _ = models.build_model(**pm.resolve(leg["build_kw"]))
            rc, plan_id, forms = gather_plan(desc, 1, budgets(leg)[0])
            assert rc == nh.NRF_OK and plan_id == GATHER_RUNTIME, (leg_id, forms)
            assert forms == ((pm.GFORM_MIXED,) if leg_id.endswith("none") else (pm.GFORM_QUAD,)) + (pm.GFORM_HASHED,) * 3, (leg_id, forms)
    dense = next(leg for leg in dm.DENSE_LEGS if leg["id"] == "dense-hot-persistent")  # T12 at 256 MB: QQHH, MARCH_UNIT -- one of 18
    desc, _, _ = models.build_model(**pm.resolve(dense["build_kw"]))
    assert gather_plan(desc, 1, 256)[1] == pm.plan_id(pm.PLANS["qqhh"][1]) and march_form(desc)[0] == pm.FORM_UNIT


# --------------------------------------------------------------------------- what a wrong gather would show
def _cells_f64(lt, level, p01):
    scale = float(lt.scale[level])
    pos = np.asarray(p01, np.float32).astype(np.float64) * scale + 0.5
    cell = np.floor(pos)
    return cell.astype(np.int64), pos - cell


def hashed_level_f64(desc, table, p01, level, dense_mask):
    """float64 trilinear feature pair of a power-of-two hashed level, and the error bound of an fp16 evaluation
    (test_probe_cpu.encode_grid_f64's).  dense_mask: level_offsets<2> (csrc/nrf_device.h) with the mask 0xffffffff in place of
    (size - 1) << 2.  The byte offset is then ((x << 2) | off_b) ^ (y P1 << 2) ^ (z P2 << 2) mod 2^32, entry (hash mod 2^30) ^
    (the level's start on the device, where a hashed level starts at a multiple of its size: below twice the table's entries,
    below 2^24), read through the buffer resource's range check.  So a corner whose hash mod 2^30 is 2^24 or more lies beyond
    the table and returns 0 -- 63 of 64 corners; the others read an entry this file cannot name and keep the right value here."""
    lt = nh.level_table(desc)
    base, size, res = int(lt.offset[level]), int(lt.offset[level + 1] - lt.offset[level]), int(lt.resolution[level])
    assert size & (size - 1) == 0 and res ** 3 > size and 2 * int(lt.offset[desc.n_levels]) <= 2 ** 24
    tab = table.reshape(-1, 2).astype(np.float16).astype(np.float64)
    cell, fr = _cells_f64(lt, level, p01)
    M = np.uint64(0xFFFFFFFF)
    out, absum = np.zeros((len(cell), 2)), np.zeros((len(cell), 2))
    for c in range(8):
        w = np.ones(len(cell))
        corner = []
        for dim in range(3):
            bit = (c >> dim) & 1
            w = w * (fr[:, dim] if bit else 1.0 - fr[:, dim])
            corner.append((cell[:, dim] + bit).astype(np.uint64))
        h = [(corner[d] * np.uint64(PRIMES[d])) & M for d in range(3)]
        e30 = (h[0] ^ h[1] ^ h[2]) & np.uint64(2 ** 30 - 1)
        v = tab[base + (e30 % np.uint64(size)).astype(np.int64)]
        if dense_mask:
            v = np.where((e30 >= np.uint64(2 ** 24))[:, None], 0.0, v)
        out += w[:, None] * v
        absum += w[:, None] * np.abs(v)
    return out, 8 * 2.0 ** -12 + 2.0 ** -11 * absum + 4 * res * 2.0 ** -23


def mutated_features(name, desc, keep, p01, feat, hit):
    """feat [n][32] (the oracle's fp16 features as float64) with what the mistake `name` would put there; rows of rays that miss
    are left alone.  Values the restatement cannot tell apart from the right ones (within twice the fp16 evaluation bound) stay
    the oracle's: only differences a kernel could not hide count."""
    out = feat.copy()
    if name == "neighbour_block":  # lane group g of step 1 reads the block of level 4 + (g ^ 1): that level's feature in this slot
        for level in range(4, 8):
            out[:, 2 * level:2 * level + 2] = feat[:, 2 * (level ^ 1):2 * (level ^ 1) + 2]
    elif name == "previous_sample":  # step 3 (levels 12..15) of a sample interpolated from the values of the one before it
        rows = np.flatnonzero(hit)
        out[rows, 24:32] = feat[np.roll(rows, 1), 24:32]
    elif name == "dense_mask":
        n_mlp = keep[0].size - int(nh.level_table(desc).offset[desc.n_levels]) * 2
        rows = np.flatnonzero(hit)
        for level in DENSE_MASK_LEVELS:
            right, bound = hashed_level_f64(desc, keep[0][n_mlp:], p01[rows], level, False)
            assert np.all(np.abs(feat[rows, 2 * level:2 * level + 2] - right) <= bound)  # (the restatement is the oracle's level)
            wrong, bound2 = hashed_level_f64(desc, keep[0][n_mlp:], p01[rows], level, True)
            seen = np.abs(wrong - right) > 2 * np.maximum(bound, bound2)
            out[rows[:, None], np.arange(2 * level, 2 * level + 2)[None, :]] = np.where(seen, dr.f16(wrong), feat[rows, 2 * level:2 * level + 2])
    elif name == "far_clamp_res":  # cell coordinates of the far levels 8..11 clamped at res instead of res - 1
        lt = nh.level_table(desc)
        for level in range(8, 12):
            cell, _ = _cells_f64(lt, level, p01[hit])
            res = int(lt.resolution[level])
            assert np.array_equal(np.minimum(cell, res), np.minimum(cell, res - 1)) and cell.max() <= res - 1 and cell.min() >= 0
    else:
        raise AssertionError(name)
    return out


MUTATIONS = ("neighbour_block", "dense_mask", "previous_sample")
# a hashed level of the mixed step 1 and one of step 2, which one probe model shows with opposite signs (a single channel is
# blind where ReLU cuts both the right and the wrong value; every hashed level behaves alike: two keep the test quick)
DENSE_MASK_LEVELS = (7, 8)


def _probe_share(leg, mutation):
    """The largest share of a frame's hit pixels that `mutation` changes, over the leg's models and poses."""
    cam, best = syn.default_camera(W, H), 0.0
    for desc, keep, info in pm.leg_models(leg):
        if mutation == "dense_mask" and not {k // 2 for kind, k, _ in info["routes"] if kind == "grid"} & set(DENSE_MASK_LEVELS):
            continue  # (a model that shows none of the mutated levels)
        o = op.Oracle(desc)
        for pose in pm.poses(leg["n_poses"]):
            hit, xyz, dirs, _ = pm.first_samples(o, cam, pose, W, H, pm.leg_options(leg))
            p01 = pm.pos01(xyz, info["bound"])
            feat = o.encode_grid(p01).view(np.float16).astype(np.float64)
            wrong = mutated_features(mutation, desc, keep, p01, feat, hit)
            want = pm.expected_values(o, xyz, dirs, info)
            got = pm.expected_values(o, xyz, dirs, info, feat=wrong.astype(np.float32))
            best = max(best, float((got != want).any(axis=1)[hit].mean()))
    return best


def _dense_share(leg, mutation):
    """The same over a dense leg's frames, of the certified hit pixels."""
    cam, best = syn.default_camera(*leg["size"]), 0.0
    for seed, grid, p in dm.leg_frames(leg):
        desc, keep, info = dm.dense_desc(leg["build_kw"], seed, grid, leg["s"])
        e = dm.expected_frame(op.Oracle(desc), cam, dm.poses()[p], *leg["size"], info)
        hit, cert = e["hit"].reshape(-1), e["certified"].reshape(-1)
        wrong = mutated_features(mutation, desc, keep, pm.pos01(e["xyz"], info["bound"]), e["feat"], hit)
        got = dr.chain(info["D"], info["R"], info["act"], wrong[cert], e["dirf"][cert], certify=False)["rgb"]
        best = max(best, float((got != e["chain"]["rgb"][cert]).any(axis=1).mean()))
    return best


@pytest.mark.parametrize("cell", list(pm.PLAN_CELLS))
@pytest.mark.parametrize("mutation", MUTATIONS)
def test_a_wrong_gather_changes_half_of_a_frame(mutation, cell):
    probe = next(leg for leg in pm.LEGS if leg["id"] == f"plan-dmhh-{cell}")
    dense = next(leg for leg in dm.DENSE_LEGS if leg["id"] == f"dense-plan-dmhh-{cell}")
    shares = _probe_share(probe, mutation), _dense_share(dense, mutation)
    print(f"plan-matrix {mutation} {cell}: changes {shares[0]:.2f} of a probe frame's hit pixels, {shares[1]:.2f} of a dense frame's certified ones")
    assert min(shares) >= 0.5, (mutation, cell, shares)


@pytest.mark.parametrize("cell", ["pow2", "generic_b"])
def test_the_far_clamp_is_the_identity(cell):
    """No cell coordinate of a far level reaches res: a clamp at res and one at res - 1 return the same quads, so no frame can
    tell them apart (module docstring).  Per level at p01 = 1 in fp32 as level_gather_quad_far computes it -- the cell is
    monotone in the position, and pos01 of a sample inside the aabb is at most 1 -- and on the first samples of the leg's frames
    (mutated_features asserts it there per level)."""
    probe = next(leg for leg in pm.LEGS if leg["id"] == f"plan-qqfh-{cell}")
    cam = syn.default_camera(W, H)
    desc, keep, info = next(pm.leg_models(probe))
    lt = nh.level_table(desc)
    for level in range(8, 12):
        top = np.float32(np.float32(np.float32(1.0) * np.float32(lt.scale[level])) + np.float32(0.5))
        assert int(top) <= int(lt.resolution[level]) - 1, (level, float(top), int(lt.resolution[level]))
    b = np.float32(info["bound"])
    assert np.all(pm.pos01(np.array([[b, -b, b]], np.float32), info["bound"]) <= 1.0)  # (the aabb's corner maps into [0, 1])
    o = op.Oracle(desc)
    for pose in pm.poses(2):
        hit, xyz, dirs, _ = pm.first_samples(o, cam, pose, W, H)
        p01 = pm.pos01(xyz, info["bound"])
        assert p01[hit].min() >= 0.0 and p01[hit].max() <= 1.0
        feat = o.encode_grid(p01).view(np.float16).astype(np.float64)
        assert np.array_equal(mutated_features("far_clamp_res", desc, keep, p01, feat, hit), feat)
