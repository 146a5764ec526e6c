"""Probe models on the CPU (no GPU): (1) the oracle alone satisfies what test_probe_gpu.py asserts of the kernels -- for every
leg's models and poses a frame equals the fp16 values of the routed features at each ray's first march sample, alpha is 1 on
hit rays and 0 elsewhere -- together with the conditions that keep those comparisons from passing vacuously; (2) the oracle's
hash-grid encoding against a plain float64 reference written from the encoding's published description."""
import ctypes as C

import numpy as np
import pytest

import models
import nerfhip as nh
import oracle_py as op
import probe_model as pm
import synthetic as syn

W, H = pm.FRAME_W, pm.FRAME_H


def plan(desc, allow_own, budget_mb):
    lib = nh.load_library()
    lib.nrf_debug_plan.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.nrf_debug_plan.restype = C.c_int
    out = (C.c_uint32 * 6)()
    assert lib.nrf_debug_plan(C.byref(desc), allow_own, budget_mb, out) == nh.NRF_OK
    return tuple(out)


_PROVED = {}


def _prove_frames(leg):
    """The frame properties and the value conditions of one leg's models, poses and options on the oracle."""
    key = (tuple(sorted(leg["build_kw"].items())), repr(leg["routes"]), leg["density_grid"], leg["option"], leg["n_poses"])
    if key in _PROVED:
        return _PROVED[key]
    opts = pm.leg_options(leg)
    cam = syn.default_camera(W, H)
    for desc, keep, info in pm.leg_models(leg):
        o = op.Oracle(desc)
        pooled = []
        for pose in pm.poses(leg["n_poses"]):
            hit, want = pm.expected_rgb(o, cam, pose, W, H, info, opts)  # (asserts oracle.network == expectation on the first samples)
            # at least 40 % of a frame's rays hit, and at least 500
            assert hit.sum() >= max(500, 0.4 * W * H), (leg["id"], int(hit.sum()))
            rgba, depth, st, counts, _ = o.render_rays(cam, pose, W, H, opts, schedule=op.SCHED_PER_RAY)
            assert np.array_equal(rgba[..., :3][hit], want[hit]), leg["id"]       # frame == expectation, exactly, on every hit ray
            assert np.all(rgba[..., 3][hit] == 1.0) and np.all(rgba[..., 3][~hit] == 0.0)
            assert np.all(rgba[..., :3][~hit] == opts.bg_color)
            assert counts[hit].max() <= 2 and np.all(counts[~hit] <= 1)  # a hit ray ends at its first sample
            # the saturation argument holds for the frame's steps: sigma dt > 17.4, exp(-x) < 2^-25, alpha == 1.0f with any exp
            h, xyz, dirs, deltas = pm.first_samples(o, cam, pose, W, H, opts)
            sigma, _ = o.network(xyz, dirs)
            assert float(sigma[h].min()) * float(deltas[h, 0].min()) > 17.4
            pooled.append(want[hit])
        pooled = np.concatenate(pooled)
        for c, route in enumerate(info["routes"]):
            u = np.unique(pooled[:, c])
            if info["sh"] and route[:2] == ("dir", 0):
                # the degree-0 coefficient is a constant by definition: the channel shows that constant (or its ReLU'd negative)
                const = np.float32(route[2]) * np.float32(pm.SH_C0)
                assert np.array_equal(u, [max(const, np.float32(0.0)) if info["act"] == "ReLU" else const])
                continue
            # a channel (one route, over the leg's poses): at least 300 distinct expected values, at least 10 % of them non-zero
            assert len(u) >= 300 and (u != 0).mean() >= 0.10, (leg["id"], route, len(u), float((u != 0).mean()))
    _PROVED[key] = True
    return True


@pytest.mark.parametrize("leg", pm.LEGS, ids=[leg["id"] for leg in pm.LEGS])
def test_probe_leg_holds_on_the_oracle_and_is_not_vacuous(leg):
    routes = [r for model in leg["routes"] for r in model]
    F, L = leg["build_kw"].get("n_features_per_level", 2), leg["build_kw"].get("n_levels", 16)
    dir_raw = syn.network_shape(syn.base_config(**{k: v for k, v in pm.resolve(leg["build_kw"]).items() if k not in ("H", "bound", "cascade")}))[5]
    # over a leg's routes every grid level appears (the levels 8..11 of the far copies among them), at least two direction
    # values, the last raw one among them; over a full leg every feature and every direction value in both signs
    assert {k // F for kind, k, _ in routes if kind == "grid"} == set(range(L))
    shown_dirs = {k for kind, k, _ in routes if kind == "dir"}
    assert len(shown_dirs) >= 2 and dir_raw - 1 in shown_dirs
    if leg["own"] in (pm.WIDE, pm.WIDE_SH):
        assert dir_raw - 1 >= 16
    if leg["full"]:
        assert set(routes) == {(kind, k, s) for kind, n in (("grid", L * F), ("dir", dir_raw)) for k in range(n) for s in (1, -1)}
    # the plan (GPU-free): the instance meant, and the gather form meant at the leg's budget
    desc, keep, info = next(pm.leg_models(leg))
    budget = int(leg["env"].get("NRF_QUAD_BUDGET_MB", leg["budget_mb"] or 8192))
    own, stage, mask, far, _, _ = plan(desc, int(leg["env"].get("NRF_WIDTH_INSTANCES", "1")), budget)
    assert (own, stage) == (leg["own"], leg["stage"]), (leg["id"], own, stage)
    addresses = sum(2 if (mask >> level) & 1 else (1 if info_nearest(leg) else 8) for level in range(L))
    if leg["addresses"] is not None:
        assert addresses == leg["addresses"] and (far != 0) == (leg["addresses"] == 56), (leg["id"], hex(mask), far)
    elif leg["budget_mb"]:
        assert mask != 0 and far == 0  # (the geometry legs: near copies of as many steps as 256 MB hold)
    else:
        assert mask == 0
    _prove_frames(leg)


def info_nearest(leg):
    return leg["build_kw"].get("interpolation") == "Nearest"


def test_legs_cover_the_axes():
    ids = [leg["id"] for leg in pm.LEGS]
    assert len(set(ids)) == len(ids)
    for name in pm.INSTANCES:
        for sched in ("persistent", "strip"):
            forms = ("none", "near") + (("far",) if name != "wide_freq12" else ()) if name in pm.QUAD_INSTANCES else (None,)
            for form in forms:
                assert f"{name}-{sched}" + (f"-{form}" if form else "") in ids
    assert sum(leg["density_grid"] == "random" for leg in pm.LEGS) * 2 >= len(pm.LEGS)
    assert {leg["own"] for leg in pm.LEGS} == set(range(13))  # every instance of the render kernel


# --------------------------------------------------------------------------- float64 reference of the hash-grid encoding
PRIMES = (1, 2654435761, 805459861)


def grid_index_f64ref(res, size, hashed, x, y, z):
    """index = x + y res + z res^2 where the level holds res^3 entries, else the xor-of-primes hash (Hash grids) or the same sum
    (Tiled grids), % size -- with the stride loop in uint32 as the published implementation has it: a term is added while
    the stride so far does not exceed the level's size, and res^3 may wrap (the LV_ADD_POW2 levels of large tables)."""
    x, y, z = (np.asarray(v, np.uint64) for v in (x, y, z))
    stride, index, M = 1, np.zeros(x.shape, np.uint64), np.uint64(0xFFFFFFFF)
    for coord in (x, y, z):
        if stride > size:
            break
        index = (index + coord * np.uint64(stride)) & M
        stride = (stride * res) & 0xFFFFFFFF
    if hashed and size < stride:
        index = (x * np.uint64(PRIMES[0]) & M) ^ (y * np.uint64(PRIMES[1]) & M) ^ (z * np.uint64(PRIMES[2]) & M)
    return (index % np.uint64(size)).astype(np.int64)


def encode_grid_f64(desc, params_table, p01, interpolation):
    """float64 features [n][L * F] and the per-value error bound of an fp16 evaluation (see test_oracle_grid_...)."""
    lt = nh.level_table(desc)
    L, F = int(desc.n_levels), int(desc.n_features_per_level)
    table = params_table.reshape(-1, F).astype(np.float16).astype(np.float64)  # the fp16-rounded table
    p = np.asarray(p01, np.float32).astype(np.float64)
    out = np.zeros((len(p), L * F))
    bound = np.zeros((len(p), L * F))
    alt = [np.zeros((len(p), L * F)) for _ in range(8)]  # Nearest only
    for l in range(L):
        res, size, scale = int(lt.resolution[l]), int(lt.offset[l + 1] - lt.offset[l]), float(lt.scale[l])
        base = int(lt.offset[l])
        pos = p * scale + 0.5
        cell = np.floor(pos)
        fr = pos - cell
        # the fp32 rounding of pos * scale + 0.5 (two roundings of a value below res + 1): a shift of the fraction by up to
        # 2 (res + 1) 2^-24 per axis, times the slope of the interpolant, at most the spread of the table (1) per axis
        slope = 1.0
        if interpolation == "Smoothstep":
            fr = fr * fr * (3.0 - 2.0 * fr)
            slope = 1.5  # max of d/dx smoothstep
        cell = cell.astype(np.int64)
        assert cell.min() >= 0
        if interpolation == "Nearest":
            # the entry at floor(pos): exact.  The two fp32 roundings of pos (at most 4 res 2^-24 in all) may move a position that
            # close to a cell boundary into the neighbouring cell: there the entry of either cell is right (`alt`, per axis)
            eps = 4 * res * 2.0 ** -24
            lo, hi = np.floor(pos - eps).astype(np.int64), np.floor(pos + eps).astype(np.int64)
            for pick in range(8):
                cand = [np.where((pick >> dim) & 1, hi[:, dim], lo[:, dim]) for dim in range(3)]
                e = grid_index_f64ref(res, size, desc.grid_type == nh.GRID_HASH, *cand)
                alt[pick][:, l * F:(l + 1) * F] = table[base + e]
            out[:, l * F:(l + 1) * F] = alt[0][:, l * F:(l + 1) * F]
            continue
        absum = np.zeros((len(p), F))
        for c in range(8):
            w = np.ones(len(p))
            corner = []
            for dim in range(3):  # trilinear weights in dimension order
                bit = (c >> dim) & 1
                w = w * (fr[:, dim] if bit else 1.0 - fr[:, dim])
                corner.append(cell[:, dim] + bit)
            e = grid_index_f64ref(res, size, desc.grid_type == nh.GRID_HASH, *corner)
            v = table[base + e]
            out[:, l * F:(l + 1) * F] += w[:, None] * v
            absum += w[:, None] * np.abs(v)
        bound[:, l * F:(l + 1) * F] = 8 * 2.0 ** -12 + 2.0 ** -11 * absum + slope * 4 * res * 2.0 ** -23 + \
            (3 * 6 * 2.0 ** -24 * absum if interpolation == "Smoothstep" else 0.0)
    return (out, bound) if interpolation != "Nearest" else (alt, None)


def special_positions(desc, rng, n_random):
    """Uniform positions, the corners and face centres of the unit cube, values next to 0 and 1, and per level cell
    boundaries from both sides."""
    lt = nh.level_table(desc)
    pos = [rng.random((n_random, 3), dtype=np.float32)]
    pos.append(np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32))
    pos.append(np.array([[0.5, 0.5, 0], [0.5, 0.5, 1], [0.5, 0, 0.5], [0.5, 1, 0.5], [0, 0.5, 0.5], [1, 0.5, 0.5],
                         [1 - 2 ** -24, 2 ** -24, 0.5], [2 ** -24, 0.5, 1 - 2 ** -24], [1, 0, 0.5], [0.25, 1, 1]], np.float32))
    for l in range(int(desc.n_levels)):
        res, scale = int(lt.resolution[l]), np.float32(lt.scale[l])
        for k in (0, 1, res // 2, res - 1):
            p = boundary_position(scale, k)
            if p is not None:
                q = np.nextafter(p, np.float32(0))
                pos.append(np.array([[p, 0.3, 0.7], [q, 0.3, 0.7], [0.6, p, q], [q, p, 0.1]], np.float32))
    return np.concatenate(pos)


def boundary_position(scale, k):
    """The smallest float32 p in [0, 1] with fp32(fp32(p * scale) + 0.5f) >= k + (k == 0) * 0.5, found by stepping nextafter:
    its grid position has cell k and fraction 0 (k >= 1), its predecessor's has cell k - 1 and the largest fraction."""
    if k == 0:
        return np.float32(0.0)
    p = np.float32((k - 0.5) / float(scale))

    def g(v):
        return np.float32(np.float32(v * scale) + np.float32(0.5))
    for _ in range(64):
        if g(p) >= k and g(np.nextafter(p, np.float32(0))) < k:
            return p if 0 <= p <= 1 else None
        p = np.nextafter(p, np.float32(0)) if g(p) >= k else np.nextafter(p, np.float32(2))
    return None


F64_SHAPES = {
    # name: (build_model keywords, interpolation)
    "T12_dense_and_hashed": (dict(log2_hashmap_size=12, H=32), "Linear"),
    "T19_base": (dict(log2_hashmap_size=19, H=32), "Linear"),
    "T22_add_pow2_levels": (dict(log2_hashmap_size=22, H=32), "Linear"),
    "tiled_add_pow2_levels": (dict(log2_hashmap_size=12, H=32, grid_type="Tiled"), "Linear"),
    "F1": (dict(log2_hashmap_size=12, H=32, n_features_per_level=1), "Linear"),
    "F4_8_levels": (dict(log2_hashmap_size=12, H=32, n_features_per_level=4, n_levels=8), "Linear"),
    "F8_4_levels": (dict(log2_hashmap_size=12, H=32, n_features_per_level=8, n_levels=4), "Linear"),
    "smoothstep": (dict(log2_hashmap_size=12, H=32, interpolation="Smoothstep"), "Smoothstep"),
    "smoothstep_F4": (dict(log2_hashmap_size=12, H=32, n_features_per_level=4, n_levels=6, interpolation="Smoothstep"), "Smoothstep"),
    "nearest": (dict(log2_hashmap_size=12, H=32, interpolation="Nearest"), "Nearest"),
    "nearest_F4": (dict(log2_hashmap_size=12, H=32, n_features_per_level=4, n_levels=8, interpolation="Nearest"), "Nearest"),
}


@pytest.mark.parametrize("name", sorted(F64_SHAPES))
def test_oracle_grid_encoding_against_a_float64_reference(name):
    """The oracle's encode_grid (the reference of every bit-exact grid test) against float64 numpy that uses only
    nh.level_table and the fp16-rounded table: trilinear weights in dimension order, the index rule above.

    Bound per value, Linear:  8 * 2^-12 + 2^-11 * sum_c w_c |v_c| + 4 * res * 2^-23
      (eight fp16 running sums of magnitude <= 0.5: half an ulp of 2^-11 each; eight products rounded to fp16: relative
      2^-11; the two fp32 roundings of pos * scale + 0.5, a value below res + 1, shift the fraction by <= 4 res 2^-24 in
      all, times the interpolant's slope, at most the table's spread of 1, over three axes: <= 4 res 2^-23 with room).
    Smoothstep: the same with the last term times 1.5 (the largest slope of x^2 (3 - 2 x)) plus 18 * 2^-24 sum_c w_c |v_c|
      (three fp32 operations of the smoothstep per axis and two products per weight: relative 2^-24 each, six per axis).
    Nearest: the entry at floor(pos), no arithmetic on values: == , where a position within 4 res 2^-24 (the same two fp32
      roundings) of a cell boundary may show the entry of the cell on either side.
    Measured worst ratio error / bound (20 000 uniform positions + corners, faces, cell boundaries from both sides):
      Linear 0.32 (T = 2^12), 0.30 (2^19), 0.29 (2^22), 0.31 (Tiled), 0.32 (F = 1), 0.32 (F = 4), 0.32 (F = 8), worst
      error 7.2e-4; Smoothstep 0.30 (F = 2), 0.30 (F = 4); Nearest: every value equal.
    A swapped corner bit, a wrong prime or a missing `% size` is an error of the order of the table's spread, ~0.25."""
    kw, interpolation = F64_SHAPES[name]
    desc, keep, cfg = models.build_model(**kw)
    o = op.Oracle(desc)
    n_mlp = keep[0].size - int(nh.level_table(desc).offset[desc.n_levels]) * int(desc.n_features_per_level)
    pos = special_positions(desc, np.random.default_rng(23), 20000)
    got = o.encode_grid(pos).view(np.float16).astype(np.float64)
    want, bound = encode_grid_f64(desc, keep[0][n_mlp:], pos, interpolation)
    raw = int(desc.n_levels) * int(desc.n_features_per_level)
    assert np.all(got[:, raw:] == 0)
    if interpolation == "Nearest":
        matches = np.stack([got[:, :raw] == w for w in want])
        assert np.all(matches.any(axis=0))
        assert matches.all(axis=0).mean() > 0.99  # (nearly every position has one candidate cell)
        return
    err = np.abs(got[:, :raw] - want)
    ratio = float((err / bound).max())
    print(f"{name}: worst error {float(err.max()):.3g}, worst error / bound {ratio:.3f}")
    assert np.all(err <= bound), (name, ratio)
    assert np.abs(want).max() > 0.3  # (the features are not all small: the bound is not trivially wide)
