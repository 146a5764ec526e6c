"""Dense probe models on the CPU (no GPU): for every leg, model and frame of tests/dense_model.py the oracle alone satisfies what
test_dense_gpu.py asserts of the kernels -- its network and its frame equal the float64 chain of tests/dense_reference.py bit for
bit on every certified sample -- together with the conditions that keep those comparisons from passing vacuously:

  * at least 25 % of a frame's pixels are hit pixels, at least 0.85 of them certified, no expectation non-finite, |value| < 2^14;
  * the oracle with an fp16 accumulator (set_mlp_accumulate 1 / 4 / 8 / 16) and every mutated chain -- hidden store skipped,
    hidden store rounded toward zero, fp16 accumulator per 16 products, one weight moved to a neighbouring column, the last
    padding column of the rgb input read as 0 -- differ on at least half of the certified hit pixels;
  * under ReLU every hidden neuron of every layer (but the sigma route's, a constant) is positive on some certified hit
    pixels and zero on others; every colour channel shows at least 300 distinct values;
  * 32 seeded single-weight moves per matrix (every shown weight where a matrix shows fewer) each change at least one certified hit pixel (of the first 1024).
Measured over all legs: certified share 0.966 .. 1.0 (degree-8 harmonics lowest), smallest detection 0.70 (oracle mode 16 and the
fp16 accumulator per 16 at 16 neurons: one block per hidden sum), 0.82 (store skipped), 0.95 (toward zero), 0.75 (moved weight),
0.54 (padding column); 2000+ distinct values per channel and frame.  `pytest -s` prints every frame's figures."""
import ctypes as C

import numpy as np
import pytest

import dense_model as dm
import dense_reference as dr
import nerfhip as nh
import oracle_py as op
import probe_model as pm
import synthetic as syn

CERTIFIED_FLOOR, DETECTION_FLOOR, HIT_FLOOR = 0.85, 0.5, 0.25
MOVES_PER_MATRIX, MOVE_PIXELS = 32, 1024


def plan(desc, allow_own, budget_mb):
    lib = nh.load_library()
    lib.nrf_debug_plan.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.nrf_debug_plan.restype = C.c_int
    out = (C.c_uint32 * 6)()
    assert lib.nrf_debug_plan(C.byref(desc), allow_own, budget_mb, out) == nh.NRF_OK
    return tuple(out)


def _differs(a, b):
    return float((a != b).any(axis=1).mean())


def shown_entries(info, which, index):
    """(row, col) of the dense weights of a matrix that a frame can show: not the sigma route's, and of the last rgb matrix the
    three colour rows."""
    mats = info[which]
    m = mats[index]
    rows, cols = np.nonzero(m)
    keep = np.abs(m[rows, cols]) == 1.0
    if which == "D":
        route_row = 0 if index == len(mats) - 1 else info["sigma_neurons"][index]
        keep &= rows != route_row
    elif index == len(mats) - 1:
        keep &= rows < 3
    return list(zip(rows[keep].tolist(), cols[keep].tolist()))


_PROVED = {}


def prove_frame(leg, seed, grid, p):
    """Everything the module docstring lists, for one frame; returns its figures."""
    key = dm.frame_key(leg, seed, grid, p)
    if key in _PROVED:
        return _PROVED[key]
    W, H = leg["size"]
    what = (leg["id"], seed, grid, p)
    cam, pose = syn.default_camera(W, H), dm.poses()[p]
    desc, keep, info = dm.dense_desc(leg["build_kw"], seed, grid, leg["s"])
    D, R, act = info["D"], info["R"], info["act"]
    o = op.Oracle(desc)
    e = dm.expected_frame(o, cam, pose, W, H, info)
    hit, cert = e["hit"].reshape(-1), e["certified"].reshape(-1)
    want = e["chain"]["rgb"]
    fig = dict(hit=float(hit.mean()), certified=float(cert.sum() / max(hit.sum(), 1)), largest=float(np.abs(want[cert]).max()))
    assert fig["hit"] >= HIT_FLOOR and fig["certified"] >= CERTIFIED_FLOOR, (what, fig)
    assert np.all(np.isfinite(want[cert])) and fig["largest"] < 2.0 ** 14, (what, fig)
    # the oracle (one fp32 summation order) == the float64 chain on every certified sample; its frame shows the same values
    sigma, rgb = o.network(e["xyz"], e["dirs"])
    assert np.array_equal(rgb[cert], want[cert]), what
    assert np.all(sigma[hit] > 5e4)
    rgba, depth, st, counts, _ = o.render_rays(cam, pose, W, H, None, schedule=op.SCHED_PER_RAY)
    rgba = rgba.reshape(-1, 4)
    assert np.array_equal(rgba[cert, :3], want[cert]) and np.all(rgba[hit, 3] == 1.0) and np.all(rgba[~hit, 3] == 0.0), what
    assert counts.reshape(-1)[hit].max() <= 2  # a hit ray ends at its first sample:
    _, _, _, deltas = pm.first_samples(o, cam, pose, W, H)
    assert float(sigma[hit].min()) * float(deltas[hit, 0].min()) > 17.4  # sigma dt > 17.4, exp(-x) < 2^-25, alpha == 1.0f with any exp
    # ---- what a wrong MLP would show
    feat, dirf, right = e["feat"][cert], e["dirf"][cert], want[cert]
    detect = {}
    for mode in (op.ACC_FP16_STEP, op.ACC_FP16_K4, op.ACC_FP16_K8, op.ACC_FP16_K16):
        detect[f"oracle_acc{mode}"] = _differs(op.Oracle(desc, accumulate=mode).network(e["xyz"][cert], e["dirs"][cert])[1], right)

    def mutated(D=D, R=R, feat=feat, dirf=dirf, **kw):
        return dr.chain(D, R, act, feat, dirf, certify=False, **kw)["rgb"]

    detect["hidden_store_skipped"] = _differs(mutated(store=dr.STORE_SKIP), right)
    detect["hidden_store_toward_zero"] = _differs(mutated(store=dr.STORE_RTZ), right)
    detect["fp16_accumulator_16"] = _differs(mutated(acc_block=16), right)
    # (of the first colour row's weights the one on the neuron that is positive most often: a move between two neurons that are
    # both zero at a pixel cannot show there; the seeded moves below take any weight and ask for one pixel)
    alive = (e["chain"]["hidden"][-1][cert] > 0).mean(axis=0)
    row, col = max((rc for rc in shown_entries(info, "R", len(R) - 1) if rc[0] == 0), key=lambda rc: alive[rc[1]])
    detect["weight_moved"] = _differs(mutated(R=dr.move_weight(R, len(R) - 1, row, col, dr.neighbour(R[-1], row, col))), right)
    if info["pad_cols"]:  # (no padding where the direction encoding fills its width: degree 4 and 8)
        stale = e["dirf"][cert].copy()
        assert np.all(stale[:, info["pad_cols"][-1] - 16] == 1.0)
        stale[:, info["pad_cols"][-1] - 16] = 0.0
        detect["last_padding_column_zero"] = _differs(mutated(dirf=stale), right)
    assert min(detect.values()) >= DETECTION_FLOOR, (what, detect)
    fig["detect"] = detect
    # ---- no dead and no always-on neuron, many values
    if act == "ReLU":
        for i, h in enumerate(e["chain"]["hidden"]):
            h = h[cert]
            both = (h > 0).any(axis=0) & (h == 0).any(axis=0)
            if i < e["chain"]["n_density_hidden"]:
                assert np.all(np.abs(h[:, info["sigma_neurons"][i]] - 1.0) <= 2.0 ** -9)  # (the interpolated constant wobbles by fp16 ulps)
                both[info["sigma_neurons"][i]] = True
            assert both.all(), (what, f"hidden layer {i}: neurons {np.flatnonzero(~both).tolist()} are never zero or never positive")
    fig["distinct"] = [len(np.unique(right[:, c])) for c in range(3)]
    assert min(fig["distinct"]) >= 300, (what, fig)
    # ---- a weight moved elsewhere is seen
    rng = np.random.default_rng(seed + 17)
    sub = slice(0, MOVE_PIXELS)
    padding = dict(D=range(info["shape"][0], info["shape"][1]), R=info["pad_cols"])
    n_moves = 0
    for which, mats in (("D", D), ("R", R)):
        for index in range(len(mats)):
            entries = shown_entries(info, which, index)
            for j in rng.permutation(len(entries))[:MOVES_PER_MATRIX]:
                row, col = entries[int(j)]
                # (not from one padding column to another, which hold the same constant; g[0], 11 at every sample, stays no input)
                same = padding[which] if index == 0 and col in padding[which] else ()
                to = dr.neighbour(mats[index], row, col, avoid=set(same) | ({0} if (which, index) == ("R", 0) else set()))
                if to is None:
                    continue
                moved = dr.move_weight(mats, index, row, col, to)
                got = mutated(feat=feat[sub], dirf=dirf[sub], **{which: moved})
                assert (got != right[sub]).any(), (what, which, index, row, col, to)
                n_moves += 1
            assert len(entries) >= min(MOVES_PER_MATRIX, 3 * leg["s"])  # (the last rgb matrix of a 16-wide model shows 23 weights)
    assert n_moves >= (len(D) + len(R)) * min(MOVES_PER_MATRIX - 4, 3 * leg["s"])
    print(f"dense-cpu {leg['id']} seed {seed} grid {grid}: hit {fig['hit']:.2f} certified {fig['certified']:.3f} largest |v| {fig['largest']:.1f} "
          f"distinct {fig['distinct']} detection " + " ".join(f"{k} {v:.2f}" for k, v in detect.items()))
    if len(_PROVED) > 64:
        _PROVED.clear()
    _PROVED[key] = fig
    return fig


@pytest.mark.parametrize("leg", dm.DENSE_LEGS, ids=[leg["id"] for leg in dm.DENSE_LEGS])
def test_dense_leg_holds_on_the_oracle_and_is_not_vacuous(leg):
    # the plan (GPU-free): the instance meant
    desc, keep, info = dm.dense_desc(leg["build_kw"], leg["seeds"][0], None, leg["s"])
    budget = int(leg["env"].get("NRF_QUAD_BUDGET_MB", leg["budget_mb"] or 8192))
    own, stage, _, _, _, _ = plan(desc, int(leg["env"].get("NRF_WIDTH_INSTANCES", "1")), budget)
    assert (own, stage) == (leg["own"], leg["stage"]), (leg["id"], own, stage)
    # the construction: every row s weights or more, every column one or more, the sigma route alone in its rows and columns
    for which in ("D", "R"):
        mats = info[which]
        for index, m in enumerate(mats):
            entries = shown_entries(info, which, index)
            rows = {r for r, _ in entries}
            assert all(sum(1 for r, _ in entries if r == row) >= min(leg["s"], m.shape[1] - 1) for row in rows)
            silent = set(range(m.shape[1])) - {c for _, c in entries}
            if which == "D":
                silent -= {info["sigma_feature"] if index == 0 else info["sigma_neurons"][index - 1]}
            elif index == 0:
                silent -= {0} | (set(range(16, 16 + info["shape"][5])) if info["frequency"] else set())
            assert not silent, (leg["id"], which, index, sorted(silent))
    if info["frequency"]:
        assert not info["R"][0][:, 16:16 + info["shape"][5]].any() and np.abs(info["R"][0][:, info["pad_cols"]]).sum(axis=0).min() >= 1
    for seed, grid, p in dm.leg_frames(leg):
        fig = prove_frame(leg, seed, grid, p)
        assert fig["certified"] >= dm.CERTIFIED_SHARE[leg.get("share", leg["instance"])]  # (the share the leg's comment states)


def test_legs_cover_every_instance_under_both_schedulers():
    ids = [leg["id"] for leg in dm.DENSE_LEGS]
    assert len(set(ids)) == len(ids)
    for name in pm.INSTANCES:
        for sched in ("persistent", "strip"):
            assert f"dense-{name}-{sched}" in ids
    assert {leg["own"] for leg in dm.DENSE_LEGS} == set(range(13))  # every instance of the render kernel
    assert {leg["option"] for leg in dm.DENSE_LEGS} == {None, "views3", "shard1of3", "large"}


def test_certificate_and_roundings_of_the_reference():
    """The helpers themselves: the quantum of fp16 values, a truncating store, and a sum the certificate must refuse."""
    x = np.array([0.0, 1.0, 0.75, 2.0 ** -24, 3 * 2.0 ** -14, 1000.0, 0.3330078125])
    assert np.array_equal(dr.quantum(x), [np.inf, 1.0, 0.25, 2.0 ** -24, 2.0 ** -14, 8.0, 2.0 ** -10])
    v = np.array([1.0 + 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 0.3, 70000.0])
    assert np.array_equal(dr.f16(v)[:2], [1.0, -(1.0 + 2.0 ** -9)])  # ties to even
    assert np.array_equal(dr.f16_toward_zero(v), [1.0, -(1.0 + 2.0 ** -10), float(np.float16(0.3)) - 2.0 ** -12, 65504.0])
    rng = np.random.default_rng(3)
    r = np.concatenate([rng.normal(0, 1, 20000) * 2.0 ** rng.integers(-28, 18, 20000), [0.0, -0.0, 65519.9, 65520.0, -65520.0, 2.0 ** -25, 3 * 2.0 ** -25],
                        (rng.integers(-4096, 4096, 4000) + 0.5) * 2.0 ** rng.integers(-26, 4, 4000)])  # (the last: ties)
    with np.errstate(over="ignore"):
        assert np.array_equal(dr.f16(r), r.astype(np.float16).astype(np.float64))  # numpy's cast rounds a float64 once, to nearest even
    t = dr.f16_toward_zero(r)
    small = np.abs(r) < 65504.0
    assert np.all(np.abs(t) <= np.abs(r)) and np.all(np.abs(t - r)[small] < np.maximum(np.abs(r[small]) * 2.0 ** -10, 2.0 ** -24))
    assert np.array_equal(dr.f16(t), t) and np.all((t == dr.f16(r)) | (np.abs(dr.f16(r)) > np.abs(r)))
    w = np.array([[1.0, -1.0, 0.0], [1.0, 0.0, 1.0]])
    ok = dr.layer_certificate(w, np.array([[1.0, 2.0 ** -24, 2.0 ** -24], [1.0, 2.0 ** -23, 2.0 ** -24]]))
    # 1 + 2^-24 needs 25 bits (S = 1 + 2^-24 is not below 2^24 q = 1): refused; 1 - 2^-23 fits 24 bits (S < 2^24 2^-23 = 2)
    assert ok.tolist() == [[False, False], [True, False]]
    assert dr.layer_certificate(w, np.array([[0.5, 2.0 ** -24, 0.0], [0.75, 0.25, 0.5]])).tolist() == [[True, True], [True, True]]
