"""Fog probe models on the CPU (no GPU): the conditions test_fog_gpu.py rests on, for every leg of probe_model.FOG_LEGS.

  * the oracle's fp32 frame, alpha and depth lie within the derived per-ray bound (fog_reference.py) of the float64
    restatement on EVERY hit ray, pixels that miss are the background exactly, and the oracle's per-ray sample counts equal
    the restatement's except on rays with a transmittance inside the stop window;
  * no fp16 tie in sigma: exp(g0) of every distinct density output lies 2^-16 relative away from an fp16 rounding boundary,
    so v_exp_f32 and libm round to the same fp16 sigma (density_scale multiplies the rounded value in fp32, in kernel and
    oracle alike: it cannot move a tie);
  * no leg passes vacuously, and the bound is tight enough to see a compositor that is subtly wrong: a sample removed from
    the middle of a ray, a stop threshold of 1e-3, max_steps off by one.

Measured over all legs: oracle worst error / bound 0.09 .. 0.56 for rgba, 0.05 .. 0.56 for depth; a leg's median bound
4e-7 .. 3e-5, the largest bound 1.1e-4.  A sample removed from the middle of a ray moves, per family (strength / instance /
option / large), 92 / 88 / 83 / 73 % of the rays with >= 3 samples beyond 4 x their bound and 43 / 29 / 30 / 31 % of them beyond
the 2/255 of the frame tests: the rest is what the suite could not see before.  A stop threshold of 1e-3 moves 88 .. 100 % of
the rays the T test stops (26 .. 62 % of the hit rays of the legs with a weight >= 3: those are the legs that see it, the
thinner fogs stop no ray), max_steps off by one every ray that reaches the cap (61 .. 94 % of the hit rays of those legs).  (`pytest -s` prints every leg's figures.)"""
import numpy as np
import pytest

import fog_reference as fr
import oracle_py as op
import probe_model as pm
import synthetic as syn

_PROVED = {}


def _moved(s, st, ref, b, opts, **variant):
    """Per ray: max |change of rgba| / bound when the chain is restated with `variant`."""
    alt = fr.composite(s, opts, **variant)
    rgba, _ = fr.frame(s, alt, opts)
    d = np.abs(rgba - ref).max(axis=1)
    return d / np.where(b > 0, b, np.inf), d


def _prove(leg):
    key = pm.fog_key(leg)
    if key in _PROVED:
        return _PROVED[key]
    W, H = leg["size"]
    opts, cam = pm.fog_options(leg), syn.default_camera(W, H)
    bg = np.float32(opts.bg_color)
    pooled = dict(hit=0, mid=0, stopped=0, capped=0, three=0, drop4=0, drop255=0, thr=0, cap_moved=0)
    object_counts, worst, worst_d, bounds = [], 0.0, 0.0, []
    for (grid, _), (desc, keep, info, pose) in zip(leg["frames"], pm.fog_models(leg)):
        assert not (info["frequency"] and any(kind == "dir" for kind, _, _ in info["routes"]))  # (v_sin_f32 != sinf: grid routes only)
        o = op.Oracle(desc)
        s, st, rgba, depth, b, db, window = fr.restate(o, info, cam, pose, W, H, opts)
        got, gdepth, gst, counts, _ = o.render_rays(cam, pose, W, H, opts, schedule=op.SCHED_PER_RAY)
        count = st["count"].reshape(H, W)
        hit = count > 0
        # ---- the oracle inside the bound, on every hit ray; the others are the background exactly
        err, derr = np.abs(got - rgba).max(axis=2), np.abs(gdepth - depth)
        assert np.all(err[hit] <= b[hit]), (leg["id"], grid, float((err[hit] / b[hit]).max()))
        assert np.all(derr[hit] <= db[hit]), (leg["id"], grid, float((derr[hit] / db[hit]).max()))
        assert np.all(got[~hit][:, :3] == bg) and np.all(got[~hit][:, 3] == 0) and np.all(gdepth[~hit] == 0)
        differ = counts != count
        assert not np.any(differ & ~window), (leg["id"], grid, int((differ & ~window).sum()))
        assert np.abs(counts.astype(np.int64) - count)[window].max(initial=0) <= 1
        assert int(counts.sum()) == gst.n_composited
        worst, worst_d = max(worst, float((err[hit] / b[hit]).max())), max(worst_d, float((derr[hit] / db[hit]).max()))
        bounds.append(b[hit])
        # ---- no fp16 tie in sigma
        valid = np.arange(s.sigma.shape[1])[None, :] < s.n[:, None]
        g0 = np.unique(s.g0[valid])
        assert 1 <= len(g0) <= 16, (leg["id"], g0)
        e = np.exp(g0.astype(np.float64))
        h = e.astype(np.float16)
        assert np.all(np.isfinite(h.astype(np.float64)))
        lo, hi = np.nextafter(h, np.float16(0)).astype(np.float64), np.nextafter(h, np.float16(np.inf)).astype(np.float64)
        edges = np.stack([(lo + h.astype(np.float64)) / 2, (hi + h.astype(np.float64)) / 2])
        assert np.all(np.abs(edges / e - 1.0).min(axis=0) >= 2.0 ** -16), (leg["id"], g0, np.abs(edges / e - 1.0).min(axis=0))
        ds = np.float32(opts.density_scale)
        sig = h.astype(np.float32) if opts.density_scale == 1.0 else (ds * h.astype(np.float32)).astype(np.float32)
        assert set(np.unique(s.sigma[valid])) <= set(sig)  # the oracle's sigma is fp16(exp(g0)) (times density_scale in fp32)
        # ---- not vacuous
        assert hit.mean() >= 0.40, (leg["id"], grid, float(hit.mean()))
        if grid is None:
            object_counts.append(count[hit])
        final = st["ws"].reshape(H, W)[hit]
        pooled["hit"] += int(hit.sum())
        pooled["mid"] += int(((final > 0.05) & (final < 0.95)).sum())
        pooled["stopped"] += int(st["stopped"].sum())
        pooled["capped"] += int(st["capped"].sum())
        # ---- sensitivity: what the bound can see
        ref = rgba.reshape(-1, 4)
        bf = b.reshape(-1)
        three = st["count"] >= 3
        ratio, d = _moved(s, st, ref, bf, opts, drop=np.where(three, st["count"] // 2, -1))
        pooled["three"] += int(three.sum())
        pooled["drop4"] += int((ratio[three] > 4).sum())
        pooled["drop255"] += int((d[three] > 2.0 / 255.0).sum())
        ratio, _ = _moved(s, st, ref, bf, opts, stop=1e-3)
        pooled["thr"] += int((ratio[st["stopped"]] > 4).sum())
        if "max_steps" in leg["opts_kw"]:
            ratio, _ = _moved(s, st, ref, bf, opts, max_steps=opts.max_steps + 1)
            ratio2, _ = _moved(s, st, ref, bf, opts, max_steps=opts.max_steps - 1)
            pooled["cap_moved"] += int((np.minimum(ratio, ratio2)[st["capped"]] > 4).sum())
    n = pooled["hit"]
    allb = np.concatenate(bounds)
    print(f"{leg['id']}: hit rays {n}, oracle worst error / bound rgba {worst:.3f} depth {worst_d:.3f}, bound median {np.median(allb):.2e} "
          f"max {allb.max():.2e}; final alpha in (0.05, 0.95) {pooled['mid'] / n:.2f}, stopped on T {pooled['stopped'] / n:.2f}, "
          f"capped {pooled['capped'] / n:.2f}; a dropped sample moves {pooled['drop4'] / max(pooled['three'], 1):.2f} of {pooled['three']} rays "
          f"beyond 4 x bound, {pooled['drop255'] / max(pooled['three'], 1):.2f} beyond 2/255; threshold 1e-3 moves "
          f"{pooled['thr'] / n:.2f} of the hit rays ({pooled['thr'] / max(pooled['stopped'], 1):.2f} of the stopped ones)"
          + (f"; max_steps +-1 moves {pooled['cap_moved'] / n:.2f} ({pooled['cap_moved'] / max(pooled['capped'], 1):.2f} of the capped ones)"
             if "max_steps" in leg["opts_kw"] else ""))
    # the object-grid frames: a median of at least 20 composited samples (a max_steps leg cannot: its rays reach the cap instead, below)
    assert np.median(np.concatenate(object_counts)) >= min(20, opts.max_steps), leg["id"]
    assert pooled["mid"] >= 0.10 * n, (leg["id"], pooled["mid"] / n)
    if leg["weight"] >= pm.W3 and "max_steps" not in leg["opts_kw"]:
        assert pooled["stopped"] >= 0.10 * n, (leg["id"], pooled["stopped"] / n)
    # a sample removed from the middle of a ray: at least half of the rays with >= 3 samples move by more than 4 x their bound
    assert pooled["three"] >= 0.5 * n or "max_steps" in leg["opts_kw"]
    if pooled["three"]:
        assert pooled["drop4"] >= 0.5 * pooled["three"], (leg["id"], pooled["drop4"] / pooled["three"])
    # a stop threshold of 1e-3: seen on the rays the test stops (a leg without such rays cannot see it: weights below 3)
    if pooled["stopped"] >= 0.10 * n:
        assert pooled["thr"] >= 0.5 * pooled["stopped"], (leg["id"], pooled["thr"] / pooled["stopped"])
    if leg["weight"] >= pm.W3 and "max_steps" not in leg["opts_kw"]:
        assert pooled["thr"] >= 0.25 * n, (leg["id"], pooled["thr"] / n)  # (these legs see the threshold on a quarter of their rays)
    if "max_steps" in leg["opts_kw"]:
        assert pooled["capped"] >= 0.25 * n, (leg["id"], pooled["capped"] / n)  # rays reach the cap ...
        assert pooled["cap_moved"] >= 0.5 * pooled["capped"] and pooled["cap_moved"] >= 0.25 * n, leg["id"]  # ... and a cap off by one, either way, moves them
    if len(_PROVED) > 64:
        _PROVED.clear()
    _PROVED[key] = True
    return True


@pytest.mark.parametrize("leg", pm.FOG_LEGS, ids=[leg["id"] for leg in pm.FOG_LEGS])
def test_fog_leg_holds_on_the_oracle_and_is_not_vacuous(leg):
    _prove(leg)


def test_fog_legs_cover_the_axes():
    ids = [leg["id"] for leg in pm.FOG_LEGS]
    assert len(set(ids)) == len(ids)
    for name, (kw, own, stage, env) in pm.INSTANCES.items():
        for sched in ("persistent", "strip"):
            legs = [leg for leg in pm.FOG_LEGS if leg["family"] == "instance" and leg["instance"] == name and leg["sched"] == sched]
            assert legs and all(leg["own"] == own and leg["stage"] == stage for leg in legs), (name, sched)
            if name == "hot":
                assert {leg["gather"] for leg in legs} == {"none", "near", "far"}
    for sched in ("persistent", "strip"):  # every one of the 13 instances, in both kernel forms
        assert {leg["own"] for leg in pm.FOG_LEGS if leg["family"] == "instance" and leg["sched"] == sched} == set(range(13))
    assert {leg["weight"] for leg in pm.FOG_LEGS if leg["family"] == "strength"} == set(pm.FOG_WEIGHTS)
    for leg in pm.FOG_LEGS:
        assert {grid for grid, _ in leg["frames"]} == {None, "random"}
    opts = {k: set() for k in ("max_steps", "density_scale", "bg_color", "min_near", "dt_gamma", "perturb")}
    for leg in pm.FOG_LEGS:
        for k, v in leg["opts_kw"].items():
            opts[k].add(v)
    assert opts == dict(max_steps={1, 7, 8, 9, 37}, density_scale={0.37, 2.0}, bg_color={0.0, 0.25}, min_near={0.05},
                        dt_gamma={0.0, 1.0 / 32.0}, perturb={5})
    # both stages other than the hot one under each of the six stage options, the generic one in both kernel forms and through a
    # width instance, a grid instance and the catch-all
    stage_legs = [leg for leg in pm.FOG_LEGS if leg["family"] == "stageoption"]
    assert len(pm.FOG_STAGE_OPTIONS) == 6 and all(leg["instance"] != "hot" and leg["stage"] != pm.HOT for leg in stage_legs)
    for oname in pm.FOG_STAGE_OPTIONS:
        under = [leg for leg in stage_legs if leg["opts_kw"] == pm.FOG_OPTIONS[oname][0]]
        assert all(leg["weight"] == pm.FOG_OPTIONS[oname][1] for leg in under), oname
        assert {leg["stage"] for leg in under} == {pm.WIDE, pm.GENERIC}, oname
        assert {leg["own"] for leg in under} >= {pm.WIDE, pm.W32, pm.GRID4, pm.GENERIC}, oname
        assert {leg["sched"] for leg in under if leg["stage"] == pm.GENERIC} == {"persistent", "strip"}, oname
    assert {"fog-option-geometry-bound4_cascade3", "fog-option-geometry-ngp_aabb32", "fog-output-views3", "fog-output-shard1of3",
            "fog-output-u8", "fog-output-rays-persistent", "fog-output-rays-strip", "fog-large-persistent", "fog-large-strip"} <= set(ids)
    switches = [leg["env"] for leg in pm.FOG_LEGS if leg["family"] == "switch"]
    for sched in (pm.PERSISTENT, pm.STRIP):
        for cap in "012":
            assert dict(sched, NRF_SAMPLE_CAP=cap) in switches
        assert dict(sched, NRF_MARCH_FF="0") in switches and dict(sched, NRF_MARCH_BUDGET="3") in switches
    assert dict(pm.PERSISTENT, NRF_TAIL_SPLIT="0") in switches
    # the legs that must equal a plain frame bit for bit render the models of the plain hot legs
    plain = {leg["sched"]: leg for leg in pm.FOG_LEGS if leg["id"] in ("fog-instance-hot-persistent-near", "fog-instance-hot-strip-near")}
    for leg in pm.FOG_LEGS:
        if leg["same_as_plain"]:
            assert pm.fog_key(leg) == pm.fog_key(plain[leg["sched"]]) and leg["plain_env"] == plain[leg["sched"]]["env"]


def test_existing_probe_legs_are_untouched():
    """sigma_weight defaults to 11: a probe leg's parameters are what they were."""
    leg = pm.LEGS[0]
    desc, keep, info = next(pm.leg_models(leg))
    desc11, keep11, _ = pm.probe_desc(leg["build_kw"], leg["routes"][0], leg["density_grid"], seed=1000, sigma_weight=11.0)
    assert info["sigma_weight"] == 11.0 and np.array_equal(keep[0], keep11[0]) and np.array_equal(keep[1], keep11[1])


def test_oracle_composite_chained_calls_against_the_float64_chain():
    """The oracle's composite stage, three calls that carry state and rays_t: the CPU half of test_fog_gpu.py's chained test."""
    fr.check_chained_composite("oracle", op.composite)
