"""Dense probe models: models whose rendered frame shows the output of BOTH MLPs exactly (helper of test_dense_cpu.py and
test_dense_gpu.py; no test in it).

A probe model (tests/probe_model.py) has one non-zero product per sum: it shows the encodings and is blind to the MLP.  A dense
probe model keeps the probe construction around the MLP -- the constant-1 grid feature routed alone with weight 11 to g[0],
so alpha == 1.0f at a ray's first sample; rgb output activation None; hidden activation ReLU or None -- and fills everything
else:

  * every row of every weight matrix holds `s` weights +1 / -1 (half of each sign) at seeded columns, and further ones so
    that every column holds at least one (in the last rgb matrix: at least one in the three colour rows, the only rows a
    frame shows); the exceptions are the rows and columns of the sigma route.  The density outputs g[1..15] are dense rows
    and feed the rgb MLP, so the fp16 handoff between the two networks is shown as well;
  * every table entry is a seeded fp16 value in [0.3, 0.9] (the sigma feature: 1.0), so interpolated features lie in about
    [0.25, 1) and are multiples of 2^-12.

With integer weights a dot product is a sum of input values, and tests/dense_reference.py certifies per sample that the sum is
exact in fp32 in ANY order; on certified samples the kernel, the oracle and the float64 chain agree bit for bit.  Samples are
uncertified where a direction value or a hidden activation close to zero has too fine a quantum.

LIMIT (Frequency models, `wide_freq12`): the 72 sine / cosine columns of the first rgb matrix hold zero weights -- v_sin_f32
against sinf is not exact (tests/test_probe_gpu.py states the reason) -- while its 8 trailing padding columns (exact 1.0) hold
weights.  A 64-wide direction block is covered exactly by `widesh_8`.

DENSE_LEGS lists what test_dense_gpu.py renders and test_dense_cpu.py proves the conditions for."""
from __future__ import annotations

import numpy as np

import dense_reference as dr
import nerfhip as nh
import probe_model as pm
import synthetic as syn

SIGMA_WEIGHT = 11.0
S = 6  # weights per row


def _fill(rng, m, s, rows, cols, extra_cols=(), shown_rows=None):
    """s weights per row of `rows` at columns drawn from `cols`, signs half and half; then one more for every column of `cols`
    and `extra_cols` that has none in `shown_rows` (default: `rows`): in the row of those that holds the fewest, with the sign
    that keeps the row's signs balanced (a ReLU neuron whose weights lean to one sign may never be zero, or never positive)."""
    k = min(s, len(cols))
    for r in rows:
        m[r, rng.choice(cols, k, replace=False)] = rng.permutation(np.resize([1.0, -1.0], k))
    shown_rows = list(rows if shown_rows is None else shown_rows)
    for c in list(cols) + list(extra_cols):
        if not m[shown_rows, c].any():
            counts = np.abs(m[shown_rows]).sum(axis=1)
            r = shown_rows[int(rng.choice(np.flatnonzero(counts == counts.min())))]
            lean = float(m[r].sum())
            m[r, c] = -np.sign(lean) if lean else float(rng.choice([1.0, -1.0]))


def dense_desc(build_kw, seed, density_grid=None, s=S):
    """density_grid: None (the synthetic object) or "random" (pm.random_density_grid).  Returns (desc, keep, info);
    info["D"], info["R"]: the matrices of the density and the rgb network, [out][in]."""
    desc, keep, cfg = pm._build(build_kw)
    feat_raw, feat_w, width, dens_hidden, rgb_hidden, dir_raw, dir_w = shape = syn.network_shape(cfg)
    act = cfg["network"]["activation"]
    assert act in ("ReLU", "None") and cfg["rgb_network"]["activation"] == act and cfg["rgb_network"]["output_activation"] == "None"
    nested = cfg["dir_encoding"]["nested"][0]["otype"]
    sh, frequency = nested == "SphericalHarmonics", nested == "Frequency"
    dir_pad = dir_w - dir_raw if sh else 0  # the padding ones of a SphericalHarmonics encoding come first, any other's last
    pad_cols = list(range(16, 16 + dir_pad)) if sh else list(range(16 + dir_raw, 16 + dir_w))  # of the rgb input: exact 1.0
    rng = np.random.default_rng(seed)
    sigma_feature = 0

    def matrices(n_in, hidden):
        dims = [n_in] + [width] * hidden + [16]
        return [np.zeros((dims[i + 1], dims[i]), np.float32) for i in range(len(dims) - 1)]

    D, R = matrices(feat_w, dens_hidden), matrices(16 + dir_w, rgb_hidden)
    # the sigma route: feature 0 -> a seeded neuron of every hidden layer -> g[0]; its rows and columns hold nothing else
    sigma_neurons = [int(rng.integers(width)) for _ in range(dens_hidden)]
    col = sigma_feature
    for i, m in enumerate(D):
        last = i == len(D) - 1
        row = 0 if last else sigma_neurons[i]
        rows = [r for r in range(m.shape[0]) if r != row]
        # (the zero padding columns of a grid encoding narrower than its padded width: a weight each, none of a row's s)
        real = [c for c in range(m.shape[1]) if c != col and (i > 0 or c < feat_raw)]
        _fill(rng, m, s, rows, real, extra_cols=range(feat_raw, feat_w) if i == 0 else ())
        m[row, col] = SIGMA_WEIGHT if last else 1.0
        col = row
    for i, m in enumerate(R):
        cols = list(range(m.shape[1]))
        if i == 0:  # g[0] = 11 is no input; the padding ones are constants: a weight each, none of a row's s
            cols = [c for c in cols if c != 0 and c not in pad_cols and not (frequency and 16 <= c < 16 + dir_raw)]
        _fill(rng, m, s, list(range(m.shape[0])), cols, extra_cols=pad_cols if i == 0 else (),
              shown_rows=[0, 1, 2] if i == len(R) - 1 else None)
    mlp = np.concatenate([m.reshape(-1) for m in D + R])
    params = keep[0].copy()
    assert nh.expected_n_params(desc) == params.size
    params[:mlp.size] = mlp
    lt = nh.level_table(desc)
    F = int(desc.n_features_per_level)
    table = params[mlp.size:].reshape(-1, F)
    assert table.shape[0] == int(lt.offset[desc.n_levels])
    table[:] = np.clip(rng.uniform(0.3, 0.9, table.shape).astype(np.float16), np.float16(0.3), np.float16(0.9)).astype(np.float32)
    level, f = divmod(sigma_feature, F)
    table[int(lt.offset[level]):int(lt.offset[level + 1]), f] = 1.0
    grid = keep[1]
    if density_grid == "random":
        grid = pm.random_density_grid(int(desc.density_grid_size), int(desc.cascade), 77)
        cfg = dict(cfg, snapshot=dict(cfg["snapshot"], mean_density=float(grid.mean())))
    else:
        assert density_grid is None
    desc2, keep2 = nh.desc_from_config(cfg, params, grid)
    info = dict(D=D, R=R, act=act, bound=float(desc2.bound), shape=shape, F=F, n_levels=int(desc2.n_levels), sh=sh, frequency=frequency,
                dir_pad=dir_pad, sigma_neurons=sigma_neurons, sigma_feature=sigma_feature, s=s, seed=seed,
                pad_cols=pad_cols)
    return desc2, keep2, info


def inputs(oracle, xyz, dirs, info):
    """The oracle's bit-exact encodings at world positions / directions: (feat [n][feat_w], dirf [n][dir_w]), fp16 values as float64."""
    feat = oracle.encode_grid(pm.pos01(xyz, info["bound"])).view(np.float16).astype(np.float64)
    dirf = oracle.encode_dir(pm.dir01(dirs)).view(np.float16).astype(np.float64)
    return feat, dirf


def expected_frame(oracle, cam, pose, W, H, info, opts=None):
    """dict(hit [H][W], certified [H][W] (hit and certified), want [H][W][3]: the float64 chain on the first samples (0 where a
    ray misses), feat, dirf, xyz, dirs of the first samples in pixel order, chain: dense_reference.chain's result)."""
    hit, xyz, dirs, _ = pm.first_samples(oracle, cam, pose, W, H, opts)
    feat, dirf = inputs(oracle, xyz, dirs, info)
    c = dr.chain(info["D"], info["R"], info["act"], feat, dirf)
    want = np.where(hit[:, None], c["rgb"], np.float32(0.0))
    return dict(hit=hit.reshape(H, W), certified=(hit & c["certified"]).reshape(H, W), want=want.reshape(H, W, 3), feat=feat, dirf=dirf,
                xyz=xyz, dirs=dirs, chain=c)


# --------------------------------------------------------------------------- legs
FRAMES = pm.FOG_FRAMES  # (density grid, index into poses()): the synthetic object from inside, the random grid from an orbit pose


def poses():
    """pm.poses(2)'s orbit pose, and a camera inside the volume that looks along a direction with no small component.  (pm's
    own inside camera looks nearly along an axis: there the spherical harmonics of degree 5 .. 8, products of powers of the
    two small components, are tiny at most pixels, their fp16 quanta too fine for the certificate -- 71 % of its pixels are
    certified at degree 8, 97 % from this one.)"""
    return [pm.poses(2)[0], syn.orbit_pose(60.0, 35.0, radius=0.4 / 0.33)]


# Two models per leg.  A seed is kept when the model satisfies every condition of test_dense_cpu.py in both frames (with some,
# one ReLU neuron of one layer is never zero, or never positive, within a frame); the others are the first that do from 4000 on.
SEEDS = (4000, 4001)
SEEDS_OF = {
    "widesh_5": (4000, 4015), "widesh_8": (4000, 4002), "w32": (4000, 4002), "w128": (4002, 4003), "depth_d2_2": (4000, 4002),
    "depth_d3_4": (4001, 4002), "generic_w32_width_instances_off": (4000, 4002),
}
LARGE = pm.FOG_LARGE

# The smallest share of certified hit pixels over an instance's frames (two models x two frames of 64 x 48, rounded down;
# test_dense_cpu.py asserts it, and 0.85 of every frame whatever stands here; `pytest -s` prints every frame's share).  The
# uncertified rest: a direction value or a hidden activation next to zero, whose fp16 quantum is too fine for S < 2^24 q.
CERTIFIED_SHARE = {
    "hot": 0.99, "wide_freq12": 1.0,  # (Frequency: no direction value enters a sum)
    "widesh_5": 0.98, "widesh_8": 0.96,  # (25 and 64 direction values)
    "w16": 0.99, "w32": 0.99, "w128": 0.99, "depth_d2_2": 0.99, "depth_d3_4": 0.99, "depth_d1_1": 0.99, "act_none": 0.99,
    "grid1_g1_16": 0.99, "grid2_g2_11": 0.99, "grid4_g4_8": 0.99, "grid8_g8_4": 0.99, "grid4_g4_6s": 0.99, "grid2_g2_16n": 0.99,
    "generic_w32_width_instances_off": 0.99, "generic_w32_h2": 0.99,
    # the plan matrix (base.json's 2^19 table, one model x two frames per march cell: test_plan_matrix_cpu.py)
    "plan-unit": 0.99, "plan-pow2": 0.99, "plan-generic_h": 0.99, "plan-generic_b": 0.99,
}
PLAN_SEED = 4000  # (the plan-matrix legs: one model per cell, kept by the rule above)


def _leg(name, sched, option=None, size=(pm.FRAME_W, pm.FRAME_H), n_seeds=2, frames=FRAMES):
    kw, own, stage, env = pm.INSTANCES[name]
    seeds = SEEDS_OF.get(name, SEEDS)[:n_seeds]
    gather = "near" if name in pm.QUAD_INSTANCES else "-"  # (the MLP does not depend on the gather form)
    genv, budget, _ = dict(pm.GATHER, **pm.NO_GATHER_AXIS)[gather]
    sched_env = pm.PERSISTENT if sched == "persistent" else pm.STRIP
    return dict(id=f"dense-{name}-{sched}" + (f"-{option}" if option else ""), instance=name, sched=sched, build_kw=dict(pm.T12, **kw),
                own=own, stage=stage, env=dict(env, **sched_env, **genv), budget_mb=budget, option=option, size=tuple(size),
                seeds=tuple(seeds), frames=tuple(frames), s=S)


def _plan_leg(plan, cell):
    """The hot instance under static plan `plan` in march cell `cell` (pm.PLANS, pm.PLAN_CELLS): encodings read in the plan's
    forms in front of both MLPs.  A cell's three plans render the same model."""
    gather = pm.PLANS[plan][0]
    genv, budget, addresses = pm.GATHER[gather]
    return dict(id=f"dense-plan-{plan}-{cell}", instance="hot", share="plan-" + cell, sched=pm.plan_sched(cell),
                build_kw=dict(pm.T19, **pm.PLAN_CELLS[cell][0]), own=pm.HOT, stage=pm.HOT, env=dict(pm.PERSISTENT, **genv),
                budget_mb=budget, addresses=addresses, option=None, size=(pm.FRAME_W, pm.FRAME_H), seeds=(PLAN_SEED,), frames=tuple(FRAMES),
                s=S, **pm.plan_fields(plan, cell))


def _legs():
    out = [_leg(name, sched) for name in pm.INSTANCES for sched in ("persistent", "strip")]
    out.append(_leg("w128", "persistent", option="views3"))
    out.append(_leg("depth_d3_4", "persistent", option="shard1of3"))
    for name in ("hot", "w32"):  # several strips per queue and a tail that is split: a 64 x 48 frame is all tail
        out.append(_leg(name, "persistent", option="large", size=LARGE, n_seeds=1, frames=FRAMES[1:]))
    out += [_plan_leg(plan, cell) for cell in pm.PLAN_CELLS for plan in pm.PLANS]  # (a cell's plans share their expectation)
    return out


DENSE_LEGS = _legs()


def frame_key(leg, seed, grid, pose_index):
    """What a frame's expectation depends on: legs that differ in scheduler or output path share it."""
    return (tuple(sorted(leg["build_kw"].items())), leg["s"], seed, grid, pose_index, leg["size"])


def leg_frames(leg):
    """(seed, density grid, pose index) of every frame of a leg."""
    return [(seed, grid, p) for seed in leg["seeds"] for grid, p in leg["frames"]]
