"""The CPU oracle against the reference's OWN kernels, bit for bit.

oracle/ref_kernels.cpp compiles the reference's render_utils.h (ray set-up, near / far, march, compaction, compositing, the
density-grid helpers) and the transfer functions of common_device.cuh for the CPU, unchanged, behind stand-in headers
(oracle/ref_shim/); tests/ref_kernels_py.py binds it.  Every comparison here is on uint32 views of the floats: both sides are CPU
code with the same libm and no contraction, so nothing takes a tolerance.  (`__expf` is libm's expf on both sides; what the device
intrinsic adds is the 2e-5 of tests/test_parity_gpu.py.)

Only what SURVEY.md Appendix D names may differ, and each such difference is asserted in its literal form:
  D-1  the reference leaves sample slots it does not write untouched: its buffers are pre-zeroed here (ref_kernels_py.march)
  D-3  a ray that misses the box has depth 0 / 0 in the reference and 0 in the oracle: masked by `near == FLT_MAX`, computed
       on the reference's own output, and the masked share can be no larger than the share of rays that miss
  D-8  matrix_multiply_1x1n takes the density scale as an int
  D-9  generate_density_grid is dead code with two bugs (test_density_grid_helpers names them)

Without a reference tree AND without the built library the module skips; with the tree and without the library it fails."""
import numpy as np
import pytest

import density_grid_replay as dgr
import models
import nerfhip as nh
import oracle_py as op
import ref_kernels_py as rk
import synthetic as syn

U32 = np.uint32
FLT_MAX = rk.FLT_MAX

# name: keywords of models.build_model(log2_hashmap_size=12, **kw): the two grids of test_march_bit_exact_and_composite and the
# rows of test_every_march_instance_matches_oracle whose side or bound is no power of two
GEOMETRIES = {
    "h32": dict(H=32, bound=1.0, cascade=1),
    "h32-b4-c3": dict(H=32, bound=4.0, cascade=3),
    "h30": dict(H=30, bound=1.0, cascade=1),
    "h64-b1.5-c2": dict(H=64, bound=1.5, cascade=2),
}
POSES = {"orbit-10-30": syn.orbit_pose(10, 30), "orbit-200--15": syn.orbit_pose(200, -15), "main": syn.REFERENCE_MAIN_POSE}


@pytest.fixture(scope="module", autouse=True)
def _library():
    rk.require()


_cache = {}


def golden_generator():
    if "gen" not in _cache:
        import importlib.util
        from pathlib import Path

        path = Path(__file__).resolve().parent / "golden" / "make_reference_golden.py"
        spec = importlib.util.spec_from_file_location("make_reference_golden", path)
        _cache["gen"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_cache["gen"])
    return _cache["gen"]


def model(name, grid="scene"):
    """(desc, Oracle, Geometry) of a geometry, built once.  grid = "speckle": the same model over a density grid in which every
    cell of EVERY cascade is occupied with probability 1/6 -- the synthetic scene occupies cascade 0 only, so with it a wrong
    cell lookup or hop in an outer cascade finds the same empty space and changes nothing (make_reference_golden.speckle_grid)."""
    key = (name, grid)
    if key not in _cache:
        desc, keep, cfg = models.build_model(log2_hashmap_size=12, **GEOMETRIES[name])
        if grid == "speckle":
            desc, keep = nh.desc_from_config(cfg, keep[0], golden_generator().speckle_grid(keep[1].size, 7))
        _cache[key] = (desc, op.Oracle(desc), rk.Geometry(desc), keep)
    return _cache[key][:3]


def cameras(W, H):
    fl = float(syn.default_camera(W, H)[0])
    return {"default": syn.default_camera(W, H),
            "skew": np.array([1.1 * fl, 0.9 * fl, 0.5 * W + 3.25, 0.5 * H - 2.5], np.float32)}  # fl_x != fl_y, off-centre


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shapes {got.shape} != {want.shape}"
    diff = got.view(U32) != want.view(U32)
    if diff.any():
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} values differ in their bits; first at {at}: "
                             f"oracle {got[at]!r} ({got.view(U32)[at]:#010x}) reference {want[at]!r} ({want.view(U32)[at]:#010x})")


def hit_share(nears, what):
    """Share of rays the REFERENCE says hit the box; every masked comparison is capped by the rest"""
    share = float((nears != FLT_MAX).mean())
    print(f"{what}: reference hit share {share:.3f}")
    assert share >= 0.5, f"{what}: the camera shows too little of the box ({share:.3f})"
    return share


# ---------------------------------------------------------------------------------------------------------------------- rays
def test_nerf_matrix_to_ngp():
    for pose in POSES.values():
        for scale in (0.33, 1.0, 0.8):
            got = np.empty(16, np.float32)
            p = np.ascontiguousarray(pose, np.float32).reshape(16)
            op.lib().nrfo_nerf_matrix_to_ngp(op._fp(p), scale, op._fp(got))
            same_bits(got.reshape(4, 4), rk.nerf_matrix_to_ngp(pose, scale), f"nerf_matrix_to_ngp scale {scale}")


@pytest.mark.parametrize("W,H", [(50, 37), (48, 40)])
def test_rays_and_near_far(W, H):
    """set_rays_o / set_rays_d (both devices' halves, interleaved) and kernel_near_far_from_aabb against Oracle.generate_rays"""
    desc, o, geo = model("h32")
    for cname, cam in cameras(W, H).items():
        for pname, pose in POSES.items():
            what = f"{W}x{H} {cname} {pname}"
            ro, rd, nr, fr = rk.frame_rays(cam, pose, geo, W, H, 0.2)
            hit_share(nr, what)
            wo, wd, wn, wf = o.generate_rays(cam, pose, W, H)
            same_bits(wo, ro, f"rays_o {what}")
            same_bits(wd, rd, f"rays_d {what}")
            same_bits(wn, nr, f"nears {what}")
            same_bits(wf, fr, f"fars {what}")


def crafted_rays():
    """Origins and directions that stress kernel_near_far_from_aabb: inside the box, exact misses, grazing, zero components of
    both signs (1 / d = +-inf; (aabb - o) * inf is +-inf or, on a face, 0 * inf = NaN)"""
    pz, nz = np.float32(0.0), np.float32(-0.0)
    s = np.float32(1 / np.sqrt(2))
    rows = [
        ((0, 0, 0), (0.3, 0.5, 0.81)), ((0.2, -0.9, 0.99), (-0.7, 0.1, 0.7)), ((0, 0, 0), (pz, pz, 1)), ((0, 0, 0), (nz, nz, -1)),
        ((0.1, -2.5, 0.3), (0.05, 0.99, -0.1)),                                 # the issue's worked ray
        ((2, 0, -3), (pz, pz, 1)), ((2, 0, -3), (nz, pz, 1)),                   # parallel to z, outside in x: exact misses
        ((0, 3, 0), (1, pz, pz)), ((0, -3, 0), (1, nz, nz)),
        ((1, 0, -3), (pz, pz, 1)), ((1, 0, -3), (nz, nz, 1)),                   # in the face x = 1: 0 * inf
        ((-1, -1, -3), (pz, pz, 1)), ((1, 1, 3), (nz, nz, -1)),                 # along an edge
        ((-3, 1, 0.5), (1, pz, pz)), ((-3, 1, 0.5), (1, nz, 0.0)),              # grazing the face y = 1
        ((-2, -2, 0), (s, s, pz)), ((-2, -2, 0), (s, s, nz)),                   # through two edges on the diagonal
        ((-2, -2, -2), (1, 1, 1)), ((-3, 0, 0), (1, 0.333333, 0)),              # corner to corner; leaves through an edge
        ((0, 0, -5), (0, 0, -1)), ((0, 0, 1.5), (0, 0, 1)),                     # the box lies behind the origin
        ((0, 0, -1.2), (0, 0, 1)), ((0, 0, -1.04), (0, 0, 1)),                  # entry just beyond / just inside min_near
        ((0, 0, 0), (pz, pz, pz)), ((2, 2, 2), (nz, nz, nz)),                   # no direction at all
    ]
    o = np.array([r[0] for r in rows], np.float32)
    d = np.array([r[1] for r in rows], np.float32)
    return o, d


@pytest.mark.parametrize("bound", [1.0, 1.5, 4.0])
@pytest.mark.parametrize("min_near", [0.05, 0.2, 5.0])
def test_near_far_crafted_rays(bound, min_near):
    """min_near below the entry, at about the entry (0.2: the rays that start 1.2 and 1.04 outside the face) and above it
    (5.0: beyond every exit, so near > far comes out, as the kernel leaves it)"""
    o, d = crafted_rays()
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    rn, rf = rk.near_far(np.ascontiguousarray(o.T), np.ascontiguousarray(d.T), aabb, min_near)
    on, of = op.near_far(aabb, o, d, min_near)
    same_bits(on, rn, "nears (crafted)")
    same_bits(of, rf, "fars (crafted)")
    if bound == 1.0 and min_near == 0.05:
        assert (rn == FLT_MAX).sum() >= 4 and (rn != FLT_MAX).sum() >= 8 and np.isnan(rn).sum() + np.isnan(rf).sum() >= 1
        # the ray (0.1, -2.5, 0.3) + t (0.05, 0.99, -0.1) enters at (-1 + 2.5) / 0.99 and leaves at (1 + 2.5) / 0.99
        assert abs(float(rn[4]) - 1.5 / 0.99) < 1e-6 and abs(float(rf[4]) - 3.5 / 0.99) < 1e-6


# --------------------------------------------------------------------------------------------------------------------- march
RADII = {"near": 4.0311, "far": 9.0}


def march_rays(name, W=48, H=40, view="near", grid="scene"):
    """The rays of a 48 x 40 frame.  "near" is the usual orbit (1.33 ngp units out: inside the unit cube's bounding sphere, so
    every position lies in cascade 0); "far" stands 2.97 units out, so that the march starts in cascade 2 of a bound-4 model,
    enters a bound-1.5 box through cascade 1, and hops through empty outer cells on its way in."""
    desc, o, geo = model(name, grid)
    cam, pose = syn.default_camera(W, H), syn.orbit_pose(45, 25, radius=RADII[view])
    return rk.frame_rays(cam, pose, geo, W, H, 0.2)


def levels_visited(geo, xyz):
    """mip_from_pos of written sample positions (render_utils.h:148-155)"""
    mx = np.abs(xyz).max(axis=-1)
    return np.clip(np.frexp(mx)[1], 0, geo.cascade - 1)


@pytest.mark.parametrize("view", list(RADII))
@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 128])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_march(name, dt_gamma, view):
    """kernel_march_rays against Oracle.march: positions, directions and both deltas planes, n_step 1, 3 and 8.  The reference's
    output buffers are zeroed first (D-1: it leaves slots it does not write untouched, the oracle zeroes them)."""
    desc, o, geo = model(name)
    ro, rd, nr, fr = march_rays(name, view=view)
    hit_share(nr, f"march {name} {view}")
    opts = nh.default_options()
    opts.dt_gamma = dt_gamma
    for n_step in (1, 3, 8):
        rx, rdr, rdl = rk.march_first_round(geo, ro, rd, nr, fr, n_step, dt_gamma)
        wx, wdr, wdl = o.march(ro, rd, nr, fr, n_step, opts)
        what = f"{name} {view} dt_gamma {dt_gamma} n_step {n_step}"
        assert (rdl[:, :, 0] > 0).sum() > len(nr) // 16, f"{what}: the march emitted almost nothing"
        same_bits(wx, rx, f"xyzs {what}")
        same_bits(wdr, rdr, f"dirs {what}")
        same_bits(wdl[:, :, 0], rdl[:, :, 0], f"deltas[0] {what}")
        same_bits(wdl[:, :, 1], rdl[:, :, 1], f"deltas[1] {what}")


@pytest.mark.parametrize("grid", ["scene", "speckle"])
@pytest.mark.parametrize("view", list(RADII))
@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 128])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_march_resumed_rounds(name, dt_gamma, view, grid):
    """The march resumed round after round, as the loop resumes it: from rays_t = t + the sum of deltas[1] (what
    kernel_composite_rays hands on, render_utils.h:716,742), rays that filled all 8 slots only.  The first round mostly
    crosses empty space once and then sits inside the object; the later rounds leave it, hop the gaps between its parts and
    run to the far side -- where the skip distance of render_utils.h:643-651 decides the bits.  Over the speckled grid every
    cascade a ray crosses emits samples, so the cell lookup of each (mip_bound = min(2^level, bound), :601-614) is on show."""
    desc, o, geo = model(name, grid)
    ro, rd, nr, fr = march_rays(name, view=view, grid=grid)
    opts = nh.default_options()
    opts.dt_gamma = dt_gamma
    t, idx = nr.copy(), np.arange(len(nr))
    rounds = hops = 0
    seen = set()
    while len(idx) and rounds < 40:
        rx, rdr, rdl = rk.march_first_round(geo, ro[idx], rd[idx], t, fr[idx], 8, dt_gamma)
        wx, wdr, wdl = o.march(ro[idx], rd[idx], t, fr[idx], 8, opts)
        what = f"{name} {view} dt_gamma {dt_gamma} round {rounds}"
        same_bits(wx, rx, f"xyzs {what}")
        same_bits(wdl, rdl, f"deltas {what}")
        written = rdl[:, :, 0] != 0
        hops += int((written & (rdl[:, :, 1] > np.float32(1.5) * rdl[:, :, 0])).sum())  # a sample that followed a hop: t - last_t spans it
        seen |= set(np.unique(levels_visited(geo, rx[written])).tolist())
        for k in range(8):
            t = (t + rdl[:, k, 1]).astype(np.float32)
        full = written.all(axis=1)
        idx, t = idx[full], t[full]
        rounds += 1
    if grid == "speckle" and view == "far":
        assert sorted(seen) == list(range(geo.cascade)), "the speckled grid's far view samples every cascade"
    print(f"resumed march {name} {view} {grid} dt_gamma {dt_gamma}: {rounds} rounds, {hops} samples behind a hop, cascades sampled {sorted(seen)}")
    assert rounds >= 3 and hops >= len(nr) // 8  # coverage floor: a hop ahead of a sample on an eighth of the rays


def test_far_view_reaches_the_outer_cascades():
    """What the "far" view is for: its rays' marches start outside cascade 0 (the entry position's level, from the reference's
    own near), so the hops through outer cascades -- mip_bound = min(2^level, bound), render_utils.h:601-603 -- are compared."""
    for name in ("h32-b4-c3", "h64-b1.5-c2"):
        desc, o, geo = model(name)
        for view, want in (("near", False), ("far", True)):
            ro, rd, nr, fr = march_rays(name, view=view)
            entry = ro + nr[:, None] * rd
            outer = levels_visited(geo, np.clip(entry, -geo.bound, geo.bound)) > 0
            print(f"{name} {view}: {outer.mean():.3f} of the rays enter in an outer cascade")
            assert (outer.mean() > 0.9) == want


@pytest.mark.parametrize("perturb", [1, 7])
@pytest.mark.parametrize("name", ["h32", "h32-b4-c3"])
def test_march_perturbed_first_round(name, perturb):
    """perturb > 0 in the first round only (i = 0, rays_alive the identity): there the reference's pcg32(n, perturb) takes the
    ray's place in the alive list, which is the ray's own number -- the index the oracle's schedule-free form uses
    ("the ray's place in the call").  The reference's own m_perturb is a bool, so it only ever passes 1."""
    desc, o, geo = model(name)
    ro, rd, nr, fr = march_rays(name)
    opts = nh.default_options()
    opts.perturb = perturb
    assert rk.lib().refk_pcg32_first_float(5, perturb) == op.lib().nrfo_pcg32_first_float(5, perturb)
    rx, rdr, rdl = rk.march_first_round(geo, ro, rd, nr, fr, 4, opts.dt_gamma, perturb)
    wx, wdr, wdl = o.march(ro, rd, nr, fr, 4, opts)
    ux = rk.march_first_round(geo, ro, rd, nr, fr, 4, opts.dt_gamma, 0)[0]
    assert (ux.view(U32) != rx.view(U32)).any(), "the perturbation changed nothing"
    same_bits(wx, rx, f"xyzs {name} perturb {perturb}")
    same_bits(wdr, rdr, f"dirs {name} perturb {perturb}")
    same_bits(wdl, rdl, f"deltas {name} perturb {perturb}")


# --------------------------------------------------------------------------------------------------------------- compositing
def composite_chain(name, composite_fn, march_fn):
    """Two chained march + composite calls of 8 slots with the random sigmas and colours of test_march_bit_exact_and_composite:
    call 2 takes the survivors of call 1 (rays_t >= 0, what kernel_compact_rays keeps) from their rays_t and state."""
    ro, rd, nr, fr = march_rays(name)
    n = len(nr)
    rng = np.random.default_rng(4)
    sig = rng.uniform(0, 400, (2, n, 8)).astype(np.float32)
    rgb = rng.random((2, n, 8, 3), dtype=np.float32)
    sig[1] *= np.float32(0.02)  # call 2: thin, so that some rays march on to the far side and leave by `deltas == 0`
    out = []
    idx, t, state = np.arange(n), nr.copy(), np.zeros((n, 5), np.float32)
    for call in range(2):
        dl = march_fn(ro[idx], rd[idx], t, fr[idx])
        t, state = composite_fn(sig[call][idx], rgb[call][idx], dl, t, state)
        out.append((idx, dl, t, state))
        keep = t >= 0
        idx, t, state = idx[keep], t[keep], state[keep]
    return out


@pytest.mark.parametrize("name", ["h32", "h32-b4-c3"])
def test_composite_chained(name):
    desc, o, geo = model(name)
    opts = nh.default_options()
    ref = composite_chain(name, rk.composite, lambda ro, rd, t, fr: rk.march_first_round(geo, ro, rd, t, fr, 8, opts.dt_gamma)[2])
    ora = composite_chain(name, op.composite, lambda ro, rd, t, fr: o.march(ro, rd, t, fr, 8, opts)[2])
    t_exit = d_exit = alive = 0
    for call, ((ri, rdl, rt, rs), (oi, odl, ot, os_)) in enumerate(zip(ref, ora)):
        assert np.array_equal(ri, oi)
        same_bits(odl, rdl, f"deltas {name} call {call}")
        same_bits(ot, rt, f"rays_t {name} call {call}")
        same_bits(os_, rs, f"state {name} call {call}")
        dead = rt == -1
        full = (rdl[:, :, 0] != 0).all(axis=1)
        opaque = (np.float32(1) - rs[:, 0]).astype(np.float64) < 1e-4  # a ray left by `T < 1e-4` ends with T below it
        t_exit += int((dead & full).sum())            # all 8 slots written and still dead: only `T < 1e-4` does that
        d_exit += int((dead & ~full & ~opaque).sum())  # dead, never opaque: only `deltas == 0` does that
        alive += int((~dead).sum())
    print(f"composite {name}: T < 1e-4 exits {t_exit}, deltas == 0 exits {d_exit}, rays handed on alive {alive}")
    assert t_exit > 0 and d_exit > 0 and alive > 0 and len(ref[1][0]) > 0


# ---------------------------------------------------------------------------------------------------- network normalisation
@pytest.mark.parametrize("name", ["h32", "h32-b4-c3"])
def test_network_normalisation(name):
    """linear_transformer<float> with the call site's arguments (1.0 / (2 * bound), 0.5; 0.5, 0.5), then the oracle's encodings and
    MLPs, then the reference's decompose_network_in_and_out on the fp16 output: Oracle.network's bits"""
    desc, o, geo = model(name)
    rng = np.random.default_rng(11)
    n = 3001
    xyz = rng.uniform(-geo.bound, geo.bound, (n, 3)).astype(np.float32)
    xyz[:8] = np.array([[-1, -1, -1], [1, 1, 1], [0, 0, 0], [-0.0, 1, -1], [1, -1, 0.5], [0.25, 0.5, 0.75], [1e-8, -1e-8, 1],
                        [0.99999994, -0.99999994, 0]], np.float32) * np.float32(geo.bound)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sig, rgb = rk.network_through_reference_maps(o, geo, xyz, d)
    wsig, wrgb = o.network(xyz, d)
    same_bits(wsig, sig, f"sigma {name}")
    same_bits(wrgb, rgb, f"rgb {name}")


# --------------------------------------------------------------------------------------------------------------- whole frame
def compare_frame(got, want, what):
    """oracle (rgba [H][W][4], depth) against the driver (rgb, depth, alpha, nears); depth under the D-3 mask"""
    rgba, depth = got
    rgb, rdepth, alpha, nears = want
    share = hit_share(nears, what)
    same_bits(rgba[..., :3], rgb, f"rgb {what}")
    same_bits(rgba[..., 3], alpha, f"alpha {what}")
    miss = nears == FLT_MAX  # D-3, from the reference's own output
    assert miss.mean() <= 1.0 - share + 1e-12
    assert np.isnan(rdepth[miss]).all() and (depth[miss] == 0).all(), "D-3: the reference's depth of a miss is 0 / 0, the oracle's 0"
    same_bits(depth[~miss], rdepth[~miss], f"depth {what}")
    # the 8-bit planes, where the reference's conversion is defined (D-2: the oracle saturates outside)
    rgb8, d8 = op.quantize_u8(rgba, np.where(miss, 0, depth).astype(np.float32))
    want8, ok = rk.to_u8(rgb)
    wantd8, okd = rk.to_u8(np.where(miss, 0, rdepth))
    print(f"{what}: 8-bit conversion defined for {ok.mean():.4f} of the colour values, {okd.mean():.4f} of the depths")
    assert ok.mean() >= 0.99 and okd.mean() >= 0.99
    assert np.array_equal(rgb8[ok], want8[ok]) and np.array_equal(d8[okd & ~miss], wantd8[okd & ~miss]), f"8-bit planes {what}"


@pytest.mark.parametrize("az,el,bg,fl_scale", [(30, 30, 1, 1.0), (200, -15, 1, 1.0), (30, 30, 0, 1.0), (120, 10, 1, 1.25)])
def test_whole_frame(az, el, bg, fl_scale):
    """render_frame's loop (nerf_render.cu:238-360) with every kernel the reference's against Oracle.render, float planes.

    The oracle's SCHED_REFERENCE restates the loop over ONE alive list of all W * H rays: the single-device program.  The
    reference as it stands is built with NGPU = 2: each device runs the loop on its half of the pixels, and `N / num_alive`
    (nerf_render.cu:300) sees N = W * H / 2 and that half's alive count.  A round's n_step decides where a ray's march is cut
    and resumed from the composited t (the sum of deltas[1], not the march's own t), so the two loops differ in the last bits
    and are held apart: one device against SCHED_REFERENCE, two devices against SCHED_REFERENCE_HALVES.
    The reference's background is an int (nerf_render.h:74), so the non-default one is 0.  The last case steps back (the usual orbit
    sits inside the box's bounding sphere: every ray hits) until part of the frame misses the box: the
    in-frame witness of D-3."""
    desc, o, geo = model("h32")
    W, H = 64, 48
    cam, pose = syn.default_camera(W, H), syn.orbit_pose(az, el, radius=4.0311 if fl_scale == 1.0 else 12.0)
    cam[:2] *= np.float32(fl_scale)
    opts = nh.default_options()
    opts.bg_color = float(bg)
    log1, log2 = [], {}
    one = rk.render_frame(o, geo, cam, pose, W, H, opts, one_device=True, log=log1)
    rgba, depth, st = o.render(cam, pose, W, H, opts, schedule=op.SCHED_REFERENCE)
    compare_frame((rgba, depth), one, f"one device az {az} bg {bg}")
    assert st.n_rounds == len(log1) and len({s for _, s in log1}) > 1, "the step rule never left n_step = 1"
    two = rk.render_frame(o, geo, cam, pose, W, H, opts, one_device=False, log=log2)
    rgba2, depth2, st2 = o.render(cam, pose, W, H, opts, schedule=op.SCHED_REFERENCE_HALVES)
    compare_frame((rgba2, depth2), two, f"two devices az {az} bg {bg}")
    assert st2.n_rounds == len(log2[0]) + len(log2[1])
    print(f"rounds: one device {len(log1)}, two devices {len(log2[0])} + {len(log2[1])}; "
          f"planes differ between the two loops in {int((rgba.view(U32) != rgba2.view(U32)).sum())} values")


# --------------------------------------------------------------------------------------------------------- deviation witnesses
def test_deviation_d3_depth_of_a_miss():
    """get_image_and_depth on a ray that missed (near = far = FLT_MAX, nothing accumulated): rgb = background, depth = 0 / 0"""
    nears = np.array([FLT_MAX, 1.0, FLT_MAX], np.float32)
    fars = np.array([FLT_MAX, 3.0, FLT_MAX], np.float32)
    image, depth = rk.get_image_and_depth(np.zeros((3, 3), np.float32), np.array([0, 2.0, 0], np.float32), nears, fars,
                                          np.zeros(3, np.float32), 1)
    assert np.isnan(depth[[0, 2]]).all() and depth[1] == np.float32(0.5) and (image == 1).all()


def test_deviation_d8_density_scale_is_an_int():
    """matrix_multiply_1x1n(int a, ...): 0.5 becomes 0, 2.7 becomes 2.  The oracle multiplies by the float.  In a frame: with
    density_scale 0.5 the literal loop renders nothing; the oracle equals the same loop with a float product in that one place;
    with an integral scale the two agree bit for bit."""
    s = np.array([0.0, 1.5, 400.0, 3.0e-3], np.float32)
    assert (rk.matrix_multiply_1x1n(0.5, s) == 0).all()
    same_bits(rk.matrix_multiply_1x1n(2.7, s), np.float32(2) * s, "int(2.7) * sigma")
    desc, o, geo = model("h32")
    W, H = 32, 24
    cam, pose = syn.default_camera(W, H), syn.orbit_pose(30, 30)
    opts = nh.default_options()
    opts.density_scale = 0.5
    rgb, rdepth, alpha, nears = rk.render_frame(o, geo, cam, pose, W, H, opts, one_device=True)
    assert (alpha == 0).all() and (rgb == 1).all(), "literal reference: a density scale of 0.5 is 0"
    rgba, depth, _ = o.render(cam, pose, W, H, opts, schedule=op.SCHED_REFERENCE)
    assert (rgba[..., 3] > 0.5).any()
    real = rk.matrix_multiply_1x1n
    try:
        rk.matrix_multiply_1x1n = lambda a, v: (np.float32(a) * np.asarray(v, np.float32)).astype(np.float32)
        compare_frame((rgba, depth), rk.render_frame(o, geo, cam, pose, W, H, opts, one_device=True), "density_scale 0.5 as a float")
    finally:
        rk.matrix_multiply_1x1n = real
    opts.density_scale = 2.0
    rgba, depth, _ = o.render(cam, pose, W, H, opts, schedule=op.SCHED_REFERENCE)
    compare_frame((rgba, depth), rk.render_frame(o, geo, cam, pose, W, H, opts, one_device=True), "density_scale 2")


# --------------------------------------------------------------------------------------------------------------- density grid
@pytest.mark.parametrize("H", [8, 32])
def test_density_grid_helpers(H):
    """init_xyzs, dd_scale, add_random and dg_update against tests/density_grid_replay.py, up to D-9: the reference's generator
    (nerf_render.cu:388-429) is dead code.  What the replay FOLLOWS: init_xyzs's lattice and cell order (render_utils.h:95-105,
    with the grid's own H: the call at nerf_render.cu:406 leaves the default 128), the scale bound_c - bound_c / H (:409-412),
    0.001691 (:417), dg_update's rule (render_utils.h:125-127) from 1/64 (:393).  What it CORRECTS: dd_scale's inverted null test
    (render_utils.h:85: with a source it scales the DESTINATION and ignores the source), the density query that is commented
    out (:415), dg_update running once after the cascade loop on the last cascade's values only (:420); and it drops add_random's
    jitter, which as written hands every thread a copy of the same generator, so every coordinate moves by the same amount."""
    lattice = rk.init_xyzs(H).reshape(-1, 3)
    for bound, c in ((1.0, 0), (4.0, 1), (1.5, 1)):
        b = dgr.cascade_bound(bound, c)
        k = np.float32(b - np.float32(b / np.float32(H)))
        want = dgr.positions(H, bound, c)
        # literal dd_scale: the source is ignored, the destination scaled in place -- so scaling the lattice in place is the replay
        junk = np.full(lattice.size, 7.0, np.float32)
        same_bits(rk.dd_scale(junk, lattice.reshape(-1), H, k).reshape(-1, 3), want, f"positions H {H} bound {bound} cascade {c}")
        same_bits(rk.dd_scale(lattice.reshape(-1), junk, H, k), np.full(lattice.size, np.float32(7.0) * k, np.float32),
                  "dd_scale literal: k * destination")
        # add_random as written: one and the same offset k * (2 * u - 1) for every element, u the seed's first float
        half = np.float32(b / np.float32(H))
        u = np.float32(op.lib().nrfo_pcg32_first_float(42, 1))
        shift = np.float32(half * np.float32(np.float32(2) * u - np.float32(1))) + np.float32(0)
        same_bits(rk.add_random(want.reshape(-1), 42, H, half), (want.reshape(-1) + shift).astype(np.float32), "add_random literal")
    # dg_update against the replay's rule: sigma -> 0.001691 * sigma -> n iterations from 1/64
    rng = np.random.default_rng(H)
    sigma = np.concatenate([rng.uniform(0, 60, H ** 3 - 6), [0, 1e-9, 9.2, 9.3, np.inf, np.nan]]).astype(np.float32)
    tmp = (dgr.SCALE * sigma).astype(np.float32)
    for decay, n_it in ((0.95, 1), (0.95, 16), (0.5, 3)):
        g = np.full(H ** 3, dgr.START, np.float32)
        for _ in range(n_it):
            g = rk.dg_update(g, tmp, decay, H)
        same_bits(dgr.update(sigma, n_it, decay), g, f"dg_update H {H} decay {decay} x{n_it}")
    neg = np.array([-1.0, -0.0, 0.5] + [0.25] * (H - 3), np.float32)  # a negative cell is left alone, -0.0 is not negative
    got = rk.dg_update(neg, np.full(H, 0.3, np.float32), 0.95, H)
    assert got[0] == -1 and got[1] == np.float32(0.3) and got[2] == np.float32(0.5) * np.float32(0.95)


# ----------------------------------------------------------------------------------------------------------- transfer curves
def test_transfer_functions():
    """linear_to_srgb of common_device.cuh against the oracle's copy, bit for bit: nrfo_rb_accumulate applies it to a frame whose
    colour space is sRGB, and with sample_count 0 over a zero accumulator the result is that value itself, (0 * 0 + v) / 1.
    srgb_to_linear has no entry point of its own in the oracle: held to its definition (the float64 curve, a few ulps) and to
    being linear_to_srgb's inverse as far as the reference's exponent 0.41666 (not 1 / 2.4) lets it be."""
    x = np.concatenate([np.linspace(0, 1, 4001), [0.04045, 0.0404501, 0.0031308, 0.00313079, 1.5, 2.0 ** -20]]).astype(np.float32)
    frame = np.zeros((len(x), 4), np.float32)
    frame[:, 0], frame[:, 1], frame[:, 2], frame[:, 3] = x, x, x, 1
    acc = op.rb_accumulate(frame, np.zeros_like(frame), 0, nh.CS_SRGB)
    same_bits(acc[:, 0], rk.linear_to_srgb(x), "linear_to_srgb")
    lin = rk.srgb_to_linear(x)
    x64 = x.astype(np.float64)
    want = np.where(x <= np.float32(0.04045), x64 / np.float64(np.float32(12.92)),
                    ((x64 + np.float64(np.float32(0.055))) / np.float64(np.float32(1.055))) ** np.float64(np.float32(2.4)))
    # two rounded fp32 operations ahead of the power (each 2^-24 relative, raised to 2.4), powf's own ulp and the result's
    assert np.all(np.abs(lin - want) <= 8 * 2.0 ** -24 * want), "srgb_to_linear against its definition"
    assert np.abs(rk.linear_to_srgb(lin[:4001]) - x[:4001]).max() < 2e-4


# ------------------------------------------------------------------------------------------------------------ golden vectors
def test_golden_vectors_regenerate_to_the_committed_bytes(tmp_path):
    """tests/golden/reference_kernels.npz, regenerated from the library: the same members in the same order, every member's .npy
    bytes equal.  (Members are compared uncompressed: the deflate stream around them may differ between zlib builds.)"""
    gen = golden_generator()
    from pathlib import Path

    committed = Path(gen.__file__).with_name("reference_kernels.npz")
    assert committed.stat().st_size <= 160753, "larger than the largest fixture that was here before it"
    out = tmp_path / "reference_kernels.npz"
    gen.write(out)
    fresh, kept = gen.read_members(out), gen.read_members(committed)
    assert [n for n, _ in fresh] == [n for n, _ in kept]
    stale = [n for (n, a), (_, b) in zip(fresh, kept) if a != b]
    assert not stale, f"tests/golden/reference_kernels.npz is stale in {stale}: run tests/golden/make_reference_golden.py"
