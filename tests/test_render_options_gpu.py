"""nrf_options (density_scale, min_near, dt_gamma, max_steps, bg_color) through every ray entry point and every stage.

The rows are those of tests/render_options.py.  The pinhole frame of the hot instance is held to float64 under each option by the
fog legs (tests/probe_model.py, "fog-option-" and, for the wide and generic stages, "fog-stageoption-"); this file ties everything
else to that frame, under the option:

  1. nrf_render_rays on the rays nrf_generate_rays writes == nrf_render of the camera, bit for bit, equal n_composited and n_rays;
  2. orthographic rays against the assembled oracle (tests/rays_oracle.py, which takes density_scale) at the frame tolerances;
  3. nrf_render_rays_clipped without limits == nrf_render_rays; a t_min at or below min_near changes no bit; the t_max ramp against
     the checker of tests/rays_clip_oracle.py;
  4. NRF_RAYS_DENSITY_ONLY against the same call without the flag, with and without the ramp;
  5. nrf_ray_hits against the density-only call clipped at the crossing sample, and against the checker of tests/ray_hits_oracle.py;
  6. nrf_hit_gradients on the hits of a density_scale 0.37 frame;
  7. the exact rows: density_scale 0 and a min_near beyond every far, where the frame is the background and n_composited the march's.

A bit-for-bit twin cannot see an option that both of its sides ignore.  So every test that rests on twins also renders the
default-options frame of the same rays on the same context and asserts rows.moved against it: the condition that
tests/test_render_rays_cpu.py::test_every_row_moves_the_frame proves on the oracle for every model and frame size used here.

Matrix: the hot models (bound 1; bound 4 with three cascades) under the persistent and the per-strip kernel take every row, the
frame size alternating between 64 x 48 and 33 x 70 from case to case; the wide and generic stages (100 x 52) and the march forms
of tests/rays_forms.py (h30 per strip, h64-b1.5-c2 persistent, wide-h30) take rows.REDUCED.  Every test here needs a GPU."""
import functools

import numpy as np
import pytest

import models
import nerfhip as nh
import oracle_py as op
import points_replay as pr
import rays_clip_oracle as rco
import rays_forms as rf
import rays_oracle as ro
import render_options as rows
import synthetic as syn
import test_ray_hits_gpu as hits
import test_render_rays_clip_gpu as clip
import test_render_rays_density_gpu as dens
import test_render_rays_gpu as rr
from test_render_rays_clip_gpu import _bits, _clipped, _context, _device_rays, _options

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = [(64, 48), (33, 70)]
HOT = [(m, s) for m in clip.SMALL for s in clip.SCHED]
RAMP = (0.7, 0.9)  # rays_clip_oracle.ramp's own
# nrf_ray_hits at opacity 0.5 on the framed rays: the share of hits the scene must have.  The existing 0.4 holds on the checker under
# every row (0.54 .. 0.67) but max_steps1, where a ray hits only if its first sample alone reaches the threshold: 0.13 .. 0.17
HIT_SHARE = {"max_steps1": 0.1}
STAGES = {"wide-frequency12": (dict(dir_otype="Frequency", n_frequencies=12), 2), "generic-sine": (dict(activation="Sine"), 1),
          "generic-F4-w32": (dict(n_features_per_level=4, n_neurons=32), 1)}
FORMS = [("h30", "strip"), ("h64-b1.5-c2", "persistent"), ("wide-h30", "strip")]


@functools.lru_cache(maxsize=None)
def _hot(model):
    return models.build_model(log2_hashmap_size=12, H=32, **clip.SMALL[model])


@functools.lru_cache(maxsize=None)
def _stage(name):
    return models.build_model(log2_hashmap_size=12, H=32, **STAGES[name][0])


def _bg(kw):
    return np.float32(kw.get("bg_color", nh.default_options().bg_color))


def _camera_rays(ctx, cam, W, H):
    o, d = torch.empty((H * W, 3), device="cuda"), torch.empty((H * W, 3), device="cuda")
    torch.cuda.synchronize()
    ctx.generate_rays(cam, syn.orbit_pose(30, 30), o.data_ptr(), d.data_ptr(), 0, 0)
    return o, d


def _default_frame(ctx, o, d, n, kw):
    """The frame of the same rays under the default options, on the same context; the row's options are put back"""
    _options(ctx)
    frame = _clipped(ctx, o, d, n)[:2]
    _options(ctx, **kw)
    return frame


def _entry_points(ctx, W, H, row, kw, what, share, twin_rays=None, ramp=RAMP, hit_rays=None):
    """Items 1, 3 (no limits), 4 and 5 of one context under one row.  twin_rays / hit_rays: None for the default camera's / the
    framed camera's of tests/test_ray_hits_gpu.py."""
    n = W * H
    # 1. the pinhole identity, and the row moved the pinhole frame
    rr._pinhole_identity(ctx, W, H, 30, 30, what)
    frame = ctx.read_f32()
    st = ctx.stats()
    o, d = _device_rays(ctx, W, H)
    rows.assert_moved(row, frame, _default_frame(ctx, o, d, n, kw), (what, "pinhole"))
    # 3. the clipped call without limit arrays
    plain = _clipped(ctx, o, d, n)
    clip._same(plain[:2], frame, (what, "clipped, no arrays"))
    assert plain[2].n_composited == st.n_composited and plain[2].n_rays == st.n_rays, what
    # 4. the density-only twin, without a limit and under the ramp
    to, td = (o, d) if twin_rays is None else twin_rays
    B = np.full((H, W, 3), _bg(kw), np.float32)
    for name, lim in (("no limit", dict()), ("t_max ramp", dict(t_max=rco.ramp(W, H, *ramp)))):
        p, dn = dens._both(ctx, to, td, n, **lim)
        dens._check_twin(p, dn, B, (what, name))
        if name == "no limit" and twin_rays is not None:
            rows.assert_moved(row, p[:2], _default_frame(ctx, to, td, n, kw), (what, "twin rays"))
    # 5. ray hits against the density-only call
    ho, hd = hits._framed_rays(ctx, W, H) if hit_rays is None else hit_rays
    for opacity in hits.OPACITIES:
        rec, dep, hst, D = hits._check_against_density_only(ctx, ho, hd, n, opacity, what, share=share if opacity == 0.5 else None)
        if row == "max_steps1":  # a crossing sample can only be a ray's first: nothing was composited before it
            hit = rec[:, 3] >= np.float32(opacity)
            assert np.all(rec[hit, 2] == 0) and hst.n_composited <= n, (what, opacity)


# ---------------------------------------------------------------- 1, 3, 4, 5: the hot instances under every row
@pytest.mark.parametrize("row", list(rows.ROWS))
@pytest.mark.parametrize("model,sched", HOT)
def test_the_hot_ray_entry_points_under_the_row(model, sched, row):
    desc, keep, _ = _hot(model)
    W, H = SIZES[(list(rows.ROWS).index(row) + HOT.index((model, sched))) % 2]
    kw = rows.fields(row, desc.bound)
    ctx = _context(desc, W, H, clip.SCHED[sched], **kw)
    try:
        assert clip._rays_instance(ctx) == (16 if sched == "persistent" else 0)
        _entry_points(ctx, W, H, row, kw, (model, sched, row, W, H), HIT_SHARE.get(row, 0.4))
    finally:
        ctx.close()


# ---------------------------------------------------------------- 1, 3, 4, 5: the other stages and march forms under the reduced rows
@pytest.mark.parametrize("row", rows.REDUCED)
@pytest.mark.parametrize("name", list(STAGES))
def test_the_wide_and_generic_stages_under_the_row(name, row):
    desc, keep, _ = _stage(name)
    W, H = 100, 52
    kw = rows.fields(row, desc.bound)
    ctx = _context(desc, W, H, None, **kw)
    try:
        assert clip._rays_instance(ctx) == STAGES[name][1], name
        if name == "generic-sine":  # (a thin object: see render_options.SINE_ZOOM)
            rays = _camera_rays(ctx, rows.zoomed_camera(W, H, rows.SINE_ZOOM), W, H)
            _entry_points(ctx, W, H, row, kw, (name, row), rows.SINE_HIT_SHARE.get(row, 0.1), twin_rays=rays, ramp=rows.SINE_RAMP, hit_rays=rays)
        else:
            _entry_points(ctx, W, H, row, kw, (name, row), 0.4)
    finally:
        ctx.close()


@pytest.mark.parametrize("row", rows.REDUCED)
@pytest.mark.parametrize("form,sched", FORMS)
def test_the_other_march_forms_under_the_row(form, sched, row):
    assert sched in rf.schedules(form)
    desc, keep, _ = rf.build(form)
    env = rf.SCHED[sched]
    W, H = rf.RW, rf.RH
    kw = rows.fields(row, desc.bound)
    ctx = _context(desc, W, H, env, **kw)
    try:
        assert clip._rays_instance(ctx) == rf.expected_instance(form, env), (form, sched)
        _entry_points(ctx, W, H, row, kw, (form, sched, row), 0.4, hit_rays=_device_rays(ctx, W, H))
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. rays a pinhole cannot describe
ORTHO_ROWS = ["density_scale0.37", "density_scale2", "min_near0.05", "dt_gamma0", "max_steps7"]


@pytest.mark.parametrize("model,sched", HOT)
def test_orthographic_rays_match_the_assembled_oracle_under_the_rows(model, sched):
    """The only check here with a reference that is not the library itself: tests/rays_oracle.py under the row's options (on the
    oracle the object covers 0.13 .. 0.15 of this frame with alpha > 0.5 under every row: the 0.05 of the default-options test stays)."""
    desc, keep, _ = _hot(model)
    W, H = 64, 48
    o, d = ro.orthographic(W, H, half_extent=1.2)
    ctx = _context(desc, W, H, clip.SCHED[sched])
    try:
        assert clip._rays_instance(ctx) == (16 if sched == "persistent" else 0)
        for row in ORTHO_ROWS:
            _options(ctx, **rows.fields(row, desc.bound))
            rr._check_against_oracle(ctx, desc, o, d, W, H, 0.05, ("orthographic", model, sched, row), rows.options(row, desc.bound))
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. the clipped call's limits
@pytest.mark.parametrize("model,sched", HOT)
def test_a_t_min_at_or_below_min_near_changes_no_bit(model, sched):
    """near_far raises near to min_near, and the clamp is `if (t_min > near) near = t_min`: a t_min that is <= min_near everywhere is
    no limit, whatever min_near is.  (And a t_min above it is one: the array is read.)"""
    desc, keep, _ = _hot(model)
    W, H = SIZES[HOT.index((model, sched)) % 2]
    n = W * H
    ctx = _context(desc, W, H, clip.SCHED[sched])
    try:
        o, d = _device_rays(ctx, W, H)
        for row in ("default", "min_near0.05"):
            kw = dict() if row == "default" else rows.fields(row, desc.bound)
            _options(ctx, **kw)
            mn = np.float32(kw.get("min_near", nh.default_options().min_near))
            ctx.render_rays(o.data_ptr(), d.data_ptr(), n)
            want, wst = ctx.read_f32(), ctx.stats()
            assert wst.n_composited > 0 and np.mean(want[0][..., 3] > 0.5) > 0.02
            below = np.minimum(np.linspace(-1.0, 2.0 * float(mn), n).astype(np.float32), mn)
            assert np.any(below == mn) and np.any(below < 0)
            for tname, t_min in (("min_near itself", np.full(n, mn, np.float32)), ("from -1 up to min_near", below), ("zero", np.zeros(n, np.float32))):
                got = _clipped(ctx, o, d, n, t_min=t_min)
                clip._same(got[:2], want, (model, sched, row, tname))
                assert got[2].n_composited == wst.n_composited and got[2].n_rays == wst.n_rays, (row, tname)
            cut = _clipped(ctx, o, d, n, t_min=rco.ramp(W, H))
            assert not np.array_equal(_bits(cut[0]), _bits(want[0])) and cut[2].n_composited < wst.n_composited, row
    finally:
        ctx.close()


@pytest.mark.parametrize("row", ["density_scale0.37", "max_steps7"])
@pytest.mark.parametrize("model,sched", HOT)
def test_the_ramp_matches_the_checker_under_the_row(model, sched, row):
    """tests/test_render_rays_clip_gpu.py::test_the_ramp_matches_the_checker with the context and the checker under the row (on the
    checker the ramp cuts 0.25 .. 0.27 of the frame fully under both rows: its 0.2 stays)."""
    clip._ramp_matches_the_checker(model, sched, "t_max", rows.fields(row))


# ---------------------------------------------------------------- 5. ray hits against the checker
# row -> (the largest share of the checker's hit rays that may be uncertain, the smallest share of rays that are certain hits): both
# are statements about the checker's scene, printed by the helper.  Checker, bound 1 / bound 4: density_scale0.37 0.184 / 0.211
# uncertain (thinner matter adds less per sample: more weight sums pass close by the threshold) and 0.425 / 0.409 certain hits;
# density_scale2 0.040 / 0.050 and 0.529 / 0.523: the default-options conditions; max_steps1 0.033 / 0.049 and 0.133 / 0.107
HITS_ORACLE_ROWS = {"density_scale0.37": (0.25, 0.4), "density_scale2": (0.12, 0.4), "max_steps1": (0.12, 0.1)}


@pytest.mark.parametrize("row", list(HITS_ORACLE_ROWS))
@pytest.mark.parametrize("model,sched", HOT)
def test_ray_hits_against_the_checker_under_the_row(model, sched, row):
    """tests/test_ray_hits_gpu.py::test_against_the_checker_at_one_half under the row, its margin rule and tolerances unchanged.
    max_steps1: every record's crossing sample is the ray's first -- the weight sum before it is 0."""
    max_uncertain, min_both = HITS_ORACLE_ROWS[row]
    rec, dep, want = hits._against_the_checker_at_one_half(model, sched, rows.fields(row), max_uncertain, min_both)
    if row == "max_steps1":
        hit = rec[:, 3] >= np.float32(0.5)
        assert hit.any() and np.all(rec[hit, 2] == 0) and np.all(want.records[want.hit, 2] == 0)


# ---------------------------------------------------------------- 6. hit gradients
def test_hit_gradients_under_density_scale_are_of_the_raw_density():
    """include/nerfhip.h on nrf_density / nrf_density_gradient / nrf_hit_gradients: "density_scale is not applied, options play no
    part" -- the gradient is of the RAW density, and the code agrees: on the hits of a density_scale 0.37 frame nrf_hit_gradients
    equals nrf_density_gradient at the replayed positions bit for bit (as tests/test_density_points_gpu.py has it at the default
    options), and a context with the default options returns the same bits at those positions, its sigma nrf_network's.  The
    records themselves are the option's: of the rays that hit under both settings at least 0.3 cross later under 0.37 (on the
    checker 0.13 .. 0.17 of the rays cross at their first sample, of 0.63 that hit: the others have room to)."""
    import test_density_points_gpu as dp
    desc, keep, _ = _hot("bound1")
    W, H = 64, 48
    n = W * H
    h = np.float32(np.float32(desc.bound) * np.float32(2.0 ** -8))
    kw = rows.fields("density_scale0.37")
    ctx = _context(desc, W, H, **kw)
    try:
        o, d = hits._framed_rays(ctx, W, H)
        f = dp._hit_frame(ctx, o, d, n)
        rec = ctx.read_f32()[0].reshape(-1, 4)
        hit = pr.is_hit(rec, n, 0.5)
        assert hit.sum() >= 0.4 * n
        pos, out = dp._hit_gradients(ctx, f, o, d, n, 0.5, 0.5, h)
        pos, out = pos[:n], out[:n]
        want_pos = pr.hit_position(o.cpu().numpy(), d.cpu().numpy(), rec[:, 0], rec[:, 1], 0.5)
        assert np.array_equal(_bits(pos[hit]), _bits(want_pos[hit]))
        assert np.all(_bits(pos[~hit]) == 0) and np.all(_bits(out[~hit]) == 0)
        scaled = dp._gradient(ctx, pos[hit, :3], h)
        assert np.array_equal(_bits(out[hit]), _bits(scaled))
        assert np.mean(np.any(scaled[:, :3] != 0, axis=1)) > 0.9
        _options(ctx)  # the default options, on the same context and on a fresh one
        f0 = dp._hit_frame(ctx, o, d, n)
        rec0 = ctx.read_f32()[0].reshape(-1, 4)
        assert np.array_equal(_bits(dp._gradient(ctx, pos[hit, :3], h)), _bits(scaled))
    finally:
        ctx.close()
    both = hit & pr.is_hit(rec0, n, 0.5)
    later = float(np.mean(rec[both, 0] > rec0[both, 0]))
    print(f"hits under both settings {np.mean(both):.3f}, of which cross later under density_scale 0.37: {later:.3f}")
    assert np.mean(both) >= 0.4 and later >= 0.3 and np.all(rec[both, 0] >= rec0[both, 0])
    fresh = _context(desc, W, H)
    try:
        raw = dp._gradient(fresh, pos[hit, :3], h)
        assert np.array_equal(_bits(raw), _bits(scaled))
        assert np.array_equal(_bits(raw[:, 3]), _bits(dp._network_sigma(fresh, pos[hit, :3])))
    finally:
        fresh.close()


# ---------------------------------------------------------------- 7. the exact rows
EXACT_INSTANCES = [(m, s) for m, s in HOT] + [("wide-frequency12", None), ("generic-sine", None)]


@pytest.mark.parametrize("name,sched", EXACT_INSTANCES)
def test_the_exact_rows(name, sched):
    """density_scale 0: every sample's alpha is 1 - exp(-0) = 0, so nothing is ever added to a pixel and no ray stops on its
    transmittance -- the frame is (bg, bg, bg, 0) with depth 0, every hit record is zero, and n_composited is the number of samples
    the march emits, which the oracle's march gives exactly (no network value enters it: no tolerance).  A min_near beyond every far:
    no ray is alive, nothing is composited.  Through nrf_render, nrf_render_rays, the clipped call, the density-only call, nrf_ray_hits."""
    hot = sched is not None
    desc, keep, _ = _hot(name) if hot else _stage(name)
    W, H = (64, 48) if hot else (100, 52)
    n = W * H
    cam, pose = syn.default_camera(W, H), syn.orbit_pose(30, 30)
    orc = op.Oracle(desc)
    ctx = _context(desc, W, H, clip.SCHED[sched] if hot else None)
    try:
        assert clip._rays_instance(ctx) == ((16 if sched == "persistent" else 0) if hot else STAGES[name][1])
        o, d = _device_rays(ctx, W, H)
        for row in rows.EXACT_ROWS:
            kw, opts = rows.fields(row, desc.bound), rows.options(row, desc.bound)
            _options(ctx, **kw)
            want_n = int(orc.render(cam, pose, W, H, opts, schedule=op.SCHED_PER_RAY)[2].n_samples)
            assert want_n == 0 if row == "min_near_beyond_far" else want_n > 1000, (row, want_n)
            bg = _bg(kw)

            def background(rgba, depth, st, what):
                print(f"{name} {sched} {row} {what}: composited {st.n_composited} (oracle {want_n})")
                assert np.all(rgba[..., :3] == bg) and np.all(rgba[..., 3] == 0) and np.all(depth == 0), (name, sched, row, what)
                assert int(st.n_composited) == want_n, (name, sched, row, what, int(st.n_composited), want_n)

            ctx.render(cam, pose)
            background(*ctx.read_f32(), ctx.stats(), "nrf_render")
            ctx.render_rays(o.data_ptr(), d.data_ptr(), n)
            background(*ctx.read_f32(), ctx.stats(), "nrf_render_rays")
            background(*_clipped(ctx, o, d, n), "nrf_render_rays_clipped")
            background(*_clipped(ctx, o, d, n, flags=nh.NRF_RAYS_DENSITY_ONLY), "density only")
            rec, dep, st = hits._hits(ctx, o, d, n, 0.5)
            print(f"{name} {sched} {row} nrf_ray_hits: composited {st.n_composited} (oracle {want_n})")
            assert np.all(rec == 0) and np.all(dep == 0), (name, sched, row, "hit records")
            assert int(st.n_composited) == want_n, (name, sched, row, "nrf_ray_hits", int(st.n_composited), want_n)
    finally:
        ctx.close()
