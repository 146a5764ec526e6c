"""nrf_render_rays and nrf_render_rays_clipped on the GPU at every march form: the rows of tests/rays_forms.py.

tests/test_render_rays_gpu.py and tests/test_render_rays_clip_gpu.py render a grid of side 32 at bound 1 (march form UNIT) and at
bound 4 with three cascades (POW2).  The rows here reach the other RAYS instances of nrf_kernels_rays.hip -- every GENERIC-form
one (a grid side or a bound that is no power of two, a bound below 1; march tables in LDS, or in global memory for a side that
is no multiple of 4), the wide POW2 one and the persistent 8-bit ones -- with the checks of those two files (their helpers are
imported, not copied):

  a  the rays nrf_generate_rays writes render the pinhole frame bit for bit;
  b  limits that limit nothing change no bit;
  c  the ramp as t_max and as t_min against the checker, at the project's tolerances for oracle frames;
  d  the clipped frame does not depend on the schedule;
  e  independence, monotonicity, empty intervals;
  f  metric depth, 8-bit outputs, views;
  g  orthographic and equirectangular rays against the assembled oracle (the panorama's origin lies inside the outer cascades).

Every test first asserts the nrf_debug_rays_instance code the row names; every case creates and closes its own context."""
import numpy as np
import pytest

import models
import nerfhip as nh
import oracle_py as op
import rays_clip_oracle as rco
import rays_forms as rf
import rays_oracle as ro
import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import test_render_rays_clip_gpu as clip  # noqa: E402  (helpers: _context, _clipped, _no_limit_changes_no_bit, ...)
import test_render_rays_gpu as rays  # noqa: E402  (helpers: _pinhole_identity, _check_against_oracle)

RW, RH = rf.RW, rf.RH
OTHER_ROWS = rf.WIDE_ROWS + rf.SINE_ROWS
POW2_SMALL = "bound4-cascade3"  # the POW2 model of the two existing files (H = 32): its persistent 8-bit instance is launched here


def _open(row, sched, W, H, env=None, **opts_kw):
    """A context for the row under the schedule (plus `env`), after asserting that it launches the RAYS instance the row names"""
    env = dict(rf.SCHED[sched], **(env or {})) if rf.ROWS[row][1] == rf.HOT else env
    ctx = clip._context(rf.build(row)[0], W, H, env, **opts_kw)
    assert clip._rays_instance(ctx) == rf.expected_instance(row, env), (row, sched)
    return ctx


@pytest.mark.parametrize("row", rf.NO_COARSE_ROWS)
def test_a_grid_without_the_coarse_level_has_no_persistent_form(row):
    for env in (rf.PERSISTENT, rf.STRIP, None):
        ctx = clip._context(rf.build(row)[0], RW, RH, env)
        assert clip._rays_instance(ctx) == 0, (row, env)
        ctx.close()


# ---------------------------------------------------------------- a. generated rays render the pinhole frame bit for bit
@pytest.mark.parametrize("W,H,az,el", [(64, 64, 30, 30), (33, 70, 250, -20)])
@pytest.mark.parametrize("row,sched", rf.hot_cases())
def test_generated_rays_render_the_pinhole_frame_bit_for_bit(row, sched, W, H, az, el):
    ctx = _open(row, sched, W, H)
    rays._pinhole_identity(ctx, W, H, az, el, (row, sched, W, H))
    ctx.close()


@pytest.mark.parametrize("row", OTHER_ROWS)
def test_generated_rays_render_the_pinhole_frame_in_the_wide_and_generic_instances(row):
    W, H = 100, 52
    ctx = _open(row, "strip", W, H)
    rays._pinhole_identity(ctx, W, H, 135, 10, row)
    ctx.close()


# ---------------------------------------------------------------- b. limits that limit nothing
@pytest.mark.parametrize("row,sched", rf.hot_cases() + [(r, "strip") for r in OTHER_ROWS])
def test_no_limit_changes_no_bit(row, sched):
    W, H = 100, 52
    _open(row, sched, W, H).close()
    clip._no_limit_changes_no_bit(rf.build(row)[0], rf.SCHED[sched] if rf.ROWS[row][1] == rf.HOT else None, W, H, (row, sched))


# ---------------------------------------------------------------- c. the ramp against the checker
def _ramp_against_the_checker(row, sched, kind, n_tol):
    desc, o, d, full, t, (want, wdepth, n, raw), (near, far) = rf.checked(row, kind)
    ctx = _open(row, sched, RW, RH)
    rgba, depth, st = clip._clipped(ctx, clip._upload(o), clip._upload(d), RW * RH, **{kind: t})
    ctx.close()
    rgba, depth = rgba.reshape(-1, 4), depth.reshape(-1)
    e_rgba, e_depth, psnr = float(np.abs(rgba - want).max()), float(np.abs(depth - wdepth).max()), models.psnr(rgba, want)
    print(f"{row} {sched} {kind}: max|d rgba| {e_rgba:.3e} max|d depth| {e_depth:.3e} psnr {psnr:.1f} dB composited {st.n_composited} "
          f"(checker {n})")
    assert np.all(np.isfinite(rgba)) and np.all(np.isfinite(depth))
    assert e_rgba <= 2.0 / 255.0 and e_depth <= 2.0 / 255.0
    assert psnr >= 45.0
    assert abs(int(st.n_composited) - n) <= n_tol(n), (st.n_composited, n)
    # pixels the checker cuts fully, and empty intervals: exactly the background (bg_color, the default options'), alpha 0, depth 0
    cut = (want[:, 3] == 0) & (full[0][:, 3] > 0.5)
    if kind == "t_max":
        assert np.mean(cut) >= (0.07 if row in rf.SINE_ROWS else 0.2)
    bg = np.float32(nh.default_options().bg_color)
    assert np.all(rgba[cut, :3] == bg) and np.all(rgba[cut, 3] == 0) and np.all(depth[cut] == 0)
    empty = ~(near < far)
    assert np.all(rgba[empty, :3] == bg) and np.all(rgba[empty, 3] == 0) and np.all(depth[empty] == 0)


@pytest.mark.parametrize("kind", ["t_max", "t_min"])
@pytest.mark.parametrize("row,sched", rf.hot_cases())
def test_the_ramp_matches_the_checker(row, sched, kind):
    _ramp_against_the_checker(row, sched, kind, lambda n: 0.002 * n + 8)


@pytest.mark.parametrize("row", rf.WIDE_ROWS)
def test_the_ramp_cuts_rays_in_the_wide_instances(row):
    _ramp_against_the_checker(row, "strip", "t_max", lambda n: 0.002 * n + 8)


@pytest.mark.parametrize("kind", ["t_max", "t_min"])
@pytest.mark.parametrize("row", rf.SINE_ROWS)
def test_the_ramp_cuts_rays_in_the_generic_instances(row, kind):
    """At the tolerances tests/test_generic_gpu.py holds the Sine shape's frames to: 2 / 255 on both planes, 45 dB, and the
    composited samples within 1 % + 16 of the oracle's."""
    _ramp_against_the_checker(row, "strip", kind, lambda n: 0.01 * n + 16)


# ---------------------------------------------------------------- d. the clipped frame does not depend on the schedule
STRIP_VARIANTS = [("strip", {}), ("strip, fast-forward off", dict(NRF_MARCH_FF="0")), ("strip, budget 3", dict(NRF_MARCH_BUDGET="3"))]
PERSISTENT_VARIANTS = [("persistent", {}), ("tail split off", dict(NRF_TAIL_SPLIT="0")), ("fast-forward off", dict(NRF_MARCH_FF="0")),
                       ("budget 3", dict(NRF_MARCH_BUDGET="3"))]


@pytest.mark.parametrize("row", rf.FF_ROWS + rf.NO_COARSE_ROWS)
def test_the_clipped_frame_does_not_depend_on_the_schedule(row):
    W, H = 100, 52
    n = W * H
    t = rco.ramp(W, H)
    frames = {}
    for name, env in (PERSISTENT_VARIANTS if rf.coarse(row) else []) + STRIP_VARIANTS:
        ctx = _open(row, "strip" if "strip" in name else "persistent", W, H, env)
        o, d = clip._device_rays(ctx, W, H)
        frames[name] = [clip._clipped(ctx, o, d, n, t_max=t)[:2],
                        clip._clipped(ctx, o, d, n, t_min=t, t_max=(t + np.float32(0.4)).astype(np.float32))[:2]]
        ctx.close()
    assert len(frames) == (7 if rf.coarse(row) else 3)
    want = frames["persistent" if rf.coarse(row) else "strip"]
    assert np.mean(want[0][0][..., 3] > 0.5) > 0.02 and np.mean(want[1][0][..., 3] > 0.05) > 0.02
    for name, got in frames.items():
        clip._same(got[0], want[0], (row, name, "t_max"))
        clip._same(got[1], want[1], (row, name, "t_min and t_max"))


# ---------------------------------------------------------------- e. independence, monotonicity, empty intervals
@pytest.mark.parametrize("row,sched", rf.hot_cases(["h64-b1.5-c2", "h30-b4-c3"]))
def test_independence_monotonicity_and_empty_intervals(row, sched):
    W, H = 100, 52
    desc = rf.build(row)[0]
    bgc = 0.25
    ctx = _open(row, sched, W, H, bg_color=bgc)
    o, d = clip._device_rays(ctx, W, H)
    n = W * H
    full = clip._clipped(ctx, o, d, n)
    t = rco.ramp(W, H)
    ramp = clip._clipped(ctx, o, d, n, t_max=t)
    a_full, a_ramp = full[0][..., 3].reshape(-1), ramp[0][..., 3].reshape(-1)
    assert np.mean((a_ramp > 0.05) & (a_ramp < a_full - 0.05)) >= 0.02  # (the ramp does cut rays in the middle of the object)

    # independence: a fixed pseudo-random half of the pixels is limited, the other half renders the unlimited frame's bits
    limited = np.random.default_rng(20240607).random(n) < 0.5
    tiles = limited.reshape(H, W)[:H // 8 * 8, :W // 8 * 8].reshape(H // 8, 8, W // 8, 8).mean(axis=(1, 3))
    assert tiles.min() > 0.2 and tiles.max() < 0.8  # every 8x8 tile mixes both kinds: rounds and tail splitting see both
    half = clip._clipped(ctx, o, d, n, t_max=np.where(limited, t, np.float32(np.nan)).astype(np.float32))
    for plane in (0, 1):
        got, free, cutf = (x[plane].reshape(n, -1) for x in (half, full, ramp))
        assert np.array_equal(clip._bits(got[~limited]), clip._bits(free[~limited])), ("unlimited half", plane)
        assert np.array_equal(clip._bits(got[limited]), clip._bits(cutf[limited])), ("limited half", plane)
    assert np.any(a_full[~limited] > 0.5) and np.any(a_ramp[limited] < a_full[limited])

    # monotonicity: the weight sum only ever adds non-negative weights
    wider = clip._clipped(ctx, o, d, n, t_max=(t + np.float32(0.15)).astype(np.float32))
    a_wider = wider[0][..., 3].reshape(-1)
    assert np.all(a_ramp <= a_wider) and np.all(a_wider <= a_full)
    assert np.any(a_ramp < a_wider) and np.any(a_wider < a_full)

    # empty intervals on scattered object pixels: exactly background, every other pixel unchanged
    oh, dh = o.cpu().numpy(), d.cpu().numpy()
    near, far = ro.near_far([desc.aabb[i] for i in range(6)], oh, dh, nh.default_options().min_near)
    on = np.flatnonzero(a_full > 0.5)
    picks = on[np.linspace(0, len(on) - 1, 12).astype(int)]
    assert len(np.unique(picks)) == 12
    t_min, t_max = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    t_max[picks[0:3]] = [0.2, 0.1, -5.0]       # t_max <= min_near
    t_min[picks[3:6]] = far[picks[3:6]]         # t_min >= far
    t_min[picks[5]] = far[picks[5]] + 1.0
    t_min[picks[6:9]] = np.inf
    t_max[picks[9:12]] = -np.inf
    rgba, depth, st = clip._clipped(ctx, o, d, n, t_min=t_min, t_max=t_max)
    rgba, depth = rgba.reshape(n, 4), depth.reshape(n)
    assert np.all(rgba[picks, :3] == np.float32(bgc)) and np.all(rgba[picks, 3] == 0) and np.all(depth[picks] == 0)
    others = np.setdiff1d(np.arange(n), picks)
    assert np.array_equal(clip._bits(rgba[others]), clip._bits(full[0].reshape(n, 4)[others]))
    assert np.array_equal(clip._bits(depth[others]), clip._bits(full[1].reshape(n)[others]))
    assert st.n_composited < full[2].n_composited
    ctx.close()


# ---------------------------------------------------------------- f. metric depth, 8-bit outputs, views
@pytest.mark.parametrize("kind", ["t_max", "t_min"])
@pytest.mark.parametrize("row,sched", rf.hot_cases(["h48-b3-c3", "h30-b4-c3"]))
def test_metric_depth(row, sched, kind):
    desc, o, d, full, t, (want, wdepth, n_chk, raw), (near, far) = rf.checked(row, kind)
    n = RW * RH
    ctx = _open(row, sched, RW, RH)
    do, dd = clip._upload(o), clip._upload(d)
    rgba, dn, _ = clip._clipped(ctx, do, dd, n, **{kind: t})
    rgba_t, D, _ = clip._clipped(ctx, do, dd, n, flags=nh.NRF_RAYS_DEPTH_T, **{kind: t})
    ctx.close()
    assert np.array_equal(clip._bits(rgba_t), clip._bits(rgba))
    D, dn = D.reshape(n), dn.reshape(n)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        span = (far - near).astype(np.float32)
        num = np.maximum((D - near).astype(np.float32), np.float32(0))
        norm = np.where(span > 0, num / np.where(span > 0, span, np.float32(1)), np.float32(0)).astype(np.float32)
    assert np.array_equal(clip._bits(dn), clip._bits(norm))
    ok = span > 0
    err = np.abs(D[ok] - raw[ok])
    print(f"{row} {sched} {kind}: max |D - checker| / span {float(np.max(err / span[ok])):.3e}, rays with samples {int(np.sum(D > 0))}")
    assert np.all(err <= clip.TOL * span[ok])
    assert np.all(D[~ok] == 0) and np.sum(D > 0) > 0.1 * n


def _limits_and_backgrounds(W, H):
    """Two views' limits (the ramp, and the ramp falling) and backgrounds (two gradients), as tests/test_render_rays_clip_gpu.py's"""
    n = W * H
    t = rco.ramp(W, H)
    lims = [t, (np.float32(1.6) - (t - np.float32(0.7))).astype(np.float32)]
    yy, xx = np.divmod(np.arange(n), W)
    bgs = [np.stack([xx / W, yy / H, np.full(n, 0.5)], axis=1).astype(np.float32),
           np.stack([np.full(n, 0.25), xx / W, yy / H], axis=1).astype(np.float32)]
    return lims, bgs


@pytest.mark.parametrize("model", [POW2_SMALL, "h64-b1.5-c2"])
def test_persistent_8bit_outputs_are_the_quantized_float_frame(model):
    """The persistent POW2 and GENERIC instances compiled for 8-bit planes (bind_output_u8), and the packed output of the float ones."""
    W, H = 100, 52
    n = W * H
    if model == POW2_SMALL:
        assert rf.march_form(32, 3, 4.0) == (rf.POW2, 1)
        ctx = clip._context(models.build_model(log2_hashmap_size=12, H=32, **clip.SMALL[model])[0], W, H, rf.PERSISTENT)
        assert clip._rays_instance(ctx) == 16
    else:
        ctx = _open(model, "persistent", W, H)
    o, d = clip._device_rays(ctx, W, H)
    lims, bgs = _limits_and_backgrounds(W, H)
    tm, bg = clip._upload(lims[0]), clip._upload(bgs[0])
    single = clip._clipped(ctx, o, d, n, t_max=tm, bg=bg)
    a = single[0][..., 3]
    assert np.mean(a > 0.5) > 0.02 and np.mean((a > 0.05) & (a < 0.95)) > 0.02
    frgba, fdepth = clip._upload(single[0]), clip._upload(single[1])
    packed, wpacked = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    rgb8, d8 = torch.zeros((n, 3), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    wrgb8, wd8 = torch.zeros((n, 3), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.quantize_rgbd8(frgba.data_ptr(), fdepth.data_ptr(), n, wpacked.data_ptr())
    ctx.quantize_u8(frgba.data_ptr(), fdepth.data_ptr(), n, wrgb8.data_ptr(), wd8.data_ptr())
    ctx.bind_output_rgbd8(packed.data_ptr())
    ctx.render_rays_clipped(o.data_ptr(), d.data_ptr(), n, 0, tm.data_ptr(), bg.data_ptr())
    ctx.bind_output_rgbd8(None)
    ctx.bind_output_u8(rgb8.data_ptr(), d8.data_ptr())
    ctx.render_rays_clipped(o.data_ptr(), d.data_ptr(), n, 0, tm.data_ptr(), bg.data_ptr())
    ctx.bind_output_u8(None, None)
    torch.cuda.synchronize()
    assert torch.equal(packed, wpacked) and int((wpacked != 0).sum()) > 0
    assert torch.equal(rgb8, wrgb8) and torch.equal(d8, wd8)
    assert int((wrgb8 != 0).sum()) > 0 and int((wd8 != 0).sum()) > 0
    ctx.close()


@pytest.mark.parametrize("sched", list(rf.SCHED))
def test_two_views_with_a_ramp_each_are_two_single_calls(sched):
    row = "h64-b1.5-c2"
    W, H = 100, 52
    n = W * H
    ctx = _open(row, sched, W, H)
    views = [clip._device_rays(ctx, W, H, az, el) for az, el in ((30, 30), (150, 10))]
    lims, bgs = _limits_and_backgrounds(W, H)
    singles = [clip._clipped(ctx, views[v][0], views[v][1], n, t_max=lims[v], bg=bgs[v])[:2] for v in range(2)]
    assert not np.array_equal(singles[0][0], singles[1][0])
    assert all(np.mean(s[0][..., 3] > 0.5) > 0.02 for s in singles)
    o2 = torch.cat([r[0] for r in views]).contiguous()
    d2 = torch.cat([r[1] for r in views]).contiguous()
    t2, bg2 = clip._upload(np.concatenate(lims)), clip._upload(np.concatenate(bgs))
    ctx.set_max_views(2)
    f = ctx.render_rays_clipped(o2.data_ptr(), d2.data_ptr(), n, 0, t2.data_ptr(), bg2.data_ptr(), n_views=2)
    assert f.n_views == 2
    for v in range(2):
        clip._same(ctx.read_view_f32(v), singles[v], (sched, "view", v))
    ctx.close()


# ---------------------------------------------------------------- g. rays a pinhole cannot describe
G_CASES = rf.hot_cases(["h64-b1.5-c2", "h48-b3-c3", "h30-b4-c3"])


@pytest.mark.parametrize("row,sched", G_CASES)
def test_orthographic_rays_match_the_assembled_oracle(row, sched):
    W, H = RW, RH
    o, d = ro.orthographic(W, H, half_extent=1.2)
    assert len(np.unique(o, axis=0)) == W * H and len(np.unique(d, axis=0)) == 1
    ctx = _open(row, sched, W, H)
    rays._check_against_oracle(ctx, rf.build(row)[0], o, d, W, H, 0.05, ("orthographic", row, sched))
    ctx.close()


@pytest.mark.parametrize("scale", [1.0, 1.25])
@pytest.mark.parametrize("row,sched", G_CASES)
def test_equirectangular_rays_match_the_assembled_oracle(row, sched, scale):
    """A panorama from the orbit camera's position (inside the box: every ray starts at min_near, in the innermost cube), and from
    1.25 times that position: outside the innermost cube, inside the next cascade, so that the walk over cube 0 starts ahead of
    the ray's origin."""
    W, H = RW, RH
    desc = rf.build(row)[0]
    origin = (rf.scene(row)[3][0] * np.float32(scale)).astype(np.float32)
    far = np.max(np.abs(origin))
    assert (far < 1.0) if scale == 1.0 else (1.0 < far < min(2.0, desc.bound))
    o, d = ro.equirectangular(W, H, origin)
    ctx = _open(row, sched, W, H)
    rays._check_against_oracle(ctx, desc, o, d, W, H, 0.0, ("equirectangular", row, sched, scale))
    ctx.close()
