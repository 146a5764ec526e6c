"""nrf_render_rays_clipped on the GPU: caller-supplied rays between per-ray limits of t, over a per-ray background.

  * limits that limit nothing (no arrays, 0 / FLT_MAX, -inf / +inf, NaN) and a background array that repeats bg_color change no
    bit of the nrf_render_rays frame -- persistent and per-strip RAYS instances of the hot shape, the wide and generic per-strip ones;
  * the ramp t(px) = 0.7 + 0.9 px / W as t_max and as t_min against the checker (tests/rays_clip_oracle.py), at the tolerances
    tests/test_render_rays_gpu.py uses for oracle frames;
  * exact properties on the GPU alone: rays without a limit do not see their neighbours' limits, alpha grows with t_max, empty
    intervals are exactly background, and the frame does not depend on the schedule (tail splitting, fast-forward, march budget,
    persistent against per-strip);
  * the per-ray background and the metric depth plane (NRF_RAYS_DEPTH_T) bit for bit; views, shards, 8-bit outputs; refusals.
Every test here needs the entry point: none passes without it."""
import ctypes as C
import os

import numpy as np
import pytest

import models
import nerfhip as nh
import oracle_py as op
import rays_clip_oracle as rco
import rays_oracle as ro
import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STRIP = {"NRF_PERSISTENT": "0"}
PERSISTENT = {"NRF_PERSISTENT": "1"}
SCHED = {"persistent": PERSISTENT, "strip": STRIP}
SMALL = {"bound1": dict(), "bound4-cascade3": dict(bound=4.0, cascade=3)}
WIDE = {"wide-frequency12": dict(dir_otype="Frequency", n_frequencies=12)}
FLT_MAX = float(ro.FLT_MAX)
TOL = np.float32(2.0 / 255.0)


def _context(desc, W, H, env=None, **opts_kw):
    """A context with the environment `env` in force at its creation (the NRF_* switches are read by nrf_create)."""
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = nh.NerfHip(0)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    ctx.load_model(desc)
    _options(ctx, **opts_kw)
    ctx.set_resolution(W, H)
    return ctx


def _options(ctx, **opts_kw):
    o = nh.default_options()
    for k, v in opts_kw.items():
        setattr(o, k, v)
    ctx.set_options(o)


def _rays_instance(ctx):
    fn = ctx.lib.nrf_debug_rays_instance
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    return int(fn(ctx.h))


def _device_rays(ctx, W, H, az=30, el=30):
    o = torch.empty((H * W, 3), device="cuda")
    d = torch.empty((H * W, 3), device="cuda")
    torch.cuda.synchronize()
    ctx.generate_rays(syn.default_camera(W, H), syn.orbit_pose(az, el), o.data_ptr(), d.data_ptr(), 0, 0)
    return o, d


def _upload(a):
    t = torch.from_numpy(np.array(a, np.float32)).cuda()  # (a copy: the shared checker arrays are read-only)
    torch.cuda.synchronize()
    return t


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    assert np.array_equal(_bits(got[0]), _bits(want[0])), what
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what


def _clipped(ctx, o, d, n, t_min=None, t_max=None, bg=None, flags=0, **kw):
    """One nrf_render_rays_clipped call with host (numpy) or device arrays for the limits: (rgba [H][W][4], depth [H][W], stats)."""
    keep = [a if (a is None or torch.is_tensor(a)) else _upload(a) for a in (t_min, t_max, bg)]
    ctx.render_rays_clipped(o.data_ptr(), d.data_ptr(), n, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), flags, **kw)
    rgba, depth = ctx.read_f32()
    return rgba, depth, ctx.stats()


# ---------------------------------------------------------------- 1. limits that limit nothing
def _no_limit_changes_no_bit(desc, env, W, H, what):
    bgc = 0.25
    ctx = _context(desc, W, H, env, bg_color=bgc)
    o, d = _device_rays(ctx, W, H)
    n = W * H
    ctx.render_rays(o.data_ptr(), d.data_ptr(), n)
    want = ctx.read_f32()
    wst = ctx.stats()
    assert wst.n_composited > 0 and np.mean(want[0][..., 3] > 0.5) > 0.02, what
    bg = np.full((n, 3), bgc, np.float32)
    inf, nan = np.full(n, np.inf, np.float32), np.full(n, np.nan, np.float32)
    cases = {"all NULL": dict(),
             "background alone": dict(bg=bg),
             "0 / FLT_MAX": dict(t_min=np.zeros(n, np.float32), t_max=np.full(n, FLT_MAX, np.float32), bg=bg),
             "-inf / +inf": dict(t_min=-inf, t_max=inf, bg=bg),
             "NaN": dict(t_min=nan, t_max=nan, bg=bg)}
    for name, kw in cases.items():
        rgba, depth, st = _clipped(ctx, o, d, n, **kw)
        _same((rgba, depth), want, (what, name))
        assert st.n_composited == wst.n_composited and st.n_rays == wst.n_rays, (what, name)
    ctx.close()


@pytest.mark.parametrize("W,H", [(64, 64), (33, 70)])
@pytest.mark.parametrize("sched", list(SCHED))
@pytest.mark.parametrize("model", list(SMALL))
def test_no_limit_changes_no_bit(model, sched, W, H):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **SMALL[model])
    _no_limit_changes_no_bit(desc, SCHED[sched], W, H, (model, sched, W, H))


@pytest.mark.parametrize("name,kw,code", [("wide-frequency12", dict(dir_otype="Frequency", n_frequencies=12), 2),
                                          ("generic-sine", dict(activation="Sine"), 1)])
def test_no_limit_changes_no_bit_in_the_wide_and_generic_instances(name, kw, code):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **kw)
    ctx = _context(desc, 100, 52)
    assert _rays_instance(ctx) == code, name
    ctx.close()
    _no_limit_changes_no_bit(desc, None, 100, 52, name)


# ---------------------------------------------------------------- 2. the ramp against the checker
RW, RH = 64, 48
_checked = {}


def _checker(model, kind, opts_kw=None):
    """The checker's frame of the ramp scene, computed once per (model, limit, options) and shared: desc, rays, the limit, rgba,
    depth, samples, raw depth, (near', far'), and the unlimited checker frame.  opts_kw: nrf_options fields other than the defaults
    (the rays of a camera do not depend on them)."""
    tag = tuple(sorted((opts_kw or {}).items()))
    opts = nh.default_options()
    for k, v in (opts_kw or {}).items():
        setattr(opts, k, v)
    if ("desc", model) not in _checked:
        desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **{**SMALL, **WIDE}[model])
        orc = op.Oracle(desc)
        o, d, _, _ = orc.generate_rays(syn.default_camera(RW, RH), syn.orbit_pose(30, 30), RW, RH)
        _checked[("desc", model)] = (desc, keep, orc, o, d)
    desc, keep, orc, o, d = _checked[("desc", model)]
    if ("full", model, tag) not in _checked:
        _checked[("full", model, tag)] = ro.render(orc, desc, o, d, opts)
    full = _checked[("full", model, tag)]
    if (model, kind, tag) not in _checked:
        t = rco.ramp(RW, RH)
        lim = {kind: t}
        res = rco.render(orc, desc, o, d, opts, **lim)
        nf = rco.near_far(desc, o, d, opts.min_near, **lim)
        for a in (*res[:2], res[3], *nf, t):
            a.setflags(write=False)
        _checked[(model, kind, tag)] = (t, res, nf)
    return (desc, o, d, full) + _checked[(model, kind, tag)]


@pytest.mark.parametrize("kind", ["t_max", "t_min"])
@pytest.mark.parametrize("sched", list(SCHED))
@pytest.mark.parametrize("model", list(SMALL))
def test_the_ramp_matches_the_checker(model, sched, kind):
    _ramp_matches_the_checker(model, sched, kind)


def _ramp_matches_the_checker(model, sched, kind, opts_kw=None):
    """opts_kw: nrf_options fields the context renders under and the checker is computed with (None: the defaults)"""
    desc, o, d, full, t, (want, wdepth, n, raw), (near, far) = _checker(model, kind, opts_kw)
    W, H = RW, RH
    ctx = _context(desc, W, H, SCHED[sched], **(opts_kw or {}))
    assert _rays_instance(ctx) == (16 if sched == "persistent" else 0)
    do, dd = _upload(o), _upload(d)
    rgba, depth, st = _clipped(ctx, do, dd, W * H, **{kind: t})
    ctx.close()
    rgba, depth = rgba.reshape(-1, 4), depth.reshape(-1)
    e_rgba, e_depth, psnr = float(np.abs(rgba - want).max()), float(np.abs(depth - wdepth).max()), models.psnr(rgba, want)
    print(f"{model} {sched} {kind}: max|d rgba| {e_rgba:.3e} max|d depth| {e_depth:.3e} psnr {psnr:.1f} dB composited {st.n_composited} "
          f"(checker {n})")
    assert np.all(np.isfinite(rgba)) and np.all(np.isfinite(depth))
    assert e_rgba <= 2.0 / 255.0 and e_depth <= 2.0 / 255.0
    assert psnr >= 45.0
    assert abs(int(st.n_composited) - n) <= 0.002 * n + 8, (st.n_composited, n)
    # pixels the checker cuts fully: exactly the background (bg_color, the default options'), alpha 0, depth 0
    cut = (want[:, 3] == 0) & (full[0][:, 3] > 0.5)
    if kind == "t_max":
        assert np.mean(cut) >= 0.2
    bg = np.float32(nh.default_options().bg_color)
    assert np.all(rgba[cut, :3] == bg) and np.all(rgba[cut, 3] == 0) and np.all(depth[cut] == 0)
    empty = ~(near < far)
    assert np.all(rgba[empty, :3] == bg) and np.all(rgba[empty, 3] == 0) and np.all(depth[empty] == 0)


def test_the_ramp_cuts_rays_in_the_wide_instance():
    """The wide per-strip instance (three waves per SIMD, a kernel of its own) with a limit that limits: the ramp as t_max against
    the checker, at the tolerances of the hot instances above -- the project's for oracle frames, the model differs only in its
    direction encoding -- and, first, on the checker alone, that the ramp cuts this model's frame partly and fully."""
    model = "wide-frequency12"
    desc, o, d, full, t, (want, wdepth, n, raw), (near, far) = _checker(model, "t_max")
    W, H = RW, RH
    partly = (want[:, 3] > 0.05) & (want[:, 3] < full[0][:, 3] - 0.05)
    cut = (want[:, 3] == 0) & (full[0][:, 3] > 0.5)
    print(f"{model}: partly cut {np.mean(partly):.3f} fully cut {np.mean(cut):.3f}")
    assert np.mean(partly) >= 0.04 and np.mean(cut) >= 0.2
    ctx = _context(desc, W, H)
    assert _rays_instance(ctx) == 2
    rgba, depth, st = _clipped(ctx, _upload(o), _upload(d), W * H, t_max=t)
    ctx.close()
    rgba, depth = rgba.reshape(-1, 4), depth.reshape(-1)
    e_rgba, e_depth, psnr = float(np.abs(rgba - want).max()), float(np.abs(depth - wdepth).max()), models.psnr(rgba, want)
    print(f"{model}: max|d rgba| {e_rgba:.3e} max|d depth| {e_depth:.3e} psnr {psnr:.1f} dB composited {st.n_composited} (checker {n})")
    assert np.all(np.isfinite(rgba)) and np.all(np.isfinite(depth))
    assert e_rgba <= 2.0 / 255.0 and e_depth <= 2.0 / 255.0 and psnr >= 45.0
    assert abs(int(st.n_composited) - n) <= 0.002 * n + 8, (st.n_composited, n)
    bg = np.float32(nh.default_options().bg_color)
    assert np.all(rgba[cut, :3] == bg) and np.all(rgba[cut, 3] == 0) and np.all(depth[cut] == 0)


# ---------------------------------------------------------------- 3. exact properties on the GPU alone
@pytest.mark.parametrize("W,H", [(64, 48), (100, 52)])
@pytest.mark.parametrize("sched", list(SCHED))
def test_independence_monotonicity_and_empty_intervals(sched, W, H):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    bgc = 0.25
    ctx = _context(desc, W, H, SCHED[sched], bg_color=bgc)
    o, d = _device_rays(ctx, W, H)
    n = W * H
    full = _clipped(ctx, o, d, n)
    t = rco.ramp(W, H)
    ramp = _clipped(ctx, o, d, n, t_max=t)
    a_full, a_ramp = full[0][..., 3].reshape(-1), ramp[0][..., 3].reshape(-1)
    assert np.mean((a_ramp > 0.05) & (a_ramp < a_full - 0.05)) >= 0.02  # (the ramp does cut rays in the middle of the object)

    # independence: a fixed pseudo-random half of the pixels is limited, the other half renders the unlimited frame's bits
    limited = np.random.default_rng(20240607).random(n) < 0.5
    tiles = limited.reshape(H, W)[:H // 8 * 8, :W // 8 * 8].reshape(H // 8, 8, W // 8, 8).mean(axis=(1, 3))
    assert tiles.min() > 0.2 and tiles.max() < 0.8  # every 8x8 tile mixes both kinds: rounds and tail splitting see both
    half = _clipped(ctx, o, d, n, t_max=np.where(limited, t, np.float32(np.nan)).astype(np.float32))
    for plane in (0, 1):
        got, free, cutf = (x[plane].reshape(n, -1) for x in (half, full, ramp))
        assert np.array_equal(_bits(got[~limited]), _bits(free[~limited])), ("unlimited half", plane)
        assert np.array_equal(_bits(got[limited]), _bits(cutf[limited])), ("limited half", plane)
    assert np.any(a_full[~limited] > 0.5) and np.any(a_ramp[limited] < a_full[limited])

    # monotonicity: the weight sum only ever adds non-negative weights
    wider = _clipped(ctx, o, d, n, t_max=(t + np.float32(0.15)).astype(np.float32))
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
    rgba, depth, st = _clipped(ctx, o, d, n, t_min=t_min, t_max=t_max)
    rgba, depth = rgba.reshape(n, 4), depth.reshape(n)
    assert np.all(rgba[picks, :3] == np.float32(bgc)) and np.all(rgba[picks, 3] == 0) and np.all(depth[picks] == 0)
    others = np.setdiff1d(np.arange(n), picks)
    assert np.array_equal(_bits(rgba[others]), _bits(full[0].reshape(n, 4)[others]))
    assert np.array_equal(_bits(depth[others]), _bits(full[1].reshape(n)[others]))
    assert st.n_composited < full[2].n_composited
    ctx.close()


@pytest.mark.parametrize("W,H", [(64, 48), (100, 52)])
def test_the_clipped_frame_does_not_depend_on_the_schedule(W, H):
    """Tail splitting off, the barrier fast-forward off, three cell trips per round, and the per-strip kernel instead of the
    persistent one: the same bits.  (Persistent against per-strip holds for the unclipped rays frame of the parent as well.)"""
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    n = W * H
    t = rco.ramp(W, H)
    frames = {}
    for name, env in (("persistent", PERSISTENT), ("tail split off", dict(PERSISTENT, NRF_TAIL_SPLIT="0")),
                      ("fast-forward off", dict(PERSISTENT, NRF_MARCH_FF="0")), ("budget 3", dict(PERSISTENT, NRF_MARCH_BUDGET="3")),
                      ("strip", STRIP), ("strip, fast-forward off", dict(STRIP, NRF_MARCH_FF="0")),
                      ("strip, budget 3", dict(STRIP, NRF_MARCH_BUDGET="3"))):
        ctx = _context(desc, W, H, env)
        assert _rays_instance(ctx) == (0 if "strip" in name else 16), name
        o, d = _device_rays(ctx, W, H)
        frames[name] = [_clipped(ctx, o, d, n, t_max=t)[:2], _clipped(ctx, o, d, n, t_min=t, t_max=(t + np.float32(0.4)).astype(np.float32))[:2]]
        ctx.close()
    want = frames["persistent"]
    assert np.mean(want[0][0][..., 3] > 0.5) > 0.02 and np.mean(want[1][0][..., 3] > 0.05) > 0.02
    for name, got in frames.items():
        _same(got[0], want[0], (name, "t_max"))
        _same(got[1], want[1], (name, "t_min and t_max"))


# ---------------------------------------------------------------- 4. the per-ray background
@pytest.mark.parametrize("sched", list(SCHED))
def test_per_ray_background_bit_for_bit(sched):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W, H = 100, 52
    n = W * H
    ctx = _context(desc, W, H, SCHED[sched], bg_color=0.0)
    o, d = _device_rays(ctx, W, H)
    t = rco.ramp(W, H)
    black, bdepth, _ = _clipped(ctx, o, d, n, t_max=t)  # bg_color 0: c and the weight sum exactly
    black = black.reshape(n, 4)
    c, ws = black[:, :3], black[:, 3]
    assert np.mean((ws > 0.05) & (ws < 0.95)) > 0.02
    # a checkerboard of two colours, every channel different
    yy, xx = np.divmod(np.arange(n), W)
    board = ((xx // 4 + yy // 4) & 1).astype(bool)
    bg = np.where(board[:, None], np.float32([0.9, 0.35, 0.1]), np.float32([0.05, 0.6, 1.0])).astype(np.float32)
    scalar = 0.625
    _options(ctx, bg_color=scalar)

    def expect(c, ws, bg):
        T = (np.float32(1) - ws).astype(np.float32)
        return (c + (T[:, None] * bg).astype(np.float32)).astype(np.float32)

    rgba, depth, _ = _clipped(ctx, o, d, n, t_max=t, bg=bg)
    rgba = rgba.reshape(n, 4)
    assert np.array_equal(_bits(rgba[:, :3]), _bits(expect(c, ws, bg)))
    assert np.array_equal(_bits(rgba[:, 3]), _bits(ws)) and np.array_equal(_bits(depth), _bits(bdepth))
    # guarded rays show their own entry; pixels beyond a short list show the scalar
    m = 31 * W + 7
    on = np.flatnonzero(ws[:m] > 0.5)
    picks = on[[len(on) // 3, 2 * len(on) // 3]]
    oh, dh = o.cpu().numpy().copy(), d.cpu().numpy().copy()
    oh[picks[0], 1] = np.nan
    dh[picks[1]] *= 2.5  # |d|^2 = 6.25
    assert picks[0] != picks[1] and np.any(ws[m:] > 0.5)
    o2, d2 = _upload(oh), _upload(dh)
    rgba, depth, _ = _clipped(ctx, o2, d2, m, t_max=t[:m].copy(), bg=bg[:m].copy())
    rgba, depth = rgba.reshape(n, 4), depth.reshape(n)
    want = np.concatenate([expect(c, ws, bg), ws[:, None]], axis=1)
    want[picks] = np.concatenate([bg[picks], np.zeros((2, 1), np.float32)], axis=1)
    wdepth = bdepth.reshape(n).copy()
    wdepth[picks] = 0
    listed = np.arange(n) < m
    assert np.array_equal(_bits(rgba[listed]), _bits(want[listed])) and np.array_equal(_bits(depth[listed]), _bits(wdepth[listed]))
    assert np.all(rgba[~listed, :3] == np.float32(scalar)) and np.all(rgba[~listed, 3] == 0) and np.all(depth[~listed] == 0)
    ctx.close()


# ---------------------------------------------------------------- 5. metric depth
@pytest.mark.parametrize("kind", ["t_max", "t_min"])
@pytest.mark.parametrize("sched", list(SCHED))
@pytest.mark.parametrize("model", list(SMALL))
def test_metric_depth(model, sched, kind):
    desc, o, d, full, t, (want, wdepth, n_chk, raw), (near, far) = _checker(model, kind)
    W, H = RW, RH
    n = W * H
    ctx = _context(desc, W, H, SCHED[sched])
    do, dd = _upload(o), _upload(d)
    rgba, dn, _ = _clipped(ctx, do, dd, n, **{kind: t})
    rgba_t, D, _ = _clipped(ctx, do, dd, n, flags=nh.NRF_RAYS_DEPTH_T, **{kind: t})
    assert np.array_equal(_bits(rgba_t), _bits(rgba))
    D, dn = D.reshape(n), dn.reshape(n)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        span = (far - near).astype(np.float32)
        num = np.maximum((D - near).astype(np.float32), np.float32(0))
        norm = np.where(span > 0, num / np.where(span > 0, span, np.float32(1)), np.float32(0)).astype(np.float32)
    assert np.array_equal(_bits(dn), _bits(norm))
    ok = span > 0
    err = np.abs(D[ok] - raw[ok])
    print(f"{model} {sched} {kind}: max |D - checker| / span {float(np.max(err / span[ok])):.3e}, rays with samples {int(np.sum(D > 0))}")
    assert np.all(err <= TOL * span[ok])
    assert np.all(D[~ok] == 0) and np.sum(D > 0) > 0.1 * n
    ctx.close()


def test_metric_depth_needs_a_float_depth_plane():
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W, H = 64, 48
    n = W * H
    ctx = _context(desc, W, H)
    o, d = _device_rays(ctx, W, H)
    packed = torch.zeros(n, dtype=torch.int32, device="cuda")
    rgb8, d8 = torch.zeros((n, 3), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for bind, unbind in ((lambda: ctx.bind_output_rgbd8(packed.data_ptr()), lambda: ctx.bind_output_rgbd8(None)),
                         (lambda: ctx.bind_output_u8(rgb8.data_ptr(), d8.data_ptr()), lambda: ctx.bind_output_u8(None, None))):
        bind()
        with pytest.raises(nh.NerfHipError) as e:
            ctx.render_rays_clipped(o.data_ptr(), d.data_ptr(), n, flags=nh.NRF_RAYS_DEPTH_T)
        assert e.value.code == nh.NRF_E_UNSUPPORTED
        ctx.render_rays_clipped(o.data_ptr(), d.data_ptr(), n)  # (without the flag the bound output renders)
        unbind()
    torch.cuda.synchronize()
    assert int((packed != 0).sum()) > 0 and int((rgb8 != 0).sum()) > 0
    rgba, D, st = _clipped(ctx, o, d, n, flags=nh.NRF_RAYS_DEPTH_T)  # ... and the context still renders
    assert st.n_composited > 0 and np.all(np.isfinite(D)) and np.any(D > 0)
    ctx.close()


# ---------------------------------------------------------------- 6. views, shards, 8-bit outputs
@pytest.mark.parametrize("sched", list(SCHED))
def test_views_shards_and_8bit_outputs(sched):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W, H = 100, 52
    n = W * H
    env = SCHED[sched]
    ctx = _context(desc, W, H, env)
    rays = [_device_rays(ctx, W, H, az, el) for az, el in ((30, 30), (150, 10))]
    t = rco.ramp(W, H)
    lims = [t, (np.float32(1.6) - (t - np.float32(0.7))).astype(np.float32)]  # the ramp, and the ramp falling
    yy, xx = np.divmod(np.arange(n), W)
    bgs = [np.stack([xx / W, yy / H, np.full(n, 0.5)], axis=1).astype(np.float32),
           np.stack([np.full(n, 0.25), xx / W, yy / H], axis=1).astype(np.float32)]
    singles = [_clipped(ctx, rays[v][0], rays[v][1], n, t_max=lims[v], bg=bgs[v])[:2] for v in range(2)]
    assert not np.array_equal(singles[0][0], singles[1][0])
    # n_views = 2 with a ramp of its own per view == two single calls
    o2 = torch.cat([r[0] for r in rays]).contiguous()
    d2 = torch.cat([r[1] for r in rays]).contiguous()
    t2, bg2 = _upload(np.concatenate(lims)), _upload(np.concatenate(bgs))
    ctx.set_max_views(2)
    f = ctx.render_rays_clipped(o2.data_ptr(), d2.data_ptr(), n, 0, t2.data_ptr(), bg2.data_ptr(), n_views=2)
    assert f.n_views == 2
    for v in range(2):
        _same(ctx.read_view_f32(v), singles[v], ("view", v))
    ctx.set_max_views(1)
    # bound 8-bit outputs == nrf_quantize_* of the float frame
    o, d = rays[0]
    tm, bg = _upload(lims[0]), _upload(bgs[0])
    frgba, fdepth = _upload(singles[0][0]), _upload(singles[0][1])
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
    ctx.close()
    # shard_count = 2 on one device + nrf_untile == the unsharded frame: both ranks are given the same arrays
    tps = nh.tiles_per_shard(W, H, 2)
    gathered = torch.zeros((2, tps * 64, 4), device="cuda")
    gdepth = torch.zeros((2, tps * 64, 1), device="cuda")
    torch.cuda.synchronize()
    for idx in range(2):
        c2 = _context(desc, W, H, env, shard_index=idx, shard_count=2)
        c2.bind_output(gathered[idx].data_ptr(), gdepth[idx].data_ptr())
        f = c2.render_rays_clipped(o.data_ptr(), d.data_ptr(), n, 0, tm.data_ptr(), bg.data_ptr())
        assert f.tile_major == 1
        c2.close()
    c1 = _context(desc, W, H, env)
    out, outd = torch.empty((H, W, 4), device="cuda"), torch.empty((H, W, 1), device="cuda")
    torch.cuda.synchronize()
    c1.untile(gathered.data_ptr(), 2, tps, 4, out.data_ptr())
    c1.untile(gdepth.data_ptr(), 2, tps, 1, outd.data_ptr())
    _same((out.cpu().numpy(), outd.cpu().numpy()[..., 0]), singles[0], "two shards")
    c1.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W, H = 64, 48
    buf = torch.zeros((W * H, 3), device="cuda")
    buf[:, 2] = 1.0
    torch.cuda.synchronize()
    p = buf.data_ptr()

    def code(fn):
        with pytest.raises(nh.NerfHipError) as e:
            fn()
        return e.value.code

    def raw(ctx, rays):
        """The entry point itself: a nrf_rays the mirror's method would not build (None: a null struct)."""
        rc = ctx.lib.nrf_render_rays_clipped(ctx.h, 1, None if rays is None else C.byref(rays), None, None)
        return int(rc)

    ctx = nh.NerfHip(0)
    assert code(lambda: ctx.render_rays_clipped(p, p, 16)) == nh.NRF_E_STATE            # no model
    ctx.load_model(desc)
    assert code(lambda: ctx.render_rays_clipped(p, p, 16)) == nh.NRF_E_STATE            # no resolution
    ctx.set_resolution(W, H)
    assert raw(ctx, None) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays_clipped(0, p, 16)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays_clipped(p, 0, 16)) == nh.NRF_E_INVALID
    assert raw(ctx, nh.Rays(p, p, 16, None, None, None, 0, 1)) == nh.NRF_E_INVALID       # reserved != 0
    assert code(lambda: ctx.render_rays_clipped(p, p, 16, flags=2)) == nh.NRF_E_INVALID  # unknown flag bits
    assert code(lambda: ctx.render_rays_clipped(p, p, 16, flags=nh.NRF_RAYS_DEPTH_T | 0x80000000)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays_clipped(p, p, W * H + 1)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays_clipped(p, p, 0)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays_clipped(p, p, 16, n_views=0)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays_clipped(p, p, 16, n_views=2)) == nh.NRF_E_STATE  # more views than the context's buffers hold
    o = nh.default_options()
    o.perturb = 7
    ctx.set_options(o)
    assert code(lambda: ctx.render_rays_clipped(p, p, W * H)) == nh.NRF_E_UNSUPPORTED
    ctx.set_options(nh.default_options())
    assert raw(ctx, nh.Rays(p, p, W * H, None, None, None, 0, 0)) == nh.NRF_OK            # ... and the context still renders
    rgba, depth = ctx.read_f32()
    assert np.all(np.isfinite(rgba)) and np.all(np.isfinite(depth))
    ctx.close()
