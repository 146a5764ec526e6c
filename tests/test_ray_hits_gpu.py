"""nrf_ray_hits on the GPU: where a caller's ray reaches an opacity threshold.

The definition is in terms of the density-only call (nrf_render_rays_clipped with NRF_RAYS_DENSITY_ONLY | NRF_RAYS_DEPTH_T), so the
exact tests render both on one context, without a tolerance:
  (A) the density-only call with t_max = rgba[0] on hit rays ends every hit ray WITH its crossing sample: its alpha plane is
      rgba[3], its depth plane the hit depth, n_composited and n_rays are equal;
  (B) with t_max = fp32(rgba[0] - rgba[1]) lowered by 4 ulps it ends BEFORE that sample: alpha on hit rays is rgba[2], < opacity
      (the march emits a sample when its start t_s < far and composites it at fp32(t_s + dt); fp32(tc - dt) is within about an ulp
      of t_s, and dt >= 0.0034 is far larger than 4 ulps);
  a miss carries the unclipped density-only alpha and depth bits and zeros in rgba[0..2]; a pixel without a ray, a refused ray and
  an empty interval are all zero.
Then: limits of the call's own (the ramp of rays_clip_oracle), monotonicity in the threshold, schedule independence (which shows
that the threshold's sample queue changes no pixel), the checker (tests/ray_hits_oracle.py) at opacity 0.5, views and shards, the
refusals, and the C++ mirror.  Every test here needs the entry point: none passes without it."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import models
import nerfhip as nh
import rays_clip_oracle as rco
import rays_forms as rf
import ray_hits_oracle as rho
import test_render_rays_clip_gpu as clip
from test_render_rays_clip_gpu import _bits, _clipped, _context, _device_rays, _options, _ptr, _upload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
DENS_T = nh.NRF_RAYS_DENSITY_ONLY | nh.NRF_RAYS_DEPTH_T
OPACITIES = [0.5, 0.9, 0.99]
INF = np.float32(np.inf)
TOL = np.float32(2.0 / 255.0)  # the project's frame tolerance (clip.TOL)


def _framed_rays(ctx, W, H, az=30, el=30):
    """The orbit camera's rays with the field of view applied to the geometric mean of the frame's sides (synthetic.default_camera
    applies it to the shorter one): at 33 x 70 and 100 x 52 the object then covers more than the 40 % of the pixels that the hit
    share is held to -- on the CPU oracle 0.65 at 64 x 64, where nothing changes, against 0.35 and 0.38 with the default camera."""
    import synthetic as syn
    cam = syn.default_camera(W, H)
    cam[:2] *= np.float32(np.sqrt(max(W, H) / min(W, H)))
    o = torch.empty((H * W, 3), device="cuda")
    d = torch.empty((H * W, 3), device="cuda")
    torch.cuda.synchronize()
    ctx.generate_rays(cam, syn.orbit_pose(az, el), o.data_ptr(), d.data_ptr(), 0, 0)
    return o, d


def _hits(ctx, o, d, n, opacity, t_min=None, t_max=None, **kw):
    """One nrf_ray_hits call with host (numpy) or device arrays for the limits: (records [H][W][4], depth [H][W], stats)"""
    keep = [a if (a is None or torch.is_tensor(a)) else _upload(a) for a in (t_min, t_max)]
    ctx.ray_hits(o.data_ptr(), d.data_ptr(), n, opacity, _ptr(keep[0]), _ptr(keep[1]), **kw)
    rgba, depth = ctx.read_f32()
    return rgba, depth, ctx.stats()


def _check_against_density_only(ctx, o, d, n, opacity, what, t_min=None, t_max=None, share=None):
    """The exact test of one call: n rays in a context of W x H >= n pixels.  Returns (records [px][4], depth [px], stats, the
    density-only frame under the call's own limits)."""
    p = np.float32(opacity)
    rgba, depth, st = _hits(ctx, o, d, n, opacity, t_min, t_max)
    rec, dep = rgba.reshape(-1, 4), depth.reshape(-1)
    hit = rec[:, 3] >= p
    print(f"{what} at {opacity}: hit share {np.mean(hit):.3f}, composited {st.n_composited}, samples {st.n_samples}")
    assert np.all(np.isfinite(rec)) and np.all(np.isfinite(dep)), what
    assert np.all(hit | np.all(rec[:, :3] == 0, axis=1)), (what, "a pixel below the threshold carries a record")
    assert np.all(rec[n:] == 0) and np.all(dep[n:] == 0), (what, "pixels without a ray")
    assert np.all(rec[hit, 2] < p) and np.all(rec[hit, 1] > 0) and np.all(rec[hit, 0] > rec[hit, 1]), what
    if share is not None:
        assert np.mean(hit) >= share, (what, float(np.mean(hit)))
    # the density-only frame under the same limits: what a miss carries
    D = _clipped(ctx, o, d, n, t_min=t_min, t_max=t_max, flags=DENS_T)
    Da, Dd = D[0][..., 3].reshape(-1), D[1].reshape(-1)
    miss = ~hit
    assert np.array_equal(_bits(rec[miss, 3]), _bits(Da[miss])) and np.array_equal(_bits(dep[miss]), _bits(Dd[miss])), (what, "misses")
    assert np.all(rec[hit, 3] <= Da[hit]), what
    base = np.full(n, INF, np.float32) if t_max is None else np.asarray(t_max, np.float32)[:n]
    h = hit[:n]
    # (A) ends WITH the crossing sample
    tA = np.where(h, np.minimum(base, rec[:n, 0]), base).astype(np.float32)
    A = _clipped(ctx, o, d, n, t_min=t_min, t_max=tA, flags=DENS_T)
    assert np.array_equal(_bits(A[0][..., 3].reshape(-1)), _bits(rec[:, 3])), (what, "A: alpha")
    assert np.array_equal(_bits(A[1].reshape(-1)), _bits(dep)), (what, "A: depth")
    assert A[2].n_composited == st.n_composited and A[2].n_rays == st.n_rays, (what, A[2].n_composited, st.n_composited, A[2].n_rays, st.n_rays)
    # (B) ends BEFORE it
    tB = np.where(h, np.minimum(base, rho.lowered(rec[:n])), base).astype(np.float32)
    B = _clipped(ctx, o, d, n, t_min=t_min, t_max=tB, flags=DENS_T)
    Ba = B[0][..., 3].reshape(-1)
    assert np.array_equal(_bits(Ba[hit]), _bits(rec[hit, 2])) and np.all(Ba[hit] < p), (what, "B: alpha before the crossing sample")
    assert st.n_composited <= D[2].n_composited
    return rec, dep, st, D


# ---------------------------------------------------------------- 1. exact, against the density-only path
@pytest.mark.parametrize("W,H", [(64, 64), (33, 70)])
@pytest.mark.parametrize("sched", list(clip.SCHED))
@pytest.mark.parametrize("model", list(clip.SMALL))
def test_a_record_is_the_density_only_ray_clipped_at_its_crossing_sample(model, sched, W, H):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **clip.SMALL[model])
    ctx = _context(desc, W, H, clip.SCHED[sched])
    assert clip._rays_instance(ctx) == (16 if sched == "persistent" else 0)
    o, d = _framed_rays(ctx, W, H)
    for opacity in OPACITIES:
        _check_against_density_only(ctx, o, d, W * H, opacity, (model, sched, W, H), share=0.4 if opacity == 0.5 else None)
    ctx.close()


@pytest.mark.parametrize("name,kw,code,share", [("wide-frequency12", dict(dir_otype="Frequency", n_frequencies=12), 2, 0.4),
                                                ("generic-sine", dict(activation="Sine"), 1, 0.1)])
def test_the_wide_and_generic_stages(name, kw, code, share):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **kw)
    W, H = 100, 52
    ctx = _context(desc, W, H)
    assert clip._rays_instance(ctx) == code, name
    o, d = _framed_rays(ctx, W, H)
    for opacity in OPACITIES:
        _check_against_density_only(ctx, o, d, W * H, opacity, name, share=share if opacity == 0.5 else None)
    ctx.close()


# the rows of tests/test_render_rays_density_gpu.py: with the tests above all 13 instances launch
FORM_CASES = [("h96", "persistent"), ("h96", "strip"), ("h64-b1.5-c2", "persistent"), ("h30", "strip"), ("wide-pow2", "strip"),
              ("wide-h30", "strip"), ("sine-h30", "strip"), ("wide-h96", "strip")]


@pytest.mark.parametrize("row,sched", FORM_CASES)
def test_the_other_march_forms(row, sched):
    assert sched in rf.schedules(row)
    desc, keep, _ = rf.build(row)
    env = rf.SCHED[sched]
    W, H = rf.RW, rf.RH
    ctx = _context(desc, W, H, env)
    assert clip._rays_instance(ctx) == rf.expected_instance(row, env), (row, sched)
    o, d = _device_rays(ctx, W, H)
    share = 0.1 if row in rf.SINE_ROWS else 0.4
    for opacity in OPACITIES:
        _check_against_density_only(ctx, o, d, W * H, opacity, (row, sched), share=share if opacity == 0.5 else None)
    ctx.close()


@pytest.mark.parametrize("sched", list(clip.SCHED))
def test_pixels_without_a_ray_and_refused_rays_are_zero(sched):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W = H = 64
    n, m = W * H, W * H - 37
    ctx = _context(desc, W, H, clip.SCHED[sched], bg_color=0.25)  # (the background plays no part)
    o, d = _device_rays(ctx, W, H)
    full = _hits(ctx, o, d, n, 0.5)[0].reshape(n, 4)
    on = np.flatnonzero(full[:m, 3] >= 0.5)
    assert len(on) > 200
    nan_o, long_d, short_d = on[[10, len(on) // 2, len(on) - 10]], on[[20, len(on) // 3, len(on) - 25]], on[[30, len(on) // 4]]
    oh, dh = o.cpu().numpy().copy(), d.cpu().numpy().copy()
    oh[nan_o] = np.nan
    dh[long_d] *= np.float32(3.0) / np.linalg.norm(dh[long_d], axis=1, keepdims=True).astype(np.float32)   # |d|^2 = 9
    dh[short_d] *= np.float32(0.4) / np.linalg.norm(dh[short_d], axis=1, keepdims=True).astype(np.float32)  # |d|^2 = 0.16
    o2, d2 = _upload(oh), _upload(dh)
    rec, dep, st, D = _check_against_density_only(ctx, o2, d2, m, 0.5, (sched, "refused rays"))
    ctx.close()
    off = np.concatenate([nan_o, long_d, short_d])
    assert np.all(rec[off] == 0) and np.all(dep[off] == 0)
    assert np.all(rec[m:] == 0) and np.all(dep[m:] == 0)
    rest = np.setdiff1d(np.arange(m), off)
    assert np.array_equal(_bits(rec[rest]), _bits(full[rest]))  # (every other ray is untouched by its neighbours)


# ---------------------------------------------------------------- 2. with limits of its own
@pytest.mark.parametrize("kind", ["t_max", "t_min"])
@pytest.mark.parametrize("sched", list(clip.SCHED))
@pytest.mark.parametrize("model", list(clip.SMALL))
def test_with_limits_of_its_own(model, sched, kind):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **clip.SMALL[model])
    W = H = 64
    n = W * H
    ctx = _context(desc, W, H, clip.SCHED[sched])
    o, d = _device_rays(ctx, W, H)
    t = rco.ramp(W, H)
    free = _clipped(ctx, o, d, n, flags=DENS_T)[0][..., 3].reshape(-1)
    for opacity in OPACITIES:
        rec, dep, st, D = _check_against_density_only(ctx, o, d, n, opacity, (model, sched, kind), **{kind: t})
        Da = D[0][..., 3].reshape(-1)
        cut = (Da == 0) & (free > 0.5)  # rays the ramp cuts fully: all zero
        if kind == "t_max":
            assert np.mean(cut) >= 0.2
        assert np.all(rec[cut] == 0) and np.all(dep[cut] == 0)
        hit = rec[:, 3] >= np.float32(opacity)
        assert hit.any()
        if kind == "t_min":
            assert np.all(rec[hit, 0] > t[hit])  # (a crossing sample ends behind t_min)
    ctx.close()


# ---------------------------------------------------------------- 3. monotone in the threshold
@pytest.mark.parametrize("sched", list(clip.SCHED))
def test_monotone_in_the_threshold(sched):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W = H = 64
    n = W * H
    ctx = _context(desc, W, H, clip.SCHED[sched])
    o, d = _device_rays(ctx, W, H)
    got = {p: _hits(ctx, o, d, n, p) for p in OPACITIES}
    free = _clipped(ctx, o, d, n, flags=DENS_T)
    ctx.close()
    rec = {p: got[p][0].reshape(-1, 4) for p in OPACITIES}
    hit = {p: rec[p][:, 3] >= np.float32(p) for p in OPACITIES}
    h = hit[0.99]
    assert np.mean(h) > 0.2
    assert np.all(hit[0.9][h]) and np.all(hit[0.5][hit[0.9]])  # the hit sets are nested
    assert np.all(rec[0.5][h, 0] <= rec[0.9][h, 0]) and np.all(rec[0.9][h, 0] <= rec[0.99][h, 0])
    assert np.any(rec[0.5][h, 0] < rec[0.99][h, 0])
    comp = [int(got[p][2].n_composited) for p in OPACITIES]
    print(f"{sched}: composited {comp} at {OPACITIES}, {free[2].n_composited} without a threshold")
    assert 0 < comp[0] < comp[1] < comp[2] < free[2].n_composited
    a_free = free[0][..., 3].reshape(-1)
    for p in OPACITIES:
        assert np.all(rec[p][:, 3] <= a_free)


# ---------------------------------------------------------------- 4. schedule independence
def test_the_records_do_not_depend_on_the_schedule():
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W = H = 64
    frames, ratio = {}, {}
    for name, env in (("persistent", clip.PERSISTENT), ("strip", clip.STRIP), ("tail split off", dict(clip.PERSISTENT, NRF_TAIL_SPLIT="0")),
                      ("fast-forward off", dict(clip.PERSISTENT, NRF_MARCH_FF="0")), ("budget 3", dict(clip.PERSISTENT, NRF_MARCH_BUDGET="3")),
                      ("no sample cap", dict(clip.PERSISTENT, NRF_SAMPLE_CAP="0")), ("strip, no sample cap", dict(clip.STRIP, NRF_SAMPLE_CAP="0"))):
        ctx = _context(desc, W, H, env)
        assert clip._rays_instance(ctx) == (0 if name.startswith("strip") else 16), name
        o, d = _device_rays(ctx, W, H)
        frames[name] = {p: _hits(ctx, o, d, W * H, p) for p in OPACITIES}
        ctx.close()
    want = frames["persistent"]
    for p in OPACITIES:
        assert np.mean(want[p][0][..., 3] >= np.float32(p)) > 0.2
        for name, got in frames.items():
            clip._same(got[p][:2], want[p][:2], (name, p))
            assert got[p][2].n_composited == want[p][2].n_composited, (name, p)
        for a, b in (("persistent", "no sample cap"), ("strip", "strip, no sample cap")):
            ra, rb = (frames[k][p][2].n_samples / frames[k][p][2].n_composited for k in (a, b))
            print(f"opacity {p}, {a}: n_samples / n_composited {ra:.3f} with the threshold's sample cap, {rb:.3f} with NRF_SAMPLE_CAP=0")


# ---------------------------------------------------------------- 5. against the checker
@pytest.mark.parametrize("model,sched", [("bound1", "persistent"), ("bound1", "strip"), ("bound4-cascade3", "persistent"),
                                         ("bound4-cascade3", "strip"), ("h30", "strip")])
def test_against_the_checker_at_one_half(model, sched):
    """A ray is `certain` when no composited sample of the checker's brought its weight sum within 2 / 255 of the threshold -- the
    project's frame tolerance, which the ramp tests apply to clipped alpha: on such a ray an alpha error within the tolerance cannot
    move the crossing sample.  There hit or miss agrees, t and dt are the checker's bits (the march is bit-exact against the oracle),
    the weight sums and the depth are within 2 / 255.  At most 0.12 of the checker's hit rays may be uncertain (checker: 0.083 /
    0.094 / 0.080); at 0.9 and 0.99 that share is 0.29 to 0.95, so those thresholds rest on the exact tests above."""
    _against_the_checker_at_one_half(model, sched)


def _against_the_checker_at_one_half(model, sched, opts_kw=None, max_uncertain=0.12, min_both=0.4):
    """opts_kw: nrf_options fields the context renders under and the checker is computed with (None: the defaults).  The margin
    rule and the tolerances are the same under any options; max_uncertain and min_both are conditions on the CHECKER's scene (that
    the comparison says something), which a caller with other options states from the checker's own figures."""
    import test_ray_hits_cpu as hcpu
    desc, orc, o, d, full = hcpu._scene(model)
    if opts_kw:
        opts = nh.default_options()
        for k, v in opts_kw.items():
            setattr(opts, k, v)
        want = rho.ray_hits(orc, desc, o, d, 0.5, opts)
    else:
        want = hcpu._hits(model, 0.5)
    W, H = rf.RW, rf.RH
    env = clip.SCHED[sched]
    ctx = _context(desc, W, H, env, **(opts_kw or {}))
    assert clip._rays_instance(ctx) == (16 if sched == "persistent" else 0)
    rgba, depth, st = _hits(ctx, _upload(o), _upload(d), W * H, 0.5)
    ctx.close()
    rec, dep = rgba.reshape(-1, 4), depth.reshape(-1)
    certain = want.margin >= TOL
    uncertain = float(np.mean(~certain[want.hit]))
    hit = rec[:, 3] >= np.float32(0.5)
    e_ws = float(np.abs(rec[certain][:, 2:] - want.records[certain][:, 2:]).max())
    e_dep = float(np.abs(dep[certain] - want.depth[certain]).max())
    print(f"{model} {sched}: uncertain share of the checker's hit rays {uncertain:.3f}; certain rays: hit / miss differs on "
          f"{int(np.sum(hit[certain] != want.hit[certain]))}, max|d ws| {e_ws:.3e}, max|d depth| {e_dep:.3e}; composited {st.n_composited} "
          f"(checker {want.n_composited})")
    assert uncertain <= max_uncertain
    assert np.array_equal(hit[certain], want.hit[certain])
    both = certain & want.hit
    assert np.mean(both) >= min_both
    assert np.array_equal(_bits(rec[both, :2]), _bits(want.records[both, :2]))
    assert e_ws <= TOL and e_dep <= TOL
    return rec, dep, want


# ---------------------------------------------------------------- 6. views and shards
@pytest.mark.parametrize("sched", list(clip.SCHED))
def test_views_shards_and_bound_outputs(sched):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W, H = 100, 52
    n = W * H
    p = 0.9
    env = clip.SCHED[sched]
    ctx = _context(desc, W, H, env)
    rays = [_device_rays(ctx, W, H, az, el) for az, el in ((30, 30), (150, 10), (250, 45))]
    t = rco.ramp(W, H)
    lims = [t, (np.float32(1.6) - (t - np.float32(0.7))).astype(np.float32), (t + np.float32(0.3)).astype(np.float32)]
    singles = [_hits(ctx, r[0], r[1], n, p, t_max=lim) for r, lim in zip(rays, lims)]
    o3 = torch.cat([r[0] for r in rays]).contiguous()
    d3 = torch.cat([r[1] for r in rays]).contiguous()
    t3 = _upload(np.concatenate(lims))
    ctx.set_max_views(3)
    f = ctx.ray_hits(o3.data_ptr(), d3.data_ptr(), n, p, 0, t3.data_ptr(), n_views=3)
    assert f.n_views == 3
    st3 = ctx.stats()
    views = [ctx.read_view_f32(v) for v in range(3)]
    assert not np.array_equal(views[0][0], views[1][0])
    for v in range(3):
        assert np.mean(views[v][0][..., 3] >= np.float32(p)) > 0.05
        clip._same(views[v], singles[v][:2], (sched, "view", v))
    assert st3.n_composited == sum(int(s[2].n_composited) for s in singles)
    # bound float outputs
    out, outd = torch.full((3, H, W, 4), 7.0, device="cuda"), torch.full((3, H, W), 7.0, device="cuda")
    torch.cuda.synchronize()
    ctx.bind_output(out.data_ptr(), outd.data_ptr())
    ctx.ray_hits(o3.data_ptr(), d3.data_ptr(), n, p, 0, t3.data_ptr(), n_views=3)
    torch.cuda.synchronize()
    ctx.bind_output(None, None)
    for v in range(3):
        clip._same((out[v].cpu().numpy(), outd[v].cpu().numpy()), singles[v][:2], (sched, "bound outputs, view", v))
    # two shards, tile-major: nrf_read_shard_f32, then nrf_untile with 4 and with 1 channel
    o, d = rays[0]
    tm = _upload(lims[0])
    tps = nh.tiles_per_shard(W, H, 2)
    gathered, gdepth = np.zeros((2, tps * 64, 4), np.float32), np.zeros((2, tps * 64, 1), np.float32)
    composited = 0
    for idx in range(2):
        c2 = _context(desc, W, H, env, shard_index=idx, shard_count=2)
        f = c2.ray_hits(o.data_ptr(), d.data_ptr(), n, p, 0, tm.data_ptr())
        assert f.tile_major == 1
        part, dpart = np.empty((f.n_tiles * 64, 4), np.float32), np.empty(f.n_tiles * 64, np.float32)
        nh._check(c2.lib.nrf_read_shard_f32(c2.h, part.ctypes.data, dpart.ctypes.data))
        gathered[idx, :f.n_tiles * 64], gdepth[idx, :f.n_tiles * 64, 0] = part, dpart
        composited += int(c2.stats().n_composited)
        c2.close()
    assert composited == singles[0][2].n_composited
    g4, g1 = _upload(gathered), _upload(gdepth)
    o4, o1 = torch.empty((H, W, 4), device="cuda"), torch.empty((H, W, 1), device="cuda")
    torch.cuda.synchronize()
    ctx.untile(g4.data_ptr(), 2, tps, 4, o4.data_ptr())
    ctx.untile(g1.data_ptr(), 2, tps, 1, o1.data_ptr())
    torch.cuda.synchronize()
    clip._same((o4.cpu().numpy(), o1.cpu().numpy()[..., 0]), singles[0][:2], (sched, "two shards"))
    ctx.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W, H = 64, 48
    n = W * H
    ctx = _context(desc, W, H, bg_color=0.25)
    o, d = _device_rays(ctx, W, H)
    po, pd = o.data_ptr(), d.data_ptr()
    bgt = _upload(np.zeros((n, 3), np.float32))
    fn = ctx.lib.nrf_ray_hits

    def raw(opacity, background=0, flags=0, reserved=0):
        r = nh.Rays(po, pd, n, None, None, background or None, flags, reserved)
        return int(fn(ctx.h, 1, C.byref(r), C.c_float(opacity), None, None))

    def code(call):
        with pytest.raises(nh.NerfHipError) as e:
            call()
        return e.value.code

    def still_renders(what):
        _check_against_density_only(ctx, o, d, n, 0.5, what, share=0.4)
        plain = _clipped(ctx, o, d, n)
        ctx.render_rays(po, pd, n)
        clip._same(ctx.read_f32(), plain[:2], what)
        assert np.mean(plain[0][..., 3] > 0.5) > 0.02 and np.all(plain[0][plain[0][..., 3] == 0][:, :3] == np.float32(0.25)), what

    for opacity in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert raw(opacity) == nh.NRF_E_INVALID, opacity
        assert code(lambda: ctx.ray_hits(po, pd, n, opacity)) == nh.NRF_E_INVALID, opacity
    still_renders("after a bad opacity")
    assert raw(0.5, background=bgt.data_ptr()) == nh.NRF_E_INVALID
    for flags in (1, 4, 2, 8, 0x80000000):
        assert raw(0.5, flags=flags) == nh.NRF_E_INVALID, hex(flags)
    assert raw(0.5, reserved=1) == nh.NRF_E_INVALID
    assert code(lambda: ctx.ray_hits(0, pd, n, 0.5)) == nh.NRF_E_INVALID and code(lambda: ctx.ray_hits(po, pd, 0, 0.5)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.ray_hits(po, pd, n + 1, 0.5)) == nh.NRF_E_INVALID
    still_renders("after bad arguments")
    packed = torch.zeros(n, dtype=torch.int32, device="cuda")
    rgb8, d8 = torch.zeros((n, 3), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for bind, unbind in ((lambda: ctx.bind_output_rgbd8(packed.data_ptr()), lambda: ctx.bind_output_rgbd8(None)),
                         (lambda: ctx.bind_output_u8(rgb8.data_ptr(), d8.data_ptr()), lambda: ctx.bind_output_u8(None, None))):
        bind()
        assert code(lambda: ctx.ray_hits(po, pd, n, 0.5)) == nh.NRF_E_UNSUPPORTED
        unbind()
        still_renders("after unbinding")
    torch.cuda.synchronize()
    assert int((packed != 0).sum()) == 0 and int((rgb8 != 0).sum()) == 0 and int((d8 != 0).sum()) == 0  # (a refused call writes nothing)
    _options(ctx, bg_color=0.25, perturb=1)
    assert code(lambda: ctx.ray_hits(po, pd, n, 0.5)) == nh.NRF_E_UNSUPPORTED
    _options(ctx, bg_color=0.25, fast_interp=1)  # ignored, as by every RAYS instance
    fast = _hits(ctx, o, d, n, 0.5)
    _options(ctx, bg_color=0.25)
    clip._same(fast[:2], _hits(ctx, o, d, n, 0.5)[:2], "fast_interp")
    still_renders("after the refusals")
    one, free = _hits(ctx, o, d, n, 1.0), _clipped(ctx, o, d, n, flags=DENS_T)  # opacity 1 is legal: a ray stops only where ws rounds to 1
    assert 0 < one[2].n_composited <= free[2].n_composited and np.all(one[0][..., 3] <= free[0][..., 3])
    assert code(lambda: ctx.render_rays_clipped(po, pd, n, flags=8)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays_clipped(po, pd, n, flags=2)) == nh.NRF_E_INVALID
    ctx.close()


# ---------------------------------------------------------------- 8. the C++ mirror
_PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>
#include "nerf_render.h"
extern "C" int hipMalloc(void** p, size_t n);
extern "C" int hipMemcpy(void* dst, const void* src, size_t n, int kind);  // 1: host to device
int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
  const float opacity = (float)std::atof(argv[5]);
  const size_t n = (size_t)W * H;
  std::vector<float> rays(6 * n);
  std::ifstream in(argv[4], std::ios::binary);
  if (!in.read(reinterpret_cast<char*>(rays.data()), (std::streamsize)(rays.size() * sizeof(float)))) return 3;
  ngp::NerfRender render(std::vector<int>{0});
  render.reload_network_from_file(argv[1]);
  render.set_resolution(ngp::Vector2i(W, H));
  void *o = nullptr, *d = nullptr;
  if (hipMalloc(&o, 12 * n) || hipMalloc(&d, 12 * n)) return 4;
  if (hipMemcpy(o, rays.data(), 12 * n, 1) || hipMemcpy(d, rays.data() + 3 * n, 12 * n, 1)) return 5;
  const std::vector<float> hits = render.ray_hits(o, d, n, opacity);
  if (hits.size() != 5 * n) return 6;
  uint64_t h = 1469598103934665603ull;  // FNV-1a over the bytes
  const unsigned char* b = reinterpret_cast<const unsigned char*>(hits.data());
  for (size_t i = 0; i < hits.size() * sizeof(float); ++i) h = (h ^ b[i]) * 1099511628211ull;
  std::printf("ray_hits %zu %016llx\n", hits.size(), (unsigned long long)h);
  return 0;
}
"""


def _fnv1a(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_cpp_mirror_returns_the_python_calls_bytes(tmp_path):
    import shutil
    import synthetic as syn
    host = ROOT / "nerf-cuda_amd" / "host"
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None or not (host / "libngp_hip.so").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, H=32)
    snap = tmp_path / "tiny.msgpack"
    syn.write_snapshot(snap, cfg, keep[0], keep[1])
    W, H, p = 64, 48, 0.9
    ctx = _context(desc, W, H)
    o, d = _device_rays(ctx, W, H)
    rgba, depth, st = _hits(ctx, o, d, W * H, p)
    ctx.close()
    assert np.mean(rgba[..., 3] >= np.float32(p)) > 0.2
    want = _fnv1a(rgba.reshape(-1).tobytes() + depth.reshape(-1).tobytes())
    np.concatenate([o.cpu().numpy().reshape(-1), d.cpu().numpy().reshape(-1)]).astype(np.float32).tofile(tmp_path / "rays.bin")
    src, exe = tmp_path / "hits.cpp", tmp_path / "hits"
    src.write_text(_PROGRAM)
    # the HIP runtime the library itself is linked against
    ldd = subprocess.run(["ldd", str(nh.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    hip = next(Path(ln.split("=>")[1].split()[0]) for ln in ldd.splitlines() if "libamdhip64" in ln and "=>" in ln)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(host), "-o", str(exe), str(src), f"-L{host}", "-lngp_hip", f"-L{host.parent}", "-lnerfhip",
                    str(hip), f"-Wl,-rpath,{host}", f"-Wl,-rpath,{host.parent}", f"-Wl,-rpath,{hip.parent}"], check=True)
    r = subprocess.run([str(exe), str(snap), str(W), str(H), str(tmp_path / "rays.bin"), repr(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ray_hits ")][-1].split()
    assert int(line[1]) == 5 * W * H and int(line[2], 16) == want, (line, hex(want))
