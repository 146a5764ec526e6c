"""NRF_RAYS_DENSITY_ONLY on the GPU: nrf_render_rays_clipped for shadow and occlusion rays -- the density network alone.

The definition is in terms of the same call without the flag, so every test renders both on one context and asserts
  * alpha (weight_sum) and depth planes, n_rays and n_composited: bit-identical / equal;
  * rgb of every pixel: ((float32(1) - alpha) * b).astype(float32), b = the pixel's background (its ray's entry of the background
    array, else the scalar bg_color), computed here from the flagged alpha plane and compared as values (-0 == +0);
and, on unflagged frames, that the scene is one where this says something: in the case's own frame samples were composited and the
object covers pixels; in the scene's frame without limits the colour network moves at least 40 % of the pixels it touches by more
than 0.05 (on the CPU oracle that share is 0.525 for the Sine model and 0.99 for the others at 64 x 48 -- of the frame without
limits: under the ramp the Sine model keeps 0.28, so the condition is asserted where it was derived).
Covered: both hot models under both schedules at full and ragged frames; the wide and generic stages; the rows of tests/rays_forms.py
that reach the other march forms; schedule independence of the flagged frame; pixels without a ray, refused rays and empty intervals;
views and shards; the refusals.  Every test here needs the flag: none passes where 4 is an unknown bit."""
import ctypes as C

import numpy as np
import pytest

import models
import nerfhip as nh
import rays_clip_oracle as rco
import rays_forms as rf
import test_render_rays_clip_gpu as clip
from test_render_rays_clip_gpu import _bits, _clipped, _context, _device_rays, _options, _upload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DENS = 4  # == nh.NRF_RAYS_DENSITY_ONLY (spelled as the number where the test is about the bit)
BGC = 0.25
F1 = np.float32(1)


def _ray_background(W, H):
    """A background of non-negative values that differ from ray to ray and from channel to channel"""
    yy, xx = np.divmod(np.arange(W * H), W)
    return np.stack([xx / W, 0.1 + 0.8 * yy / H, 0.25 + 0.125 * ((3 * xx + 5 * yy) % 7)], axis=1).astype(np.float32)


def _transmitted(alpha, b):
    """(1 - weight_sum) * b in fp32: the subtraction rounded, then the product rounded"""
    T = (F1 - np.asarray(alpha, np.float32)).astype(np.float32)
    return (T[..., None] * np.asarray(b, np.float32)).astype(np.float32)


def _colour_share(rgba, b):
    """share of the pixels with alpha > 0 whose rgb differs from (1 - alpha) * b by more than 0.05 in some channel"""
    a = rgba[..., 3]
    differs = np.any(np.abs(rgba[..., :3] - _transmitted(a, b)) > 0.05, axis=-1)
    return float(np.mean(differs[a > 0])) if np.any(a > 0) else 0.0


def _scene_shows_colour(ctx, o, d, n, what):
    """The scene's unflagged frame without limits, over the scalar bg_color: the colour network did contribute to what the flag removes"""
    rgba, depth, st = _clipped(ctx, o, d, n)
    share = _colour_share(rgba, np.float32(BGC))
    print(f"{what}: without limits alpha > 0.5 on {np.mean(rgba[..., 3] > 0.5):.3f}, colour network visible on {share:.3f} of the hit pixels")
    assert st.n_composited > 0 and np.mean(rgba[..., 3] > 0.5) > 0.02, what
    assert share >= 0.4, (what, share)


def _check_twin(plain, dens, b, what, vacuity=True):
    """plain / dens: (rgba, depth, stats) of the same call without / with the flag; b: the background of every pixel, [H][W][3]"""
    (rgba, depth, st), (rgba_d, depth_d, st_d) = plain, dens
    a = rgba[..., 3]
    if vacuity:
        print(f"{what}: composited {st.n_composited}, alpha > 0.5 on {np.mean(a > 0.5):.3f}, colour network visible on "
              f"{_colour_share(rgba, b):.3f} of the hit pixels")
        assert st.n_composited > 0, what
        assert np.mean(a > 0.5) > 0.02, what
    assert np.array_equal(_bits(rgba_d[..., 3]), _bits(a)), (what, "alpha")
    assert np.array_equal(_bits(depth_d), _bits(depth)), (what, "depth")
    assert st_d.n_rays == st.n_rays and st_d.n_composited == st.n_composited, (what, st_d.n_rays, st.n_rays, st_d.n_composited, st.n_composited)
    want = _transmitted(rgba_d[..., 3], b)
    assert np.array_equal(rgba_d[..., :3], want), (what, "rgb", float(np.abs(rgba_d[..., :3] - want).max()))


def _both(ctx, o, d, n, flags=0, **kw):
    plain = _clipped(ctx, o, d, n, flags=flags, **kw)
    return plain, _clipped(ctx, o, d, n, flags=flags | nh.NRF_RAYS_DENSITY_ONLY, **kw)


def _cases(W, H):
    t = rco.ramp(W, H)
    return {"no arrays": dict(), "t_max": dict(t_max=t), "t_min": dict(t_min=t), "background": dict(bg=_ray_background(W, H)),
            "depth_t": dict(t_max=t, flags=nh.NRF_RAYS_DEPTH_T)}


CASES = ["no arrays", "t_max", "t_min", "background", "depth_t"]


# ---------------------------------------------------------------- 1. same alpha and depth, transmitted background
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("W,H", [(64, 64), (33, 70)])
@pytest.mark.parametrize("sched", list(clip.SCHED))
@pytest.mark.parametrize("model", list(clip.SMALL))
def test_same_alpha_and_depth_transmitted_background(model, sched, W, H, case):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **clip.SMALL[model])
    ctx = _context(desc, W, H, clip.SCHED[sched], bg_color=BGC)
    assert clip._rays_instance(ctx) == (16 if sched == "persistent" else 0)
    o, d = _device_rays(ctx, W, H)
    kw = _cases(W, H)[case]
    _scene_shows_colour(ctx, o, d, W * H, (model, sched, W, H))
    plain, dens = _both(ctx, o, d, W * H, **kw)
    ctx.close()
    b = kw["bg"].reshape(H, W, 3) if "bg" in kw else np.full((H, W, 3), BGC, np.float32)
    _check_twin(plain, dens, b, (model, sched, W, H, case))


# ---------------------------------------------------------------- 2. other stages and march forms
def _ramp_twin(desc, env, W, H, code, what):
    ctx = _context(desc, W, H, env, bg_color=BGC)
    assert clip._rays_instance(ctx) == code, what
    o, d = _device_rays(ctx, W, H)
    _scene_shows_colour(ctx, o, d, W * H, what)
    plain, dens = _both(ctx, o, d, W * H, t_max=rco.ramp(W, H))
    ctx.close()
    _check_twin(plain, dens, np.full((H, W, 3), BGC, np.float32), what)


@pytest.mark.parametrize("name,kw,code", [("wide-frequency12", dict(dir_otype="Frequency", n_frequencies=12), 2),
                                          ("generic-sine", dict(activation="Sine"), 1)])
def test_the_wide_and_generic_stages(name, kw, code):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **kw)
    _ramp_twin(desc, None, 100, 52, code, name)


# (wide-h96 is not one of the rows the feature's description lists: it is the only one that reaches the wide stage's GENERIC march
#  with its tables in LDS)
FORM_CASES = [("h96", "persistent"), ("h96", "strip"), ("h64-b1.5-c2", "persistent"), ("h30", "strip"), ("wide-pow2", "strip"),
              ("wide-h30", "strip"), ("sine-h30", "strip"), ("wide-h96", "strip")]


@pytest.mark.parametrize("row,sched", FORM_CASES)
def test_the_other_march_forms(row, sched):
    assert sched in rf.schedules(row)
    desc, keep, _ = rf.build(row)
    env = rf.SCHED[sched]
    _ramp_twin(desc, env, rf.RW, rf.RH, rf.expected_instance(row, env), (row, sched))


# ---------------------------------------------------------------- 3. schedule independence
def test_the_flagged_frame_does_not_depend_on_the_schedule():
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W = H = 64
    t = rco.ramp(W, H)
    frames = {}
    for name, env in (("persistent", clip.PERSISTENT), ("strip", clip.STRIP), ("tail split off", dict(clip.PERSISTENT, NRF_TAIL_SPLIT="0")),
                      ("fast-forward off", dict(clip.PERSISTENT, NRF_MARCH_FF="0")), ("budget 3", dict(clip.PERSISTENT, NRF_MARCH_BUDGET="3"))):
        ctx = _context(desc, W, H, env, bg_color=BGC)
        assert clip._rays_instance(ctx) == (0 if name == "strip" else 16), name
        o, d = _device_rays(ctx, W, H)
        frames[name] = _clipped(ctx, o, d, W * H, t_max=t, flags=nh.NRF_RAYS_DENSITY_ONLY)[:2]
        ctx.close()
    want = frames["persistent"]
    assert np.mean(want[0][..., 3] > 0.5) > 0.02
    for name, got in frames.items():
        clip._same(got, want, name)


# ---------------------------------------------------------------- 4. pixels without a ray, refused rays, empty intervals
@pytest.mark.parametrize("sched", list(clip.SCHED))
def test_pixels_without_a_ray_refused_rays_and_empty_intervals(sched):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W = H = 64
    n, m = W * H, W * H - 37
    ctx = _context(desc, W, H, clip.SCHED[sched], bg_color=BGC)
    o, d = _device_rays(ctx, W, H)
    full = _clipped(ctx, o, d, n)
    a_full = full[0][..., 3].reshape(n)
    yy, xx = np.divmod(np.arange(n), W)
    block = np.flatnonzero((yy >= 24) & (yy < 36) & (xx >= 20) & (xx < 44))  # 12 x 24 pixels across the middle of the object
    assert np.mean(a_full[block] > 0.5) > 0.5
    on = np.setdiff1d(np.flatnonzero(a_full[:m] > 0.5), block)  # object pixels that have a ray, outside the block
    assert len(on) > 200
    nan_o, long_d = on[[10, len(on) // 2, len(on) - 10]], on[[20, len(on) // 3, len(on) - 25]]
    oh, dh = o.cpu().numpy().copy(), d.cpu().numpy().copy()
    oh[nan_o] = np.nan
    dh[long_d] *= np.float32(3.0) / np.linalg.norm(dh[long_d], axis=1, keepdims=True).astype(np.float32)  # |d|^2 = 9
    t_max = np.full(n, np.nan, np.float32)
    t_max[block] = np.float32(0.5 * nh.default_options().min_near)  # t_max < near: near >= min_near
    bg = _ray_background(W, H)
    o2, d2 = _upload(oh), _upload(dh)
    plain, dens = _both(ctx, o2, d2, m, t_max=t_max[:m].copy(), bg=bg[:m].copy())
    ctx.close()
    listed = np.arange(n) < m
    b = np.where(listed[:, None], bg, np.float32(BGC)).reshape(H, W, 3)
    _check_twin(plain, dens, b, sched)
    rgba, depth = dens[0].reshape(n, 4), dens[1].reshape(n)
    off = np.concatenate([nan_o, long_d, block])
    assert np.all(listed[off])
    assert np.all(rgba[off, 3] == 0) and np.all(depth[off] == 0) and np.array_equal(rgba[off, :3], bg[off])
    assert np.all(rgba[~listed, 3] == 0) and np.all(depth[~listed] == 0) and np.all(rgba[~listed, :3] == np.float32(BGC))
    assert np.any(rgba[listed, 3] > 0.5)


# ---------------------------------------------------------------- 5. views and shards
@pytest.mark.parametrize("sched", list(clip.SCHED))
def test_views_and_shards(sched):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W, H = 100, 52
    n = W * H
    env = clip.SCHED[sched]
    ctx = _context(desc, W, H, env, bg_color=BGC)
    rays = [_device_rays(ctx, W, H, az, el) for az, el in ((30, 30), (150, 10), (250, 45))]
    t = rco.ramp(W, H)
    lims = [t, (np.float32(1.6) - (t - np.float32(0.7))).astype(np.float32), (t + np.float32(0.3)).astype(np.float32)]
    bg0 = _ray_background(W, H)
    bgs = [bg0, bg0[:, ::-1].copy(), (np.float32(0.5) * bg0).astype(np.float32)]
    o3 = torch.cat([r[0] for r in rays]).contiguous()
    d3 = torch.cat([r[1] for r in rays]).contiguous()
    t3, bg3 = _upload(np.concatenate(lims)), _upload(np.concatenate(bgs))
    ctx.set_max_views(3)
    views = {}
    for flags in (0, nh.NRF_RAYS_DENSITY_ONLY):
        f = ctx.render_rays_clipped(o3.data_ptr(), d3.data_ptr(), n, 0, t3.data_ptr(), bg3.data_ptr(), flags, n_views=3)
        assert f.n_views == 3
        st = ctx.stats()
        views[flags] = [ctx.read_view_f32(v) + (st,) for v in range(3)]
    ctx.close()
    assert not np.array_equal(views[DENS][0][0], views[DENS][1][0])
    for v in range(3):
        _check_twin(views[0][v], views[DENS][v], bgs[v].reshape(H, W, 3), (sched, "view", v))
    # two shards, tile-major, read through nrf_read_shard_f32: both ranks are given the same arrays
    o, d = rays[0]
    tm, bg = _upload(lims[0]), _upload(bgs[0])
    tps = nh.tiles_per_shard(W, H, 2)
    gathered = {0: np.full((2, tps * 64, 5), np.nan, np.float32), DENS: np.full((2, tps * 64, 5), np.nan, np.float32)}
    for idx in range(2):
        c2 = _context(desc, W, H, env, bg_color=BGC, shard_index=idx, shard_count=2)
        got = {}
        for flags in (0, nh.NRF_RAYS_DENSITY_ONLY):
            f = c2.render_rays_clipped(o.data_ptr(), d.data_ptr(), n, 0, tm.data_ptr(), bg.data_ptr(), flags)
            assert f.tile_major == 1
            part, dpart = np.empty((f.n_tiles * 64, 4), np.float32), np.empty(f.n_tiles * 64, np.float32)
            nh._check(c2.lib.nrf_read_shard_f32(c2.h, part.ctypes.data, dpart.ctypes.data))
            gathered[flags][idx, :f.n_tiles * 64, :4], gathered[flags][idx, :f.n_tiles * 64, 4] = part, dpart
            got[flags] = (part, dpart, c2.stats())
        c2.close()
        # the shard as it lies in its buffer (padding pixels are zero in both): alpha, depth, statistics
        assert np.array_equal(_bits(got[DENS][0][:, 3]), _bits(got[0][0][:, 3])) and np.array_equal(_bits(got[DENS][1]), _bits(got[0][1]))
        assert got[DENS][2].n_rays == got[0][2].n_rays and got[DENS][2].n_composited == got[0][2].n_composited
    frames = {k: nh.untile_numpy(g, W, H) for k, g in gathered.items()}
    assert not np.any(np.isnan(frames[0])) and not np.any(np.isnan(frames[DENS]))
    clip._same((frames[0][..., :4], frames[0][..., 4]), views[0][0][:2], (sched, "two shards, full"))
    clip._same((frames[DENS][..., :4], frames[DENS][..., 4]), views[DENS][0][:2], (sched, "two shards, density only"))


# ---------------------------------------------------------------- 6. refusals
def test_refusals():
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W, H = 64, 48
    n = W * H
    ctx = _context(desc, W, H, bg_color=BGC)
    o, d = _device_rays(ctx, W, H)
    p, q = o.data_ptr(), d.data_ptr()

    def code(fn):
        with pytest.raises(nh.NerfHipError) as e:
            fn()
        return e.value.code

    packed = torch.zeros(n, dtype=torch.int32, device="cuda")
    rgb8, d8 = torch.zeros((n, 3), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for bind, unbind in ((lambda: ctx.bind_output_rgbd8(packed.data_ptr()), lambda: ctx.bind_output_rgbd8(None)),
                         (lambda: ctx.bind_output_u8(rgb8.data_ptr(), d8.data_ptr()), lambda: ctx.bind_output_u8(None, None))):
        bind()
        assert code(lambda: ctx.render_rays_clipped(p, q, n, flags=DENS)) == nh.NRF_E_UNSUPPORTED
        assert code(lambda: ctx.render_rays_clipped(p, q, n, flags=DENS | nh.NRF_RAYS_DEPTH_T)) == nh.NRF_E_UNSUPPORTED
        unbind()
        plain, dens = _both(ctx, o, d, n)  # ... and the context renders a correct flagged frame afterwards
        _check_twin(plain, dens, np.full((H, W, 3), BGC, np.float32), "after unbinding")
    torch.cuda.synchronize()
    assert int((packed != 0).sum()) == 0 and int((rgb8 != 0).sum()) == 0  # (a refused call writes nothing)
    for flags in (8, DENS | 2, DENS | 0x80000000, 2, 0x80000000, DENS | 8):
        assert code(lambda: ctx.render_rays_clipped(p, q, n, flags=flags)) == nh.NRF_E_INVALID, hex(flags)
    _options(ctx, bg_color=BGC, perturb=1)
    assert code(lambda: ctx.render_rays_clipped(p, q, n, flags=DENS)) == nh.NRF_E_UNSUPPORTED
    _options(ctx, bg_color=BGC, fast_interp=1)  # ignored, as by every RAYS instance
    fast = _clipped(ctx, o, d, n, flags=DENS)
    _options(ctx, bg_color=BGC)
    plain, dens = _both(ctx, o, d, n)
    _check_twin(plain, dens, np.full((H, W, 3), BGC, np.float32), "after the refusals")
    clip._same(fast[:2], dens[:2], "fast_interp")
    assert nh.NRF_RAYS_DENSITY_ONLY == DENS
    ctx.close()
