"""nrf_render_rays on the GPU: frames from caller-supplied rays.

  * the rays nrf_generate_rays writes for a camera render that camera's nrf_render frame BIT FOR BIT -- through the persistent
    RAYS instance (base.json shape) and through the per-strip RAYS instances of every stage (hot, wide, generic);
  * rays a pinhole cannot describe (orthographic: one origin per ray; an equirectangular panorama) against the oracle
    assembled in tests/rays_oracle.py, at the project's frame tolerances;
  * short ray lists and guarded rays are exactly background and disturb no other pixel; views, shards, 8-bit outputs; refusals.
Every test here needs the entry point: none passes without it."""
import ctypes as C
import os

import numpy as np
import pytest

import models
import nerfhip as nh
import oracle_py as op
import rays_oracle as ro
import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STRIP = {"NRF_PERSISTENT": "0"}
PERSISTENT = {"NRF_PERSISTENT": "1"}
SMALL = {"bound1": dict(), "bound4-cascade3": dict(bound=4.0, cascade=3)}


def _context(desc, W, H, env=None, **opts_kw):
    """A context with the environment `env` in force at its creation (NRF_PERSISTENT is read by nrf_create)."""
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = nh.NerfHip(0)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    ctx.load_model(desc)
    o = nh.default_options()
    for k, v in opts_kw.items():
        setattr(o, k, v)
    ctx.set_options(o)
    ctx.set_resolution(W, H)
    return ctx


def _rays_instance(ctx):
    fn = ctx.lib.nrf_debug_rays_instance
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    return int(fn(ctx.h))


def _device_rays(ctx, cam, pose, W, H):
    o = torch.empty((H * W, 3), device="cuda")
    d = torch.empty((H * W, 3), device="cuda")
    torch.cuda.synchronize()
    ctx.generate_rays(cam, pose, o.data_ptr(), d.data_ptr(), 0, 0)
    return o, d


def _upload(a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    torch.cuda.synchronize()
    return t


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_frame(got, want, what):
    assert np.array_equal(_bits(got[0]), _bits(want[0])), what
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what


def _pinhole_identity(ctx, W, H, az, el, what):
    cam, pose = syn.default_camera(W, H), syn.orbit_pose(az, el)
    ctx.render(cam, pose)
    want = ctx.read_f32()
    wst = ctx.stats()
    assert wst.n_composited > 0, what
    o, d = _device_rays(ctx, cam, pose, W, H)
    f = ctx.render_rays(o.data_ptr(), d.data_ptr(), W * H)
    assert (f.width, f.height, f.n_views, f.tile_major) == (W, H, 1, 0)
    got = ctx.read_f32()
    st = ctx.stats()
    _same_frame(got, want, what)
    assert st.n_composited == wst.n_composited and st.n_rays == wst.n_rays, what


@pytest.mark.parametrize("W,H,az,el", [(64, 64, 30, 30), (100, 52, 135, 10), (8, 8, 300, 45), (33, 70, 250, -20)])
@pytest.mark.parametrize("sched", ["persistent", "strip"])
@pytest.mark.parametrize("model", list(SMALL))
def test_generated_rays_render_the_pinhole_frame_bit_for_bit(model, sched, W, H, az, el):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **SMALL[model])
    ctx = _context(desc, W, H, PERSISTENT if sched == "persistent" else STRIP)
    assert _rays_instance(ctx) == (16 if sched == "persistent" else 0)  # base.json shape: persistent RAYS instance / per-strip hot one
    _pinhole_identity(ctx, W, H, az, el, (model, sched, W, H))
    ctx.close()


@pytest.mark.parametrize("name,kw,code", [("hot", dict(), 0), ("wide-frequency12", dict(dir_otype="Frequency", n_frequencies=12), 2),
                                          ("generic-sine", dict(activation="Sine"), 1),
                                          ("generic-F4-w32", dict(n_features_per_level=4, n_neurons=32), 1)])
def test_every_stage_has_a_ray_instance(name, kw, code):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **kw)
    W, H = 100, 52
    # (hot: the per-strip instance; the others render rays per strip whatever NRF_PERSISTENT says -- the persistent RAYS
    #  instance is the hot shape's)
    ctx = _context(desc, W, H, STRIP if name == "hot" else None)
    assert _rays_instance(ctx) == code, name
    _pinhole_identity(ctx, W, H, 135, 10, name)
    ctx.close()


def _check_against_oracle(ctx, desc, o, d, W, H, min_cover, what, opts=None):
    """opts: the options the context renders under (None: the defaults), handed to the assembled oracle"""
    orc = op.Oracle(desc)
    want, wdepth, n = ro.render(orc, desc, o, d, opts)
    want, wdepth = want.reshape(H, W, 4), wdepth.reshape(H, W)
    cover = float(np.mean(want[..., 3] > 0.5))
    print(f"{what}: oracle samples {n}, pixels with alpha > 0.5: {cover:.3f}")
    assert cover >= min_cover and n > 0, (what, cover, n)  # (an all-background frame would pass everything below)
    do, dd = _upload(o), _upload(d)
    ctx.render_rays(do.data_ptr(), dd.data_ptr(), W * H)
    rgba, depth = ctx.read_f32()
    st = ctx.stats()
    e_rgba, e_depth, psnr = float(np.abs(rgba - want).max()), float(np.abs(depth - wdepth).max()), models.psnr(rgba, want)
    print(f"{what}: max|d rgba| {e_rgba:.3e} max|d depth| {e_depth:.3e} psnr {psnr:.1f} dB composited {st.n_composited} (oracle {n})")
    assert np.all(np.isfinite(rgba)) and np.all(np.isfinite(depth))
    assert e_rgba <= 2.0 / 255.0, what
    assert e_depth <= 2.0 / 255.0, what
    assert psnr >= 45.0, what
    assert abs(int(st.n_composited) - n) <= 0.002 * n + 8, (what, st.n_composited, n)


@pytest.mark.parametrize("sched", ["persistent", "strip"])
@pytest.mark.parametrize("model", list(SMALL))
def test_orthographic_rays_match_the_assembled_oracle(model, sched):
    """One origin per ray, one shared direction: the case only per-lane origins can render.  The object is framed with a
    half-extent of 1.2 around it, whatever the model's bound."""
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **SMALL[model])
    W, H = 64, 48
    o, d = ro.orthographic(W, H, half_extent=1.2)
    assert len(np.unique(o, axis=0)) == W * H and len(np.unique(d, axis=0)) == 1
    ctx = _context(desc, W, H, PERSISTENT if sched == "persistent" else STRIP)
    assert _rays_instance(ctx) == (16 if sched == "persistent" else 0)
    _check_against_oracle(ctx, desc, o, d, W, H, 0.05, ("orthographic", model, sched))
    ctx.close()


@pytest.mark.parametrize("sched", ["persistent", "strip"])
@pytest.mark.parametrize("model", list(SMALL))
def test_equirectangular_rays_match_the_assembled_oracle(model, sched):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32, **SMALL[model])
    W, H = 64, 48
    origin = op.Oracle(desc).generate_rays(syn.default_camera(W, H), syn.orbit_pose(30, 30), W, H)[0][0]  # the orbit camera's position
    o, d = ro.equirectangular(W, H, origin)
    ctx = _context(desc, W, H, PERSISTENT if sched == "persistent" else STRIP)
    _check_against_oracle(ctx, desc, o, d, W, H, 0.0, ("equirectangular", model, sched))
    ctx.close()


@pytest.mark.parametrize("sched", ["persistent", "strip"])
def test_short_ray_lists_and_guarded_rays_are_background(sched):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W, H = 100, 52
    bg = 0.25
    ctx = _context(desc, W, H, PERSISTENT if sched == "persistent" else STRIP, bg_color=bg)
    cam, pose = syn.default_camera(W, H), syn.orbit_pose(30, 30)
    o, d = _device_rays(ctx, cam, pose, W, H)
    ctx.render_rays(o.data_ptr(), d.data_ptr(), W * H)
    full = ctx.read_f32()
    assert np.mean(full[0][..., 3] > 0.5) > 0.02
    # (a) a list that ends in the middle of a row, inside the object's rows
    n = 27 * W + 41
    ctx.render_rays(o.data_ptr(), d.data_ptr(), n)
    rgba, depth = (a.reshape(W * H, -1) for a in ctx.read_f32())
    assert np.array_equal(_bits(rgba[:n]), _bits(full[0].reshape(-1, 4)[:n])) and np.array_equal(_bits(depth[:n]), _bits(full[1].reshape(-1, 1)[:n]))
    assert np.all(rgba[n:, :3] == np.float32(bg)) and np.all(rgba[n:, 3] == 0) and np.all(depth[n:] == 0)
    assert np.any(full[0].reshape(-1, 4)[n:, 3] > 0.5)  # (the tail does cover part of the object)
    # (b) guarded rays scattered over pixels the object covers
    on = np.flatnonzero(full[0].reshape(-1, 4)[:, 3] > 0.5)
    picks = on[np.linspace(0, len(on) - 1, 9).astype(int)]
    oh, dh = o.cpu().numpy().copy(), d.cpu().numpy().copy()
    oh[picks[0], 1] = np.nan
    dh[picks[1], 0] = np.nan
    dh[picks[2]] = 0.0
    oh[picks[3]] = [5000.0, 0.0, 0.0]
    oh[picks[4], 2] = np.inf
    dh[picks[5], 1] = -np.inf
    dh[picks[6]] *= 0.4      # |d|^2 = 0.16
    dh[picks[7]] *= 2.5      # |d|^2 = 6.25
    oh[picks[8]] = [-3000.0, 3000.0, 3000.0]
    o2, d2 = _upload(oh), _upload(dh)
    ctx.render_rays(o2.data_ptr(), d2.data_ptr(), W * H)
    rgba, depth = (a.reshape(W * H, -1) for a in ctx.read_f32())
    assert np.all(rgba[picks, :3] == np.float32(bg)) and np.all(rgba[picks, 3] == 0) and np.all(depth[picks] == 0)
    keep_px = np.setdiff1d(np.arange(W * H), picks)
    assert np.array_equal(_bits(rgba[keep_px]), _bits(full[0].reshape(-1, 4)[keep_px]))
    assert np.array_equal(_bits(depth[keep_px]), _bits(full[1].reshape(-1, 1)[keep_px]))
    ctx.close()


@pytest.mark.parametrize("sched", ["persistent", "strip"])
def test_views_shards_and_8bit_outputs(sched):
    desc, keep, _ = models.build_model(log2_hashmap_size=12, H=32)
    W, H = 100, 52
    env = PERSISTENT if sched == "persistent" else STRIP
    ctx = _context(desc, W, H, env)
    cam = syn.default_camera(W, H)
    poses = [syn.orbit_pose(30, 30), syn.orbit_pose(150, 10), syn.orbit_pose(260, -20)]
    n_px = W * H
    rays = [_device_rays(ctx, cam, p, W, H) for p in poses]
    o3 = torch.cat([r[0] for r in rays]).contiguous()
    d3 = torch.cat([r[1] for r in rays]).contiguous()
    torch.cuda.synchronize()
    singles = []
    for ro_, rd_ in rays:
        ctx.render_rays(ro_.data_ptr(), rd_.data_ptr(), n_px)
        singles.append(ctx.read_f32())
    # n_views = 3 in one call == three single calls
    ctx.set_max_views(3)
    f = ctx.render_rays(o3.data_ptr(), d3.data_ptr(), n_px, n_views=3)
    assert f.n_views == 3
    for v in range(3):
        _same_frame(ctx.read_view_f32(v), singles[v], ("view", v))
    # ... and with a short list per view: view v's rays start at v * rays_per_view
    n = 31 * W + 7
    o3s = torch.cat([r[0][:n] for r in rays]).contiguous()
    d3s = torch.cat([r[1][:n] for r in rays]).contiguous()
    torch.cuda.synchronize()
    ctx.render_rays(o3s.data_ptr(), d3s.data_ptr(), n, n_views=3)
    for v in range(3):
        rgba, depth = ctx.read_view_f32(v)
        assert np.array_equal(_bits(rgba.reshape(-1, 4)[:n]), _bits(singles[v][0].reshape(-1, 4)[:n])), v
        assert np.array_equal(_bits(depth.reshape(-1)[:n]), _bits(singles[v][1].reshape(-1)[:n])), v
        assert np.all(rgba.reshape(-1, 4)[n:, 3] == 0) and np.all(depth.reshape(-1)[n:] == 0), v
    ctx.set_max_views(1)
    # bound 8-bit outputs == nrf_quantize_* of the float frame
    o, d = rays[0]
    frgba, fdepth = _upload(singles[0][0]), _upload(singles[0][1])
    packed, wpacked = torch.zeros(n_px, dtype=torch.int32, device="cuda"), torch.zeros(n_px, dtype=torch.int32, device="cuda")
    rgb8, d8 = torch.zeros((n_px, 3), dtype=torch.uint8, device="cuda"), torch.zeros(n_px, dtype=torch.uint8, device="cuda")
    wrgb8, wd8 = torch.zeros((n_px, 3), dtype=torch.uint8, device="cuda"), torch.zeros(n_px, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.quantize_rgbd8(frgba.data_ptr(), fdepth.data_ptr(), n_px, wpacked.data_ptr())
    ctx.quantize_u8(frgba.data_ptr(), fdepth.data_ptr(), n_px, wrgb8.data_ptr(), wd8.data_ptr())
    ctx.bind_output_rgbd8(packed.data_ptr())
    ctx.render_rays(o.data_ptr(), d.data_ptr(), n_px)
    ctx.bind_output_rgbd8(None)
    ctx.bind_output_u8(rgb8.data_ptr(), d8.data_ptr())
    ctx.render_rays(o.data_ptr(), d.data_ptr(), n_px)
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
        o, d = _device_rays(c2, cam, poses[0], W, H)
        c2.bind_output(gathered[idx].data_ptr(), gdepth[idx].data_ptr())
        f = c2.render_rays(o.data_ptr(), d.data_ptr(), n_px)
        assert f.tile_major == 1
        c2.close()
    c1 = _context(desc, W, H, env)
    out, outd = torch.empty((H, W, 4), device="cuda"), torch.empty((H, W, 1), device="cuda")
    torch.cuda.synchronize()
    c1.untile(gathered.data_ptr(), 2, tps, 4, out.data_ptr())
    c1.untile(gdepth.data_ptr(), 2, tps, 1, outd.data_ptr())
    _same_frame((out.cpu().numpy(), outd.cpu().numpy()[..., 0]), singles[0], "two shards")
    c1.close()


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

    ctx = nh.NerfHip(0)
    assert code(lambda: ctx.render_rays(p, p, 16)) == nh.NRF_E_STATE            # no model
    ctx.load_model(desc)
    assert code(lambda: ctx.render_rays(p, p, 16)) == nh.NRF_E_STATE            # no resolution
    ctx.set_resolution(W, H)
    assert code(lambda: ctx.render_rays(0, p, 16)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays(p, 0, 16)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays(p, p, W * H + 1)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays(p, p, 0)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays(p, p, 16, n_views=0)) == nh.NRF_E_INVALID
    assert code(lambda: ctx.render_rays(p, p, 16, n_views=2)) == nh.NRF_E_STATE  # more views than the context's buffers hold
    o = nh.default_options()
    o.perturb = 7
    ctx.set_options(o)
    assert code(lambda: ctx.render_rays(p, p, W * H)) == nh.NRF_E_UNSUPPORTED
    ctx.set_options(nh.default_options())
    ctx.render_rays(p, p, W * H)  # ... and the context still renders
    rgba, depth = ctx.read_f32()
    assert np.all(np.isfinite(rgba)) and np.all(np.isfinite(depth))
    ctx.close()
