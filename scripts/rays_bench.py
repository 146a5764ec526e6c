"""What rendering from caller-supplied rays costs against the pinhole path, on the flagship workload: the 1080p, T = 2^19
base.json-shaped model in 16-view launches.  One process alternates up to thirteen legs, so that all of them see the same box and clock:

  views          nrf_render_views of 16 orbit cameras (code nrf_render_rays does not touch: the baseline)
  rays           nrf_render_rays on the nrf_generate_rays output of the same cameras, persistent RAYS instance
  rays_strip     the same through the per-strip RAYS instance (a context created under NRF_PERSISTENT=0)
  rays_clipped   nrf_render_rays_clipped on the same rays with t_max = +inf in every entry and a background array that repeats
                 bg_color: the limits limit nothing, so the leg prices the reads (4 + 12 B per ray) and renders the same frame
  rays_clipped_strip   the same through the per-strip RAYS instance
  rays_density   nrf_render_rays_clipped on the same rays with NRF_RAYS_DENSITY_ONLY and no arrays: the density-only twin of the
                 persistent RAYS instance (no direction encoding, no colour network) -- its full twin is the rays leg
  rays_density_strip   the same through the per-strip instance -- its full twin is the rays_strip leg
  rays_hit50, rays_hit99   nrf_ray_hits on the same rays at opacity 0.5 / 0.99, persistent RAYS_HIT instance: the density-only ray
                 that stops at the threshold -- the yardstick is the rays_density leg of the same process
  rays_hit50_strip, rays_hit99_strip   the same through the per-strip instance -- against rays_density_strip
  rays_hit50_nocap, rays_hit99_nocap   the persistent legs in a context created under NRF_SAMPLE_CAP=0: every ray queues up to eight
                 samples per round, so n_samples / n_composited shows what the threshold's sample queue (FrameParams::hit_exp) saves
(--lib: another build of the library, e.g. the parent commit's; a build without nrf_render_rays_clipped runs the first three legs,
one without the flag the first five, one without nrf_ray_hits the first seven.)

Per leg: device ms per view (hipEvents around the call's launches, nrf_stats.render_ms) -- median, minimum, maximum over the
repetitions --, samples, composited samples per view, and the shader clock the persistent kernel measured in its launches (0: the
per-strip kernel has no such stamp).  The frames of all legs are compared bit for bit first; of a density-only leg the alpha and
depth planes, and its rgb planes with (1 - alpha) * bg_color; of a hit leg three views are held to the density-only call clipped at
the crossing sample's end and just below its start, as tests/test_ray_hits_gpu.py holds its frames.  Medians and ratios leave out a leg's first repetition, which follows
the read-back of that comparison.  Prints one JSON object.

Run it under a time limit:   timeout -k 10 300 python3 scripts/rays_bench.py [--reps 7] [--out profiles/.../rays_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nerf-cuda_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch  # noqa: E402
import models, nerfhip as nh, synthetic as syn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--views", type=int, default=16)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--out", default=None)
ap.add_argument("--lib", default=None, help="libnerfhip.so to measure (default: this tree's)")
ap.add_argument("--legs", default=None, help="comma-separated subset of the legs (views is always run: it is the baseline); two "
                "builds are compared with the SAME legs -- the clock a leg sees depends on what the process runs beside it")
args = ap.parse_args()
CLIPPED = True
if args.lib:
    import ctypes  # noqa: E402
    nh.LIB_PATH = type(nh.LIB_PATH)(args.lib).resolve()
    CLIPPED = hasattr(ctypes.CDLL(str(nh.LIB_PATH)), "nrf_render_rays_clipped")
    if not CLIPPED:
        del nh._SIGS["nrf_render_rays_clipped"]
W, H, V = args.width, args.height, args.views
cams = np.stack([syn.default_camera(W, H)] * V)
poses = np.stack([syn.orbit_pose(360.0 * i / V, 30.0) for i in range(V)])
desc, keep, _ = models.build_model(log2_hashmap_size=19, H=128)


def context(persistent, **env):
    env = dict(env, NRF_PERSISTENT=persistent)
    os.environ.update(env)
    try:
        c = nh.NerfHip(0)
    finally:
        for k in env:
            os.environ.pop(k, None)
    c.load_model(desc)
    c.set_resolution(W, H)
    c.set_max_views(V)
    return c


cp, cs = context("1"), context("0")
rays_o = torch.empty((V, W * H, 3), device="cuda")
rays_d = torch.empty((V, W * H, 3), device="cuda")
torch.cuda.synchronize()
for v in range(V):
    cp.generate_rays(cams[v], poses[v], rays_o[v].data_ptr(), rays_d[v].data_ptr(), 0, 0)
import ctypes as C  # noqa: E402
inst = cp.lib.nrf_debug_rays_instance
inst.restype, inst.argtypes = C.c_int, [C.c_void_p]
assert inst(cp.h) == 16 and inst(cs.h) == 0, (inst(cp.h), inst(cs.h))

LEGS = {
    "views": lambda: cp.render_views(cams, poses),
    "rays": lambda: cp.render_rays(rays_o.data_ptr(), rays_d.data_ptr(), W * H, n_views=V),
    "rays_strip": lambda: cs.render_rays(rays_o.data_ptr(), rays_d.data_ptr(), W * H, n_views=V),
}
CTX = {"views": cp, "rays": cp, "rays_strip": cs}
if CLIPPED:
    t_max = torch.full((V, W * H), float("inf"), device="cuda")
    bg = torch.full((V, W * H, 3), float(nh.default_options().bg_color), device="cuda")
    torch.cuda.synchronize()
    for name, c in (("rays_clipped", cp), ("rays_clipped_strip", cs)):
        LEGS[name] = lambda c=c: c.render_rays_clipped(rays_o.data_ptr(), rays_d.data_ptr(), W * H, 0, t_max.data_ptr(),
                                                        bg.data_ptr(), 0, n_views=V)
        CTX[name] = c
    DENSITY = getattr(nh, "NRF_RAYS_DENSITY_ONLY", 4)
    try:  # (a library from before the flag answers NRF_E_INVALID)
        cp.render_rays_clipped(rays_o.data_ptr(), rays_d.data_ptr(), W * H, flags=DENSITY)
        for name, c in (("rays_density", cp), ("rays_density_strip", cs)):
            LEGS[name] = lambda c=c: c.render_rays_clipped(rays_o.data_ptr(), rays_d.data_ptr(), W * H, flags=DENSITY, n_views=V)
            CTX[name] = c
    except nh.NerfHipError as e:
        assert e.code == nh.NRF_E_INVALID, e
HITS = CLIPPED and "rays_density" in LEGS and hasattr(cp.lib, "nrf_ray_hits")
cn = None
if HITS:
    cn = context("1", NRF_SAMPLE_CAP="0")
    for tag, p in (("50", 0.5), ("99", 0.99)):
        for suffix, c in (("", cp), ("_strip", cs), ("_nocap", cn)):
            LEGS[f"rays_hit{tag}{suffix}"] = lambda c=c, p=p: c.ray_hits(rays_o.data_ptr(), rays_d.data_ptr(), W * H, p, n_views=V)
            CTX[f"rays_hit{tag}{suffix}"] = c
if args.legs:
    LEGS = {k: f for k, f in LEGS.items() if k == "views" or k in args.legs.split(",")}
    assert "rays" in LEGS, "the rays leg is the one the ratios are taken against"

# all legs render the same frames
frames = {}
for name, run in LEGS.items():
    run()
    frames[name] = [CTX[name].read_view_f32(v) for v in (0, V // 2, V - 1)]
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_hits(c, p, v, what):
    """view v of a hit leg against the density-only call of the same context: clipped at the crossing sample's end it yields the
    records' weight sums and depths, clipped 4 ulps below its start the weight sums before it; misses carry the unclipped bits"""
    DT = DENSITY | nh.NRF_RAYS_DEPTH_T
    o, d = rays_o[v].data_ptr(), rays_d[v].data_ptr()
    c.ray_hits(o, d, W * H, p)
    rgba, depth = c.read_f32()
    rec, dep = rgba.reshape(-1, 4), depth.reshape(-1)
    hit = rec[:, 3] >= np.float32(p)
    assert np.all(hit | np.all(rec[:, :3] == 0, axis=1)) and np.all(rec[hit, 2] < np.float32(p)), what
    c.render_rays_clipped(o, d, W * H, flags=DT)
    free, fdep = c.read_f32()
    assert np.array_equal(bits(rec[~hit, 3]), bits(free.reshape(-1, 4)[~hit, 3])) and np.array_equal(bits(dep[~hit]), bits(fdep.reshape(-1)[~hit])), what
    low = (rec[:, 0] - rec[:, 1]).astype(np.float32)
    for _ in range(4):
        low = np.nextafter(low, np.float32(-np.inf))
    for kind, lim in (("A", rec[:, 0]), ("B", low)):
        t = torch.from_numpy(np.where(hit, lim, np.float32(np.inf)).astype(np.float32)).cuda()
        torch.cuda.synchronize()
        c.render_rays_clipped(o, d, W * H, 0, t.data_ptr(), 0, DT)
        got, gdep = c.read_f32()
        if kind == "A":
            assert np.array_equal(bits(got[..., 3].reshape(-1)), bits(rec[:, 3])) and np.array_equal(bits(gdep.reshape(-1)), bits(dep)), (what, kind)
        else:
            assert np.array_equal(bits(got[..., 3].reshape(-1)[hit]), bits(rec[hit, 2])), (what, kind)
    return float(np.mean(hit)), rgba, depth


hit_share = {}
for name in list(LEGS)[1:]:
    if "hit" in name:  # (checked on one-view calls of its context; the 16-view frames of the leg against those records)
        p = 0.5 if "hit50" in name else 0.99
        for (v, a) in zip((0, V // 2, V - 1), frames[name]):
            hit_share[name], one, one_depth = check_hits(CTX[name], p, v, (name, v))
            assert np.array_equal(bits(a[0]), bits(one)) and np.array_equal(bits(a[1]), bits(one_depth)), (name, v)
        continue
    for a, b in zip(frames[name], frames["views"]):
        if "density" in name:  # alpha and depth of the full frame; rgb = the background that gets through, two roundings
            alpha = a[0][..., 3]
            through = ((np.float32(1) - alpha).astype(np.float32) * np.float32(nh.default_options().bg_color)).astype(np.float32)
            assert np.array_equal(alpha.view(np.uint32), b[0][..., 3].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), name
            assert np.array_equal(a[0][..., :3], np.repeat(through[..., None], 3, axis=-1)), name
            continue
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), name
del frames

ms = {k: [] for k in LEGS}
clock = {k: [] for k in LEGS}
samples, composited = {}, {}
for _ in range(args.reps):
    for name, run in LEGS.items():
        run()
        st = CTX[name].stats()
        ms[name].append(st.render_ms / V)
        clock[name].append(st.shader_clock_mhz)
        samples[name] = int(st.n_samples)
        composited[name] = int(st.n_composited)
res = {"workload": f"{V} views of {W}x{H}, T = 2^19 base.json shape", "reps": args.reps, "lib": os.path.relpath(str(nh.LIB_PATH), ROOT), "legs": {}}
for name in LEGS:
    full = np.array(ms[name])
    a = full[1:] if len(full) > 1 else full  # without the first repetition, which follows the read-back
    ck = np.array(clock[name][1:] or clock[name])
    res["legs"][name] = {"ms_per_view_median": round(float(np.median(a)), 4), "ms_per_view_min": round(float(a.min()), 4),
                         "ms_per_view_max": round(float(a.max()), 4), "n_samples": samples[name],
                         "n_composited_per_view": round(composited[name] / V, 1),
                         "n_samples_over_n_composited": round(samples[name] / max(composited[name], 1), 4),
                         "shader_clock_mhz": round(float(np.median(ck)), 1),
                         "ms_per_view_all": [round(float(x), 4) for x in full]}
    print(f"{name:18s} {np.median(a):7.4f} ms/view (min {a.min():.4f}, max {a.max():.4f})  samples {samples[name]}  "
          f"composited/view {composited[name] / V:.0f}  shader_clock_mhz {np.median(ck):.0f}", file=sys.stderr, flush=True)
m = {k: res["legs"][k]["ms_per_view_median"] for k in LEGS}
spread = (res["legs"]["views"]["ms_per_view_max"] - res["legs"]["views"]["ms_per_view_min"]) / m["views"]
res["rays_over_views"] = round(m["rays"] / m["views"], 4)
for a, b in (("rays_strip", "rays"), ("rays_clipped", "rays"), ("rays_clipped_strip", "rays_strip"), ("rays_density", "rays"),
             ("rays_density_strip", "rays_strip"), ("rays_hit50", "rays_density"), ("rays_hit99", "rays_density"),
             ("rays_hit50_strip", "rays_density_strip"), ("rays_hit99_strip", "rays_density_strip"), ("rays_hit50_nocap", "rays_hit50"),
             ("rays_hit99_nocap", "rays_hit99")):
    if a in m and b in m:
        res[f"{a}_over_{b}"] = round(m[a] / m[b], 4)
a = np.array(ms["rays"][1:] or ms["rays"])  # without the first repetition, which follows the read-back
res["rays_run_to_run_spread"] = round(float((a.max() - a.min()) / np.median(a)), 4)
res["views_run_to_run_spread"] = round(spread, 4)  # (max - min) / median of the baseline leg
if hit_share:
    res["hit_share_last_view"] = {k: round(v, 4) for k, v in hit_share.items()}
q1, q3 = np.percentile(np.array(ms["views"][1:] or ms["views"]), [25, 75])
res["views_interquartile_spread"] = round(float((q3 - q1) / m["views"]), 4)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
cp.close()
cs.close()
if cn is not None:
    cn.close()
