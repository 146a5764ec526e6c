"""What the point queries cost: nrf_density, nrf_density_gradient and nrf_hit_gradients at the hit positions of the flagship
workload -- 16 views of 1080p at opacity 0.5, the T = 2^19 base.json-shaped model.  One process alternates four legs, so that all
of them see the same box and clock:

  density         nrf_density at the hit positions
  gradient        nrf_density_gradient at the hit positions (h = 2^-8 bound)
  hit_gradients   nrf_hit_gradients on the 16-view hit frame itself: every pixel of the frame is read, the hits are evaluated
  network_7n      the unfused composition, the yardstick: torch builds the 7 n taps ([n][7][3], 84 B per point written and read
                  again, plus as many directions) and ONE nrf_network call evaluates them -- through --parent-lib, the parent
                  commit's build of the library, in a context of its own in this process (without the option: this tree's)

Before timing, `gradient` is held to the yardstick bit for bit as tests/test_density_points_gpu.py holds it (the taps in numpy,
the differences in numpy), `density` to the yardstick's centre taps and `hit_gradients` to `gradient` at the positions it reports.
Per leg: device time between two events on the stream the calls run on, in nanoseconds per point (per hit) -- median, minimum
and maximum over the repetitions without the first.  Prints one JSON object.

Run it under a time limit:   timeout -k 10 300 python3 scripts/points_bench.py [--reps 7] [--parent-lib PATH] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nerf-cuda_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch  # noqa: E402
import models, nerfhip as nh, synthetic as syn  # noqa: E402
import points_replay as pr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--views", type=int, default=16)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--check-points", type=int, default=200000, help="points of the bit-for-bit check (the replay runs in numpy)")
ap.add_argument("--parent-lib", default=None, help="libnerfhip.so of the parent commit: the yardstick leg runs through it")
ap.add_argument("--out", default=None)
args = ap.parse_args()
W, H, V = args.width, args.height, args.views
OPACITY, FRAC = 0.5, 0.5
NEW = ("nrf_density", "nrf_density_gradient", "nrf_hit_gradients")

desc, keep, _ = models.build_model(log2_hashmap_size=19, H=128)
bound = np.float32(desc.bound)
h = np.float32(bound * np.float32(2.0 ** -8))
ctx = nh.NerfHip(0)
if args.parent_lib:  # a second library in the process: loaded without the three names it does not have, its context made through it
    sigs = {k: nh._SIGS.pop(k) for k in NEW}
    parent_lib = nh.load_library(args.parent_lib)
    nh._SIGS.update(sigs)
    assert not hasattr(parent_lib, "nrf_density"), "--parent-lib has the point queries: it is no parent"
    this_lib, nh._lib = nh._lib, parent_lib
    yard = nh.NerfHip(0)
    nh._lib = this_lib
else:
    yard = nh.NerfHip(0)
for c in (ctx, yard):
    c.load_model(desc)
    c.set_resolution(W, H)
    c.set_max_views(V)

cams = np.stack([syn.default_camera(W, H)] * V)
poses = np.stack([syn.orbit_pose(360.0 * i / V, 30.0) for i in range(V)])
rays_o = torch.empty((V, W * H, 3), device="cuda")
rays_d = torch.empty((V, W * H, 3), device="cuda")
torch.cuda.synchronize()
for v in range(V):
    ctx.generate_rays(cams[v], poses[v], rays_o[v].data_ptr(), rays_d[v].data_ptr(), 0, 0)
records = torch.empty((V * W * H, 4), device="cuda")  # the hit frame in a buffer of ours (nrf_bind_output), so that torch can read it
rec_depth = torch.empty(V * W * H, device="cuda")
torch.cuda.synchronize()
ctx.bind_output(records.data_ptr(), rec_depth.data_ptr())
frame = ctx.ray_hits(rays_o.data_ptr(), rays_d.data_ptr(), W * H, OPACITY, n_views=V)
assert frame.tile_major == 0 and frame.n_views == V and frame.rgba == records.data_ptr() and frame.view_stride_px == W * H
PX = int(frame.n_views) * int(frame.view_stride_px)
# a stream of torch's own for the legs: the library launches on the stream it is given and torch's tap arithmetic runs on the same
# one, so the yardstick's taps are complete when nrf_network reads them and two events on it bracket exactly one leg
# (a NULL stream would send the library's launches to the context's stream, which does not wait for torch's)
stream = torch.cuda.Stream()
sp = stream.cuda_stream
assert sp != 0
hit_pos = torch.empty((PX, 4), device="cuda")
hit_out = torch.empty((PX, 4), device="cuda")
torch.cuda.synchronize()
ctx.hit_gradients(frame, rays_o.data_ptr(), rays_d.data_ptr(), W * H, OPACITY, FRAC, float(h), hit_pos.data_ptr(), hit_out.data_ptr())
stride = int(frame.view_stride_px)
is_hit = ((torch.arange(PX, device="cuda") % stride) < W * H) & (records[:, 3] >= OPACITY)
xyz = hit_pos[is_hit][:, :3].contiguous()
N = int(xyz.shape[0])
assert 0 < 7 * N < 2 ** 32
print(f"{N} hit positions of {V} views ({N / (V * W * H):.3f} of the pixels)", file=sys.stderr, flush=True)

sigma = torch.empty(N, device="cuda")
grad = torch.empty((N, 4), device="cuda")
taps = torch.empty((N, 7, 3), device="cuda")
dirs = torch.zeros((N, 7, 3), device="cuda")
dirs[:, :, 2] = 1.0
sig7 = torch.empty((N, 7), device="cuda")
rgb7 = torch.empty((N, 7, 3), device="cuda")
torch.cuda.synchronize()


def network_7n():
    """the unfused composition: the taps of tests/points_replay.py built by torch, one nrf_network call"""
    taps.copy_(xyz[:, None, :].expand(N, 7, 3))
    for k in range(3):
        taps[:, 1 + 2 * k, k] = xyz[:, k] + float(h)
        taps[:, 2 + 2 * k, k] = xyz[:, k] - float(h)
    yard.network(taps.data_ptr(), dirs.data_ptr(), 7 * N, sig7.data_ptr(), rgb7.data_ptr(), stream=sp)


LEGS = {
    "density": lambda: ctx.density(xyz.data_ptr(), N, sigma.data_ptr(), stream=sp),
    "gradient": lambda: ctx.density_gradient(xyz.data_ptr(), N, float(h), grad.data_ptr(), stream=sp),
    "hit_gradients": lambda: ctx.hit_gradients(frame, rays_o.data_ptr(), rays_d.data_ptr(), W * H, OPACITY, FRAC, float(h),
                                               hit_pos.data_ptr(), hit_out.data_ptr(), stream=sp),
    "network_7n": network_7n,
}

# ---- bit for bit, before any timing
with torch.cuda.stream(stream):
    for run in LEGS.values():
        run()
torch.cuda.synchronize()
M = min(N, args.check_points)
x_h = xyz[:M].cpu().numpy()
ok = pr.guard(x_h, h, bound)
assert np.array_equal(pr.bits(taps[:M].cpu().numpy()), pr.bits(pr.taps(x_h, h))), "torch's taps are the replay's"
want = pr.gradient(sig7[:M].cpu().numpy(), h)
want[~ok] = 0.0
for what, a, b in (("gradient against the yardstick", grad[:M].cpu().numpy(), want), ("density against the yardstick's centre taps", sigma[:M].cpu().numpy(), sig7[:M, 0].cpu().numpy())):
    print(f"{what}: {int(np.sum(pr.bits(a) != pr.bits(b)))} of {a.size} words differ", file=sys.stderr, flush=True)
assert np.array_equal(pr.bits(grad[:M].cpu().numpy()), pr.bits(want)), "gradient against the yardstick"
assert np.array_equal(pr.bits(sigma[:M].cpu().numpy()), pr.bits(sig7[:M, 0].cpu().numpy())), "density against the yardstick's centre taps"
assert torch.equal(hit_out[is_hit].view(torch.int32), grad.view(torch.int32)), "hit_gradients against gradient"
assert bool((hit_out[~is_hit] == 0).all()) and bool((hit_pos[~is_hit] == 0).all())
print(f"bit for bit: {M} points against the yardstick ({int((~ok).sum())} refused by the guard), {N} hits against gradient", file=sys.stderr, flush=True)

# ---- timing
ns = {k: [] for k in LEGS}
for _ in range(args.reps):
    for name, run in LEGS.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            run()
            e1.record(stream)
        e1.synchronize()
        ns[name].append(e0.elapsed_time(e1) * 1e6 / N)
res = {"workload": f"hit positions of {V} views of {W}x{H} at opacity {OPACITY}, T = 2^19 base.json shape", "n_points": N,
       "hit_share": round(N / (V * W * H), 4), "h": float(h), "frac": FRAC, "reps": args.reps,
       "lib": os.path.relpath(str(nh.LIB_PATH), ROOT), "yardstick_lib": args.parent_lib or os.path.relpath(str(nh.LIB_PATH), ROOT), "legs": {}}
for name in LEGS:
    full = np.array(ns[name])
    a = full[1:] if len(full) > 1 else full
    res["legs"][name] = {"ns_per_point_median": round(float(np.median(a)), 3), "ns_per_point_min": round(float(a.min()), 3),
                         "ns_per_point_max": round(float(a.max()), 3), "ns_per_point_all": [round(float(x), 3) for x in full]}
    print(f"{name:14s} {np.median(a):8.3f} ns/point (min {a.min():.3f}, max {a.max():.3f})", file=sys.stderr, flush=True)
y = res["legs"]["network_7n"]
res["yardstick_spread"] = round((y["ns_per_point_max"] - y["ns_per_point_min"]) / y["ns_per_point_median"], 4)
res["gradient_over_network_7n"] = round(res["legs"]["gradient"]["ns_per_point_median"] / y["ns_per_point_median"], 4)
res["hit_gradients_over_gradient"] = round(res["legs"]["hit_gradients"]["ns_per_point_median"] / res["legs"]["gradient"]["ns_per_point_median"], 4)
res["gradient_over_density"] = round(res["legs"]["gradient"]["ns_per_point_median"] / res["legs"]["density"]["ns_per_point_median"], 4)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
ctx.close()
yard.close()
