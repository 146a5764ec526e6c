"""What a baked texture costs: nrf_bake_mesh_texture on the blob model's mesh (tests/points_replay.blob_model(), testbed's lattice of
128^3 points over the aabb, iso 30.3) after nrf_simplify_mesh(2), res 8 on a width of 4096 -- one full network pass per texel, the
position and the direction made by the lane -- against the calls a caller has for the same points, each between two events on the
stream the work runs on:

  bake              nrf_bake_mesh_texture: two clears, the texel kernel, the UV kernel, the counter's download (the call synchronises)
  point_attributes  nrf_point_attributes with given directions on the evaluated texels' positions: SEVEN network passes per point
                    (its normal is reported all the same), positions and directions read from memory
  network           nrf_network on the same positions and directions: ONE pass, both read from memory

Before timing, the texels are held bit for bit to tests/bake_replay.py and nrf_network.  Median, minimum and maximum over the
repetitions without the first; one JSON object.

Run it under a time limit:   timeout -k 10 300 python3 scripts/bake_bench.py [--reps 11] [--size 128] [--res 8] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nerf-cuda_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch  # noqa: E402
import nerfhip as nh  # noqa: E402
import bake_replay as br, points_replay as pr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--iso", type=float, default=30.3)
ap.add_argument("--simplify", type=int, default=2)
ap.add_argument("--res", type=int, default=8)
ap.add_argument("--width", type=int, default=4096)
ap.add_argument("--out", default=None)
args = ap.parse_args()

desc, keep, _ = pr.blob_model()
bound = float(desc.bound)
ctx = nh.NerfHip(0)
ctx.load_model(desc)
stream = torch.cuda.Stream()
sp = stream.cuda_stream
assert sp != 0
N = args.size
cell = float(np.float32(2.0 * bound) / np.float32(N - 1))
m = ctx.extract_mesh(nh.Lattice.make([-bound] * 3, [cell] * 3, (N, N, N)), args.iso)
before = int(m.n_triangles)
if args.simplify:
    ctx.simplify_mesh(args.simplify)
v, t = ctx.read_mesh()
tex = ctx.bake_mesh_texture(args.res, args.width)
texels, rgba, uvs = ctx.read_mesh_texture()
want = br.bake(v, t, args.res, args.width, bound)
g = want["guard"]
n = int(g.sum())
assert n > 0 and tex.n_refused == want["n_refused"] and tex.height == want["height"]
x, d = torch.from_numpy(want["x"][g]).cuda(), torch.from_numpy(want["d"][g]).cuda()
sigma, rgb = torch.empty(n, device="cuda"), torch.empty((n, 3), device="cuda")
nrm, col = torch.empty((n, 4), device="cuda"), torch.empty((n, 4), device="cuda")
torch.cuda.synchronize()
ctx.network(x.data_ptr(), d.data_ptr(), n, sigma.data_ptr(), rgb.data_ptr())
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
got = texels[want["py"][g], want["px"][g]]
assert np.array_equal(bits(got[:, :3]), bits(rgb.cpu().numpy())) and np.array_equal(bits(got[:, 3]), bits(sigma.cpu().numpy())), "texels against nrf_network"
assert np.array_equal(rgba[want["py"][g], want["px"][g]], br.rgba8(rgb.cpu().numpy())) and int((rgba != 0).sum()) == n
h = float(np.float32(bound) / np.float32(128.0))

legs = {"bake": lambda: ctx.bake_mesh_texture(args.res, args.width, stream=sp),
        "point_attributes": lambda: ctx.point_attributes(x.data_ptr(), n, h, nrm.data_ptr(), col.data_ptr(), d.data_ptr(), stream=sp),
        "network": lambda: ctx.network(x.data_ptr(), d.data_ptr(), n, sigma.data_ptr(), rgb.data_ptr(), stream=sp)}
ms = {k: [] for k in legs}
for _ in range(args.reps):
    for name, run in legs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            run()
            e1.record(stream)
        e1.synchronize()
        ms[name].append(e0.elapsed_time(e1))
res = {"model": "points_replay.blob_model()", "device": torch.cuda.get_device_name(0), "reps": args.reps, "lattice": f"{N}^3", "iso": args.iso,
       "simplify": args.simplify, "triangles_extracted": before, "triangles": len(t), "res": args.res, "atlas": [int(tex.width), int(tex.height)],
       "work_items": ((len(t) + 1) // 2) * (args.res + 2) * (args.res + 1), "texels_evaluated": n, "texels_refused": int(tex.n_refused), "legs": {}}
for name, full in ms.items():
    a = np.array(full[1:] if len(full) > 1 else full)
    res["legs"][name] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4), "ms_max": round(float(a.max()), 4),
                         "ns_per_point": round(float(np.median(a)) * 1e6 / n, 3)}
    print(f"{name:17s} {np.median(a):9.4f} ms (min {a.min():.4f}, max {a.max():.4f})", file=sys.stderr, flush=True)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
ctx.close()
