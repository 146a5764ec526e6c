"""What vertex normals and colours cost: nrf_mesh_attributes at the vertices of testbed's default mesh -- 128^3 points over the aabb of
the benchmark's synthetic model (T = 2^19, base.json shape), iso 2.5, h = bound / 128 -- against the composition a caller had before
it, each between two events on the stream the work runs on:

  mesh_attributes   nrf_mesh_attributes: seven network passes per point in one launch (the call synchronises at its end)
  point_attributes  nrf_point_attributes on the mesh's device vertices: the same kernel into the caller's buffers, no synchronisation
  gradient          nrf_density_gradient on the same vertices: seven passes of the density network
  network           nrf_network on the same vertices and the replayed directions: the eighth pass, both networks
  composed          gradient + network, the sums of the two device times; what the caller also paid -- the records' download, the
                    normalisation on the host and the directions' upload -- is not in it

Before timing, the attributes are held bit for bit to tests/attr_replay.py on the gradient leg's records and to the network leg's
sigma and rgb.  Median, minimum and maximum over the repetitions without the first; one JSON object.

--iso_quantile Q takes that quantile of the lattice's sigmas as iso instead: the synthetic model's tables are noise, so such a surface
has about one vertex per lattice point (scripts/mesh_bench.py) and the figures are throughput, not launch latency.

Run it under a time limit:   timeout -k 10 300 python3 scripts/attr_bench.py [--reps 11] [--iso_quantile 0.9] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nerf-cuda_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch  # noqa: E402
import models, nerfhip as nh  # noqa: E402
import attr_replay as ar  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--iso", type=float, default=2.5)
ap.add_argument("--iso_quantile", type=float, default=None, help="instead of --iso: that quantile of the lattice's sigmas (a large surface)")
ap.add_argument("--out", default=None)
args = ap.parse_args()

desc, keep, _ = models.build_model(log2_hashmap_size=19, H=128)
bound = float(desc.bound)
ctx = nh.NerfHip(0)
ctx.load_model(desc)
stream = torch.cuda.Stream()
sp = stream.cuda_stream
assert sp != 0
N = args.size
cell = float(np.float32(2.0 * bound / (N - 1)))
lat = nh.Lattice.make([-bound] * 3, [cell] * 3, (N, N, N))
h = float(np.float32(bound) / np.float32(128.0))
if args.iso_quantile is not None:
    lattice_sigma = torch.empty(N ** 3, device="cuda")
    torch.cuda.synchronize()
    ctx.density_lattice(lat, lattice_sigma.data_ptr())
    args.iso = float(torch.quantile(lattice_sigma[:: max(1, N ** 3 // 1000000)], args.iso_quantile))
    del lattice_sigma
m = ctx.extract_mesh(lat, args.iso)
nv = int(m.n_vertices)
assert nv > 0
grad, nrm, col = (torch.empty((nv, 4), device="cuda") for _ in range(3))
sigma, rgb = torch.empty(nv, device="cuda"), torch.empty((nv, 3), device="cuda")
torch.cuda.synchronize()
ctx.density_gradient(m.vertices, nv, h, grad.data_ptr())
want, length, d, ok = ar.records(grad.cpu().numpy())
dirs = torch.from_numpy(d).cuda()
torch.cuda.synchronize()
ctx.network(m.vertices, dirs.data_ptr(), nv, sigma.data_ptr(), rgb.data_ptr())
ctx.mesh_attributes(h)
got_n, got_c = ctx.read_mesh_attributes()
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
refused = ~np.any(bits(grad.cpu().numpy()) != 0, axis=1)  # (a vertex within h of a face: zeros in every record)
assert np.array_equal(bits(got_n), bits(want)) and np.array_equal(bits(got_c[:, 3]), bits(length)), "normals against the replay"
keep_ = ~refused
assert np.array_equal(bits(got_c[keep_, :3]), bits(rgb.cpu().numpy()[keep_])) and np.array_equal(bits(got_n[keep_, 3]), bits(sigma.cpu().numpy()[keep_])), \
    "colours against nrf_network"

legs = {"mesh_attributes": lambda: ctx.mesh_attributes(h, stream=sp),
        "point_attributes": lambda: ctx.point_attributes(m.vertices, nv, h, nrm.data_ptr(), col.data_ptr(), stream=sp),
        "gradient": lambda: ctx.density_gradient(m.vertices, nv, h, grad.data_ptr(), stream=sp),
        "network": lambda: ctx.network(m.vertices, dirs.data_ptr(), nv, sigma.data_ptr(), rgb.data_ptr(), stream=sp)}
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
ms["composed"] = [a + b for a, b in zip(ms["gradient"], ms["network"])]
res = {"model": "T = 2^19 base.json shape (models.build_model(log2_hashmap_size=19, H=128))", "device": torch.cuda.get_device_name(0),
       "reps": args.reps, "lattice": f"{N}^3", "iso": args.iso, "h": h, "n_vertices": nv, "refused_vertices": int(refused.sum()),
       "degenerate_vertices": int((~ok & keep_).sum()), "legs": {}}
for name, full in ms.items():
    a = np.array(full[1:] if len(full) > 1 else full)
    res["legs"][name] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4), "ms_max": round(float(a.max()), 4)}
    print(f"{name:17s} {np.median(a):9.4f} ms (min {a.min():.4f}, max {a.max():.4f})", file=sys.stderr, flush=True)
res["mesh_attributes_over_composed"] = round(res["legs"]["mesh_attributes"]["ms_median"] / res["legs"]["composed"]["ms_median"], 4)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
ctx.close()
