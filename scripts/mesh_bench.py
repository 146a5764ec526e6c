"""What a mesh extraction costs: nrf_extract_mesh over the aabb of the benchmark's synthetic model (T = 2^19, base.json shape) on
128^3 and 256^3 lattices, split into its three phases, each between two events on the stream the work runs on:

  lattice      nrf_density_lattice: the density network at every lattice point, positions made in the kernel
  density      nrf_density on the same positions uploaded as [n][3] (its nine kernel instances are byte for byte the parent
               commit's: this leg IS the parent's nrf_density) -- the lattice mode reads 12 bytes per point less
  count_scan   launch_mesh_count: the count kernel and the three passes of the two prefix sums
  emit         launch_mesh_emit: vertices and triangles at their offsets
  extract      the whole nrf_extract_mesh call on the given sigmas, host clock (it synchronises twice: the sizes, the flag)

The phases are the library's own launchers (csrc/nrf_launch.h), called through their C++ symbols.  iso is the 0.9 quantile of the
lattice's sigmas: the synthetic model's tables are noise, so its iso-surface is far larger than a trained model's at the same
resolution -- the emit figure is an upper bound of a sort.  Before timing, the lattice leg is held to the density leg bit for bit
and the mesh of the phases to nrf_extract_mesh's.  Median, minimum and maximum over the repetitions without the first; one JSON object.

Run it under a time limit:   timeout -k 10 300 python3 scripts/mesh_bench.py [--reps 21] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nerf-cuda_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch  # noqa: E402
import models, nerfhip as nh, synthetic as syn  # noqa: E402
import mesh_replay as mr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
ap.add_argument("--out", default=None)
args = ap.parse_args()

desc, keep, _ = models.build_model(log2_hashmap_size=19, H=128)
bound = float(desc.bound)
ctx = nh.NerfHip(0)
ctx.load_model(desc)
lib = ctx.lib
count = getattr(lib, "_ZN3nrf17launch_mesh_countERKNS_11MeshLatticeEPKffPjS5_S5_PvS5_P12ihipStream_t")
count.restype, count.argtypes = C.c_int, [C.POINTER(nh.Lattice), C.c_void_p, C.c_float] + [C.c_void_p] * 6
emit = getattr(lib, "_ZN3nrf16launch_mesh_emitERKNS_11MeshLatticeEPKffPKjS6_S6_jjPfPjS8_P12ihipStream_t")
emit.restype, emit.argtypes = C.c_int, [C.POINTER(nh.Lattice), C.c_void_p, C.c_float] + [C.c_void_p] * 3 + [C.c_uint32] * 2 + [C.c_void_p] * 4
stream = torch.cuda.Stream()
sp = stream.cuda_stream
assert sp != 0
clock = None
try:  # the shader clock the library reports with a frame's statistics
    ctx.set_resolution(64, 64)
    ctx.render(syn.default_camera(64, 64), syn.orbit_pose(30, 30))
    clock = float(ctx.stats().shader_clock_mhz)
except Exception as e:  # noqa: BLE001
    print(f"no clock: {e}", file=sys.stderr)

res = {"model": "T = 2^19 base.json shape (models.build_model(log2_hashmap_size=19, H=128))", "reps": args.reps, "shader_clock_mhz": clock,
       "device": torch.cuda.get_device_name(0), "sizes": {}}
for N in args.sizes:
    n = N ** 3
    cell = float(np.float32(2.0 * bound / (N - 1)))
    lat = nh.Lattice.make([-bound] * 3, [cell] * 3, (N, N, N))
    xyz = torch.from_numpy(mr.positions([-bound] * 3, [cell] * 3, (N, N, N)).reshape(-1, 3)).cuda()
    sigma, sigma2 = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    codes, vbase, tbase = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    partials = torch.empty(2 * ((n + 2047) // 2048), dtype=torch.int32, device="cuda")
    totals = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.density_lattice(lat, sigma.data_ptr())
    ctx.density(xyz.data_ptr(), n, sigma2.data_ptr())
    assert torch.equal(sigma.view(torch.int32), sigma2.view(torch.int32)), "lattice against density"
    iso = float(torch.quantile(sigma[:: max(1, n // 1000000)], 0.9))
    m = ctx.extract_mesh(lat, iso, sigma.data_ptr())
    nv, nt = int(m.n_vertices), int(m.n_triangles)
    v_ref, t_ref = ctx.read_mesh()
    vertices, triangles = torch.empty((max(nv, 1), 3), device="cuda"), torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def count_scan():
        assert count(C.byref(lat), sigma.data_ptr(), iso, codes.data_ptr(), vbase.data_ptr(), tbase.data_ptr(), partials.data_ptr(),
                     totals.data_ptr(), sp) == 0

    def emit_():
        assert emit(C.byref(lat), sigma.data_ptr(), iso, codes.data_ptr(), vbase.data_ptr(), tbase.data_ptr(), nv, nt, vertices.data_ptr(),
                    triangles.data_ptr(), totals.data_ptr() + 8, sp) == 0

    count_scan()
    emit_()
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [nv, nt, 0, 0], (totals.cpu().tolist(), nv, nt)
    assert np.array_equal(vertices[:nv].cpu().numpy().view(np.uint32), v_ref.view(np.uint32)), "the phases' vertices against nrf_extract_mesh's"
    assert np.array_equal(triangles[:nt].cpu().numpy().view(np.uint32), t_ref), "the phases' triangles against nrf_extract_mesh's"
    legs = {"lattice": lambda: ctx.density_lattice(lat, sigma.data_ptr(), stream=sp),
            "density": lambda: ctx.density(xyz.data_ptr(), n, sigma2.data_ptr(), stream=sp), "count_scan": count_scan, "emit": emit_}
    ms = {k: [] for k in list(legs) + ["extract"]}
    for _ in range(args.reps):
        for name, run in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                run()
                e1.record(stream)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.extract_mesh(lat, iso, sigma.data_ptr(), stream=sp)
        ms["extract"].append((time.perf_counter() - t0) * 1e3)
    out = {"points": n, "iso": iso, "n_vertices": nv, "n_triangles": nt, "legs": {}}
    for name, full in ms.items():
        a = np.array(full[1:] if len(full) > 1 else full)
        out["legs"][name] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4), "ms_max": round(float(a.max()), 4)}
        print(f"{N}^3 {name:10s} {np.median(a):9.4f} ms (min {a.min():.4f}, max {a.max():.4f})", file=sys.stderr, flush=True)
    d = out["legs"]["density"]
    out["density_spread"] = round((d["ms_max"] - d["ms_min"]) / d["ms_median"], 4)
    out["lattice_over_density"] = round(out["legs"]["lattice"]["ms_median"] / d["ms_median"], 4)
    res["sizes"][f"{N}^3"] = out
    del xyz, sigma, sigma2, codes, vbase, tbase, partials, vertices, triangles
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
ctx.close()
