#!/usr/bin/env python3
"""Generates tests/golden/reference_kernels.npz: outputs of the REFERENCE's own kernels, compiled for the CPU.

Made by oracle/_ref/libref_kernels.so (oracle/ref_kernels.cpp: the reference's render_utils.h unchanged, behind stand-in
headers), not by the oracle: these are the vectors tests/test_reference_kernels_gpu.py holds the HIP stage entry points to on
a machine that has neither the reference tree nor that library.  Data only: inputs and recorded results.

Per march geometry (GEOMETRIES; two of them a second time over a speckled density grid) one 48 x 40 frame, thinned to every STRIDE-th ray (`<name>/index` holds the ray numbers):
  cam, W, H, model keywords (meta, JSON); per geometry the pose and the FNV-1a hash of the density grid's bytes
  rays_o, rays_d, nears, fars                                   (set_rays_o / set_rays_d, both devices' halves; near / far)
  xyzs<k>, dirs<k>, deltas<k> for n_step k = 1, 3, 8            (kernel_march_rays, first round; buffers pre-zeroed: D-1)
  p01, d01                                                      (linear_transformer on xyzs1 / dirs1: the network's inputs)
  two chained march + composite calls of 8 slots on synthetic sigmas and colours (composite_inputs below, integers only,
  so that the test rebuilds them without a random generator): t1, state1; the survivors `keep2`, their second march
  deltas2 (from t1), t2, state2                                 (kernel_composite_rays)

The writer fixes every zip member's date so that the same vectors give the same members; the regeneration test
(tests/test_reference_kernels_cpu.py) compares member names and every member's .npy bytes.
Run from the repo root, after `make -C oracle ref`:  python tests/golden/make_reference_golden.py
"""
import io
import json
import sys
import zipfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "nerf-cuda_amd"), str(ROOT / "tests")]

W, H = 48, 40
STRIDE = 16   # every 16th ray, starting at ray 5: 120 of 1 920
FIRST = 5
AZIMUTH, ELEVATION = 45, 25
RADIUS_NEAR, RADIUS_FAR = 4.0311, 9.0  # a model with outer cascades is seen from 2.97 ngp units: the march starts outside cascade 0
MIN_NEAR, DT_GAMMA = 0.2, 1.0 / 128
GEOMETRIES = {
    "h32": dict(H=32, bound=1.0, cascade=1),
    "h32-b4-c3": dict(H=32, bound=4.0, cascade=3),
    "h30": dict(H=30, bound=1.0, cascade=1),
    "h64-b1.5-c2": dict(H=64, bound=1.5, cascade=2),
    "h32-b4-c3-speckle": dict(H=32, bound=4.0, cascade=3),   # the same models over speckle_grid: every cascade emits samples
    "h64-b1.5-c2-speckle": dict(H=64, bound=1.5, cascade=2),
}


def grid_hash(grid) -> np.uint64:
    """FNV-1a (64 bit) over the bytes of the fp32 density grid"""
    import oracle_py as op

    return np.uint64(op.fnv1a(np.ascontiguousarray(grid, np.float32)))


def mix64(i):
    """splitmix64's finaliser on uint64 values: integers only, the same wherever it runs"""
    z = (np.asarray(i, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def unit24(i):
    """fp32 values in [0, 1) from the top 24 bits of mix64: exact"""
    return (mix64(i) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def speckle_grid(n_cells, salt):
    """A density grid in which every cell of every cascade is occupied (1.0) with probability 1/6.  The synthetic scene occupies
    cascade 0 only: over it a wrong cell lookup or hop in an outer cascade finds the same empty space and shows nowhere."""
    return (unit24(np.arange(n_cells, dtype=np.uint64) + np.uint64(salt << 32)) < np.float32(1.0 / 6)).astype(np.float32)


def build(name):
    """(desc, keepalive) of a GEOMETRIES row; a name ending in -speckle swaps the scene's density grid for speckle_grid"""
    import models
    import nerfhip as nh

    kw = GEOMETRIES[name]
    desc, keep, cfg = models.build_model(log2_hashmap_size=12, **kw)
    if name.endswith("-speckle"):
        desc, keep = nh.desc_from_config(cfg, keep[0], speckle_grid(keep[1].size, kw["H"] + kw["cascade"]))
    return desc, keep


def composite_inputs(n, call):
    """sigmas [n][8] in [0, 40) (call 0: thin, so that rays survive eight slots) or [0, 400) (call 1) and colours [n][8][3] in
    [0, 1), from mix64 of the slot number -- the same values wherever they are rebuilt"""
    unit = unit24(np.arange(n * 8 * 4, dtype=np.uint64).reshape(n, 8, 4) + np.uint64((call + 1) << 40))
    sig = unit[:, :, 0] * np.float32(40.0 if call == 0 else 400.0)
    return np.ascontiguousarray(sig, np.float32), np.ascontiguousarray(unit[:, :, 1:], np.float32)


def vectors():
    import models
    import nerfhip as nh
    import oracle_py as op
    import ref_kernels_py as rk
    import synthetic as syn

    rk.lib()
    cam = syn.default_camera(W, H)
    out = {"cam": cam,
           "meta": np.frombuffer(json.dumps({"W": W, "H": H, "stride": STRIDE, "first": FIRST, "min_near": MIN_NEAR,
                                             "dt_gamma": DT_GAMMA, "log2_hashmap_size": 12, "geometries": GEOMETRIES},
                                            sort_keys=True).encode(), np.uint8)}
    index = np.arange(FIRST, W * H, STRIDE)
    for name, kw in GEOMETRIES.items():
        desc, keep = build(name)
        geo = rk.Geometry(desc)
        pose = syn.orbit_pose(AZIMUTH, ELEVATION, radius=RADIUS_FAR if kw["cascade"] > 1 else RADIUS_NEAR)
        ro, rd, nr, fr = rk.frame_rays(cam, pose, geo, W, H, MIN_NEAR)
        ro, rd, nr, fr = ro[index], rd[index], nr[index], fr[index]
        n = len(index)
        g = {"index": index.astype(np.int32), "pose": pose, "grid_hash": grid_hash(geo.grid), "rays_o": ro, "rays_d": rd, "nears": nr, "fars": fr}
        for n_step in (1, 3, 8):
            g[f"xyzs{n_step}"], g[f"dirs{n_step}"], g[f"deltas{n_step}"] = rk.march_first_round(geo, ro, rd, nr, fr, n_step, DT_GAMMA)
        g["p01"], g["d01"] = rk.normalise(geo.bound, g["xyzs1"], g["dirs1"])
        sig, rgb = composite_inputs(n, 0)
        g["t1"], g["state1"] = rk.composite(sig, rgb, g["deltas8"], nr, np.zeros((n, 5), np.float32))
        keep2 = np.flatnonzero(g["t1"] >= 0)
        g["keep2"] = keep2.astype(np.int32)
        g["deltas2"] = rk.march_first_round(geo, ro[keep2], rd[keep2], g["t1"][keep2], fr[keep2], 8, DT_GAMMA)[2]
        sig, rgb = composite_inputs(len(keep2), 1)
        g["t2"], g["state2"] = rk.composite(sig, rgb, g["deltas2"], g["t1"][keep2], g["state1"][keep2])
        for k, v in g.items():
            out[f"{name}/{k}"] = v
    return out


def members(arrays):
    """[(member name, .npy bytes)] in insertion order"""
    res = []
    for k, v in arrays.items():
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.ascontiguousarray(v), version=(1, 0), allow_pickle=False)
        res.append((k + ".npy", buf.getvalue()))
    return res


def write(path):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, data in members(vectors()):
            info = zipfile.ZipInfo(name, date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, data, compresslevel=9)


def read_members(path):
    with zipfile.ZipFile(path) as z:
        return [(i.filename, z.read(i)) for i in z.infolist()]


if __name__ == "__main__":
    target = Path(__file__).with_name("reference_kernels.npz")
    write(target)
    print(f"wrote {target.name}: {target.stat().st_size} bytes")
