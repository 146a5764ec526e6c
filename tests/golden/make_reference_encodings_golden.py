#!/usr/bin/env python3
"""Generates tests/golden/reference_encodings.npz: outputs of the REFERENCE's own encoding kernels, compiled for the CPU.

Made by oracle/_ref/libref_encodings.so (oracle/ref_encodings.cpp: tiny-cuda-nn's grid.h, spherical_harmonics.h, frequency.h,
identity.h and common_device.h unchanged, behind stand-in headers), not by the oracle: these are the rows
tests/test_reference_encodings_gpu.py holds nrf_encode_grid / nrf_encode_dir / nrf_network / nrf_density to on a machine that
has neither the reference tree nor that library.  Data only: inputs, model keywords and recorded results.

This module also DEFINES the model matrix of tests/test_reference_encodings_cpu.py (GRID_MODELS, DIR_MODELS) and its inputs
(positions(), directions()); the fixture records a subset (FIXTURE_GRID, FIXTURE_DIR, N_DIR) and stores seeds and hashes, not
tables: a model is rebuilt from its keywords, and `table_fnv1a` tells a drifting generator from a wrong kernel.

  meta (JSON)                 per model: the build_model keywords, FNV-1a of the grid table's fp16 bits, the constructor's offsets and
                              resolutions, the first hashed level, the stage instance the device-free plan selects
  pos [264][3]                256 random points of [0, 1]^3 and the edge list of test_encode_grid_bit_exact
  grid/<model> [264][padded]  kernel_grid<__half, 3, F> + transpose_encoded_position, fp16 bits
  dir [N_DIR][3]              directions mapped to [0, 1]
  dir/<model> [N_DIR][padded] kernel_sh / frequency_encoding / identity, fp16 bits, padding included
  net_xyz, net_dir [128][3]   world positions and directions (multiples of 2^-12, so that x / 2 + 1 / 2 is exact whichever way the
                              device evaluates it) for the models of NET_MODELS
  net_grid/<model>, net_dir/<model>   the kernels' rows of those points' normalised coordinates

Run from the repo root, after `make -C oracle ref`:  python tests/golden/make_reference_encodings_golden.py
"""
import ctypes as C
import json
import io
import sys
import zipfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "nerf-cuda_amd"), str(ROOT / "tests")]


# Every model has H = 32 (the density grid plays no part).  The first row is the reference's own configuration
# (R/configs/nerf/base.json through R/include/nerf-cuda/nerf_network.h:95-135: L = 16, F = 2, T = 2^19, Nmin = 16, Linear, derived
# scale); the others are named for what they add.
GRID_MODELS = {
    "reference": dict(),
    "t12": dict(log2_hashmap_size=12),                                                  # dense and hashed levels in one model
    "t12-smoothstep": dict(log2_hashmap_size=12, interpolation="Smoothstep"),
    "t12-nearest": dict(log2_hashmap_size=12, interpolation="Nearest"),
    "t12-wide": dict(log2_hashmap_size=12, dir_otype="Frequency", n_frequencies=4),     # the wide instance family
    "f1-l16": dict(log2_hashmap_size=12, n_features_per_level=1),
    "f1-l5": dict(log2_hashmap_size=12, n_features_per_level=1, n_levels=5),            # F L = 5: padded to 16
    "f4-l3-smoothstep": dict(log2_hashmap_size=12, n_features_per_level=4, n_levels=3, interpolation="Smoothstep"),  # 12 -> 16
    "f8-l5-nearest": dict(log2_hashmap_size=12, n_features_per_level=8, n_levels=5, interpolation="Nearest"),        # 40 -> 48
    "f8-l3": dict(log2_hashmap_size=14, n_features_per_level=8, n_levels=3),            # 24 -> 32
    "dense-l3": dict(grid_type="Dense", n_levels=3, base_resolution=8, per_level_scale=2.0),  # 6 -> 16
    "tiled-2048": dict(grid_type="Tiled"),                                              # top resolution 2048: res^3 = 2^33
    "scale2-l8": dict(log2_hashmap_size=12, n_levels=8, per_level_scale=2.0),           # exp2f exact; top resolution 2048
    "scale1.5-l9": dict(log2_hashmap_size=15, n_levels=9, per_level_scale=1.5, base_resolution=5),
}
FIRST_HASHED = {"reference": 5, "t12": 1}  # asserted in the CPU test: 23^3 > 2^12 >= 16^3; 112^3 > 2^19 >= 81^3

DIR_MODELS = {**{f"sh{d}": dict(sh_degree=d) for d in range(1, 9)},
              **{f"frequency{n}": dict(dir_otype="Frequency", n_frequencies=n) for n in range(1, 7)},
              "identity": dict(dir_otype="Identity")}
DIR_GRID = dict(log2_hashmap_size=4, n_levels=2, base_resolution=2)  # the smallest grid: only the direction encoding matters

FIXTURE_GRID = list(GRID_MODELS)
FIXTURE_DIR = ["sh1", "sh2", "sh3", "sh4", "sh6", "sh8", "frequency1", "frequency2", "frequency4", "frequency6", "identity"]
NET_MODELS = ["reference", "t12-wide", "f4-l3-smoothstep"]
N_DIR = 160

EDGE = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0.5], [0.5, 1, 0], [0.25, 0.5, 0.75], [1 - 2 ** -24, 2 ** -24, 0.5],
                 [0.5, 0.5, 0.5], [1 / 3, 2 / 3, 1.0]], np.float32)  # tests/test_parity_gpu.py::test_encode_grid_bit_exact


def positions():
    """264 points of [0, 1]^3: the edge list, then 256 random ones"""
    return np.concatenate([EDGE, np.random.default_rng(20).random((256, 3), dtype=np.float32)])


def directions(n=4096):
    """n directions mapped to [0, 1]: the axes, the diagonals and the centre first, then unit vectors"""
    axes = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    diag = [[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    special = np.array(axes + diag, np.float32)
    special /= np.linalg.norm(special, axis=1, keepdims=True).astype(np.float32)
    d = np.random.default_rng(21).normal(size=(n - len(special) - 1, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.concatenate([special, d]).astype(np.float32)
    d01 = d * np.float32(0.5) + np.float32(0.5)
    return np.concatenate([d01, np.full((1, 3), 0.5, np.float32)]).astype(np.float32)


def network_points(n=128):
    """(xyz, dirs) in world coordinates, bound 1: multiples of 2^-12 inside (-1, 1), the directions near unit length"""
    rng = np.random.default_rng(22)
    xyz = (rng.integers(-4095, 4096, (n, 3)) / 4096.0).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return xyz, (np.round(d * 4096.0) / 4096.0).astype(np.float32)


def normalised(v):
    """linear_transformer with weight 1 / (2 bound), bias 0.5 at bound 1 (R/src/nerf_render.cu:311-314): exact for network_points"""
    return (np.asarray(v, np.float32) * np.float32(0.5) + np.float32(0.5)).astype(np.float32)


_models = {}


def build(name):
    """(desc, keepalive) of a GRID_MODELS / DIR_MODELS row, built once"""
    if name not in _models:
        import models

        kw = GRID_MODELS[name] if name in GRID_MODELS else {**DIR_GRID, **DIR_MODELS[name]}
        desc, keep, _ = models.build_model(H=32, **kw)
        _models[name] = (desc, keep)
    return _models[name]


def table_f16(desc, keep, offsets):
    """the grid's parameters as the network stores them: the tail of the fp32 blob, cast to fp16 (nerf_network.h:434-436)"""
    n = int(offsets[-1]) * int(desc.n_features_per_level)
    return np.ascontiguousarray(keep[0][-n:].astype(np.float16)).view(np.uint16)


def padded16(n):
    return (n + 15) // 16 * 16


def dir_kind(desc):
    """(kind, arg, raw width) for ref_kernels_py.encode_dir"""
    kind = int(desc.dir_encoding)
    arg = int(desc.sh_degree) if kind == 0 else int(desc.n_frequencies) if kind == 1 else 0
    return kind, arg, {0: arg * arg, 1: 6 * arg, 2: 3}[kind]


def reference_grid(name, pos01):
    """(rows, info) of a grid model: the reference's constructor makes the table geometry, its kernels the rows"""
    import oracle_py as op
    import ref_kernels_py as rk

    desc, keep = build(name)
    F, L = int(desc.n_features_per_level), int(desc.n_levels)
    made = rk.grid_table(F, L, int(desc.log2_hashmap_size), int(desc.base_resolution), float(desc.per_level_scale), int(desc.grid_type))
    assert made is not None, f"{name}: the reference's constructor refuses this model"
    offsets, res, _ = made
    table = table_f16(desc, keep, offsets)
    rows = rk.grid_encode(desc, offsets, table, pos01, padded16(F * L))
    sizes = np.diff(offsets.astype(np.int64))
    hashed = [int(l) for l in range(L) if int(desc.grid_type) == 0 and int(res[l]) ** 3 > sizes[l]]
    info = dict(table_fnv1a=f"{op.fnv1a(table):016x}", offsets=[int(v) for v in offsets], resolutions=[int(v) for v in res],
                first_hashed=hashed[0] if hashed else None)
    return rows, info


def reference_dir(name, d01):
    import ref_kernels_py as rk

    kind, arg, raw = dir_kind(build(name)[0])
    return rk.encode_dir(kind, arg, d01, padded16(raw))


def stage_code(desc):
    """nrf_debug_rays_instance's code of the stage instance the device-free plan selects: 0 register-resident, 1 generic, 2 wide"""
    import nerfhip as nh

    lib = nh.load_library()
    lib.nrf_debug_plan.argtypes, lib.nrf_debug_plan.restype = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint32)], C.c_int
    out = (C.c_uint32 * 6)()
    assert lib.nrf_debug_plan(C.byref(desc), 1, 1, out) == nh.NRF_OK
    return {0: 0, 1: 1, 2: 2}[int(out[1])]  # NET_HOT, NET_GENERIC, NET_WIDE


def vectors():
    pos, d01 = positions(), directions()[-N_DIR:]  # (the tail: random unit vectors and the centre) ...
    d01 = np.concatenate([directions()[:14], d01])  # ... behind the axes and diagonals
    xyz, dirs = network_points()
    v = {"pos": pos, "dir": d01, "net_xyz": xyz, "net_dir": dirs}
    meta = {"grid": {}, "dir": {}, "net": NET_MODELS}
    for name in FIXTURE_GRID:
        rows, info = reference_grid(name, pos)
        v[f"grid/{name}"] = rows
        meta["grid"][name] = dict(kw=GRID_MODELS[name], stage=stage_code(build(name)[0]), **info)
    for name in FIXTURE_DIR:
        v[f"dir/{name}"] = reference_dir(name, d01)
        meta["dir"][name] = dict(kw={**DIR_GRID, **DIR_MODELS[name]})
    for name in NET_MODELS:
        v[f"net_grid/{name}"], _ = reference_grid(name, normalised(xyz))
        kind, arg, raw = dir_kind(build(name)[0])
        import ref_kernels_py as rk

        v[f"net_dir/{name}"] = rk.encode_dir(kind, arg, normalised(dirs), padded16(raw))
    v["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    return v


def members(v):
    for name in sorted(v):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.ascontiguousarray(v[name]), version=(1, 0), allow_pickle=False)
        yield name + ".npy", buf.getvalue()


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
    target = Path(__file__).with_name("reference_encodings.npz")
    write(target)
    print(f"wrote {target.name}: {target.stat().st_size} bytes")
