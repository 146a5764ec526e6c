"""nrf_density / nrf_density_gradient / nrf_hit_gradients, the parts that need no GPU: the declarations and the bindings, the nine
points_kernel symbols of the built library, and the one text of the definition -- host/points_plan_check.cpp (csrc/nrf_points_plan.h
under AddressSanitizer + UBSan) against tests/points_replay.py, the numpy replay the GPU tests use, bit for bit on random and edge
rows.  Every test here needs the feature: none passes without it."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import nerfhip as nh
import points_replay as pr
import test_ray_hits_cpu as hcpu

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["nrf_density", "nrf_density_gradient", "nrf_hit_gradients"]


# ---------------------------------------------------------------- 1. the declarations
def test_the_header_declares_them_and_the_binding_has_them():
    header = (ROOT / "include" / "nerfhip.h").read_text()
    want = {
        "nrf_density": ["nrf_context* ctx", "const void* xyz", "uint32_t n", "void* sigma_f32", "void* stream"],
        "nrf_density_gradient": ["nrf_context* ctx", "const void* xyz", "uint32_t n", "float h", "void* out_f32x4", "void* stream"],
        "nrf_hit_gradients": ["nrf_context* ctx", "const nrf_frame* hits", "const nrf_rays* rays", "float opacity", "float frac", "float h",
                              "void* pos_f32x4", "void* out_f32x4", "void* stream"],
    }
    lib = nh.load_library()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m is not None, name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want[name], name
        assert name in nh.exported_symbols()
        assert getattr(lib, name).restype is C.c_int
    assert lib.nrf_density_gradient.argtypes[3] is C.c_float
    assert lib.nrf_hit_gradients.argtypes[3:6] == [C.c_float] * 3
    for method in ("density", "density_gradient", "hit_gradients"):
        assert callable(getattr(nh.NerfHip, method))
    assert nh.NRF_ABI_VERSION == 7 == lib.nrf_abi_version()  # additions: no structure changes
    mirror = (ROOT / "nerf-cuda_amd" / "host" / "nerf_render.h").read_text()
    for method in ("density", "density_gradient", "hit_gradients", "normals_from_gradients"):
        assert re.search(r"\b" + method + r"\s*\(", mirror), method


def test_normals_from_gradients():
    rec = np.float32([[3, 0, 4, 7], [0, 0, 0, 5], [0, -2, 0, 1], [1e-30, 0, 0, 0]])
    n = nh.normals_from_gradients(rec)
    assert n.dtype == np.float32 and n.shape == (4, 3)
    assert np.allclose(n[0], [-0.6, 0, -0.8]) and np.all(n[1] == 0) and np.allclose(n[2], [0, 1, 0]) and np.allclose(n[3], [-1, 0, 0])
    assert nh.normals_from_gradients(rec.reshape(2, 2, 4)).shape == (2, 2, 3)


# ---------------------------------------------------------------- 2. the instances
def test_the_library_holds_nine_points_instances(tmp_path):
    found = []
    for name in hcpu._kernel_names(tmp_path):
        m = re.search(r"\bpoints_kernel<([^>]*)>", name)
        if m:
            found.append(tuple(int(a.strip()) for a in m.group(1).split(",")))
    # NET_HOT 0, NET_GENERIC 1, NET_WIDE 2 (nrf_launch.h) x POINTS_VALUE 0, POINTS_GRADIENT 1, POINTS_HIT_GRADIENT 2
    assert sorted(found) == [(net, mode) for net in (0, 1, 2) for mode in (0, 1, 2)], found


# ---------------------------------------------------------------- 3. one text of the definition
def _rows():
    """(x[3], h, bound, o[3], d[3], t, dt, frac) as fp32 [n][14]: random rows, then the edges"""
    rng = np.random.default_rng(20261019)
    F = np.float32
    rows = []
    for bound in (1.0, 4.0, 1.5):
        n = 300
        x = rng.uniform(-1.05 * bound, 1.05 * bound, (n, 3))
        h = bound * rng.choice([2.0 ** -8, 0.003, 2.0 ** -7, 0.1], n)
        o = rng.uniform(-3, 3, (n, 3))
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        t = rng.uniform(0.05, 6, n)
        dt = rng.uniform(0.0034, 0.05, n)
        frac = rng.choice([0.0, 0.5, 1.0, 0.3], n)
        rows.append(np.column_stack([x, h, np.full(n, bound), o, d, t, dt, frac]).astype(np.float32))
    denorm = np.float32(1e-45)
    for bound in (F(1.0), F(4.0)):
        for h in (F(bound * F(2.0 ** -8)), F(F(0.003) * bound), denorm, F(2e-39)):
            up, dn = np.nextafter(bound, F(np.inf)), np.nextafter(bound, F(0))
            for v in (bound, -bound, F(bound - h), F(h - bound), np.nextafter(F(bound - h), F(np.inf)), np.nextafter(F(h - bound), F(-np.inf)),
                      up, -up, dn, -dn, F(np.nan), F(np.inf), F(-np.inf), F(0), F(-0.0), denorm, F(-2) * bound):
                for axis in range(3):
                    x = np.zeros(3, np.float32)
                    x[axis] = v
                    rows.append(np.concatenate([x, [h, bound], x[::-1], [F(1), v, F(0.5)], [v, F(0.01), F(1)]]).astype(np.float32)[None])
    edge = np.concatenate(rows)
    assert edge.shape[1] == 14
    return edge


def test_the_plan_header_and_the_numpy_replay_are_one_definition(tmp_path):
    """host/points_plan_check.cpp (make -C nerf-cuda_amd/host points_asan): a stand-alone program, AddressSanitizer + UBSan, no GPU,
    no library; rows in, taps / guards / hit positions / inv2h out, all as bit patterns"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    host = ROOT / "nerf-cuda_amd" / "host"
    exe = tmp_path / "points_plan_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe), str(host / "points_plan_check.cpp")], check=True)
    rows = _rows()
    text = "\n".join(" ".join(f"{w:08x}" for w in r) for r in pr.bits(rows)) + "\n"
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"points_plan_check: {len(rows)} rows" in out.stderr
    got = [ln.split() for ln in out.stdout.splitlines()]
    assert len(got) == len(rows) and all(len(g) == 30 for g in got)
    taps_got = np.array([[int(w, 16) for w in g[:21]] for g in got], np.uint32).reshape(-1, 7, 3)
    guards_got = np.array([[int(g[21]), int(g[22])] for g in got], bool)
    pos_got = np.array([[int(w, 16) for w in g[23:27]] for g in got], np.uint32)
    inv_got = np.array([int(g[27], 16) for g in got], np.uint32)
    valid_got = np.array([[int(g[28]), int(g[29])] for g in got], bool)
    n_guard_in = n_guard_out = 0
    for i, r in enumerate(rows):
        x, h, bound, o, d, t, dt, frac = r[:3], r[3], r[4], r[5:8], r[8:11], r[11], r[12], r[13]
        assert np.array_equal(taps_got[i], pr.bits(pr.taps(x, h))[0]), (i, r)
        want_guards = [bool(pr.guard(x, h, bound, 1)[0]), bool(pr.guard(x, h, bound)[0])]
        assert list(guards_got[i]) == want_guards, (i, r)
        n_guard_in += want_guards[1]
        n_guard_out += not want_guards[1]
        assert np.array_equal(pos_got[i], pr.bits(pr.hit_position(o, d, t, dt, frac))[0]), (i, r)
        assert inv_got[i] == pr.bits(pr.inv2h(h)).reshape(-1)[0], (i, r)
        with np.errstate(all="ignore"):
            assert list(valid_got[i]) == [bool(h > 0 and h <= bound), bool(0 <= frac <= 1)], (i, r)
    assert n_guard_in > 300 and n_guard_out > 300
    # the definition's own statements, on the replay: +-bound passes the centre's guard and fails the stencil's; +-(bound - h) passes both
    F = np.float32
    for bound in (F(1), F(4)):
        h = F(bound * F(2.0 ** -8))
        for s in (F(1), F(-1)):
            assert pr.guard([s * bound, 0, 0], h, bound, 1)[0] and not pr.guard([s * bound, 0, 0], h, bound)[0]
            assert pr.guard([s * F(bound - h), 0, 0], h, bound)[0]
            assert not pr.guard([s * np.nextafter(bound, F(np.inf)), 0, 0], h, bound, 1)[0]
        for bad in (np.nan, np.inf, -np.inf):
            assert not pr.guard([0, bad, 0], h, bound, 1)[0] and not pr.guard([0, 0, bad], h, bound)[0]
    mk = (host / "Makefile").read_text()
    assert re.search(r"^points_asan: points_plan_check$", mk, re.M)
    rule = mk.split("points_plan_check: points_plan_check.cpp")[1].split("\n# ")[0]
    assert "-fsanitize=address,undefined" in rule and "-ffp-contract=off" in rule
