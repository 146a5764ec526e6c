"""nrf_point_attributes / nrf_mesh_attributes / nrf_read_mesh_attributes, the parts that need no GPU: the declarations and the bindings,
the six attr_kernel symbols of the built library, the one text of the definition -- host/attr_plan_check.cpp (csrc/nrf_attr_plan.h,
plain and under AddressSanitizer + UBSan through `make attr_asan`) against tests/attr_replay.py, the numpy replay the GPU tests use,
bit for bit on random and edge rows -- and NerfRender::save_ply's bytes.  Every test here needs the feature: none passes without it."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import attr_replay as ar
import nerfhip as nh
import test_ray_hits_cpu as hcpu

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nerf-cuda_amd" / "host"
F = np.float32
NAMES = ["nrf_point_attributes", "nrf_mesh_attributes", "nrf_read_mesh_attributes"]


# ---------------------------------------------------------------- 1. the declarations
def test_the_header_declares_them_and_the_binding_has_them():
    header = (ROOT / "include" / "nerfhip.h").read_text()
    want = {
        "nrf_point_attributes": ["nrf_context* ctx", "const void* xyz", "const void* dir", "uint32_t n", "float h", "void* normal_f32x4",
                                 "void* color_f32x4", "void* stream"],
        "nrf_mesh_attributes": ["nrf_context* ctx", "float h", "void* stream", "nrf_mesh_attr* out"],
        "nrf_read_mesh_attributes": ["nrf_context* ctx", "float* normals_f32x4", "float* colors_f32x4"],
    }
    lib = nh.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(nh.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(nrf_[a-z0-9_]+)\b", out))
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m is not None, name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want[name], name
        assert name in nh.exported_symbols() and name in exported
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(want[name]), name
    assert lib.nrf_point_attributes.argtypes[4] is C.c_float and lib.nrf_mesh_attributes.argtypes[1] is C.c_float
    assert re.search(r"typedef struct nrf_mesh_attr \{\s*uint64_t n_vertices;\s*void\* normals;[^}]*void\* colors;[^}]*\} nrf_mesh_attr;", header)
    assert [f[0] for f in nh.MeshAttr._fields_] == ["n_vertices", "normals", "colors"] and C.sizeof(nh.MeshAttr) == 24
    for method in ("point_attributes", "mesh_attributes", "read_mesh_attributes"):
        assert callable(getattr(nh.NerfHip, method))
    assert nh.NRF_ABI_VERSION == 7 == lib.nrf_abi_version()  # additions: no structure changes
    mirror = (HOST / "nerf_render.h").read_text()
    for method in ("mesh_attributes", "save_ply", "save_obj", "normals_from_gradients"):
        assert re.search(r"\b" + method + r"\s*\(", mirror), method


def test_the_library_holds_six_attr_instances(tmp_path):
    found = []
    for name in hcpu._kernel_names(tmp_path):
        m = re.search(r"\battr_kernel<([^>]*)>", name)
        if m:
            found.append(tuple(int(a.strip()) for a in m.group(1).split(",")))
    # NET_HOT 0, NET_GENERIC 1, NET_WIDE 2 (nrf_launch.h) x the direction from the normal 0, given 1
    assert sorted(found) == [(net, dirs) for net in (0, 1, 2) for dirs in (0, 1)], found


# ---------------------------------------------------------------- 2. one text of the definition
def _rows():
    """gradient triples as fp32 [n][3]: random ones over the whole exponent range, then the edges"""
    rng = np.random.default_rng(20261019)
    n = 9000
    # every exponent of a float from the denormals to the last binade, random mantissas and signs
    e = rng.integers(-149, 128, (n, 3)).astype(np.float64)
    rand = (rng.choice([-1.0, 1.0], (n, 3)) * rng.uniform(1.0, 2.0, (n, 3)) * 2.0 ** e).astype(np.float32)
    # ... and rows whose three components are of one magnitude (the rows above mostly have one dominant component)
    e1 = rng.integers(-70, 64, (1000, 1)).astype(np.float64)
    near = (rng.normal(size=(1000, 3)) * 2.0 ** e1).astype(np.float32)
    special = [F(0), F(-0.0), F(1e-45), F(-1e-45), F(1e-39), F(np.inf), F(-np.inf), F(np.nan), F(1), F(-3), F(2.0 ** -31), F(3e38)]
    edge = [[a, b, c] for a in special for b in (F(0), F(-0.0), F(1), F(2.0 ** -30), F(np.nan), F(np.inf)) for c in (F(0), F(-2), F(1e-45))]
    # l2 just below and just at 2^-60: one component of 2^-30 (l2 = 2^-60 exactly) and its neighbours; two and three components
    p = F(2.0 ** -30)
    lo, hi = np.nextafter(p, F(0)), np.nextafter(p, F(1))
    for v in (p, lo, hi, -p, -lo, -hi):
        for axis in range(3):
            r = [F(0)] * 3
            r[axis] = v
            edge.append(r)
    s2, s3 = F(2.0 ** -30.5), F(2.0 ** -30) / F(np.sqrt(3.0))
    for v in (s2, np.nextafter(s2, F(0)), np.nextafter(s2, F(1))):
        edge += [[v, v, F(0)], [F(0), -v, v], [v, F(-0.0), v]]
    for v in (s3, np.nextafter(s3, F(0)), np.nextafter(s3, F(1))):
        edge.append([v, -v, v])
    # squares that overflow (2^64 squared is 2^128), singly and in the sums; the largest that do not
    big = F(2.0 ** 64)
    for v in (big, np.nextafter(big, F(0)), F(2.0 ** 63.4), F(2.0 ** 63.6), F(3.4e38)):
        edge += [[v, F(0), F(0)], [F(1), -v, F(1)], [v, v, F(0)], [v, v, v], [F(0), F(0), -v]]
    rows = np.concatenate([rand, near, np.array(edge, np.float32)])
    return rows


def _run(exe, rows):
    text = "\n".join(" ".join(f"{w:08x}" for w in r) for r in ar.bits(rows)) + "\n"
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"attr_plan_check: {len(rows)} rows" in out.stderr
    got = [ln.split() for ln in out.stdout.splitlines()]
    assert len(got) == len(rows) and all(len(g) == 14 for g in got)
    words = np.array([[int(w, 16) for w in g[:7] + g[8:11]] for g in got], np.uint32)
    ok = np.array([int(g[7]) for g in got], bool)
    c8 = np.array([[int(w) for w in g[11:14]] for g in got], np.uint8)
    return words, ok, c8


def test_the_plan_header_and_the_numpy_replay_are_one_definition(tmp_path):
    """host/attr_plan_check.cpp, a stand-alone program (no GPU, no library): gradient triples in, (n, len, d), the direction inputs and
    the 8-bit values out, all held to tests/attr_replay.py bit for bit -- built plainly, and once more through `make attr_asan`
    (AddressSanitizer + UBSan) in a copy of the two directories the rule needs.
    The unit-length bound, derived: with u = 2^-24, l2 carries at most 3u of relative error (a product and two sums on its longest
    path), the square root halves that and adds u, the division adds u: each component carries at most 3.5u, so the squared norm at
    most 7u plus second-order terms: | |n|^2 - 1 | <= 8 * 2^-24 in float64."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rows = _rows()
    assert 9500 <= len(rows) <= 12000
    want_n, want_len, want_d, want_ok = ar.direction(rows)
    want = np.concatenate([ar.bits(want_n), ar.bits(want_len)[:, None], ar.bits(want_d), ar.bits(ar.dir01(want_d))], axis=1)
    want_c8 = ar.color_u8(rows)
    # both kinds are well represented, and the edges fall on both sides
    assert want_ok.sum() > 3000 and (~want_ok).sum() > 3000
    p = F(2.0 ** -30)
    assert ar.direction([[p, 0, 0]])[3][0] and not ar.direction([[np.nextafter(p, F(0)), 0, 0]])[3][0]
    assert not ar.direction([[F(2.0 ** 64), 0, 0]])[3][0] and ar.direction([[np.nextafter(F(2.0 ** 64), F(0)), 0, 0]])[3][0]
    deg = ar.direction([[0, -0.0, np.nan], [-1e-45, 0, 0], [np.inf, 1, 1]])
    assert not deg[3].any() and np.all(ar.bits(deg[0]) == 0) and np.all(ar.bits(deg[1]) == 0) and np.all(ar.bits(deg[2]) == 0)
    assert list(ar.color_u8(F([np.nan, -1, 0, 0.5, 1, 2, np.inf, -np.inf, 0.999, 1 / 255]))) == [0, 0, 0, 127, 255, 255, 255, 0, 254, 1]
    # the plain build
    plain = tmp_path / "attr_plan_check"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-o", str(plain), str(HOST / "attr_plan_check.cpp")], check=True)
    # the sanitizer build, through the Makefile's own rule
    work = tmp_path / "tree" / "nerf-cuda_amd"
    (work / "host").mkdir(parents=True)
    (work / "csrc").mkdir()
    for rel in ("host/Makefile", "host/attr_plan_check.cpp", "csrc/nrf_attr_plan.h", "csrc/nrf_points_plan.h"):
        shutil.copy(ROOT / "nerf-cuda_amd" / rel, work / rel)
    r = subprocess.run(["make", "-C", str(work / "host"), "attr_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "-fsanitize=address,undefined" in r.stdout and "-ffp-contract=off" in r.stdout and "attr_plan_check: 4 rows" in r.stderr + r.stdout
    for exe in (plain, work / "host" / "attr_plan_check"):
        words, ok, c8 = _run(exe, rows)
        bad = np.nonzero(np.any(words != want, axis=1) | (ok != want_ok) | np.any(c8 != want_c8, axis=1))[0]
        assert len(bad) == 0, (exe.name, len(bad), rows[bad[:5]], words[bad[:5]], want[bad[:5]])
    # unit length
    err = ar.norm_error(want_n[want_ok])
    print(f"{want_ok.sum()} non-degenerate rows of {len(rows)}: max | |n|^2 - 1 | = {err.max() / 2.0 ** -24:.3f} x 2^-24")
    assert np.all(err <= ar.NORM_BOUND)
    mk = (HOST / "Makefile").read_text()
    assert re.search(r"^attr_asan: attr_plan_check$", mk, re.M)


# ---------------------------------------------------------------- 3. the PLY writer
_PLY_PROGRAM = r"""
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>
#include "nerf_render.h"
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const std::vector<float> vertices = {0.f, 0.f, 0.f, 1.f, 0.f, -0.f, 1.f, 1.f, 0.25f, 0.f, 1.5f, 1e-40f};
  const std::vector<uint32_t> triangles = {0, 1, 2, 0, 2, 3};
  const std::vector<float> normals = {0.f, 0.f, 1.f, -0.f, 0.6f, 0.8f, 0.f, 0.f, 0.f, -1.f, 0.f, 0.f};
  const std::vector<float> colors = {0.f, 0.5f, 1.f, nan, -1.f, 2.f, 0.999f, 0.003921569f, inf, 0.2f, 0.7f, -inf};
  if (!ngp::NerfRender::save_ply(argv[1], vertices, triangles, normals, colors)) return 3;
  if (ngp::NerfRender::save_ply(std::string(argv[1]) + ".bad", vertices, triangles, normals, std::vector<float>(9))) return 4;  // one colour short
  if (!ngp::NerfRender::save_ply(std::string(argv[1]) + ".empty", {}, {}, {}, {})) return 5;
  return 0;
}
"""


def parse_ply(data: bytes):
    """the numpy parser of the PLY files save_ply writes: (vertices [n][3], normals [n][3], colours u8 [n][3], triangles [m][3]); it
    checks the header's text and the byte count"""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0" and head[-1] == "end_header"
    nv = int(re.fullmatch(r"element vertex (\d+)", head[2]).group(1))
    assert head[3:12] == [f"property float {k}" for k in ("x", "y", "z", "nx", "ny", "nz")] + [f"property uchar {k}" for k in ("red", "green", "blue")]
    nt = int(re.fullmatch(r"element face (\d+)", head[12]).group(1))
    assert head[13] == "property list uchar int vertex_indices" and len(head) == 15
    assert len(data) == end + 27 * nv + 13 * nt, (len(data), end, nv, nt)
    vt = np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
    ft = np.dtype([("k", "u1"), ("idx", "<i4", 3)])
    assert vt.itemsize == 27 and ft.itemsize == 13
    v = np.frombuffer(data, vt, nv, end)
    f = np.frombuffer(data, ft, nt, end + 27 * nv)
    assert np.all(f["k"] == 3)
    return v["xyz"].reshape(nv, 3), v["n"].reshape(nv, 3), v["rgb"].reshape(nv, 3), f["idx"].reshape(nt, 3)


def test_save_ply_writes_what_the_parser_reads(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None or not (HOST / "libngp_hip.so").exists():
        pytest.skip("the C++ host mirror is not built")
    src, exe, ply = tmp_path / "ply.cpp", tmp_path / "ply", tmp_path / "two.ply"
    src.write_text(_PLY_PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(HOST), "-I", str(ROOT / "include"), "-o", str(exe), str(src), f"-L{HOST}", "-lngp_hip",
                    f"-L{HOST.parent}", "-lnerfhip", f"-Wl,-rpath,{HOST}", f"-Wl,-rpath,{HOST.parent}"], check=True)
    r = subprocess.run([str(exe), str(ply)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    v, n, rgb, t = parse_ply(ply.read_bytes())
    nan, inf = np.nan, np.inf
    assert np.array_equal(ar.bits(v), ar.bits(F([[0, 0, 0], [1, 0, -0.0], [1, 1, 0.25], [0, 1.5, 1e-40]])))
    assert np.array_equal(ar.bits(n), ar.bits(F([[0, 0, 1], [-0.0, 0.6, 0.8], [0, 0, 0], [-1, 0, 0]])))
    colors = F([[0, 0.5, 1], [nan, -1, 2], [0.999, 0.003921569, inf], [0.2, 0.7, -inf]])
    assert np.array_equal(rgb, ar.color_u8(colors))
    assert rgb.tolist() == [[0, 127, 255], [0, 0, 255], [254, 1, 255], [51, 178, 0]]
    assert t.tolist() == [[0, 1, 2], [0, 2, 3]]
    ev, en, ergb, et = parse_ply((tmp_path / "two.ply.empty").read_bytes())
    assert len(ev) == 0 and len(et) == 0
    assert not (tmp_path / "two.ply.bad").exists()
