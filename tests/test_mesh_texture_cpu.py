"""nrf_bake_mesh_texture / nrf_read_mesh_texture / nrf_mesh_texture_size, the parts that need no GPU: the declarations and the bindings,
the three bake_kernel symbols of the built library, the host-only size call, the one text of the definition -- host/bake_plan_check.cpp
(csrc/nrf_bake_plan.h, plain and under AddressSanitizer + UBSan through `make bake_asan`) against tests/bake_replay.py, the numpy replay
the GPU tests use, bit for bit --, the properties of the layout itself, and the files NerfRender::save_obj_textured writes.  Every test
here needs the feature: none passes without it."""
import ctypes as C
import re
import shutil
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import attr_replay as ar
import bake_replay as br
import nerfhip as nh
import test_ray_hits_cpu as hcpu

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nerf-cuda_amd" / "host"
F = np.float32
NAMES = ["nrf_mesh_texture_size", "nrf_bake_mesh_texture", "nrf_read_mesh_texture"]


# ---------------------------------------------------------------- 1. the declarations
def test_the_header_declares_them_and_the_binding_has_them():
    header = (ROOT / "include" / "nerfhip.h").read_text()
    want = {
        "nrf_mesh_texture_size": ["uint64_t n_triangles", "uint32_t res", "uint32_t width", "uint32_t* height"],
        "nrf_bake_mesh_texture": ["nrf_context* ctx", "uint32_t res", "uint32_t width", "void* stream", "nrf_mesh_texture* out"],
        "nrf_read_mesh_texture": ["nrf_context* ctx", "float* texels_f32x4", "uint32_t* rgba8", "float* uvs"],
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
    assert "(csrc/nrf_bake_plan.h is this text as code.)" in header
    assert [f[0] for f in nh.MeshTexture._fields_] == ["width", "height", "res", "cols", "n_triangles", "n_refused", "texels", "rgba8", "uvs"]
    src = '#include "nerfhip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(nrf_mesh_texture),' \
          ' offsetof(nrf_mesh_texture, n_triangles), offsetof(nrf_mesh_texture, texels), offsetof(nrf_mesh_texture, uvs));return 0;}'
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is not None:
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            (Path(td) / "s.c").write_text(src)
            subprocess.run([cc, "-I", str(ROOT / "include"), str(Path(td) / "s.c"), "-o", str(Path(td) / "s")], check=True)
            sizes = [int(v) for v in subprocess.run([str(Path(td) / "s")], capture_output=True, text=True, check=True).stdout.split()]
        T = nh.MeshTexture
        assert sizes == [C.sizeof(T), T.n_triangles.offset, T.texels.offset, T.uvs.offset] == [56, 16, 32, 48]
    for method in ("bake_mesh_texture", "read_mesh_texture"):
        assert callable(getattr(nh.NerfHip, method))
    assert callable(nh.mesh_texture_size)
    assert nh.NRF_ABI_VERSION == 7 == lib.nrf_abi_version()  # additions: no structure changes
    mirror = (HOST / "nerf_render.h").read_text()
    for method in ("bake_mesh_texture", "save_obj_textured", "save_obj", "save_ply"):
        assert re.search(r"\b" + method + r"\s*\(", mirror), method


def test_the_library_holds_three_bake_instances(tmp_path):
    names = hcpu._kernel_names(tmp_path)
    found = sorted(int(m.group(1)) for m in (re.search(r"\bbake_kernel<(\d+)>", n) for n in names) if m)
    assert found == [0, 1, 2], found  # NET_HOT 0, NET_GENERIC 1, NET_WIDE 2 (nrf_launch.h)
    assert any(re.search(r"\bbake_uv_kernel\b", n) for n in names)


def test_the_size_call_is_the_replays_layout():
    lib = nh.load_library()

    def size(nt, res, width):
        h = C.c_uint32(0xABABABAB)
        rc = int(lib.nrf_mesh_texture_size(nt, res, width, C.byref(h)))
        assert rc == nh.NRF_OK or h.value == 0xABABABAB  # a refused call writes nothing
        return rc, h.value, lib.nrf_last_error().decode()

    for nt, res, width in [(0, 2, 4), (1, 2, 4), (2, 2, 4), (3, 2, 4), (4601, 10, 4096), (4600, 10, 1000), (7, 256, 258), (126, 256, 258),
                           (100000, 8, 4096), (1000001, 2, 16384), (1, 256, 16384), (65535, 30, 16384)]:
        want = br.layout(nt, res, width)
        assert want is not None, (nt, res, width)
        assert size(nt, res, width)[:2] == (nh.NRF_OK, want[0]), (nt, res, width)
        assert nh.mesh_texture_size(nt, res, width) == want[0]
    assert br.layout(0, 2, 4)[0] == 0 and br.layout(1, 2, 4)[0] == 3 and br.layout(3, 2, 4)[0] == 6
    # the parameters
    for res, width in [(1, 100), (0, 100), (257, 1000), (2, 3), (8, 9), (8, 16385), (256, 257)]:
        assert br.layout(10, res, width) is None and size(10, res, width)[0] == nh.NRF_E_INVALID, (res, width)
    assert int(lib.nrf_mesh_texture_size(10, 8, 100, None)) == nh.NRF_E_INVALID
    # the limits: too high at this width -- the message names the smallest width that fits; the texel limit; nothing fits
    for nt, res, width in [(130, 256, 258), (4600, 10, 12), (12000000, 2, 16384), (1492000, 8, 8192), (2100, 256, 258), (2100, 256, 16384), (2000, 256, 16384)]:
        assert br.layout(nt, res, width) is None and br.params_valid(res, width)
        rc, _, msg = size(nt, res, width)
        fit = br.smallest_width(nt, res)
        assert rc == nh.NRF_E_INVALID, (nt, res, width)
        if fit:
            assert f"smallest width that fits is {fit}" in msg and br.layout(nt, res, fit) is not None, (msg, fit)
            assert fit == res + 2 or br.layout(nt, res, fit - 1) is None
        else:
            assert "no width fits" in msg, msg
    assert br.smallest_width(130, 256) == 516 and br.smallest_width(2100, 256) == 0 and br.smallest_width(12000000, 2) == 0 and br.smallest_width(2000, 256) > 0
    with pytest.raises(nh.NerfHipError) as e:
        nh.mesh_texture_size(130, 256, 258)
    assert e.value.code == nh.NRF_E_INVALID


# ---------------------------------------------------------------- 2. one text of the definition
BOUND = F(1.0)


def _mesh(seed, n_random, odd):
    """vertices [n][3] and triangles [m][3] (uint32): random triangles well inside the box, then the edges -- a triangle whose
    extrapolated texels leave the box, degenerate ones, indices that are not there, NaN, +-inf, outside the bound, denormals, -0"""
    rng = np.random.default_rng(seed)
    v = list(rng.uniform(-0.6, 0.6, (3 * n_random, 3)).astype(np.float32))
    t = [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(n_random)]

    def add(*rows):
        first = len(v)
        v.extend(F(r) for r in rows)
        return list(range(first, first + len(rows)))

    t.append(add([0.99, 0.2, -0.3], [-0.5, 0.99, 0.1], [0.3, -0.2, -0.99]))    # inside, but its outside texels are not
    a, b, c = add([0.25, -0.5, 0.125], [0.5, 0.25, -0.75], [-0.125, 0.0, 0.5])
    t += [[a, a, b], [a, a, a], [a, b, a], [c, b, a]]                         # zero area (and the last one turned round)
    t.append(add([0.0, 0.0, 0.0], [0.25, 0.25, 0.25], [0.5, 0.5, 0.5]))         # collinear
    t.append(add([1e-20, 0, 0], [0, 1e-20, 0], [0, 0, 1e-20]))                  # an area below the floor
    t.append(add([3e-16, 0, 0], [0, 3.3e-16, 0], [0, 0, 0]))                    # ... and about at it: l2 near 2^-60 / 4
    t.append(add([-0.0, 0.0, -0.0], [1e-45, -1e-45, 1e-39], [-0.0, 0.5, 0.0]))  # signed zeros and denormals
    nv_now = len(v)
    t += [[a, b, nv_now + 40], [0xFFFFFFFF, a, b], [a, 0x80000000, c]]          # vertices that are not there
    t.append(add([np.nan, 0.1, 0.2], [0.3, 0.1, 0.0], [0.0, 0.4, 0.1]))
    t.append(add([0.1, 0.1, 0.2], [0.3, np.inf, 0.0], [0.0, 0.4, 0.1]))
    t.append(add([0.1, 0.1, 0.2], [0.3, 0.1, 0.0], [0.0, 0.4, -np.inf]))
    t.append(add([0.9, 0.1, 0.2], [1.5, 0.1, 0.0], [0.9, 0.4, 0.1]))            # partly outside the bound
    t.append(add([-3.0, 0.1, 0.2], [-4.0, 2.0, 0.0], [-5.0, 0.4, 0.1]))         # wholly
    t.append(add([1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [-1.0, 1.0, 1.0]))          # on the faces themselves: accepted where rounding allows
    t.append(add([3e38, 0, 0], [-3e38, 0, 0], [0, 3e38, 0]))                    # differences that overflow
    v = np.array(v, np.float32)
    t = np.array(t, np.uint64).astype(np.uint32)
    tri = t if (len(t) % 2 == 1) == odd else t[:-1]
    # (vertices past the largest index that is still named pad the count: the named-but-absent indices stay absent)
    return v, tri


def _run(exe, res, width, bound, v, t):
    text = f"{res} {width} {int(ar.bits(F(bound)).reshape(-1)[0]):08x} {len(v)} {len(t)}\n"
    text += "\n".join(" ".join(f"{w:08x}" for w in r) for r in ar.bits(v)) + "\n"
    text += "\n".join(" ".join(str(int(i)) for i in r) for r in t) + "\n"
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln.split() for ln in out.stdout.splitlines()]
    assert lines[0][0] == "layout"
    if lines[0][1] == "0":
        return None, int(lines[0][2]), out.stderr
    head = [int(w) for w in lines[0][2:]]
    tl = [ln for ln in lines if ln[0] == "t"]
    ul = [ln for ln in lines if ln[0] == "u"]
    assert len(tl) + len(ul) + 1 == len(lines)
    ints = np.array([[int(w) for w in ln[1:7]] for ln in tl], np.int64).reshape(-1, 6)
    words = np.array([[int(w, 16) for w in ln[7:13]] for ln in tl], np.uint32).reshape(-1, 6)
    uv = np.array([[int(w, 16) for w in ln[2:8]] for ln in ul], np.uint32).reshape(-1, 6)
    assert [int(ln[1]) for ln in ul] == list(range(len(ul)))
    return (head, ints, words, uv), 0, out.stderr


# (res, width, random triangles, odd count): one column; ragged right margins; a large r
CASES = [(2, 4, 5, True), (2, 4, 4, False), (3, 17, 9, True), (3, 5, 2, False), (8, 10, 3, True), (8, 47, 12, False), (5, 50, 20, True),
         (64, 145, 1, True), (64, 66, 0, False)]


def _hold(exe, res, width, v, t):
    got, _, err = _run(exe, res, width, BOUND, v, t)
    want = br.bake(v, t, res, width, BOUND)
    head, ints, words, uv = got
    assert head == [want["height"], want["cols"], (len(t) + 1) // 2], (res, width)
    assert f"{len(want['guard'])} owned texels, {want['n_refused']} refused" in err, err
    w_ints = np.stack([want["px"], want["py"], want["tri"], want["i"], want["j"], want["guard"].astype(np.int64)], axis=1)
    assert np.array_equal(ints, w_ints), (res, width, np.nonzero(np.any(ints != w_ints, axis=1))[0][:5])
    w_words = np.concatenate([ar.bits(want["x"]), ar.bits(want["d"])], axis=1)
    bad = np.nonzero(np.any(words != w_words, axis=1))[0]
    assert len(bad) == 0, (res, width, len(bad), ints[bad[:5]], words[bad[:5]], w_words[bad[:5]])
    assert np.array_equal(uv, ar.bits(want["uvs"]).reshape(-1, 6)), (res, width)
    return want


def test_the_plan_header_and_the_numpy_replay_are_one_definition(tmp_path):
    """host/bake_plan_check.cpp, a stand-alone program (no GPU, no library): a mesh in, the layout, every owned texel's atlas
    coordinates, owner, (i, j), guard, position and direction bits and the UV bits out, all held to tests/bake_replay.py bit for bit --
    built plainly, and once more through `make bake_asan` (AddressSanitizer + UBSan) in a copy of the two directories the rule needs."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    plain = tmp_path / "bake_plan_check"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-o", str(plain), str(HOST / "bake_plan_check.cpp")], check=True)
    work = tmp_path / "tree" / "nerf-cuda_amd"
    (work / "host").mkdir(parents=True)
    (work / "csrc").mkdir()
    for rel in ("host/Makefile", "host/bake_plan_check.cpp", "csrc/nrf_bake_plan.h", "csrc/nrf_attr_plan.h", "csrc/nrf_points_plan.h"):
        shutil.copy(ROOT / "nerf-cuda_amd" / rel, work / rel)
    r = subprocess.run(["make", "-C", str(work / "host"), "bake_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "-fsanitize=address,undefined" in r.stdout and "-ffp-contract=off" in r.stdout and "30 owned texels, 15 refused" in r.stderr + r.stdout
    assert re.search(r"^bake_asan: bake_plan_check$", (HOST / "Makefile").read_text(), re.M)
    seen = dict(degenerate=0, absent=0, refused_positions=0, accepted=0, odd=0)
    for exe in (plain, work / "host" / "bake_plan_check"):
        for k, (res, width, n_random, odd) in enumerate(CASES):
            v, t = _mesh(100 + k, n_random, odd)
            assert (len(t) % 2 == 1) == odd
            want = _hold(exe, res, width, v, t)
            named = np.all(t.astype(np.int64) < len(v), axis=1)
            seen["absent"] += int((~named).sum())
            seen["odd"] += len(t) % 2
            seen["refused_positions"] += int((~want["guard"] & named[want["tri"]]).sum())
            seen["accepted"] += int(want["guard"].sum())
            seen["degenerate"] += int((np.all(want["d"] == 0, axis=1) & want["guard"]).sum())
        # a mesh with nothing in it, and one triangle alone
        none = _hold(exe, 4, 20, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
        assert none["height"] == 0 and len(none["guard"]) == 0
        _hold(exe, 4, 20, F([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]]), np.array([[0, 1, 2]], np.uint32))
        # refused layouts
        zero = np.zeros((1, 3), np.float32)
        for nt, res, width in [(130, 256, 258), (2100, 256, 258), (3, 1, 100), (3, 8, 9)]:
            got, fit, _ = _run(exe, res, width, BOUND, zero, np.zeros((nt, 3), np.uint32))
            assert got is None and fit == br.smallest_width(nt, res), (nt, res, width, fit)
    print(seen)
    assert all(n > 0 for n in seen.values()), seen


# ---------------------------------------------------------------- 3. the properties of the layout
@pytest.mark.parametrize("res,width,nt", [(2, 4, 7), (2, 9, 8), (3, 17, 11), (5, 50, 41), (8, 47, 12), (10, 1000, 333), (64, 145, 5), (256, 258, 3)])
def test_the_owned_texels_tile_the_atlas(res, width, nt):
    h, cols, pairs = br.layout(nt, res, width)
    owner, claims = br.owner_map(nt, res, width)
    assert owner.shape == (h, width) and claims.max() == 1          # pairwise disjoint
    half = (res + 1) * (res + 2) // 2
    assert np.array_equal(np.bincount(owner[owner >= 0], minlength=nt), np.full(nt, half))
    assert int((owner < 0).sum()) == h * width - nt * half         # with the unowned ones, the atlas exactly once
    # what is unowned: the right margin, the cells after the last pair, the odd half of the last cell
    assert np.all(owner[:, cols * (res + 2):] < 0)
    if nt % 2:
        q = pairs - 1
        cell = owner[(q // cols) * (res + 1):(q // cols + 1) * (res + 1), (q % cols) * (res + 2):(q % cols + 1) * (res + 2)]
        assert int((cell == nt - 1).sum()) == half and int((cell < 0).sum()) == half
    # the corners sit on texels of their own triangle
    uv, corners = br.uvs(nt, res, width)
    for c in range(3):
        assert np.array_equal(owner[corners[:, c, 1], corners[:, c, 0]], np.arange(nt))
    with np.errstate(all="ignore"):
        back_x = uv[:, :, 0].astype(np.float64) * width - 0.5
        back_y = uv[:, :, 1].astype(np.float64) * h - 0.5
    assert np.all(np.abs(back_x - corners[:, :, 0]) < 1e-2) and np.all(np.abs(back_y - corners[:, :, 1]) < 1e-2)
    # a bilinear fetch anywhere inside a triangle's footprint reads texels of that triangle only
    rng = np.random.default_rng(res * 1000 + nt)
    bary = rng.dirichlet([1.0, 1.0, 1.0], (nt, 64))                                     # strictly inside
    bary[:, :8] = rng.dirichlet([0.02, 0.02, 0.02], (nt, 8)).clip(1e-9, None)           # ... and hard by the corners and edges
    bary /= bary.sum(axis=2, keepdims=True)
    p = np.einsum("tkc,tcx->tkx", bary, corners.astype(np.float64))
    x0, y0 = np.floor(p[:, :, 0]).astype(np.int64), np.floor(p[:, :, 1]).astype(np.int64)
    fx, fy = p[:, :, 0] - x0, p[:, :, 1] - y0
    me = np.arange(nt)[:, None]
    for dx, dy, wgt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
        xs, ys = x0 + dx, y0 + dy
        inside = (xs >= 0) & (xs < width) & (ys >= 0) & (ys < h)
        got = np.where(inside, owner[np.clip(ys, 0, h - 1), np.clip(xs, 0, width - 1)], -2)
        assert np.all((got == me) | (wgt == 0.0)), (res, width, nt, dx, dy)


def test_texel_zero_is_the_first_corner_and_the_corners_are_the_vertices():
    rng = np.random.default_rng(7)
    n = 500
    va, vb, vc = (rng.uniform(-1, 1, (n, 3)).astype(np.float32) for _ in range(3))
    va[0] = [-0.0, 0.0, 1e-45]
    zero = np.zeros(n, np.int64)
    for res in (2, 3, 8, 64, 256):
        x = br.position(va, vb, vc, zero, zero, res)
        assert np.array_equal(x, va)                                # in value (-0 + 0 is +0)
        # s = 1 at i = r - 1: the corner b up to the rounding of va + (vb - va)
        xb = br.position(va, vb, vc, zero + res - 1, zero, res)
        xc = br.position(va, vb, vc, zero, zero + res - 1, res)
        assert np.max(np.abs(xb.astype(np.float64) - vb)) <= 2.0 ** -22 and np.max(np.abs(xc.astype(np.float64) - vc)) <= 2.0 ** -22
    # the direction looks against the face normal
    d, ok = br.face_direction(va, vb, vc)
    nrm = np.cross((vb - va).astype(np.float64), (vc - va).astype(np.float64))
    assert ok.all() and np.all(np.sum(d * nrm, axis=1) < 0) and np.all(ar.norm_error(d) <= ar.NORM_BOUND)
    assert list(br.rgba8(F([[0, 0.5, 1], [np.nan, 2, -1]]))) == [0xFFFF7F00, 0xFF00FF00]


# ---------------------------------------------------------------- 4. the OBJ, the MTL and the PNG
def parse_png(data: bytes):
    """uint8 [h][w][3] of an 8-bit RGB PNG without interlace whose rows all have filter 0 (what png_lite.h writes); checks the CRCs"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1][0] == b"IEND"
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT"))
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert np.all(rows[:, 0] == 0)
    return rows[:, 1:].reshape(h, w, 3)


def parse_obj_textured(path: Path):
    """(vertices float32 [n][3], vt float32 [m][2], faces int64 [k][3][2] = (vertex, vt) 0-based, the atlas uint8 [h][w][3]) of the three
    files save_obj_textured writes; checks that they name each other"""
    v, vt, faces, mtllib, usemtl = [], [], [], None, None
    for ln in path.read_text().splitlines():
        f = ln.split()
        if not f or f[0] == "#":
            continue
        if f[0] == "v":
            v.append([float(a) for a in f[1:4]])
        elif f[0] == "vt":
            assert not faces and len(f) == 3
            vt.append([float(a) for a in f[1:3]])
        elif f[0] == "f":
            assert len(f) == 4
            faces.append([[int(a) - 1 for a in c.split("/")] for c in f[1:4]])
        elif f[0] == "mtllib":
            mtllib = f[1]
        elif f[0] == "usemtl":
            assert not faces
            usemtl = f[1]
        else:
            raise AssertionError(ln)
    assert mtllib == path.with_suffix(".mtl").name
    mtl = (path.parent / mtllib).read_text().splitlines()
    assert f"newmtl {usemtl}" in mtl
    maps = [ln.split()[1] for ln in mtl if ln.startswith("map_Kd ")]
    assert maps == [path.with_suffix(".png").name]
    atlas = parse_png((path.parent / maps[0]).read_bytes())
    return (np.array(v, np.float64).astype(np.float32).reshape(-1, 3), np.array(vt, np.float64).astype(np.float32).reshape(-1, 2),
            np.array(faces, np.int64).reshape(-1, 3, 2), atlas)


_OBJ_PROGRAM = r"""
#include <cstdint>
#include <string>
#include <vector>
#include "nerf_render.h"
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::vector<float> vertices = {0.f, 0.f, 0.f, 1.f, 0.f, -0.f, 1.f, 1.f, 0.25f, 0.f, 1.5f, 1e-40f};
  const std::vector<uint32_t> triangles = {0, 1, 2, 0, 2, 3, 3, 2, 1};
  const uint32_t w = 9, h = 3;                       // r = 2 on a ragged width of two columns, three triangles in one row
  std::vector<float> uvs;
  const uint32_t corner[3][3][2] = {{{0, 0}, {1, 0}, {0, 1}}, {{3, 2}, {2, 2}, {3, 1}}, {{4, 0}, {5, 0}, {4, 1}}};
  for (int t = 0; t < 3; ++t)
    for (int c = 0; c < 3; ++c) uvs.push_back(((float)corner[t][c][0] + 0.5f) / (float)w), uvs.push_back(((float)corner[t][c][1] + 0.5f) / (float)h);
  std::vector<uint32_t> rgba8(w * h);
  for (uint32_t i = 0; i < w * h; ++i) rgba8[i] = ((i * 37u) & 255u) | (((i * 11u) & 255u) << 8) | ((255u - i) << 16) | ((i % 3 ? 255u : 0u) << 24);
  const std::string path = argv[1];
  if (!ngp::NerfRender::save_obj_textured(path + "/two.obj", vertices, triangles, uvs, rgba8, w, h)) return 3;
  if (ngp::NerfRender::save_obj_textured(path + "/bad.obj", vertices, triangles, std::vector<float>(12), rgba8, w, h)) return 4;  // one triangle short
  if (ngp::NerfRender::save_obj_textured(path + "/bad.obj", vertices, triangles, uvs, rgba8, w, h + 1)) return 5;
  if (!ngp::NerfRender::save_obj_textured(path + "/empty.obj", {}, {}, {}, {}, 0, 0)) return 6;
  if (!ngp::NerfRender::save_obj(path + "/plain.obj", vertices, triangles)) return 7;
  return 0;
}
"""


def test_save_obj_textured_writes_files_that_name_each_other(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None or not (HOST / "libngp_hip.so").exists():
        pytest.skip("the C++ host mirror is not built")
    src, exe = tmp_path / "obj.cpp", tmp_path / "obj"
    src.write_text(_OBJ_PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(HOST), "-I", str(ROOT / "include"), "-o", str(exe), str(src), f"-L{HOST}", "-lngp_hip",
                    f"-L{HOST.parent}", "-lnerfhip", f"-Wl,-rpath,{HOST}", f"-Wl,-rpath,{HOST.parent}"], check=True)
    out = tmp_path / "out.dir"
    out.mkdir()
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(p.name for p in out.iterdir()) == ["empty.mtl", "empty.obj", "plain.obj", "two.mtl", "two.obj", "two.png"]
    v, vt, faces, atlas = parse_obj_textured(out / "two.obj")
    assert np.array_equal(ar.bits(v), ar.bits(F([[0, 0, 0], [1, 0, -0.0], [1, 1, 0.25], [0, 1.5, 1e-40]])))
    uv, corners = br.uvs(3, 2, 9)
    assert np.array_equal(corners.tolist(), [[[0, 0], [1, 0], [0, 1]], [[3, 2], [2, 2], [3, 1]], [[4, 0], [5, 0], [4, 1]]])
    want_vt = uv.reshape(-1, 2).copy()
    want_vt[:, 1] = F(1) - want_vt[:, 1]
    assert np.array_equal(ar.bits(vt), ar.bits(want_vt))            # (%.9g round-trips a float)
    tri = np.array([[0, 1, 2], [0, 2, 3], [3, 2, 1]])
    assert np.array_equal(faces[:, :, 0], tri) and np.array_equal(faces[:, :, 1], np.arange(9).reshape(3, 3))
    i = np.arange(27, dtype=np.uint32)
    want = np.stack([(i * 37) & 255, (i * 11) & 255, (255 - i) & 255], axis=1).astype(np.uint8).reshape(3, 9, 3)
    assert atlas.shape == (3, 9, 3) and np.array_equal(atlas, want)
    assert "map_Kd" not in (out / "empty.mtl").read_text() and "mtllib empty.mtl" in (out / "empty.obj").read_text()
    assert "vt" not in (out / "plain.obj").read_text()              # the plain writer is as it was
