"""nrf_refine_mesh / nrf_read_mesh_refinement, the parts that need no GPU: the declarations and the bindings, and the one text of the
definition -- host/refine_plan_check.cpp (csrc/nrf_refine_plan.h under AddressSanitizer + UBSan) against tests/refine_replay.py, the
numpy replay the GPU tests use, bit for bit, on an analytic density computed in numpy.  Every test here needs the feature: none
passes without it."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_replay as mr
import refine_replay as rr
from test_mesh_cpu import _problem, noise_field

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nerf-cuda_amd" / "host"
F = np.float32
BOUND = F(1.0)
ISO = F(1.0)
STEPS = [0, 1, 5, 16]


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("refine") / "refine_plan_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe), str(HOST / "refine_plan_check.cpp")], check=True)
    return exe


def density(x):
    """exp(6 (0.6 - |x|)): a ball whose sigma crosses ISO = 1 at radius 0.6 and changes by a factor of 3 across a cell of the lattices
    below -- with NaN, +inf, -inf and values EQUAL to iso in small boxes of space picked by a hash of floor(7 x), and nrf_density's
    guard: 0 where a coordinate is outside [-BOUND, BOUND]"""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    x64 = x.astype(np.float64)
    s = np.exp(6.0 * (0.6 - np.sqrt(np.sum(x64 * x64, axis=1)))).astype(np.float32)
    c = np.floor(x64 * 7.0).astype(np.int64)
    h = ((c[:, 0] * 73856093) ^ (c[:, 1] * 19349663) ^ (c[:, 2] * 83492791)) % 29
    for k, value in enumerate((np.nan, np.inf, -np.inf, ISO)):
        s[h == k] = value
    s[~np.all(np.abs(x) <= BOUND, axis=1)] = 0
    return s


def own_lattice(dims=(11, 10, 9)):
    """a lattice that sticks out of the box, its sigmas the density's own: every crossing edge is a bracket"""
    origin, cell = [-1.25, -1.0, -0.875], [float(F(2.5 / (dims[0] - 1))), float(F(2.0 / (dims[1] - 1))), float(F(1.75 / (dims[2] - 1)))]
    sigma = density(mr.positions(origin, cell, dims).reshape(-1, 3)).reshape(dims)
    return origin, cell, tuple(dims), ISO, sigma


def foreign_lattice(dims=(7, 6, 5)):
    """a caller's noise lattice inside the box: its crossing edges are the noise's, not the density's -- many do not bracket ISO"""
    _, _, dims, _, sigma = noise_field(dims, seed=3, iso=0.5)
    return [-0.75, -0.5, -0.625], [0.25, 0.2, 0.3125], dims, ISO, sigma


def _hex(a):
    return " ".join(f"{w:08x}" for w in np.asarray(a, np.uint32).reshape(-1))


def _run(exe, origin, cell, dims, iso, words, answers, n_steps):
    """the check program on one problem -> (words, bracketed, asked bits [n_steps + 2][n][3], bracket bits [n][4], vertex bits [n][3])"""
    n = len(words)
    text = _hex(mr.bits(list(origin) + list(cell))) + " " + " ".join(str(int(d)) for d in dims) + f" {_hex(mr.bits([iso]))} {n_steps} {n}\n"
    text += "".join(f"{w:08x} {_hex(mr.bits(answers[:, i]))}\n" for i, w in enumerate(words))
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "refine_plan_check: 1 problems" in out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ["refine", str(n), str(n_steps), "1", "1"] and len(lines) == n + 1
    rows = np.array([[int(w, 16) for w in ln.split()] for ln in lines[1:]], np.uint32).reshape(n, 2 + 3 * (n_steps + 2) + 7)
    asked = rows[:, 2:2 + 3 * (n_steps + 2)].reshape(n, n_steps + 2, 3).transpose(1, 0, 2)
    return rows[:, 0], rows[:, 1].astype(bool), asked, rows[:, -7:-3], rows[:, -3:]


# ---------------------------------------------------------------- 0. the declarations
def test_the_header_declares_them_and_the_binding_has_them(tmp_path):
    import nerfhip as nh
    header = (ROOT / "include" / "nerfhip.h").read_text()
    want = {
        "nrf_refine_mesh": ["nrf_context* ctx", "uint32_t n_steps", "void* stream", "nrf_mesh_refine* out"],
        "nrf_read_mesh_refinement": ["nrf_context* ctx", "uint32_t* edges", "float* brackets_f32x4"],
    }
    lib = nh.load_library()
    for name, args in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m is not None, name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == args, name
        assert name in nh.exported_symbols()
        assert getattr(lib, name).restype is C.c_int
    assert lib.nrf_refine_mesh.argtypes[1] is C.c_uint32
    assert [f[0] for f in nh.MeshRefine._fields_] == ["n_vertices", "n_unbracketed", "vertices", "edges", "brackets", "n_steps", "reserved"]
    for method in ("refine_mesh", "read_mesh_refinement"):
        assert callable(getattr(nh.NerfHip, method))
    assert nh.NRF_ABI_VERSION == 7 == lib.nrf_abi_version()  # an addition: the version does not change
    # the struct as the C compiler lays it out
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is not None:
        src, exe = tmp_path / "s.c", tmp_path / "s"
        src.write_text('#include "nerfhip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(){printf("%zu %zu %zu\\n", sizeof(nrf_mesh_refine),'
                       ' offsetof(nrf_mesh_refine, brackets), offsetof(nrf_mesh_refine, n_steps));return 0;}')
        subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert sizes == [C.sizeof(nh.MeshRefine), nh.MeshRefine.brackets.offset, nh.MeshRefine.n_steps.offset] == [48, 32, 40]
    mirror = (HOST / "nerf_render.h").read_text()
    assert re.search(r"\brefine_mesh\s*\(\s*uint32_t n_steps\s*\)", mirror)
    assert "--mesh_refine" in (HOST / "testbed.cpp").read_text()
    comment = header[header.index("Mesh refinement"):header.index("int nrf_refine_mesh")]
    assert "(p << 3) | m" in comment and "0.5f * (lo + hi)" in comment and "UNBRACKETED" in comment


def test_the_library_holds_the_refine_instances_and_the_edge_kernel(tmp_path):
    import test_ray_hits_cpu as hcpu
    names = hcpu._kernel_names(tmp_path)
    # NET_HOT 0, NET_GENERIC 1, NET_WIDE 2 (nrf_launch.h)
    refine = sorted(int(m.group(1)) for m in (re.search(r"\brefine_kernel<(\d+)>", n) for n in names) if m)
    assert refine == [0, 1, 2], refine
    for kernel in ("mesh_edges_kernel", "mesh_emit_kernel", "meshcc_scatter_kernel"):
        assert any(re.search(r"\b" + kernel + r"\b", n) for n in names), kernel


def test_the_make_target():
    mk = (HOST / "Makefile").read_text()
    assert re.search(r"^refine_asan: refine_plan_check$", mk, re.M)
    rule = mk.split("refine_plan_check: refine_plan_check.cpp")[1].split("\n# ")[0]
    assert "-fsanitize=address,undefined" in rule and "-ffp-contract=off" in rule and "-fno-sanitize-recover=all" in rule
    for name in ("Makefile", "../CMakeLists.txt"):
        text = (ROOT / "nerf-cuda_amd" / name).read_text()
        assert "nrf_kernels_refine" in text and "nrf_refine_plan.h" in text, name


# ---------------------------------------------------------------- 1. edge words
def test_the_edge_words_of_the_extraction_are_the_replays(check_program):
    problems = [own_lattice(), foreign_lattice(), noise_field((3, 5, 4), seed=9, zero_boundary=True)]
    out = subprocess.run([str(check_program), "edges"], input="".join(_problem(*p) for p in problems), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines, at = out.stdout.splitlines(), 0
    for p in problems:
        m = mr.mesh(*p)
        assert lines[at].split() == ["edges", str(len(m.vertices))] and len(m.vertices) > 0
        got = np.array([int(w, 16) for w in lines[at + 1:at + 1 + len(m.vertices)]], np.uint32)
        want = rr.edge_words(m, p[2])
        assert np.array_equal(got, want)
        assert np.all(np.diff(want.astype(np.int64)) > 0) and int(want.max()) < 1 << 30  # ascending with (p, m): emit's numbering
        at += 1 + len(m.vertices)
    assert at == len(lines)


# ---------------------------------------------------------------- 2. one text of the definition
@pytest.mark.parametrize("n_steps", STEPS)
def test_the_check_program_is_the_replay_on_the_densitys_own_lattice(check_program, n_steps):
    origin, cell, dims, iso, sigma = own_lattice()
    flat = sigma.reshape(-1)
    assert np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any() and (flat == iso).any()
    x = mr.positions(origin, cell, dims).reshape(-1, 3)
    outside = ~np.all(np.abs(x) <= BOUND, axis=1)
    assert outside.any() and np.all(flat[outside] == 0)
    m = mr.mesh(origin, cell, dims, iso, sigma)
    words = rr.edge_words(m, dims)
    assert len(words) > 300
    assert outside[m.edge_p].any() or outside[m.edge_q].any()  # an edge that leaves the box: its far end answers 0
    want = rr.refine(origin, cell, dims, iso, words, np.zeros_like(m.vertices), n_steps, density)
    assert want.bracketed.all()  # the lattice is the density's own
    special = ~np.isfinite(want.answers) | (want.answers == iso)
    assert special[:2].any() and (n_steps == 0 or special[2:].any())  # NaN, inf and iso itself among the answers, midpoints included
    got_words, got_bracketed, asked, brackets, vertices = _run(check_program, origin, cell, dims, iso, words, want.answers, n_steps)
    assert np.array_equal(got_words, words) and np.array_equal(got_bracketed, want.bracketed)
    assert np.array_equal(asked, mr.bits(want.asked))
    assert np.array_equal(brackets, mr.bits(want.brackets)) and np.array_equal(vertices, mr.bits(want.vertices))
    rr.check_refinement(want.vertices, want.brackets, origin, cell, dims, iso, words, n_steps)
    if n_steps == 0:  # mesh_vertex on the same sigmas
        assert np.array_equal(mr.bits(want.vertices), mr.bits(m.vertices))
        assert np.array_equal(mr.bits(want.brackets[:, 2]), mr.bits(flat[m.edge_p])) and np.array_equal(mr.bits(want.brackets[:, 3]), mr.bits(flat[m.edge_q]))
    else:
        assert np.any(mr.bits(want.vertices) != mr.bits(m.vertices))


@pytest.mark.parametrize("n_steps", STEPS)
def test_the_check_program_is_the_replay_on_a_lattice_that_disagrees(check_program, n_steps):
    origin, cell, dims, iso, sigma = foreign_lattice()
    m = mr.mesh(origin, cell, dims, F(0.5), sigma)
    words = rr.edge_words(m, dims)
    before = np.full_like(m.vertices, 7.0)
    want = rr.refine(origin, cell, dims, iso, words, before, n_steps, density)
    assert 0 < want.bracketed.sum() < len(words)
    got_words, got_bracketed, asked, brackets, vertices = _run(check_program, origin, cell, dims, iso, words, want.answers, n_steps)
    assert np.array_equal(got_bracketed, want.bracketed) and np.array_equal(asked, mr.bits(want.asked))
    assert np.array_equal(brackets, mr.bits(want.brackets))
    k = want.bracketed
    assert np.array_equal(vertices[k], mr.bits(want.vertices)[k]) and np.all(vertices[~k] == 0)
    assert np.array_equal(mr.bits(want.vertices)[~k], mr.bits(before)[~k])  # an unbracketed vertex keeps its bits
    assert np.array_equal(mr.bits(want.brackets[~k, :2]), mr.bits(np.tile(np.array([0, 1], np.float32), ((~k).sum(), 1))))
    assert np.array_equal(mr.bits(want.brackets[~k, 2:]), mr.bits(want.answers[:2, ~k].T))
    assert np.array_equal(mr.bits(want.asked[2:, ~k]), mr.bits(np.broadcast_to(rr.point(*rr.edge_positions(origin, cell, dims, words), np.full(len(words), 0.5))[~k],
                                                                               want.asked[2:, ~k].shape)))  # ... and asks for its midpoint every time
    rr.check_refinement(want.vertices, want.brackets, origin, cell, dims, iso, words, n_steps, bracketed=k)


def test_the_checker_does_refuse():
    origin, cell, dims, iso, sigma = own_lattice()
    m = mr.mesh(origin, cell, dims, iso, sigma)
    words = rr.edge_words(m, dims)
    want = rr.refine(origin, cell, dims, iso, words, m.vertices, 5, density)
    rr.check_refinement(want.vertices, want.brackets, origin, cell, dims, iso, words, 5)
    wide, swapped, moved = want.brackets.copy(), want.brackets.copy(), want.vertices.copy()
    wide[3, 1] = wide[3, 0] + F(2.0 ** -4)
    swapped[4, 3] = swapped[4, 2]
    moved[5] += F(0.5)
    for v, b, n in ((want.vertices, wide, 5), (want.vertices, swapped, 5), (moved, want.brackets, 5), (want.vertices, want.brackets, 4)):
        with pytest.raises(AssertionError):
            rr.check_refinement(v, b, origin, cell, dims, iso, words, n)


def test_refused_problems(check_program):
    head = _hex(mr.bits([0, 0, 0, 1, 1, 1])) + " 2 2 2 " + _hex(mr.bits([0.5]))
    for tail, want in ((" 17 0\n", "refine 0 17 1 0"), (" 16 0\n", "refine 0 16 1 1")):
        out = subprocess.run([str(check_program)], input=head + tail, capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip() == want, (out.stdout, out.stderr)
    out = subprocess.run([str(check_program)], input=_hex(mr.bits([0, 0, 0, 1, 1, 1])) + " 1 2 2 " + _hex(mr.bits([0.5])) + " 3 0\n", capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "refine 0 3 0 1"
