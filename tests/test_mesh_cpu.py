"""nrf_density_lattice / nrf_extract_mesh / nrf_read_mesh, the parts that need no GPU: the declarations and the bindings, the
orientation table in exact integer arithmetic, and the one text of the definition -- host/mesh_plan_check.cpp (csrc/nrf_mesh_plan.h
under AddressSanitizer + UBSan) against tests/mesh_replay.py, the numpy replay the GPU tests use, float bits and indices.  Every
test here needs the feature: none passes without it."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_replay as mr

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nerf-cuda_amd" / "host"
F = np.float32


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("mesh") / "mesh_plan_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe), str(HOST / "mesh_plan_check.cpp")], check=True)
    return exe


def _problem(origin, cell, dims, iso, sigma):
    head = [f"{w:08x}" for w in mr.bits(list(origin) + list(cell))] + [str(int(d)) for d in dims] + [f"{mr.bits([iso])[0]:08x}"]
    return " ".join(head) + "\n" + " ".join(f"{w:08x}" for w in mr.bits(sigma).reshape(-1)) + "\n"


def _run(exe, problems):
    """[(vertex bits [nv][3], triangles [nt][3])] of the check program on a list of (origin, cell, dims, iso, sigma)"""
    out = subprocess.run([str(exe)], input="".join(_problem(*p) for p in problems), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"mesh_plan_check: {len(problems)} problems" in out.stderr
    res, lines, at = [], out.stdout.splitlines(), 0
    while at < len(lines):
        head = lines[at].split()
        assert head[0] == "mesh" and head[3:] == ["1", "1"], head
        nv, nt = int(head[1]), int(head[2])
        v = np.array([[int(w, 16) for w in ln.split()[1:]] for ln in lines[at + 1:at + 1 + nv]], np.uint32).reshape(-1, 3)
        t = np.array([[int(w) for w in ln.split()[1:]] for ln in lines[at + 1 + nv:at + 1 + nv + nt]], np.uint32).reshape(-1, 3)
        assert all(ln.startswith("v ") for ln in lines[at + 1:at + 1 + nv]) and all(ln.startswith("t ") for ln in lines[at + 1 + nv:at + 1 + nv + nt])
        res.append((v, t))
        at += 1 + nv + nt
    assert len(res) == len(problems)
    return res


def _same(got, problem):
    want = mr.mesh(*problem)
    assert got[0].shape == want.vertices.shape and got[1].shape == want.triangles.shape, (got[0].shape, want.vertices.shape, got[1].shape)
    assert np.array_equal(got[0], mr.bits(want.vertices)) and np.array_equal(got[1], want.triangles)
    return want


def sphere_field(n=17, r0=0.61):
    """r0 - |x| on the n^3 lattice over [-1, 1]^3 (fp32), iso 0: a ball well inside the lattice"""
    origin, cell, dims = [-1.0] * 3, [2.0 / (n - 1)] * 3, (n, n, n)
    x = mr.positions(origin, cell, dims).astype(np.float64)
    return origin, cell, dims, F(0.0), (r0 - np.sqrt(np.sum(x * x, axis=-1))).astype(np.float32)


def noise_field(dims, seed=5, iso=0.5, zero_boundary=False):
    """noise in [0, 1) with NaN, +-inf and values equal to iso strewn in; cells that differ by axis"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 1, dims).astype(np.float32)
    flat = s.reshape(-1)
    n = len(flat)
    k = max(1, n // 40)
    for value in (np.nan, np.inf, -np.inf, iso, iso):
        flat[rng.choice(n, k, replace=False)] = value
    if zero_boundary:
        s[0], s[-1], s[:, 0], s[:, -1], s[:, :, 0], s[:, :, -1] = 0, 0, 0, 0, 0, 0
    return [-0.5, 0.25, 1.0], [0.125, 0.3, 0.07], tuple(dims), F(iso), s


# ---------------------------------------------------------------- 0. the declarations
def test_the_header_declares_them_and_the_binding_has_them():
    import nerfhip as nh
    header = (ROOT / "include" / "nerfhip.h").read_text()
    want = {
        "nrf_density_lattice": ["nrf_context* ctx", "const nrf_lattice* lattice", "void* sigma_f32", "void* stream"],
        "nrf_extract_mesh": ["nrf_context* ctx", "const nrf_lattice* lattice", "float iso", "const void* sigma_f32", "void* stream", "nrf_mesh* out"],
        "nrf_read_mesh": ["nrf_context* ctx", "float* vertices", "uint32_t* triangles"],
    }
    lib = nh.load_library()
    for name, args in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m is not None, name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == args, name
        assert name in nh.exported_symbols()
        assert getattr(lib, name).restype is C.c_int
    assert lib.nrf_extract_mesh.argtypes[2] is C.c_float
    assert C.sizeof(nh.Lattice) == 40 and C.sizeof(nh.Mesh) == 40
    for method in ("density_lattice", "extract_mesh", "read_mesh"):
        assert callable(getattr(nh.NerfHip, method))
    assert nh.NRF_ABI_VERSION == 7 == lib.nrf_abi_version()  # an addition: the version does not change
    mirror = (HOST / "nerf_render.h").read_text()
    for method in ("extract_mesh", "save_obj"):
        assert re.search(r"\b" + method + r"\s*\(", mirror), method
    comment = header[header.index("Mesh extraction"):header.index("int nrf_extract_mesh")]
    assert "nrf_density_gradient takes out->vertices as it is" in comment and "vertex normal" in comment  # the [n][3] layout and why


def test_the_library_holds_the_lattice_instances_and_the_mesh_kernels(tmp_path):
    import test_ray_hits_cpu as hcpu
    names = hcpu._kernel_names(tmp_path)
    # NET_HOT 0, NET_GENERIC 1, NET_WIDE 2 (nrf_launch.h); the nine points_kernel instances stay what they were (test_density_points_cpu.py)
    lattice = sorted(int(m.group(1)) for m in (re.search(r"\bpoints_lattice_kernel<(\d+)>", n) for n in names) if m)
    assert lattice == [0, 1, 2], lattice
    for kernel in ("mesh_count_kernel", "mesh_scan_reduce_kernel", "mesh_scan_partials_kernel", "mesh_scan_write_kernel", "mesh_emit_kernel"):
        assert any(re.search(r"\b" + kernel + r"\b", n) for n in names), kernel


# ---------------------------------------------------------------- (a) the orientation table
def _tet_points(t):
    return [np.array(mr.code_offset(c), np.int64) for c in mr.tet_corners(t)]


def test_the_orientation_table_in_exact_integers(check_program):
    """All 6 x 14 non-empty cases: corners as integers, vertices at DOUBLED edge midpoints; the normal (b - a) x (c - a) dotted with
    (outside centroid - inside centroid), scaled to integers, must be positive, and every crossing edge of the tetrahedron is used.
    The header's table (the check program prints it) must be the replay's."""
    dumped = {}
    out = subprocess.run([str(check_program), "table"], capture_output=True, text=True, check=True).stdout
    for ln in out.splitlines():
        w = [int(a) for a in ln.split()]
        dumped.setdefault((w[0], w[1]), []).append([(w[2], w[3]), (w[4], w[5]), (w[6], w[7])])
    cases = 0
    for t in range(6):
        P = _tet_points(t)
        codes = mr.tet_corners(t)
        assert sorted(tuple(p) for p in P) == sorted({tuple(p) for p in P}) and int(round(abs(np.linalg.det(np.array(P[1:]) - P[0])))) == 1
        for mask in range(1, 15):
            ins = [i for i in range(4) if (mask >> i) & 1]
            out_ = [i for i in range(4) if not (mask >> i) & 1]
            tris = mr.tet_triangles(t, mask)
            assert len(tris) == (2 if len(ins) == 2 else 1)
            toward = len(ins) * sum(P[i] for i in out_) - len(out_) * sum(P[i] for i in ins)  # (centroid difference) x n_in x n_out
            used = set()
            for tri in tris:
                assert all((a in ins) != (b in ins) for a, b in tri)  # crossing edges only
                v = [P[a] + P[b] for a, b in tri]
                normal = np.cross(v[1] - v[0], v[2] - v[0])
                assert int(np.dot(normal, toward)) > 0, (t, mask, tri)
                used |= {frozenset(e) for e in tri}
            assert used == {frozenset((a, b)) for a in ins for b in out_}, (t, mask)
            # the header's words: edges as (from, to) corner codes of the cell, from a subset of to
            want = [[(codes[min(a, b)], codes[max(a, b)]) for a, b in tri] for tri in tris]
            assert dumped.get((t, mask)) == want, (t, mask, dumped.get((t, mask)), want)
            assert all(f & to == f for tri in want for f, to in tri)
            cases += 1
    assert cases == 84 and len(dumped) == 84
    assert mr.tet_triangles(0, 0) == [] and mr.tet_triangles(5, 15) == []
    # the six tetrahedra tile the cell: their edges are the seven edge kinds, each a pair (from, to) with from a subset of to
    kinds = {(mr.tet_corners(t)[a], mr.tet_corners(t)[b]) for t in range(6) for a in range(4) for b in range(a + 1, 4)}
    assert len(kinds) == 19 and {f ^ to for f, to in kinds} == set(range(1, 8))


# ---------------------------------------------------------------- (b) one text of the definition
def test_the_check_program_is_the_replay_on_every_corner_configuration(check_program):
    problems = []
    for config in range(256):
        s = np.array([1.0 if (config >> c) & 1 else 0.25 * (c + 1) / 9 for c in range(8)], np.float32)
        # sigma[i][j][k] of corner code c = i + 2 j + 4 k
        grid = np.zeros((2, 2, 2), np.float32)
        for c in range(8):
            grid[c & 1, (c >> 1) & 1, (c >> 2) & 1] = s[c]
        problems.append(([0.5, -1.0, 2.0], [1.0, 0.5, 0.25], (2, 2, 2), F(0.7), grid))
    got = _run(check_program, problems)
    n_tri = []
    for config, (g, p) in enumerate(zip(got, problems)):
        want = _same(g, p)
        n_tri.append(len(want.triangles))
        mr.check_indices(want.triangles, len(want.vertices))
        x = mr.positions(*p[:3]).reshape(-1, 3)
        mr.check_placement(want.vertices, x[want.edge_p], x[want.edge_q])
    assert n_tri[0] == n_tri[255] == 0 and min(n_tri[1:255]) >= 1 and max(n_tri) <= 12


def test_the_check_program_is_the_replay_on_noise_and_on_a_ball(check_program):
    noise = noise_field((9, 7, 5))
    assert np.isnan(noise[4]).any() and np.isposinf(noise[4]).any() and np.isneginf(noise[4]).any() and (noise[4] == noise[3]).any()
    ball = sphere_field()
    got = _run(check_program, [noise, ball, noise_field((3, 5, 4), seed=9, zero_boundary=True)])
    for g, p in zip(got, (noise, ball, noise_field((3, 5, 4), seed=9, zero_boundary=True))):
        want = _same(g, p)
        assert len(want.triangles) > 0
    # the numbering the definition states, on the replay: vertex ids ascend with (p, m), triangles with the min corner's p
    want = mr.mesh(*ball)
    assert np.all(np.diff(want.edge_p) >= 0)
    d = want.edge_q - want.edge_p
    same_p = np.diff(want.edge_p) == 0
    assert np.all(np.diff(d)[same_p] != 0)


def test_the_make_target():
    mk = (HOST / "Makefile").read_text()
    assert re.search(r"^mesh_asan: mesh_plan_check$", mk, re.M)
    rule = mk.split("mesh_plan_check: mesh_plan_check.cpp")[1].split("\n# ")[0]
    assert "-fsanitize=address,undefined" in rule and "-ffp-contract=off" in rule and "-fno-sanitize-recover=all" in rule
    for name in ("Makefile", "../CMakeLists.txt"):
        text = (ROOT / "nerf-cuda_amd" / name).read_text()
        assert "nrf_kernels_mesh" in text and "nrf_mesh_plan.h" in text, name


# ---------------------------------------------------------------- (c) properties
def test_the_ball_is_a_closed_oriented_sphere():
    origin, cell, dims, iso, s = sphere_field()
    m = mr.mesh(origin, cell, dims, iso, s)
    ins = m.inside
    assert ins.any() and not (ins[0].any() or ins[-1].any() or ins[:, 0].any() or ins[:, -1].any() or ins[:, :, 0].any() or ins[:, :, -1].any())
    V = mr.check_all(m, origin, cell, dims)
    n_v, n_f = len(m.vertices), len(m.triangles)
    assert 3 * n_f % 2 == 0
    n_e = 3 * n_f // 2
    assert n_v - n_e + n_f == 2, (n_v, n_e, n_f)
    ball = 4.0 / 3.0 * np.pi * 0.61 ** 3
    print(f"ball: {n_v} vertices, {n_f} triangles, volume {V:.4f} (a ball of that radius: {ball:.4f})")
    assert 0.8 * ball < V < ball  # (a polyhedron inscribed up to the interpolation's error)
    # ... and the checkers do refuse: a flipped triangle, a dropped triangle, a vertex moved off its edge
    flipped = m.triangles.copy()
    flipped[7] = flipped[7][[0, 2, 1]]
    for bad in (flipped, m.triangles[1:]):
        with pytest.raises(AssertionError):
            mr.check_closed_and_oriented(bad)
    x = mr.positions(origin, cell, dims).reshape(-1, 3)
    moved = m.vertices.copy()
    moved[3] += F(0.2)
    with pytest.raises(AssertionError):
        mr.check_placement(moved, x[m.edge_p], x[m.edge_q])
    with pytest.raises(AssertionError):
        mr.check_volume(m.vertices, m.triangles[:, [0, 2, 1]], m.inside, cell)
