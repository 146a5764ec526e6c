"""nrf_mesh_components / nrf_read_mesh_components / nrf_filter_mesh, the parts that need no GPU: the declarations, the bindings and
the mirrors, and the one text of the definition -- host/meshcc_plan_check.cpp (csrc/nrf_meshcc_plan.h under AddressSanitizer + UBSan)
against tests/meshcc_replay.py, the numpy replay the GPU tests use: labels, table and filtered indices, identical.  The fields the
GPU tests share are built here.  Every test here needs the feature: none passes without it."""
import ctypes as C
import functools
import re
import shutil
import subprocess
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

import mesh_replay as mr
import meshcc_replay as cr
from test_mesh_cpu import noise_field

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nerf-cuda_amd" / "host"
F = np.float32
CUTS = [(m, f) for m in (0, 1, 25, 649, 1225, 10 ** 9) for f in (0, cr.KEEP_LARGEST)]

Field = namedtuple("Field", "origin cell dims iso sigma mesh parts")


# ---------------------------------------------------------------- the fields (caller-supplied sigma lattices)
def _unit(dims):
    return [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], tuple(dims)


def balls_field(with_first=True):
    """max_i (r_i - |x - c_i|) in float64, then fp32, iso 0: four balls (the third is the second moved by whole cells, so their sigmas
    and their meshes are identical) and one inside point by itself"""
    dims = (28, 24, 16)
    balls = [((7, 7, 7.5), 5.2), ((20.25, 6.5, 6), 3.3), ((20.25, 17.5, 9), 3.3), ((7, 18, 8), 2.4)]
    x = np.stack(np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij"), axis=-1)
    s = np.max([r - np.sqrt(np.sum((x - np.array(c, np.float64)) ** 2, axis=-1)) for c, r in balls[0 if with_first else 1:]], axis=0).astype(np.float32)
    s[13, 21, 13] = 0.4
    return _unit(dims) + (F(0.0), s)


def snake_field():
    """sigma 1 on a one-point-thick serpentine in the plane k = 1: rows i = 2, 6, .., 22 over j = 2 .. 23, consecutive rows joined at
    j = 23 and j = 2 alternately -- one long thin component"""
    dims = (26, 26, 4)
    s = np.zeros(dims, np.float32)
    rows = list(range(2, 23, 4))
    for i in rows:
        s[i, 2:24, 1] = 1.0
    for n, i in enumerate(rows[:-1]):
        s[i:i + 5, 23 if n % 2 == 0 else 2, 1] = 1.0
    return _unit(dims) + (F(0.5), s)


def dots_field():
    dims = (32, 32, 32)
    s = np.zeros(dims, np.float32)
    s[1:31:3, 1:31:3, 1:31:3] = 1.0
    return _unit(dims) + (F(0.5), s)


FIELDS = {
    "balls": balls_field,
    "twins": lambda: balls_field(with_first=False),
    "snake": snake_field,
    "noise33": lambda: tuple(noise_field((33, 33, 33), iso=0.88)),
    "noise17": lambda: tuple(noise_field((17, 16, 9), iso=0.88)),
    "dots": dots_field,
}


@functools.lru_cache(maxsize=None)
def field(name):
    """the field, its replayed mesh and its replayed components: computed once, shared, never written"""
    origin, cell, dims, iso, sigma = FIELDS[name]()
    mesh = mr.mesh(origin, cell, dims, iso, sigma)
    parts = cr.parts(len(mesh.vertices), mesh.triangles)
    for a in (sigma, mesh.vertices, mesh.triangles, parts.labels, parts.table):
        a.setflags(write=False)
    return Field(origin, cell, dims, iso, sigma, mesh, parts)


# ---------------------------------------------------------------- 0. the declarations
def test_the_header_declares_them_and_the_binding_has_them():
    import nerfhip as nh
    header = (ROOT / "include" / "nerfhip.h").read_text()
    want = {
        "nrf_mesh_components": ["nrf_context* ctx", "void* stream", "nrf_mesh_parts* out"],
        "nrf_read_mesh_components": ["nrf_context* ctx", "uint32_t* labels", "uint32_t* components"],
        "nrf_filter_mesh": ["nrf_context* ctx", "uint64_t min_triangles", "uint32_t flags", "void* stream", "nrf_mesh* out"],
    }
    lib = nh.load_library()
    for name, args in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m is not None, name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == args, name
        assert name in nh.exported_symbols()
        assert getattr(lib, name).restype is C.c_int
    assert lib.nrf_filter_mesh.argtypes[1] is C.c_uint64 and lib.nrf_filter_mesh.argtypes[2] is C.c_uint32
    assert re.search(r"enum\s*\{\s*NRF_MESH_KEEP_LARGEST\s*=\s*1\s*\}", header) and nh.NRF_MESH_KEEP_LARGEST == 1 == cr.KEEP_LARGEST
    assert header.index("int nrf_read_mesh_attributes") < header.index("typedef struct nrf_mesh_parts") < header.index("int nrf_mesh_components")
    assert "csrc/nrf_meshcc_plan.h is this text as code" in header
    assert C.sizeof(nh.MeshParts) == 32 and C.sizeof(nh.Mesh) == 40
    assert [f[0] for f in nh.MeshParts._fields_] == ["n_components", "labels", "components", "n_rounds", "reserved"]
    for method in ("mesh_components", "read_mesh_components", "filter_mesh"):
        assert callable(getattr(nh.NerfHip, method))
    assert nh.NRF_ABI_VERSION == 7 == lib.nrf_abi_version()  # an addition: the version does not change
    mirror = (HOST / "nerf_render.h").read_text()
    assert re.search(r"\bMeshComponents\s+mesh_components\s*\(\s*\)", mirror)
    assert re.search(r"\bMesh\s+filter_mesh\s*\(\s*uint64_t\s+min_triangles\s*,\s*bool\s+keep_largest\s*\)", mirror)
    testbed = (HOST / "testbed.cpp").read_text()
    assert '"--mesh_min_triangles"' in testbed and '"--mesh_largest"' in testbed
    assert testbed.index("extract_mesh(origin") < testbed.index("filter_mesh(mesh_min_triangles") < testbed.index("mesh_attributes(b /")


def test_the_struct_is_what_the_c_compiler_makes_of_the_header(tmp_path):
    import nerfhip as nh
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "s.c"
    src.write_text('#include "nerfhip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(nrf_mesh_parts),'
                   ' offsetof(nrf_mesh_parts, labels), offsetof(nrf_mesh_parts, components), offsetof(nrf_mesh_parts, n_rounds),'
                   ' offsetof(nrf_mesh_parts, reserved));return 0;}')
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "s")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()]
    P = nh.MeshParts
    assert got == [C.sizeof(P), P.labels.offset, P.components.offset, P.n_rounds.offset, P.reserved.offset]


def test_the_library_holds_the_kernels_and_the_scan_is_shared(tmp_path):
    import test_ray_hits_cpu as hcpu
    names = hcpu._kernel_names(tmp_path)
    for kernel in ("meshcc_init_kernel", "meshcc_hook_kernel", "meshcc_compress_kernel", "meshcc_roots_kernel", "meshcc_table_vertices_kernel",
                   "meshcc_table_triangles_kernel", "meshcc_best_kernel", "meshcc_keep_kernel", "meshcc_scatter_kernel"):
        assert any(re.search(r"\b" + kernel + r"\b", n) for n in names), kernel
    # one scan: the new file has no scan kernel of its own and launches the mesh's
    assert sorted(n.split("(")[0].split("::")[-1] for n in names if "scan" in n and "mesh" in n) == \
        ["mesh_scan_partials_kernel", "mesh_scan_reduce_kernel", "mesh_scan_write_kernel"], [n for n in names if "scan" in n]
    src = (ROOT / "nerf-cuda_amd" / "csrc" / "nrf_kernels_meshcc.hip").read_text()
    assert "asm" not in src  # plain C++ and HIP atomics
    api = (ROOT / "nerf-cuda_amd" / "csrc" / "nrf_api.hip").read_text()
    assert api.count("launch_mesh_scan(") >= 2 and "launch_mesh_scan(" in (ROOT / "nerf-cuda_amd" / "csrc" / "nrf_kernels_mesh.hip").read_text()


def test_the_make_target():
    mk = (HOST / "Makefile").read_text()
    assert re.search(r"^meshcc_asan: meshcc_plan_check$", mk, re.M)
    rule = mk.split("meshcc_plan_check: meshcc_plan_check.cpp")[1].split("\n# ")[0]
    assert "-fsanitize=address,undefined" in rule and "-fno-sanitize-recover=all" in rule
    for name in ("Makefile", "../CMakeLists.txt"):
        text = (ROOT / "nerf-cuda_amd" / name).read_text()
        assert "nrf_kernels_meshcc" in text and "nrf_meshcc_plan.h" in text, name


# ---------------------------------------------------------------- 1. the fields are what they should exercise
def test_the_fields():
    b = field("balls")
    assert (len(b.mesh.vertices), len(b.mesh.triangles)) == (3086, 6152)
    assert b.parts.table.tolist() == [[0, 1518, 3032], [440, 326, 648], [1844, 14, 24], [1858, 614, 1224], [1866, 614, 1224]]
    mr.check_closed_and_oriented(b.mesh.triangles)
    t = field("twins")
    assert sorted(t.parts.table[:, 2].tolist())[-2:] == [1224, 1224] and len(t.parts.table) == 4
    s = field("snake")
    assert (len(s.mesh.vertices), len(s.mesh.triangles), len(s.parts.table)) == (1756, 3508, 1)
    mr.check_closed_and_oriented(s.mesh.triangles)
    n = field("noise33")
    assert (len(n.mesh.vertices), len(n.mesh.triangles), len(n.parts.table)) == (69728, 131268, 1046)
    assert np.isnan(n.sigma).any() and np.isposinf(n.sigma).any() and np.isneginf(n.sigma).any()
    with pytest.raises(AssertionError):
        mr.check_closed_and_oriented(n.mesh.triangles)  # open at the boundary
    m = field("noise17")
    assert (len(m.mesh.vertices), len(m.mesh.triangles), len(m.parts.table)) == (4306, 7580, 90)
    d = field("dots")
    assert len(d.parts.table) == 1000 and np.all(d.parts.table[:, 1] == 14) and np.all(d.parts.table[:, 2] == 24)
    for name in FIELDS:
        f = field(name)
        cr.check_parts(f.parts.labels, f.parts.table, len(f.mesh.vertices), f.mesh.triangles)
        print(f"{name}: {len(f.mesh.vertices)} vertices, {len(f.mesh.triangles)} triangles, {len(f.parts.table)} components, "
              f"{f.parts.sweeps} sweeps of plain label propagation")
    assert s.parts.sweeps > 40  # a labelling that stops after a fixed few passes fails here
    # ... and the checker does refuse: a label that is not the minimum, a merged pair of components, a wrong count
    bad = b.parts.labels.copy()
    bad[bad == 440] = 441
    with pytest.raises(AssertionError):
        cr.check_parts(bad, b.parts.table, len(bad), b.mesh.triangles)
    bad = b.parts.labels.copy()
    bad[1] = 1
    with pytest.raises(AssertionError):
        cr.check_parts(bad, b.parts.table, len(bad), b.mesh.triangles)
    wrong = b.parts.table.copy()
    wrong[0, 2] -= 1
    with pytest.raises(AssertionError):
        cr.check_parts(b.parts.labels, wrong, len(b.parts.labels), b.mesh.triangles)


def test_the_keep_rule_of_the_replay():
    table = field("balls").parts.table
    assert cr.kept_labels(table, 25, 0) == [0, 440, 1858, 1866] and cr.kept_labels(table, 649, 0) == [0, 1858, 1866]
    assert cr.kept_labels(table, 0, 1) == [0] and cr.kept_labels(table, 3032, 1) == [0] and cr.kept_labels(table, 3033, 1) == []
    assert cr.kept_labels(field("twins").parts.table, 0, 1) == [int(field("twins").parts.table[-2, 0])]  # the lower-labelled twin
    assert cr.kept_labels(field("dots").parts.table, 24, 1) == [0] and len(cr.kept_labels(field("dots").parts.table, 24, 0)) == 1000
    assert cr.kept_labels(np.zeros((0, 3), np.uint32), 0, 1) == []


# ---------------------------------------------------------------- 2. one text of the definition
@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("meshcc") / "meshcc_plan_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", str(exe), str(HOST / "meshcc_plan_check.cpp")], check=True)
    return exe


def _problem(n_vertices, triangles, min_triangles, flags):
    t = np.asarray(triangles, np.int64).reshape(-1)
    return f"{n_vertices} {len(t) // 3} {min_triangles} {flags}\n" + " ".join(map(str, t.tolist())) + "\n"


def _run(exe, problems):
    """[(labels, table, n_rounds, old vertex ids, remapped triangles)] of the check program on a list of (nv, triangles, min, flags)"""
    out = subprocess.run([str(exe)], input="".join(_problem(*p) for p in problems), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"meshcc_plan_check: {len(problems)} problems" in out.stderr
    lines, at, res = out.stdout.splitlines(), 0, []

    def block(tag, count, width):
        nonlocal at
        rows = lines[at:at + count]
        assert len(rows) == count and all(r.startswith(tag + " ") for r in rows), (tag, at)
        at += count
        return np.array(" ".join(r[len(tag) + 1:] for r in rows).split(), np.int64).astype(np.uint32).reshape(count, width) if count else np.zeros((0, width), np.uint32)

    while at < len(lines):
        head = lines[at].split()
        assert head[0] == "parts" and head[4] == "1", head
        nv, nc, rounds = int(head[1]), int(head[2]), int(head[3])
        at += 1
        lab, table = block("l", nv, 1).reshape(-1), block("c", nc, 3)
        kept = lines[at].split()
        assert kept[0] == "kept" and kept[3] == "1", kept
        at += 1
        res.append((lab, table, rounds, block("o", int(kept[1]), 1).reshape(-1), block("t", int(kept[2]), 3)))
    assert len(res) == len(problems)
    return res


def _same(got, problem, want=None):
    nv, triangles, min_triangles, flags = problem
    lab, table, rounds, old, tri = got
    want = want or cr.parts(nv, triangles)
    assert np.array_equal(lab, want.labels) and np.array_equal(table, want.table), (nv, min_triangles, flags)
    cr.check_parts(lab, table, nv, triangles)
    f = cr.filter_mesh(want, nv, triangles, min_triangles, flags)
    assert np.array_equal(old, f.old_vertex) and np.array_equal(tri, f.triangles), (nv, min_triangles, flags)
    assert rounds >= (1 if nv else 0)
    return want, f


def test_the_check_program_is_the_replay_on_hand_made_lists(check_program):
    lists = [
        (0, []),                                # the empty mesh
        (3, [(0, 1, 2)]),                       # one triangle
        (5, [(0, 1, 2)]),                       # ... and two vertices no triangle names
        (5, [(0, 1, 2), (2, 3, 4)]),            # two triangles sharing one vertex
        (9, [(6, 7, 8), (3, 4, 5), (5, 6, 2)]),  # hooks that arrive from above
        (7, [(6, 5, 4), (4, 3, 2), (2, 1, 0)]),  # a descending chain
        (4, []),                                # vertices only
    ]
    problems = [(nv, np.array(t, np.uint32).reshape(-1, 3), m, f) for nv, t in lists for m, f in CUTS + [(2, 0), (2, 1)]]
    got = _run(check_program, problems)
    for g, p in zip(got, problems):
        _same(g, p)
    by = {(p[0], len(p[1]), p[2], p[3]): g for g, p in zip(got, problems)}
    assert by[(5, 1, 0, 0)][1].tolist() == [[0, 3, 1], [3, 1, 0], [4, 1, 0]]
    assert by[(0, 0, 0, 0)][1].shape == (0, 3) and by[(0, 0, 0, 1)][3].shape == (0,) and by[(0, 0, 0, 0)][2] == 0
    assert by[(5, 2, 2, 1)][1].tolist() == [[0, 5, 2]] and by[(5, 2, 2, 1)][4].tolist() == [[0, 1, 2], [2, 3, 4]]
    assert by[(5, 1, 1, 0)][3].tolist() == [0, 1, 2] and by[(5, 1, 0, 1)][3].tolist() == [0, 1, 2] and by[(5, 1, 2, 1)][3].tolist() == []
    assert by[(4, 0, 0, 1)][3].tolist() == [0] and by[(4, 0, 0, 0)][3].tolist() == [0, 1, 2, 3] and by[(4, 0, 1, 0)][3].tolist() == []
    # an unknown flag bit is refused by the plan's own predicate
    out = subprocess.run([str(check_program)], input="3 1 0 2\n0 1 2\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0] == "parts 3 1 2 0" and out[-1] == "kept 0 0 0"


@pytest.mark.parametrize("name", list(FIELDS))
def test_the_check_program_is_the_replay_on_the_fields(check_program, name):
    f = field(name)
    nv, t = len(f.mesh.vertices), f.mesh.triangles
    problems = [(nv, t, m, flags) for m, flags in CUTS]
    kept = []
    for g, p in zip(_run(check_program, problems), problems):
        want, flt = _same(g, p, f.parts)
        kept.append(len(flt.old_triangle))
        if p[2] == 0 and p[3] == 0:  # keeping everything leaves the indices as they were
            assert np.array_equal(g[4], t) and np.array_equal(g[3], np.arange(nv))
            print(f"{name}: {g[2]} rounds of hook + compress in the serial reference")
    assert kept[0] == len(t) and kept[-1] == 0 and kept[-2] == 0  # (min_triangles = 10^9 keeps nothing, with or without the flag)
    assert kept[1] == int(f.parts.table[:, 2].max())  # (0, KEEP_LARGEST)


# ---------------------------------------------------------------- 3. the labelling under stale loads
STALE_SEEDS = 64
STALE_FIELDS = ["snake", "balls", "twins", "noise17", "dots"]


@pytest.fixture(scope="module")
def stale_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("meshcc_stale") / "meshcc_stale_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", str(exe), str(HOST / "meshcc_stale_check.cpp")], check=True)
    return exe


def _run_stale(exe, problems, seeds=STALE_SEEDS):
    """{name: (labels, least rounds, most rounds, host rounds, walks, stale walks)} of the stale-load program on [(name, nv, triangles)]"""
    text = "".join(f"{name} {nv} {len(np.asarray(t).reshape(-1)) // 3} {seeds}\n" + " ".join(map(str, np.asarray(t, np.int64).reshape(-1).tolist())) + "\n"
                   for name, nv, t in problems)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"meshcc_stale_check: {len(problems)} problems" in out.stderr
    lines, at, res = out.stdout.splitlines(), 0, {}
    for name, nv, t in problems:
        head = lines[at].split()
        assert head[:4] == ["mesh", name, str(nv), str(len(np.asarray(t).reshape(-1)) // 3)] and head[4:6] == ["runs", str(2 * seeds)], head
        assert [head[6], head[9], head[11], head[13]] == ["rounds", "host", "walks", "stale"], head
        rows = lines[at + 1:at + 1 + nv]
        assert len(rows) == nv and all(r.startswith("l ") for r in rows)
        res[name] = (np.array([r[2:] for r in rows], np.int64).astype(np.uint32), int(head[7]), int(head[8]), int(head[10]), int(head[12]), int(head[14]))
        at += 1 + nv
    assert at == len(lines)
    return res


def _hand_made():
    """[(name, nv, triangles)]: each list with ascending, descending and shuffled vertex numbering; an index >= nv stays invalid"""
    lists = {
        "fan": (10, [(0, i, i + 1) for i in range(1, 9)]),
        "strip": (40, [(i, i + 1, i + 2) for i in range(38)]),
        "pair": (5, [(0, 1, 2), (2, 3, 4)]),                                   # two triangles that share one vertex
        "lonely": (6, [(0, 1, 2), (2, 4, 5)]),                                 # vertex 3 is named by no triangle
        "invalid": (9, [(0, 1, 2), (2, 3, 9), (3, 4, 5), (5, 6, 0xffffffff), (6, 7, 8), (8, 4, 3)]),
        "comb": (64, [(i, i + 1, 63 - i) for i in range(0, 31)] + [(2 * i, 2 * i + 1, 62) for i in range(31)]),
    }
    out = []
    for name, (nv, tri) in lists.items():
        t = np.array(tri, np.int64).reshape(-1, 3)
        for order, perm in (("up", np.arange(nv)), ("down", np.arange(nv)[::-1]), ("mixed", np.random.default_rng(nv).permutation(nv))):
            out.append((f"{name}_{order}", nv, np.where(t < nv, perm[np.minimum(t, nv - 1)], t)))
    return out


def test_the_stale_make_target():
    mk = (HOST / "Makefile").read_text()
    assert re.search(r"^meshcc_stale_asan: meshcc_stale_check$", mk, re.M)
    rule = mk.split("meshcc_stale_check: meshcc_stale_check.cpp ../csrc/nrf_meshcc_plan.h")[1].split("\n# ")[0]
    assert "-fsanitize=address,undefined" in rule and "-fno-sanitize-recover=all" in rule
    assert "meshcc_stale_check" in mk.split("\nclean:")[1].split("\n#")[0]
    # one text: the kernels, the serial reference and the stale-load program call the same hook and compress
    plan = (ROOT / "nerf-cuda_amd" / "csrc" / "nrf_meshcc_plan.h").read_text()
    kernels = (ROOT / "nerf-cuda_amd" / "csrc" / "nrf_kernels_meshcc.hip").read_text()
    program = (HOST / "meshcc_stale_check.cpp").read_text()
    for fn in ("meshcc_hook_lower(", "meshcc_compress("):
        assert plan.count(fn) >= 2 and fn in kernels and fn in program, fn
    assert "atomicMin(&parent[root], low)" in kernels
    assert "meshcc_hook_of(" in program and "meshcc_root(" in program and "meshcc_triangle_valid(" in program


def test_stale_loads_on_hand_made_lists(stale_program):
    problems = _hand_made()
    assert len(problems) == 18
    got = _run_stale(stale_program, problems)
    for name, nv, t in problems:
        lab, lo, hi, host, walks, stale = got[name]
        want = cr.parts(nv, t[np.all(t < nv, axis=1)])  # (the replay knows no invalid index: such a triangle joins nothing)
        assert np.array_equal(lab, want.labels), name
        assert 1 <= lo <= hi <= nv + 1, (name, lo, hi)
        assert stale > 0 or nv < 10, name  # the memory did hand out old values (two triangles may leave none to hand out)
        print(f"{name}: {nv} vertices, rounds {lo} .. {hi} over {2 * STALE_SEEDS} runs (serial {host}), {stale} of {walks} walks loaded an old value")
    assert got["lonely_up"][0].tolist() == [0, 0, 0, 3, 0, 0] and got["invalid_up"][0].tolist() == [0, 0, 0, 3, 3, 3, 3, 3, 3]


@pytest.mark.parametrize("name", STALE_FIELDS)
def test_stale_loads_on_the_fields(stale_program, name):
    f = field(name)
    nv = len(f.mesh.vertices)
    lab, lo, hi, host, walks, stale = _run_stale(stale_program, [(name, nv, f.mesh.triangles)])[name]
    assert np.array_equal(lab, f.parts.labels)
    assert 2 <= lo <= hi <= nv + 1
    assert stale > 0
    print(f"{name}: {nv} vertices, rounds {lo} .. {hi} over {2 * STALE_SEEDS} runs (serial {host}), {stale} of {walks} walks loaded an old value")
