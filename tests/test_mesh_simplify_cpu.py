"""nrf_simplify_mesh / nrf_read_mesh_simplification, the parts that need no GPU: the declarations, the bindings and the mirrors, and
the one text of the definition -- host/simplify_plan_check.cpp (csrc/nrf_simplify_plan.h under AddressSanitizer + UBSan) against
tests/simplify_replay.py, the numpy replay the GPU tests use: kept vertices, edge words, sources, vertex_map and remapped triangles,
identical, and every vertex's own cluster, key and representative.  The simplified fields the GPU tests share are built here.  Every
test here needs the feature: none passes without it."""
import ctypes as C
import functools
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_replay as mr
import refine_replay as rr
import simplify_replay as sr
import test_mesh_components_cpu as cc

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "nerf-cuda_amd" / "host"
F = np.float32
FACTORS = [1, 2, 3, 4, 7]  # 7 exceeds dots' spacing and divides no dimension of any field
CLOSED = ["balls", "twins", "snake", "dots"]
# (vertices, triangles) of the replay at factors 1, 2, 3, 4, 7
COUNTS = {
    "balls": [(1060, 2100), (270, 524), (126, 236), (78, 148), (24, 32)],
    "twins": [(552, 1088), (140, 268), (64, 116), (44, 76), (16, 20)],
    "snake": [(592, 1180), (144, 272), (32, 56), (0, 0), (8, 12)],
    "noise33": [(27673, 57154), (4635, 14188), (1315, 5664), (708, 3442), (124, 980)],
    "noise17": [(1776, 3268), (338, 862), (98, 256), (58, 208), (18, 70)],
    "dots": [(8000, 12000), (2500, 3000), (0, 0), (432, 1080), (112, 480)],
}


@functools.lru_cache(maxsize=None)
def words(name):
    """the edge words of the field's replayed mesh: computed once, shared, never written"""
    f = cc.field(name)
    w = rr.edge_words(f.mesh, f.dims)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def simplified(name, factor):
    """the replay's simplification of the field's replayed mesh: computed once, shared, never written"""
    f = cc.field(name)
    s = sr.simplify(f.origin, f.cell, f.dims, factor, words(name), f.mesh.vertices, f.mesh.triangles)
    for a in s:
        a.setflags(write=False)
    return s


# ---------------------------------------------------------------- 0. the declarations
def test_the_header_declares_them_and_the_binding_has_them(tmp_path):
    import nerfhip as nh
    header = (ROOT / "include" / "nerfhip.h").read_text()
    want = {
        "nrf_simplify_mesh": ["nrf_context* ctx", "uint32_t factor", "void* stream", "nrf_mesh_simplify* out"],
        "nrf_read_mesh_simplification": ["nrf_context* ctx", "uint32_t* sources", "uint32_t* vertex_map"],
    }
    lib = nh.load_library()
    for name, args in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m is not None, name
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == args, name
        assert name in nh.exported_symbols()
        assert getattr(lib, name).restype is C.c_int
    assert lib.nrf_simplify_mesh.argtypes[1] is C.c_uint32
    fields = ["n_vertices", "n_triangles", "n_vertices_before", "n_triangles_before", "vertices", "triangles", "edges", "sources", "vertex_map",
              "factor", "reserved"]
    assert [f[0] for f in nh.MeshSimplify._fields_] == fields
    for method in ("simplify_mesh", "read_mesh_simplification"):
        assert callable(getattr(nh.NerfHip, method))
    assert nh.NRF_ABI_VERSION == 7 == lib.nrf_abi_version()  # an addition: the version does not change
    # the struct as the C compiler lays it out
    cc_ = shutil.which("gcc") or shutil.which("cc")
    if cc_ is not None:
        src, exe = tmp_path / "s.c", tmp_path / "s"
        src.write_text('#include "nerfhip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(){printf("%zu", sizeof(nrf_mesh_simplify));\n'
                       + "".join(f'printf(" %zu", offsetof(nrf_mesh_simplify, {f}));\n' for f in fields) + "return 0;}")
        subprocess.run([cc_, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert sizes == [C.sizeof(nh.MeshSimplify)] + [getattr(nh.MeshSimplify, f).offset for f in fields]
        assert sizes == [80, 0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76]
    assert header.index("int nrf_read_mesh_refinement") < header.index("typedef struct nrf_mesh_simplify") < header.index("int nrf_simplify_mesh")
    comment = header[header.index("Mesh simplification"):header.index("typedef struct nrf_mesh_simplify")]
    assert "csrc/nrf_simplify_plan.h is this text as code" in comment and "(uint64)hi << 32 | v" in comment and "0x7f800000" in comment
    assert "16 MB for a 256^3 lattice at factor 2" in comment
    mirror = (HOST / "nerf_render.h").read_text()
    assert re.search(r"\bSimplifiedMesh\s+simplify_mesh\s*\(\s*uint32_t\s+factor\s*\)", mirror)
    testbed = (HOST / "testbed.cpp").read_text()
    assert '"--mesh_simplify"' in testbed
    assert testbed.index("filter_mesh(mesh_min_triangles") < testbed.index("refine_mesh((uint32_t)mesh_refine") \
        < testbed.index("simplify_mesh((uint32_t)mesh_simplify") < testbed.index("mesh_attributes(b /")


def test_the_library_holds_the_kernels_and_the_scan_is_shared(tmp_path):
    import test_ray_hits_cpu as hcpu
    names = hcpu._kernel_names(tmp_path)
    for kernel in ("simplify_key_kernel", "simplify_triangle_kernel", "simplify_codes_kernel", "simplify_scatter_kernel"):
        assert any(re.search(r"\b" + kernel + r"\b", n) for n in names), kernel
    # one scan: the new file has no scan kernel of its own and launches the mesh's
    assert sorted(n.split("::")[-1] for n in names if "scan" in n and "mesh" in n) == ["mesh_scan_partials_kernel", "mesh_scan_reduce_kernel", "mesh_scan_write_kernel"]
    src = (ROOT / "nerf-cuda_amd" / "csrc" / "nrf_kernels_simplify.hip").read_text()
    assert "asm" not in src and "atomicMin(&keys[cid]" in src  # plain C++ and HIP atomics
    assert "SIMPLIFY_MAX_GROUPS = 2048" in src and "__launch_bounds__(256)" in src
    api = (ROOT / "nerf-cuda_amd" / "csrc" / "nrf_api.hip").read_text()
    body = api[api.index("int nrf_simplify_mesh("):api.index("int nrf_read_mesh_simplification(")]
    assert "launch_mesh_scan(" in body and "launch_simplify_mark(" in body and "launch_simplify_scatter(" in body


def test_the_make_target():
    mk = (HOST / "Makefile").read_text()
    assert re.search(r"^simplify_asan: simplify_plan_check$", mk, re.M)
    rule = mk.split("simplify_plan_check: simplify_plan_check.cpp")[1].split("\n# ")[0]
    assert "-fsanitize=address,undefined" in rule and "-ffp-contract=off" in rule and "-fno-sanitize-recover=all" in rule
    for name in ("Makefile", "../CMakeLists.txt"):
        text = (ROOT / "nerf-cuda_amd" / name).read_text()
        assert "nrf_kernels_simplify" in text and "nrf_simplify_plan.h" in text, name


# ---------------------------------------------------------------- 1. the replay and the checkers
def test_the_replay_on_the_fields_and_what_it_keeps():
    for name, counts in COUNTS.items():
        f = cc.field(name)
        got = []
        for factor in FACTORS:
            s = simplified(name, factor)
            got.append((len(s.vertices), len(s.triangles)))
            sr.check_all(s.vertices, s.triangles, s.edges, s.sources, s.vertex_map, f.mesh.vertices, words(name), f.dims, factor)
        print(f"{name}: {len(f.mesh.vertices)} / {len(f.mesh.triangles)} -> {got}")
        assert got == counts, name
    # duplicate triangles are kept: the legs that have some
    for name, factor, dup in (("dots", 4, 270), ("dots", 7, 264), ("noise17", 3, 20), ("noise17", 4, 26), ("noise33", 3, 204), ("balls", 4, 0)):
        t = simplified(name, factor).triangles
        assert len(t) - len(np.unique(t, axis=0)) == dup, (name, factor)


@pytest.mark.parametrize("name", CLOSED)
def test_closed_before_is_balanced_after(name):
    f = cc.field(name)
    mr.check_closed_and_oriented(f.mesh.triangles)
    sr.check_balanced(f.mesh.triangles)
    for factor in FACTORS:
        sr.check_balanced(simplified(name, factor).triangles)
    with pytest.raises(AssertionError):  # ... and the noise is open at the boundary, before and after
        sr.check_balanced(simplified("noise17", 2).triangles)


def test_the_signed_volume_of_the_balls():
    f = cc.field("balls")
    before = sr.signed_volume(f.mesh.vertices, f.mesh.triangles)
    assert before > 0  # (counter-clockwise seen from outside)
    for factor in (1, 2):
        s = simplified("balls", factor)
        after = sr.signed_volume(s.vertices, s.triangles)
        print(f"balls: signed volume {before:.3f} -> {after:.3f} at factor {factor}")
        assert 0 < after < before


def test_each_checker_rejects_a_wrong_mesh():
    f, w, s = cc.field("balls"), words("balls"), simplified("balls", 2)
    args = [s.vertices, s.triangles, s.edges, s.sources, s.vertex_map, f.mesh.vertices, w, f.dims, 2]
    sr.check_all(*args)

    def wrong(index, change):
        bad = list(args)
        bad[index] = args[index].copy()
        change(bad[index])
        return bad

    def set_(i, value):
        def change(a):
            a[i] = value
        return change

    with pytest.raises(AssertionError, match="collapsed"):
        sr.check_triangles(wrong(1, set_((5, 1), s.triangles[5, 0]))[1], len(s.vertices))
    with pytest.raises(AssertionError, match="out of range"):
        sr.check_triangles(wrong(1, set_((7, 2), len(s.vertices)))[1], len(s.vertices))
    with pytest.raises(AssertionError, match="unreferenced"):
        sr.check_referenced(s.triangles, len(s.vertices) + 1)
    only = int(s.triangles[0, 0])
    with pytest.raises(AssertionError, match="unreferenced"):  # every mention of one vertex rerouted to another
        sr.check_referenced(np.where(s.triangles == only, s.triangles[0, 1], s.triangles), len(s.vertices))
    swapped = s.sources.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    with pytest.raises(AssertionError, match="ascend"):
        sr.check_sources(swapped, s.vertices, s.edges, f.mesh.vertices, w)
    moved = s.vertices.copy()
    moved[9, 1] = np.nextafter(moved[9, 1], F(np.inf))
    with pytest.raises(AssertionError, match="bits"):
        sr.check_sources(s.sources, moved, s.edges, f.mesh.vertices, w)
    with pytest.raises(AssertionError, match="edge word"):
        sr.check_sources(s.sources, s.vertices, wrong(2, set_(0, int(s.edges[0]) ^ 1))[2], f.mesh.vertices, w)
    kept_one = int(s.sources[2])
    with pytest.raises(AssertionError, match="itself"):
        sr.check_vertex_map(wrong(4, set_(kept_one, 3))[4], s.sources, w, f.dims, 2)
    with pytest.raises(AssertionError, match="beyond"):
        sr.check_vertex_map(wrong(4, set_(0, len(s.sources)))[4], s.sources, w, f.dims, 2)
    # an entry of a dropped vertex pointed at another cluster's representative, and two entries in one cluster
    dropped = int(np.nonzero((s.vertex_map != sr.NONE) & ~np.isin(np.arange(len(w)), s.sources))[0][0])
    other = (int(s.vertex_map[dropped]) + 1) % len(s.sources)
    with pytest.raises(AssertionError, match="cluster"):
        sr.check_vertex_map(wrong(4, set_(dropped, other))[4], s.sources, w, f.dims, 2)
    with pytest.raises(AssertionError, match="cluster"):
        sr.check_vertex_map(wrong(4, set_(dropped, sr.NONE))[4], s.sources, w, f.dims, 2)
    with pytest.raises(AssertionError, match="directed edge"):
        sr.check_balanced(s.triangles[1:])
    with pytest.raises(AssertionError, match="directed edge"):  # one triangle turned over
        sr.check_balanced(wrong(1, set_(0, s.triangles[0, ::-1].copy()))[1])
    sr.check_balanced(np.zeros((0, 3), np.uint32))
    sr.check_balanced(np.array([[0, 1, 2], [0, 2, 1]], np.uint32))  # mutually opposite: balanced, and kept


# ---------------------------------------------------------------- 2. one text of the definition
@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("simplify") / "simplify_plan_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe), str(HOST / "simplify_plan_check.cpp")], check=True)
    return exe


def _problem(origin, cell, dims, factor, w, vertices, triangles):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).view(np.uint32)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    head = " ".join(f"{x:08x}" for x in mr.bits(list(origin) + list(cell)).reshape(-1)) + " " + " ".join(str(int(d)) for d in dims)
    rows = "\n".join(f"{int(a)} {x:08x} {y:08x} {z:08x}" for a, (x, y, z) in zip(np.asarray(w).tolist(), v.tolist()))
    return f"{head} {int(factor)} {len(v)} {len(t)}\n{rows}\n" + " ".join(map(str, t.reshape(-1).tolist())) + "\n"


def _run(exe, problems):
    """[(cluster, key, rep, sources, edges, vertex bits, vertex_map, triangles)] of the check program on a list of _problem arguments"""
    out = subprocess.run([str(exe)], input="".join(_problem(*p) for p in problems), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"simplify_plan_check: {len(problems)} problems" in out.stderr
    lines, at, res = out.stdout.splitlines(), 0, []

    def block(tag, count):
        nonlocal at
        rows = lines[at:at + count]
        assert len(rows) == count and all(r.startswith(tag + " ") for r in rows), (tag, at)
        at += count
        return [r.split()[1:] for r in rows]

    for _ in problems:
        head = lines[at].split()
        assert head[0] == "simplified" and head[5:] == ["1", "1"], head
        kv, kt, nv = int(head[1]), int(head[2]), int(head[3])
        at += 1
        r, o, m, t = block("r", nv), block("o", kv), block("m", nv), block("t", kt)
        res.append((np.array([int(x[0]) for x in r], np.int64), np.array([int(x[1], 16) for x in r], np.uint64), np.array([int(x[2]) for x in r], np.int64),
                    np.array([int(x[0]) for x in o], np.uint32), np.array([int(x[1]) for x in o], np.uint32),
                    np.array([[int(y, 16) for y in x[2:]] for x in o], np.uint32).reshape(kv, 3), np.array([int(x[0]) for x in m], np.uint32),
                    np.array(t, np.int64).astype(np.uint32).reshape(kt, 3)))
    assert at == len(lines)
    return res


def _same(got, problem, want=None):
    origin, cell, dims, factor, w, vertices, triangles = problem
    want = want or sr.simplify(origin, cell, dims, factor, w, vertices, triangles)
    cluster, key, rep, sources, edges, bits, vmap, tri = got
    none = want.cluster < 0
    assert np.array_equal(np.where(cluster == sr.NONE, -1, cluster), want.cluster), factor
    assert np.array_equal(key[~none], want.key[~none]) and np.array_equal(np.where(rep == sr.NONE, -1, rep), want.rep), factor
    assert np.array_equal(sources, want.sources) and np.array_equal(edges, want.edges) and np.array_equal(vmap, want.vertex_map), factor
    assert np.array_equal(bits, want.vertices.view(np.uint32).reshape(-1, 3)) and np.array_equal(tri, want.triangles), factor
    return want


@pytest.mark.parametrize("name", list(cc.FIELDS))
def test_the_check_program_is_the_replay_on_the_fields(check_program, name):
    f = cc.field(name)
    problems = [(f.origin, f.cell, f.dims, factor, words(name), f.mesh.vertices, f.mesh.triangles) for factor in FACTORS]
    for g, p, counts in zip(_run(check_program, problems), problems, COUNTS[name]):
        want = _same(g, p, simplified(name, p[3]))
        assert (len(want.sources), len(want.triangles)) == counts
        sr.check_all(g[5].view(np.float32), g[7], g[4], g[3], g[6], f.mesh.vertices, words(name), f.dims, p[3])


def test_the_check_program_on_a_corner_and_on_a_triangle_out_of_range(check_program):
    # a 2 x 2 x 2 lattice with corner 0 the only inside one: all seven edges of point 0 cross, one owner point, one cluster at every factor
    s = np.zeros((2, 2, 2), np.float32)
    s[0, 0, 0] = 1.0
    origin, cell, dims = [-1.0, 0.5, 2.0], [0.5, 0.25, 2.0], (2, 2, 2)
    m = mr.mesh(origin, cell, dims, F(0.5), s)
    w = rr.edge_words(m, dims)
    assert len(m.vertices) == 7 and len(m.triangles) == 6 and sorted(w.tolist()) == [1, 2, 3, 4, 5, 6, 7]
    # ... and with the opposite corner the only inside one: seven edges of seven owner points, the same fan of six triangles
    s7 = np.zeros((2, 2, 2), np.float32)
    s7[1, 1, 1] = 1.0
    m7 = mr.mesh(origin, cell, dims, F(0.5), s7)
    w7 = rr.edge_words(m7, dims)
    assert len(m7.vertices) == 7 and sorted((w7 >> 3).tolist()) == [0, 1, 2, 3, 4, 5, 6] and len(m7.triangles) == 6
    problems = [(origin, cell, dims, k, w, m.vertices, m.triangles) for k in (1, 2, 256)]
    problems += [(origin, cell, dims, k, w7, m7.vertices, m7.triangles) for k in (2, 3)]
    far = (origin, cell, dims, 1, w7, m7.vertices, m7.triangles)
    # a triangle that names a vertex out of range is dropped, the others are not disturbed
    f = cc.field("noise17")
    bad = f.mesh.triangles.copy()
    bad[5, 1] = len(f.mesh.vertices)
    bad[11, 2] = 0xFFFFFFFF
    problems += [(f.origin, f.cell, f.dims, k, words("noise17"), f.mesh.vertices, bad) for k in (1, 2)]
    # an edge word whose point is not in the lattice has no cluster: its vertex is dropped with the triangles that name it
    odd = words("noise17").copy()
    odd[3] = (int(np.prod(f.dims)) << 3) | 1
    problems += [(f.origin, f.cell, f.dims, 1, odd, f.mesh.vertices, f.mesh.triangles)]
    got = _run(check_program, problems)
    for g, p in zip(got, problems):
        _same(g, p)
    for g in got[:5]:  # one owner point: one cluster at every factor, every triangle collapses, nothing is left
        assert len(g[3]) == 0 and len(g[7]) == 0 and np.all(g[6] == sr.NONE) and len(set(g[2].tolist())) == 1
    for g, k in zip(got[5:7], (1, 2)):  # ... as if the two triangles had not been there
        without = sr.simplify(f.origin, f.cell, f.dims, k, words("noise17"), f.mesh.vertices, np.delete(bad, [5, 11], axis=0))
        assert np.array_equal(g[7], without.triangles) and np.array_equal(g[3], without.sources)
    assert got[7][0][3] == sr.NONE and 3 not in got[7][3].tolist()
    g = _run(check_program, [far])[0]  # seven clusters of one vertex each at factor 1: the mesh as it was
    _same(g, far)
    assert np.array_equal(g[3], np.arange(7)) and np.array_equal(g[7], m7.triangles) and np.array_equal(g[6], np.arange(7))
    # an empty mesh, and a factor the entry point refuses
    empty = (origin, cell, dims, 3, np.zeros(0, np.uint32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    g = _run(check_program, [empty])[0]
    assert all(len(a) == 0 for a in g)
    for factor in (0, 257, 0xFFFFFFFF):
        out = subprocess.run([str(check_program)], input=_problem(*empty[:3], factor, *empty[4:]), capture_output=True, text=True, check=True)
        assert out.stdout.split() == ["simplified", "0", "0", "0", "0", "0", "0"], factor


def test_the_key_rule_with_nan_inf_and_ties(check_program):
    """positions moved by hand: NaN and +-inf rank last (0x7f800000), equal distances go to the smaller id"""
    f = cc.field("balls")
    w = words("balls")
    factor = 2
    base = simplified("balls", factor)
    v = f.mesh.vertices.copy()
    members = [np.nonzero(base.cluster == c)[0] for c in np.unique(base.cluster)]
    big = [m for m in members if len(m) >= 4]
    assert len(big) >= 6
    # cluster 0: its representative becomes NaN -> another member wins;  1: +inf;  2: -inf in one coordinate;
    # 3: ALL members NaN or inf -> the smallest id wins;  4, 5: two members put on the centre itself -> the smaller id wins
    r0 = int(base.rep[big[0][0]])
    v[r0, 0] = np.nan
    r1 = int(base.rep[big[1][0]])
    v[r1] = np.inf
    r2 = int(base.rep[big[2][0]])
    v[r2, 2] = -np.inf
    v[big[3]] = np.nan
    v[big[3][1], 0] = np.inf
    nb = sr.blocks(f.dims, factor)

    def centre(members_):
        c = int(base.cluster[members_[0]])
        b = [c // (nb[1] * nb[2]), (c // nb[2]) % nb[1], c % nb[2]]
        return np.array([(2 * b[k] + 1) * factor * 0.5 for k in range(3)], np.float32)  # (origin 0, cell 1: exact)

    for group in (big[4], big[5]):
        v[group[1]] = centre(group)  # (d2 == +0: key == the id)
        v[group[3]] = centre(group)
    problem = (f.origin, f.cell, f.dims, factor, w, v, f.mesh.triangles)
    g = _run(check_program, [problem])[0]
    want = _same(g, problem)
    cluster, key, rep = g[0], g[1], g[2]
    hi = (key >> np.uint64(32)).astype(np.int64)
    for r in (r0, r1, r2):
        assert hi[r] == 0x7F800000 and rep[r] != r and hi[rep[r]] < 0x7F800000
    assert np.all(hi[big[3]] == 0x7F800000) and np.all(rep[big[3]] == big[3][0])
    for group in (big[4], big[5]):
        assert key[group[1]] == group[1] and key[group[3]] == group[3] and np.all(rep[group] == group[1])
    # the key rule, whatever made the keys: the low word is the id, the high word orders as d2 does, rep is the arg-min of its cluster
    assert np.array_equal((key & np.uint64(0xFFFFFFFF)).astype(np.int64), np.arange(len(v)))
    for m in members:
        assert np.all(rep[m] == m[np.argmin(key[m])])
    sr.check_all(g[5].view(np.float32), g[7], g[4], g[3], g[6], v, w, f.dims, factor)
    sr.check_balanced(g[7])  # moving vertices does not open the chain
    assert len(want.sources) == len(base.sources)  # one representative per cluster, as before
