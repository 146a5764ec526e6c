"""nrf_simplify_mesh and nrf_read_mesh_simplification on the GPU.

The definition (include/nerfhip.h, csrc/nrf_simplify_plan.h) is held index for index and bit for bit to tests/simplify_replay.py, the
numpy replay -- one sort by (cluster, key), a different algorithm from the kernels' atomic minimum into a key table -- that
tests/test_mesh_simplify_cpu.py holds to the plan header; what a simplified mesh has to be whatever the code says is checked by
simplify_replay's property checkers, which share no code with either.  The fields are test_mesh_components_cpu's: caller-supplied
sigma lattices, so no model is needed except where one is the point.  Nothing here rests on a tolerance.  Every test here needs the
entry points: none passes without them."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_replay as mr
import meshcc_replay as cr
import nerfhip as nh
import refine_replay as rr
import simplify_replay as sr
import test_density_points_gpu as dp
import test_point_attributes_cpu as pac
from test_mesh_components_cpu import FIELDS, field
from test_mesh_components_gpu import _filter, _mesh_of, _snapshot
from test_mesh_cpu import noise_field
from test_mesh_gpu import ISO, _blob, _box_lattice, _extract, _lattice_sigma, _peek
from test_mesh_refine_gpu import _off_fp16, _refine
from test_mesh_simplify_cpu import COUNTS, FACTORS, simplified, words
from test_point_attributes_gpu import _mesh_attributes, _step
from test_ray_hits_gpu import _fnv1a
from test_render_rays_clip_gpu import _bits, _context, _upload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
HOSTDIR = ROOT / "nerf-cuda_amd" / "host"
F = np.float32
LARGEST = cr.KEEP_LARGEST


def _simplify(ctx, factor, before):
    """(struct, vertices, triangles, edges, sources, vertex_map) of one nrf_simplify_mesh call on a mesh of `before` = (vertices,
    triangles); the arrays through nrf_read_mesh, nrf_read_mesh_refinement and nrf_read_mesh_simplification AND the struct's pointers"""
    s = ctx.simplify_mesh(factor)
    v, t = ctx.read_mesh()
    e, none = ctx.read_mesh_refinement(brackets=False)
    src, vmap = ctx.read_mesh_simplification()
    nv, nt = int(s.n_vertices), int(s.n_triangles)
    assert (s.n_vertices_before, s.n_triangles_before) == before and s.factor == factor and s.reserved == 0 and none is None
    assert v.shape == (nv, 3) and t.shape == (nt, 3) and e.shape == (nv,) and src.shape == (nv,) and vmap.shape == (before[0],)
    assert np.array_equal(_bits(_peek(s.vertices, 3 * nv, np.float32)), _bits(v).reshape(-1))
    assert np.array_equal(_peek(s.triangles, 3 * nt, np.uint32), t.reshape(-1))
    assert np.array_equal(_peek(s.edges, nv, np.uint32), e) and np.array_equal(_peek(s.sources, nv, np.uint32), src)
    assert np.array_equal(_peek(s.vertex_map, before[0], np.uint32), vmap)
    if not nv:
        assert not s.vertices and not s.edges and not s.sources
    if not nt:
        assert not s.triangles
    return s, v, t, e, src, vmap


def _is_replay(got, want):
    s, v, t, e, src, vmap = got
    assert (s.n_vertices, s.n_triangles) == (len(want.sources), len(want.triangles))
    assert np.array_equal(src, want.sources) and np.array_equal(vmap, want.vertex_map) and np.array_equal(e, want.edges)
    assert np.array_equal(_bits(v), _bits(want.vertices)) and np.array_equal(t, want.triangles)


# ---------------------------------------------------------------- 1. the fields against the replay
@pytest.mark.parametrize("name", list(FIELDS))
def test_the_fields_are_the_replay(name):
    bare = nh.NerfHip(0)  # no model: none is needed
    f = field(name)
    w = words(name)
    before = (len(f.mesh.vertices), len(f.mesh.triangles))
    for factor, counts in zip(FACTORS[:4], COUNTS[name]):
        _, dev = _mesh_of(bare, name)
        got = _simplify(bare, factor, before)
        _is_replay(got, simplified(name, factor))
        s, v, t, e, src, vmap = got
        assert (s.n_vertices, s.n_triangles) == counts
        sr.check_all(v, t, e, src, vmap, f.mesh.vertices, w, f.dims, factor)
        if name in ("balls", "twins", "snake", "dots"):
            sr.check_balanced(t)
        print(f"{name} at factor {factor}: {before[0]} / {before[1]} -> {s.n_vertices} / {s.n_triangles}")
        if counts == (0, 0):  # nothing left: NRF_OK, and a following nrf_read_mesh returns empty arrays
            assert int(bare.lib.nrf_read_mesh(bare.h, None, None)) == nh.NRF_OK and np.all(vmap == sr.NONE)
            v2, t2 = bare.read_mesh()
            assert v2.shape == (0, 3) and t2.shape == (0, 3)
            again = _simplify(bare, factor, (0, 0))  # ... and the empty mesh simplifies to itself
            assert (again[0].n_vertices, again[0].n_triangles) == (0, 0) and not again[0].vertex_map
    bare.close()


# ---------------------------------------------------------------- 2. sizes
# One grid-stride pass of the launches here is 2048 workgroups x 256 lanes = 524 288 vertices or triangles.  noise_field's (60, 56, 50)
# = 168 000 points at iso 0.5 has 569 684 vertices and 1 192 836 triangles, both beyond one pass, on a third of the points of the
# (129, 65, 64) lattice of test_mesh_gpu.py (whose sparse noise at iso 0.97 has 621 728 vertices): half the points inside gives 3.4
# vertices a point.  (3, 5, 4): 126 vertices and 174 triangles, counts that end inside a workgroup.
SIZES = [((60, 56, 50), (569684, 1192836)), ((3, 5, 4), (126, 174))]


@pytest.mark.parametrize("dims,counts", SIZES)
def test_sizes_on_a_callers_noise_lattice(dims, counts):
    origin, cell, dims, iso, sigma = noise_field(dims, seed=dims[0], iso=0.5)
    ext = mr.mesh(origin, cell, dims, iso, sigma)
    w = rr.edge_words(ext, dims)
    assert (len(ext.vertices), len(ext.triangles)) == counts
    bare = nh.NerfHip(0)
    dev = _upload(sigma.reshape(-1))
    for factor in (2, 5):
        m, v0, t0 = _extract(bare, origin, cell, dims, float(iso), dev)
        assert np.array_equal(_bits(v0), _bits(ext.vertices)) and np.array_equal(t0, ext.triangles)
        got = _simplify(bare, factor, counts)
        want = sr.simplify(origin, cell, dims, factor, w, ext.vertices, ext.triangles)
        _is_replay(got, want)
        sr.check_all(got[1], got[2], got[3], got[4], got[5], ext.vertices, w, dims, factor)
        print(f"noise {dims} at factor {factor}: {counts[0]} / {counts[1]} -> {got[0].n_vertices} / {got[0].n_triangles}")
    bare.close()


# ---------------------------------------------------------------- 3. determinism
def test_twice_the_same_bytes():
    origin, cell, dims, iso, sigma = noise_field((33, 33, 33), iso=0.88)
    bare = nh.NerfHip(0)
    dev = _upload(sigma.reshape(-1))
    runs = []
    for _ in range(2):
        m, v0, t0 = _extract(bare, origin, cell, dims, float(iso), dev)
        got = _simplify(bare, 2, (int(m.n_vertices), int(m.n_triangles)))
        runs.append(b"".join(a.tobytes() for a in got[1:]))
    assert runs[0] == runs[1] and len(runs[0]) > 100000
    bare.close()


# ---------------------------------------------------------------- 4. with the blob model
def test_with_the_blob_model_the_other_stages_see_the_simplified_mesh():
    desc, keep, _ = _blob()
    ctx = _context(desc, 64, 64)
    h = _step(F(desc.bound))
    origin, cell, dims = _box_lattice((33, 33, 33), -0.75, 0.75)
    m, v0, t0 = _extract(ctx, origin, cell, dims, ISO)
    n0 = int(m.n_vertices)
    w0, _ = ctx.read_mesh_refinement(brackets=False)
    r, refined, e, b = _refine(ctx, 6, n0)
    assert refined.tobytes() != v0.tobytes()
    got = _simplify(ctx, 2, (n0, int(m.n_triangles)))
    s, v, t, edges, src, vmap = got
    # the keys are taken at the REFINED positions
    _is_replay(got, sr.simplify(origin, cell, dims, 2, w0, refined, t0))
    sr.check_all(v, t, edges, src, vmap, refined, w0, dims, 2)
    sr.check_balanced(t)  # the blob's surface is closed, and stays closed as a chain
    n = int(s.n_vertices)
    print(f"blob 33^3: {n0} / {len(t0)} -> {n} / {s.n_triangles} at factor 2")
    assert 0 < n < n0 // 3
    # the attributes of the result are the point call's on its vertices
    a, nrm, col = _mesh_attributes(ctx, h)
    pn, pc = torch.full((n, 4), 7.0, device="cuda"), torch.full((n, 4), 7.0, device="cuda")
    torch.cuda.synchronize()
    ctx.point_attributes(s.vertices, n, float(h), pn.data_ptr(), pc.data_ptr())
    assert a.n_vertices == n and np.array_equal(_bits(pn.cpu().numpy()), _bits(nrm)) and np.array_equal(_bits(pc.cpu().numpy()), _bits(col))
    assert np.any(nrm[:, :3] != 0)
    # a refinement after it depends on the carried edge words only: exactly the refined vertices of the unsimplified mesh at sources
    r2, v2, e2, b2 = _refine(ctx, 6, n)
    assert np.array_equal(_bits(v2), _bits(refined[src])) and np.array_equal(e2, w0[src]) and np.array_equal(_bits(b2), _bits(b[src]))
    assert r2.n_unbracketed == 0
    # a filter after it is the components replay on the simplified triangles
    fm, fv, ft = _filter(ctx, 0, LARGEST)
    parts = cr.parts(n, t)
    want = cr.filter_mesh(parts, n, t, 0, LARGEST)
    assert np.array_equal(_bits(fv), _bits(v2[want.old_vertex])) and np.array_equal(ft, want.triangles) and fm.n_triangles > 100
    assert np.array_equal(ctx.read_mesh_refinement(brackets=False)[0], w0[src][want.old_vertex])
    ctx.close()


# ---------------------------------------------------------------- 5. state and refusals
def test_state_and_refusals():
    import synthetic as syn
    ctx, desc = dp._ctx("hot", 64, 48)
    lib = ctx.lib
    ctx.render(syn.default_camera(64, 48), syn.orbit_pose(30, 30))
    frame = [a.copy() for a in ctx.read_f32()]
    st = bytes(ctx.stats())
    STATE, INV, OK = nh.NRF_E_STATE, nh.NRF_E_INVALID, nh.NRF_OK
    SENTINEL = bytes([0xAB]) * C.sizeof(nh.MeshSimplify)
    ROOM = 20000  # vertices the host array of reads() holds

    def simplify(context, factor=2, out=True):
        s = nh.MeshSimplify.from_buffer_copy(SENTINEL)
        rc = int(lib.nrf_simplify_mesh(context.h, C.c_uint32(factor), None, C.byref(s) if out else None))
        assert rc == OK or bytes(s) == SENTINEL  # a refused call writes nothing
        return rc

    def read(context):
        return int(lib.nrf_read_mesh_simplification(context.h, None, None))

    def reads(context):
        """the read calls of what a simplification invalidates: labelling, attributes, brackets"""
        one = np.zeros((ROOM, 4), np.float32)
        return (int(lib.nrf_read_mesh_components(context.h, None, None)), int(lib.nrf_read_mesh_attributes(context.h, None, None)),
                int(lib.nrf_read_mesh_refinement(context.h, None, one.ctypes.data_as(C.POINTER(C.c_float)))))

    # before any mesh
    bare = nh.NerfHip(0)
    assert simplify(bare) == STATE and read(bare) == STATE and simplify(ctx) == STATE and read(ctx) == STATE
    assert simplify(bare, out=False) == INV and simplify(bare, factor=0) == INV and simplify(bare, factor=257) == INV
    bare.close()
    s = nh.MeshSimplify.from_buffer_copy(SENTINEL)
    assert int(lib.nrf_simplify_mesh(None, C.c_uint32(2), None, C.byref(s))) == INV and bytes(s) == SENTINEL
    assert int(lib.nrf_read_mesh_simplification(None, None, None)) == INV
    # a mesh, not yet simplified; refused calls leave it untouched
    origin, cell, dims = _box_lattice((17, 16, 9), [-0.9, -0.8, -0.95], [0.85, 0.9, 0.7])
    iso = _off_fp16(np.median(_lattice_sigma(ctx, nh.Lattice.make(origin, cell, dims))))
    m, v0, t0 = _extract(ctx, origin, cell, dims, iso)
    before = (int(m.n_vertices), int(m.n_triangles))
    assert 100 < before[0] <= ROOM and read(ctx) == STATE
    for factor in (0, 257, 0xFFFFFFFF):
        assert simplify(ctx, factor=factor) == INV, factor
    assert simplify(ctx, out=False) == INV
    with pytest.raises(nh.NerfHipError) as e:
        ctx.simplify_mesh(0)
    assert e.value.code == INV
    with pytest.raises(nh.NerfHipError) as e:
        ctx.read_mesh_simplification()
    assert e.value.code == STATE
    v, t = ctx.read_mesh()
    assert v.tobytes() == v0.tobytes() and t.tobytes() == t0.tobytes() and read(ctx) == STATE
    # labelling, attributes and brackets of the mesh; the simplification invalidates the three
    ctx.mesh_components()
    ctx.mesh_attributes(float(_step(F(desc.bound))))
    ctx.refine_mesh(2)
    ctx.mesh_attributes(float(_step(F(desc.bound))))
    assert reads(ctx) == (OK, OK, OK)
    refined, _ = ctx.read_mesh()
    w0, _ = ctx.read_mesh_refinement(brackets=False)
    got = _simplify(ctx, 256, before)  # (the legal edge: one block holds the lattice, nothing is left)
    assert (got[0].n_vertices, got[0].n_triangles) == (0, 0) and reads(ctx) == (STATE, STATE, STATE) and read(ctx) == OK
    _extract(ctx, origin, cell, dims, iso)
    assert read(ctx) == STATE  # a new extraction invalidates the records
    ctx.mesh_components()
    ctx.refine_mesh(2)
    ctx.mesh_attributes(float(_step(F(desc.bound))))
    got = _simplify(ctx, 1, before)
    _is_replay(got, sr.simplify(origin, cell, dims, 1, w0, refined, t0))
    assert 0 < got[0].n_vertices < before[0] and reads(ctx) == (STATE, STATE, STATE) and read(ctx) == OK
    # asked again, they describe the SIMPLIFIED mesh; a second simplification works on it; a filter invalidates the records
    assert ctx.mesh_components().n_components == len(cr.parts(len(got[1]), got[2]).table)
    second = _simplify(ctx, 3, (int(got[0].n_vertices), int(got[0].n_triangles)))
    _is_replay(second, sr.simplify(origin, cell, dims, 3, got[3], got[1], got[2]))
    assert read(ctx) == OK
    ctx.filter_mesh(0)
    assert read(ctx) == STATE
    # statistics and the context's frame: untouched by refused and by served calls alike
    assert bytes(ctx.stats()) == st
    for a, b in zip(ctx.read_f32(), frame):
        assert np.array_equal(_bits(a), _bits(b))
    ctx.close()


# ---------------------------------------------------------------- 6. the C++ mirror
_PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nerf_render.h"
static uint64_t fnv(uint64_t hash, const void* p, size_t bytes) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < bytes; ++i) hash = (hash ^ b[i]) * 1099511628211ull;
  return hash;
}
int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const uint32_t n = (uint32_t)std::atoi(argv[2]);
  const float lo = (float)std::atof(argv[3]), iso = (float)std::atof(argv[4]);
  ngp::NerfRender render(std::vector<int>{0});
  render.reload_network_from_file(argv[1]);
  const float origin[3] = {lo, lo, lo}, step = (float)((double)-2.0 * lo / (n - 1)), cell[3] = {step, step, step};
  const uint32_t dims[3] = {n, n, n};
  const ngp::NerfRender::Mesh before = render.extract_mesh(origin, cell, dims, iso);
  render.refine_mesh((uint32_t)std::atoi(argv[5]));
  const ngp::NerfRender::SimplifiedMesh mesh = render.simplify_mesh((uint32_t)std::atoi(argv[6]));
  uint64_t hash = fnv(1469598103934665603ull, mesh.vertices.data(), mesh.vertices.size() * sizeof(float));
  hash = fnv(hash, mesh.triangles.data(), mesh.triangles.size() * sizeof(uint32_t));
  hash = fnv(hash, mesh.sources.data(), mesh.sources.size() * sizeof(uint32_t));
  hash = fnv(hash, mesh.vertex_map.data(), mesh.vertex_map.size() * sizeof(uint32_t));
  std::printf("simplified %zu %zu %zu %zu %016llx\n", mesh.vertices.size() / 3, mesh.triangles.size() / 3, mesh.sources.size(), mesh.vertex_map.size(),
              (unsigned long long)hash);
  if (mesh.vertex_map.size() != before.vertices.size() / 3) return 4;
  return mesh.vertices_dev || mesh.vertices.empty() ? 0 : 3;
}
"""


def test_the_cpp_mirror_returns_the_python_calls_bytes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None or not (HOSTDIR / "libngp_hip.so").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, snap = _snapshot(tmp_path)
    n = 17
    origin, cell, dims = _box_lattice((n, n, n), -0.75, 0.75)
    ctx = _context(desc, 64, 64)
    m, v0, t0 = _extract(ctx, origin, cell, dims, ISO)
    ctx.refine_mesh(6)
    s, v, t, e, src, vmap = _simplify(ctx, 2, (int(m.n_vertices), int(m.n_triangles)))
    ctx.close()
    assert s.n_triangles > 10
    exe_src, exe = tmp_path / "simplify.cpp", tmp_path / "simplify"
    exe_src.write_text(_PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(HOSTDIR), "-I", str(ROOT / "include"), "-o", str(exe), str(exe_src), f"-L{HOSTDIR}", "-lngp_hip",
                    f"-L{HOSTDIR.parent}", "-lnerfhip", f"-Wl,-rpath,{HOSTDIR}", f"-Wl,-rpath,{HOSTDIR.parent}"], check=True)
    r = subprocess.run([str(exe), str(snap), str(n), "-0.75", repr(ISO), "6", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("simplified ")][-1].split()
    assert [int(x) for x in line[1:5]] == [s.n_vertices, s.n_triangles, s.n_vertices, m.n_vertices], line
    assert int(line[5], 16) == _fnv1a(v.tobytes() + t.tobytes() + src.tobytes() + vmap.tobytes()), line


# ---------------------------------------------------------------- 7. testbed --save_mesh out.ply --mesh_largest --mesh_refine 6 --mesh_simplify 2
def test_testbed_saves_the_simplified_mesh(tmp_path):
    if not (HOSTDIR / "testbed").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, snap = _snapshot(tmp_path)
    n, b = 33, F(desc.bound)
    # testbed's lattice: n^3 points over the model's aabb, the step formed in fp32
    origin, cell, dims = [float(-b)] * 3, [float(F(F(2.0) * b) / F(n - 1))] * 3, (n, n, n)
    ctx = _context(desc, 64, 64)
    m, v0, t0 = _extract(ctx, origin, cell, dims, ISO)
    f = ctx.filter_mesh(0, keep_largest=True)
    ctx.refine_mesh(6)
    s, v, t, e, src, vmap = _simplify(ctx, 2, (int(f.n_vertices), int(f.n_triangles)))
    ctx.close()
    assert s.n_triangles > 10
    out = tmp_path / "out.ply"
    r = subprocess.run([str(HOSTDIR / "testbed"), str(snap), "64", "64", str(tmp_path) + "/", "--save_mesh", str(out), "--mesh_largest",
                        "--mesh_refine", "6", "--mesh_simplify", "2", "--mesh_res", str(n), "--mesh_iso", repr(ISO)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("mesh simplify: ")]
    assert len(line) == 1, r.stdout
    print(line[0])
    got = re.fullmatch(r"mesh simplify: factor (\d+), vertices (\d+) -> (\d+), triangles (\d+) -> (\d+), [0-9.]+ s", line[0])
    assert got and [int(g) for g in got.groups()] == [2, f.n_vertices, s.n_vertices, f.n_triangles, s.n_triangles], line[0]
    pv, pn, prgb, pt = pac.parse_ply(out.read_bytes())
    assert np.array_equal(_bits(pv), _bits(v)) and np.array_equal(pt, t.astype(np.int32)) and len(pn) == s.n_vertices
