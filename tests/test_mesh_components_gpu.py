"""nrf_mesh_components, nrf_read_mesh_components and nrf_filter_mesh on the GPU.

The definition (include/nerfhip.h, csrc/nrf_meshcc_plan.h) is held index for index and bit for bit to tests/meshcc_replay.py, the
numpy replay -- plain min-label propagation, a different algorithm from the kernels' -- that tests/test_mesh_components_cpu.py holds to
the plan header; what a labelling has to be whatever the code says is checked by meshcc_replay.check_parts, which shares no code with
either.  The fields are test_mesh_components_cpu's: caller-supplied sigma lattices, so no model is needed except where one is the
point.  Nothing here rests on a tolerance.  Every test here needs the entry points: none passes without them."""
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
import test_density_points_gpu as dp
import test_point_attributes_cpu as pac
from test_mesh_components_cpu import FIELDS, field
from test_mesh_gpu import ISO, _blob, _box_lattice, _extract, _peek
from test_point_attributes_gpu import _mesh_attributes, _step
from test_ray_hits_gpu import _fnv1a
from test_render_rays_clip_gpu import _bits, _context, _upload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
HOSTDIR = ROOT / "nerf-cuda_amd" / "host"
F = np.float32
LARGEST = cr.KEEP_LARGEST


def _mesh_of(ctx, name):
    """the field's mesh becomes the context's: (field, the device lattice -- kept alive by the caller)"""
    f = field(name)
    dev = _upload(f.sigma.reshape(-1))
    m, v, t = _extract(ctx, f.origin, f.cell, f.dims, float(f.iso), dev)
    assert np.array_equal(_bits(v), _bits(f.mesh.vertices)) and np.array_equal(t, f.mesh.triangles)
    return f, dev


def _components(ctx, n_vertices):
    """(struct, labels, table) of one nrf_mesh_components call; the arrays through nrf_read_mesh_components AND the struct's pointers"""
    p = ctx.mesh_components()
    lab, table = ctx.read_mesh_components()
    nc = int(p.n_components)
    assert lab.shape == (n_vertices,) and table.shape == (nc, 3) and p.reserved == 0
    assert np.array_equal(_peek(p.labels, n_vertices, np.uint32), lab) and np.array_equal(_peek(p.components, 3 * nc, np.uint32), table.reshape(-1))
    return p, lab, table


def _filter(ctx, min_triangles, flags):
    """(struct, vertices, triangles) of one nrf_filter_mesh call; the arrays through nrf_read_mesh AND the struct's pointers"""
    m = ctx.filter_mesh(min_triangles, bool(flags & LARGEST))
    v, t = ctx.read_mesh()
    assert v.shape == (m.n_vertices, 3) and t.shape == (m.n_triangles, 3)
    assert np.array_equal(_bits(_peek(m.vertices, 3 * m.n_vertices, np.float32)), _bits(v).reshape(-1))
    assert np.array_equal(_peek(m.triangles, 3 * m.n_triangles, np.uint32), t.reshape(-1))
    return m, v, t


def _is_replay(v, t, vertices, triangles, parts, min_triangles, flags):
    """v, t are the replay's filter of (vertices, triangles): vertex bits and indices identical"""
    want = cr.filter_mesh(parts, len(vertices), triangles, min_triangles, flags)
    assert v.shape == (len(want.old_vertex), 3) and t.shape == want.triangles.shape, (v.shape, t.shape, len(want.old_vertex), want.triangles.shape)
    assert np.array_equal(_bits(v), _bits(vertices[want.old_vertex])) and np.array_equal(t, want.triangles)
    return want


# ---------------------------------------------------------------- 1. labels, table, n_components
@pytest.mark.parametrize("name", list(FIELDS))
def test_labels_and_table_are_the_replay(name):
    bare = nh.NerfHip(0)  # no model: none is needed
    f, dev = _mesh_of(bare, name)
    nv = len(f.mesh.vertices)
    p, lab, table = _components(bare, nv)
    assert np.array_equal(lab, f.parts.labels) and np.array_equal(table, f.parts.table) and p.n_components == len(f.parts.table)
    cr.check_parts(lab, table, nv, f.mesh.triangles)
    print(f"{name}: {nv} vertices, {len(f.mesh.triangles)} triangles, {p.n_components} components, n_rounds {p.n_rounds}")
    assert p.n_rounds >= 2
    p2, lab2, table2 = _components(bare, nv)
    assert lab2.tobytes() == lab.tobytes() and table2.tobytes() == table.tobytes() and p2.n_components == p.n_components
    # the mesh itself is read, never written
    v, t = bare.read_mesh()
    assert np.array_equal(_bits(v), _bits(f.mesh.vertices)) and np.array_equal(t, f.mesh.triangles)
    bare.close()


# ---------------------------------------------------------------- 2. filter on the balls
@pytest.mark.parametrize("name,min_triangles,flags,counts,labels", [
    ("balls", 25, 0, (3072, 6128), [0, 440, 1858, 1866]),   # drops only the dot
    ("balls", 649, 0, (2746, 5480), [0, 1858, 1866]),
    ("balls", 0, LARGEST, (1518, 3032), [0]),
    ("twins", 0, LARGEST, (614, 1224), None),               # the two equal balls tie: the lower label wins
])
def test_filter_on_the_balls(name, min_triangles, flags, counts, labels):
    bare = nh.NerfHip(0)
    f, dev = _mesh_of(bare, name)
    if labels is None:
        twins = [int(r[0]) for r in f.parts.table if int(r[2]) == 1224]
        assert len(twins) == 2
        labels = [min(twins)]
    m, v, t = _filter(bare, min_triangles, flags)  # (labels the mesh itself: no nrf_mesh_components before it)
    assert (m.n_vertices, m.n_triangles) == counts
    want = _is_replay(v, t, f.mesh.vertices, f.mesh.triangles, f.parts, min_triangles, flags)
    assert want.kept_labels == labels
    assert m.sigma == dev.data_ptr()  # out->sigma is the extraction's
    mr.check_closed_and_oriented(t)  # a filtered closed mesh is closed
    mr.check_indices(t, len(v))      # ... and every vertex is referenced
    bare.close()


# ---------------------------------------------------------------- 3. filter on sparse noise and dots
@pytest.mark.parametrize("name", ["noise33", "dots"])
def test_filter_on_noise_and_dots(name):
    bare = nh.NerfHip(0)
    f = field(name)
    sizes = f.parts.table[:, 2].astype(np.int64)
    inside = int(np.median(sizes)) + 1 if name == "noise33" else 24  # (dots: every component has 24, so 24 keeps all of the thousand)
    dev = _upload(f.sigma.reshape(-1))
    nv, nt = len(f.mesh.vertices), len(f.mesh.triangles)
    for min_triangles, flags in [(inside, 0), (inside, LARGEST), (0, LARGEST)]:
        _extract(bare, f.origin, f.cell, f.dims, float(f.iso), dev)
        m, v, t = _filter(bare, min_triangles, flags)
        want = _is_replay(v, t, f.mesh.vertices, f.mesh.triangles, f.parts, min_triangles, flags)
        mr.check_indices(t, len(v))
        print(f"{name}: min_triangles {min_triangles}, flags {flags}: {len(want.kept_labels)} of {len(sizes)} components, {m.n_vertices} vertices, {m.n_triangles} triangles")
        if flags:
            assert len(want.kept_labels) == 1 and (name != "dots" or want.kept_labels == [0])
        elif name == "noise33":
            assert 0 < m.n_triangles < nt and 0 < len(want.kept_labels) < len(sizes)
    # keep-all is bit-identical to the unfiltered mesh, also through the labelling of an explicit call
    _extract(bare, f.origin, f.cell, f.dims, float(f.iso), dev)
    bare.mesh_components()
    m, v, t = _filter(bare, 0, 0)
    assert (m.n_vertices, m.n_triangles) == (nv, nt)
    assert v.tobytes() == f.mesh.vertices.tobytes() and t.tobytes() == f.mesh.triangles.tobytes()
    # keep-none: zero counts, NRF_OK, and a following nrf_read_mesh returns empty arrays
    for min_triangles, flags in [(10 ** 9, 0), (int(sizes.max()) + 1, LARGEST)]:
        _extract(bare, f.origin, f.cell, f.dims, float(f.iso), dev)
        m, v, t = _filter(bare, min_triangles, flags)
        assert (m.n_vertices, m.n_triangles) == (0, 0) and not m.vertices and not m.triangles and v.shape == (0, 3) and t.shape == (0, 3)
        assert int(bare.lib.nrf_read_mesh(bare.h, None, None)) == nh.NRF_OK
        # ... and the empty mesh has no components, and filters to itself
        p, lab, table = _components(bare, 0)
        assert p.n_components == 0 and p.n_rounds == 0 and not p.labels and not p.components
        m, v, t = _filter(bare, 0, 0)
        assert (m.n_vertices, m.n_triangles) == (0, 0)
    bare.close()


# ---------------------------------------------------------------- 4. state and refusals
def test_state_and_refusals():
    import synthetic as syn
    ctx, desc = dp._ctx("hot", 64, 48)
    lib = ctx.lib
    ctx.render(syn.default_camera(64, 48), syn.orbit_pose(30, 30))
    frame = [a.copy() for a in ctx.read_f32()]
    st = bytes(ctx.stats())
    STATE, INV, OK = nh.NRF_E_STATE, nh.NRF_E_INVALID, nh.NRF_OK

    def components(context, out=True):
        p = nh.MeshParts.from_buffer_copy(bytes([0xAB]) * C.sizeof(nh.MeshParts))
        rc = int(lib.nrf_mesh_components(context.h, None, C.byref(p) if out else None))
        assert rc == OK or bytes(p) == bytes([0xAB]) * C.sizeof(nh.MeshParts)  # a refused call writes nothing
        return rc

    def filt(context, min_triangles=0, flags=0, out=True):
        m = nh.Mesh.from_buffer_copy(bytes([0xAB]) * C.sizeof(nh.Mesh))
        rc = int(lib.nrf_filter_mesh(context.h, min_triangles, flags, None, C.byref(m) if out else None))
        assert rc == OK or bytes(m) == bytes([0xAB]) * C.sizeof(nh.Mesh)
        return rc

    def read(context):
        return int(lib.nrf_read_mesh_components(context.h, None, None))

    # before any mesh
    bare = nh.NerfHip(0)
    assert components(bare) == STATE and filt(bare) == STATE and read(bare) == STATE and components(ctx) == STATE and filt(ctx) == STATE
    assert components(bare, out=False) == INV and filt(bare, out=False) == INV and filt(bare, flags=2) == INV
    bare.close()
    # a mesh, not yet labelled; refused calls leave it untouched
    f, dev = _mesh_of(ctx, "balls")
    nv = len(f.mesh.vertices)
    assert read(ctx) == STATE
    for flags in (2, 3, 0x80000000, 0xfffffffe):
        assert filt(ctx, flags=flags) == INV, flags
    assert filt(ctx, out=False) == INV and components(ctx, out=False) == INV
    with pytest.raises(nh.NerfHipError) as e:
        ctx.read_mesh_components()
    assert e.value.code == STATE
    v, t = ctx.read_mesh()
    assert np.array_equal(_bits(v), _bits(f.mesh.vertices)) and np.array_equal(t, f.mesh.triangles)
    assert components(ctx) == OK and read(ctx) == OK
    # nrf_filter_mesh invalidates the labelling; asked again, it describes the FILTERED mesh
    m, v, t = _filter(ctx, 649, 0)
    assert read(ctx) == STATE
    p, lab, table = _components(ctx, int(m.n_vertices))
    again = cr.parts(len(v), t)
    assert np.array_equal(lab, again.labels) and np.array_equal(table, again.table) and table[:, 2].tolist() == [3032, 1224, 1224]
    cr.check_parts(lab, table, len(v), t)
    # ... and a second filter works on the filtered mesh, with the labelling just made
    m2, v2, t2 = _filter(ctx, 0, LARGEST)
    _is_replay(v2, t2, v, t, again, 0, LARGEST)
    assert (m2.n_vertices, m2.n_triangles) == (1518, 3032)
    # a new nrf_extract_mesh invalidates too
    assert components(ctx) == OK and read(ctx) == OK
    _mesh_of(ctx, "balls")
    assert read(ctx) == STATE and components(ctx) == OK and read(ctx) == OK
    assert ctx.mesh_components().n_components == 5
    # statistics and the context's frame: untouched by refused and by served calls alike
    assert bytes(ctx.stats()) == st
    for a, b in zip(ctx.read_f32(), frame):
        assert np.array_equal(_bits(a), _bits(b))
    ctx.close()


# ---------------------------------------------------------------- 5. with a model: filter, then attributes
def test_attributes_after_the_filter_are_those_of_the_filtered_vertices():
    desc, keep, _ = _blob()
    ctx = _context(desc, 64, 64)
    h = _step(F(desc.bound))
    origin, cell, dims = _box_lattice((17, 16, 9), -0.75, 0.75)
    m, v, t = _extract(ctx, origin, cell, dims, ISO)
    base = cr.parts(len(v), t)
    ctx.mesh_attributes(float(h))
    assert int(ctx.lib.nrf_read_mesh_attributes(ctx.h, None, None)) == nh.NRF_OK
    fm, fv, ft = _filter(ctx, 0, LARGEST)
    want = _is_replay(fv, ft, v, t, base, 0, LARGEST)
    print(f"blob 17x16x9: {len(base.table)} components {base.table[:, 2].tolist()}, the largest has {fm.n_vertices} vertices, {fm.n_triangles} triangles")
    assert fm.n_vertices == len(want.old_vertex) > 0
    # the attributes of the mesh it replaced are invalid ...
    assert int(ctx.lib.nrf_read_mesh_attributes(ctx.h, None, None)) == nh.NRF_E_STATE
    # ... and the new ones are those of the filtered vertices
    a, nrm, col = _mesh_attributes(ctx, h)
    n = int(fm.n_vertices)
    assert a.n_vertices == n
    pn, pc = torch.full((n, 4), 7.0, device="cuda"), torch.full((n, 4), 7.0, device="cuda")
    torch.cuda.synchronize()
    ctx.point_attributes(fm.vertices, n, float(h), pn.data_ptr(), pc.data_ptr())
    assert np.array_equal(_bits(pn.cpu().numpy()), _bits(nrm)) and np.array_equal(_bits(pc.cpu().numpy()), _bits(col))
    assert np.any(nrm[:, :3] != 0)
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
  if (argc != 6) return 2;
  const uint32_t n = (uint32_t)std::atoi(argv[2]);
  const float lo = (float)std::atof(argv[3]), iso = (float)std::atof(argv[4]);
  ngp::NerfRender render(std::vector<int>{0});
  render.reload_network_from_file(argv[1]);
  const float origin[3] = {lo, lo, lo}, step = (float)((double)-2.0 * lo / (n - 1)), cell[3] = {step, step, step};
  const uint32_t dims[3] = {n, n, n};
  render.extract_mesh(origin, cell, dims, iso);
  const ngp::NerfRender::MeshComponents parts = render.mesh_components();
  uint64_t hash = fnv(1469598103934665603ull, parts.labels.data(), parts.labels.size() * sizeof(uint32_t));
  hash = fnv(hash, parts.table.data(), parts.table.size() * sizeof(uint32_t));
  std::printf("parts %zu %zu %016llx\n", parts.labels.size(), parts.table.size() / 3, (unsigned long long)hash);
  const ngp::NerfRender::Mesh mesh = render.filter_mesh((uint64_t)std::atoll(argv[5]), true);
  hash = fnv(1469598103934665603ull, mesh.vertices.data(), mesh.vertices.size() * sizeof(float));
  hash = fnv(hash, mesh.triangles.data(), mesh.triangles.size() * sizeof(uint32_t));
  std::printf("mesh %zu %zu %016llx\n", mesh.vertices.size() / 3, mesh.triangles.size() / 3, (unsigned long long)hash);
  return mesh.vertices_dev || mesh.vertices.empty() ? 0 : 3;
}
"""


def _snapshot(tmp_path):
    import synthetic as syn
    desc, keep, cfg = _blob()
    snap = tmp_path / "blob.msgpack"
    syn.write_snapshot(snap, cfg, keep[0], keep[1])
    return desc, snap


def test_the_cpp_mirror_returns_the_python_calls_bytes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None or not (HOSTDIR / "libngp_hip.so").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, snap = _snapshot(tmp_path)
    n = 17
    origin, cell, dims = _box_lattice((n, n, n), -0.75, 0.75)
    ctx = _context(desc, 64, 64)
    m, v, t = _extract(ctx, origin, cell, dims, ISO)
    p, lab, table = _components(ctx, int(m.n_vertices))
    fm, fv, ft = _filter(ctx, 1, LARGEST)
    ctx.close()
    assert fm.n_triangles > 100
    src, exe = tmp_path / "meshcc.cpp", tmp_path / "meshcc"
    src.write_text(_PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(HOSTDIR), "-I", str(ROOT / "include"), "-o", str(exe), str(src), f"-L{HOSTDIR}", "-lngp_hip",
                    f"-L{HOSTDIR.parent}", "-lnerfhip", f"-Wl,-rpath,{HOSTDIR}", f"-Wl,-rpath,{HOSTDIR.parent}"], check=True)
    r = subprocess.run([str(exe), str(snap), str(n), "-0.75", repr(ISO), "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("parts ")][-1].split()
    assert (int(line[1]), int(line[2])) == (m.n_vertices, p.n_components) and int(line[3], 16) == _fnv1a(lab.tobytes() + table.tobytes()), line
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("mesh ")][-1].split()
    assert (int(line[1]), int(line[2])) == (fm.n_vertices, fm.n_triangles) and int(line[3], 16) == _fnv1a(fv.tobytes() + ft.tobytes()), line


# ---------------------------------------------------------------- 7. testbed --save_mesh out.ply --mesh_largest
def test_testbed_saves_the_filtered_mesh(tmp_path):
    if not (HOSTDIR / "testbed").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, snap = _snapshot(tmp_path)
    n, b = 33, F(desc.bound)
    # testbed's lattice: n^3 points over the model's aabb, the step formed in fp32
    origin, cell, dims = [float(-b)] * 3, [float(F(F(2.0) * b) / F(n - 1))] * 3, (n, n, n)
    ctx = _context(desc, 64, 64)
    m, v, t = _extract(ctx, origin, cell, dims, ISO)
    p, lab, table = _components(ctx, int(m.n_vertices))
    fm, fv, ft = _filter(ctx, 0, LARGEST)
    ctx.close()
    assert fm.n_triangles > 100
    out = tmp_path / "out.ply"
    r = subprocess.run([str(HOSTDIR / "testbed"), str(snap), "64", "64", str(tmp_path) + "/", "--save_mesh", str(out), "--mesh_largest",
                        "--mesh_res", str(n), "--mesh_iso", repr(ISO)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("mesh filter: ")]
    assert len(line) == 1, r.stdout
    print(line[0])
    got = re.fullmatch(r"mesh filter: (\d+) components, (\d+) kept, vertices (\d+) -> (\d+), triangles (\d+) -> (\d+), [0-9.]+ s", line[0])
    assert got and [int(g) for g in got.groups()] == [p.n_components, 1, m.n_vertices, fm.n_vertices, m.n_triangles, fm.n_triangles], line[0]
    pv, pn, prgb, pt = pac.parse_ply(out.read_bytes())
    assert np.array_equal(_bits(pv), _bits(fv)) and np.array_equal(pt, ft.astype(np.int32)) and len(pn) == fm.n_vertices
