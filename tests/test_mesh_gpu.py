"""nrf_density_lattice, nrf_extract_mesh and nrf_read_mesh on the GPU.

The definition (include/nerfhip.h, csrc/nrf_mesh_plan.h) is held bit for bit and index for index to tests/mesh_replay.py, the numpy
replay that tests/test_mesh_cpu.py holds to the header; the lattice's sigmas are held to nrf_density on the replayed positions.  What
a mesh has to be whatever the code says -- closed, oriented, every vertex on its edge, a volume between the full cells' and the full
plus the mixed cells' -- is checked by mesh_replay's property checkers, which share no code with the polygoniser.
Stages: hot (bound 1, and bound 4 with three cascades), wide, generic, as in test_density_points_gpu.py; the model with a surface is
points_replay.blob_model().  Every test here needs the entry points: none passes without them."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_replay as mr
import nerfhip as nh
import points_replay as pr
import test_density_points_gpu as dp
from test_mesh_cpu import noise_field
from test_ray_hits_gpu import _fnv1a
from test_render_rays_clip_gpu import _bits, _context, _upload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
ISO = 30.3  # not an fp16 value: no sigma of the model equals it
BLOB_LATTICES = {"33^3": (33, 33, 33), "17x16x9": (17, 16, 9)}


@functools.lru_cache(maxsize=None)
def _hip():
    """the HIP runtime this process has already loaded (libnerfhip.so and torch share it), for reads at raw device pointers"""
    nh.load_library()
    path = next(ln.split()[-1] for ln in Path("/proc/self/maps").read_text().splitlines() if "libamdhip64" in ln)
    lib = C.CDLL(path)
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.hipMemcpy.restype = C.c_int
    return lib


def _peek(ptr, count, dtype):
    """host copy of `count` elements at a raw device pointer"""
    out = np.empty(count, dtype)
    if count:
        assert ptr
        assert _hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) == 0
    return out


def _lattice_sigma(ctx, lat):
    s = torch.full((lat.n_points,), 7.0, device="cuda")
    torch.cuda.synchronize()
    ctx.density_lattice(lat, s.data_ptr())
    return s.cpu().numpy()


def _box_lattice(dims, lo, hi):
    """the lattice of `dims` points over [lo, hi] per axis"""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), 3), np.broadcast_to(np.asarray(hi, np.float64), 3)
    cell = [float(F((hi[c] - lo[c]) / (dims[c] - 1))) for c in range(3)]
    return [float(F(v)) for v in lo], cell, tuple(dims)


def _extract(ctx, origin, cell, dims, iso, sigma=None):
    """(Mesh struct, vertices, triangles) of one nrf_extract_mesh call; the arrays through nrf_read_mesh AND the struct's pointers"""
    lat = nh.Lattice.make(origin, cell, dims)
    m = ctx.extract_mesh(lat, iso, 0 if sigma is None else sigma.data_ptr())
    v, t = ctx.read_mesh()
    assert v.shape == (m.n_vertices, 3) and t.shape == (m.n_triangles, 3)
    assert np.array_equal(_bits(_peek(m.vertices, 3 * m.n_vertices, np.float32)), _bits(v).reshape(-1))
    assert np.array_equal(_peek(m.triangles, 3 * m.n_triangles, np.uint32), t.reshape(-1))
    return m, v, t


def _is_replay(v, t, origin, cell, dims, iso, sigma):
    want = mr.mesh(origin, cell, dims, iso, sigma)
    assert v.shape == want.vertices.shape and t.shape == want.triangles.shape, (v.shape, want.vertices.shape, t.shape, want.triangles.shape)
    assert np.array_equal(_bits(v), _bits(want.vertices)) and np.array_equal(t, want.triangles)
    return want


@functools.lru_cache(maxsize=None)
def _blob():
    return pr.blob_model()


# ---------------------------------------------------------------- 1. lattice sigma
@pytest.mark.parametrize("stage", list(dp.STAGES))
def test_lattice_sigma_is_nrf_density_on_the_replayed_positions(stage):
    ctx, desc = dp._ctx(stage)
    b = float(desc.bound)
    for dims in [(2, 2, 2), (3, 5, 4), (17, 16, 9), (33, 33, 33)]:
        origin, cell, dims = _box_lattice(dims, [-0.9 * b, -0.8 * b, -0.95 * b], [0.85 * b, 0.9 * b, 0.7 * b])  # cells differ by axis
        assert len(set(cell)) == 3
        x = mr.positions(origin, cell, dims).reshape(-1, 3)
        got, want = _lattice_sigma(ctx, nh.Lattice.make(origin, cell, dims)), dp._density(ctx, x)
        print(f"{stage} {dims}: sigma {want.min():.3g} .. {want.max():.3g}")
        assert np.all(want > 0) and np.array_equal(_bits(got), _bits(want)), (stage, dims)
    # a lattice that sticks out of the box: zeros there, the others as nrf_density has them
    origin, cell, dims = _box_lattice((9, 7, 5), [-1.5 * b, -0.5 * b, -0.5 * b], [1.5 * b, b, 0.5 * b])
    x = mr.positions(origin, cell, dims).reshape(-1, 3)
    inside = pr.guard(x, 0.0, b, 1)
    assert 0 < inside.sum() < len(x) and inside.reshape(dims)[:, -1].any()  # (y reaches the face itself: evaluated)
    got = _lattice_sigma(ctx, nh.Lattice.make(origin, cell, dims))
    assert np.all(_bits(got[~inside]) == 0) and np.all(got[inside] > 0)
    assert np.array_equal(_bits(got), _bits(dp._density(ctx, x)))
    assert np.array_equal(_bits(got[inside]), _bits(dp._density(ctx, x[inside])))
    ctx.close()


# ---------------------------------------------------------------- 2. mesh from the model
@pytest.mark.parametrize("name", list(BLOB_LATTICES))
def test_the_blob_is_the_replay_of_its_sigmas_and_a_closed_surface(name):
    """The blob at iso 30.3 on [-0.75, 0.75]^3.  The CPU oracle (oracle_py.Oracle.network on the replayed 33^3 lattice) has 1069
    points inside, none of them on the lattice's boundary and none equal to iso, and its replayed mesh has 2318 vertices and 4632
    triangles (17 x 16 x 9: 62 points inside, 350 vertices, 696 triangles): the floor of 1000 triangles at 33^3 stands."""
    desc, keep, _ = _blob()
    ctx = _context(desc, 64, 64)
    origin, cell, dims = _box_lattice(BLOB_LATTICES[name], -0.75, 0.75)
    lat = nh.Lattice.make(origin, cell, dims)
    m, v, t = _extract(ctx, origin, cell, dims, ISO)
    sigma = _peek(m.sigma, lat.n_points, np.float32)
    assert np.array_equal(_bits(sigma), _bits(_lattice_sigma(ctx, lat)))
    want = _is_replay(v, t, origin, cell, dims, ISO, sigma)
    ins = want.inside
    assert ins.any() and not (ins[0].any() or ins[-1].any() or ins[:, 0].any() or ins[:, -1].any() or ins[:, :, 0].any() or ins[:, :, -1].any())
    V = mr.check_all(mr.Mesh(v, t, want.edge_p, want.edge_q, ins), origin, cell, dims)
    print(f"blob {name}: {ins.sum()} points inside, {m.n_vertices} vertices, {m.n_triangles} triangles, volume {V:.5f}")
    assert V > 0
    if name == "33^3":
        assert m.n_triangles >= 1000
    m2, v2, t2 = _extract(ctx, origin, cell, dims, ISO)
    assert (m2.n_vertices, m2.n_triangles) == (m.n_vertices, m.n_triangles)
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()
    ctx.close()


# ---------------------------------------------------------------- 3. mesh from a caller's lattice
# (65, 64, 33) -- 137 280 points -- exceeds a scan tile (2048 points) but not one grid-stride pass of the count and emit launches
# (2048 workgroups x 256 lanes = 524 288 points): the next size up, (129, 65, 64) = 536 640 points, does.  Its noise has 3 % of the
# points inside instead of half, which keeps the replay of its surface short.
NOISE = [((2, 2, 2), 0.5), ((3, 5, 4), 0.5), ((33, 33, 33), 0.5), ((129, 65, 64), 0.97)]


@pytest.mark.parametrize("dims,iso", NOISE)
def test_a_callers_noise_lattice_is_the_replay_and_a_closed_surface(dims, iso):
    origin, cell, dims, iso, sigma = noise_field(dims, seed=dims[0], iso=iso, zero_boundary=True)
    if min(dims) >= 33:  # (in the small ones the zeroed boundary layer leaves a handful of points)
        assert np.isnan(sigma).any() and np.isposinf(sigma).any() and np.isneginf(sigma).any() and (sigma == iso).any()
    bare = nh.NerfHip(0)  # no model: none is needed
    dev = _upload(sigma.reshape(-1))
    m, v, t = _extract(bare, origin, cell, dims, iso, dev)
    assert m.sigma == dev.data_ptr()
    want = _is_replay(v, t, origin, cell, dims, iso, sigma)
    V = mr.check_all(mr.Mesh(v, t, want.edge_p, want.edge_q, want.inside), origin, cell, dims)
    print(f"noise {dims}: {m.n_vertices} vertices, {m.n_triangles} triangles, volume {V:.5f}")
    assert (m.n_triangles > 0 and V > 0) if min(dims) > 2 else m.n_triangles == 0
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(sigma.reshape(-1)))  # the caller's lattice is read, never written
    bare.close()


def test_all_outside_and_all_inside_are_empty():
    bare = nh.NerfHip(0)
    origin, cell, dims = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], (5, 4, 3)
    for value in (0.0, 1.0, np.nan, np.inf):
        dev = _upload(np.full(60, value, np.float32))
        m, v, t = _extract(bare, origin, cell, dims, 0.5, dev)
        assert (m.n_vertices, m.n_triangles) == (0, 0) and len(v) == 0 and len(t) == 0, value
    # ... and a mesh after an empty one
    s = np.zeros(dims, np.float32)
    s[2, 2, 1] = 1.0
    m, v, t = _extract(bare, origin, cell, dims, 0.5, _upload(s.reshape(-1)))
    _is_replay(v, t, origin, cell, dims, 0.5, s)
    assert m.n_vertices == 14 and m.n_triangles == 24  # one point inside: its 14 edges, the 24 tetrahedra around it
    bare.close()


# ---------------------------------------------------------------- 4. normals
def test_density_gradient_takes_the_vertices_as_they_are():
    desc, keep, _ = _blob()
    ctx = _context(desc, 64, 64)
    origin, cell, dims = _box_lattice(BLOB_LATTICES["33^3"], -0.75, 0.75)
    m, v, t = _extract(ctx, origin, cell, dims, ISO)
    n = int(m.n_vertices)
    h = float(F(desc.bound) * F(2.0 ** -7))
    direct = torch.full((n, 4), 7.0, device="cuda")
    torch.cuda.synchronize()
    ctx.density_gradient(m.vertices, n, h, direct.data_ptr())
    direct = direct.cpu().numpy()
    again = dp._gradient(ctx, v, h)
    assert np.array_equal(_bits(direct), _bits(again))
    assert np.any(direct[:, :3] != 0)
    g = direct[:, :3].astype(np.float64)
    print(f"blob: {n} vertices, outward normals (dot(-g, v) > 0) on {np.mean(np.sum(-g * v.astype(np.float64), axis=1) > 0):.4f}, "
          f"|g| > 0 on {np.mean(np.sum(g * g, axis=1) > 0):.4f}")
    ctx.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals():
    import synthetic as syn
    ctx, desc = dp._ctx("hot", 64, 48)
    lib = ctx.lib
    ctx.render(syn.default_camera(64, 48), syn.orbit_pose(30, 30))
    frame = [a.copy() for a in ctx.read_f32()]
    st = bytes(ctx.stats())
    good = dict(origin=[-0.5, -0.5, -0.5], cell=[0.25, 0.25, 0.25], dims=(5, 5, 5))
    sig = torch.full((125,), 7.0, device="cuda")
    torch.cuda.synchronize()
    SENTINEL = bytes([0xAB]) * C.sizeof(nh.Mesh)

    def extract(lat, iso=1.0, sigma=0, out=True, context=ctx):
        m = nh.Mesh.from_buffer_copy(SENTINEL)
        rc = int(lib.nrf_extract_mesh(context.h, C.byref(lat) if lat is not None else None, C.c_float(iso), C.c_void_p(sigma), None,
                                      C.byref(m) if out else None))
        assert bytes(m) == SENTINEL or rc == nh.NRF_OK
        return rc

    def lattice(lat, sigma=None, context=ctx):
        return int(lib.nrf_density_lattice(context.h, C.byref(lat) if lat is not None else None,
                                           C.c_void_p(sig.data_ptr() if sigma is None else sigma), None))

    def make(**kw):
        return nh.Lattice.make(**{**good, **kw})

    bad = [("a dimension below 2", make(dims=d)) for d in ((1, 5, 5), (5, 0, 5), (5, 5, 1))]
    bad += [("more than 2^27 points", make(dims=d)) for d in ((1024, 1024, 129), (65536, 65536, 65536), (2 ** 27 + 1, 1, 1), (2 ** 32 - 1, 2, 2))]
    bad += [("cell", make(cell=[0.25, v, 0.25])) for v in (0.0, -0.25, float("nan"), float("inf"), float("-inf"))]
    bad += [("origin", make(origin=[v, 0.0, 0.0])) for v in (float("nan"), float("inf"), float("-inf"))]
    reserved = make()
    reserved.reserved = 1
    bad.append(("reserved", reserved))
    INV = nh.NRF_E_INVALID
    for what, lat in bad:
        assert extract(lat) == INV, what
        assert extract(lat, sigma=sig.data_ptr()) == INV, what
        assert lattice(lat) == INV, what
    assert extract(None) == INV and extract(make(), out=False) == INV and lattice(None) == INV and lattice(make(), sigma=0) == INV
    for iso in (float("nan"), float("inf"), float("-inf")):
        assert extract(make(), iso=iso) == INV and extract(make(), iso=iso, sigma=sig.data_ptr()) == INV, iso
    with pytest.raises(nh.NerfHipError) as e:
        ctx.extract_mesh(reserved, 1.0)
    assert e.value.code == INV
    # no model and no sigma; nothing to read before the first mesh
    bare = nh.NerfHip(0)
    assert extract(make(), context=bare) == nh.NRF_E_STATE and lattice(make(), context=bare) == nh.NRF_E_STATE
    assert int(lib.nrf_read_mesh(bare.h, None, None)) == nh.NRF_E_STATE
    bare.close()
    # a refused call wrote nothing; the legal edges pass: 2 x 2 x 2, exactly 2^27 points is not tried (1.6 GB of workspace), FLT_MAX as iso
    torch.cuda.synchronize()
    assert bool((sig == 7).all())
    assert extract(make(dims=(2, 2, 2))) == nh.NRF_OK and extract(make(), iso=3.4028234663852886e38) == nh.NRF_OK
    assert lattice(make()) == nh.NRF_OK
    torch.cuda.synchronize()
    assert bool((sig > 0).all())
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
int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const uint32_t n = (uint32_t)std::atoi(argv[2]);
  const float lo = (float)std::atof(argv[3]), iso = (float)std::atof(argv[4]);
  ngp::NerfRender render(std::vector<int>{0});
  render.reload_network_from_file(argv[1]);
  const float origin[3] = {lo, lo, lo}, step = (float)((double)-2.0 * lo / (n - 1)), cell[3] = {step, step, step};
  const uint32_t dims[3] = {n, n, n};
  const ngp::NerfRender::Mesh mesh = render.extract_mesh(origin, cell, dims, iso);
  uint64_t hash = 1469598103934665603ull;  // FNV-1a over the vertices' bytes, then the triangles'
  const unsigned char* b = reinterpret_cast<const unsigned char*>(mesh.vertices.data());
  for (size_t i = 0; i < mesh.vertices.size() * sizeof(float); ++i) hash = (hash ^ b[i]) * 1099511628211ull;
  b = reinterpret_cast<const unsigned char*>(mesh.triangles.data());
  for (size_t i = 0; i < mesh.triangles.size() * sizeof(uint32_t); ++i) hash = (hash ^ b[i]) * 1099511628211ull;
  std::printf("mesh %zu %zu %016llx\n", mesh.vertices.size() / 3, mesh.triangles.size() / 3, (unsigned long long)hash);
  const std::string path = std::string(argv[1]) + ".obj";
  if (!ngp::NerfRender::save_obj(path, mesh.vertices, mesh.triangles)) return 3;
  if (!ngp::NerfRender::save_obj(path + ".n.obj", mesh.vertices, mesh.triangles, mesh.vertices)) return 4;  // (any [n][3] array serves)
  return 0;
}
"""


def test_the_cpp_mirror_returns_the_python_calls_bytes(tmp_path):
    import shutil
    import synthetic as syn
    host = ROOT / "nerf-cuda_amd" / "host"
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None or not (host / "libngp_hip.so").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, keep, cfg = _blob()
    snap = tmp_path / "blob.msgpack"
    syn.write_snapshot(snap, cfg, keep[0], keep[1])
    n = 17
    origin, cell, dims = _box_lattice((n, n, n), -0.75, 0.75)
    ctx = _context(desc, 64, 64)
    m, v, t = _extract(ctx, origin, cell, dims, ISO)
    ctx.close()
    assert m.n_triangles > 100
    want = _fnv1a(v.tobytes() + t.tobytes())
    src, exe = tmp_path / "mesh.cpp", tmp_path / "mesh"
    src.write_text(_PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(host), "-I", str(ROOT / "include"), "-o", str(exe), str(src), f"-L{host}", "-lngp_hip",
                    f"-L{host.parent}", "-lnerfhip", f"-Wl,-rpath,{host}", f"-Wl,-rpath,{host.parent}"], check=True)
    r = subprocess.run([str(exe), str(snap), str(n), "-0.75", repr(ISO)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("mesh ")][-1].split()
    assert (int(line[1]), int(line[2])) == (m.n_vertices, m.n_triangles) and int(line[3], 16) == want, (line, hex(want))
    obj = (tmp_path / "blob.msgpack.obj").read_text().splitlines()
    assert sum(ln.startswith("v ") for ln in obj) == m.n_vertices and sum(ln.startswith("f ") for ln in obj) == m.n_triangles
    faces = np.array([[int(w) for w in ln.split()[1:]] for ln in obj if ln.startswith("f ")])
    assert np.array_equal(faces - 1, t)
    with_normals = (tmp_path / "blob.msgpack.obj.n.obj").read_text().splitlines()
    assert sum(ln.startswith("vn ") for ln in with_normals) == m.n_vertices and with_normals[-1].count("//") == 3
