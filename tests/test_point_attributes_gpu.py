"""nrf_point_attributes, nrf_mesh_attributes and nrf_read_mesh_attributes on the GPU.

The definition (include/nerfhip.h, csrc/nrf_attr_plan.h) is held bit for bit to code the library already ships: a normal record is the
numpy replay (tests/attr_replay.py, itself held to the header by tests/test_point_attributes_cpu.py) of the SAME call's
nrf_density_gradient record, sigma included; the colour and the sigma are nrf_network's at the point and the replayed direction.  The
guard test is the proof that a refused coordinate never becomes an address.  Stages: hot (bound 1, and bound 4 with three cascades),
wide, generic, as in test_density_points_gpu.py; the model with a surface is points_replay.blob_model().
Every test here needs the entry points: none passes without them."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import attr_replay as ar
import nerfhip as nh
import points_replay as pr
import test_density_points_gpu as dp
import test_point_attributes_cpu as pac
from test_mesh_gpu import ISO, _blob, _box_lattice, _extract, _peek
from test_ray_hits_gpu import _fnv1a
from test_render_rays_clip_gpu import _bits, _context, _upload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
# a partial chunk, a full one, a chunk edge, a block edge (256 points), and one chunk more than one grid-stride pass of 1024 workgroups
# of 4 waves with 64 points each, the last chunk ragged
SIZES = [1, 63, 64, 65, 257, 4 * 1024 * 64 + 65]
INNER = 0.99  # the points stay within bound (1 - 2^-7) = 0.9921875 bound: none is refused at h = 2^-7 bound


def _step(bound):
    return F(F(bound) * F(2.0 ** -7))


def _attributes(ctx, x, h, dirs=None):
    """(normal records [n][4], colour records [n][4]) of one nrf_point_attributes call, outputs pre-filled with a sentinel"""
    x = pr.f32(x).reshape(-1, 3)
    n = len(x)
    tx = _upload(x)
    td = None if dirs is None else _upload(pr.f32(dirs).reshape(-1, 3))
    nrm, col = torch.full((n, 4), 7.0, device="cuda"), torch.full((n, 4), 7.0, device="cuda")
    torch.cuda.synchronize()
    ctx.point_attributes(tx.data_ptr(), n, float(h), nrm.data_ptr(), col.data_ptr(), 0 if td is None else td.data_ptr())
    return nrm.cpu().numpy(), col.cpu().numpy()


def _network(ctx, x, dirs):
    """(sigma [n], rgb [n][3]) of one nrf_network call"""
    x = pr.f32(x).reshape(-1, 3)
    n = len(x)
    tx, td = _upload(x), _upload(pr.f32(dirs).reshape(-1, 3))
    s, rgb = torch.full((n,), 7.0, device="cuda"), torch.full((n, 3), 7.0, device="cuda")
    torch.cuda.synchronize()
    ctx.network(tx.data_ptr(), td.data_ptr(), n, s.data_ptr(), rgb.data_ptr())
    return s.cpu().numpy(), rgb.cpu().numpy()


def _points(stage_bound, n, seed=41):
    x = dp._cube(n, stage_bound, seed=seed, inner=INNER)
    assert pr.guard(x, _step(stage_bound), stage_bound).all()
    return x


# ---------------------------------------------------------------- 1. + 2. normals and colours
@pytest.mark.parametrize("stage", list(dp.STAGES))
def test_normals_are_the_replay_of_nrf_density_gradient(stage):
    ctx, desc = dp._ctx(stage)
    b = F(desc.bound)
    h = _step(b)
    cube = _points(b, max(SIZES))
    for n in SIZES:
        x = cube[-n:]
        nrm, col = _attributes(ctx, x, h)
        want, length, d, ok = ar.records(dp._gradient(ctx, x, h))
        print(f"{stage} n {n}: degenerate {int((~ok).sum())}, |g| {length.min():.4g} .. {length.max():.4g}, sigma {want[:, 3].min():.3g} .. {want[:, 3].max():.3g}")
        assert np.array_equal(_bits(nrm), _bits(want)), (stage, n)
        assert np.array_equal(_bits(col[:, 3]), _bits(length)), (stage, n)
        assert np.all(want[:, 3] > 0)
        if n >= 257:  # (the synthetic models' tables are noise: practically every point has a gradient)
            assert ok.mean() > 0.9 and np.all(ar.norm_error(nrm[ok, :3]) <= ar.NORM_BOUND)
    again = _attributes(ctx, cube[-257:], h)
    assert np.array_equal(_bits(again[0]), _bits(nrm[-257:])) and np.array_equal(_bits(again[1]), _bits(col[-257:]))
    ctx.close()


@pytest.mark.parametrize("stage", list(dp.STAGES))
def test_colours_are_nrf_networks_at_the_replayed_direction(stage):
    ctx, desc = dp._ctx(stage)
    b = F(desc.bound)
    h = _step(b)
    cube = _points(b, max(SIZES))
    for n in SIZES:
        x = cube[-n:]
        nrm, col = _attributes(ctx, x, h)
        _, _, d, ok = ar.records(dp._gradient(ctx, x, h))
        sigma, rgb = _network(ctx, x, d)
        assert np.array_equal(_bits(col[:, :3]), _bits(rgb)), (stage, n)
        assert np.array_equal(_bits(nrm[:, 3]), _bits(sigma)), (stage, n)
        assert np.array_equal(_bits(sigma), _bits(dp._density(ctx, x))), (stage, n)
    # (the colour depends on the direction: the equality above is no accident of a constant)
    assert len(np.unique(col[:, :3], axis=0)) > 100
    _, flipped = _network(ctx, cube[-257:], -d[-257:])
    assert not np.array_equal(_bits(flipped), _bits(col[-257:, :3]))
    ctx.close()


# ---------------------------------------------------------------- 3. given directions
@pytest.mark.parametrize("stage", list(dp.STAGES))
def test_given_directions_colour_the_point_and_leave_the_normal(stage):
    ctx, desc = dp._ctx(stage)
    b = F(desc.bound)
    h = _step(b)
    cube = _points(b, max(SIZES))
    rng = np.random.default_rng(53)
    for n in SIZES:
        x = cube[-n:]
        dirs = dp._unit(n, seed=59 + n)
        dirs[::5] = 0.0                                                         # zeros
        dirs[1::7] *= rng.uniform(0.1, 3.0, (len(dirs[1::7]), 1)).astype(F)   # not unit length
        nrm0, col0 = _attributes(ctx, x, h)
        nrm, col = _attributes(ctx, x, h, dirs)
        sigma, rgb = _network(ctx, x, dirs)
        assert np.array_equal(_bits(col[:, :3]), _bits(rgb)), (stage, n)
        assert np.array_equal(_bits(nrm), _bits(nrm0)) and np.array_equal(_bits(col[:, 3]), _bits(col0[:, 3])), (stage, n)
        assert np.array_equal(_bits(nrm[:, 3]), _bits(sigma)), (stage, n)
        if n >= 257:
            assert not np.array_equal(_bits(col[:, :3]), _bits(col0[:, :3]))
    ctx.close()


# ---------------------------------------------------------------- 4. the guard
@pytest.mark.parametrize("stage", list(dp.STAGES))
def test_refused_coordinates_yield_zeros_and_disturb_nobody(stage):
    ctx, desc = dp._ctx(stage)
    b = F(desc.bound)
    h = _step(b)
    x = dp._cube(257, b, inner=0.9)
    bad = x.copy()
    bad[0, 1] = np.nan
    bad[63, 2] = -np.inf
    bad[64, 0] = np.inf
    bad[100, 2] = np.nextafter(b, F(np.inf))     # the centre leaves the box
    bad[130, 1] = F(b - h * F(0.5))              # the centre is inside, the +y tap is not
    bad[131, 0] = F(h * F(0.5) - b)              # ... the -x tap
    bad[132, 2] = b                              # on the face itself
    bad[256, 0] = F(-2) * b
    off = np.array([0, 63, 64, 100, 130, 131, 132, 256])
    rest = np.setdiff1d(np.arange(257), off)
    ok = pr.guard(bad, h, b, 7)
    assert not ok[off].any() and ok[rest].all() and pr.guard(x, h, b, 7).all()
    assert pr.guard(bad[[130, 131, 132]], h, b, 1).all()  # (only their stencils leave)
    for dirs in (None, dp._unit(257, seed=61)):
        n0, c0 = _attributes(ctx, x, h, dirs)
        n1, c1 = _attributes(ctx, bad, h, dirs)
        assert np.all(n0[:, 3] > 0) and np.any(c0[:, :3] != 0)
        assert np.all(_bits(n1[off]) == 0) and np.all(_bits(c1[off]) == 0)
        assert np.array_equal(_bits(n1[rest]), _bits(n0[rest])) and np.array_equal(_bits(c1[rest]), _bits(c0[rest]))
        # ... and without the refused neighbours at all
        n2, c2 = _attributes(ctx, bad[rest], h, None if dirs is None else dirs[rest])
        assert np.array_equal(_bits(n2), _bits(n0[rest])) and np.array_equal(_bits(c2), _bits(c0[rest]))
    ctx.close()


# ---------------------------------------------------------------- 5. degenerate gradients
@pytest.mark.parametrize("stage", list(dp.STAGES))
def test_a_flat_density_has_no_normal_but_a_colour(stage):
    """The stage's model with every hash-grid parameter zero: the density network sees the same features everywhere, sigma is one
    constant and every central difference is exactly 0."""
    desc0, keep0, cfg = dp._model(stage)
    params = np.array(keep0[0], np.float32).copy()
    lt = nh.level_table(desc0)
    n_grid = int(lt.offset[desc0.n_levels]) * int(desc0.n_features_per_level)
    params[len(params) - n_grid:] = 0.0
    desc, keep = nh.desc_from_config(cfg, params, np.array(keep0[1], np.float32))
    ctx = _context(desc, 64, 64)
    b = F(desc.bound)
    h = _step(b)
    x = _points(b, 257)
    nrm, col = _attributes(ctx, x, h)
    sigma, rgb = _network(ctx, x, np.zeros((257, 3), np.float32))
    assert len(np.unique(_bits(sigma))) == 1 and sigma[0] > 0 and np.isfinite(sigma[0])
    assert np.all(_bits(nrm[:, :3]) == 0) and np.all(_bits(col[:, 3]) == 0)  # positive zeros
    assert np.array_equal(_bits(nrm[:, 3]), _bits(sigma))
    assert np.array_equal(_bits(col[:, :3]), _bits(rgb))
    assert np.all(_bits(dp._gradient(ctx, x, h)[:, :3]) == 0)
    ctx.close()


# ---------------------------------------------------------------- 6. the mesh
def _mesh_attributes(ctx, h):
    """(struct, normal records, colour records) of one nrf_mesh_attributes call; the arrays through nrf_read_mesh_attributes AND the
    struct's pointers"""
    a = ctx.mesh_attributes(float(h))
    nrm, col = ctx.read_mesh_attributes()
    n = int(a.n_vertices)
    assert nrm.shape == (n, 4) and col.shape == (n, 4)
    assert np.array_equal(_bits(_peek(a.normals, 4 * n, np.float32)), _bits(nrm).reshape(-1))
    assert np.array_equal(_bits(_peek(a.colors, 4 * n, np.float32)), _bits(col).reshape(-1))
    return a, nrm, col


def test_mesh_attributes_are_point_attributes_at_the_vertices():
    """The blob at iso 30.3 on 33^3 points over [-0.75, 0.75]^3, h = 2^-7 bound: no vertex is refused (0.75 + 2^-7 < 1).  The CPU
    oracle (oracle_py.Oracle.network on the seven taps of the 2318 vertices of its replayed mesh, tests/attr_replay.py on the
    differences) has 0 degenerate vertices and outward normals, dot(n, v) > 0, on a share of 1.0000 of them; the GPU's two numbers are
    printed, not asserted."""
    desc, keep, _ = _blob()
    ctx = _context(desc, 64, 64)
    b = F(desc.bound)
    h = _step(b)
    origin, cell, dims = _box_lattice((33, 33, 33), -0.75, 0.75)
    m, v, t = _extract(ctx, origin, cell, dims, ISO)
    n = int(m.n_vertices)
    assert n > 1000 and pr.guard(v, h, b, 7).all()
    a, nrm, col = _mesh_attributes(ctx, h)
    assert a.n_vertices == n
    # the same as the point call on the device vertices as they are
    pn, pc = torch.full((n, 4), 7.0, device="cuda"), torch.full((n, 4), 7.0, device="cuda")
    torch.cuda.synchronize()
    ctx.point_attributes(m.vertices, n, float(h), pn.data_ptr(), pc.data_ptr())
    assert np.array_equal(_bits(pn.cpu().numpy()), _bits(nrm)) and np.array_equal(_bits(pc.cpu().numpy()), _bits(col))
    want, length, d, ok = ar.records(dp._gradient(ctx, v, h))
    assert np.array_equal(_bits(nrm), _bits(want)) and np.array_equal(_bits(col[:, 3]), _bits(length))
    assert np.all(ar.norm_error(nrm[ok, :3]) <= ar.NORM_BOUND)
    assert np.all(nrm[:, 3] > 0) and np.any(col[:, :3] != 0)
    outward = np.sum(nrm[:, :3].astype(np.float64) * v.astype(np.float64), axis=1) > 0
    print(f"blob: {n} vertices, outward normals (dot(n, v) > 0) on {np.mean(outward):.4f}, degenerate vertices {int((~ok).sum())}")
    # a new mesh invalidates the attributes until they are made again
    m2, v2, t2 = _extract(ctx, origin, cell, dims, ISO)
    assert int(ctx.lib.nrf_read_mesh_attributes(ctx.h, None, None)) == nh.NRF_E_STATE
    a2, nrm2, col2 = _mesh_attributes(ctx, h)
    assert nrm2.tobytes() == nrm.tobytes() and col2.tobytes() == col.tobytes()
    # an empty mesh: iso above every sigma
    m3, v3, t3 = _extract(ctx, origin, cell, dims, 3.0e38)
    assert m3.n_vertices == 0
    a3, nrm3, col3 = _mesh_attributes(ctx, h)
    assert a3.n_vertices == 0 and len(nrm3) == 0 and len(col3) == 0
    ctx.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    import synthetic as syn
    ctx, desc = dp._ctx("hot-bound4", 64, 48)
    lib = ctx.lib
    b = float(desc.bound)
    ctx.render(syn.default_camera(64, 48), syn.orbit_pose(30, 30))
    frame = [a.copy() for a in ctx.read_f32()]
    st = bytes(ctx.stats())
    x, d = _upload(dp._cube(100, b, inner=0.9)), _upload(dp._unit(100))
    nrm, col = torch.full((100, 4), 7.0, device="cuda"), torch.full((100, 4), 7.0, device="cuda")
    torch.cuda.synchronize()
    px, pd, pn, pc = x.data_ptr(), d.data_ptr(), nrm.data_ptr(), col.data_ptr()
    h = 0.01
    SENTINEL = bytes([0xAB]) * C.sizeof(nh.MeshAttr)

    def pa(xyz=px, dirs=pd, n=100, step=h, normal=pn, color=pc, context=ctx):
        return int(lib.nrf_point_attributes(context.h, C.c_void_p(xyz), C.c_void_p(dirs), n, C.c_float(step), C.c_void_p(normal),
                                            C.c_void_p(color), None))

    def ma(step=h, out=True, context=ctx):
        a = nh.MeshAttr.from_buffer_copy(SENTINEL)
        rc = int(lib.nrf_mesh_attributes(context.h, C.c_float(step), None, C.byref(a) if out else None))
        assert bytes(a) == SENTINEL or rc == nh.NRF_OK
        return rc

    INV, STATE = nh.NRF_E_INVALID, nh.NRF_E_STATE
    # NULL pointers with n > 0 (a NULL direction is no refusal); n == 0 does nothing
    assert pa(xyz=0) == INV and pa(normal=0) == INV and pa(color=0) == INV
    assert pa(xyz=0, dirs=0, n=0, normal=0, color=0) == nh.NRF_OK
    # the step
    steps = (0.0, -0.01, float("nan"), float("inf"), float(np.nextafter(F(b), F(np.inf))))
    for step in steps:
        assert pa(step=step) == INV and pa(step=step, dirs=0) == INV, step
    with pytest.raises(nh.NerfHipError) as e:
        ctx.point_attributes(px, 100, 0.0, pn, pc)
    assert e.value.code == INV
    # mesh attributes before any mesh; nothing to read
    assert ma() == STATE and int(lib.nrf_read_mesh_attributes(ctx.h, None, None)) == STATE
    # no model: the point call, the mesh call before a mesh, and after a mesh made from a caller's lattice
    bare = nh.NerfHip(0)
    assert pa(context=bare) == STATE and ma(context=bare) == STATE
    s = np.zeros((5, 4, 3), np.float32)
    s[2, 2, 1] = 1.0
    lat = nh.Lattice.make([0.0, 0.0, 0.0], [0.1, 0.1, 0.1], (5, 4, 3))
    mesh = bare.extract_mesh(lat, 0.5, _upload(s.reshape(-1)).data_ptr())
    assert mesh.n_vertices == 14
    assert ma(context=bare) == STATE and int(lib.nrf_read_mesh_attributes(bare.h, None, None)) == STATE
    bare.close()
    # a refused call wrote nothing
    torch.cuda.synchronize()
    assert bool((nrm == 7).all()) and bool((col == 7).all())
    # with a mesh: the step and the NULL struct are refused, and there is still nothing to read
    ctx.extract_mesh(nh.Lattice.make([-0.5 * b] * 3, [0.25 * b] * 3, (5, 5, 5)), 1.0)
    assert ma(out=False) == INV
    for step in steps:
        assert ma(step=step) == INV, step
    assert int(lib.nrf_read_mesh_attributes(ctx.h, None, None)) == STATE
    # the legal edges pass: h == bound on points at the centre, with and without directions; served calls
    assert ma() == nh.NRF_OK and int(lib.nrf_read_mesh_attributes(ctx.h, None, None)) == nh.NRF_OK
    zero = _upload(np.zeros((100, 3), np.float32))
    assert pa(xyz=zero.data_ptr(), step=b) == nh.NRF_OK and pa(xyz=zero.data_ptr(), step=b, dirs=0) == nh.NRF_OK
    assert pa() == nh.NRF_OK
    torch.cuda.synchronize()
    assert bool((nrm[:, 3] > 0).all()) and bool((col[:, :3] != 7).any())
    # statistics and the context's frame: untouched by refused and by served calls alike
    assert bytes(ctx.stats()) == st
    for got, want in zip(ctx.read_f32(), frame):
        assert np.array_equal(_bits(got), _bits(want))
    ctx.close()


# ---------------------------------------------------------------- 8. the C++ mirror and the PLY file
_PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "nerf_render.h"
int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const uint32_t n = (uint32_t)std::atoi(argv[2]);
  const float lo = (float)std::atof(argv[3]), iso = (float)std::atof(argv[4]), h = (float)std::atof(argv[5]);
  ngp::NerfRender render(std::vector<int>{0});
  render.reload_network_from_file(argv[1]);
  const float origin[3] = {lo, lo, lo}, step = (float)((double)-2.0 * lo / (n - 1)), cell[3] = {step, step, step};
  const uint32_t dims[3] = {n, n, n};
  const ngp::NerfRender::Mesh mesh = render.extract_mesh(origin, cell, dims, iso);
  const ngp::NerfRender::MeshAttributes a = render.mesh_attributes(h);
  uint64_t hash = 1469598103934665603ull;  // FNV-1a over the bytes of the normals, the colours, the sigmas and the lengths
  for (const std::vector<float>* part : {&a.normals, &a.colors, &a.sigmas, &a.lengths}) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(part->data());
    for (size_t i = 0; i < part->size() * sizeof(float); ++i) hash = (hash ^ b[i]) * 1099511628211ull;
  }
  std::printf("attributes %zu %zu %016llx\n", a.normals.size() / 3, a.sigmas.size(), (unsigned long long)hash);
  if (!ngp::NerfRender::save_ply(std::string(argv[1]) + ".ply", mesh.vertices, mesh.triangles, a.normals, a.colors)) return 3;
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
    h = float(_step(desc.bound))
    origin, cell, dims = _box_lattice((n, n, n), -0.75, 0.75)
    ctx = _context(desc, 64, 64)
    m, v, t = _extract(ctx, origin, cell, dims, ISO)
    a, nrm, col = _mesh_attributes(ctx, h)
    ctx.close()
    assert m.n_triangles > 100 and a.n_vertices == m.n_vertices
    normals, colors = np.ascontiguousarray(nrm[:, :3]), np.ascontiguousarray(col[:, :3])
    want = _fnv1a(normals.tobytes() + colors.tobytes() + np.ascontiguousarray(nrm[:, 3]).tobytes() + np.ascontiguousarray(col[:, 3]).tobytes())
    src, exe = tmp_path / "attr.cpp", tmp_path / "attr"
    src.write_text(_PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(host), "-I", str(ROOT / "include"), "-o", str(exe), str(src), f"-L{host}", "-lngp_hip",
                    f"-L{host.parent}", "-lnerfhip", f"-Wl,-rpath,{host}", f"-Wl,-rpath,{host.parent}"], check=True)
    r = subprocess.run([str(exe), str(snap), str(n), "-0.75", repr(ISO), repr(h)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("attributes ")][-1].split()
    assert int(line[1]) == int(line[2]) == m.n_vertices and int(line[3], 16) == want, (line, hex(want))
    pv, pn, prgb, pt = pac.parse_ply((tmp_path / "blob.msgpack.ply").read_bytes())
    assert np.array_equal(_bits(pv), _bits(v)) and np.array_equal(_bits(pn), _bits(normals)) and np.array_equal(pt, t.astype(np.int32))
    assert np.array_equal(prgb, ar.color_u8(colors)) and len(np.unique(prgb, axis=0)) > 1
