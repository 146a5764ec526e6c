"""nrf_bake_mesh_texture and nrf_read_mesh_texture on the GPU.

The definition (include/nerfhip.h, csrc/nrf_bake_plan.h) is held bit for bit to tests/bake_replay.py, the numpy replay that
tests/test_mesh_texture_cpu.py holds to the plan header: the layout, the owner of every texel, the UVs and the count of refused texels
are the replay's, and every accepted texel is nrf_network's answer, bit for bit, at the replayed position and the replayed head-on
direction; everything else in both planes is zero bits.  The guard test is the proof that a refused coordinate or index never becomes
an address.  Stages: hot (bound 1, and bound 4 with three cascades), wide, generic, as in test_density_points_gpu.py; the model with a
surface is points_replay.blob_model().  Nothing here rests on a tolerance.  Every test here needs the entry points: none passes
without them."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bake_replay as br
import mesh_replay as mr
import nerfhip as nh
import test_density_points_gpu as dp
import test_mesh_texture_cpu as tcpu
from test_mesh_components_gpu import _snapshot
from test_mesh_gpu import ISO, _blob, _box_lattice, _extract, _lattice_sigma, _peek
from test_point_attributes_gpu import _network, _step
from test_ray_hits_gpu import _fnv1a
from test_render_rays_clip_gpu import _bits, _context, _upload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
HOSTDIR = ROOT / "nerf-cuda_amd" / "host"
F = np.float32
ONE_PASS = 1024 * 4 * 64  # work items of one grid-stride pass: 1024 workgroups of 4 waves with 64 lanes


def _bake(ctx, res, width):
    """(struct, texels [H][W][4], rgba8 [H][W], uvs [T][3][2]) of one nrf_bake_mesh_texture call; the arrays through
    nrf_read_mesh_texture AND the struct's pointers"""
    t = ctx.bake_mesh_texture(res, width)
    tex, rgba, uvs = ctx.read_mesh_texture()
    h, w, nt = int(t.height), int(t.width), int(t.n_triangles)
    assert tex.shape == (h, w, 4) and rgba.shape == (h, w) and uvs.shape == (nt, 3, 2) and (t.res, t.width) == (res, width)
    assert np.array_equal(_bits(_peek(t.texels, 4 * h * w, np.float32)), _bits(tex).reshape(-1))
    assert np.array_equal(_peek(t.rgba8, h * w, np.uint32), rgba.reshape(-1))
    assert np.array_equal(_bits(_peek(t.uvs, 6 * nt, np.float32)), _bits(uvs).reshape(-1))
    if not nt:
        assert h == 0 and not t.texels and not t.rgba8 and not t.uvs
    return t, tex, rgba, uvs


def _is_replay(ctx, got, v, t, bound):
    """holds one bake of the mesh (v, t) to the replay and to nrf_network; returns the replay's dict with `rgb` and `sigma` of the
    accepted texels added"""
    s, tex, rgba, uvs = got
    res, width = int(s.res), int(s.width)
    want = br.bake(v, t, res, width, bound)
    assert (s.height, s.cols, s.n_triangles, s.n_refused) == (want["height"], want["cols"], len(t), want["n_refused"])
    assert np.array_equal(_bits(uvs), _bits(want["uvs"]))
    g = want["guard"]
    sigma, rgb = _network(ctx, want["x"][g], want["d"][g]) if g.any() else (np.zeros(0, np.float32), np.zeros((0, 3), np.float32))
    want_tex = np.zeros((want["height"], width, 4), np.float32)
    want_rgba = np.zeros((want["height"], width), np.uint32)
    want_tex[want["py"][g], want["px"][g]] = np.concatenate([rgb, sigma[:, None]], axis=1)
    want_rgba[want["py"][g], want["px"][g]] = br.rgba8(rgb)
    bad = np.nonzero(np.any(_bits(tex) != _bits(want_tex), axis=2))
    assert len(bad[0]) == 0, (len(bad[0]), bad[0][:5], bad[1][:5], tex[bad][:5], want_tex[bad][:5])
    assert np.array_equal(rgba, want_rgba)
    # alpha is the coverage mask: 255 on the accepted texels, the whole word 0 elsewhere
    covered = np.zeros((want["height"], width), bool)
    covered[want["py"][g], want["px"][g]] = True
    assert np.array_equal(rgba >> np.uint32(24) == 255, covered) and np.all(rgba[~covered] == 0)
    want["rgb"], want["sigma"] = rgb, sigma
    return want


# ---------------------------------------------------------------- 1. bit for bit, per stage
@pytest.mark.parametrize("stage", list(dp.STAGES))
def test_texels_are_nrf_networks_at_the_replayed_positions_and_directions(stage):
    ctx, desc = dp._ctx(stage)
    b = F(desc.bound)
    origin, cell, dims = _box_lattice((9, 9, 9), -0.75 * float(b), 0.75 * float(b))
    iso = float(np.median(_lattice_sigma(ctx, nh.Lattice.make(origin, cell, dims))))
    m, v, t = _extract(ctx, origin, cell, dims, iso)
    assert m.n_triangles > 100
    for res, width in ((2, 31), (5, 67)):  # ragged right margins of 3 and 4 texels
        assert width % (res + 2)
        got = _bake(ctx, res, width)
        want = _is_replay(ctx, got, v, t, b)
        assert want["n_refused"] == 0 and want["height"] > 2 * (res + 1) and np.all(want["sigma"] > 0)
        print(f"{stage} r {res}: {m.n_triangles} triangles, atlas {width} x {want['height']}, {len(want['sigma'])} texels, "
              f"{len(np.unique(want['rgb'], axis=0))} colours")
        assert len(np.unique(want["rgb"], axis=0)) > 100
        again = _bake(ctx, res, width)
        assert again[1].tobytes() == got[1].tobytes() and again[2].tobytes() == got[2].tobytes() and again[3].tobytes() == got[3].tobytes()
    v2, t2 = ctx.read_mesh()
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()  # the mesh is only read
    ctx.close()


# ---------------------------------------------------------------- 2. the blob: more work items than one grid-stride pass
def test_the_blob_at_res_10_walks_the_grid_stride_loop_twice():
    desc, keep, _ = _blob()
    ctx = _context(desc, 64, 64)
    b = F(desc.bound)
    origin, cell, dims = _box_lattice((33, 33, 33), -0.75, 0.75)
    m, v, t = _extract(ctx, origin, cell, dims, ISO)
    res, width = 10, 1000
    items = ((int(m.n_triangles) + 1) // 2) * (res + 2) * (res + 1)
    assert m.n_triangles > 4000 and items > ONE_PASS, (m.n_triangles, items)
    got = _bake(ctx, res, width)
    want = _is_replay(ctx, got, v, t, b)
    assert want["n_refused"] == 0 and len(want["sigma"]) == int(m.n_triangles) * 66
    print(f"blob: {m.n_triangles} triangles, {items} work items, atlas {width} x {want['height']}, "
          f"{len(np.unique(want['rgb'], axis=0))} colours, degenerate triangles {int(np.all(want['d'] == 0, axis=1).sum()) // 66}")
    # (the colour depends on the direction: the equality above is no accident of a constant)
    assert len(np.unique(want["rgb"], axis=0)) > 1000
    g = want["guard"]
    _, flipped = _network(ctx, want["x"][g][:4096], -want["d"][g][:4096])
    assert not np.array_equal(_bits(flipped), _bits(want["rgb"][:4096]))
    ctx.close()


# ---------------------------------------------------------------- 3. the bake sees the current mesh
def test_after_simplify_and_refine_the_bake_sees_the_current_mesh():
    desc, keep, _ = _blob()
    ctx = _context(desc, 64, 64)
    b = F(desc.bound)
    origin, cell, dims = _box_lattice((17, 17, 17), -0.75, 0.75)
    m, v0, t0 = _extract(ctx, origin, cell, dims, ISO)
    read = lambda: int(ctx.lib.nrf_read_mesh_texture(ctx.h, None, None, None))  # noqa: E731
    assert read() == nh.NRF_E_STATE
    first = _bake(ctx, 3, 52)
    _is_replay(ctx, first, v0, t0, b)
    assert read() == nh.NRF_OK
    # the attributes and the labelling neither disturb the texture nor are disturbed by it
    ctx.mesh_attributes(float(_step(b)))
    nrm, col = ctx.read_mesh_attributes()
    ctx.mesh_components()
    again = _bake(ctx, 3, 52)
    assert again[1].tobytes() == first[1].tobytes() and read() == nh.NRF_OK
    nrm2, col2 = ctx.read_mesh_attributes()
    assert nrm2.tobytes() == nrm.tobytes() and col2.tobytes() == col.tobytes()
    assert int(ctx.lib.nrf_read_mesh_components(ctx.h, None, None)) == nh.NRF_OK
    # simplified: fewer triangles, the earlier texture is gone until the mesh is baked again
    s = ctx.simplify_mesh(2)
    assert 10 < s.n_triangles < m.n_triangles and read() == nh.NRF_E_STATE
    with pytest.raises(nh.NerfHipError) as e:
        ctx.read_mesh_texture()
    assert e.value.code == nh.NRF_E_STATE
    v1, t1 = ctx.read_mesh()
    second = _bake(ctx, 3, 52)
    _is_replay(ctx, second, v1, t1, b)
    assert second[0].height < first[0].height and read() == nh.NRF_OK
    # refined: the same triangles at other positions
    r = ctx.refine_mesh(4)
    assert read() == nh.NRF_E_STATE
    v2, t2 = ctx.read_mesh()
    assert t2.tobytes() == t1.tobytes() and v2.tobytes() != v1.tobytes() and r.n_vertices == len(v2)
    third = _bake(ctx, 3, 52)
    _is_replay(ctx, third, v2, t2, b)
    assert third[1].tobytes() != second[1].tobytes() and third[3].tobytes() == second[3].tobytes()
    e2, br2 = ctx.read_mesh_refinement()  # the refinement records are untouched by a bake
    assert len(e2) == len(v2) and br2 is not None
    # a filter and a new extraction invalidate it as well
    ctx.filter_mesh(0)
    assert read() == nh.NRF_E_STATE
    _bake(ctx, 2, 40)
    _extract(ctx, origin, cell, dims, ISO)
    assert read() == nh.NRF_E_STATE
    ctx.close()


# ---------------------------------------------------------------- 4. a mesh the lattice boundary cuts; an odd triangle count
def _cut_ball(radius):
    """a caller's sigma on 9 x 8 x 7 points inside the box: a ball about a corner region of the lattice, which the boundary cuts"""
    origin, cell, dims = _box_lattice((9, 8, 7), [-0.8, -0.7, -0.6], [0.7, 0.8, 0.75])
    x = mr.positions(origin, cell, dims).astype(np.float64)
    sigma = (radius - np.linalg.norm(x - np.array([0.55, -0.5, 0.6]), axis=3)).astype(np.float32)
    return origin, cell, dims, sigma


def test_a_surface_the_lattice_boundary_cuts_and_the_last_cell():
    """Caller's sigma arrays whose surface the lattice boundary cuts, the count looked for on the CPU with mesh_replay: the first field
    with an odd triangle count is baked, and the odd half of its last cell has to be zeros.  None of the 40 fields has one, and none can:
    every triangle of the Kuhn split's boundary faces is crossed by the surface's boundary in 0 or 2 of its edges and every lattice point
    of the boundary has an even number of boundary edges, so an open mesh has an even number of boundary edges and, with
    3 T = 2 E_inner + E_boundary, an even T; vertex clustering maps that chain's boundary with it (the replayed simplifications of
    these fields at factors 1, 2, 3 have even counts too).  An odd count therefore reaches the entry point through no call of the
    library; the odd half is held where a mesh can be written down, in tests/test_mesh_texture_cpu.py.  What is held here: the open
    mesh of the first field against the replay, its last, partly filled atlas row included, and, should a field ever have an odd count,
    the empty half."""
    ctx, desc = dp._ctx("hot")
    b = F(desc.bound)
    fields = [_cut_ball(radius) for radius in np.arange(0.45, 0.95, 0.0125)]
    counts = [len(mr.mesh(origin, cell, dims, 0.0, sigma).triangles) for origin, cell, dims, sigma in fields]
    odd = [k for k, n in enumerate(counts) if n % 2 == 1]
    print(f"boundary-cut fields: triangle counts {counts}, odd ones {odd}")
    origin, cell, dims, sigma = fields[odd[0] if odd else 0]
    m, v, t = _extract(ctx, origin, cell, dims, 0.0, sigma=_upload(sigma.reshape(-1)))
    nt = int(m.n_triangles)
    assert nt == counts[odd[0] if odd else 0] and nt > 20, nt
    res, width = 4, 6 * 5 + 3
    got = _bake(ctx, res, width)
    want = _is_replay(ctx, got, v, t, b)
    pairs = (nt + 1) // 2
    assert want["n_refused"] == 0 and pairs % want["cols"] != 0  # (the last row of cells is not full: zeros after the last pair)
    y0, x0 = ((pairs - 1) // want["cols"]) * (res + 1), ((pairs - 1) % want["cols"] + 1) * (res + 2)
    assert np.all(got[2][y0:, x0:] == 0) and np.all(_bits(got[1][y0:, x0:]) == 0)
    if nt % 2 == 1:
        q = nt // 2  # the last pair
        y0, x0 = (q // want["cols"]) * (res + 1), (q % want["cols"]) * (res + 2)
        cell_rgba = got[2][y0:y0 + res + 1, x0:x0 + res + 2]
        cell_tex = got[1][y0:y0 + res + 1, x0:x0 + res + 2]
        jc, ic = np.mgrid[0:res + 1, 0:res + 2]
        odd_half = ic + jc > res
        assert np.all(cell_rgba[odd_half] == 0) and np.all(_bits(cell_tex[odd_half]) == 0) and np.all(cell_rgba[~odd_half] >> np.uint32(24) == 255)
    ctx.close()


# ---------------------------------------------------------------- 5. the guard
def _per_triangle(want, tex, res):
    """float32 [n_triangles][half][4] and bool [n_triangles][half]: every triangle's texels and their guard, ordered by (j, i)"""
    half = (res + 1) * (res + 2) // 2
    order = np.lexsort((want["i"], want["j"], want["tri"]))
    nt = len(want["uvs"])
    vals = tex[want["py"], want["px"]][order].reshape(nt, half, 4)
    return vals, want["guard"][order].reshape(nt, half)


def test_refused_texels_are_zeros_and_disturb_nobody():
    """A caller's lattice over [-1.5, 1.5]^3 on a model of bound 1, a cylinder of radius 0.6 along x: the surface leaves the box through
    two faces.  Then the same cylinder with every sigma beyond |x| = 0.75 below iso: a mesh that lacks the triangles out there and shares
    the ones within, with other numbers.  The shared triangles, found by their vertices' bits, have the same texels in both bakes."""
    ctx, desc = dp._ctx("hot")
    b = F(desc.bound)
    origin, cell, dims = _box_lattice((13, 13, 13), -1.5, 1.5)
    x = mr.positions(origin, cell, dims).astype(np.float64)
    sigma = (0.6 - np.hypot(x[..., 1] - 0.03, x[..., 2] + 0.02)).astype(np.float32)
    res, width = 4, 6 * 17 + 5
    m, v, t = _extract(ctx, origin, cell, dims, 0.0, sigma=_upload(sigma.reshape(-1)))
    got = _bake(ctx, res, width)
    want = _is_replay(ctx, got, v, t, b)
    g = want["guard"]
    half = (res + 1) * (res + 2) // 2
    vals, ok = _per_triangle(want, got[1], res)
    whole, none = ok.all(axis=1), ~ok.any(axis=1)
    print(f"guard: {m.n_triangles} triangles, {want['n_refused']} of {len(g)} texels refused; triangles wholly accepted {whole.sum()}, "
          f"wholly refused {none.sum()}, partly {(~whole & ~none).sum()}")
    assert got[0].n_refused == want["n_refused"] > 0 and whole.sum() > 50 and none.sum() > 50 and (~whole & ~none).sum() > 10
    assert np.all(_bits(got[1][want["py"][~g], want["px"][~g]]) == 0) and np.all(got[2][want["py"][~g], want["px"][~g]] == 0)
    # ... and without the refused neighbours at all
    sigma2 = np.where(np.abs(x[..., 0]) <= 0.75, sigma, F(-1.0)).astype(np.float32)
    m2, v2, t2 = _extract(ctx, origin, cell, dims, 0.0, sigma=_upload(sigma2.reshape(-1)))
    assert np.all(np.abs(v2) <= 1.0)  # (its cut lies between |x| = 0.75 and 1: every vertex is in the box)
    got2 = _bake(ctx, res, width)
    want2 = _is_replay(ctx, got2, v2, t2, b)
    vals2, ok2 = _per_triangle(want2, got2[1], res)
    key2 = {v2[tri].tobytes(): k for k, tri in enumerate(t2.astype(np.int64))}
    keys = [v[tri].tobytes() for tri in t.astype(np.int64)]
    shared = [(k, key2[key]) for k, key in enumerate(keys) if key in key2]
    print(f"guard: the second mesh has {m2.n_triangles} triangles, {len(shared)} shared, {want2['n_refused']} texels refused")
    assert len(shared) > 50 and any(k != k2 for k, k2 in shared)
    k1, k2 = np.array(shared).T
    assert whole[k1].all() and ok2[k2].all() and np.array_equal(_bits(vals[k1]), _bits(vals2[k2]))
    assert not any(keys[k] in key2 for k in np.nonzero(~whole)[0])  # no triangle with a refused texel is in the second mesh
    ctx.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals():
    import synthetic as syn
    ctx, desc = dp._ctx("hot-bound4", 64, 48)
    lib = ctx.lib
    b = float(desc.bound)
    ctx.render(syn.default_camera(64, 48), syn.orbit_pose(30, 30))
    frame = [a.copy() for a in ctx.read_f32()]
    st = bytes(ctx.stats())
    SENTINEL = bytes([0xAB]) * C.sizeof(nh.MeshTexture)
    INV, STATE, OK = nh.NRF_E_INVALID, nh.NRF_E_STATE, nh.NRF_OK

    def bake(res=4, width=64, out=True, context=ctx):
        s = nh.MeshTexture.from_buffer_copy(SENTINEL)
        rc = int(lib.nrf_bake_mesh_texture(context.h, res, width, None, C.byref(s) if out else None))
        assert bytes(s) == SENTINEL or rc == OK  # a refused call writes nothing
        return rc

    def read(context=ctx):
        return int(lib.nrf_read_mesh_texture(context.h, None, None, None))

    # before any mesh: the arguments are judged first, then the state
    assert bake(out=False) == INV
    for res, width in [(1, 64), (0, 64), (257, 1000), (4, 5), (4, 16385), (4, 0), (256, 257)]:
        assert bake(res, width) == INV, (res, width)
    assert bake() == STATE and read() == STATE
    assert int(lib.nrf_bake_mesh_texture(None, 4, 64, None, C.byref(nh.MeshTexture()))) == INV
    assert int(lib.nrf_read_mesh_texture(None, None, None, None)) == INV
    # no model: before a mesh, and after a mesh made from a caller's lattice
    bare = nh.NerfHip(0)
    assert bake(context=bare) == STATE and bake(out=False, context=bare) == INV and bake(1, 64, context=bare) == INV
    s = np.zeros((5, 4, 3), np.float32)
    s[2, 2, 1] = 1.0
    mesh = bare.extract_mesh(nh.Lattice.make([0.0, 0.0, 0.0], [0.1, 0.1, 0.1], (5, 4, 3)), 0.5, _upload(s.reshape(-1)).data_ptr())
    assert mesh.n_vertices == 14
    assert bake(context=bare) == STATE and read(context=bare) == STATE
    bare.close()
    # with a mesh of the model: the arguments; an atlas beyond the limits, with the width that would do in the message
    origin, cell, dims = _box_lattice((9, 9, 9), -0.75 * b, 0.75 * b)
    iso = float(np.median(_lattice_sigma(ctx, nh.Lattice.make(origin, cell, dims))))
    m, v, t = _extract(ctx, origin, cell, dims, iso)
    nt = int(m.n_triangles)
    assert nt > 130
    assert bake(out=False) == INV and bake(1, 64) == INV and bake(4, 5) == INV and bake(257, 1000) == INV and bake(4, 16385) == INV
    assert bake(64, 66) == INV and br.layout(nt, 64, 66) is None and br.smallest_width(nt, 64) > 66
    assert f"smallest width that fits is {br.smallest_width(nt, 64)}" in lib.nrf_last_error().decode(), lib.nrf_last_error()
    assert bake(256, 16384) == INV and br.params_valid(256, 16384) and br.smallest_width(nt, 256) == 0
    assert "no width fits" in lib.nrf_last_error().decode(), lib.nrf_last_error()
    assert read() == STATE
    with pytest.raises(nh.NerfHipError) as e:
        ctx.bake_mesh_texture(64, 66)
    assert e.value.code == INV
    # the legal edges pass: the smallest res on one column, and the smallest width that fits at the res refused above
    got = _bake(ctx, 2, 4)
    assert got[0].height == 3 * ((nt + 1) // 2) and got[0].cols == 1
    assert bake(64, br.smallest_width(nt, 64)) == OK and bake(64, br.smallest_width(nt, 64) - 1) == INV
    # a refused call leaves the texture that is there
    assert bake(1, 64) == INV and bake(64, 66) == INV
    assert read() == OK
    # an empty mesh is accepted: height 0, nothing to copy
    m3, v3, t3 = _extract(ctx, origin, cell, dims, 3.0e38)
    assert m3.n_triangles == 0 and read() == STATE
    empty = _bake(ctx, 4, 64)
    assert (empty[0].height, empty[0].n_triangles, empty[0].n_refused, empty[0].cols) == (0, 0, 0, 10) and read() == OK
    # statistics and the context's frame: untouched by refused and by served calls alike
    assert bytes(ctx.stats()) == st
    for a, bb in zip(ctx.read_f32(), frame):
        assert np.array_equal(_bits(a), _bits(bb))
    ctx.close()


# ---------------------------------------------------------------- 7. the C++ mirror and the files
_PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "nerf_render.h"
static uint64_t fnv(uint64_t hash, const void* p, size_t bytes) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < bytes; ++i) hash = (hash ^ b[i]) * 1099511628211ull;
  return hash;
}
int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const uint32_t n = (uint32_t)std::atoi(argv[2]);
  const float lo = (float)std::atof(argv[3]), iso = (float)std::atof(argv[4]);
  ngp::NerfRender render(std::vector<int>{0});
  render.reload_network_from_file(argv[1]);
  const float origin[3] = {lo, lo, lo}, step = (float)((double)-2.0 * lo / (n - 1)), cell[3] = {step, step, step};
  const uint32_t dims[3] = {n, n, n};
  render.extract_mesh(origin, cell, dims, iso);
  const ngp::NerfRender::SimplifiedMesh mesh = render.simplify_mesh((uint32_t)std::atoi(argv[5]));
  const ngp::NerfRender::MeshTexture tex = render.bake_mesh_texture((uint32_t)std::atoi(argv[6]), (uint32_t)std::atoi(argv[7]));
  uint64_t hash = fnv(1469598103934665603ull, tex.texels.data(), tex.texels.size() * sizeof(float));
  hash = fnv(hash, tex.rgba8.data(), tex.rgba8.size() * sizeof(uint32_t));
  hash = fnv(hash, tex.uvs.data(), tex.uvs.size() * sizeof(float));
  std::printf("texture %u %u %u %zu %llu %016llx\n", tex.width, tex.height, tex.res, tex.uvs.size() / 6, (unsigned long long)tex.refused,
              (unsigned long long)hash);
  if (!ngp::NerfRender::save_obj_textured(std::string(argv[1]) + ".obj", mesh.vertices, mesh.triangles, tex.uvs, tex.rgba8, tex.width, tex.height))
    return 3;
  return 0;
}
"""


def test_the_cpp_mirror_returns_the_python_calls_bytes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None or not (HOSTDIR / "libngp_hip.so").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, snap = _snapshot(tmp_path)
    n, res, width = 17, 6, 203
    origin, cell, dims = _box_lattice((n, n, n), -0.75, 0.75)
    ctx = _context(desc, 64, 64)
    _extract(ctx, origin, cell, dims, ISO)
    ctx.simplify_mesh(2)
    v, t = ctx.read_mesh()
    s, tex, rgba, uvs = _bake(ctx, res, width)
    ctx.close()
    assert s.n_triangles > 10
    src, exe = tmp_path / "bake.cpp", tmp_path / "bake"
    src.write_text(_PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(HOSTDIR), "-I", str(ROOT / "include"), "-o", str(exe), str(src), f"-L{HOSTDIR}", "-lngp_hip",
                    f"-L{HOSTDIR.parent}", "-lnerfhip", f"-Wl,-rpath,{HOSTDIR}", f"-Wl,-rpath,{HOSTDIR.parent}"], check=True)
    r = subprocess.run([str(exe), str(snap), str(n), "-0.75", repr(ISO), "2", str(res), str(width)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("texture ")][-1].split()
    assert [int(a) for a in line[1:6]] == [width, s.height, res, s.n_triangles, s.n_refused], line
    assert int(line[6], 16) == _fnv1a(tex.tobytes() + rgba.tobytes() + uvs.tobytes()), line
    # the files: 3 vt per triangle = the uvs with v flipped, faces that name them, an image of the atlas's size and bytes
    pv, vt, faces, atlas = tcpu.parse_obj_textured(Path(str(snap) + ".obj"))
    nt = int(s.n_triangles)
    want_vt = uvs.reshape(-1, 2).copy()
    want_vt[:, 1] = F(1) - want_vt[:, 1]
    assert len(vt) == 3 * nt and np.array_equal(_bits(vt), _bits(want_vt))
    assert np.array_equal(_bits(pv), _bits(v)) and np.array_equal(faces[:, :, 0], t.astype(np.int64))
    assert np.array_equal(faces[:, :, 1], np.arange(3 * nt).reshape(nt, 3))
    assert atlas.shape == (s.height, width, 3)
    assert np.array_equal(atlas, np.stack([(rgba >> np.uint32(8 * k)) & np.uint32(255) for k in range(3)], axis=2).astype(np.uint8))
    assert len(np.unique(atlas.reshape(-1, 3), axis=0)) > 100


# ---------------------------------------------------------------- 8. testbed --save_mesh out.obj --mesh_simplify 2 --mesh_texture 8
def test_testbed_saves_the_textured_mesh(tmp_path):
    if not (HOSTDIR / "testbed").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, snap = _snapshot(tmp_path)
    n, b = 33, F(desc.bound)
    # testbed's lattice: n^3 points over the model's aabb, the step formed in fp32
    origin, cell, dims = [float(-b)] * 3, [float(F(F(2.0) * b) / F(n - 1))] * 3, (n, n, n)
    ctx = _context(desc, 64, 64)
    _extract(ctx, origin, cell, dims, ISO)
    ctx.simplify_mesh(2)
    v, t = ctx.read_mesh()
    s, tex, rgba, uvs = _bake(ctx, 8, 4096)
    ctx.close()
    out = tmp_path / "out.obj"
    r = subprocess.run([str(HOSTDIR / "testbed"), str(snap), "64", "64", str(tmp_path) + "/", "--save_mesh", str(out), "--mesh_simplify", "2",
                        "--mesh_texture", "8", "--mesh_res", str(n), "--mesh_iso", repr(ISO)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("mesh texture: ")]
    assert len(line) == 1, r.stdout
    print(line[0])
    got = re.fullmatch(r"mesh texture: res (\d+), atlas (\d+) x (\d+), (\d+) triangles, (\d+) texels refused, [0-9.]+ s", line[0])
    assert got and [int(a) for a in got.groups()] == [8, 4096, s.height, s.n_triangles, s.n_refused], line[0]
    pv, vt, faces, atlas = tcpu.parse_obj_textured(out)
    assert np.array_equal(_bits(pv), _bits(v)) and np.array_equal(faces[:, :, 0], t.astype(np.int64)) and len(vt) == 3 * len(t)
    assert atlas.shape == (s.height, 4096, 3)
    assert np.array_equal(atlas, np.stack([(rgba >> np.uint32(8 * k)) & np.uint32(255) for k in range(3)], axis=2).astype(np.uint8))
