"""nrf_refine_mesh and nrf_read_mesh_refinement on the GPU.

The definition (include/nerfhip.h, csrc/nrf_refine_plan.h) is held bit for bit to tests/refine_replay.py, the numpy replay that
tests/test_mesh_refine_cpu.py holds to the header, with nrf_density itself as the replay's density; the edge words are held to the
edges of tests/mesh_replay.py's extraction.  What a refinement has to be whatever the code says -- brackets of width 2^-n_steps that
straddle iso, every vertex still on its edge, the mesh still closed, oriented and within its volume bounds -- is checked by property
checkers that share no code with either.  Stages: hot (bound 1, and bound 4 with three cascades), wide, generic, as in
test_density_points_gpu.py; the model with a surface is points_replay.blob_model().  Every test here needs the entry points: none
passes without them."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_replay as mr
import meshcc_replay as cr
import nerfhip as nh
import points_replay as pr
import refine_replay as rr
import test_density_points_gpu as dp
from test_mesh_cpu import noise_field
from test_mesh_gpu import ISO, _blob, _box_lattice, _extract, _lattice_sigma, _peek
from test_point_attributes_gpu import _mesh_attributes, _step
from test_ray_hits_gpu import _fnv1a
from test_render_rays_clip_gpu import _bits, _context, _upload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
NOISE_SCALE = F(64.0)  # noise_field's sigmas are in [0, 1) and the stage models' above 5: times 64 (exact), iso 0.5 becomes 32, about their median


def _refine(ctx, n_steps, n_vertices):
    """(struct, vertices, edges, brackets) of one nrf_refine_mesh call; the arrays through nrf_read_mesh / nrf_read_mesh_refinement AND
    the struct's pointers"""
    r = ctx.refine_mesh(n_steps)
    v, _ = ctx.read_mesh()
    e, b = ctx.read_mesh_refinement()
    n = int(r.n_vertices)
    assert n == n_vertices and v.shape == (n, 3) and e.shape == (n,) and b.shape == (n, 4) and r.n_steps == n_steps and r.reserved == 0
    assert np.array_equal(_bits(_peek(r.vertices, 3 * n, np.float32)), _bits(v).reshape(-1))
    assert np.array_equal(_peek(r.edges, n, np.uint32), e)
    assert np.array_equal(_bits(_peek(r.brackets, 4 * n, np.float32)), _bits(b).reshape(-1))
    return r, v, e, b


def _is_replay(ctx, got, origin, cell, dims, iso, words, before, n_steps):
    """got = _refine's tuple is the replay on those edge words with nrf_density as the density"""
    r, v, e, b = got
    want = rr.refine(origin, cell, dims, iso, words, before, n_steps, lambda x: dp._density(ctx, x))
    assert np.array_equal(e, words)
    assert np.array_equal(_bits(b), _bits(want.brackets)), int(np.any(_bits(b) != _bits(want.brackets), axis=1).sum())
    assert np.array_equal(_bits(v), _bits(want.vertices)), int(np.any(_bits(v) != _bits(want.vertices), axis=1).sum())
    assert r.n_unbracketed == int((~want.bracketed).sum())
    return want


def _off_fp16(value):
    """the fp32 value with its lowest mantissa bit set: no fp16 value, so no sigma of a model equals it"""
    return float((np.array([value], np.float32).view(np.uint32) | np.uint32(1)).view(np.float32)[0])


def _scaled_noise(dims, seed, iso=0.5):
    """noise_field's sigmas and iso times 64, on a lattice of our own inside the box of bound 1 (noise_field's sticks out of it)"""
    _, _, dims, iso, sigma = noise_field(dims, seed=seed, iso=iso)
    origin, cell, dims = _box_lattice(dims, [-0.9, -0.8, -0.95], [0.85, 0.9, 0.7])
    with np.errstate(all="ignore"):
        return origin, cell, dims, F(iso * NOISE_SCALE), (sigma * NOISE_SCALE).astype(np.float32)


# ---------------------------------------------------------------- 1. the replay, stage by stage
@pytest.mark.parametrize("stage", list(dp.STAGES))
def test_refinement_is_the_replay_with_nrf_density(stage):
    ctx, desc = dp._ctx(stage)
    b = float(desc.bound)
    for dims in [(3, 5, 4), (17, 16, 9)]:
        origin, cell, dims = _box_lattice(dims, [-0.9 * b, -0.8 * b, -0.95 * b], [0.85 * b, 0.9 * b, 0.7 * b])  # cells differ by axis
        lat = nh.Lattice.make(origin, cell, dims)
        sigma = _lattice_sigma(ctx, lat)
        iso = _off_fp16(np.median(sigma))
        m, v0, t0 = _extract(ctx, origin, cell, dims, iso)
        ext = mr.mesh(origin, cell, dims, iso, sigma)
        assert np.array_equal(_bits(v0), _bits(ext.vertices)) and m.n_vertices > 20
        words = rr.edge_words(ext, dims)
        e0, none = ctx.read_mesh_refinement(brackets=False)  # readable after the extraction, before any refinement
        assert none is None and np.array_equal(e0, words)
        moved = {}
        for n_steps in (0, 1, 6):
            got = _refine(ctx, n_steps, len(words))
            want = _is_replay(ctx, got, origin, cell, dims, iso, words, v0, n_steps)
            assert want.bracketed.all() and got[0].n_unbracketed == 0  # the lattice is the network's own
            rr.check_refinement(got[1], got[3], origin, cell, dims, iso, words, n_steps)
            moved[n_steps] = float(np.mean(np.any(_bits(got[1]) != _bits(v0), axis=1)))
            _, t = ctx.read_mesh()
            assert np.array_equal(t, t0)
        print(f"{stage} {dims}: iso {iso:.6g}, {len(words)} vertices, share moved by n_steps 0 / 1 / 6: {moved[0]:.3f} / {moved[1]:.3f} / {moved[6]:.3f}")
        assert moved[0] == 0.0 and moved[1] > 0.0 and moved[6] > 0.0  # n_steps 0 is the extraction's interpolation on the same sigmas
    ctx.close()


# ---------------------------------------------------------------- 2. vertex counts
def _corner():
    """one lattice point of a 2 x 2 x 2 lattice inside, a corner with four edges: FOUR vertices.  No lattice has fewer -- the edges of
    a Kuhn cell leave no point with fewer than four, so a count of 1 cannot be reached through the entry points -- and four lanes of a
    wave are as partial a chunk as one"""
    origin, cell, dims = _box_lattice((2, 2, 2), [-0.9, -0.8, -0.95], [0.85, 0.9, 0.7])
    s = np.zeros(dims, np.float32)
    s[1, 0, 0] = 64.0
    return origin, cell, dims, F(32.0), s


# vertices: a partial chunk (4; 55), across a chunk's 64 (126), across a workgroup's 256 (523), and more than ONE grid-stride pass of
# points_grid's 1024 workgroups x 4 waves x 64 = 262 144 vertices (296 757 on 49 x 45 x 40 = 88 200 points: well below (129, 65, 64))
COUNTS = [("corner", 4), ((3, 3, 3), 55), ((3, 5, 4), 126), ((7, 6, 5), 523), ((49, 45, 40), 296757)]


@pytest.mark.parametrize("dims,count", COUNTS)
def test_vertex_counts_on_a_callers_noise_lattice(dims, count):
    """A caller's lattice on a context that has a model: the crossing edges are the noise's, the sigmas the bisection sees are the
    network's -- where both ends of an edge fall on one side of iso the vertex is unbracketed and keeps its bits."""
    ctx, desc = dp._ctx("hot")
    assert float(desc.bound) == 1.0
    origin, cell, dims, iso, sigma = _corner() if dims == "corner" else _scaled_noise(dims, seed=dims[0])
    dev = _upload(sigma.reshape(-1))
    m, v0, t0 = _extract(ctx, origin, cell, dims, float(iso), dev)
    assert m.n_vertices == count
    ext = mr.mesh(origin, cell, dims, iso, sigma)
    assert np.array_equal(_bits(v0), _bits(ext.vertices))
    words = rr.edge_words(ext, dims)
    got = _refine(ctx, 2, count)
    want = _is_replay(ctx, got, origin, cell, dims, float(iso), words, v0, 2)
    k = want.bracketed
    print(f"noise {dims}: {count} vertices, {got[0].n_unbracketed} unbracketed")
    assert np.array_equal(_bits(got[1][~k]), _bits(v0[~k]))  # (the replay says so too; this is the sentence of the header)
    if count > 100:
        assert 0 < got[0].n_unbracketed < count and np.any(_bits(got[1][k]) != _bits(v0[k]))
    rr.check_refinement(got[1], got[3], origin, cell, dims, float(iso), words, 2, bracketed=k)
    _, t = ctx.read_mesh()
    assert np.array_equal(t, t0) and np.array_equal(_bits(dev.cpu().numpy()), _bits(sigma.reshape(-1)))
    ctx.close()


# ---------------------------------------------------------------- 3. the blob
def test_the_blob_moves_onto_its_iso_surface():
    """The blob at iso 30.3 on 33^3 points over [-0.75, 0.75]^3, n_steps = 6.  The CPU oracle (oracle_py.Oracle.network as the density
    of tests/refine_replay.py on the replayed lattice) has 2318 vertices, none unbracketed, and a median of |sigma(v) - iso| over the
    vertices of 0.44062 before and 0.02813 after the refinement (n_steps = 2: 0.03437); sigma is an fp16 value, and those are 0.0156
    apart at 30.  The GPU's two medians are printed and must fall strictly."""
    desc, keep, _ = _blob()
    ctx = _context(desc, 64, 64)
    origin, cell, dims = _box_lattice((33, 33, 33), -0.75, 0.75)
    lat = nh.Lattice.make(origin, cell, dims)
    m, v0, t0 = _extract(ctx, origin, cell, dims, ISO)
    sigma = _peek(m.sigma, lat.n_points, np.float32)
    ext = mr.mesh(origin, cell, dims, ISO, sigma)
    assert np.array_equal(_bits(v0), _bits(ext.vertices)) and np.array_equal(t0, ext.triangles)
    words = rr.edge_words(ext, dims)
    r, v, e, b = _refine(ctx, 6, len(words))
    assert r.n_unbracketed == 0 and np.array_equal(e, words)
    v2, t = ctx.read_mesh()
    assert np.array_equal(t, t0) and v2.tobytes() == v.tobytes()
    rr.check_refinement(v, b, origin, cell, dims, ISO, words, 6)
    V = mr.check_all(mr.Mesh(v, t, ext.edge_p, ext.edge_q, ext.inside), origin, cell, dims)
    V0 = mr.signed_volume(v0, t0)
    before = float(np.median(np.abs(dp._density(ctx, v0).astype(np.float64) - float(F(ISO)))))
    after = float(np.median(np.abs(dp._density(ctx, v).astype(np.float64) - float(F(ISO)))))
    print(f"blob: {len(words)} vertices, median |sigma(v) - iso| {before:.5f} before, {after:.5f} after {r.n_steps} steps; volume {V0:.5f} -> {V:.5f}")
    assert after < before
    ctx.close()


# ---------------------------------------------------------------- 4. after a filter
def test_refinement_after_a_filter_is_the_replay_on_the_kept_edge_words():
    ctx, desc = dp._ctx("hot")
    origin, cell, dims, iso, sigma = _scaled_noise((17, 16, 9), seed=5, iso=0.88)
    dev = _upload(sigma.reshape(-1))
    m, v0, t0 = _extract(ctx, origin, cell, dims, float(iso), dev)
    ext = mr.mesh(origin, cell, dims, iso, sigma)
    assert np.array_equal(_bits(v0), _bits(ext.vertices)) and np.array_equal(t0, ext.triangles)
    words = rr.edge_words(ext, dims)
    parts = cr.parts(len(v0), t0)
    assert len(parts.table) > 3  # several components
    kept = cr.filter_mesh(parts, len(v0), t0, 0, cr.KEEP_LARGEST)
    old = np.asarray(kept.old_vertex, np.int64)
    f = ctx.filter_mesh(0, keep_largest=True)
    assert 0 < f.n_vertices == len(old) < len(v0)
    vf, tf = ctx.read_mesh()
    assert np.array_equal(_bits(vf), _bits(v0[old])) and np.array_equal(tf, kept.triangles)
    ef, _ = ctx.read_mesh_refinement(brackets=False)
    assert np.array_equal(ef, words[old])  # the kept subset of the unfiltered words, in order
    assert int(ctx.lib.nrf_read_mesh_refinement(ctx.h, None, np.empty((len(old), 4), np.float32).ctypes.data_as(C.POINTER(C.c_float)))) == nh.NRF_E_STATE
    got = _refine(ctx, 3, len(old))
    want = _is_replay(ctx, got, origin, cell, dims, float(iso), words[old], vf, 3)
    print(f"noise {dims}: {len(parts.table)} components, the largest has {len(old)} of {len(v0)} vertices, {got[0].n_unbracketed} unbracketed")
    rr.check_refinement(got[1], got[3], origin, cell, dims, float(iso), words[old], 3, bracketed=want.bracketed)
    _, t = ctx.read_mesh()
    assert np.array_equal(t, kept.triangles)
    # a filter after a refinement carries the refined bits and the words, and the brackets of the mesh it replaced are gone
    f2 = ctx.filter_mesh(0)
    v3, _ = ctx.read_mesh()
    e3, _ = ctx.read_mesh_refinement(brackets=False)
    assert f2.n_vertices == len(old) and v3.tobytes() == got[1].tobytes() and np.array_equal(e3, words[old])
    assert int(ctx.lib.nrf_read_mesh_refinement(ctx.h, None, np.empty((len(old), 4), np.float32).ctypes.data_as(C.POINTER(C.c_float)))) == nh.NRF_E_STATE
    ctx.close()


# ---------------------------------------------------------------- 5. idempotence and state
def test_idempotence_and_what_a_refinement_leaves_valid():
    desc, keep, _ = _blob()
    ctx = _context(desc, 64, 64)
    h = _step(F(desc.bound))
    origin, cell, dims = _box_lattice((17, 16, 9), -0.75, 0.75)
    m, v0, t0 = _extract(ctx, origin, cell, dims, ISO)
    n = int(m.n_vertices)
    parts = ctx.mesh_components()
    labels, table = ctx.read_mesh_components()
    _mesh_attributes(ctx, h)
    r1, v1, e1, b1 = _refine(ctx, 6, n)
    assert r1.vertices == m.vertices  # in place
    # the labelling is still served, the attributes are not until asked again
    labels2, table2 = ctx.read_mesh_components()
    assert labels2.tobytes() == labels.tobytes() and table2.tobytes() == table.tobytes() and parts.n_components == len(table)
    assert int(ctx.lib.nrf_read_mesh_attributes(ctx.h, None, None)) == nh.NRF_E_STATE
    # twice the same bytes, from the refined positions as from the extraction's; another step count and back
    r2, v2, e2, b2 = _refine(ctx, 6, n)
    assert v2.tobytes() == v1.tobytes() and e2.tobytes() == e1.tobytes() and b2.tobytes() == b1.tobytes()
    r3, v3, e3, b3 = _refine(ctx, 2, n)
    assert v3.tobytes() != v1.tobytes()
    r4, v4, e4, b4 = _refine(ctx, 6, n)
    assert v4.tobytes() == v1.tobytes() and b4.tobytes() == b1.tobytes()
    # the attributes of the refined mesh are the point call's at the refined vertices
    a, nrm, col = _mesh_attributes(ctx, h)
    pn, pc = torch.full((n, 4), 7.0, device="cuda"), torch.full((n, 4), 7.0, device="cuda")
    x = _upload(v1)
    torch.cuda.synchronize()
    ctx.point_attributes(x.data_ptr(), n, float(h), pn.data_ptr(), pc.data_ptr())
    assert a.n_vertices == n and np.array_equal(_bits(pn.cpu().numpy()), _bits(nrm)) and np.array_equal(_bits(pc.cpu().numpy()), _bits(col))
    assert np.all(nrm[:, 3] > 0)
    # a new extraction: the brackets are gone, the edge words are its own; an empty mesh refines to an empty one
    m5, v5, t5 = _extract(ctx, origin, cell, dims, ISO)
    assert v5.tobytes() == v0.tobytes()
    assert int(ctx.lib.nrf_read_mesh_refinement(ctx.h, None, b1.ctypes.data_as(C.POINTER(C.c_float)))) == nh.NRF_E_STATE
    assert np.array_equal(ctx.read_mesh_refinement(brackets=False)[0], e1)
    _extract(ctx, origin, cell, dims, 3.0e38)
    r6, v6, e6, b6 = _refine(ctx, 6, 0)
    assert (r6.n_vertices, r6.n_unbracketed) == (0, 0) and not r6.vertices and not r6.edges and not r6.brackets
    ctx.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals():
    import synthetic as syn
    ctx, desc = dp._ctx("hot", 64, 48)
    lib = ctx.lib
    ctx.render(syn.default_camera(64, 48), syn.orbit_pose(30, 30))
    frame = [a.copy() for a in ctx.read_f32()]
    st = bytes(ctx.stats())
    SENTINEL = bytes([0xAB]) * C.sizeof(nh.MeshRefine)

    def refine(n_steps, out=True, context=ctx):
        r = nh.MeshRefine.from_buffer_copy(SENTINEL)
        rc = int(lib.nrf_refine_mesh(context.h, C.c_uint32(n_steps), None, C.byref(r) if out else None))
        assert bytes(r) == SENTINEL or rc == nh.NRF_OK
        return rc

    brackets = np.full((256, 4), 7.0, np.float32)
    words = np.full(256, 7, np.uint32)

    def read(context, edges=True, with_brackets=True):
        return int(lib.nrf_read_mesh_refinement(context.h, words.ctypes.data_as(C.POINTER(C.c_uint32)) if edges else None,
                                                brackets.ctypes.data_as(C.POINTER(C.c_float)) if with_brackets else None))

    # no mesh yet
    assert refine(6) == nh.NRF_E_STATE and read(ctx) == nh.NRF_E_STATE and read(ctx, with_brackets=False) == nh.NRF_E_STATE
    origin, cell, dims = _box_lattice((3, 5, 4), [-0.9, -0.8, -0.95], [0.85, 0.9, 0.7])
    iso = _off_fp16(np.median(_lattice_sigma(ctx, nh.Lattice.make(origin, cell, dims))))
    m, v0, t0 = _extract(ctx, origin, cell, dims, iso)
    assert 0 < m.n_vertices <= 256  # (what the two host arrays above hold)
    # brackets before any refinement; the edge words are there
    assert read(ctx) == nh.NRF_E_STATE and np.all(brackets == 7) and np.all(words == 7)
    assert read(ctx, with_brackets=False) == nh.NRF_OK and np.all(words[:m.n_vertices] != 7)
    assert int(lib.nrf_read_mesh_refinement(ctx.h, None, None)) == nh.NRF_OK
    # n_steps above 16, a NULL out, a NULL context
    for n_steps in (17, 18, 255, 2 ** 32 - 1):
        assert refine(n_steps) == nh.NRF_E_INVALID, n_steps
    assert refine(6, out=False) == nh.NRF_E_INVALID
    r = nh.MeshRefine.from_buffer_copy(SENTINEL)
    assert int(lib.nrf_refine_mesh(None, C.c_uint32(6), None, C.byref(r))) == nh.NRF_E_INVALID and bytes(r) == SENTINEL
    assert int(lib.nrf_read_mesh_refinement(None, None, None)) == nh.NRF_E_INVALID
    with pytest.raises(nh.NerfHipError) as e:
        ctx.refine_mesh(17)
    assert e.value.code == nh.NRF_E_INVALID
    # a refused call wrote nothing: the vertices, and still no brackets
    v, t = ctx.read_mesh()
    assert v.tobytes() == v0.tobytes() and t.tobytes() == t0.tobytes() and read(ctx) == nh.NRF_E_STATE
    # no model: a mesh of a caller's lattice has edge words, but no network to ask
    bare = nh.NerfHip(0)
    assert refine(6, context=bare) == nh.NRF_E_STATE
    s = np.zeros(dims, np.float32)
    s[1, 2, 1] = 1.0
    dev = _upload(s.reshape(-1))
    mb, vb, tb = _extract(bare, origin, cell, dims, 0.5, dev)
    assert mb.n_vertices == 14 and refine(6, context=bare) == nh.NRF_E_STATE and refine(17, context=bare) == nh.NRF_E_INVALID
    assert read(bare, with_brackets=False) == nh.NRF_OK and read(bare) == nh.NRF_E_STATE
    assert bare.read_mesh()[0].tobytes() == vb.tobytes()
    bare.close()
    # the legal edges pass: 0 and 16 steps
    assert refine(0) == nh.NRF_OK and refine(16) == nh.NRF_OK and read(ctx) == nh.NRF_OK and np.all(brackets[:m.n_vertices, 1] - brackets[:m.n_vertices, 0] == 2.0 ** -16)
    # statistics and the context's frame: untouched by refused and by served calls alike
    assert bytes(ctx.stats()) == st
    for a, b in zip(ctx.read_f32(), frame):
        assert np.array_equal(_bits(a), _bits(b))
    ctx.close()


# ---------------------------------------------------------------- 7. the C++ mirror
_PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nerf_render.h"
int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const uint32_t n = (uint32_t)std::atoi(argv[2]), n_steps = (uint32_t)std::atoi(argv[5]);
  const float lo = (float)std::atof(argv[3]), iso = (float)std::atof(argv[4]);
  ngp::NerfRender render(std::vector<int>{0});
  render.reload_network_from_file(argv[1]);
  const float origin[3] = {lo, lo, lo}, step = (float)((double)-2.0 * lo / (n - 1)), cell[3] = {step, step, step};
  const uint32_t dims[3] = {n, n, n};
  const ngp::NerfRender::Mesh mesh = render.extract_mesh(origin, cell, dims, iso);
  const ngp::NerfRender::MeshRefinement refined = render.refine_mesh(n_steps);
  if (refined.vertices.size() != mesh.vertices.size() || refined.vertices_dev != mesh.vertices_dev) return 3;
  uint64_t hash = 1469598103934665603ull;  // FNV-1a over the refined vertices' bytes
  const unsigned char* b = reinterpret_cast<const unsigned char*>(refined.vertices.data());
  for (size_t i = 0; i < refined.vertices.size() * sizeof(float); ++i) hash = (hash ^ b[i]) * 1099511628211ull;
  std::printf("refined %zu %llu %016llx\n", refined.vertices.size() / 3, (unsigned long long)refined.unbracketed, (unsigned long long)hash);
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
    m, v0, t0 = _extract(ctx, origin, cell, dims, ISO)
    r, v, e, b = _refine(ctx, 6, int(m.n_vertices))
    ctx.close()
    assert m.n_vertices > 100 and v.tobytes() != v0.tobytes()
    want = _fnv1a(v.tobytes())
    src, exe = tmp_path / "refine.cpp", tmp_path / "refine"
    src.write_text(_PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(host), "-I", str(ROOT / "include"), "-o", str(exe), str(src), f"-L{host}", "-lngp_hip",
                    f"-L{host.parent}", "-lnerfhip", f"-Wl,-rpath,{host}", f"-Wl,-rpath,{host.parent}"], check=True)
    run = subprocess.run([str(exe), str(snap), str(n), "-0.75", repr(ISO), "6"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("refined ")][-1].split()
    assert (int(line[1]), int(line[2])) == (m.n_vertices, r.n_unbracketed) and int(line[3], 16) == want, (line, hex(want))


# ---------------------------------------------------------------- 8. testbed --save_mesh out.ply --mesh_largest --mesh_refine 6
def test_testbed_saves_the_refined_mesh(tmp_path):
    import re
    import synthetic as syn
    import test_point_attributes_cpu as pac
    host = ROOT / "nerf-cuda_amd" / "host"
    if not (host / "testbed").exists():
        pytest.skip("the C++ host mirror is not built")
    desc, keep, cfg = _blob()
    snap = tmp_path / "blob.msgpack"
    syn.write_snapshot(snap, cfg, keep[0], keep[1])
    n, b = 33, F(desc.bound)
    # testbed's lattice: n^3 points over the model's aabb, the step formed in fp32
    origin, cell, dims = [float(-b)] * 3, [float(F(F(2.0) * b) / F(n - 1))] * 3, (n, n, n)
    ctx = _context(desc, 64, 64)
    m, v0, t0 = _extract(ctx, origin, cell, dims, ISO)
    f = ctx.filter_mesh(0, keep_largest=True)
    r, v, e, br = _refine(ctx, 6, int(f.n_vertices))
    _, t = ctx.read_mesh()
    ctx.close()
    assert f.n_triangles > 100
    out = tmp_path / "out.ply"
    run = subprocess.run([str(host / "testbed"), str(snap), "64", "64", str(tmp_path) + "/", "--save_mesh", str(out), "--mesh_largest",
                          "--mesh_refine", "6", "--mesh_res", str(n), "--mesh_iso", repr(ISO)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("mesh refine: ")]
    assert len(line) == 1, run.stdout
    print(line[0])
    got = re.fullmatch(r"mesh refine: (\d+) steps, (\d+) vertices, (\d+) unbracketed, [0-9.]+ s", line[0])
    assert got and [int(g) for g in got.groups()] == [6, f.n_vertices, r.n_unbracketed], line[0]
    pv, pn, prgb, pt = pac.parse_ply(out.read_bytes())
    assert np.array_equal(_bits(pv), _bits(v)) and np.array_equal(pt, t.astype(np.int32)) and len(pn) == f.n_vertices
