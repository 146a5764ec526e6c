"""nrf_mesh_components and nrf_filter_mesh past one grid-stride pass of their launches.

The meshcc kernels run at most 2048 workgroups of 256 lanes, 524 288 vertices or triangles a trip, and the shared mesh scan walks its tile
sums 256 at a time with a carry.  test_mesh_components_gpu.py stays far below both.  Here two caller-supplied noise lattices give
meshes of more than half a million vertices and a million triangles -- A: one giant component (deep forests, many rounds) next to 23
crumbs; B: 21 166 small components with roots on both sides of the pass boundary -- so every kernel takes a second, ragged trip (a
third over the triangles), the roots' scan takes a second carry step and the keep scan a third, the kept counts and the scatter's
output are themselves longer than a pass, and one table row gathers more than a million increments.  Everything is held to
tests/mesh_replay.py and tests/meshcc_replay.py index for index and bit for bit; nothing rests on a tolerance.  The last test walks
one context through small, large and small meshes: the scan workspace, the labels, rows and table and the second buffers regrow from
small capacities and are then reused at large ones.

The numpy replay of A takes several seconds on the CPU, once per module: that, not the GPU, is most of this file's time."""
import functools
import time

import numpy as np
import pytest

import mesh_replay as mr
import meshcc_replay as cr
import nerfhip as nh
from test_mesh_components_cpu import Field, field
from test_mesh_components_gpu import LARGEST, _components, _filter, _is_replay
from test_mesh_cpu import noise_field
from test_mesh_gpu import _extract
from test_render_rays_clip_gpu import _bits, _upload

pytestmark = pytest.mark.gpu

PASS = 2048 * 256   # lanes of one trip of a meshcc launch
SCAN_TILE = 2048    # code words per tile of the mesh scan; its partials kernel takes 256 tiles per carry step
LATTICES = {
    "A": lambda: noise_field((60, 56, 50), seed=60, iso=0.5),
    "B": lambda: noise_field((129, 65, 64), seed=129, iso=0.97, zero_boundary=True),
}
# (vertices, triangles, components, labels >= PASS, triangles of the largest component, roots scan tiles, keep scan tiles)
COUNTS = {
    "A": (569684, 1192836, 24, 6, 1192522, 279, 583),
    "B": (621728, 1159292, 21166, 3227, 1032, 304, 567),
}
FILTERS = [("A", 0, LARGEST), ("B", 0, LARGEST), ("B", 25, 0), ("A", 31, 0), ("A", 0, 0), ("B", 0, 0), ("A", 10 ** 9, 0), ("B", 10 ** 9, 0)]


@functools.lru_cache(maxsize=None)
def big(name):
    """the lattice, its replayed mesh and its replayed components: computed once, shared, never written"""
    origin, cell, dims, iso, sigma = LATTICES[name]()
    mesh = mr.mesh(origin, cell, dims, iso, sigma)
    parts = cr.parts(len(mesh.vertices), mesh.triangles)
    for a in (sigma, mesh.vertices, mesh.triangles, parts.labels, parts.table):
        a.setflags(write=False)
    return Field(origin, cell, dims, iso, sigma, mesh, parts)


def _tiles(n):
    return -(-n // SCAN_TILE)


def _mesh_of(ctx, f):
    """the field's mesh becomes the context's, held to the replay: the device lattice, kept alive by the caller"""
    dev = _upload(f.sigma.reshape(-1))
    m, v, t = _extract(ctx, f.origin, f.cell, f.dims, float(f.iso), dev)
    assert np.array_equal(_bits(v), _bits(f.mesh.vertices)) and np.array_equal(t, f.mesh.triangles)
    return dev


def _labelled(ctx, f, what):
    """one nrf_mesh_components of the context's mesh, which is f's: labels, table, count and rounds against the replay"""
    nv = len(f.mesh.vertices)
    start = time.perf_counter()
    p, lab, table = _components(ctx, nv)
    seconds = time.perf_counter() - start
    assert np.array_equal(lab, f.parts.labels) and np.array_equal(table, f.parts.table) and p.n_components == len(f.parts.table)
    assert 2 <= p.n_rounds <= nv + 1
    print(f"{what}: {nv} vertices, {len(f.mesh.triangles)} triangles, {p.n_components} components, n_rounds {p.n_rounds}, "
          f"{seconds:.3f} s with both read-backs")
    return p, lab, table


# ---------------------------------------------------------------- 0. the lattices are what they should exercise
@pytest.mark.parametrize("name", list(LATTICES))
def test_the_lattices_pass_the_boundaries(name):
    f = big(name)
    nv, nt = len(f.mesh.vertices), len(f.mesh.triangles)
    want_nv, want_nt, want_nc, want_high, want_largest, roots_tiles, keep_tiles = COUNTS[name]
    assert (nv, nt, len(f.parts.table)) == (want_nv, want_nt, want_nc)
    for n in (nv, nt):
        assert n > PASS and n % 256 != 0 and n % 2048 != 0
    assert nt > 2 * PASS  # a third trip over the triangles
    sizes = f.parts.table[:, 2].astype(np.int64)
    assert int((f.parts.table[:, 0] >= PASS).sum()) == want_high and int(sizes.max()) == want_largest
    assert int((sizes == sizes.max()).sum()) == 1  # no tie
    assert (_tiles(nv), _tiles(max(nv, nt))) == (roots_tiles, keep_tiles)
    assert _tiles(nv) > 256  # a second carry step in the roots' scan
    if name == "A":
        assert _tiles(max(nv, nt)) > 512  # a third in the keep scan
        assert sorted(sizes.tolist())[-5:-1] == [24, 24, 24, 30]
        assert sizes.max() > 2 * PASS  # one table row gathers more than a million increments over three trips
    else:
        assert int(np.median(sizes)) == 24
        below = f.parts.table[:, 0] < PASS
        assert below.any() and not below.all()  # roots on both sides of the pass boundary
    cr.check_parts(f.parts.labels, f.parts.table, nv, f.mesh.triangles)


# ---------------------------------------------------------------- 1. labels, table, n_components
@pytest.mark.parametrize("name", list(LATTICES))
def test_labels_and_table_past_one_pass(name):
    f = big(name)
    bare = nh.NerfHip(0)  # no model: none is needed
    dev = _mesh_of(bare, f)
    nv = len(f.mesh.vertices)
    p, lab, table = _labelled(bare, f, name)
    cr.check_parts(lab, table, nv, f.mesh.triangles)
    p2, lab2, table2 = _components(bare, nv)
    assert lab2.tobytes() == lab.tobytes() and table2.tobytes() == table.tobytes() and p2.n_components == p.n_components
    # the mesh itself is read, never written
    v, t = bare.read_mesh()
    assert np.array_equal(_bits(v), _bits(f.mesh.vertices)) and np.array_equal(t, f.mesh.triangles)
    del dev
    bare.close()


# ---------------------------------------------------------------- 2. the filter
@pytest.mark.parametrize("name,min_triangles,flags", FILTERS)
def test_filter_past_one_pass(name, min_triangles, flags):
    f = big(name)
    bare = nh.NerfHip(0)
    dev = _mesh_of(bare, f)
    nv, nt = len(f.mesh.vertices), len(f.mesh.triangles)
    sizes = f.parts.table[:, 2].astype(np.int64)
    giant = int(f.parts.table[int(np.argmax(sizes)), 0])
    start = time.perf_counter()
    m, v, t = _filter(bare, min_triangles, flags)  # (labels the mesh itself: no nrf_mesh_components before it)
    seconds = time.perf_counter() - start
    want = _is_replay(v, t, f.mesh.vertices, f.mesh.triangles, f.parts, min_triangles, flags)
    mr.check_indices(t, len(v))
    print(f"{name}: min_triangles {min_triangles}, flags {flags}: {len(want.kept_labels)} of {len(sizes)} components, {m.n_vertices} vertices, "
          f"{m.n_triangles} triangles, {seconds:.3f} s with the labelling and the read-backs")
    if flags & LARGEST:
        assert want.kept_labels == [giant] and m.n_triangles == COUNTS[name][4]
    elif min_triangles == 25:
        assert 0 < len(want.kept_labels) < len(sizes) and 0 < m.n_triangles < nt and 0 < m.n_vertices < nv
    elif min_triangles == 31:
        assert want.kept_labels == [giant] and m.n_triangles == COUNTS[name][4]
    elif min_triangles == 0:
        assert (m.n_vertices, m.n_triangles) == (nv, nt)
        assert v.tobytes() == f.mesh.vertices.tobytes() and t.tobytes() == f.mesh.triangles.tobytes()
    else:
        assert (m.n_vertices, m.n_triangles) == (0, 0) and not m.vertices and not m.triangles and v.shape == (0, 3) and t.shape == (0, 3)
    if name == "A" and flags & LARGEST:
        # the kept counts and the scatter's output are themselves longer than a pass ...
        assert m.n_triangles == 1192522 and m.n_vertices > PASS and m.n_triangles > PASS
        # ... and the filtered mesh, labelled again, is one component with label 0 and the kept counts
        p, lab, table = _components(bare, int(m.n_vertices))
        assert p.n_components == 1 and table.tolist() == [[0, m.n_vertices, m.n_triangles]] and not lab.any()
        cr.check_parts(lab, table, len(v), t)
    del dev
    bare.close()


# ---------------------------------------------------------------- 3. buffers grow from small capacities and are reused at large ones
def test_small_large_small_in_one_context():
    snake, A = field("snake"), big("A")
    bare = nh.NerfHip(0)
    # small: the scan workspace, labels, rows, table and second buffers get a small mesh's capacities
    dev = _mesh_of(bare, snake)
    _labelled(bare, snake, "snake")
    m, v, t = _filter(bare, 0, LARGEST)
    _is_replay(v, t, snake.mesh.vertices, snake.mesh.triangles, snake.parts, 0, LARGEST)
    # large: the extraction sizes the scan workspace for 168 000 lattice points, the labelling and the filter need it for 1 192 836
    # triangles -- 583 tile sums where 83 were enough
    assert _tiles(int(np.prod(A.dims))) < _tiles(len(A.mesh.triangles))
    dev = _mesh_of(bare, A)
    _labelled(bare, A, "A after snake")
    m, v, t = _filter(bare, 0, LARGEST)
    _is_replay(v, t, A.mesh.vertices, A.mesh.triangles, A.parts, 0, LARGEST)
    mr.check_indices(t, len(v))
    assert m.n_vertices > PASS and m.n_triangles > PASS
    # small again, in buffers of the large capacities
    dev = _mesh_of(bare, snake)
    p, lab, table = _labelled(bare, snake, "snake after A")
    cr.check_parts(lab, table, len(snake.mesh.vertices), snake.mesh.triangles)
    m, v, t = _filter(bare, 0, 0)
    assert v.tobytes() == snake.mesh.vertices.tobytes() and t.tobytes() == snake.mesh.triangles.tobytes()
    del dev
    bare.close()
