"""The definition of nrf_simplify_mesh in numpy -- TEST INFRASTRUCTURE ONLY -- written from the comment in include/nerfhip.h, by a
different algorithm from the library's: one stable sort of the vertices by (cluster, key) whose first entry per cluster is the
representative (no key table, no atomic minimum, no scan), and property checkers of a simplified mesh that share no code with it
or with csrc/nrf_simplify_plan.h.

tests/test_mesh_simplify_cpu.py holds host/simplify_plan_check.cpp (the plan header under the sanitizers) to this module, and the GPU
tests hold the kernels to it.  Every numpy operation on float32 arrays is one fp32 rounding, which is what the library's build
(-ffp-contract=off -fno-fast-math) makes of the header; everything else is integers and copied float bits: every comparison is exact."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
MAX_FACTOR = 256

# vertices float32 [n][3], triangles uint32 [m][3], edges uint32 [n], sources uint32 [n], vertex_map uint32 [n before];
# cluster int64 [n before], key uint64 [n before], rep int64 [n before] (-1: no cluster)
Simplified = namedtuple("Simplified", "vertices triangles edges sources vertex_map cluster key rep")


def blocks(dims, factor):
    return [(int(d) - 1) // int(factor) + 1 for d in dims]


def clusters(dims, factor, words):
    """(cluster id int64 [n], block indices int64 [n][3]) of the edge words; -1 where the owner point is not in the lattice"""
    nx, ny, nz = (int(d) for d in dims)
    p = np.asarray(words, np.uint32).astype(np.int64) >> 3
    k, ij = p % nz, p // nz
    j, i = ij % ny, ij // ny
    b = np.stack([i, j, k], axis=1) // int(factor)
    nb = blocks(dims, factor)
    cid = (b[:, 0] * nb[1] + b[:, 1]) * nb[2] + b[:, 2]
    cid[p >= nx * ny * nz] = -1
    return cid, b


def keys(origin, cell, dims, factor, words, vertices):
    """(cluster int64 [n], key uint64 [n]) of every vertex"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    cid, b = clusters(dims, factor, words)
    with np.errstate(all="ignore"):
        d = []
        for c in range(3):
            n = ((2 * b[:, c] + 1) * int(factor)).astype(np.float32)
            half = F(0.5) * F(cell[c])
            cc = (F(origin[c]) + (n * half).astype(np.float32)).astype(np.float32)
            d.append((v[:, c] - cc).astype(np.float32))
        xx, yy, zz = ((a * a).astype(np.float32) for a in d)
        d2 = ((xx + yy).astype(np.float32) + zz).astype(np.float32)
        hi = np.where(d2 < F(np.inf), d2.view(np.uint32), np.uint32(0x7F800000)).astype(np.uint64)
    return cid, (hi << np.uint64(32)) | np.arange(len(v), dtype=np.uint64)


def simplify(origin, cell, dims, factor, words, vertices, triangles):
    assert 1 <= int(factor) <= MAX_FACTOR
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    w = np.ascontiguousarray(words, np.uint32).reshape(-1)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3).astype(np.int64)
    nv = len(v)
    assert len(w) == nv
    cid, key = keys(origin, cell, dims, factor, w, v)
    rep = np.full(nv, -1, np.int64)
    order = np.lexsort((key, cid))  # by cluster, then by key: the first of a cluster's run is its minimum
    order = order[cid[order] >= 0]
    if len(order):
        sc = cid[order]
        first = np.r_[True, sc[1:] != sc[:-1]]
        run = np.cumsum(first) - 1
        rep[order] = order[first][run]
    t = t[np.all(t < nv, axis=1)] if len(t) else t
    r = rep[t] if len(t) else np.zeros((0, 3), np.int64)
    alive = np.all(r >= 0, axis=1) & (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2])
    r = r[alive]
    kept = np.zeros(nv, bool)
    kept[r.reshape(-1)] = True
    new_id = np.cumsum(kept) - kept
    sources = np.nonzero(kept)[0]
    vmap = np.full(nv, NONE, np.int64)
    has = rep >= 0
    ok = has.copy()
    ok[has] = kept[rep[has]]
    vmap[ok] = new_id[rep[ok]]
    return Simplified(v[sources].copy(), new_id[r].astype(np.uint32).reshape(-1, 3), w[sources].copy(), sources.astype(np.uint32),
                      vmap.astype(np.uint32), cid, key, rep)


def signed_volume(vertices, triangles):
    """sum over the triangles of a . (b x c) / 6, in float64"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if not len(t):
        return 0.0
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ---------------------------------------------------------------- property checkers (nothing above is used below)
def check_triangles(triangles, n_vertices):
    """every triangle has three distinct indices, all < n_vertices"""
    t = np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    assert np.all(t >= 0) and np.all(t < n_vertices), "a triangle names a vertex out of range"
    assert np.all(t[:, 0] != t[:, 1]) and np.all(t[:, 1] != t[:, 2]) and np.all(t[:, 0] != t[:, 2]), "a collapsed triangle"


def check_referenced(triangles, n_vertices):
    """every vertex is referenced"""
    t = np.asarray(triangles).reshape(-1).astype(np.int64)
    seen = np.zeros(n_vertices, bool)
    seen[t[t < n_vertices]] = True
    assert seen.all(), "an unreferenced vertex"


def check_sources(sources, vertices, edges, old_vertices, old_edges):
    """sources ascends, and the vertices and edge words are those of sources, bit for bit"""
    s = np.asarray(sources).reshape(-1).astype(np.int64)
    ov = np.ascontiguousarray(old_vertices, np.float32).reshape(-1, 3).view(np.uint32)
    oe = np.asarray(old_edges, np.uint32).reshape(-1)
    assert np.all(np.diff(s) > 0), "sources do not ascend"
    assert len(s) == 0 or (s[0] >= 0 and s[-1] < len(ov)), "a source out of range"
    nv = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).view(np.uint32)
    assert len(nv) == len(s) == len(np.asarray(edges).reshape(-1))
    assert np.array_equal(nv, ov[s]), "a vertex is not its source's bits"
    assert np.array_equal(np.asarray(edges, np.uint32).reshape(-1), oe[s]), "an edge word is not its source's"


def check_vertex_map(vertex_map, sources, old_edges, dims, factor):
    """vertex_map is consistent with sources (a kept vertex maps to itself, every entry is a new id or NONE, an entry's source lies
    in the vertex's own cluster) and with "same cluster gives the same entry" """
    m = np.asarray(vertex_map).reshape(-1).astype(np.int64)
    s = np.asarray(sources).reshape(-1).astype(np.int64)
    e = np.asarray(old_edges, np.uint32).reshape(-1).astype(np.int64)
    assert len(m) == len(e)
    real = m != NONE
    assert np.all(m[real] < len(s)), "an entry beyond the kept vertices"
    assert np.array_equal(m[s], np.arange(len(s))), "a kept vertex does not map to itself"
    ny, nz = int(dims[1]), int(dims[2])
    p = e >> 3
    block = np.stack([p // (ny * nz) // factor, (p // nz) % ny // factor, p % nz // factor], axis=1)
    span = int(block.max()) + 1 if len(block) else 1
    cluster = (block[:, 0] * span + block[:, 1]) * span + block[:, 2]
    assert np.array_equal(cluster[real], cluster[s[m[real]]]), "an entry's source lies in another cluster"
    entry = {}
    for c, x in zip(cluster.tolist(), m.tolist()):
        assert entry.setdefault(c, x) == x, "two vertices of one cluster have different entries"


def check_balanced(triangles):
    """the multiset of directed edges equals that of their opposites: closed as a chain"""
    t = np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    if not len(t):
        return
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    span = int(t.max()) + 1
    fwd, bwd = np.sort(a * span + b), np.sort(b * span + a)
    assert np.array_equal(fwd, bwd), "a directed edge occurs more often than its opposite"


def check_all(got_vertices, got_triangles, got_edges, sources, vertex_map, old_vertices, old_edges, dims, factor):
    n = len(np.asarray(sources).reshape(-1))
    check_triangles(got_triangles, n)
    check_referenced(got_triangles, n)
    check_sources(sources, got_vertices, got_edges, old_vertices, old_edges)
    check_vertex_map(vertex_map, sources, old_edges, dims, factor)
