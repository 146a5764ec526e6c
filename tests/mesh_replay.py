"""The definition of nrf_density_lattice / nrf_extract_mesh in vectorised numpy -- TEST INFRASTRUCTURE ONLY -- written from the
comment at the head of csrc/nrf_mesh_plan.h, and property checkers of a triangle mesh that share no code with it.

Every numpy operation on float32 arrays is one fp32 rounding, which is what the library's build (-ffp-contract=off -fno-fast-math)
makes of the header; tests/test_mesh_cpu.py holds this module to the header bit for bit through host/mesh_plan_check.cpp, and the
GPU tests hold the kernels to this module."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

F = np.float32
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]  # xyz, xzy, yxz, yzx, zxy, zyx
SWAP = [0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da]  # bit `mask` of SWAP[t]: swap the last two indices (test_mesh_cpu.py proves it)

Mesh = namedtuple("Mesh", "vertices triangles edge_p edge_q inside")  # edge_p / edge_q: the lattice points of each vertex's edge


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def bits(a):
    return f32(a).view(np.uint32)


def code_offset(code):
    return code & 1, (code >> 1) & 1, (code >> 2) & 1


def tet_corners(t):
    """the four corners of tetrahedron t as corner codes of the cell (bit 0 = +x, bit 1 = +y, bit 2 = +z)"""
    a, b, _ = PERMS[t]
    return [0, 1 << a, (1 << a) | (1 << b), 7]


def tet_triangles(t, mask):
    """the triangles of tetrahedron t with inside mask `mask` (bit i = corner i inside): a list of triangles, each three edges
    (x, y) of corner NUMBERS 0 .. 3, in the definition's order and with the swap applied"""
    ins = [i for i in range(4) if (mask >> i) & 1]
    out = [i for i in range(4) if not (mask >> i) & 1]
    if not ins or not out:
        return []
    if len(ins) == 2:
        (a, b), (c, d) = ins, out
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    else:
        lone = ins[0] if len(ins) == 1 else out[0]
        r = [i for i in range(4) if i != lone]
        tris = [[(lone, r[0]), (lone, r[1]), (lone, r[2])]]
    if (SWAP[t] >> mask) & 1:
        tris = [[e0, e2, e1] for e0, e1, e2 in tris]
    return tris


def positions(origin, cell, dims):
    """[nx][ny][nz][3] fp32: x_c = origin_c + (float)index_c * cell_c, the product rounded, then the sum"""
    origin, cell = f32(origin), f32(cell)
    axes = []
    with np.errstate(all="ignore"):
        for c in range(3):
            s = (np.arange(dims[c]).astype(np.float32) * cell[c]).astype(np.float32)
            axes.append((origin[c] + s).astype(np.float32))
    x = np.empty(tuple(dims) + (3,), np.float32)
    x[..., 0] = axes[0][:, None, None]
    x[..., 1] = axes[1][None, :, None]
    x[..., 2] = axes[2][None, None, :]
    return x


def mesh(origin, cell, dims, iso, sigma):
    nx, ny, nz = (int(d) for d in dims)
    n = nx * ny * nz
    s = f32(sigma).reshape(nx, ny, nz)
    iso = F(iso)
    with np.errstate(all="ignore"):
        inside = s >= iso  # NaN is outside
    x = positions(origin, cell, (nx, ny, nz))
    lin = np.arange(n).reshape(nx, ny, nz)
    # crossing edges: cross[p][m]
    cross = np.zeros((nx, ny, nz, 8), bool)
    for m in range(1, 8):
        di, dj, dk = code_offset(m)
        cross[:nx - di, :ny - dj, :nz - dk, m] = inside[:nx - di, :ny - dj, :nz - dk] != inside[di:, dj:, dk:]
    cross = cross.reshape(n, 8)
    counts = cross.sum(axis=1)
    vbase = np.concatenate([[0], np.cumsum(counts)[:-1]])
    vid = vbase[:, None] + np.cumsum(cross, axis=1) - cross  # id of edge m of p where it crosses
    nv = int(counts.sum())
    vertices = np.zeros((nv, 3), np.float32)
    edge_p, edge_q = np.zeros(nv, np.int64), np.zeros(nv, np.int64)
    xf, sf = x.reshape(n, 3), s.reshape(n)
    for m in range(1, 8):
        di, dj, dk = code_offset(m)
        p = np.nonzero(cross[:, m])[0]
        q = p + (di * ny + dj) * nz + dk
        with np.errstate(all="ignore"):
            d = (sf[q] - sf[p]).astype(np.float32)
            num = (iso - sf[p]).astype(np.float32)
            u = (num / d).astype(np.float32)
            u[~((u >= 0) & (u <= 1))] = F(0.5)
            e = (xf[q] - xf[p]).astype(np.float32)
            ue = (u[:, None] * e).astype(np.float32)
            vertices[vid[p, m]] = (xf[p] + ue).astype(np.float32)
        edge_p[vid[p, m]], edge_q[vid[p, m]] = p, q
    # triangles, cell by cell in order of the min corner, then tetrahedron, then table order
    cells = lin[:nx - 1, :ny - 1, :nz - 1].reshape(-1)
    ci = inside.reshape(n)
    keys, tris = [], []
    for t in range(6):
        codes = tet_corners(t)
        offs = [(c & 1) * ny * nz + ((c >> 1) & 1) * nz + ((c >> 2) & 1) for c in codes]
        mask = sum(ci[cells + offs[i]].astype(np.int64) << i for i in range(4))
        for mk in range(1, 15):
            sel = cells[mask == mk]
            if not len(sel):
                continue
            for w, tri in enumerate(tet_triangles(t, mk)):
                ids = []
                for a, b in tri:
                    lo, hi = min(a, b), max(a, b)
                    ids.append(vid[sel + offs[lo], codes[lo] ^ codes[hi]])
                    assert np.all(cross[sel + offs[lo], codes[lo] ^ codes[hi]])
                tris.append(np.stack(ids, axis=1))
                keys.append(np.stack([sel, np.full(len(sel), t), np.full(len(sel), w)], axis=1))
    if tris:
        tris, keys = np.concatenate(tris), np.concatenate(keys)
        order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        triangles = tris[order].astype(np.uint32)
    else:
        triangles = np.zeros((0, 3), np.uint32)
    return Mesh(vertices, triangles, edge_p, edge_q, inside)


# ---------------------------------------------------------------- property checkers (nothing above is used below)
def check_closed_and_oriented(triangles):
    """every directed edge (a, b) of the triangles occurs exactly once, and (b, a) exactly once"""
    t = np.asarray(triangles, np.uint64).reshape(-1, 3)
    if not len(t):
        return
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    big = np.uint64(1 << 32)
    fwd, rev = np.sort(a * big + b), np.sort(b * big + a)
    assert np.all(fwd[1:] != fwd[:-1]), "a directed edge occurs twice"
    assert np.array_equal(fwd, rev), "a directed edge has no opposite"


def check_indices(triangles, n_vertices):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    assert np.all(t < n_vertices) and np.all(t >= 0)
    assert np.all(t[:, 0] != t[:, 1]) and np.all(t[:, 1] != t[:, 2]) and np.all(t[:, 0] != t[:, 2])
    used = np.zeros(n_vertices, bool)
    used[t.reshape(-1)] = True
    assert used.all(), "a vertex is not referenced"


def check_placement(vertices, xp, xq):
    """every vertex lies within the bounding box of its edge (xp, xq: the positions of the edge's two lattice points)"""
    v, xp, xq = (np.asarray(a, np.float64).reshape(-1, 3) for a in (vertices, xp, xq))
    assert np.all(v >= np.minimum(xp, xq)) and np.all(v <= np.maximum(xp, xq))


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return float(np.sum(np.sum(a * np.cross(b, c), axis=1)) / 6.0)


def check_volume(vertices, triangles, inside, cell):
    """V_full <= V <= V_full + V_mixed: the surface lies inside the cells with some but not all corners inside"""
    ins = np.asarray(inside, bool)
    corners = sum(ins[di:ins.shape[0] - 1 + di, dj:ins.shape[1] - 1 + dj, dk:ins.shape[2] - 1 + dk].astype(np.int64)
                  for di in (0, 1) for dj in (0, 1) for dk in (0, 1))
    vol = float(np.prod(np.asarray(cell, np.float32).astype(np.float64)))
    v_full, v_mixed = vol * int(np.sum(corners == 8)), vol * int(np.sum((corners > 0) & (corners < 8)))
    V = signed_volume(vertices, triangles)
    tol = 1e-6 * abs(V)
    assert v_full - tol <= V <= v_full + v_mixed + tol, (v_full, V, v_full + v_mixed)
    return V, v_full, v_mixed


def check_all(m, origin, cell, dims):
    """all four on a Mesh of mesh() or on the GPU's arrays wrapped in one; returns the volume"""
    x = np.stack(np.meshgrid(*[np.float32(origin[c]) + (np.arange(dims[c]).astype(np.float32) * np.float32(cell[c])).astype(np.float32)
                               for c in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    check_closed_and_oriented(m.triangles)
    check_indices(m.triangles, len(m.vertices))
    check_placement(m.vertices, x[m.edge_p], x[m.edge_q])
    return check_volume(m.vertices, m.triangles, m.inside, cell)[0]
