"""The definition of nrf_refine_mesh in vectorised numpy -- TEST INFRASTRUCTURE ONLY -- written from the comment at the head of
csrc/nrf_refine_plan.h, and a property checker of a refinement that shares no code with it.

Every numpy operation on float32 arrays is one fp32 rounding, which is what the library's build (-ffp-contract=off -fno-fast-math)
makes of the header; tests/test_mesh_refine_cpu.py holds this module to the header bit for bit through host/refine_plan_check.cpp,
and the GPU tests hold the kernel to this module.  The density is a callable `density(x [n][3] fp32) -> sigma [n] fp32` that has
nrf_density's guard in it (0 where a coordinate is outside the box or not finite): nrf_density itself on the GPU, an analytic field
on the CPU."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import mesh_replay as mr

F = np.float32
MAX_STEPS = 16

# asked [n_steps + 2][n][3]: the positions the definition asks the density for, in order; answers [n_steps + 2][n]: what it said
Refined = namedtuple("Refined", "vertices brackets bracketed asked answers")


def edge_words(m, dims):
    """the edge word (p << 3) | m of every vertex of a mesh_replay.Mesh, from its edge_p / edge_q"""
    ny, nz = int(dims[1]), int(dims[2])
    d = np.asarray(m.edge_q, np.int64) - np.asarray(m.edge_p, np.int64)
    code = np.zeros(len(d), np.int64)
    for c in range(1, 8):
        di, dj, dk = mr.code_offset(c)
        code[d == (di * ny + dj) * nz + dk] = c
    assert np.all(code > 0)
    return ((np.asarray(m.edge_p, np.int64) << 3) | code).astype(np.uint32)


def edge_positions(origin, cell, dims, words):
    """(xp, xq) [n][3] fp32 each: the positions of the two lattice points of every edge word"""
    nx, ny, nz = (int(d) for d in dims)
    w = np.asarray(words, np.uint32).astype(np.int64)
    p, m = w >> 3, w & 7
    assert np.all(m > 0) and np.all(p < nx * ny * nz)
    k, ij = p % nz, p // nz
    j, i = ij % ny, ij // ny
    x = mr.positions(origin, cell, (nx, ny, nz))
    qi, qj, qk = i + (m & 1), j + ((m >> 1) & 1), k + ((m >> 2) & 1)
    assert np.all(qi < nx) and np.all(qj < ny) and np.all(qk < nz)
    return x[i, j, k], x[qi, qj, qk]


def point(xp, xq, u):
    with np.errstate(all="ignore"):
        e = (xq - xp).astype(np.float32)
        ue = (f32(u)[:, None] * e).astype(np.float32)
        return (xp + ue).astype(np.float32)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def refine(origin, cell, dims, iso, words, vertices, n_steps, density):
    """nrf_refine_mesh on the vertices [n][3] with those edge words"""
    assert 0 <= n_steps <= MAX_STEPS
    iso = F(iso)
    xp, xq = edge_positions(origin, cell, dims, words)
    n = len(xp)
    asked, answers = [xp, xq], [f32(density(xp)).reshape(n), f32(density(xq)).reshape(n)]
    s0, s1 = answers
    with np.errstate(all="ignore"):
        in0 = s0 >= iso
        bracketed = in0 != (s1 >= iso)
    lo, hi = np.zeros(n, np.float32), np.ones(n, np.float32)
    slo, shi = s0.copy(), s1.copy()
    for _ in range(n_steps):
        um = (F(0.5) * (lo + hi).astype(np.float32)).astype(np.float32)
        x = point(xp, xq, um)
        sm = f32(density(x)).reshape(n)
        asked.append(x)
        answers.append(sm)
        with np.errstate(all="ignore"):
            same = (sm >= iso) == in0
        low, high = bracketed & same, bracketed & ~same
        lo[low], slo[low] = um[low], sm[low]
        hi[high], shi[high] = um[high], sm[high]
    with np.errstate(all="ignore"):
        d = (shi - slo).astype(np.float32)
        num = (iso - slo).astype(np.float32)
        r = (num / d).astype(np.float32)
        r[~((r >= 0) & (r <= 1))] = F(0.5)
        w = (hi - lo).astype(np.float32)
        u = (lo + (r * w).astype(np.float32)).astype(np.float32)
    out = f32(vertices).reshape(n, 3).copy()
    out[bracketed] = point(xp, xq, u)[bracketed]
    return Refined(out, np.stack([lo, hi, slo, shi], axis=1), bracketed, np.stack(asked) if n else np.zeros((n_steps + 2, 0, 3), np.float32),
                   np.stack(answers) if n else np.zeros((n_steps + 2, 0), np.float32))


# ---------------------------------------------------------------- the property checker (nothing above is used below)
def check_refinement(vertices, brackets, origin, cell, dims, iso, words, n_steps, bracketed=None):
    """what a refinement has to be whatever the code says: for every bracketed vertex hi - lo == 2^-n_steps, 0 <= lo < hi <= 1, s_lo
    and s_hi on different sides of iso, and the vertex within the bounding box of its edge.  bracketed None: all of them have to be."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    b = np.asarray(brackets, np.float32).reshape(-1, 4).astype(np.float64)
    w = np.asarray(words, np.uint32).astype(np.int64)
    assert len(v) == len(b) == len(w)
    on_lo, on_hi = np.asarray(brackets, np.float32).reshape(-1, 4)[:, 2] >= np.float32(iso), np.asarray(brackets, np.float32).reshape(-1, 4)[:, 3] >= np.float32(iso)
    if bracketed is None:
        bracketed = np.ones(len(v), bool)
    k = np.asarray(bracketed, bool)
    assert np.array_equal(on_lo != on_hi, k), "a bracket does not straddle iso, or an unbracketed edge does"
    assert np.all(b[k, 1] - b[k, 0] == 2.0 ** -n_steps), "hi - lo is not 2^-n_steps"
    assert np.all(b[k, 0] >= 0) and np.all(b[k, 0] < b[k, 1]) and np.all(b[k, 1] <= 1)
    assert np.all(b[~k, 0] == 0) and np.all(b[~k, 1] == 1)
    axes = [np.float32(origin[c]) + (np.arange(dims[c]).astype(np.float32) * np.float32(cell[c])).astype(np.float32) for c in range(3)]
    p, m = w >> 3, w & 7
    idx = [p // (int(dims[1]) * int(dims[2])), (p // int(dims[2])) % int(dims[1]), p % int(dims[2])]
    xp = np.stack([axes[c][idx[c]] for c in range(3)], axis=1)
    xq = np.stack([axes[c][idx[c] + ((m >> c) & 1)] for c in range(3)], axis=1)
    mr.check_placement(v[k], xp[k], xq[k])
