"""The definition of nrf_bake_mesh_texture (include/nerfhip.h) replayed in numpy -- TEST INFRASTRUCTURE ONLY.

The atlas layout, the ownership of every texel, its position in its triangle's plane, the head-on viewing direction of a triangle, the
guard, the packed 8-bit texel and the UVs.  Integers are exact; every numpy operation on float32 arrays is one fp32 rounding and
numpy's float32 division and sqrt are the correctly rounded IEEE ones, which is what the library's build (-ffp-contract=off
-fno-fast-math) makes of csrc/nrf_bake_plan.h.  tests/test_mesh_texture_cpu.py holds this module to that header bit for bit through
host/bake_plan_check.cpp, and the GPU tests hold the kernels to this module.  The unit vector and the 8-bit rule are attr_replay's.
It shares no code with the header."""
from __future__ import annotations

import numpy as np

import attr_replay as ar

F = np.float32
RES_MIN, RES_MAX = 2, 256
WIDTH_MAX = HEIGHT_MAX = 16384
TEXELS_MAX = 1 << 26


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def bits(a):
    return f32(a).view(np.uint32)


def params_valid(res, width):
    return RES_MIN <= res <= RES_MAX and res + 2 <= width <= WIDTH_MAX


def height_of(n_triangles, res, width):
    """rows (r + 1), without the limits"""
    cols = width // (res + 2)
    pairs = (n_triangles + 1) // 2
    return -(-pairs // cols) * (res + 1)


def fits(width, height):
    return height <= HEIGHT_MAX and width * height <= TEXELS_MAX


def layout(n_triangles, res, width):
    """(height, cols, n_pairs), or None where the call is refused"""
    if not params_valid(res, width):
        return None
    h = height_of(n_triangles, res, width)
    if not fits(width, h):
        return None
    return h, width // (res + 2), (n_triangles + 1) // 2


def smallest_width(n_triangles, res):
    """the smallest legal width whose atlas holds n_triangles, or 0"""
    if not RES_MIN <= res <= RES_MAX:
        return 0
    for width in range(res + 2, WIDTH_MAX + 1):
        if fits(width, height_of(n_triangles, res, width)):
            return width
    return 0


def cell_texels(n_triangles, res, width):
    """every texel of every pair's cell, in work-item order (pair, then j', then i'): dict of int64 arrays pair, ic, jc, tri, i, j, px,
    py, and exists (tri < n_triangles)"""
    h, cols, pairs = layout(n_triangles, res, width)
    r = res
    w = np.arange(pairs * (r + 2) * (r + 1), dtype=np.int64)
    pair, rem = np.divmod(w, (r + 2) * (r + 1))
    jc, ic = np.divmod(rem, r + 2)
    even = ic + jc <= r
    tri = 2 * pair + np.where(even, 0, 1)
    i = np.where(even, ic, r + 1 - ic)
    j = np.where(even, jc, r - jc)
    px = (pair % cols) * (r + 2) + ic
    py = (pair // cols) * (r + 1) + jc
    return dict(pair=pair, ic=ic, jc=jc, tri=tri, i=i, j=j, px=px, py=py, exists=tri < n_triangles)


def owner_map(n_triangles, res, width):
    """int64 [height][width]: the triangle that owns each atlas texel, -1 where none does; and how often each texel was claimed"""
    h, cols, pairs = layout(n_triangles, res, width)
    c = cell_texels(n_triangles, res, width)
    owner = np.full((h, width), -1, np.int64)
    claims = np.zeros((h, width), np.int64)
    e = c["exists"]
    np.add.at(claims, (c["py"][e], c["px"][e]), 1)
    owner[c["py"][e], c["px"][e]] = c["tri"][e]
    return owner, claims


def position(va, vb, vc, i, j, res):
    """x_k = (va_k + s e1_k) + t e2_k with s = i / (r - 1), t = j / (r - 1): products rounded, then the sums, in this order"""
    va, vb, vc = f32(va), f32(vb), f32(vc)
    den = F(res - 1)
    with np.errstate(all="ignore"):
        s = (np.asarray(i).astype(np.float32) / den).astype(np.float32)[:, None]
        t = (np.asarray(j).astype(np.float32) / den).astype(np.float32)[:, None]
        e1 = (vb - va).astype(np.float32)
        e2 = (vc - va).astype(np.float32)
        p1 = (s * e1).astype(np.float32)
        p2 = (t * e2).astype(np.float32)
        a = (va + p1).astype(np.float32)
        return (a + p2).astype(np.float32)


def face_normal(va, vb, vc):
    """n = e1 x e2: per component two rounded products and one rounded difference"""
    va, vb, vc = f32(va), f32(vb), f32(vc)
    with np.errstate(all="ignore"):
        e1 = (vb - va).astype(np.float32)
        e2 = (vc - va).astype(np.float32)
        n = np.empty_like(e1)
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            n[:, k] = ((e1[:, a] * e2[:, b]).astype(np.float32) - (e1[:, b] * e2[:, a]).astype(np.float32)).astype(np.float32)
    return n


def face_direction(va, vb, vc):
    """(d [n][3], ok [n]): the unit direction of -n as the point attributes form one from a gradient; degenerate: zeros"""
    _, _, d, ok = ar.direction(-face_normal(va, vb, vc))
    return d, ok


def in_box(x, bound):
    with np.errstate(all="ignore"):
        return np.all(np.abs(f32(x)) <= F(bound), axis=-1)


def uvs(n_triangles, res, width):
    """float32 [n_triangles][3][2]"""
    h, cols, pairs = layout(n_triangles, res, width)
    r = res
    t = np.arange(n_triangles, dtype=np.int64)
    q = t >> 1
    x0, y0 = (q % cols) * (r + 2), (q // cols) * (r + 1)
    odd = (t & 1) == 1
    px = np.stack([np.where(odd, x0 + r + 1, x0), np.where(odd, x0 + 2, x0 + r - 1), np.where(odd, x0 + r + 1, x0)], axis=1)
    py = np.stack([np.where(odd, y0 + r, y0), np.where(odd, y0 + r, y0), np.where(odd, y0 + 1, y0 + r - 1)], axis=1)
    with np.errstate(all="ignore"):
        u = ((px.astype(np.float32) + F(0.5)).astype(np.float32) / F(width)).astype(np.float32)
        v = ((py.astype(np.float32) + F(0.5)).astype(np.float32) / F(h)).astype(np.float32) if n_triangles else u
    return np.stack([u, v], axis=2).astype(np.float32), np.stack([px, py], axis=2)


def bake(vertices, triangles, res, width, bound):
    """The whole definition but for the network.  Returns a dict: height, cols; per texel of an EXISTING triangle, in work-item order:
    px, py, tri, i, j, guard (evaluated or not), x [n][3], d [n][3] (zeros where the triangle names a vertex >= n_vertices); uvs; and
    n_refused = the number of those texels with guard false"""
    v = f32(vertices).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3).astype(np.int64)
    nv, nt = len(v), len(t)
    h, cols, pairs = layout(nt, res, width)
    c = cell_texels(nt, res, width)
    e = c["exists"]
    tri, i, j = c["tri"][e], c["i"][e], c["j"][e]
    named_ok = np.all(t < nv, axis=1) if nt else np.zeros(0, bool)
    vs = np.concatenate([v, np.zeros((1, 3), np.float32)])  # (a stand-in row for the indices that are refused anyway)
    safe = np.where(named_ok[:, None], t, nv)
    va, vb, vc = vs[safe[:, 0]], vs[safe[:, 1]], vs[safe[:, 2]]
    d_tri, _ = face_direction(va, vb, vc) if nt else (np.zeros((0, 3), np.float32), None)
    x = position(va[tri], vb[tri], vc[tri], i, j, res) if len(tri) else np.zeros((0, 3), np.float32)
    tri_ok = named_ok[tri] if len(tri) else np.zeros(0, bool)
    x = np.where(tri_ok[:, None], x, F(0)).astype(np.float32)
    d = np.where(tri_ok[:, None], d_tri[tri], F(0)).astype(np.float32) if len(tri) else np.zeros((0, 3), np.float32)
    guard = tri_ok & in_box(x, bound)
    uv, corners = uvs(nt, res, width)
    return dict(height=h, cols=cols, px=c["px"][e], py=c["py"][e], tri=tri, i=i, j=j, guard=guard, x=x, d=d, uvs=uv, corners=corners,
                n_refused=int((~guard).sum()))


def rgba8(rgb):
    """u8(r) | u8(g) << 8 | u8(b) << 16 | 255 << 24"""
    c = ar.color_u8(f32(rgb).reshape(-1, 3)).astype(np.uint32)
    return (c[:, 0] | c[:, 1] << np.uint32(8) | c[:, 2] << np.uint32(16) | np.uint32(255) << np.uint32(24)).astype(np.uint32)
