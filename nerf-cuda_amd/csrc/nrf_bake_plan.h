// nrf_bake_plan.h -- the definition of the mesh texture (nrf_bake_mesh_texture) without a device: the atlas layout, which triangle owns
// which texel, where a texel lies in its triangle's plane, the head-on viewing direction of a triangle, the guard, the packed 8-bit
// texel and the UVs.  bake_kernel / bake_uv_kernel (nrf_kernels_bake.hip), nrf_mesh_texture_size (nrf_api.hip) and
// host/bake_plan_check.cpp compile this text, so the kernel's definition and the tests' replay are one.  All integer arithmetic is
// exact.  Every fp32 operation is ONE rounding, the division and the square root the correctly rounded IEEE ones: the library is built
// with -ffp-contract=off -fno-fast-math, and a host build of this header has to be (host/Makefile: bake_asan).
//
// Parameters: res = r texels along a triangle's legs, 2 <= r <= 256; width = the atlas width in texels, r + 2 <= width <= 16384.
// Cells: triangles are paired, pair q = t >> 1 owns a cell of (r + 2) x (r + 1) texels; cols = width / (r + 2), rows = ceil(n_pairs /
// cols), height = rows (r + 1); pair q's cell origin is (x0, y0) = ((q % cols)(r + 2), (q / cols)(r + 1)).  height <= 16384 and
// width * height <= 2^26; an empty mesh has height 0.
//
//      j'                                     a cell at r = 4: E = the even triangle 2q, O = the odd triangle 2q + 1
//      4  E O O O O O                         E's corners a, b, c sit at (0, 0), (r - 1, 0), (0, r - 1); the texels with i + j = r and
//      3  E E O O O O                         (r, 0), (0, r) lie one step outside its hypotenuse and are evaluated at the extrapolated
//      2  E E E O O O                         position in the triangle's plane, so a bilinear fetch anywhere inside the triangle reads
//      1  E E E E O O                         texels of the same triangle only.  O is E turned by half a turn: (i, j) = (r + 1 - i',
//      0  E E E E E O                         r - j'), its corners a, b, c at (r + 1, r), (2, r), (r + 1, 1)
//         0 1 2 3 4 5  i'
#pragma once
#include <cstdint>

#include "nrf_attr_plan.h"

namespace nrf {

constexpr uint32_t BAKE_RES_MIN = 2, BAKE_RES_MAX = 256;
constexpr uint32_t BAKE_WIDTH_MAX = 16384, BAKE_HEIGHT_MAX = 16384;
constexpr uint64_t BAKE_TEXELS_MAX = 1ull << 26;

NRF_POINTS_HD inline bool bake_params_valid(uint32_t res, uint32_t width) {
  return res >= BAKE_RES_MIN && res <= BAKE_RES_MAX && width >= res + 2u && width <= BAKE_WIDTH_MAX;
}
NRF_POINTS_HD inline uint32_t bake_cell_width(uint32_t res) { return res + 2u; }
NRF_POINTS_HD inline uint32_t bake_cell_height(uint32_t res) { return res + 1u; }
NRF_POINTS_HD inline uint32_t bake_cell_texels(uint32_t res) { return (res + 2u) * (res + 1u); }    // <= 258 * 257
NRF_POINTS_HD inline uint32_t bake_half_texels(uint32_t res) { return (res + 2u) * (res + 1u) / 2u; }  // what one triangle owns
NRF_POINTS_HD inline uint64_t bake_pairs(uint64_t n_triangles) { return (n_triangles + 1u) >> 1; }
NRF_POINTS_HD inline uint32_t bake_cols(uint32_t res, uint32_t width) { return width / (res + 2u); }
// rows (res + 1) in 64 bits: the caller compares it with the limits before it becomes a 32-bit height
NRF_POINTS_HD inline uint64_t bake_height64(uint64_t n_triangles, uint32_t res, uint32_t width) {
  const uint64_t cols = bake_cols(res, width);
  const uint64_t rows = (bake_pairs(n_triangles) + cols - 1u) / cols;
  return rows * (res + 1u);
}
NRF_POINTS_HD inline bool bake_atlas_fits(uint32_t width, uint64_t height64) {
  return height64 <= BAKE_HEIGHT_MAX && (uint64_t)width * height64 <= BAKE_TEXELS_MAX;
}
// the smallest legal width whose atlas holds n_triangles at this res, or 0 when none does (host side: at most 8192 steps).  A width
// between two multiples of r + 2 has the columns of the smaller one and only a wider margin, so multiples are all there is to try.
inline uint32_t bake_smallest_width(uint64_t n_triangles, uint32_t res) {
  if (res < BAKE_RES_MIN || res > BAKE_RES_MAX) return 0;
  for (uint32_t width = res + 2u; width <= BAKE_WIDTH_MAX; width += res + 2u)
    if (bake_atlas_fits(width, bake_height64(n_triangles, res, width))) return width;
  return 0;
}

// What the kernels need of a layout
struct BakeLayout {
  uint32_t res = 0, width = 0, height = 0, cols = 0;
  uint32_t n_triangles = 0, n_pairs = 0;
};
// the number of work items: every texel of every pair's cell.  <= width * height <= 2^26
NRF_POINTS_HD inline uint32_t bake_work_items(const BakeLayout& B) { return B.n_pairs * bake_cell_texels(B.res); }

// Work item w -> the pair, the cell texel (i', j'), the owner triangle and its (i, j)
struct BakeTexel {
  uint32_t pair, ic, jc;  // the cell texel (i', j')
  uint32_t tri, i, j;     // the owner and the texel's coordinates in the owner's frame
  uint32_t px, py;        // the atlas texel
};
NRF_POINTS_HD inline BakeTexel bake_texel(const BakeLayout& B, uint32_t w) {
  const uint32_t r = B.res, cw = r + 2u, ct = bake_cell_texels(r);
  BakeTexel T;
  T.pair = w / ct;
  const uint32_t rem = w - T.pair * ct;
  T.jc = rem / cw;
  T.ic = rem - T.jc * cw;
  const bool even = T.ic + T.jc <= r;
  T.tri = 2u * T.pair + (even ? 0u : 1u);
  T.i = even ? T.ic : r + 1u - T.ic;
  T.j = even ? T.jc : r - T.jc;
  T.px = (T.pair % B.cols) * cw + T.ic;
  T.py = (T.pair / B.cols) * (r + 1u) + T.jc;
  return T;
}

// The position of texel (i, j) of the triangle (va, vb, vc): s = i / (r - 1), t = j / (r - 1), x_k = (va_k + s e1_k) + t e2_k with
// e1 = vb - va, e2 = vc - va: the products are rounded, then the sums, in this order
NRF_POINTS_HD inline void bake_position(const float (&va)[3], const float (&vb)[3], const float (&vc)[3], uint32_t i, uint32_t j, uint32_t res,
                                        float (&x)[3]) {
  const float den = (float)(res - 1u);
  const float s = (float)i / den;
  const float t = (float)j / den;
  for (int k = 0; k < 3; ++k) {
    const float e1 = vb[k] - va[k];
    const float e2 = vc[k] - va[k];
    const float p1 = s * e1;
    const float p2 = t * e2;
    const float a = va[k] + p1;
    x[k] = a + p2;
  }
}

// The face normal n = e1 x e2 (outward by the extraction's orientation rule): per component two rounded products and one rounded
// difference; and the head-on viewing direction d = attr_direction(-n): the negations are exact.  A degenerate triangle
// (attr_length2_ok false) has d = (0, 0, 0).  Returns whether the triangle has a direction.
NRF_POINTS_HD inline void bake_normal(const float (&va)[3], const float (&vb)[3], const float (&vc)[3], float (&n)[3]) {
  const float e1x = vb[0] - va[0], e1y = vb[1] - va[1], e1z = vb[2] - va[2];
  const float e2x = vc[0] - va[0], e2y = vc[1] - va[1], e2z = vc[2] - va[2];
  const float yz = e1y * e2z, zy = e1z * e2y;
  const float zx = e1z * e2x, xz = e1x * e2z;
  const float xy = e1x * e2y, yx = e1y * e2x;
  n[0] = yz - zy;
  n[1] = zx - xz;
  n[2] = xy - yx;
}
NRF_POINTS_HD inline bool bake_direction(const float (&va)[3], const float (&vb)[3], const float (&vc)[3], float (&d)[3]) {
  float n[3], nrm[3], len;
  bake_normal(va, vb, vc, n);
  return attr_direction(-n[0], -n[1], -n[2], d, nrm, len);
}

// The guard.  A texel is evaluated if and only if its triangle exists, names vertices of the mesh only and every coordinate of the
// texel's position is finite and within [-bound, bound] (nrf_density's one-tap guard).  bake_triangle_ok is the half that is decided
// BEFORE a vertex is read: an index is the one thing here that becomes an address ahead of the network.
NRF_POINTS_HD inline bool bake_triangle_ok(uint32_t tri, uint32_t n_triangles, const uint32_t* triangles, uint32_t n_vertices) {
  if (tri >= n_triangles) return false;
  return triangles[3u * (uint64_t)tri] < n_vertices && triangles[3u * (uint64_t)tri + 1u] < n_vertices &&
         triangles[3u * (uint64_t)tri + 2u] < n_vertices;
}
NRF_POINTS_HD inline bool bake_position_ok(const float (&x)[3], float bound) { return points_guard(x, 0.0f, bound, 1); }

// The packed texel: the library's 8-bit rule per channel, alpha 255 = covered
NRF_POINTS_HD inline uint32_t bake_rgba8(float r, float g, float b) {
  return (uint32_t)attr_color_u8(r) | (uint32_t)attr_color_u8(g) << 8 | (uint32_t)attr_color_u8(b) << 16 | 255u << 24;
}

// The UVs of triangle tri's corners a, b, c: the atlas texel (px, py) of a corner has u = (px + 0.5) / width, v = (py + 0.5) / height
// (the sum is exact, the division rounded).  Even: (x0, y0), (x0 + r - 1, y0), (x0, y0 + r - 1); odd: (x0 + r + 1, y0 + r),
// (x0 + 2, y0 + r), (x0 + r + 1, y0 + 1).  uv = (u_a, v_a, u_b, v_b, u_c, v_c).
NRF_POINTS_HD inline void bake_corner_texels(const BakeLayout& B, uint32_t tri, uint32_t (&p)[6]) {
  const uint32_t r = B.res, q = tri >> 1;
  const uint32_t x0 = (q % B.cols) * (r + 2u), y0 = (q / B.cols) * (r + 1u);
  if (!(tri & 1u)) {
    p[0] = x0, p[1] = y0;
    p[2] = x0 + r - 1u, p[3] = y0;
    p[4] = x0, p[5] = y0 + r - 1u;
  } else {
    p[0] = x0 + r + 1u, p[1] = y0 + r;
    p[2] = x0 + 2u, p[3] = y0 + r;
    p[4] = x0 + r + 1u, p[5] = y0 + 1u;
  }
}
NRF_POINTS_HD inline void bake_uv(const BakeLayout& B, uint32_t tri, float (&uv)[6]) {
  uint32_t p[6];
  bake_corner_texels(B, tri, p);
  const float fw = (float)B.width, fh = (float)B.height;
  for (int c = 0; c < 3; ++c) {
    const float cx = (float)p[2 * c] + 0.5f;
    const float cy = (float)p[2 * c + 1] + 0.5f;
    uv[2 * c] = cx / fw;
    uv[2 * c + 1] = cy / fh;
  }
}

// ---- the host's side ----
// The layout of n_triangles at (res, width).  Returns false when the parameters are out of range or the atlas is beyond the limits.
inline bool bake_layout(uint64_t n_triangles, uint32_t res, uint32_t width, BakeLayout& B) {
  if (!bake_params_valid(res, width)) return false;
  const uint64_t h = bake_height64(n_triangles, res, width);
  if (!bake_atlas_fits(width, h)) return false;
  B.res = res;
  B.width = width;
  B.height = (uint32_t)h;
  B.cols = bake_cols(res, width);
  B.n_triangles = (uint32_t)n_triangles;  // (height <= 16384 bounds the pairs far below 2^32)
  B.n_pairs = (uint32_t)bake_pairs(n_triangles);
  return true;
}
inline uint64_t bake_texel_bytes(const BakeLayout& B) { return (uint64_t)B.width * B.height * 16u; }
inline uint64_t bake_rgba8_bytes(const BakeLayout& B) { return (uint64_t)B.width * B.height * 4u; }
inline uint64_t bake_uv_bytes(uint64_t n_triangles) { return n_triangles * 24u; }

}  // namespace nrf
