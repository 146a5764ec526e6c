// Sanitizer driver of csrc/nrf_bake_plan.h (make bake_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the definition of
// the mesh texture (nrf_bake_mesh_texture) -- the atlas layout, the ownership of every texel, its position in its triangle's plane, the
// head-on direction, the guard and the UVs -- compiled from the text the kernels compile.  One case on stdin:
//     res width (decimal)  bound (fp32 bit pattern, hexadecimal)  n_vertices n_triangles (decimal)
//     n_vertices rows of three fp32 bit patterns (hexadecimal)    n_triangles rows of three indices (decimal)
// and on stdout:
//     layout 0 W           the parameters are out of range or the atlas is beyond the limits; W = the smallest width that fits, or 0
//     layout 1 height cols n_pairs
//     t px py tri i j guard x[3] d[3]     one line per texel of an EXISTING triangle (tri < n_triangles), in work-item order: the atlas
//                                         texel, the owner and (i, j) there, whether it is evaluated, and the bits of the position
//                                         and of the direction (zeros where the triangle names a vertex >= n_vertices)
//     u tri u_a v_a u_b v_b u_c v_c       the bits of the UVs, one line per triangle
// tests/test_mesh_texture_cpu.py holds the output to the numpy replay the GPU tests use (tests/bake_replay.py).  Built with
// -ffp-contract=off, as the library is: every operation is one fp32 rounding.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/nrf_bake_plan.h"

static float as_float(uint32_t u) {
  float f;
  std::memcpy(&f, &u, sizeof f);
  return f;
}
static uint32_t as_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}

int main() {
  uint32_t res, width, bound_bits, nv, nt;
  if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNx32 " %" SCNu32 " %" SCNu32, &res, &width, &bound_bits, &nv, &nt) != 5) {
    std::fprintf(stderr, "bake_plan_check: no header\n");
    return 2;
  }
  if (nv > (1u << 20) || nt > (1u << 20)) {
    std::fprintf(stderr, "bake_plan_check: more than 2^20 vertices or triangles\n");
    return 2;
  }
  std::vector<float> v(3 * (size_t)nv);
  std::vector<uint32_t> tri(3 * (size_t)nt);
  for (float& f : v) {
    uint32_t u;
    if (std::scanf("%" SCNx32, &u) != 1) return 2;
    f = as_float(u);
  }
  for (uint32_t& i : tri)
    if (std::scanf("%" SCNu32, &i) != 1) return 2;
  const float bound = as_float(bound_bits);
  nrf::BakeLayout B;
  if (!nrf::bake_layout(nt, res, width, B)) {
    std::printf("layout 0 %" PRIu32 "\n", nrf::bake_smallest_width(nt, res));
    return 0;
  }
  std::printf("layout 1 %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", B.height, B.cols, B.n_pairs);
  const uint32_t n = nrf::bake_work_items(B);
  long owned = 0, refused = 0;
  for (uint32_t w = 0; w < n; ++w) {
    const nrf::BakeTexel T = nrf::bake_texel(B, w);
    if (T.tri >= nt) continue;
    float x[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    bool ok = false;
    if (nrf::bake_triangle_ok(T.tri, nt, tri.data(), nv)) {
      float p[3][3];
      for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 3; ++k) p[c][k] = v[3 * (size_t)tri[3 * (size_t)T.tri + c] + k];
      nrf::bake_position(p[0], p[1], p[2], T.i, T.j, res, x);
      ok = nrf::bake_position_ok(x, bound);
      nrf::bake_direction(p[0], p[1], p[2], d);
    }
    ++owned;
    refused += !ok;
    std::printf("t %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %d %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32
                " %08" PRIx32 "\n",
                T.px, T.py, T.tri, T.i, T.j, (int)ok, as_bits(x[0]), as_bits(x[1]), as_bits(x[2]), as_bits(d[0]), as_bits(d[1]), as_bits(d[2]));
  }
  for (uint32_t t = 0; t < nt; ++t) {
    float uv[6];
    nrf::bake_uv(B, t, uv);
    std::printf("u %" PRIu32, t);
    for (float f : uv) std::printf(" %08" PRIx32, as_bits(f));
    std::printf("\n");
  }
  std::fprintf(stderr, "bake_plan_check: %ld owned texels, %ld refused\n", owned, refused);
  return 0;
}
