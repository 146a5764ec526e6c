// Sanitizer driver of csrc/nrf_simplify_plan.h (make simplify_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the clusters,
// the keys, the representatives and the remap of nrf_simplify_mesh on the CPU, compiled from the text the kernels compile.  Problems on
// stdin, any number of them; floats as the 8 hex digits of their bits, everything else decimal:
//     ox oy oz  cx cy cz  nx ny nz  factor n_vertices n_triangles
//     word x y z          (n_vertices lines: the edge word and the position's bits)
//     a b c               (n_triangles index triples)
// and per problem on stdout
//     simplified <kept vertices> <kept triangles> <n_vertices> <n_triangles> <ok> <factor valid>
//     r <cluster> <key, 16 hex digits> <rep>     one line per vertex of the problem: its own cluster and key, and its representative
//     o <old id> <word> <x> <y> <z>              one line per kept vertex: sources, the carried edge word and the carried bits
//     m <entry>                                  one line per vertex of the problem: vertex_map
//     t <a> <b> <c>                              one line per kept triangle, remapped
// A problem with a factor outside 1 .. 256 prints "simplified 0 0 <n_vertices> <n_triangles> 0 0" alone.
// tests/test_mesh_simplify_cpu.py holds the output to the numpy replay the GPU tests use (tests/simplify_replay.py).
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../csrc/nrf_simplify_plan.h"

int main() {
  long problems = 0;
  for (;;) {
    uint32_t bits[6], dims[3], factor, nv, nt;
    const int got = std::scanf("%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32
                               " %" SCNu32 " %" SCNu32,
                               &bits[0], &bits[1], &bits[2], &bits[3], &bits[4], &bits[5], &dims[0], &dims[1], &dims[2], &factor, &nv, &nt);
    if (got == EOF || got == 0) break;
    if (got != 12) {
      std::fprintf(stderr, "simplify_plan_check: problem %ld has a short header\n", problems);
      return 2;
    }
    nrf::MeshLattice L;
    __builtin_memcpy(L.origin, bits, 12);
    __builtin_memcpy(L.cell, bits + 3, 12);
    for (int c = 0; c < 3; ++c) L.dims[c] = dims[c];
    if (!nrf::mesh_lattice_valid(L.origin, L.cell, L.dims) || nv > (1u << 24) || nt > (1u << 24)) {
      std::fprintf(stderr, "simplify_plan_check: problem %ld: a lattice the entry points refuse, or more than 2^24 vertices or triangles\n", problems);
      return 2;
    }
    std::vector<uint32_t> edges(nv), vertices(3 * (size_t)nv), triangles(3 * (size_t)nt);
    for (size_t v = 0; v < nv; ++v)
      if (std::scanf("%" SCNu32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &edges[v], &vertices[3 * v], &vertices[3 * v + 1], &vertices[3 * v + 2]) != 4) {
        std::fprintf(stderr, "simplify_plan_check: problem %ld has %zu of %" PRIu32 " vertices\n", problems, v, nv);
        return 2;
      }
    for (size_t i = 0; i < triangles.size(); ++i)
      if (std::scanf("%" SCNu32, &triangles[i]) != 1) {
        std::fprintf(stderr, "simplify_plan_check: problem %ld has %zu of %zu indices\n", problems, i, triangles.size());
        return 2;
      }
    if (!nrf::simplify_factor_valid(factor)) {
      std::printf("simplified 0 0 %" PRIu32 " %" PRIu32 " 0 0\n", nv, nt);
      ++problems;
      continue;
    }
    const nrf::Simplified S = nrf::simplify_host(L, factor, nv, vertices.data(), edges.data(), triangles.data(), nt);
    const size_t kv = S.sources.size(), kt = S.triangles.size() / 3;
    const bool ok = S.ok && S.vertices.size() == 3 * kv && S.edges.size() == kv && S.vertex_map.size() == nv;
    std::printf("simplified %zu %zu %" PRIu32 " %" PRIu32 " %d 1\n", kv, kt, nv, nt, (int)ok);
    const uint32_t n_clusters = nrf::simplify_clusters(L, factor);
    for (uint32_t v = 0; v < nv; ++v) {
      float x[3];
      __builtin_memcpy(x, &vertices[3 * (size_t)v], 12);
      uint32_t b[3];
      const uint32_t cid = nrf::simplify_cluster(L, factor, edges[v], b);
      const uint64_t key = cid < n_clusters ? nrf::simplify_key(L, factor, b, x, v) : 0;
      std::printf("r %" PRIu32 " %016" PRIx64 " %" PRIu32 "\n", cid, key, nrf::simplify_rep(L, factor, n_clusters, edges.data(), S.keys.data(), nv, v));
    }
    for (size_t i = 0; i < kv; ++i)
      std::printf("o %" PRIu32 " %" PRIu32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", S.sources[i], S.edges[i], S.vertices[3 * i], S.vertices[3 * i + 1],
                  S.vertices[3 * i + 2]);
    for (uint32_t v = 0; v < nv; ++v) std::printf("m %" PRIu32 "\n", S.vertex_map[v]);
    for (size_t i = 0; i < kt; ++i) std::printf("t %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", S.triangles[3 * i], S.triangles[3 * i + 1], S.triangles[3 * i + 2]);
    if (!ok) {
      std::fprintf(stderr, "simplify_plan_check: problem %ld: the scan and the scatter disagree\n", problems);
      return 4;
    }
    ++problems;
  }
  std::fprintf(stderr, "simplify_plan_check: %ld problems\n", problems);
  return 0;
}
