// Sanitizer driver of csrc/nrf_meshcc_plan.h (make meshcc_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the labelling,
// the table and the filter of nrf_mesh_components / nrf_filter_mesh on the CPU, compiled from the text the kernels compile.  Problems
// on stdin, any number of them, all decimal:
//     n_vertices n_triangles min_triangles flags  a b c  (n_triangles index triples)
// and per problem on stdout
//     parts <n_vertices> <n_components> <n_rounds> <flags valid>
//     l <label>                        one line per vertex
//     c <label> <vertices> <triangles> one line per component, ascending label
//     kept <kept vertices> <kept triangles> <ok>
//     o <old id>                       one line per kept vertex: the old id of new vertex 0, 1, ...
//     t <a> <b> <c>                    one line per kept triangle, remapped
// A problem with unknown flag bits prints its parts and "kept 0 0 0".  tests/test_mesh_components_cpu.py holds the output to the numpy
// replay the GPU tests use (tests/meshcc_replay.py).  The vertices' float bits are not part of a problem: the filter moves the vertex
// ids themselves through meshcc_move_vertex, as three words each, and checks that they arrive where "o" says.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../csrc/nrf_meshcc_plan.h"

int main() {
  long problems = 0;
  for (;;) {
    uint32_t nv, flags;
    uint64_t nt, min_triangles;
    const int got = std::scanf("%" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu32, &nv, &nt, &min_triangles, &flags);
    if (got == EOF || got == 0) break;
    if (got != 4) {
      std::fprintf(stderr, "meshcc_plan_check: problem %ld has a short header\n", problems);
      return 2;
    }
    if (nv > (1u << 24) || nt > (1u << 24)) {
      std::fprintf(stderr, "meshcc_plan_check: at most 2^24 vertices and triangles here\n");
      return 2;
    }
    std::vector<uint32_t> triangles(3 * (size_t)nt);
    for (size_t i = 0; i < triangles.size(); ++i)
      if (std::scanf("%" SCNu32, &triangles[i]) != 1) {
        std::fprintf(stderr, "meshcc_plan_check: problem %ld has %zu of %zu indices\n", problems, i, triangles.size());
        return 2;
      }
    const nrf::MeshccParts P = nrf::meshcc_label_host(nv, triangles.data(), nt);
    const size_t nc = P.components.size() / 3;
    const bool valid = nrf::meshcc_flags_valid(flags);
    std::printf("parts %" PRIu32 " %zu %" PRIu32 " %d\n", nv, nc, P.n_rounds, (int)valid);
    for (uint32_t v = 0; v < nv; ++v) std::printf("l %" PRIu32 "\n", P.labels[v]);
    for (size_t r = 0; r < nc; ++r)
      std::printf("c %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", P.components[3 * r], P.components[3 * r + 1], P.components[3 * r + 2]);
    if (!valid) {
      std::printf("kept 0 0 0\n");
      ++problems;
      continue;
    }
    // the vertex "positions" are the ids themselves: what meshcc_move_vertex carries must arrive at its new place unchanged
    std::vector<uint32_t> ids(3 * (size_t)nv);
    for (uint32_t v = 0; v < nv; ++v) ids[3 * (size_t)v] = v, ids[3 * (size_t)v + 1] = ~v, ids[3 * (size_t)v + 2] = v ^ 0x5a5a5a5au;
    const nrf::MeshccFiltered F = nrf::meshcc_filter_host(P, nv, ids.data(), triangles.data(), nt, min_triangles, flags);
    const size_t kv = F.old_vertex.size(), kt = F.old_triangle.size();
    bool ok = F.ok && F.vertices.size() == 3 * kv && F.triangles.size() == 3 * kt;
    for (size_t i = 0; ok && i < kv; ++i)
      ok = F.vertices[3 * i] == F.old_vertex[i] && F.vertices[3 * i + 1] == ~F.old_vertex[i] && F.vertices[3 * i + 2] == (F.old_vertex[i] ^ 0x5a5a5a5au);
    std::printf("kept %zu %zu %d\n", kv, kt, (int)ok);
    for (size_t i = 0; i < kv; ++i) std::printf("o %" PRIu32 "\n", F.old_vertex[i]);
    for (size_t i = 0; i < kt; ++i) std::printf("t %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", F.triangles[3 * i], F.triangles[3 * i + 1], F.triangles[3 * i + 2]);
    if (!ok) {
      std::fprintf(stderr, "meshcc_plan_check: problem %ld: the scan and the scatter disagree\n", problems);
      return 4;
    }
    ++problems;
  }
  std::fprintf(stderr, "meshcc_plan_check: %ld problems\n", problems);
  return 0;
}
