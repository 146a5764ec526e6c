// Sanitizer driver of csrc/nrf_mesh_plan.h (make mesh_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the count, the
// scan and the emit of the mesh extraction (nrf_extract_mesh) on the CPU, compiled from the text the kernels compile.  Problems on
// stdin, any number of them; floats are fp32 bit patterns (hexadecimal), the dimensions decimal:
//     origin[3] cell[3] nx ny nz iso  sigma[nx * ny * nz]
// and per problem on stdout
//     mesh <n_vertices> <n_triangles> <lattice valid> <iso valid>
//     v <x> <y> <z>        one line per vertex, bit patterns
//     t <a> <b> <c>        one line per triangle, decimal
// With the argument "table" it prints the triangle table instead: "<t> <mask> <from> <to> x 3" per triangle, corner codes of the cell.
// tests/test_mesh_cpu.py holds the output to the numpy replay the GPU tests use (tests/mesh_replay.py).  Built with
// -ffp-contract=off, as the library is: every operation is one fp32 rounding.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/nrf_mesh_plan.h"

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

static const nrf::MeshTable TABLE = nrf::mesh_make_table();

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "table")) {
    for (uint32_t t = 0; t < 6; ++t)
      for (uint32_t mask = 0; mask < 16; ++mask)
        for (uint32_t w = 0; w < 2; ++w) {
          const uint32_t word = TABLE.tri[t][mask][w];
          if ((w < nrf::mesh_tet_triangles(mask)) != (word >> 31)) return 3;
          if (!(word >> 31)) continue;
          std::printf("%u %u", t, mask);
          for (int c = 0; c < 3; ++c) std::printf(" %u %u", (word >> (6 * c)) & 7u, (word >> (6 * c + 3)) & 7u);
          std::printf("\n");
        }
    return 0;
  }
  long problems = 0;
  for (;;) {
    uint32_t w[6], iso_bits;
    nrf::MeshLattice L;
    int got = 0;
    for (; got < 6; ++got)
      if (std::scanf("%" SCNx32, &w[got]) != 1) break;
    if (got == 0) break;
    if (got != 6 || std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNx32, &L.dims[0], &L.dims[1], &L.dims[2], &iso_bits) != 4) {
      std::fprintf(stderr, "mesh_plan_check: problem %ld has a short header\n", problems);
      return 2;
    }
    for (int c = 0; c < 3; ++c) L.origin[c] = as_float(w[c]), L.cell[c] = as_float(w[3 + c]);
    const float iso = as_float(iso_bits);
    const bool valid = nrf::mesh_lattice_valid(L.origin, L.cell, L.dims);
    const uint64_t n = valid ? nrf::mesh_points(L) : 0;
    if (n > (1u << 22)) {
      std::fprintf(stderr, "mesh_plan_check: at most 2^22 points here\n");
      return 2;
    }
    if (!valid) {  // (the sigmas of a refused lattice cannot be counted: it has to be the last problem)
      std::printf("mesh 0 0 0 %d\n", (int)nrf::mesh_iso_valid(iso));
      ++problems;
      break;
    }
    std::vector<float> sigma(n);
    for (uint64_t p = 0; p < n; ++p) {
      uint32_t u;
      if (std::scanf("%" SCNx32, &u) != 1) {
        std::fprintf(stderr, "mesh_plan_check: problem %ld has %" PRIu64 " of %" PRIu64 " sigmas\n", problems, p, n);
        return 2;
      }
      sigma[p] = as_float(u);
    }
    std::vector<uint32_t> codes(n), vbase(n), tbase(n);
    for (uint64_t p = 0; p < n; ++p) codes[p] = nrf::mesh_count_point(L, sigma.data(), iso, (uint32_t)p);
    uint64_t nv = 0, nt = 0;
    nrf::mesh_scan_host(codes.data(), n, vbase.data(), tbase.data(), nv, nt);
    // exactly the element counts: AddressSanitizer sees any write the bounds checks let through
    std::vector<float> vertices(nrf::mesh_vertex_bytes(nv) / 4);
    std::vector<uint32_t> triangles(nrf::mesh_triangle_bytes(nt) / 4);
    bool ok = true;
    for (uint64_t p = 0; p < n; ++p)
      ok = nrf::mesh_emit_point(L, sigma.data(), iso, (uint32_t)p, codes.data(), vbase.data(), tbase.data(), TABLE, (uint32_t)nv, (uint32_t)nt,
                                vertices.data(), triangles.data()) && ok;
    if (!ok) {
      std::fprintf(stderr, "mesh_plan_check: problem %ld: count and emit disagree\n", problems);
      return 4;
    }
    std::printf("mesh %" PRIu64 " %" PRIu64 " 1 %d\n", nv, nt, (int)nrf::mesh_iso_valid(iso));
    for (uint64_t i = 0; i < nv; ++i)
      std::printf("v %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", as_bits(vertices[3 * i]), as_bits(vertices[3 * i + 1]), as_bits(vertices[3 * i + 2]));
    for (uint64_t i = 0; i < nt; ++i) std::printf("t %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", triangles[3 * i], triangles[3 * i + 1], triangles[3 * i + 2]);
    ++problems;
  }
  std::fprintf(stderr, "mesh_plan_check: %ld problems\n", problems);
  return 0;
}
