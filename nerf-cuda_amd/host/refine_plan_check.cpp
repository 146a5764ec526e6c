// Sanitizer driver of csrc/nrf_refine_plan.h (make refine_asan: AddressSanitizer + UBSan, host only, no libnerfhip.so): the bisection
// of nrf_refine_mesh on the CPU, compiled from the text refine_kernel compiles.  The density is not here: the caller supplies, per
// vertex, the sigmas a density answers to the n_steps + 2 positions the definition asks for, in order (the positions depend on the
// earlier answers; tests/refine_replay.py, which has a density, records them).  Problems on stdin, any number of them; floats are fp32
// bit patterns (hexadecimal), counts decimal:
//     origin[3] cell[3] nx ny nz iso n_steps n_vertices   then per vertex   word sigma[n_steps + 2]
// and per problem on stdout
//     refine <n_vertices> <n_steps> <lattice valid> <n_steps valid>
//     <word> <bracketed> position[n_steps + 2][3] lo hi s_lo s_hi x y z      one line per vertex, bit patterns
// position[0] = xp, position[1] = xq, position[2 + k] = point(um) of step k; (x, y, z) is the refined vertex, zeros where the edge is
// unbracketed (the vertex keeps the bits it has, which this program never sees).
// With the argument "edges" it reads mesh_plan_check's problems instead (origin[3] cell[3] nx ny nz iso sigma[nx * ny * nz]) and
// prints "edges <n_vertices>" and the edge word of every vertex of the extraction, one per line: count, scan and refine_emit_edges.
// tests/test_mesh_refine_cpu.py holds the output to the numpy replay the GPU tests use.  Built with -ffp-contract=off, as the library
// is: every operation is one fp32 rounding.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/nrf_refine_plan.h"

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

// origin[3] cell[3] nx ny nz iso: 1 = read, 0 = end of input, -1 = short
static int read_head(nrf::MeshLattice& L, float& iso) {
  uint32_t w[6], iso_bits;
  int got = 0;
  for (; got < 6; ++got)
    if (std::scanf("%" SCNx32, &w[got]) != 1) break;
  if (got == 0) return 0;
  if (got != 6 || std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNx32, &L.dims[0], &L.dims[1], &L.dims[2], &iso_bits) != 4) return -1;
  for (int c = 0; c < 3; ++c) L.origin[c] = as_float(w[c]), L.cell[c] = as_float(w[3 + c]);
  iso = as_float(iso_bits);
  return 1;
}

static int edges_main() {
  long problems = 0;
  for (;;) {
    nrf::MeshLattice L;
    float iso;
    const int head = read_head(L, iso);
    if (head == 0) break;
    if (head < 0 || !nrf::mesh_lattice_valid(L.origin, L.cell, L.dims) || nrf::mesh_points(L) > (1u << 22)) {
      std::fprintf(stderr, "refine_plan_check: problem %ld: a short header or a lattice that is not valid (at most 2^22 points here)\n", problems);
      return 2;
    }
    const uint64_t n = nrf::mesh_points(L);
    std::vector<float> sigma(n);
    for (uint64_t p = 0; p < n; ++p) {
      uint32_t u;
      if (std::scanf("%" SCNx32, &u) != 1) return 2;
      sigma[p] = as_float(u);
    }
    std::vector<uint32_t> codes(n), vbase(n), tbase(n);
    for (uint64_t p = 0; p < n; ++p) codes[p] = nrf::mesh_count_point(L, sigma.data(), iso, (uint32_t)p);
    uint64_t nv = 0, nt = 0;
    nrf::mesh_scan_host(codes.data(), n, vbase.data(), tbase.data(), nv, nt);
    // exactly the element count: AddressSanitizer sees any write the bounds check lets through; and one short, to see it refuse
    std::vector<uint32_t> edges(nv), fewer(nv ? nv - 1 : 0);
    bool ok = true, refused = false;
    for (uint64_t p = 0; p < n; ++p) {
      ok = nrf::refine_emit_edges((uint32_t)p, codes[p], vbase[p], (uint32_t)nv, edges.data()) && ok;
      refused = !nrf::refine_emit_edges((uint32_t)p, codes[p], vbase[p], (uint32_t)fewer.size(), fewer.data()) || refused;
    }
    if (!ok || refused != (nv > 0)) {
      std::fprintf(stderr, "refine_plan_check: problem %ld: the bounds check of the edge words failed\n", problems);
      return 4;
    }
    std::printf("edges %" PRIu64 "\n", nv);
    for (uint64_t i = 0; i < nv; ++i) std::printf("%08" PRIx32 "\n", edges[i]);
    ++problems;
  }
  std::fprintf(stderr, "refine_plan_check: %ld problems\n", problems);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "edges")) return edges_main();
  long problems = 0;
  for (;;) {
    nrf::MeshLattice L;
    float iso;
    uint32_t n_steps, n_vertices;
    const int head = read_head(L, iso);
    if (head == 0) break;
    if (head < 0 || std::scanf("%" SCNu32 " %" SCNu32, &n_steps, &n_vertices) != 2) {
      std::fprintf(stderr, "refine_plan_check: problem %ld has a short header\n", problems);
      return 2;
    }
    const bool valid = nrf::mesh_lattice_valid(L.origin, L.cell, L.dims), steps_valid = nrf::refine_steps_valid(n_steps);
    if (!valid || !steps_valid) {  // (the vertices of a refused problem cannot be counted: it has to be the last one)
      std::printf("refine 0 %" PRIu32 " %d %d\n", n_steps, (int)valid, (int)steps_valid);
      ++problems;
      break;
    }
    std::printf("refine %" PRIu32 " %" PRIu32 " 1 1\n", n_vertices, n_steps);
    std::vector<float> answers(n_steps + 2);
    for (uint32_t v = 0; v < n_vertices; ++v) {
      uint32_t word;
      if (std::scanf("%" SCNx32, &word) != 1) return 2;
      for (float& a : answers) {
        uint32_t u;
        if (std::scanf("%" SCNx32, &u) != 1) return 2;
        a = as_float(u);
      }
      if ((word >> 3) >= nrf::mesh_points(L) || !(word & 7u)) {
        std::fprintf(stderr, "refine_plan_check: problem %ld: vertex %" PRIu32 " has no edge of the lattice\n", problems, v);
        return 2;
      }
      // the kernel's loop: pass 0 and 1 are the lattice points, every later pass a midpoint of the bracket as it stands
      nrf::RefineState R = nrf::refine_start(0.f, 0.f, iso);
      std::vector<uint32_t> asked;
      for (uint32_t pass = 0; pass < n_steps + 2; ++pass) {
        float x[3];
        const float um = nrf::refine_mid(R);
        nrf::refine_pass_position(L, word, R, pass, x);
        for (int c = 0; c < 3; ++c) asked.push_back(as_bits(x[c]));
        const float s = answers[pass];
        if (pass == 0) R.slo = s;
        else if (pass == 1) R = nrf::refine_start(R.slo, s, iso);
        else nrf::refine_step(R, um, s, iso);
      }
      float out[3] = {0.f, 0.f, 0.f};
      if (R.bracketed) {
        float xp[3], xq[3];
        nrf::refine_edge(L, word, xp, xq);
        nrf::refine_point(xp, xq, nrf::refine_finish(R, iso), out);
      }
      std::printf("%08" PRIx32 " %d", word, (int)R.bracketed);
      for (uint32_t a : asked) std::printf(" %08" PRIx32, a);
      std::printf(" %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32, as_bits(R.lo), as_bits(R.hi), as_bits(R.slo), as_bits(R.shi));
      std::printf(" %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", as_bits(out[0]), as_bits(out[1]), as_bits(out[2]));
    }
    ++problems;
  }
  std::fprintf(stderr, "refine_plan_check: %ld problems\n", problems);
  return 0;
}
