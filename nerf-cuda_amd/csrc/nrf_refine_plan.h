// nrf_refine_plan.h -- the arithmetic of the mesh refinement (nrf_refine_mesh) without a device: a vertex of the extraction sits on a
// crossing edge of the lattice, one endpoint inside and one outside, so the edge is a bracket of the iso value and bisection along
// it converges whatever the density does in between.  refine_kernel (nrf_kernels_refine.hip) and host/refine_plan_check.cpp compile
// this text, so the kernel's definition and the tests' replay are one.  Every floating-point operation is ONE fp32 rounding: the
// library is built with -ffp-contract=off -fno-fast-math, and a host build of this header has to be (host/Makefile: refine_asan).
//
// Edge word  w = (p << 3) | m: lattice point p (< 2^27, so the word fits in 30 bits) and its edge m = 1 .. 7 (nrf_mesh_plan.h).
//            (i, j, k) = mesh_ijk(p); xp = mesh_position(i, j, k); xq = mesh_position of the point edge m runs to.
// Points     e_c = xq_c - xp_c;  point(u)_c = xp_c + u * e_c   (difference, product, sum: one rounding each -- mesh_vertex's form)
// Density    s(x) = nrf_density at x: the centre-only guard of nrf_points_plan.h; a refused point has sigma 0.
// Steps      1. s0 = s(xp), s1 = s(xq): at the lattice positions themselves.  in0 = mesh_inside(s0, iso), in1 = mesh_inside(s1, iso).
//            2. in0 == in1: unbracketed.  The vertex keeps its bits, the bracket record is (0, 1, s0, s1).
//            3. lo = 0, hi = 1, slo = s0, shi = s1.
//            4. n_steps times: um = 0.5f * (lo + hi) (exact for n_steps <= 16); sm = s(point(um));
//               mesh_inside(sm, iso) == in0 ? (lo, slo) = (um, sm) : (hi, shi) = (um, sm).
//            5. d = shi - slo; num = iso - slo; r = num / d; if (!(r >= 0 && r <= 1)) r = 0.5f; u = lo + r * (hi - lo); v = point(u).
//               The bracket record is (lo, hi, slo, shi).
// With n_steps == 0 this is mesh_vertex on the network's own sigmas (u = 0 + r * 1 = r).  An unbracketed vertex still asks for
// n_steps midpoints -- 0.5 every time, its bracket does not move -- and drops the answers: all lanes of a wave run all passes.
#pragma once
#include "nrf_mesh_plan.h"

namespace nrf {

constexpr uint32_t REFINE_MAX_STEPS = 16;
inline bool refine_steps_valid(uint32_t n_steps) { return n_steps <= REFINE_MAX_STEPS; }
inline uint64_t refine_edge_bytes(uint64_t n_vertices) { return n_vertices * 4; }
inline uint64_t refine_bracket_bytes(uint64_t n_vertices) { return n_vertices * 16; }

NRF_MESH_HD inline uint32_t refine_edge_word(uint32_t p, uint32_t m) { return (p << 3) | m; }

// The edge words of p's crossing edges at their scanned offsets, in emit's order (mesh_emit_point: ascending m from vbase[p]).  A
// write that would fall outside n_vertices is dropped and the function returns false.
NRF_MESH_HD inline bool refine_emit_edges(uint32_t p, uint32_t code, uint32_t vbase, uint32_t n_vertices, uint32_t* edges) {
  bool ok = true;
  uint32_t vid = vbase;
  for (uint32_t m = 1; m < 8; ++m) {
    if (!((code >> m) & 1u)) continue;
    if (vid < n_vertices) edges[vid] = refine_edge_word(p, m);
    else ok = false;
    ++vid;
  }
  return ok;
}

// the positions of the two lattice points of edge word w
NRF_MESH_HD inline void refine_edge(const MeshLattice& L, uint32_t w, float (&xp)[3], float (&xq)[3]) {
  const uint32_t p = w >> 3, m = w & 7u;
  uint32_t ijk[3];
  mesh_ijk(L, p, ijk);
  mesh_position(L, ijk[0], ijk[1], ijk[2], xp);
  mesh_position(L, ijk[0] + (m & 1u), ijk[1] + ((m >> 1) & 1u), ijk[2] + ((m >> 2) & 1u), xq);
}

NRF_MESH_HD inline void refine_point(const float (&xp)[3], const float (&xq)[3], float u, float (&x)[3]) {
  for (int c = 0; c < 3; ++c) {
    const float e = xq[c] - xp[c];
    const float ue = u * e;
    x[c] = xp[c] + ue;
  }
}

struct RefineState {
  float lo, hi, slo, shi;
  bool in0, bracketed;
};

// steps 1 .. 3
NRF_MESH_HD inline RefineState refine_start(float s0, float s1, float iso) {
  RefineState R;
  R.lo = 0.0f;
  R.hi = 1.0f;
  R.slo = s0;
  R.shi = s1;
  R.in0 = mesh_inside(s0, iso);
  R.bracketed = R.in0 != mesh_inside(s1, iso);
  return R;
}

// step 4: the midpoint a step asks for, and what its sigma does to the bracket (nothing where there is none)
NRF_MESH_HD inline float refine_mid(const RefineState& R) {
  const float sum = R.lo + R.hi;
  return 0.5f * sum;
}
NRF_MESH_HD inline void refine_step(RefineState& R, float um, float sm, float iso) {
  if (!R.bracketed) return;
  if (mesh_inside(sm, iso) == R.in0) {
    R.lo = um;
    R.slo = sm;
  } else {
    R.hi = um;
    R.shi = sm;
  }
}

// step 5: the secant step inside the final bracket
NRF_MESH_HD inline float refine_finish(const RefineState& R, float iso) {
  const float d = R.shi - R.slo;
  const float num = iso - R.slo;
  float r = num / d;
  if (!(r >= 0.0f && r <= 1.0f)) r = 0.5f;
  const float w = R.hi - R.lo;
  const float rw = r * w;
  return R.lo + rw;
}

// Pass `pass` of n_steps + 2 of edge word w: the position whose sigma the pass asks for (0: xp, 1: xq, then point(um) of the bracket
// as it stands), recomputed from the word every time so that nothing but the bracket lives across a network pass.
NRF_MESH_HD inline void refine_pass_position(const MeshLattice& L, uint32_t w, const RefineState& R, uint32_t pass, float (&x)[3]) {
  float xp[3], xq[3];
  refine_edge(L, w, xp, xq);
  if (pass >= 2u) {
    refine_point(xp, xq, refine_mid(R), x);
  } else {
    for (int c = 0; c < 3; ++c) x[c] = pass == 0u ? xp[c] : xq[c];
  }
}

}  // namespace nrf
