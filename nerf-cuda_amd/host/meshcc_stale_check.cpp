// The labelling of csrc/nrf_meshcc_plan.h under loads that return stale values (make meshcc_stale_asan: AddressSanitizer + UBSan, host
// only, no libnerfhip.so).  nrf_kernels_meshcc.hip argues that hook and compress are right "whatever mix of older and newer values of
// parent[] its loads return"; every other CPU run of that text is serial and exact, and a GPU run meets whatever its timing brings.
// Here the kernels' own functions (meshcc_root, meshcc_hook_of, meshcc_hook_lower, meshcc_compress, meshcc_triangle_valid) run over a
// memory that hands out old values on purpose.
//
// The memory.  A launch is the set of lanes of one kernel -- one per triangle (hook) or per vertex (compress) -- run one after the other
// in an order drawn from a seeded generator.  For every address the memory keeps the value at the launch's start and every value
// stored since.  Before each root walk the lane gets a VIEW of parent[]: every element drawn from that element's list, uniformly or
// with three draws in four going to the oldest value.  lower() -- the kernel's atomicMin -- and compress's store act on the true
// current value, and lower() returns the true old one.  A launch boundary collapses every list to the current value.  The loop is the
// host's (label_mesh): hook, compress, stop when no hook lowered anything, fail beyond n_vertices + 1 rounds.
// A mesh of at most FULL_VIEW vertices gets the whole view drawn for every walk, O(n_vertices) each.  Above that only the elements the
// walk is about to load are drawn afresh (found by following the draws from the start; a walk descends, so it loads no address
// twice); the rest of the view keeps draws of earlier walks, which no load of this walk reads.  What the walk returns is meshcc_root's
// over that view either way.
//
// Checked for every seed, against a union-find built up front from the triangles and not against the text under test:
//   (I)  after every store, the stored value is <= its index and in the same component as its index;
//   (M)  no store raises a value: parents only fall (what a plain store in place of the minimum breaks);
//   every walk returns a member of its start's component;
//   the round in which no hook lowered anything has three equal exact roots for every valid triangle;
//   the labels are meshcc_label_host's and the component minima of the union-find; rounds <= n_vertices + 1.
//
// Problems on stdin, any number:   name n_vertices n_triangles seeds  a b c (n_triangles index triples)
// and per problem on stdout
//     mesh <name> <n_vertices> <n_triangles> runs <2 * seeds> rounds <min> <max> host <meshcc_label_host's> walks <n> stale <n>
//     l <label>                        one line per vertex
// (stale: walks that loaded at least one value that was not the current one).  tests/test_mesh_components_cpu.py feeds it and holds the
// labels to tests/meshcc_replay.py.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../csrc/nrf_meshcc_plan.h"

namespace {

constexpr uint32_t FULL_VIEW = 64;

struct Rng {
  uint64_t s;
  uint64_t next() {  // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return (uint32_t)(((next() >> 32) * (uint64_t)n) >> 32); }
};

[[noreturn]] void fail(const char* name, uint64_t seed, int bias, const char* what, uint64_t a, uint64_t b) {
  std::fprintf(stderr, "meshcc_stale_check: %s, seed %" PRIu64 ", %s: %s (%" PRIu64 ", %" PRIu64 ")\n", name, seed,
               bias ? "oldest-biased" : "uniform", what, a, b);
  std::exit(4);
}

// components by union-find over the valid triangles: least[v] = the smallest vertex of v's component
std::vector<uint32_t> least_of_component(uint32_t nv, const std::vector<uint32_t>& tri) {
  std::vector<uint32_t> up(nv);
  std::iota(up.begin(), up.end(), 0u);
  auto find = [&up](uint32_t x) {
    while (up[x] != x) x = up[x] = up[up[x]];
    return x;
  };
  auto join = [&](uint32_t x, uint32_t y) {
    x = find(x), y = find(y);
    if (x != y) up[x > y ? x : y] = x > y ? y : x;  // the smaller one stays the representative
  };
  for (size_t t = 0; t + 2 < tri.size(); t += 3)
    if (tri[t] < nv && tri[t + 1] < nv && tri[t + 2] < nv) join(tri[t], tri[t + 1]), join(tri[t], tri[t + 2]);
  std::vector<uint32_t> least(nv);
  for (uint32_t v = 0; v < nv; ++v) least[v] = find(v);
  return least;
}

struct Memory {
  const char* name;
  uint32_t nv;
  const std::vector<uint32_t>& tri;
  const std::vector<uint32_t>& least;
  uint64_t seed = 0;
  int bias = 0;
  Rng rng{0};
  std::vector<uint32_t> cur, view, touched, order;
  std::vector<std::vector<uint32_t>> lists;  // per address: the value at the launch's start, then every value stored since
  uint64_t walks = 0, stale = 0;

  Memory(const char* name_, uint32_t nv_, const std::vector<uint32_t>& tri_, const std::vector<uint32_t>& least_)
      : name(name_), nv(nv_), tri(tri_), least(least_), cur(nv_), view(nv_), lists(nv_) {}

  void init(uint64_t seed_, int bias_) {  // meshcc_init_kernel
    seed = seed_, bias = bias_;
    rng.s = seed_ * 2 + (uint64_t)bias_ + 0x1234567ull * nv;
    for (uint32_t v = 0; v < nv; ++v) cur[v] = view[v] = v, lists[v].assign(1, v);
    touched.clear();
  }
  void launch_boundary() {
    for (uint32_t x : touched) lists[x].assign(1, cur[x]), view[x] = cur[x];
    touched.clear();
  }
  const std::vector<uint32_t>& shuffled(uint64_t n) {
    order.resize(n);
    std::iota(order.begin(), order.end(), 0u);
    for (uint64_t i = n; i > 1; --i) std::swap(order[i - 1], order[rng.below((uint32_t)i)]);
    return order;
  }
  uint32_t draw(uint32_t x) {
    const std::vector<uint32_t>& l = lists[x];
    if (l.size() == 1 || (bias && rng.below(4) != 0)) return l[0];
    return l[rng.below((uint32_t)l.size())];
  }
  // the view of the walk from x
  void give_view(uint32_t x) {
    if (nv <= FULL_VIEW)
      for (uint32_t a : touched) view[a] = draw(a);  // (an untouched element has one value, and the view holds it)
    bool old = false;
    for (uint32_t y = x;;) {
      if (nv > FULL_VIEW) view[y] = draw(y);
      old = old || view[y] != cur[y];
      if (view[y] >= y) break;
      y = view[y];
    }
    ++walks;
    stale += old;
  }
  uint32_t root(uint32_t x) {
    give_view(x);
    const uint32_t r = nrf::meshcc_root(view.data(), x);
    if (r > x || least[r] != least[x]) fail(name, seed, bias, "a walk left its start's component: start, end", x, r);
    return r;
  }
  void store(uint32_t x, uint32_t value) {
    if (value > x || least[value] != least[x]) fail(name, seed, bias, "(I) broke: index, stored value", x, value);
    if (value > cur[x]) fail(name, seed, bias, "(M) broke, a store raised a value: index, stored value", x, value);
    cur[x] = value;
    lists[x].push_back(value);
    if (lists[x].size() == 2) touched.push_back(x);
  }
  uint32_t exact_root(uint32_t x) const {
    while (cur[x] != x) x = cur[x];
    return x;
  }

  bool hook_launch() {
    bool lowered = false;
    launch_boundary();
    for (uint32_t t : shuffled(tri.size() / 3)) {
      const uint32_t a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
      if (!nrf::meshcc_triangle_valid(a, b, c, nv)) continue;
      const nrf::MeshccHook h = nrf::meshcc_hook_of([this](uint32_t x) { return root(x); }, a, b, c);
      lowered = nrf::meshcc_hook_lower(h, [this](uint32_t r, uint32_t low) {
                  const uint32_t old = cur[r];
                  if (low < old) store(r, low);
                  return old;
                }) || lowered;
    }
    return lowered;
  }
  void compress_launch() {
    launch_boundary();
    for (uint32_t v : shuffled(nv)) {
      give_view(v);
      nrf::meshcc_compress(view.data(), v, [this](uint32_t x, uint32_t r) { store(x, r); });
      if (least[cur[v]] != least[v]) fail(name, seed, bias, "a walk left its start's component: start, end", v, cur[v]);
    }
  }
  uint32_t label() {  // label_mesh's loop
    uint32_t rounds = 0;
    while (nv) {
      const bool lowered = hook_launch();
      if (!lowered)
        for (size_t t = 0; t + 2 < tri.size(); t += 3) {
          if (!nrf::meshcc_triangle_valid(tri[t], tri[t + 1], tri[t + 2], nv)) continue;
          const uint32_t r = exact_root(tri[t]);
          if (exact_root(tri[t + 1]) != r || exact_root(tri[t + 2]) != r)
            fail(name, seed, bias, "no hook lowered anything, yet a triangle spans two roots: triangle, root of its first vertex", t / 3, r);
        }
      compress_launch();
      ++rounds;
      if (!lowered) break;
      if (rounds > nv) fail(name, seed, bias, "the labelling did not settle within n_vertices + 1 rounds: rounds, n_vertices", rounds, nv);
    }
    return rounds;
  }
};

}  // namespace

int main() {
  long problems = 0;
  for (;;) {
    char name[64];
    uint32_t nv, seeds;
    uint64_t nt;
    const int got = std::scanf("%63s %" SCNu32 " %" SCNu64 " %" SCNu32, name, &nv, &nt, &seeds);
    if (got == EOF || got == 0) break;
    if (got != 4 || nv > (1u << 20) || nt > (1u << 20)) {
      std::fprintf(stderr, "meshcc_stale_check: problem %ld has a bad header\n", problems);
      return 2;
    }
    std::vector<uint32_t> tri(3 * (size_t)nt);
    for (size_t i = 0; i < tri.size(); ++i)
      if (std::scanf("%" SCNu32, &tri[i]) != 1) {
        std::fprintf(stderr, "meshcc_stale_check: problem %ld has %zu of %zu indices\n", problems, i, tri.size());
        return 2;
      }
    const std::vector<uint32_t> least = least_of_component(nv, tri);
    const nrf::MeshccParts host = nrf::meshcc_label_host(nv, tri.data(), nt);
    if (host.labels != least) fail(name, 0, 0, "meshcc_label_host is not the union-find", 0, 0);
    Memory M(name, nv, tri, least);
    uint32_t lo = ~0u, hi = 0;
    for (int bias = 0; bias < 2; ++bias)
      for (uint32_t seed = 0; seed < seeds; ++seed) {
        M.init(seed, bias);
        const uint32_t rounds = M.label();
        if (M.cur != host.labels) fail(name, seed, bias, "the labels are not meshcc_label_host's", 0, 0);
        lo = rounds < lo ? rounds : lo;
        hi = rounds > hi ? rounds : hi;
      }
    std::printf("mesh %s %" PRIu32 " %" PRIu64 " runs %" PRIu32 " rounds %" PRIu32 " %" PRIu32 " host %" PRIu32 " walks %" PRIu64 " stale %" PRIu64 "\n",
                name, nv, nt, 2 * seeds, seeds ? lo : 0, hi, host.n_rounds, M.walks, M.stale);
    for (uint32_t v = 0; v < nv; ++v) std::printf("l %" PRIu32 "\n", host.labels[v]);
    ++problems;
  }
  std::fprintf(stderr, "meshcc_stale_check: %ld problems\n", problems);
  return 0;
}
