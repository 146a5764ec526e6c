// nrf_step_plan.h -- the step table of the barrier fast-forward, without a HIP call (plain C++17: a host compiler builds it
// alone; the kernels compile the same text).  The march's step sequence t_{k+1} = t_k + clamp(t_k * dt_gamma, dt_min, dt_max)
// (render_utils.h:593-653, nrf_device.h march_next) depends on nothing of a ray but its start value, and near_far clamps that
// to min_near: every ray that does not enter through an aabb face walks the SAME members.  step_table tabulates them once per
// (min_near, dt_gamma, bound, H); step_land returns what the stepping loop `while (t < tb) t += dt(t)` returns, from the table
// where the ray is on it.  nrf_api.hip builds and uploads the table (step_table_for), render_persistent_kernel stages it in LDS
// (nrf_render.h), nrf_debug_step_table returns both functions' answers (tests/test_step_table_cpu.py).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#ifndef NRF_STEP_TABLE
#define NRF_STEP_TABLE 1  // make EXTRA=-DNRF_STEP_TABLE=0: no kernel knows the table (A/B builds: the listings of the loop alone)
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NRF_STEP_HD __host__ __device__
#else
#define NRF_STEP_HD
#endif

namespace nrf {

constexpr int STEP_TABLE_CAPACITY = 1024;  // entries (4 KB of LDS); the lower bound's depth is log2 of it
constexpr int STEP_TABLE_DEPTH = 10;
static_assert((1 << STEP_TABLE_DEPTH) == STEP_TABLE_CAPACITY, "step_land's probes cover the capacity");

// the launch constants of the sequence, as march_const (nrf_device.h) makes them
NRF_STEP_HD inline float step_dt_min() { return 2 * 1.7320508075688772f / 1024; }  // MIN_STEPSIZE, render_utils.h:181-183
NRF_STEP_HD inline float step_dt_max(float bound, uint32_t H) { return 2 * bound / (float)H; }

// clamp(x, lo, hi) for lo <= hi: the value of v_med3_f32 for every x that is not NaN (x = t * dt_gamma with t not NaN)
NRF_STEP_HD inline float step_clamp(float x, float lo, float hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_fmed3f(x, lo, hi);
#else
  return fminf(hi, fmaxf(lo, x));
#endif
}
// one member to the next: three operations, each rounded to fp32 on its own (the product must not fuse into the add: the
// clamp stands between them in the march, and the translation units are built with -ffp-contract=off)
NRF_STEP_HD inline float step_next(float t, float dt_gamma, float dt_min, float dt_max) {
  const float p = t * dt_gamma;
  const float dt = step_clamp(p, dt_min, dt_max);
  return t + dt;
}
NRF_STEP_HD inline uint32_t step_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bit_cast(uint32_t, x);
#else
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
#endif
}

// The members t_0 = min_near, t_1, ... into out[capacity]; returns their number.  The table ends with the first member
// beyond min_near + 2 sqrt(3) bound (the longest stretch a ray spends in the aabb) plus one step, or at `capacity` entries.
// No table (0) for inputs whose sequence is not strictly increasing and finite: the loop serves those.
NRF_STEP_HD inline int step_table(float min_near, float dt_gamma, float bound, uint32_t H, int capacity, float* out) {
  if (capacity > STEP_TABLE_CAPACITY) capacity = STEP_TABLE_CAPACITY;
  if (capacity < 2 || H == 0 || !(min_near >= 0.0f) || !(dt_gamma >= 0.0f) || !(bound > 0.0f)) return 0;
  const float dt_min = step_dt_min(), dt_max = step_dt_max(bound, H);
  if (!(dt_min <= dt_max)) return 0;  // (the median of three is a clamp only then)
  const float reach = min_near + 2 * 1.7320508075688772f * bound;
  int n = 0, beyond = 0;
  float t = min_near;
  while (n < capacity) {
    if (n > 0 && !(t > out[n - 1])) return 0;  // t + dt == t: the march itself never ends there (nrf_device.h ray guard)
    if (!(t <= 3.0e38f)) return 0;
    out[n++] = t;
    if (t > reach && ++beyond == 2) break;
    t = step_next(t, dt_gamma, dt_min, dt_max);
  }
  return n;
}

// What `while (t < tb) t += clamp(t * dt_gamma, dt_min, dt_max);` returns.  A start with the bits of table[0] and a target up to
// the last member: the first member m with !(m < tb), by a lower bound of fixed depth without a branch.  A target beyond the
// last member: the loop from that member.  A target that is NaN, -inf, the NONE value or anything else at or below the start
// leaves t as it is, as the loop does.  Every other start, and a null table: the loop from t.
NRF_STEP_HD inline float step_land(const float* table, int n, float t, float tb, float dt_gamma, float dt_min, float dt_max) {
  if (!(t < tb)) return t;
  if (table != nullptr && n > 0 && step_bits(t) == step_bits(table[0])) {
    const float last = table[n - 1];
    if (!(last < tb)) {
      int pos = 0;  // members below tb: table[pos] is the answer (pos <= n - 1 since table[n - 1] is not below tb)
#if defined(__clang__)
#pragma unroll
#endif
      for (int s = STEP_TABLE_CAPACITY / 2; s > 0; s >>= 1) {
        const int j = pos + s;
        const float m = table[(j <= n ? j : n) - 1];
        pos = (j <= n && m < tb) ? j : pos;
      }
      return table[pos];
    }
    t = last;
  }
  while (t < tb) t = step_next(t, dt_gamma, dt_min, dt_max);
  return t;
}

// Where the table lies in the persistent workgroup's LDS: behind everything the instance stages today (lds_bytes: the launch's
// LDS without it, nrf_launch.h render_persistent_launch_lds_bytes), when its n floats still fit the compute unit (cu_bytes) --
// it has the lowest priority.  Returns the byte offset, or -1: the kernel gets no table and steps.
inline int step_table_lds_offset(uint32_t lds_bytes, int n, uint32_t cu_bytes) {
  const uint64_t off = ((uint64_t)lds_bytes + 15u) & ~(uint64_t)15u;
  return n > 0 && off + 4u * (uint64_t)n <= cu_bytes ? (int)off : -1;
}

}  // namespace nrf
