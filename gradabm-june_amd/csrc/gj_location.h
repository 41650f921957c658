// Infection-location series (gj_location_stats): the step's new infections attributed to the networks they came
// through, per agent group, as 64-bit integers in units of 2^-30 of an infection.  A stand-alone kernel that runs
// after the step on the few agents infected in it: it reads new_infected (4 B per agent, coalesced), and every agent
// with new_infected == 1 is taken by a group of 16 lanes - a wave attributes four agents at a time - which walks that
// agent's by-agent rows, set by set, and gathers the venues' pass-1 sums from the plan's `cum` workspaces.  (A world has
// one or two edges per agent and set: what an agent costs is the chain row pointers -> venue ids -> cum of every set,
// so agents side by side, not more lanes per agent, is what shortens the launch.)  Nothing of gj_tiled.h is involved.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gradjune_hip.h"
#include "gj_device.h"

namespace gj {

constexpr uint32_t kLocBadLabel = GJ_LOC_ERR_LABEL, kLocBadValue = GJ_LOC_ERR_VALUE, kLocBadRows = GJ_LOC_ERR_ROWS;
constexpr int kLocLdsBins = GJ_LOC_LDS_BINS;     // 8 B * 4096 = 32 KiB of LDS per workgroup
constexpr int kLocBlocks = GJ_LOC_BLOCKS;
constexpr int kLocLoads = 4;                     // new_infected loads in flight per lane: 256 agents per wave and round
constexpr int kLocGroup = 16;                    // lanes per newly infected agent; lane i of a group holds t_i
static_assert(GJ_MAX_NETS <= kLocGroup && kWave % kLocGroup == 0 && GJ_LOC_UNIT == (1ll << 30), "gj_location_stats");

// The loop the sparse per-agent kernels share (k_location_stats here, the three of gj_infector.h): a workgroup takes a
// contiguous share of the n agents in rounds of kLocLoads * 64 agents per wave; a lane reads flag[] for its agents
// (4 B per agent, coalesced), the wave ballots `flagged` over the round's 256 agents and hands the flagged ones to its
// four groups of kLocGroup lanes, four agents at a time: take(on, a, flag[a]) runs in EVERY lane of the wave - the sums
// of a group go through shuffles - with `on` false in a group that has no agent this time.
// kDenseFrom > 0: a round with at least that many flagged agents is not handed to the groups; every lane takes its own
// flagged agents, one after the other, with solo(a, flag[a]) - 64 agents side by side where the groups hold four.
struct NoSolo {
  __device__ void operator()(int64_t, float) const {}
};
template <int kDenseFrom = 0, typename Flagged, typename Take, typename Solo = NoSolo>
__device__ __forceinline__ void for_flagged_agents(int64_t n, const float* __restrict__ flag, Flagged flagged, Take take,
                                                   Solo solo = Solo()) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, waves = blockDim.x / kWave;
  const int slot = lane / kLocGroup;
  const int64_t round = (int64_t)kLocLoads * kWave;
  int64_t per = (n + gridDim.x - 1) / gridDim.x;
  per = (per + round - 1) / round * round;
  const int64_t u0 = (int64_t)blockIdx.x * per, u1 = (u0 + per < n) ? u0 + per : n;
  for (int64_t base = u0 + wave * round; base < u1; base += waves * round) {
    float nu[kLocLoads];
    unsigned long long m[kLocLoads], any = 0;
#pragma unroll
    for (int j = 0; j < kLocLoads; ++j) {
      const int64_t i = base + j * kWave + lane;
      nu[j] = i < u1 ? flag[i] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kLocLoads; ++j) any |= m[j] = __ballot(flagged(nu[j]));
    if (kDenseFrom > 0) {
      int count = 0;
#pragma unroll
      for (int j = 0; j < kLocLoads; ++j) count += __popcll(m[j]);
      if (count >= kDenseFrom) {                       // (uniform over the wave)
#pragma unroll
        for (int j = 0; j < kLocLoads; ++j)
          if (flagged(nu[j])) solo(base + j * kWave + lane, nu[j]);
        continue;
      }
    }
    while (any) {                                      // the round's flagged agents, one per group of lanes at a time
      bool on = false;
      int64_t a = 0;
      float v = 0.0f;
#pragma unroll
      for (int p = 0; p < kWave / kLocGroup; ++p) {
        bool found = false;
#pragma unroll
        for (int j = 0; j < kLocLoads; ++j) {
          if (found || !m[j]) continue;
          const int bit = __ffsll((long long)m[j]) - 1;
          m[j] &= m[j] - 1;
          found = true;
          const float x = __shfl(nu[j], bit, kWave);
          if (slot == p) on = true, a = base + j * kWave + bit, v = x;
        }
      }
      any = 0;
#pragma unroll
      for (int j = 0; j < kLocLoads; ++j) any |= m[j];
      take(on, a, v);
    }
  }
}

struct LocSet {                                  // one edge set with networks active in this step
  const int32_t* rowptr;                         // by-agent rows [n_agents + 1]; NULL: the set contributes nothing
  const int32_t* venue;                          // [n_edges], the set's own venue numbering
  const float* cum;                              // [n_venues][stride]
  int32_t n_edges, n_venues;
  int32_t stride, nk;                            // networks on the set: columns 0 .. nk of cum
  int32_t first;                                 // position of the set's first network in gj_step_params.nets
  int32_t _pad;
  int32_t mask[GJ_MAX_NETS_PER_SET];             // gj_mask_kind
  int32_t table[GJ_MAX_NETS_PER_SET];            // leisure table, -1: none
};

// w_n (receiving = true) or m_n (false) of gj_mask_kind for an agent of class c with quarantine factor q: 1 (RAW), q (Q),
// q * L[day_type][c] (QL), and on the receiving side that times (age > 75) (QL_AGE75).
__device__ __forceinline__ double mask_weight(int m, double q, int c, const float* tables, int table, int day_type,
                                              bool receiving) {
  double w = (m == GJ_MASK_RAW) ? 1.0 : q;
  if (m >= GJ_MASK_QL) w = w * (c < 200 ? (double)tables[(int64_t)table * GJ_TABLE_SIZE + day_type * 200 + c] : 0.0);
  if (receiving && m == GJ_MASK_QL_AGE75) w = w * (((c % 100) > 75) ? 1.0 : 0.0);
  return w;
}

// t_n[a] = w_n[a] * s0[a] * sum over a's edges of cum_n[v] for the network n == sub of the calling lane (0 for
// sub >= n_nets), by the group of kLocGroup lanes that holds agent a (`on` false: empty rows): the lanes stride over the
// edges of every set's row, the sums go through the group's butterfly.  Set: LocSet or a struct derived from it.
template <typename Set>
__device__ __forceinline__ double network_term(const Set* sets, int n_sets, bool on, int64_t a, int sub, double s0, double q,
                                               int c, const float* tables, int day_type, uint32_t& err) {
  double t = 0.0;
  for (int s = 0; s < n_sets; ++s) {
    const Set& S = sets[s];
    if (!S.rowptr) continue;                         // (uniform)
    int32_t r0 = 0, r1 = 0;
    if (on) {
      r0 = S.rowptr[a], r1 = S.rowptr[a + 1];
      if (r0 < 0 || r1 < r0 || r1 > S.n_edges) err |= kLocBadRows, r0 = r1 = 0;
    }
    double acc[GJ_MAX_NETS_PER_SET];
#pragma unroll
    for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) acc[k] = 0.0;
    for (int64_t e = (int64_t)r0 + sub; e < r1; e += kLocGroup) {   // the group's lanes stride over the agent's edges
      const int32_t v = S.venue[e];
      if ((uint32_t)v >= (uint32_t)S.n_venues) { err |= kLocBadRows; continue; }
      const float* row = S.cum + (int64_t)v * S.stride;
#pragma unroll
      for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k)
        if (k < S.nk) acc[k] += (double)row[k];
    }
#pragma unroll
    for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
      if (k >= S.nk) continue;                       // (nk is uniform: whole waves skip)
      const double sum = group_sum<kLocGroup>(acc[k]);
      double tk = mask_weight(S.mask[k], q, c, tables, S.table[k], day_type, true) * s0 * sum;
      if (!(tk >= 0.0)) { tk = 0.0; err |= kLocBadValue; }      // NaN or negative: counts as 0
      if (sub == S.first + k) t = tk;
    }
  }
  return t;
}

struct LocArgs {
  int64_t n;
  const float* nu;                               // new_infected
  const float* s0;                               // susceptibility before the step
  const float* stage;                            // NULL iff !has_q
  const int32_t* group;                          // NULL: every agent in group 0
  const uint8_t* cls;                            // agent_class (NULL: no tabled network)
  const float* tables;
  unsigned long long* out;                       // [n_groups][n_cols]
  uint32_t* err;
  int32_t n_groups, n_cols, n_nets, background;
  int32_t n_sets, has_q, day_type;
  float q_thr;
  int32_t cols[GJ_MAX_NETS];
  LocSet sets[GJ_MAX_SETS];
};

// LDS: the workgroup adds into a histogram of n_groups * n_cols 64-bit bins and flushes its non-zero bins at the end;
// otherwise every add is a global 64-bit atomic.  Integer adds: no order of the agents or of the workgroups shows.
template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_location_stats(const LocArgs A) {
  extern __shared__ unsigned long long loc_hist[];     // LDS: [n_groups * n_cols]
  const int bins = LDS ? A.n_groups * A.n_cols : 0;
  if (LDS) {
    for (int i = threadIdx.x; i < bins; i += blockDim.x) loc_hist[i] = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x % kWave;
  const int sub = lane % kLocGroup, first_lane = lane - sub;
  uint32_t err = 0;
  int col = 0;                                         // the output column of this lane's network (sub < n_nets)
#pragma unroll
  for (int i = 0; i < GJ_MAX_NETS; ++i)
    if (sub == i) col = A.cols[i];
  auto add = [&](int g, int c, unsigned long long units) {
    const int64_t bin = (int64_t)g * A.n_cols + c;
    if (LDS) atomicAdd(&loc_hist[bin], units);
    else atomicAdd(&A.out[bin], units);
  };
  // One newly infected agent per group of kLocGroup lanes (`on`: this group has one; a and nu are the same in its
  // lanes).  Every lane of the wave runs all of it - the sums go through shuffles - so an agent that is refused, and
  // a group without one, walk empty rows instead of leaving.
  auto take = [&](bool on, int64_t a, float nu) {
    if (on && nu != 1.0f) err |= kLocBadValue, on = false;
    int g = 0, c = 0;
    double s0 = 0.0, q = 0.0;
    if (on) {
      g = A.group ? A.group[a] : 0;
      if ((uint32_t)g >= (uint32_t)A.n_groups) err |= kLocBadLabel, on = false;
    }
    if (on) {
      s0 = (double)A.s0[a];
      q = (!A.has_q || A.stage[a] < A.q_thr) ? 1.0 : 0.0;
      c = A.cls ? A.cls[a] : 0;
    }
    const double t = network_term(A.sets, A.n_sets, on, a, sub, s0, q, c, A.tables, A.day_type, err);   // t_n, n == sub
    double T = 0.0, t_best = 0.0;                      // T in the order of nets; the largest term, lowest index on a tie
    int best = 0;
    for (int i = 0; i < A.n_nets; ++i) {
      const double ti = __shfl(t, first_lane + i, kWave);
      T += ti;
      if (i == 0 || ti > t_best) t_best = ti, best = i;
    }
    const bool shared = T > 0.0 && T < HUGE_VAL;
    const unsigned long long unit = (unsigned long long)GJ_LOC_UNIT;
    unsigned long long units = (shared && sub < A.n_nets) ? (unsigned long long)floor(t / T * (double)GJ_LOC_UNIT) : 0ull;
    const unsigned long long given = group_sum<kLocGroup>(units);
    if (!on) return;
    if (shared) {
      if (sub == best) units += unit - given;          // every infection contributes exactly one unit of 2^30
      if (units) add(g, col, units);
    } else if (sub == 0) {
      add(g, A.background, unit);                      // nobody transmitted: the reference's probability floor
    }
  };
  for_flagged_agents(A.n, A.nu, [](float x) { return x != 0.0f; }, take);   // (NaN is flagged too, and refused in take)
  if (err) atomicOr(A.err, err);
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += blockDim.x) {
      const unsigned long long v = loc_hist[i];
      if (v) atomicAdd(&A.out[i], v);
    }
  }
}

}  // namespace gj
