// Infector attribution (gj_infector_scatter / gj_infector_gather / gj_infector_clear): the step's new infections carried
// one level further than gj_location.h does - through the venue, to the agents who transmitted.  The transpose of the
// location kernel, with the structure of the backward pass: a scatter of every new infection's unit of 2^30 into 64-bit
// integers per (venue, network) - U - then a gather per infectious agent of its share of the U of its venues.  Both
// are sparse: they touch the step's new infections and the currently infectious agents, through the loop and the
// per-network terms of gj_location.h.  Nothing of gj_tiled.h is involved.
// The who-infects-whom matrix (gj_infection_matrix_scatter / _gather / _clear) is the same two passes with the units kept
// apart by the group of the INFECTED agent - UG [n_venues][stride][G] beside U - so that pass 2 sums over pairs of groups:
// the same kernels, instantiated with kMatrix.
#pragma once
#include "gj_location.h"

namespace gj {

struct InfSet : LocSet {                         // LocSet, and what the way back through the venue needs
  const float* pc;                               // v_pcontact [n_venues]
  unsigned long long* U;                         // [n_venues][stride]
  unsigned long long* UG;                        // matrix: [n_venues][stride][n_groups], the units by the infected's group
  float beta[GJ_MAX_NETS_PER_SET];
};

struct InfArgs {
  int64_t n;
  const float* flag;                             // scatter, clear: new_infected; gather: transmission
  const float* s0;                               // scatter: susceptibility before the step
  const float* stage;                            // NULL iff !has_q
  const int32_t* group;                          // gather, matrix scatter; NULL: every agent in group 0
  const uint8_t* cls;
  const float* tables;
  double* caused;                                // gather, or NULL
  unsigned long long* out;                       // gather: [n_groups], or NULL; matrix gather: [n_groups][n_groups]
  unsigned long long* unattributed;              // scatter; matrix scatter: [n_groups], or NULL
  int32_t* cohort;                               // scatter, or NULL
  uint32_t* err;
  int32_t n_groups, n_nets, n_sets, has_q, day_type, cohort_value;
  float q_thr;
  int32_t _pad;
  InfSet sets[GJ_MAX_SETS];
};

// Pass 1.  One newly infected agent per group of kLocGroup lanes: t_i and T exactly as k_location_stats forms them, then
// a second walk over the same rows that splits the infection's 2^30 units over the (edge, network) pairs in proportion
// to t_{i,e} = w_i * s0 * cum_i[v_e] and adds them to U with 64-bit integer atomics: no order of the agents or of the
// workgroups shows in U.
// kMatrix: the same infection, the same t_i, T, floors, remainder and tie-break, added to UG[v][k][group[a]] instead of
// U[v][k] - so UG sums over the groups to U, cell by cell - and counted in unattributed[group[a]] when nobody transmitted
// it.  No cohort is written and U is not touched.
template <bool kMatrix>
__global__ __launch_bounds__(kThreads) void k_infector_scatter(const InfArgs A) {
  const int lane = threadIdx.x % kWave;
  const int sub = lane % kLocGroup, first_lane = lane - sub;
  uint32_t err = 0;
  unsigned long long lost = 0;                         // infections nobody transmitted, counted by this lane
  auto take = [&](bool on, int64_t a, float nu) {
    if (on && nu != 1.0f) err |= kLocBadValue, on = false;
    int c = 0, g = 0;
    double s0 = 0.0, q = 0.0;
    if (kMatrix && on) {
      g = A.group ? A.group[a] : 0;
      if ((uint32_t)g >= (uint32_t)A.n_groups) err |= kLocBadLabel, on = false;
    }
    if (on) {
      s0 = (double)A.s0[a];
      q = (!A.has_q || A.stage[a] < A.q_thr) ? 1.0 : 0.0;
      c = A.cls ? A.cls[a] : 0;
      if (!kMatrix && sub == 0 && A.cohort) A.cohort[a] = A.cohort_value;
    }
    const double t = network_term(A.sets, A.n_sets, on, a, sub, s0, q, c, A.tables, A.day_type, err);
    double T = 0.0;                                    // in the order of nets, as the location kernel adds them
    for (int i = 0; i < A.n_nets; ++i) T += __shfl(t, first_lane + i, kWave);
    const bool shared = T > 0.0 && T < HUGE_VAL;
    const unsigned long long unit = (unsigned long long)GJ_LOC_UNIT;
    // the second walk: this lane's edges again (the lines are in cache).  A network whose t_i is 0 - by its mask, or
    // refused as NaN or negative - scatters nothing; the lane keeps its largest term for the remainder
    unsigned long long given = 0, *best_cell = nullptr;
    double best_t = -1.0;
    unsigned long long best_key = ~0ull;               // (network << 32) | position in the row: lowest wins a tie
    for (int s = 0; s < A.n_sets; ++s) {
      const InfSet& S = A.sets[s];
      if (!S.rowptr) continue;                         // (uniform)
      int32_t r0 = 0, r1 = 0;
      if (on && shared) {
        r0 = S.rowptr[a], r1 = S.rowptr[a + 1];
        if (r0 < 0 || r1 < r0 || r1 > S.n_edges) r0 = r1 = 0;      // (reported by the first walk)
      }
      double ws[GJ_MAX_NETS_PER_SET];                  // w_k * s0, 0 for a network that scatters nothing
#pragma unroll
      for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
        ws[k] = 0.0;
        if (k >= S.nk) continue;
        const double tk = __shfl(t, first_lane + S.first + k, kWave);
        if (tk > 0.0) ws[k] = mask_weight(S.mask[k], q, c, A.tables, S.table[k], A.day_type, true) * s0;
      }
      for (int64_t e = (int64_t)r0 + sub; e < r1; e += kLocGroup) {
        const int32_t v = S.venue[e];
        if ((uint32_t)v >= (uint32_t)S.n_venues) continue;
        const float* row = S.cum + (int64_t)v * S.stride;
        // (g is 0 and the set's UG unused unless kMatrix)
        unsigned long long* cell = kMatrix ? S.UG + (int64_t)v * S.stride * A.n_groups + g : S.U + (int64_t)v * S.stride;
        const int64_t step = kMatrix ? A.n_groups : 1;               // from one network column of the venue to the next
#pragma unroll
        for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
          if (k >= S.nk || !(ws[k] > 0.0)) continue;
          double te = ws[k] * (double)row[k];
          if (!(te >= 0.0)) { te = 0.0; err |= kLocBadValue; }
          const double r = te / T * (double)GJ_LOC_UNIT;
          const unsigned long long u = r >= (double)GJ_LOC_UNIT ? unit : (unsigned long long)floor(r);
          if (u) atomicAdd(cell + k * step, u);
          given += u;
          const unsigned long long key = ((unsigned long long)(S.first + k) << 32) | (unsigned long long)(e - r0);
          if (te > best_t || (te == best_t && key < best_key)) best_t = te, best_key = key, best_cell = cell + k * step;
        }
      }
    }
    given = group_sum<kLocGroup>(given);
    const unsigned long long my_key = best_key;
#pragma unroll
    for (int off = kLocGroup / 2; off > 0; off >>= 1) {      // the group's largest term, lowest key on a tie
      const double ot = __shfl_xor(best_t, off, kWave);
      const unsigned long long ok = __shfl_xor(best_key, off, kWave);
      if (ot > best_t || (ot == best_t && ok < best_key)) best_t = ot, best_key = ok;
    }
    if (!on) return;
    if (shared) {      // every attributed infection scatters exactly 2^30 (given > unit: negative sums in cum, reported)
      if (best_cell && my_key == best_key && given < unit) atomicAdd(best_cell, unit - given);
    } else if (sub == 0) {
      if (!kMatrix) ++lost;
      else if (A.unattributed) atomicAdd(A.unattributed + g, 1ull);
    }
  };
  for_flagged_agents(A.n, A.flag, [](float x) { return x != 0.0f; }, take);   // (NaN is flagged too, and refused in take)
  if (err) atomicOr(A.err, err);
  if (lost) atomicAdd(A.unattributed, lost);
}

// The step's U back to zero by the way it was filled: the rows of the flagged agents again, plain stores of 0 into every
// column of the venues they name.
// kMatrix: UG instead - a venue has stride * n_groups cells of 8 B in a row: the group's lanes take the agent's edges one
// after the other and stride over the venue's cells together (whole cache lines per store instruction).
template <bool kMatrix>
__global__ __launch_bounds__(kThreads) void k_infector_clear(const InfArgs A) {
  const int sub = threadIdx.x % kLocGroup;
  auto take = [&](bool on, int64_t a, float) {
    if (!on) return;
    for (int s = 0; s < A.n_sets; ++s) {
      const InfSet& S = A.sets[s];
      if (!S.rowptr) continue;
      const int32_t r0 = S.rowptr[a], r1 = S.rowptr[a + 1];
      if (r0 < 0 || r1 < r0 || r1 > S.n_edges) continue;
      if (kMatrix) {
        const int64_t cells = (int64_t)S.stride * A.n_groups;
        for (int64_t e = r0; e < r1; ++e) {
          const int32_t v = S.venue[e];
          if ((uint32_t)v >= (uint32_t)S.n_venues) continue;
          for (int64_t k = sub; k < cells; k += kLocGroup) S.UG[(int64_t)v * cells + k] = 0ull;
        }
        continue;
      }
      for (int64_t e = (int64_t)r0 + sub; e < r1; e += kLocGroup) {
        const int32_t v = S.venue[e];
        if ((uint32_t)v >= (uint32_t)S.n_venues) continue;
        for (int k = 0; k < S.stride; ++k) S.U[(int64_t)v * S.stride + k] = 0ull;
      }
    }
  };
  for_flagged_agents(A.n, A.flag, [](float x) { return x != 0.0f; }, take);
}

// Pass 2.  One infectious agent b per group of lanes: over its rows, wherever a venue's U is not zero,
//   U / 2^30 * beta_i * pc[v] * m_i[b] * transmission[b] / cum_i[v]
// - b's share of what the venue's new infections scattered there - summed in fp64 over the group.  Then caused[b] +=
// credit (one group per agent: a plain read-modify-write) and out[group[b]] += llrint(credit * 2^30) as 64-bit integers:
// through an LDS histogram of n_groups bins, or with global atomics.
// Late in an epidemic a third of the agents are infectious, and four agents per wave at a time are too few chains of
// dependent loads (row pointers, venue ids, U) in flight: a round of 256 agents with kInfDense or more infectious ones
// is taken one agent per LANE instead - a lane walks its agents' rows alone, edge by edge.  (Measured on the 10 M-agent
// C3 world, same run: groups alone 204 us at 1 % infected and 3449 us at 30 %; lanes alone 445 us and 1289 us; this
// kernel 221 us and 1287 us.  profiles/ab_infector_gather_forms.json, profiles/infector_c3_10m.json.)
// kMatrix (always LDS: n_groups^2 <= kLocLdsBins): the same walk, and where U is not zero the venue's n_groups cells of UG
// each give a term of their own - the expression above with UG[v][k][g'] for U - rounded on its own and added to
// bin [group[b]][g'] as it is formed: sums of integers, so neither form of the walk nor any order shows in out.  Nothing
// is summed per agent then, and caused is not written.
constexpr int kInfDense = 16;
template <bool LDS, bool kMatrix = false>
__global__ __launch_bounds__(kThreads) void k_infector_gather(const InfArgs A) {
  static_assert(LDS || !kMatrix, "the matrix is summed in LDS");
  extern __shared__ unsigned long long inf_hist[];     // LDS: [n_groups], kMatrix: [n_groups][n_groups]
  const int bins = !LDS ? 0 : kMatrix ? A.n_groups * A.n_groups : A.n_groups;
  if (LDS) {
    for (int i = threadIdx.x; i < bins; i += blockDim.x) inf_hist[i] = 0;
    __syncthreads();
  }
  const int sub = threadIdx.x % kLocGroup;
  uint32_t err = 0;
  // the share of `units` at a venue that goes to an agent transmitting w = m * transmission there
  auto share = [](unsigned long long units, double beta_pc, double w, double cum) -> double {
    return (double)units / (double)GJ_LOC_UNIT * beta_pc * w / cum;
  };
  // what agent b (of group g) of class c gets from network k of set S at venue v
  auto term = [&](const InfSet& S, int32_t v, int k, double q, int c, float tr, int g) -> double {
    const int64_t cell = (int64_t)v * S.stride + k;
    const unsigned long long u = S.U[cell];
    if (!u) return 0.0;                                // cum is read at the few venues with a new infection only
    const double cum = (double)S.cum[cell];
    if (!(cum > 0.0 && cum < HUGE_VAL)) { err |= kLocBadValue; return 0.0; }      // cannot follow from pass 1
    const double m = mask_weight(S.mask[k], q, c, A.tables, S.table[k], A.day_type, false);
    const double beta_pc = (double)S.beta[k] * (double)S.pc[v], w = m * (double)tr;
    if (!kMatrix) return share(u, beta_pc, w, cum);
    const unsigned long long* by_group = S.UG + cell * A.n_groups;
    for (int h = 0; h < A.n_groups; ++h) {             // straight into the histogram: no per-lane array over g'
      const unsigned long long ug = by_group[h];
      if (!ug) continue;
      const double t = share(ug, beta_pc, w, cum) * (double)GJ_LOC_UNIT;
      if (!(t >= 0.0 && t < (double)(1ll << 62))) { err |= kLocBadValue; continue; }      // NaN, or beyond any step
      const unsigned long long units = (unsigned long long)llrint(t);
      if (units) atomicAdd(&inf_hist[g * A.n_groups + h], units);
    }
    return 0.0;
  };
  auto settle = [&](int64_t b, int g, double credit) {
    if (credit == 0.0) return;
    if (!(credit > 0.0 && credit < (double)(1ll << 32))) { err |= kLocBadValue; return; }   // NaN, or beyond any step
    if (A.caused) A.caused[b] += credit;
    if (A.out) {
      const unsigned long long units = (unsigned long long)llrint(credit * (double)GJ_LOC_UNIT);
      if (units) {
        if (LDS) atomicAdd(&inf_hist[g], units);
        else atomicAdd(&A.out[g], units);
      }
    }
  };
  auto take = [&](bool on, int64_t b, float tr) {
    int g = 0, c = 0;
    double q = 0.0;
    if (on) {
      g = A.group ? A.group[b] : 0;
      if ((uint32_t)g >= (uint32_t)A.n_groups) err |= kLocBadLabel, on = false;
    }
    if (on) {
      q = (!A.has_q || A.stage[b] < A.q_thr) ? 1.0 : 0.0;
      c = A.cls ? A.cls[b] : 0;
    }
    double acc = 0.0;
    for (int s = 0; s < A.n_sets; ++s) {
      const InfSet& S = A.sets[s];
      if (!S.rowptr) continue;                         // (uniform)
      int32_t r0 = 0, r1 = 0;
      if (on) {
        r0 = S.rowptr[b], r1 = S.rowptr[b + 1];
        if (r0 < 0 || r1 < r0 || r1 > S.n_edges) err |= kLocBadRows, r0 = r1 = 0;
      }
      for (int64_t e = (int64_t)r0 + sub; e < r1; e += kLocGroup) {
        const int32_t v = S.venue[e];
        if ((uint32_t)v >= (uint32_t)S.n_venues) { err |= kLocBadRows; continue; }
#pragma unroll
        for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k)
          if (k < S.nk) acc += term(S, v, k, q, c, tr, g);
      }
    }
    const double credit = group_sum<kLocGroup>(acc);      // (kMatrix: 0, nothing to settle)
    if (on && sub == 0) settle(b, g, credit);
  };
  auto solo = [&](int64_t b, float tr) {
    const int g = A.group ? A.group[b] : 0;
    if ((uint32_t)g >= (uint32_t)A.n_groups) { err |= kLocBadLabel; return; }
    const double q = (!A.has_q || A.stage[b] < A.q_thr) ? 1.0 : 0.0;
    const int c = A.cls ? A.cls[b] : 0;
    double credit = 0.0;
    for (int s = 0; s < A.n_sets; ++s) {
      const InfSet& S = A.sets[s];
      if (!S.rowptr) continue;
      const int32_t r0 = S.rowptr[b], r1 = S.rowptr[b + 1];
      if (r0 < 0 || r1 < r0 || r1 > S.n_edges) { err |= kLocBadRows; continue; }
      for (int32_t e = r0; e < r1; ++e) {
        const int32_t v = S.venue[e];
        if ((uint32_t)v >= (uint32_t)S.n_venues) { err |= kLocBadRows; continue; }
        for (int k = 0; k < S.nk; ++k) credit += term(S, v, k, q, c, tr, g);
      }
    }
    settle(b, g, credit);
  };
  for_flagged_agents<kInfDense>(A.n, A.flag, [](float x) { return x > 0.0f; }, take, solo);
  if (err) atomicOr(A.err, err);
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += blockDim.x) {
      const unsigned long long v = inf_hist[i];
      if (v) atomicAdd(&A.out[i], v);
    }
  }
}

}  // namespace gj
