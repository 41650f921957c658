// Transmission trees (gj_infection_tree): one SAMPLED infector per new infection, where gj_infector.h hands every
// infectious agent its expected share.  The same launch point and the same loop: every agent a with new_infected == 1 is
// taken by a group of kLocGroup lanes, which
//   1. forms t_i, T and the integer shares u_{i,e} of gj_infector_scatter - through network_term and mask_weight, the
//      very functions - and picks ONE (venue, network) pair with probability u / 2^30 (the largest pair takes the
//      remainder too: its cell of U), from 30 bits of a Philox block of the agent's own;
//   2. walks that venue's members (the by-venue rows, gj_venue_rows) and picks ONE of them with probability W_b / S,
//      W_b = floor(m_i[b] * transmission[b] * 2^36), from 64 further bits of the same block.
// W_b / S is m * transmission / (the venue's sum) up to the 2^-36 floor, so the expectation of the sample is the credit
// gj_infector_gather gives b: summed over many runs the tree's offspring counts converge to `caused`.
// Every choice is made on integers - prefix sums of u and of W against an integer draw - so neither the lanes that walk a
// row nor the order of the agents shows in the result.  Nothing of gj_tiled.h is involved.
#pragma once
#include "gj_location.h"

namespace gj {

constexpr int kTreeMaxRow = GJ_TREE_MAX_VENUE_ROW;
constexpr int kTreeBatch = 4;                    // members of a venue row in flight per lane
constexpr int kTreeLong = kTreeBatch * kWave;    // a venue row longer than this is walked by the whole wave
constexpr int kTreeWeightBits = 36, kTreeWeightCap = 46;     // W = min(floor(w * 2^36), 2^46); 2^18 members: S < 2^64
static_assert((1ll << 18) == GJ_TREE_MAX_VENUE_ROW && GJ_LOC_MAX_COLS <= kThreads, "gj_infection_tree");

struct TreeSet : LocSet {                        // LocSet, and the way back through the venue
  const int32_t* v_rowptr;                       // by-venue rows [n_venues + 1]; NULL: no member is found (unresolved)
  const int32_t* v_agent;                        // [n_edges], owned agents
};

struct TreeArgs {
  int64_t n;
  const float* flag;                             // new_infected
  const float* s0;                               // susceptibility before the step
  const float* stage;                            // NULL iff !has_q
  const float* tr;                               // the step's transmission
  const uint8_t* cls;
  const float* tables;
  int32_t* infector;                             // [n]: global id, -2: nobody transmitted, -3: unresolved
  int32_t* via;                                  // [n]: location column
  int32_t* venue;                                // [n]: venue in its set's numbering, -1 with -2
  int32_t* row_of;                               // [n]
  unsigned long long* counts;                    // [n_cols]
  unsigned long long* unresolved;
  uint32_t* err;
  uint64_t seed, step;
  int64_t agent_offset;
  int32_t n_cols, n_nets, n_sets, has_q, day_type, background, row_value;
  float q_thr;
  int32_t cols[GJ_MAX_NETS];
  TreeSet sets[GJ_MAX_SETS];                     // in the order of plan->sets: the canonical order of the pairs
};

// exclusive prefix sum over an aligned group of G lanes, in lane order (integers: exact); sub: the lane's index in it
template <int G>
__device__ __forceinline__ unsigned long long lanes_exclusive_scan(unsigned long long v, int sub) {
  unsigned long long x = v;
#pragma unroll
  for (int off = 1; off < G; off <<= 1) {
    const unsigned long long y = __shfl_up(x, off, G);
    if (sub >= off) x += y;
  }
  return x - v;
}
__device__ __forceinline__ unsigned long long group_exclusive_scan(unsigned long long v, int sub) {
  return lanes_exclusive_scan<kLocGroup>(v, sub);
}

// the value `v` of the one lane of the group with `mine` set (`first_lane`: the group's first; no such lane: of that one)
__device__ __forceinline__ int group_pick(bool mine, int v, int first_lane) {
  const unsigned long long b = (__ballot(mine) >> first_lane) & ((1ull << kLocGroup) - 1);
  return __shfl(v, first_lane + (b ? __ffsll((long long)b) - 1 : 0), kWave);
}

__global__ __launch_bounds__(kThreads) void k_infection_tree(const TreeArgs A) {
  __shared__ unsigned long long tree_hist[GJ_LOC_MAX_COLS];
  for (int i = threadIdx.x; i < A.n_cols; i += blockDim.x) tree_hist[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x % kWave;
  const int sub = lane % kLocGroup, first_lane = lane - sub;
  uint32_t err = 0;
  unsigned long long open = 0;                         // unresolved infections, counted by this lane
  // A venue row is taken kTreeBatch * kLocGroup members at a time: a lane first loads its kTreeBatch members, then their
  // transmissions - independent loads, all in flight together; a walk is a chain of dependent loads, not bytes - and
  // reads the mask's inputs (stage, class, table) only for the few members that transmit at all.
  // load: the lane's members of the batch at `base` and their transmissions (0 for no member, or a bad one)
  // (idx of width: the lane's place among the lanes that walk the row together - a group, or the whole wave)
  auto load = [&](const int32_t* members, int32_t base, int32_t len, int idx, int width, int32_t (&b)[kTreeBatch],
                  float (&tr)[kTreeBatch]) {
#pragma unroll
    for (int j = 0; j < kTreeBatch; ++j) {
      const int32_t pos = base + j * width + idx;
      b[j] = pos < len ? members[pos] : -1;
      if (pos < len && (b[j] < 0 || b[j] >= A.n)) err |= kLocBadRows, b[j] = -1;
    }
#pragma unroll
    for (int j = 0; j < kTreeBatch; ++j) tr[j] = b[j] >= 0 ? A.tr[b[j]] : 0.0f;
  };
  // W_b of member b, transmitting tr, of a venue for the network (mask, table) and the infected agent a
  auto weight = [&](int32_t b, float tr, int64_t a, int mask, int table) -> unsigned long long {
    if (tr == 0.0f || b == a) return 0ull;             // (0 times any weight is 0, or NaN: no weight either way)
    const double q = (!A.has_q || A.stage[b] < A.q_thr) ? 1.0 : 0.0;
    const int c = A.cls ? A.cls[b] : 0;
    const double w = mask_weight(mask, q, c, A.tables, table, A.day_type, false) * (double)tr;
    if (!(w > 0.0)) return 0ull;                       // (NaN too)
    const double x = w * (double)(1ull << kTreeWeightBits);
    if (x >= (double)(1ull << kTreeWeightCap)) { err |= kLocBadValue; return 1ull << kTreeWeightCap; }
    return (unsigned long long)floor(x);
  };
  // Every lane of the wave runs all of it, as in the sibling kernels: a group without an agent, or with a refused one,
  // walks empty rows.  The loops over a row run while ANY group of the wave has edges left.
  auto take = [&](bool on, int64_t a, float nu) {
    if (on && nu != 1.0f) err |= kLocBadValue, on = false;
    int c = 0;
    double s0 = 0.0, q = 0.0;
    if (on) {
      s0 = (double)A.s0[a];
      q = (!A.has_q || A.stage[a] < A.q_thr) ? 1.0 : 0.0;
      c = A.cls ? A.cls[a] : 0;
    }
    const double t = network_term(A.sets, A.n_sets, on, a, sub, s0, q, c, A.tables, A.day_type, err);
    double T = 0.0;                                    // in the order of nets, as the location kernel adds them
    for (int i = 0; i < A.n_nets; ++i) T += __shfl(t, first_lane + i, kWave);
    const bool shared = on && T > 0.0 && T < HUGE_VAL;
    uint32_t r[4] = {0, 0, 0, 0};
    if (shared) philox4x32_10((uint64_t)(A.agent_offset + a), A.step | (1ull << 60), A.seed, r);
    const unsigned long long unit = (unsigned long long)GJ_LOC_UNIT;
    const unsigned long long r1 = r[0] & (uint32_t)(unit - 1), R = (unsigned long long)r[2] | ((unsigned long long)r[3] << 32);
    // the one walk: the pairs in canonical order - set, position in the row, network column - against r1; the largest
    // term as the scatter tracks it.  hit / best: (set << 8 | network << 4 | column) and the venue of this lane's candidate
    unsigned long long given = 0;                      // (the same in every lane of the group)
    double best_t = -1.0;
    unsigned long long best_key = ~0ull;               // (network << 32) | position in the row: lowest wins a tie
    int best_pair = -1, best_v = -1, hit_pair = -1, hit_v = -1;
    for (int s = 0; s < A.n_sets; ++s) {
      const TreeSet& S = A.sets[s];
      if (!S.rowptr) continue;                         // (uniform)
      int32_t r0 = 0, len = 0;
      if (shared) {
        r0 = S.rowptr[a];
        const int32_t re = S.rowptr[a + 1];
        len = (r0 < 0 || re < r0 || re > S.n_edges) ? 0 : re - r0;      // (reported by the first walk)
      }
      double ws[GJ_MAX_NETS_PER_SET];                  // w_k * s0, 0 for a network that scatters nothing
#pragma unroll
      for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
        ws[k] = 0.0;
        if (k >= S.nk) continue;
        const double tk = __shfl(t, first_lane + S.first + k, kWave);
        if (tk > 0.0) ws[k] = mask_weight(S.mask[k], q, c, A.tables, S.table[k], A.day_type, true) * s0;
      }
      for (int32_t base = 0; __any(base < len); base += kLocGroup) {      // chunks of kLocGroup positions
        const int32_t pos = base + sub;
        int32_t v = -1;
        if (pos < len) {
          v = S.venue[(int64_t)r0 + pos];
          if ((uint32_t)v >= (uint32_t)S.n_venues) v = -1;
        }
        unsigned long long u[GJ_MAX_NETS_PER_SET], mine = 0;
#pragma unroll
        for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
          u[k] = 0;
          if (k >= S.nk || v < 0 || !(ws[k] > 0.0)) continue;
          double te = ws[k] * (double)S.cum[(int64_t)v * S.stride + k];
          if (!(te >= 0.0)) { te = 0.0; err |= kLocBadValue; }
          const double x = te / T * (double)GJ_LOC_UNIT;
          u[k] = x >= (double)GJ_LOC_UNIT ? unit : (unsigned long long)floor(x);
          mine += u[k];
          const unsigned long long key = ((unsigned long long)(S.first + k) << 32) | (unsigned long long)pos;
          if (te > best_t || (te == best_t && key < best_key)) best_t = te, best_key = key, best_pair = s << 8 | (S.first + k) << 4 | k, best_v = v;
        }
        unsigned long long before = given + group_exclusive_scan(mine, sub);
#pragma unroll
        for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
          if (k >= S.nk) continue;
          if (before <= r1 && r1 < before + u[k]) hit_pair = s << 8 | (S.first + k) << 4 | k, hit_v = v;
          before += u[k];
        }
        given += group_sum<kLocGroup>(mine);
      }
    }
    const unsigned long long my_key = best_key;
#pragma unroll
    for (int off = kLocGroup / 2; off > 0; off >>= 1) {      // the group's largest term, lowest key on a tie
      const double ot = __shfl_xor(best_t, off, kWave);
      const unsigned long long ok = __shfl_xor(best_key, off, kWave);
      if (ot > best_t || (ot == best_t && ok < best_key)) best_t = ot, best_key = ok;
    }
    const bool by_prefix = r1 < given;
    const bool owner = by_prefix ? hit_pair >= 0 : (best_pair >= 0 && my_key == best_key);
    int pair = group_pick(owner, by_prefix ? hit_pair : best_pair, first_lane);
    const int v = group_pick(owner, by_prefix ? hit_v : best_v, first_lane);
    if (!shared || v < 0) pair = -1;                   // nobody transmitted
    // the venue's members: their weights summed, then the first whose inclusive prefix sum exceeds the target
    int32_t found = -1;
    bool resolved = false;
    for (int s = 0; s < A.n_sets; ++s) {
      const TreeSet& S = A.sets[s];
      const bool here = pair >= 0 && (pair >> 8) == s && S.v_rowptr != nullptr;
      const int k = pair & 15;
      int32_t m0 = 0, len = 0;
      if (here) {
        m0 = S.v_rowptr[v];
        const int32_t me = S.v_rowptr[v + 1];
        if (m0 < 0 || me < m0 || me > S.n_edges || me - m0 > kTreeMaxRow) err |= kLocBadRows;
        else len = me - m0;
      }
      if (!__any(len > 0)) continue;
      int mask = 0, table = -1;
#pragma unroll
      for (int j = 0; j < GJ_MAX_NETS_PER_SET; ++j)
        if (j == k) mask = S.mask[j], table = S.table[j];
      // A long row - more than one batch of the whole wave - is taken by the whole wave, one such row after the other:
      // the launch ends with its longest row, which 64 lanes walk in a quarter of the steps.  The same integers in the
      // same row order: the result cannot differ.
      const bool is_long = len > kTreeLong;
      const int32_t long_len = is_long ? len : 0;
      if (is_long) len = 0;
      for (unsigned long long todo = __ballot(is_long && sub == 0); todo; todo &= todo - 1) {
        const int src = __ffsll((long long)todo) - 1;
        const int32_t L = __shfl(long_len, src, kWave), M0 = __shfl(m0, src, kWave);
        const int64_t a_l = __shfl((long long)a, src, kWave);
        const unsigned long long R_l = __shfl(R, src, kWave);
        const int mask_l = __shfl(mask, src, kWave), table_l = __shfl(table, src, kWave);
        const int32_t* members = S.v_agent + M0;
        int32_t b[kTreeBatch];
        float tr[kTreeBatch];
        unsigned long long sum = 0;
        for (int32_t base = 0; base < L; base += kTreeBatch * kWave) {
          load(members, base, L, lane, kWave, b, tr);
#pragma unroll
          for (int j = 0; j < kTreeBatch; ++j) sum += weight(b[j], tr[j], a_l, mask_l, table_l);
        }
        sum = wave_sum(sum);
        if (sum == 0) continue;                          // (uniform) unresolved
        const unsigned long long target = __umul64hi(R_l, sum);
        unsigned long long before = 0;
        int32_t mine = -1;
        for (int32_t base = 0; base < L && before <= target; base += kTreeBatch * kWave) {
          load(members, base, L, lane, kWave, b, tr);
#pragma unroll
          for (int j = 0; j < kTreeBatch; ++j) {         // kWave consecutive members at a time, in row order
            const unsigned long long w = weight(b[j], tr[j], a_l, mask_l, table_l);
            const unsigned long long lo = before + lanes_exclusive_scan<kWave>(w, lane);
            if (lo <= target && target < lo + w) mine = b[j];
            before += wave_sum(w);
          }
        }
        const unsigned long long who = __ballot(mine >= 0);
        const int32_t got = __shfl(mine, who ? __ffsll((long long)who) - 1 : 0, kWave);
        if (first_lane == src) found = got, resolved = true;
      }
      if (!__any(len > 0)) continue;
      const int32_t* members = S.v_agent + m0;
      int32_t b[kTreeBatch];
      float tr[kTreeBatch];
      unsigned long long w[kTreeBatch], sum = 0;
      for (int32_t base = 0; __any(base < len); base += kTreeBatch * kLocGroup) {
        load(members, base, len, sub, kLocGroup, b, tr);
#pragma unroll
        for (int j = 0; j < kTreeBatch; ++j) sum += w[j] = weight(b[j], tr[j], a, mask, table);
      }
      // (most venues - a household, a small company - are one batch: its members and weights are still in registers)
      const bool again = __any(len > kTreeBatch * kLocGroup);
      sum = group_sum<kLocGroup>(sum);
      if (sum == 0) len = 0;
      const unsigned long long target = __umul64hi(R, sum);
      unsigned long long before = 0;
      int32_t mine = -1;
      for (int32_t base = 0; __any(base < len); base += kTreeBatch * kLocGroup) {
        if (again) {
          load(members, base, len, sub, kLocGroup, b, tr);
#pragma unroll
          for (int j = 0; j < kTreeBatch; ++j) w[j] = weight(b[j], tr[j], a, mask, table);
        }
#pragma unroll
        for (int j = 0; j < kTreeBatch; ++j) {         // kLocGroup consecutive members at a time, in row order
          const unsigned long long lo = before + group_exclusive_scan(w[j], sub);
          if (len > 0 && lo <= target && target < lo + w[j]) mine = b[j];
          before += group_sum<kLocGroup>(w[j]);
        }
        if (before > target) len = 0;                  // (the same in every lane of the group: found)
      }
      const int32_t got = group_pick(mine >= 0, mine, first_lane);
      if (here && sum != 0) found = got, resolved = true;
    }
    if (!on || sub != 0) return;
    int col = A.background;
    if (pair >= 0) {
      const int net = (pair >> 4) & 15;
#pragma unroll
      for (int i = 0; i < GJ_MAX_NETS; ++i)
        if (i == net) col = A.cols[i];
    }
    A.infector[a] = pair < 0 ? -2 : resolved ? (int32_t)(A.agent_offset + found) : -3;
    A.via[a] = col;
    A.venue[a] = pair < 0 ? -1 : v;
    A.row_of[a] = A.row_value;
    if (pair >= 0 && !resolved) ++open;
    atomicAdd(&tree_hist[col], 1ull);
  };
  for_flagged_agents(A.n, A.flag, [](float x) { return x != 0.0f; }, take);   // (NaN is flagged too, and refused in take)
  if (err) atomicOr(A.err, err);
  if (open) atomicAdd(A.unresolved, open);
  __syncthreads();
  for (int i = threadIdx.x; i < A.n_cols; i += blockDim.x) {
    const unsigned long long n = tree_hist[i];
    if (n) atomicAdd(&A.counts[i], n);
  }
}

}  // namespace gj
