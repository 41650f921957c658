// gfx950 (MI355X / CDNA4) kernels + C ABI for the per-timestep infection message-passing path
// of GradABM-JUNE.  ABI: include/gradjune_hip.h.  Reference semantics: SURVEY.md section 8a.
//
// Per step (gj_step): three dependent launches on the caller's stream
//   k_transmission    a1+a2   elementwise over agents           (HBM-bound, streaming)
//   k_venue_reduce    a3-a5   segmented sum per venue (pass 1)   (HBM/MALL-bound, index stream + gather)
//   [k_combine_long]          ordered combine of >2048-edge venues' partial sums
//   k_agent_gather    a4,a6-a9 per-agent gather over its venues + epilogue + Gumbel decision
//                              + state update (pass 2, fused)
// The path is a sparse segmented reduction: no MFMA.  The rules that matter are coalesced index
// streams, many independent gathers in flight, LDS staging of per-venue partial sums and wave64
// shuffles for the segmented combine.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/gradjune_hip.h"
#include "gj_device.h"
#include "gj_tiled.h"
#include "gj_agent.h"
#include "gj_location.h"
#include "gj_infector.h"
#include "gj_tree.h"
#include "gj_contact.h"
#include "gj_testing.h"

namespace gj {

// ------------------------------------------------------------------------------------------
// kernel-argument blocks (passed by value; < 4 KiB)
// ------------------------------------------------------------------------------------------
struct SetP1 {
  const int32_t* v_rowptr;
  const int32_t* v_agent;
  const float* v_pc;
  float* cum;
  int32_t stride;
  int32_t nk;                              // networks active on this set in this step
  float beta[GJ_MAX_NETS_PER_SET];
  int32_t table[GJ_MAX_NETS_PER_SET];      // -1: no leisure table
  int32_t raw;                             // 1: household (raw transmission), 0: q*transmission
  int32_t leisure;                         // 1: any network of the set uses a table
};

struct P1Args {
  SetP1 sets[GJ_MAX_SETS];
  const gj_block* blocks;
  const float* trans;
  const float* qtrans;
  const uint8_t* cls;
  const float* tables;
  float* partial;
  int32_t day_type;
};

struct SetP2 {
  const int32_t* a_rowptr;
  const int32_t* a_venue;
  const float* cum;
  int32_t stride;
  int32_t nk;
  int32_t mask[GJ_MAX_NETS_PER_SET];
  int32_t table[GJ_MAX_NETS_PER_SET];
};

struct P2Args {
  SetP2 groups[GJ_MAX_SETS];   // active edge sets in accumulation order
  int32_t n_groups;
  int32_t any_leisure;
  int64_t n_agents;
  const uint8_t* cls;
  const float* tables;
  const float* stage;
  float* susceptibility;
  float* is_infected;
  float* infection_time;
  float* not_infected_probs;
  float* new_infected;
  float* trans_susc;
  const float* exp_noise;
  float now, dt, q_thr;
  int32_t day_type, has_q, sample;
  uint64_t seed, step;
  int64_t agent_offset;
  const gj_clock* clock;
};

// ------------------------------------------------------------------------------------------
// a1 + a2   transmission profile and quarantine-masked copy
//   reference: grad_june/transmission.py:39-51, grad_june/policies/quarantine_policies.py:13-33
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float transmission_value(float mx, float shp, float rt, float sh, float t_inf,
                                                    float inf, float now) {
  const ProfileHead h = profile_head(shp, rt, sh, t_inf, now);
  return mx * h.sign * h.aux * h.aux2 * inf;
}

// (Round 3, measured and not adopted: listing a chunk's infected agents in LDS and evaluating them densely, one per
// lane, from scattered parameter loads - a tenth of the arithmetic at 3 % prevalence, but the list can only be worked
// off behind a barrier and a second, uncoalesced round trip: 110 us against 70 on C3, whose timed steps run at 5-25 %
// prevalence.)
__global__ __launch_bounds__(kThreads) void k_transmission(
    int64_t n, const float* __restrict__ mx, const float* __restrict__ shp, const float* __restrict__ rt,
    const float* __restrict__ sh, const float* __restrict__ t_inf, const float* __restrict__ inf,
    const float* __restrict__ stage, float* __restrict__ trans, float* __restrict__ qtrans, float now_arg,
    int has_q, float q_thr, const gj_clock* __restrict__ clock) {
  const float now = clock ? clock->now : now_arg;      // device clock: a captured step replayed for later timesteps
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 f = load_nt(reinterpret_cast<const float4*>(inf) + i);      // (non-temporal: read once per step, see gj_tiled.h)
    float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // is_infected == 0 makes the product 0 whatever the profile (finite for every agent the reference gives a
    // finite value for), so the five parameter streams are only read where someone is infected: early in an
    // epidemic most 128-byte lines of them are never touched
    unsigned m = (f.x != 0.0f ? 1u : 0u) | (f.y != 0.0f ? 2u : 0u) | (f.z != 0.0f ? 4u : 0u) | (f.w != 0.0f ? 8u : 0u);
    if (m) {
      const float4 a = load_nt(reinterpret_cast<const float4*>(mx) + i);
      const float4 b = load_nt(reinterpret_cast<const float4*>(shp) + i);
      const float4 c = load_nt(reinterpret_cast<const float4*>(rt) + i);
      const float4 d = load_nt(reinterpret_cast<const float4*>(sh) + i);
      const float4 e = load_nt(reinterpret_cast<const float4*>(t_inf) + i);
      // The profile (~100 instructions since round 3, ~690 with libm - see inv_gamma) is evaluated by a wave for all 64
      // lanes whenever one of them needs it.  Each lane therefore takes ITS infected agents one after the other: a wave makes
      // as many evaluations as its busiest lane has infected agents (at 1 % prevalence ~1 instead of ~2 with one
      // evaluation per component, at 30 % 3.4 of 4): 67 -> 62 us on C3.  (Measured, not adopted: exp(-lgamma(shape)),
      // 60 % of those instructions and a per-agent constant, cached in a sixth parameter array - 6 us SLOWER: with
      // the evaluations compacted the launch is bound by its reads again, and the cache adds 4 bytes per agent.)
      while (m) {
        const int k = __builtin_ctz(m);
        m &= m - 1u;
#define GJ_PICK(v) (k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w)
        const float val = transmission_value(GJ_PICK(a), GJ_PICK(b), GJ_PICK(c), GJ_PICK(d), GJ_PICK(e), GJ_PICK(f), now);
#undef GJ_PICK
        r.x = k == 0 ? val : r.x;
        r.y = k == 1 ? val : r.y;
        r.z = k == 2 ? val : r.z;
        r.w = k == 3 ? val : r.w;
      }
    }
    reinterpret_cast<float4*>(trans)[i] = r;
    if (has_q) {
      const float4 s = reinterpret_cast<const float4*>(stage)[i];
      float4 q;
      q.x = (s.x < q_thr ? 1.0f : 0.0f) * r.x;
      q.y = (s.y < q_thr ? 1.0f : 0.0f) * r.y;
      q.z = (s.z < q_thr ? 1.0f : 0.0f) * r.z;
      q.w = (s.w < q_thr ? 1.0f : 0.0f) * r.w;
      reinterpret_cast<float4*>(qtrans)[i] = q;
    }
  }
  // tail (n % 4 agents): first threads of block 0
  if (blockIdx.x == 0) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    if (threadIdx.x < (n & 3)) {
      const float r = inf[i] != 0.0f ? transmission_value(mx[i], shp[i], rt[i], sh[i], t_inf[i], inf[i], now) : 0.0f;
      trans[i] = r;
      if (has_q) qtrans[i] = (stage[i] < q_thr ? 1.0f : 0.0f) * r;
    }
  }
}

// ------------------------------------------------------------------------------------------
// a3 + a4 + a5   pass 1: cum_n[v] = sum_{e in venue v} trans_n[agent(e)] * (beta_n * p_contact[v])
//   reference: grad_june/infection_networks/base.py:61-79,86-87 (+ leisure_network.py:61-72)
//
// One workgroup per schedule entry (gj_block).
//  STREAM: the block owns whole venues [v0,v1) with <= 2048 edges in total.  All 256 threads
//          stream the block's contiguous edge range with coalesced index loads, 8 independent
//          gathers in flight per thread, and stage the gathered values in LDS; then `lanes`
//          lanes per venue sum each venue's LDS segment (lanes == 1: in edge order, i.e. the
//          reference's scatter_add_ order) and combine with wave64 shuffles.
//  LONG:   the block owns edges [e0,e1) of ONE venue; register accumulation, wave shuffles,
//          cross-wave combine through LDS, partial sum to plan.partial[slot].
// ------------------------------------------------------------------------------------------
template <bool LEISURE>
__device__ __forceinline__ float gather_x(const P1Args& A, const float* __restrict__ src, int32_t a,
                                          const float* __restrict__ tab) {
  float x = src[a];
  if (LEISURE) x = tab[A.cls[a]] * x;   // (q*L)*t == L*(q*t) exactly for q in {0,1}
  return x;
}

template <int G>
__device__ __forceinline__ void stream_reduce(const SetP1& S, const gj_block& b, int k, const float* lds,
                                              int tid) {
  const int R = b.v1 - b.v0;
  const int grp = tid / G, lane = tid % G;
  constexpr int kGroups = kThreads / G;
  const float beta = S.beta[k];
  for (int r = grp; r < R; r += kGroups) {
    const int v = b.v0 + r;
    const int s = S.v_rowptr[v] - b.e0;
    const int t = S.v_rowptr[v + 1] - b.e0;
    const float y = beta * S.v_pc[v];
    float sum = 0.0f;
    for (int i = s + lane; i < t; i += G) sum += lds[i] * y;
    if (G > 1) sum = group_sum<G>(sum);
    if (lane == 0) S.cum[(int64_t)v * S.stride + k] = sum;
  }
}

__global__ __launch_bounds__(kThreads) void k_venue_reduce(const P1Args A) {
  __shared__ float lds[GJ_STREAM_EDGES];
  __shared__ float wsum[kThreads / kWave][GJ_MAX_NETS_PER_SET];
  const gj_block b = A.blocks[blockIdx.x];
  const SetP1& S = A.sets[b.set];
  const int nk = S.nk;
  if (nk == 0) return;  // set not active in this step (block-uniform)
  const int tid = threadIdx.x;
  const float* __restrict__ src = S.raw ? A.trans : A.qtrans;

  if (b.kind == 0) {
    const int ne = b.e1 - b.e0;
    for (int k = 0; k < nk; ++k) {
      const float* tab = S.leisure ? A.tables + (int64_t)S.table[k] * GJ_TABLE_SIZE + A.day_type * 200 : nullptr;
      // stage: coalesced index stream, kEdgesPerThread independent gathers per thread
      int32_t ag[kEdgesPerThread];
#pragma unroll
      for (int j = 0; j < kEdgesPerThread; ++j) {
        const int i = j * kThreads + tid;
        ag[j] = (i < ne) ? S.v_agent[b.e0 + i] : -1;
      }
#pragma unroll
      for (int j = 0; j < kEdgesPerThread; ++j) {
        const int i = j * kThreads + tid;
        if (ag[j] >= 0) lds[i] = S.leisure ? gather_x<true>(A, src, ag[j], tab) : gather_x<false>(A, src, ag[j], tab);
      }
      __syncthreads();
      switch (b.lanes) {
        case 1: stream_reduce<1>(S, b, k, lds, tid); break;
        case 4: stream_reduce<4>(S, b, k, lds, tid); break;
        case 16: stream_reduce<16>(S, b, k, lds, tid); break;
        default: stream_reduce<64>(S, b, k, lds, tid); break;
      }
      if (k + 1 < nk) __syncthreads();
    }
    return;
  }

  // LONG: one venue, edges [e0,e1)
  float acc[GJ_MAX_NETS_PER_SET];
  float y[GJ_MAX_NETS_PER_SET];
  const float pc = S.v_pc[b.v0];
#pragma unroll
  for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
    acc[k] = 0.0f;
    y[k] = (k < nk) ? S.beta[k] * pc : 0.0f;
  }
  if (!S.leisure && nk == 1) {
    float a0 = 0.0f;
    int e = b.e0 + tid;
    for (; e + 3 * kThreads < b.e1; e += 4 * kThreads) {
      const int32_t i0 = S.v_agent[e], i1 = S.v_agent[e + kThreads], i2 = S.v_agent[e + 2 * kThreads],
                    i3 = S.v_agent[e + 3 * kThreads];
      const float x0 = src[i0], x1 = src[i1], x2 = src[i2], x3 = src[i3];
      a0 += x0 * y[0];
      a0 += x1 * y[0];
      a0 += x2 * y[0];
      a0 += x3 * y[0];
    }
    for (; e < b.e1; e += kThreads) a0 += src[S.v_agent[e]] * y[0];
    acc[0] = a0;
  } else if (!S.leisure) {
    // several networks on a set without tables (do_venue_reduce accepts them): the STREAM loop's term per network.
    // (Until the CSR kernels were pinned per venue this case fell into the branch above, which sums network 0 only:
    // a long venue's cum of every further network was 0.)
    for (int e = b.e0 + tid; e < b.e1; e += kThreads) {
      const float x = src[S.v_agent[e]];
#pragma unroll
      for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k)
        if (k < nk) acc[k] += x * y[k];
    }
  } else {
    const float* tabs = A.tables + A.day_type * 200;
    for (int e = b.e0 + tid; e < b.e1; e += kThreads) {
      const int32_t a = S.v_agent[e];
      const float x = src[a];
      const int c = A.cls[a];
#pragma unroll
      for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k)
        if (k < nk) acc[k] += (tabs[(int64_t)S.table[k] * GJ_TABLE_SIZE + c] * x) * y[k];
    }
  }
  const int wave = tid / kWave, lane = tid % kWave;
#pragma unroll
  for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
    if (k < nk) {
      const float w = group_sum<kWave>(acc[k]);
      if (lane == 0) wsum[wave][k] = w;
    }
  }
  __syncthreads();
  if (tid < nk) {
    float s = 0.0f;
#pragma unroll
    for (int w = 0; w < kThreads / kWave; ++w) s += wsum[w][tid];
    A.partial[(int64_t)b.slot * GJ_MAX_NETS_PER_SET + tid] = s;
  }
}

// ordered combine of the partial sums of one long venue (deterministic: chunk order)
struct CombineArgs {
  struct { float* cum; int32_t stride; int32_t nk; } sets[GJ_MAX_SETS];
  const gj_long_row* rows;
  const float* partial;
  int32_t n_rows;
};

__global__ __launch_bounds__(kThreads) void k_combine_long(const CombineArgs C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int row = i / GJ_MAX_NETS_PER_SET, k = i % GJ_MAX_NETS_PER_SET;
  if (row >= C.n_rows) return;
  const gj_long_row r = C.rows[row];
  const auto& S = C.sets[r.set];
  if (k >= S.nk) return;
  float s = 0.0f;
  for (int slot = r.slot0; slot < r.slot1; ++slot) s += C.partial[(int64_t)slot * GJ_MAX_NETS_PER_SET + k];
  S.cum[(int64_t)r.v * S.stride + k] = s;
}

// ------------------------------------------------------------------------------------------
// a4 + a6 + a7 (+ a8 + a9)   pass 2, one thread per agent:
//   ts[a] = sum_n  sum_{e in row a of set(n)} cum_n[venue(e)] * susc_n[a]      (network order = params order)
//   p = clamp(exp(-clamp(ts,1e-6,100) * dt), 0, 1);  Gumbel decision;  state update
//   reference: base.py:80-83,118-141; leisure_network.py:74-85,107-120; infection.py:13-18; model.py:103-110
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_agent_gather(const P2Args P) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= P.n_agents) return;
  float susc = P.susceptibility[a];
  float q = 1.0f;
  if (P.has_q) q = (P.stage[a] < P.q_thr) ? 1.0f : 0.0f;
  int c = 0;
  if (P.any_leisure) c = P.cls[a];
  const float* tabs = P.tables + P.day_type * 200;

  float ts = 0.0f;
  for (int g = 0; g < P.n_groups; ++g) {
    const SetP2& S = P.groups[g];
    const int r0 = S.a_rowptr[a], r1 = S.a_rowptr[a + 1];
    if (S.nk == 1 && S.mask[0] <= GJ_MASK_Q) {
      const float w = (S.mask[0] == GJ_MASK_RAW) ? susc : q * susc;
      float acc = 0.0f;
      for (int e = r0; e < r1; ++e) acc += S.cum[(int64_t)S.a_venue[e] * S.stride] * w;
      ts += acc;
    } else {
      float w[GJ_MAX_NETS_PER_SET], acc[GJ_MAX_NETS_PER_SET];
#pragma unroll
      for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
        acc[k] = 0.0f;
        w[k] = 0.0f;
        if (k < S.nk) {
          const int m = S.mask[k];
          float wk = (m == GJ_MASK_RAW) ? susc : q;
          if (m >= GJ_MASK_QL) wk = wk * tabs[(int64_t)S.table[k] * GJ_TABLE_SIZE + c];
          if (m != GJ_MASK_RAW) wk = wk * susc;
          if (m == GJ_MASK_QL_AGE75) wk = wk * (((c % 100) > 75) ? 1.0f : 0.0f);
          w[k] = wk;
        }
      }
      for (int e = r0; e < r1; ++e) {
        const float* cv = S.cum + (int64_t)S.a_venue[e] * S.stride;
#pragma unroll
        for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k)
          if (k < S.nk) acc[k] += cv[k] * w[k];
      }
#pragma unroll
      for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k)
        if (k < S.nk) ts += acc[k];
    }
  }
  if (P.trans_susc) P.trans_susc[a] = ts;
  const float p = not_infected_prob(ts, P.dt);
  if (P.not_infected_probs) P.not_infected_probs[a] = p;
  if (!P.sample) return;

  float e0, e1;
  if (P.exp_noise) {
    e0 = P.exp_noise[a];
    e1 = P.exp_noise[P.n_agents + a];
  } else {
    e0 = e1 = 1.0f;
  }
  const float nw = P.exp_noise ? gumbel_new_infected(p, e0, e1)
                               : own_new_infected(p, infection_uniform(P.seed, P.clock ? P.clock->step : P.step,
                                                                       P.agent_offset + a));
  if (P.new_infected) P.new_infected[a] = nw;
  if (nw != 0.0f) {   // unchanged values are not rewritten
    float inf = P.is_infected[a], t_inf = P.infection_time[a];
    infect(nw, P.clock ? P.clock->now : P.now, susc, inf, t_inf);
    P.susceptibility[a] = susc;
    P.is_infected[a] = inf;
    P.infection_time[a] = t_inf;
  }
}

// a8 + a9 on a caller-supplied probability vector
__global__ __launch_bounds__(kThreads) void k_sample_infect(int64_t n, const float* __restrict__ p_not,
                                                            const float* __restrict__ noise, uint64_t seed,
                                                            uint64_t step, int64_t agent_offset, float now,
                                                            float* __restrict__ new_inf, float* __restrict__ susc,
                                                            float* __restrict__ inf, float* __restrict__ t_inf) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;
  float e0, e1;
  if (noise) {
    e0 = noise[a];
    e1 = noise[n + a];
  } else {
    e0 = e1 = 1.0f;
  }
  const float nw = noise ? gumbel_new_infected(p_not[a], e0, e1)
                         : own_new_infected(p_not[a], infection_uniform(seed, step, agent_offset + a));
  if (new_inf) new_inf[a] = nw;
  if (susc != nullptr && nw != 0.0f) {   // state pointers NULL: sample only
    float s = susc[a], i = inf[a], t = t_inf[a];
    infect(nw, now, s, i, t);
    susc[a] = s;
    inf[a] = i;
    t_inf[a] = t;
  }
}

// f3: d loss / d log_beta of the networks on one edge set (include/gradjune_hip.h, gj_adjoint_beta_*)
struct AdjBetaArgs {
  int64_t n_venues;
  int32_t stride, nk;
  const float* cum_fwd;
  const float* cum_bwd;
  const float* v_pc;
  const double* weights;
  float beta[GJ_MAX_NETS_PER_SET];
  int32_t cols[GJ_MAX_NETS_PER_SET];
  double* partial;
};

// (1024 lanes per workgroup, two venues' loads in flight per lane: a lane's terms are added in venue order, one after the
// other in fp64, so its loop is a chain of memory round trips - 6 M households over 256 x 256 lanes were 92 of them)
constexpr int kAdjBetaThreads = 1024;
__global__ __launch_bounds__(kAdjBetaThreads) void k_adjoint_beta_partial(const AdjBetaArgs A) {
  __shared__ double part[kAdjBetaThreads / kWave][GJ_MAX_NETS_PER_SET];
  double acc[GJ_MAX_NETS_PER_SET];
#pragma unroll
  for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) acc[k] = 0.0;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  auto term = [&](double pc, double w, const float (&f)[GJ_MAX_NETS_PER_SET], const float (&b)[GJ_MAX_NETS_PER_SET]) {
    if (!(pc > 0.0)) return;
#pragma unroll
    for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
      if (k >= A.nk) break;
      const double beta = (double)A.beta[k];
      if (beta == 0.0) continue;
      acc[k] += (double)f[k] * (double)b[k] / (beta * pc) * w;
    }
  };
  for (int64_t v0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v0 < A.n_venues; v0 += 2 * step) {
    const int64_t v1 = v0 + step;
    const bool two = v1 < A.n_venues;
    const int64_t u1 = two ? v1 : v0;
    const double pc0 = (double)A.v_pc[v0], pc1 = (double)A.v_pc[u1];
    const double w0 = A.weights ? A.weights[v0] : 1.0, w1 = A.weights ? A.weights[u1] : 1.0;
    float f0[GJ_MAX_NETS_PER_SET], b0[GJ_MAX_NETS_PER_SET], f1[GJ_MAX_NETS_PER_SET], b1[GJ_MAX_NETS_PER_SET];
#pragma unroll
    for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
      const bool on = k < A.nk;
      f0[k] = on ? A.cum_fwd[v0 * A.stride + k] : 0.0f;
      b0[k] = on ? A.cum_bwd[v0 * A.stride + k] : 0.0f;
      f1[k] = on ? A.cum_fwd[u1 * A.stride + k] : 0.0f;
      b1[k] = on ? A.cum_bwd[u1 * A.stride + k] : 0.0f;
    }
    term(pc0, w0, f0, b0);
    if (two) term(pc1, w1, f1, b1);
  }
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
#pragma unroll
  for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
    const double x = wave_sum(acc[k]);
    if (lane == 0) part[wave][k] = x;
  }
  __syncthreads();
  if ((int)threadIdx.x < A.nk) {
    double x = 0.0;
    for (int w = 0; w < kAdjBetaThreads / kWave; ++w) x += part[w][threadIdx.x];
    A.partial[(int64_t)blockIdx.x * GJ_MAX_NETS + A.cols[threadIdx.x]] += x;     // this (row, column) is this workgroup's alone
  }
}

__global__ void k_adjoint_beta_finish(int32_t n_cols, const double* partial, const float* scale, double* out) {
  const int c = threadIdx.x;
  if (c >= n_cols) return;
  double x = 0.0;
  for (int b = 0; b < GJ_ADJ_BETA_BLOCKS; ++b) x += partial[(int64_t)b * GJ_MAX_NETS + c];
  out[c] = x * (double)(*scale) * 2.302585092994046;      // ln(10)
}

// a2 alone: q*transmission for a caller-supplied transmission vector
__global__ __launch_bounds__(kThreads) void k_quarantine_transmission(int64_t n, const float* __restrict__ stage,
                                                                      const float* __restrict__ trans,
                                                                      float* __restrict__ qtrans, float q_thr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) qtrans[i] = (stage[i] < q_thr ? 1.0f : 0.0f) * trans[i];
}

// halo pack / unpack
__global__ __launch_bounds__(kThreads) void k_pack(int64_t n, const int32_t* __restrict__ idx,
                                                   const float* __restrict__ src, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = src[idx[i]];
}
__global__ __launch_bounds__(kThreads) void k_unpack(int64_t n, const int32_t* __restrict__ idx,
                                                     const float* __restrict__ in, float* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[idx[i]] = in[i];
}

// ------------------------------------------------------------------------------------------
// host side: argument checking and launch
// ------------------------------------------------------------------------------------------
static inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? GJ_OK : (int)e;
}

template <typename K, typename... Args>
static int launch(K kernel, int64_t blocks, int threads, size_t lds, hipStream_t stream, const Args&... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)threads), lds, stream, args...);
  return launch_status();
}

// workgroups for n items at `per_block` items each (one lane per item: kThreads): at least one, at most `cap` (0: no cap)
static inline int64_t grid_for(int64_t n, int64_t cap = 0, int per_block = kThreads) {
  int64_t blocks = (n + per_block - 1) / per_block;
  if (cap > 0 && blocks > cap) blocks = cap;
  return blocks < 1 ? 1 : blocks;
}

// every pointer 16-byte aligned (NULL counts as aligned): what selects a kernel's four-agents-per-lane path
template <typename... P>
static inline bool aligned16(const P*... p) {
  return ((... | (uintptr_t)p) % 16) == 0;
}

static int check_tiled(const gj_plan* plan);

static int check_plan(const gj_plan* plan) {
  if (!plan) return GJ_E_NULL;
  if (plan->n_agents < 0 || plan->n_ext_agents < plan->n_agents) return GJ_E_RANGE;
  if (plan->n_ext_agents > INT32_MAX) return GJ_E_RANGE;
  if (plan->n_sets < 0 || plan->n_sets > GJ_MAX_SETS) return GJ_E_RANGE;
  for (int s = 0; s < plan->n_sets; ++s) {
    const gj_edge_set& S = plan->sets[s];
    if (S.n_edges < 0 || S.n_edges > INT32_MAX || S.n_venues < 0 || S.n_venues > INT32_MAX) return GJ_E_RANGE;
    if (S.cum_stride < 1 || S.cum_stride > GJ_MAX_NETS_PER_SET) return GJ_E_PLAN;
    if (!S.v_pcontact && S.n_venues > 0) return GJ_E_NULL;
    if (S.n_venues > 0 && !S.cum) return GJ_E_NULL;
    if (plan->tiled) continue;
    if (!S.v_rowptr || !S.a_rowptr) return GJ_E_NULL;
    if (S.n_edges > 0 && (!S.v_agent || !S.a_venue)) return GJ_E_NULL;
  }
  if (plan->tiled) return check_tiled(plan);
  if (plan->n_blocks < 0 || (plan->n_blocks > 0 && !plan->blocks)) return GJ_E_PLAN;
  if (plan->n_long_rows < 0 || (plan->n_long_rows > 0 && (!plan->long_rows || !plan->partial))) return GJ_E_PLAN;
  return GJ_OK;
}

// group the step's networks by edge set, keeping order; networks of one set must be adjacent
struct Groups {
  int n;
  int set[GJ_MAX_SETS];
  int first[GJ_MAX_SETS];
  int nk[GJ_MAX_SETS];
};

static int group_networks(const gj_plan* plan, const gj_step_params* p, Groups* G) {
  if (!p) return GJ_E_NULL;
  if (p->transpose && !plan->tiled) return GJ_E_PLAN;   // the backward passes exist for the tiled layout
  if (p->n_nets < 0 || p->n_nets > GJ_MAX_NETS) return GJ_E_RANGE;
  if (p->day_type < 0 || p->day_type > 1) return GJ_E_RANGE;
  G->n = 0;
  bool seen[GJ_MAX_SETS] = {false};
  for (int i = 0; i < p->n_nets; ++i) {
    const gj_network& N = p->nets[i];
    if (N.set < 0 || N.set >= plan->n_sets) return GJ_E_RANGE;
    if (N.mask_kind < GJ_MASK_RAW || N.mask_kind > GJ_MASK_QL_AGE75) return GJ_E_RANGE;
    if (N.mask_kind >= GJ_MASK_QL) {
      if (N.table < 0 || N.table >= plan->n_tables || !plan->tables || !plan->agent_class) return GJ_E_PLAN;
    }
    if (G->n > 0 && G->set[G->n - 1] == N.set) {
      if (G->nk[G->n - 1] >= plan->sets[N.set].cum_stride) return GJ_E_PLAN;
      // transmissions of one set come from one source array: RAW and masked kinds cannot mix
      const int m0 = p->nets[G->first[G->n - 1]].mask_kind;
      if ((m0 == GJ_MASK_RAW) != (N.mask_kind == GJ_MASK_RAW)) return GJ_E_PLAN;
      G->nk[G->n - 1]++;
    } else {
      if (seen[N.set]) return GJ_E_PLAN;  // not adjacent
      seen[N.set] = true;
      G->set[G->n] = N.set;
      G->first[G->n] = i;
      G->nk[G->n] = 1;
      G->n++;
    }
  }
  return GJ_OK;
}

// The networks of group g as every kernel argument block takes them.  Entries past nk are 0.
struct NetGroup {
  int32_t nk;
  int32_t raw;                               // the set's transmissions are the raw ones (household), not q * transmission
  int32_t leisure;                           // any network of the set uses a table
  float beta[GJ_MAX_NETS_PER_SET];
  int32_t mask[GJ_MAX_NETS_PER_SET];
  int32_t table[GJ_MAX_NETS_PER_SET];        // -1: no leisure table
  int32_t age75[GJ_MAX_NETS_PER_SET];
};

// (RAW and masked kinds cannot mix on a set - group_networks - so the first network decides)
static inline bool group_is_raw(const gj_step_params* p, const Groups& G, int g) {
  return p->nets[G.first[g]].mask_kind == GJ_MASK_RAW;
}

static NetGroup classify_group(const gj_step_params* p, const Groups& G, int g) {
  NetGroup C = {};
  C.nk = G.nk[g];
  C.raw = group_is_raw(p, G, g);
  for (int k = 0; k < C.nk; ++k) {
    const gj_network& N = p->nets[G.first[g] + k];
    const bool tabled = N.mask_kind >= GJ_MASK_QL;
    C.beta[k] = N.beta;
    C.mask[k] = N.mask_kind;
    C.table[k] = tabled ? N.table : -1;
    C.age75[k] = N.mask_kind == GJ_MASK_QL_AGE75;
    if (tabled) C.leisure = 1;
  }
  return C;
}

// a set either is a leisure set (every network has a table) or, where the kernel needs it, has exactly one network
static int check_group(const NetGroup& C, bool plain_is_single = true) {
  if (C.leisure) {
    for (int k = 0; k < C.nk; ++k)
      if (C.table[k] < 0) return GJ_E_PLAN;
  } else if (plain_is_single && C.nk != 1) {
    return GJ_E_PLAN;   // several networks on one set need per-network tables
  }
  return GJ_OK;
}

// full: the launch reads/writes is_infected and infection_time too (a1, a9)
static int check_state(const gj_plan* plan, const gj_agent_state* st, const gj_step_params* p, bool full = true) {
  if (!st) return GJ_E_NULL;
  if (plan->n_agents == 0) return GJ_OK;
  if (!st->transmission || !st->susceptibility) return GJ_E_NULL;
  if (full && (!st->is_infected || !st->infection_time)) return GJ_E_NULL;
  if (p->has_quarantine && (!st->current_stage || !st->q_transmission)) return GJ_E_NULL;
  return GJ_OK;
}

static int do_transmission(const gj_plan* plan, const gj_agent_state* st, const gj_step_params* p,
                           hipStream_t stream) {
  if (!st->max_infectiousness || !st->shape || !st->rate || !st->shift) return GJ_E_NULL;
  const int64_t n = plan->n_agents;
  if (n == 0) return GJ_OK;
  return launch(k_transmission, grid_for((n + 3) / 4, 256 * 16), kThreads, 0, stream, n, st->max_infectiousness,
                st->shape, st->rate, st->shift, st->infection_time, st->is_infected, st->current_stage,
                st->transmission, st->q_transmission, p->now, p->has_quarantine, p->q_threshold, p->clock);
}

static int do_venue_reduce(const gj_plan* plan, const gj_agent_state* st, const gj_step_params* p, const Groups& G,
                           hipStream_t stream) {
  if (plan->n_blocks == 0 || G.n == 0) return GJ_OK;
  P1Args A;
  for (int s = 0; s < GJ_MAX_SETS; ++s) {
    A.sets[s] = SetP1{};
    A.sets[s].nk = 0;
  }
  for (int g = 0; g < G.n; ++g) {
    const gj_edge_set& E = plan->sets[G.set[g]];
    SetP1& S = A.sets[G.set[g]];
    S.v_rowptr = E.v_rowptr;
    S.v_agent = E.v_agent;
    S.v_pc = E.v_pcontact;
    S.cum = E.cum;
    S.stride = E.cum_stride;
    const NetGroup C = classify_group(p, G, g);
    S.nk = C.nk;
    S.raw = C.raw;
    S.leisure = C.leisure;
    memcpy(S.beta, C.beta, sizeof(S.beta));
    memcpy(S.table, C.table, sizeof(S.table));
    // (on purpose: the CSR kernels loop over the networks of a plain set, so several of them on one set are accepted)
    if (const int rc = check_group(C, /*plain_is_single=*/false)) return rc;
  }
  A.blocks = plan->blocks;
  A.trans = st->transmission;
  A.qtrans = p->has_quarantine ? st->q_transmission : st->transmission;
  A.cls = plan->agent_class;
  A.tables = plan->tables;
  A.partial = plan->partial;
  A.day_type = p->day_type;
  int rc = launch(k_venue_reduce, plan->n_blocks, kThreads, 0, stream, A);
  if (rc != GJ_OK) return rc;
  if (plan->n_long_rows > 0) {
    CombineArgs C;
    for (int s = 0; s < GJ_MAX_SETS; ++s) {
      C.sets[s].cum = A.sets[s].cum;
      C.sets[s].stride = A.sets[s].stride;
      C.sets[s].nk = A.sets[s].nk;
    }
    C.rows = plan->long_rows;
    C.partial = plan->partial;
    C.n_rows = plan->n_long_rows;
    rc = launch(k_combine_long, grid_for((int64_t)plan->n_long_rows * GJ_MAX_NETS_PER_SET), kThreads, 0, stream, C);
  }
  return rc;
}

static int do_agent_gather(const gj_plan* plan, const gj_agent_state* st, const gj_step_params* p, const Groups& G,
                           const gj_step_io* io, int sample, hipStream_t stream) {
  const int64_t n = plan->n_agents;
  if (n == 0) return GJ_OK;
  if (io && io->agent_sums) return GJ_E_PLAN;      // the CSR kernel multiplies by the susceptibility per term: tiled layout only
  P2Args P;
  P.n_groups = G.n;
  P.any_leisure = 0;
  for (int g = 0; g < G.n; ++g) {
    const gj_edge_set& E = plan->sets[G.set[g]];
    SetP2& S = P.groups[g];
    S.a_rowptr = E.a_rowptr;
    S.a_venue = E.a_venue;
    S.cum = E.cum;
    S.stride = E.cum_stride;
    const NetGroup C = classify_group(p, G, g);   // not checked: the kernel takes any mix of kinds, network by network
    S.nk = C.nk;
    memcpy(S.mask, C.mask, sizeof(S.mask));
    for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) S.table[k] = C.table[k] < 0 ? 0 : C.table[k];   // (no table: 0, unread)
    P.any_leisure |= C.leisure;
  }
  P.n_agents = n;
  P.cls = plan->agent_class;
  P.tables = plan->tables;
  P.stage = st->current_stage;
  P.susceptibility = st->susceptibility;
  P.is_infected = st->is_infected;
  P.infection_time = st->infection_time;
  P.not_infected_probs = io ? io->not_infected_probs : nullptr;
  P.new_infected = io ? io->new_infected : nullptr;
  P.trans_susc = io ? io->trans_susc : nullptr;
  P.exp_noise = io ? io->exp_noise : nullptr;
  P.now = p->now;
  P.dt = p->delta_time;
  P.q_thr = p->q_threshold;
  P.day_type = p->day_type;
  P.has_q = p->has_quarantine;
  P.sample = sample;
  P.seed = p->seed;
  P.step = p->step;
  P.agent_offset = p->agent_offset;
  P.clock = p->clock;
  return launch(k_agent_gather, grid_for(n), kThreads, 0, stream, P);
}

// ------------------------------------------------------------------------------------------
// tiled layout: host side
// ------------------------------------------------------------------------------------------
static int check_tiled(const gj_plan* plan) {
  const gj_tiled* T = plan->tiled;
  if (T->n_slices < 1 || T->slice_agents < 64 || T->slice_agents % 64 || T->slice_agents > kMaxSliceAgents) return GJ_E_PLAN;
  // slices cover owned + halo agents; halo agents start on a slice boundary (phase D runs on the
  // slices of owned agents only)
  if ((int64_t)T->n_slices * T->slice_agents < plan->n_ext_agents) return GJ_E_PLAN;
  if (T->n_work < 0 || (T->n_work > 0 && !T->work)) return GJ_E_PLAN;
  for (int s = 0; s < plan->n_sets; ++s) {
    const gj_tiled_set& S = T->sets[s];
    if (S.n_blocks < 0) return GJ_E_PLAN;
    if (S.n_blocks == 0) continue;
    if (!S.blk_v0 || !S.blk_e0 || !S.tile_sptr || !S.tile_jpos || !S.chunk_ptr) return GJ_E_NULL;
    const bool run = S.run_pv_blk || S.run_pv_win || S.run_blk_r0 || S.run_win_lo || S.run_win_n;
    if (run) {   // all or none; one window of cum per slice must fit phase D's table region
      if (!S.run_pv_blk || !S.run_pv_win || !S.run_blk_r0 || !S.run_win_lo || !S.run_win_n) return GJ_E_NULL;
      if (S.run_max_window < 0 || S.run_max_window > 32768 || S.run_tiled_edges < 0 ||
          S.run_tiled_edges > plan->sets[s].n_edges || S.ell_k)
        return GJ_E_PLAN;
    }
    if (S.presum && (!S.ell_k || T->presum_wgs < 1 || T->presum_wgs > 4096)) return GJ_E_PLAN;
    const int64_t held = run ? (int64_t)S.run_tiled_edges : plan->sets[s].n_edges;
    if (held > 0 && (!S.e_lv || !S.a_la || !S.val || !S.chunk_desc)) return GJ_E_NULL;
    if (S.max_block_venues < 1 || S.max_block_venues > 65536) return GJ_E_PLAN;
    // phases A and D address val / a_la / chunk_desc with 32-bit byte offsets: < 2^30 edges per set (a larger set
    // is split over several edge sets of the same venue type)
    if (plan->sets[s].n_edges >= ((int64_t)1 << 30) - 8 * (int64_t)S.n_blocks) return GJ_E_RANGE;
    if (S.ell_k) {   // direct form of pass 2: 16-bit venue ids, one 2/4/8/16-byte row per agent
      if (S.ell_k != 2 && S.ell_k != 4 && S.ell_k != 8) return GJ_E_PLAN;
      if (!S.ell) return GJ_E_NULL;
      if (plan->sets[s].n_venues > 65534) return GJ_E_PLAN;
    }
  }
  return GJ_OK;
}

// edges the tiled arrays of a set hold (a run form keeps one edge per owned agent out of them)
static inline int64_t tiled_edges(const gj_plan* plan, int s) {
  const gj_tiled_set& S = plan->tiled->sets[s];
  return S.run_pv_blk ? (int64_t)S.run_tiled_edges : plan->sets[s].n_edges;
}

// pass 1 of this set runs in the direct form (k_tile_presum + k_presum_reduce) instead of phases A + B
static inline bool uses_presum(const gj_plan* plan, int s) {
  const gj_tiled* T = plan->tiled;
  return T->presum_wgs > 0 && T->sets[s].presum != nullptr && T->sets[s].ell_k != 0 && T->sets[s].n_blocks > 0 &&
         plan->sets[s].n_edges > 0;
}

template <typename K>
static int allow_lds(K kernel, size_t bytes) {
  if (bytes > 160 * 1024) return GJ_E_PLAN;
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
  }
  return GJ_OK;
}

static void fill_set_a(const gj_plan* plan, const gj_step_params* p, const Groups& G, TSetA* sets) {
  const gj_tiled* T = plan->tiled;
  for (int s = 0; s < GJ_MAX_SETS; ++s) sets[s] = TSetA{};
  for (int g = 0; g < G.n; ++g) {
    const int s = G.set[g];
    const gj_tiled_set& S = T->sets[s];
    sets[s].a_la = S.a_la;
    sets[s].tile_sptr = S.tile_sptr;
    sets[s].tile_jpos = S.tile_jpos;
    sets[s].chunk_ptr = S.chunk_ptr;
    sets[s].chunk_desc = reinterpret_cast<const int4*>(S.chunk_desc);
    sets[s].val = S.val;
    sets[s].J = S.n_blocks;
    sets[s].active = (S.n_blocks > 0 && tiled_edges(plan, s) > 0) ? G.nk[g] : 0;
    sets[s].presum = uses_presum(plan, s);
    sets[s].raw = group_is_raw(p, G, g);
    sets[s].wide = S.desc_wide;          // 0 / 1: descriptor format, 2: explicit slots
    sets[s].direct = S.ell_k != 0;
    sets[s].multi_slots = S.multi_slots;
  }
}

// LDS of phases A and D: one slice (fp32 values in A, 64-bit fixed-point sums in D)
static size_t slice_lds(const gj_tiled* T, size_t elem) { return (size_t)T->slice_agents * elem; }
// phase D: 64-bit sums + two flag bits per agent (saturated up / down, gj_tiled.h fx_flag)
static size_t agents_lds(const gj_tiled* T) { return (size_t)T->slice_agents * sizeof(fx_t) + 2 * ((size_t)T->slice_agents / 8); }

// the direct forms read four agents' classes as one dword (see gj_plan.agent_class)
static inline bool classes_by_dword(const gj_plan* plan) {
  return plan->agent_class && (uintptr_t)plan->agent_class % 4 == 0;
}

// Bit pattern of the largest |term| a venue sum of this set takes: 2^14 (the window of the 2^-36 fixed point) while the
// largest venue has at most 4 096 edges, else 2^26 / next_pow2(edges) - terms x edges then stays below 2^62 fixed-point
// units and no sum can wrap.  A term beyond it saturates its venue (gj_tiled.h).  0 edges = not stated: 2^14.
static uint32_t venue_term_limit(int32_t max_venue_edges) {
  int e = 14;
  int64_t p2 = 4096;
  while (p2 < (int64_t)max_venue_edges && e > -20) {
    p2 <<= 1;
    --e;
  }
  const float lim = ldexpf(1.0f, e);
  uint32_t bits;
  memcpy(&bits, &lim, sizeof(bits));
  return bits;
}

// pass 1 of the sets in its direct form: LDS tables of fixed-point sums per workgroup (k_tile_presum)
static int presum_fill(const gj_plan* plan, const gj_step_params* p, const Groups& G, int g, TPSet* X) {
  const gj_tiled* T = plan->tiled;
  const int s = G.set[g];
  const gj_tiled_set& S = T->sets[s];
  const gj_edge_set& E = plan->sets[s];
  const int64_t owned_slices = (plan->n_agents + T->slice_agents - 1) / T->slice_agents;
  X->ell = S.ell;
  X->plane_stride = owned_slices * (int64_t)T->slice_agents * 2;
  X->partial = reinterpret_cast<fx_t*>(S.presum);
  X->planes = S.ell_k / 2;
  X->V = (int32_t)E.n_venues;
  X->stride = E.cum_stride;
  const NetGroup C = classify_group(p, G, g);
  X->nk = C.nk;
  X->raw = C.raw;
  X->leisure = C.leisure;
  X->term_limit = venue_term_limit(S.max_venue_edges);
  memcpy(X->table, C.table, sizeof(X->table));
  memcpy(X->age75, C.age75, sizeof(X->age75));
  if (C.leisure && !classes_by_dword(plan)) return GJ_E_PLAN;
  return check_group(C);
}

static int tiled_presum(const gj_plan* plan, const gj_agent_state* st, const gj_step_params* p, const Groups& G,
                        hipStream_t stream) {
  const gj_tiled* T = plan->tiled;
  TilePArgs P;
  P.n_sets = 0;
  for (int g = 0; g < G.n; ++g) {
    if (!uses_presum(plan, G.set[g])) continue;
    if (P.n_sets == GJ_MAX_PRESUM) return GJ_E_PLAN;
    const int rc = presum_fill(plan, p, G, g, &P.sets[P.n_sets++]);
    if (rc) return rc;
  }
  if (P.n_sets == 0 || plan->n_agents == 0) return GJ_OK;
  // the LDS table of a set: (venues of a group x networks + 64 scratch) 8-byte sums, leisure weights, one flag bit per sum
  const int64_t budget = 160 * 1024;
  size_t lds = 0;
  for (int t = 0; t < P.n_sets; ++t) {
    TPSet& X = P.sets[t];
    const int64_t fixed = 64 * 8 + (X.leisure ? (int64_t)X.nk * 200 * 4 : 0) + 64;
    int64_t per_venue = (int64_t)X.nk * 8;                  // + its flag bits: 1/8 byte per sum, counted below
    int64_t gv = (budget - fixed) * 8 / (per_venue * 8 + X.nk);
    if (T->direct_table_floats > 0 && gv > T->direct_table_floats / X.nk) gv = T->direct_table_floats / X.nk;   // tests: several groups
    if (gv > X.V) gv = X.V;
    if (gv < 1) gv = 1;
    X.group_venues = (int32_t)gv;
    const size_t need = (size_t)(gv * X.nk + 64) * 8 + (X.leisure ? (size_t)X.nk * 200 * 4 : 0) + ((size_t)(gv * X.nk + 64 + 31) / 32) * 4;
    if (need > lds) lds = need;
  }
  int64_t apw = (plan->n_agents + T->presum_wgs - 1) / T->presum_wgs;
  apw = (apw + 63) / 64 * 64;
  P.agents_per_wg = (int32_t)apw;
  P.n_agents = plan->n_agents;
  P.trans = st->transmission;
  P.qtrans = p->has_quarantine ? st->q_transmission : st->transmission;
  if (!aligned16(P.trans, P.qtrans)) return GJ_E_PLAN;
  P.cls = plan->agent_class;
  P.tables = plan->tables;
  P.day_type = p->day_type;
  P.transpose = p->transpose;
  int rc = allow_lds(k_tile_presum, lds);
  if (rc) return rc;
  return launch(k_tile_presum, T->presum_wgs, kTileThreads, lds, stream, P);
}

static int tiled_presum_reduce(const gj_plan* plan, const gj_step_params* p, const Groups& G, hipStream_t stream) {
  const gj_tiled* T = plan->tiled;
  PReduceArgs R;
  R.n_sets = 0;
  R.n_wgs = T->presum_wgs;
  R._pad = 0;
  int64_t total = 0;
  for (int g = 0; g < G.n; ++g) {
    const int s = G.set[g];
    if (!uses_presum(plan, s)) continue;
    if (R.n_sets == GJ_MAX_PRESUM) return GJ_E_PLAN;
    PReduceSet& X = R.sets[R.n_sets++];
    const gj_edge_set& E = plan->sets[s];
    X.partial = reinterpret_cast<const fx_t*>(T->sets[s].presum);
    X.v_pc = E.v_pcontact;
    X.cum = E.cum;
    X.V = (int32_t)E.n_venues;
    X.stride = E.cum_stride;
    X.nk = G.nk[g];
    X.first = (int32_t)total;
    const NetGroup C = classify_group(p, G, g);
    memcpy(X.beta, C.beta, sizeof(X.beta));
    total += (int64_t)X.V * X.nk;
  }
  if (R.n_sets == 0 || total == 0) return GJ_OK;
  if (total > INT32_MAX) return GJ_E_RANGE;
  R.total = (int32_t)total;
  return launch(k_presum_reduce, grid_for(total, 0, kWave), kThreads, 0, stream, R);
}

static int tiled_scatter(const gj_plan* plan, const gj_agent_state* st, const gj_step_params* p, const Groups& G,
                         hipStream_t stream) {
  const gj_tiled* T = plan->tiled;
  if (plan->n_ext_agents == 0 || G.n == 0) return GJ_OK;
  TileAArgs A;
  fill_set_a(plan, p, G, A.sets);
  A.n_sets = plan->n_sets;
  A.slice_agents = T->slice_agents;
  A.n_agents = plan->n_ext_agents;     // phase A also scatters the halo agents' values
  A.trans = st->transmission;
  A.qtrans = p->has_quarantine ? st->q_transmission : st->transmission;
  const size_t lds = slice_lds(T, sizeof(float));
  int rc = allow_lds(k_tile_scatter, lds);
  if (rc) return rc;
  rc = launch(k_tile_scatter, T->n_slices, kTileThreads, lds, stream, A);
  if (rc) return rc;
  return tiled_presum(plan, st, p, G, stream);
}

static int tiled_venues(const gj_plan* plan, const gj_agent_state* st, const gj_step_params* p, const Groups& G, int mode,
                        hipStream_t stream, const gj_aux* aux = nullptr) {
  const gj_tiled* T = plan->tiled;
  if (G.n == 0) return GJ_OK;
  if (T->n_work == 0) return mode == 2 ? GJ_OK : tiled_presum_reduce(plan, p, G, stream);
  TileBArgs B;
  for (int s = 0; s < GJ_MAX_SETS; ++s) B.sets[s] = TSetB{};
  size_t lds = 16;
  for (int g = 0; g < G.n; ++g) {
    const int s = G.set[g];
    const gj_tiled_set& S = T->sets[s];
    const gj_edge_set& E = plan->sets[s];
    TSetB& X = B.sets[s];
    X.blk_v0 = S.blk_v0;
    X.blk_e0 = S.blk_e0;
    X.e_lv = S.e_lv;
    // gj_aux.e_lv8: the same ids in one byte per slot, for the forward step of a set whose blocks hold <= 255 venues
    X.e_lv8 = (aux && !p->transpose) ? aux->e_lv8[s] : nullptr;
    if (X.e_lv8 && (S.max_block_venues > 255 || (uintptr_t)X.e_lv8 % 8 != 0)) return GJ_E_PLAN;
    X.e_cls = S.e_cls;
    X.val = S.val;
    X.v_pc = E.v_pcontact;
    X.cum = E.cum;
    X.stride = E.cum_stride;
    X.nk = S.n_blocks > 0 ? G.nk[g] : 0;
    if (uses_presum(plan, s)) X.nk = 0;          // pass 1 of the set is k_tile_presum's, pass 2 phase D's: nothing here
    X.direct = S.ell_k != 0;
    const NetGroup C = classify_group(p, G, g);
    X.leisure = C.leisure;
    memcpy(X.beta, C.beta, sizeof(X.beta));
    memcpy(X.table, C.table, sizeof(X.table));
    memcpy(X.age75, C.age75, sizeof(X.age75));
    if (C.leisure && !S.e_cls && E.n_edges > 0) return GJ_E_PLAN;
    if (const int rc = check_group(C)) return rc;
    X.pv_blk = nullptr;
    X.blk_r0 = nullptr;
    X.x = nullptr;
    X.n_x = 0;
    if (S.run_pv_blk && mode != 2) {     // run form: phase B reads the primary edges' values from the per-agent array
      if (X.leisure) return GJ_E_PLAN;
      X.x = (p->has_quarantine && !C.raw) ? st->q_transmission : st->transmission;
      if (!X.x) return GJ_E_NULL;
      if (!aligned16(X.x, S.run_pv_blk)) return GJ_E_PLAN;
      X.pv_blk = S.run_pv_blk;
      X.blk_r0 = S.run_blk_r0;
      X.n_x = plan->n_ext_agents;
    }
    // Phase B of a set that carries several networks sums all of them in one pass per group of slots, with an LDS
    // atomic only where a run of one venue ends (multi_sums; its pass-1 weights are class-major, padded to 4 or 8
    // networks).  Decided here, per set and step, from the active networks alone: such an item is bound by the LDS
    // pipe at any block or tile width.  A single-network set keeps run_sums - its items are bound by bytes.
    X.multinet = X.leisure && X.nk >= 2;
    const size_t n_sums = (size_t)X.nk * S.max_block_venues + 64;               // + a scratch sum per lane of a wave
    const size_t weights = !X.leisure ? 0 : 200 * ((size_t)(X.multinet ? class_pad(X.nk) : X.nk) + (size_t)X.nk);
    const size_t need = ((n_sums + 1) & ~(size_t)1) * sizeof(fx_t) + weights * sizeof(float) +   // (the weights 16-byte aligned)
                        2 * ((n_sums + 31) / 32 * 4);                                 // two flag bits per sum
    X.term_limit = venue_term_limit(S.max_venue_edges);
    if (X.nk && need > lds) lds = need;
  }
  B.work = T->work;
  B.tables = plan->tables;
  B.day_type = p->day_type;
  B.mode = mode;
  B.transpose = p->transpose;
  int rc = allow_lds(k_tile_venues, lds);
  if (rc) return rc;
  rc = launch(k_tile_venues, T->n_work, kTileThreads, lds, stream, B);
  if (rc || mode == 2) return rc;
  return tiled_presum_reduce(plan, p, G, stream);
}

static int tiled_agents(const gj_plan* plan, const gj_agent_state* st, const gj_step_params* p, const Groups& G,
                        const gj_step_io* io, int sample, hipStream_t stream) {
  const gj_tiled* T = plan->tiled;
  if (plan->n_agents == 0) return GJ_OK;
  TileDArgs D;
  fill_set_a(plan, p, G, D.sets);
  D.n_sets = plan->n_sets;
  D.slice_agents = T->slice_agents;
  D.n_agents = plan->n_agents;
  D.stage = st->current_stage;
  D.susceptibility = st->susceptibility;
  D.is_infected = st->is_infected;
  D.infection_time = st->infection_time;
  D.not_infected_probs = io ? io->not_infected_probs : nullptr;
  D.new_infected = io ? io->new_infected : nullptr;
  D.trans_susc = io ? io->trans_susc : nullptr;
  D.agent_sums = io ? io->agent_sums : nullptr;
  D.exp_noise = io ? io->exp_noise : nullptr;
  D.now = p->now;
  D.dt = p->delta_time;
  D.q_thr = p->q_threshold;
  D.has_q = p->has_quarantine;
  D.sample = sample;
  D.seed = p->seed;
  D.step = p->step;
  D.agent_offset = p->agent_offset;
  D.clock = p->clock;
  D.acc_scratch = T->agent_scratch;
  size_t lds = agents_lds(T);
  // direct form of pass 2: the sets whose cum is read from an LDS table behind the slice's (compacted) sums
  D.n_direct = 0;
  D.day_type = p->day_type;
  D.transpose = p->transpose;
  D.cls = plan->agent_class;
  D.tables = plan->tables;
  const int64_t owned_slices = (plan->n_agents + T->slice_agents - 1) / T->slice_agents;
  for (int g = 0; g < G.n; ++g) {
    const int s = G.set[g];
    const gj_tiled_set& S = T->sets[s];
    const gj_edge_set& E = plan->sets[s];
    const bool run = S.run_pv_win != nullptr;
    if ((!S.ell_k && !run) || S.n_blocks == 0 || E.n_edges == 0) continue;
    if (D.n_direct == GJ_MAX_DIRECT) return GJ_E_PLAN;
    TDirect& X = D.direct[D.n_direct++];
    X.ell = run ? S.run_pv_win : S.ell;
    X.cum = E.cum;
    X.planes = run ? 1 : S.ell_k / 2;
    X.plane_stride = owned_slices * (int64_t)T->slice_agents * 2;
    X.V = run ? S.run_max_window : (int32_t)E.n_venues;      // (run form: the table is one slice's window of cum)
    X.win_lo = run ? S.run_win_lo : nullptr;
    X.win_n = run ? S.run_win_n : nullptr;
    if (run && (uintptr_t)S.run_pv_win % 8 != 0) return GJ_E_PLAN;
    X.stride = E.cum_stride;
    const NetGroup C = classify_group(p, G, g);
    X.nk = C.nk;
    X.raw = C.raw;
    X.leisure = C.leisure;
    memcpy(X.table, C.table, sizeof(X.table));
    memcpy(X.age75, C.age75, sizeof(X.age75));
    if (C.leisure && !classes_by_dword(plan)) return GJ_E_PLAN;
    if (const int rc = check_group(C)) return rc;
  }
  D.table_floats = D.table1_floats = 0;
  D._pad3 = 0;
  if (D.n_direct) {
    // LDS of the direct form (the slice's sums are in registers by then): two class-weight buffers, then two table
    // regions, each followed by 64 floats of slack for the last DMA piece.  Region 0 takes the largest table (in
    // groups of venues if it is larger than everything), region 1 what is left: a set whose whole table fits there is
    // staged while the previous set - in region 0 - is still being read.
    const int64_t budget = 160 * 1024 / 4 - 2 * kClassWeightFloats - 2 * kWave;
    int64_t largest = 0;
    for (int t = 0; t < D.n_direct; ++t) {
      const int64_t sz = (int64_t)D.direct[t].V * D.direct[t].stride;
      largest = largest > sz ? largest : sz;
    }
    int64_t cap0 = largest < budget ? largest : budget;
    if (T->direct_table_floats > 0 && T->direct_table_floats < cap0) cap0 = T->direct_table_floats;
    if (cap0 < GJ_MAX_NETS_PER_SET) cap0 = GJ_MAX_NETS_PER_SET;
    int64_t cap1 = budget - cap0;
    if (T->direct_table_floats > 0 && T->direct_table_floats < cap1) cap1 = T->direct_table_floats;
    int prev_region = -1;
    for (int t = 0; t < D.n_direct; ++t) {
      TDirect& X = D.direct[t];
      const int64_t sz = (int64_t)X.V * X.stride;
      X.region = (prev_region == 0 && sz <= cap1) ? 1 : 0;
      const int64_t cap = X.region ? cap1 : cap0;
      X.group_venues = sz <= cap ? X.V : (int32_t)(cap / X.stride);
      if (X.group_venues < 1 || (X.win_lo && sz > cap)) return GJ_E_PLAN;   // a window is staged whole
      prev_region = X.region;
    }
    D.table_floats = (int32_t)cap0;
    D.table1_floats = (int32_t)cap1;
    const size_t direct_lds = 4 * ((size_t)2 * kClassWeightFloats + (size_t)cap0 + kWave + (size_t)cap1 + kWave);
    if (direct_lds > lds) lds = direct_lds;
  }
  D.io_vec4 = aligned16(D.susceptibility, D.not_infected_probs, D.new_infected, D.trans_susc, D.acc_scratch, D.agent_sums);
  int rc = allow_lds(k_tile_agents, lds);
  if (rc) return rc;
  rc = launch(k_tile_agents, owned_slices, kTileThreads, lds, stream, D);
  if (rc || !D.acc_scratch) return rc;
  return launch(k_tile_epilogue, grid_for(plan->n_agents), kThreads, 0, stream, D);
}

// ---- argument rules that several entry points share ----
// the symptoms update's inputs (gj_symptoms_update, gj_adjoint_symptoms, gj_symptoms_step_stats)
static int check_symptoms(const uint8_t* agent_class, const float* new_infected, const float* current_stage,
                          const float* next_stage, const float* time_to_next_stage, const gj_symptoms_params* params,
                          const float* progresses, const float* dwell) {
  if (!agent_class || !new_infected || !current_stage || !next_stage || !time_to_next_stage || !params)
    return GJ_E_NULL;
  if (params->n_stages < 3 || params->n_stages > GJ_MAX_STAGES) return GJ_E_RANGE;
  if ((progresses == nullptr) != (dwell == nullptr)) return GJ_E_NULL;   // inject both or neither
  if (!progresses && !params->progress) return GJ_E_NULL;
  return GJ_OK;
}

// the per-step statistics' arguments and grid (gj_step_stats, gj_symptoms_step_stats); vec4: every array the kernel reads
// four agents at a time is 16-byte aligned
static StatsArgs stats_args(int64_t n, const uint8_t* agent_class, const float* is_infected, const float* current_stage,
                            int32_t n_bins, const int32_t* bin_edges, int32_t dead_stage, double* out, bool vec4) {
  StatsArgs S;
  S.n = n;
  S.cls = agent_class;
  S.inf = is_infected;
  S.stage = current_stage;
  S.n_bins = n_bins;
  for (int b = 0; b <= GJ_MAX_AGE_BINS; ++b) S.edges[b] = (b <= n_bins) ? bin_edges[b] : 0;
  S.dead = dead_stage;
  S.vec4 = (vec4 && (uintptr_t)agent_class % 4 == 0) ? 1 : 0;
  S.out = out;
  return S;
}
// lanes of a kernel that takes four agents per lane where vec4 holds (+ 3: the scalar tail's lanes)
static inline int64_t vec4_lanes(int64_t n, int vec4) { return vec4 ? (n >> 2) + 3 : n; }

// the required arguments of the transmission adjoint (gj_adjoint_transmission, gj_adjoint_transmission_params)
static int check_profile_adjoint(const gj_agent_state* st, const float* trans_bar, const float* grad_inf_out,
                                 const float* grad_time_inout) {
  if (!st || !trans_bar || !grad_inf_out || !grad_time_inout) return GJ_E_NULL;
  if (!st->max_infectiousness || !st->shape || !st->rate || !st->shift || !st->infection_time || !st->is_infected)
    return GJ_E_NULL;
  return GJ_OK;
}

}  // namespace gj


// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

#ifdef GJ_DIAG_STAMPS
// diagnostics build only: the venue launch's per-workgroup timestamps, [3 * 8192] uint64 (start, end, XCD) to host memory
int gj_diag_venue_stamps(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(gj::gj_diag_venue), sizeof(unsigned long long) * 3 * gj::kDiagVenueSlots);
}
#endif

int gj_version(void) { return GJ_ABI_VERSION; }

const char* gj_error_string(int code) {
  switch (code) {
    case GJ_OK: return "ok";
    case GJ_E_NULL: return "required pointer is NULL";
    case GJ_E_RANGE: return "count or index out of range";
    case GJ_E_PLAN: return "inconsistent plan or network list";
    case GJ_E_NODEVICE: return "no HIP device, or not a gfx950 (MI355X) device";
    default: break;
  }
  if (code > 0) return hipGetErrorString((hipError_t)code);
  return "unknown error";
}

int gj_check_device(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return GJ_E_NODEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return GJ_E_NODEVICE;
  // the code object holds gfx950 (CDNA4, MI355X) kernels only, sized for its 160 KiB of LDS per CU
  const char* want = "gfx950";
  for (int i = 0; want[i]; ++i)
    if (prop.gcnArchName[i] != want[i]) return GJ_E_NODEVICE;
  return GJ_OK;
}

int gj_transmission_update(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params,
                           void* stream) {
  int rc = gj::check_plan(plan);
  if (rc) return rc;
  if (!params) return GJ_E_NULL;
  rc = gj::check_state(plan, state, params);
  if (rc) return rc;
  return gj::do_transmission(plan, state, params, (hipStream_t)stream);
}

int gj_quarantine_transmission(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params,
                               void* stream) {
  int rc = gj::check_plan(plan);
  if (rc) return rc;
  if (!params) return GJ_E_NULL;
  rc = gj::check_state(plan, state, params, false);
  if (rc) return rc;
  if (!params->has_quarantine || plan->n_agents == 0) return GJ_OK;
  const int64_t n = plan->n_agents;
  return gj::launch(gj::k_quarantine_transmission, gj::grid_for(n), gj::kThreads, 0, (hipStream_t)stream, n,
                    state->current_stage, state->transmission, state->q_transmission, params->q_threshold);
}

int gj_venue_reduce(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params, void* stream) {
  int rc = gj::check_plan(plan);
  if (rc) return rc;
  gj::Groups G;
  rc = gj::group_networks(plan, params, &G);
  if (rc) return rc;
  rc = gj::check_state(plan, state, params, false);
  if (rc) return rc;
  if (plan->tiled) {
    rc = gj::tiled_scatter(plan, state, params, G, (hipStream_t)stream);
    if (rc) return rc;
    return gj::tiled_venues(plan, state, params, G, 1, (hipStream_t)stream);
  }
  return gj::do_venue_reduce(plan, state, params, G, (hipStream_t)stream);
}

int gj_agent_gather(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params,
                    const gj_step_io* io, int sample, void* stream) {
  int rc = gj::check_plan(plan);
  if (rc) return rc;
  gj::Groups G;
  rc = gj::group_networks(plan, params, &G);
  if (rc) return rc;
  rc = gj::check_state(plan, state, params, sample != 0);
  if (rc) return rc;
  if (plan->tiled) {
    rc = gj::tiled_venues(plan, state, params, G, 2, (hipStream_t)stream);
    if (rc) return rc;
    return gj::tiled_agents(plan, state, params, G, io, sample, (hipStream_t)stream);
  }
  return gj::do_agent_gather(plan, state, params, G, io, sample, (hipStream_t)stream);
}

int gj_sample_infect(int64_t n_agents, const float* not_infected_probs, const float* exp_noise, uint64_t seed,
                     uint64_t step, int64_t agent_offset, float now, float* new_infected, float* susceptibility,
                     float* is_infected, float* infection_time, void* stream) {
  if (n_agents < 0) return GJ_E_RANGE;
  if (n_agents == 0) return GJ_OK;
  if (!not_infected_probs) return GJ_E_NULL;
  const int n_state = (susceptibility != nullptr) + (is_infected != nullptr) + (infection_time != nullptr);
  if (n_state != 0 && n_state != 3) return GJ_E_NULL;   // all three or none (sample only)
  if (n_state == 0 && !new_infected) return GJ_E_NULL;
  return gj::launch(gj::k_sample_infect, gj::grid_for(n_agents), gj::kThreads, 0, (hipStream_t)stream, n_agents,
                    not_infected_probs, exp_noise, seed, step, agent_offset, now, new_infected, susceptibility,
                    is_infected, infection_time);
}

int gj_adjoint_sample(int64_t n, const float* susceptibility0, const float* infection_time0, const float* acc,
                      const float* exp_noise, uint64_t seed, uint64_t step, int64_t agent_offset, float now,
                      float delta_time, const float* g_susc, const float* g_inf, const float* g_time,
                      const float* g_new, float* x_out, float* grad_susc_out, float* grad_time_out, void* stream) {
  if (n < 0) return GJ_E_RANGE;
  if (n == 0) return GJ_OK;
  if (!susceptibility0 || !infection_time0 || !acc || !x_out || !grad_susc_out || !grad_time_out) return GJ_E_NULL;
  return gj::launch(gj::k_adjoint_sample, gj::grid_for(n), gj::kThreads, 0, (hipStream_t)stream, n, susceptibility0,
                    infection_time0, acc, exp_noise, seed, step, agent_offset, now, delta_time, g_susc, g_inf, g_time,
                    g_new, x_out, grad_susc_out, grad_time_out);
}

namespace gj {
// The fp64 sums of gj_adjoint_seed and gj_adjoint_vaccinate: their arguments from the labelling's gj_seed_plan (checked
// here; `plan` NULL: no labels, one group of all n agents, cut into chunks in index order) and their two launches.
static int seed_sum_args(const gj_seed_plan* plan, int64_t n, int32_t n_groups, double* contrib, double* partial,
                         double* out, SeedSumArgs& R) {
  R.n = n;
  R.n_groups = n_groups;
  R.contrib = contrib;
  R.partial = partial;
  R.out = out;
  if (plan) {
    if (plan->n_sorted < 0 || plan->n_sorted > n || plan->n_chunks < 0 ||
        plan->n_chunks > plan->n_sorted / GJ_SEED_CHUNK + n_groups)
      return GJ_E_RANGE;
    if (!plan->seg_offsets || !plan->chunk_first) return GJ_E_NULL;
    if (plan->n_chunks > 0 && (!plan->order || !plan->chunk_group)) return GJ_E_NULL;
    R.n_sorted = plan->n_sorted;
    R.n_chunks = plan->n_chunks;
    R.order = plan->order;
    R.seg_offsets = plan->seg_offsets;
    R.chunk_first = plan->chunk_first;
    R.chunk_group = plan->chunk_group;
  } else {
    R.n_sorted = n;
    R.n_chunks = (n + GJ_SEED_CHUNK - 1) / GJ_SEED_CHUNK;
    R.order = nullptr;
    R.seg_offsets = nullptr;
    R.chunk_first = nullptr;
    R.chunk_group = nullptr;
  }
  if (grid_for(R.n_chunks, 0, kThreads / kWave) > 0x7fffffff) return GJ_E_RANGE;
  if (n > 0 && !contrib) return GJ_E_NULL;
  if (R.n_chunks > 0 && !partial) return GJ_E_NULL;
  return GJ_OK;
}
static int seed_sum_launch(const SeedSumArgs& R, hipStream_t stream) {
  constexpr int kWaves = kThreads / kWave;      // one wave per chunk, then one per group
  if (R.n_chunks > 0) {
    const int rc = launch(k_adjoint_seed_chunks, grid_for(R.n_chunks, 0, kWaves), kThreads, 0, stream, R);
    if (rc) return rc;
  }
  return launch(k_adjoint_seed_finish, grid_for(R.n_groups, 0, kWaves), kThreads, 0, stream, R);
}
}  // namespace gj

int gj_adjoint_seed(int64_t n, const float* p_not_by_group, const int32_t* group, int32_t n_groups,
                    const gj_seed_plan* plan, const float* susceptibility0, const float* infection_time0,
                    const float* exp_noise, uint64_t seed, uint64_t step, int64_t agent_offset, float now,
                    const float* g_susc, const float* g_inf, const float* g_time, const float* g_new,
                    double* contrib_workspace, double* partial_workspace, double* grad_fraction, float* grad_susc_out,
                    float* grad_time_out, void* stream) {
  if (n < 0 || n_groups < 1 || n_groups > GJ_MAX_GROUPS) return GJ_E_RANGE;
  if (!group && n_groups != 1) return GJ_E_RANGE;
  if (!grad_fraction) return GJ_E_NULL;
  if (group && !plan) return GJ_E_NULL;
  gj::SeedSumArgs R;
  if (const int rc = gj::seed_sum_args(group ? plan : nullptr, n, n_groups, contrib_workspace, partial_workspace,
                                       grad_fraction, R))
    return rc;
  const int64_t agent_blocks = gj::grid_for(n);
  if (agent_blocks > 0x7fffffff) return GJ_E_RANGE;
  if (n > 0 && (!p_not_by_group || !susceptibility0 || !infection_time0)) return GJ_E_NULL;
  if (n > 0) {
    gj::SeedAdjArgs A;
    A.n = n;
    A.p_not = p_not_by_group;
    A.group = group;
    A.n_groups = n_groups;
    A.susc0 = susceptibility0;
    A.time0 = infection_time0;
    A.noise = exp_noise;
    A.seed = seed;
    A.step = step;
    A.agent_offset = agent_offset;
    A.now = now;
    A.g_susc = g_susc;
    A.g_inf = g_inf;
    A.g_time = g_time;
    A.g_new = g_new;
    A.contrib = contrib_workspace;
    A.grad_susc = grad_susc_out;
    A.grad_time = grad_time_out;
    const int rc = gj::launch(gj::k_adjoint_seed_agents, agent_blocks, gj::kThreads, 0, (hipStream_t)stream, A);
    if (rc) return rc;
  }
  return gj::seed_sum_launch(R, (hipStream_t)stream);
}

// vaccination: the tables are copied into the launch's arguments (the caller's struct may change after the call returns)
int gj_vaccinate(int64_t n, const uint8_t* agent_class, const gj_vaccinate_tables* tables, uint64_t seed,
                 uint64_t stream, int64_t agent_offset, float* susceptibility, float* newly_out, int64_t* count_out,
                 void* hip_stream) {
  if (n < 0 || agent_offset < 0) return GJ_E_RANGE;
  if (n == 0) return GJ_OK;
  if (!agent_class || !tables || !susceptibility) return GJ_E_NULL;
  gj::VaccinateArgs A;
  A.T = *tables;
  A.n = n;
  A.cls = agent_class;
  A.seed = seed;
  A.stream = stream;
  A.agent_offset = agent_offset;
  A.susc = susceptibility;
  A.newly = newly_out;
  A.count = reinterpret_cast<unsigned long long*>(count_out);
  A.vec4 = (agent_offset % 4 == 0 && gj::aligned16(susceptibility, newly_out) && (uintptr_t)agent_class % 4 == 0) ? 1 : 0;
  return gj::launch(gj::k_vaccinate, gj::grid_for(gj::vec4_lanes(n, A.vec4), gj::kVaccineBlocks, gj::kVaccineThreads),
                    gj::kVaccineThreads, 0, (hipStream_t)hip_stream, A);
}

int gj_adjoint_vaccinate(int64_t n, const uint8_t* agent_class, const gj_vaccinate_tables* tables, uint64_t seed,
                         uint64_t stream, int64_t agent_offset, const float* susceptibility0, const float* g_out,
                         const int32_t* band, int32_t n_bands, const gj_seed_plan* plan, double* contrib_workspace,
                         double* partial_workspace, double* grad_efficacy, float* g_in, void* hip_stream) {
  if (n < 0 || agent_offset < 0 || n_bands < 1 || n_bands > GJ_MAX_GROUPS) return GJ_E_RANGE;
  if (!grad_efficacy || !plan) return GJ_E_NULL;
  gj::SeedSumArgs R;
  if (const int rc = gj::seed_sum_args(plan, n, n_bands, contrib_workspace, partial_workspace, grad_efficacy, R))
    return rc;
  if (n > 0) {
    if (!agent_class || !tables || !susceptibility0 || !band) return GJ_E_NULL;
    gj::VaccinateAdjArgs A;
    A.T = *tables;
    A.n = n;
    A.cls = agent_class;
    A.seed = seed;
    A.stream = stream;
    A.agent_offset = agent_offset;
    A.susc0 = susceptibility0;
    A.g_out = g_out;
    A.band = band;
    A.n_bands = n_bands;
    A.vec4 = (agent_offset % 4 == 0 && gj::aligned16(susceptibility0, g_out, g_in) && gj::aligned16(band) &&
              gj::aligned16(contrib_workspace) && (uintptr_t)agent_class % 4 == 0) ? 1 : 0;
    A.contrib = contrib_workspace;
    A.g_in = g_in;
    const int rc = gj::launch(gj::k_adjoint_vaccinate_agents, gj::grid_for(gj::vec4_lanes(n, A.vec4), 2048),
                              gj::kThreads, 0, (hipStream_t)hip_stream, A);
    if (rc) return rc;
  }
  return gj::seed_sum_launch(R, (hipStream_t)hip_stream);
}

// waning immunity: the tables are copied into the launch's arguments, as gj_vaccinate's are
int gj_immunity_step(int64_t n, const uint8_t* agent_class, const gj_immunity_tables* tables, const float* current_stage,
                     int32_t recovered_stage, const float* new_infected, float* susceptibility, float* is_infected,
                     uint8_t* flags_out, float* reinfected_out, int64_t* count_out, int64_t* susc_sum_out,
                     void* hip_stream) {
  if (n < 0 || recovered_stage < 0 || recovered_stage >= GJ_MAX_STAGES) return GJ_E_RANGE;
  if (n == 0) return GJ_OK;
  if (!agent_class || !tables || !current_stage || !susceptibility || !is_infected) return GJ_E_NULL;
  gj::ImmunityArgs A;
  A.T = *tables;
  A.n = n;
  A.cls = agent_class;
  A.stage = current_stage;
  A.recovered = (float)recovered_stage;
  A.new_inf = new_infected;
  A.susc = susceptibility;
  A.inf = is_infected;
  A.flags = flags_out;
  A.reinf = reinfected_out;
  A.count = reinterpret_cast<unsigned long long*>(count_out);
  A.susc_sum = reinterpret_cast<unsigned long long*>(susc_sum_out);
  A.vec4 = (gj::aligned16(current_stage, new_infected, susceptibility, is_infected, reinfected_out) &&
            (uintptr_t)agent_class % 4 == 0 && (uintptr_t)flags_out % 4 == 0) ? 1 : 0;
  return gj::launch(gj::k_immunity, gj::grid_for(gj::vec4_lanes(n, A.vec4), gj::kVaccineBlocks, gj::kVaccineThreads),
                    gj::kVaccineThreads, 0, (hipStream_t)hip_stream, A);
}

int gj_adjoint_immunity(int64_t n, const uint8_t* flags, const uint8_t* agent_class, const gj_immunity_tables* tables,
                        const float* susceptibility0, const float* g_susc, const float* g_inf, const int32_t* band,
                        int32_t n_bands, const gj_seed_plan* plan, double* contrib_workspace, double* partial_workspace,
                        double* sum_A, double* sum_B, float* g_susc_in, float* g_inf_in, float* g_new,
                        void* hip_stream) {
  if (n < 0 || n_bands < 1 || n_bands > GJ_MAX_GROUPS) return GJ_E_RANGE;
  if (!sum_A || !sum_B || !plan) return GJ_E_NULL;
  gj::SeedSumArgs RA, RB;
  if (const int rc = gj::seed_sum_args(plan, n, n_bands, contrib_workspace, partial_workspace, sum_A, RA)) return rc;
  if (const int rc = gj::seed_sum_args(plan, n, n_bands, contrib_workspace ? contrib_workspace + n : nullptr,
                                       partial_workspace ? partial_workspace + RA.n_chunks : nullptr, sum_B, RB))
    return rc;
  if (n > 0) {
    if (!flags || !agent_class || !tables || !susceptibility0 || !band) return GJ_E_NULL;
    gj::ImmunityAdjArgs A;
    A.T = *tables;
    A.n = n;
    A.flags = flags;
    A.cls = agent_class;
    A.susc0 = susceptibility0;
    A.g_susc = g_susc;
    A.g_inf = g_inf;
    A.band = band;
    A.n_bands = n_bands;
    A.contrib_a = contrib_workspace;
    A.contrib_b = contrib_workspace + n;
    A.g_susc_in = g_susc_in;
    A.g_inf_in = g_inf_in;
    A.g_new = g_new;
    A.vec4 = (gj::aligned16(susceptibility0, g_susc, g_inf, g_susc_in, g_inf_in, g_new) && gj::aligned16(band) &&
              gj::aligned16(A.contrib_a, A.contrib_b) && (uintptr_t)agent_class % 4 == 0 && (uintptr_t)flags % 4 == 0)
                 ? 1 : 0;
    const int rc = gj::launch(gj::k_adjoint_immunity_agents, gj::grid_for(gj::vec4_lanes(n, A.vec4), 2048), gj::kThreads,
                              0, (hipStream_t)hip_stream, A);
    if (rc) return rc;
  }
  if (const int rc = gj::seed_sum_launch(RA, (hipStream_t)hip_stream)) return rc;
  return gj::seed_sum_launch(RB, (hipStream_t)hip_stream);
}

namespace gj {
// the sets of gj_contact_mark / gj_contact_mask, checked and copied into the launch's arguments (the caller's array may
// change after the call returns); `marking`: the release time is read, and must be a non-negative number
static int contact_sets(const gj_contact_set* sets, int32_t n_sets, bool marking, ContactSet* out) {
  if (n_sets < 1 || n_sets > GJ_MAX_SETS) return GJ_E_RANGE;
  if (!sets) return GJ_E_NULL;
  for (int s = 0; s < GJ_MAX_SETS; ++s) out[s] = ContactSet{};
  for (int s = 0; s < n_sets; ++s) {
    const gj_contact_set& S = sets[s];
    if (S.n_venues < 0 || S.n_venues > INT32_MAX) return GJ_E_RANGE;
    if (marking && !(S.release >= 0.0f)) return GJ_E_RANGE;                  // (a NaN too)
    if (!S.a_rowptr || !S.a_venue || !S.until) return GJ_E_NULL;
    uint32_t bits = 0;
    if (marking) memcpy(&bits, &S.release, sizeof bits);
    out[s] = ContactSet{S.a_rowptr, S.a_venue, S.until, (int32_t)S.n_venues, bits & 0x7fffffffu};   // (-0 marks as +0)
  }
  return GJ_OK;
}
}  // namespace gj

int gj_contact_mark(int64_t n, const float* current_stage, float stage_threshold, const gj_contact_set* sets,
                    int32_t n_sets, uint32_t* err, void* stream) {
  if (n < 0) return GJ_E_RANGE;
  gj::ContactMarkArgs A;
  if (const int rc = gj::contact_sets(sets, n_sets, true, A.sets)) return rc;
  if (!err || (n > 0 && !current_stage)) return GJ_E_NULL;
  if (n == 0) return GJ_OK;
  A.n = n;
  A.stage = current_stage;
  A.err = err;
  A.threshold = stage_threshold;
  A.n_sets = n_sets;
  A.vec4 = gj::aligned16(current_stage) ? 1 : 0;
  return gj::launch(gj::k_contact_mark, gj::grid_for(gj::vec4_lanes(n, A.vec4), gj::kContactBlocks), gj::kThreads, 0,
                    (hipStream_t)stream, A);
}

int gj_contact_mask(int64_t n, const float* current_stage, float q_threshold, const gj_contact_set* sets,
                    int32_t n_sets, float now, float compliance, uint64_t seed, uint64_t stream, int64_t agent_offset,
                    float* qstate, uint32_t* err, void* hip_stream) {
  if (n < 0 || agent_offset < 0) return GJ_E_RANGE;
  gj::ContactMaskArgs A;
  if (const int rc = gj::contact_sets(sets, n_sets, false, A.sets)) return rc;
  if (!err || (n > 0 && (!current_stage || !qstate))) return GJ_E_NULL;
  if (n == 0) return GJ_OK;
  A.n = n;
  A.stage = current_stage;
  A.qstate = qstate;
  A.err = err;
  A.seed = seed;
  A.stream = stream;
  A.agent_offset = agent_offset;
  A.threshold = q_threshold;
  A.now = now;
  A.compliance = compliance;
  A.n_sets = n_sets;
  A.vec4 = (agent_offset % 4 == 0 && gj::aligned16(current_stage, qstate)) ? 1 : 0;
  return gj::launch(gj::k_contact_mask, gj::grid_for(gj::vec4_lanes(n, A.vec4), gj::kContactBlocks), gj::kThreads, 0,
                    (hipStream_t)hip_stream, A);
}

// testing: the tables are copied into the launch's arguments, as gj_vaccinate's are
int gj_testing_step(int64_t n, const uint8_t* agent_class, const gj_testing_tables* tables, const float* current_stage,
                    const float* infection_time, float stage_threshold, int32_t active, float now, float q_threshold,
                    float isolate_release, float compliance, uint64_t seed, uint64_t decide_stream,
                    uint64_t comply_stream, int64_t agent_offset, uint32_t* decided, float* result_time, float* positive,
                    float* isolate_until, float* confirmed_time, float* newly_confirmed_out, float* qstate_out,
                    uint8_t* flags_out, int64_t* counts_out, void* hip_stream) {
  if (n < 0 || agent_offset < 0 || !(now >= 0.0f) || (decide_stream & 0xFFFFFFFFull)) return GJ_E_RANGE;
  if (n == 0) return GJ_OK;
  if (!tables) return GJ_E_NULL;
  if (tables->n_delays < 1 || tables->n_delays > GJ_TESTING_MAX_DELAYS) return GJ_E_RANGE;
  if (qstate_out && !isolate_until) return GJ_E_NULL;
  if (!agent_class || !current_stage || !infection_time || !decided || !result_time || !positive || !confirmed_time)
    return GJ_E_NULL;
  gj::TestingArgs A;
  A.T = *tables;
  A.n = n;
  A.cls = agent_class;
  A.stage = current_stage;
  A.inf_time = infection_time;
  A.decided = decided;
  A.result_time = result_time;
  A.positive = positive;
  A.isolate_until = isolate_until;
  A.confirmed_time = confirmed_time;
  A.newly = newly_confirmed_out;
  A.qstate = qstate_out;
  A.flags = flags_out;
  A.counts = reinterpret_cast<unsigned long long*>(counts_out);
  A.seed = seed;
  A.decide_stream = decide_stream;
  A.comply_stream = comply_stream;
  A.agent_offset = agent_offset;
  A.threshold = stage_threshold;
  A.q_threshold = q_threshold;
  A.now = now;
  A.release = isolate_release;
  A.compliance = compliance;
  A.active = active ? 1 : 0;
  A.vec4 = (gj::aligned16(current_stage, infection_time, result_time, isolate_until, newly_confirmed_out, qstate_out) &&
            (uintptr_t)decided % 16 == 0 && (uintptr_t)agent_class % 4 == 0 && (uintptr_t)flags_out % 4 == 0) ? 1 : 0;
  return gj::launch(gj::k_testing_step, gj::grid_for(gj::vec4_lanes(n, A.vec4), gj::kVaccineBlocks, gj::kVaccineThreads),
                    gj::kVaccineThreads, 0, (hipStream_t)hip_stream, A);
}

int gj_adjoint_testing(int64_t n, const uint8_t* flags, const float* current_stage, const float* g_y, const float* g_row,
                       const int32_t* band, int32_t n_bands, const gj_seed_plan* plan, double* contrib_workspace,
                       double* partial_workspace, double* grad_probability, float* g_stage, float* g_y_in,
                       void* hip_stream) {
  if (n < 0 || n_bands < 1 || n_bands > GJ_MAX_GROUPS) return GJ_E_RANGE;
  if (!grad_probability || !plan) return GJ_E_NULL;
  gj::SeedSumArgs R;
  if (const int rc = gj::seed_sum_args(plan, n, n_bands, contrib_workspace, partial_workspace, grad_probability, R))
    return rc;
  if (n > 0) {
    if (!flags || !current_stage || !band) return GJ_E_NULL;
    gj::TestingAdjArgs A;
    A.n = n;
    A.flags = flags;
    A.stage = current_stage;
    A.g_y = g_y;
    A.g_row = g_row;
    A.band = band;
    A.n_bands = n_bands;
    A.vec4 = (gj::aligned16(current_stage, g_y, g_stage, g_y_in) && gj::aligned16(band) &&
              gj::aligned16(contrib_workspace) && (uintptr_t)flags % 4 == 0) ? 1 : 0;
    A.contrib = contrib_workspace;
    A.g_stage = g_stage;
    A.g_y_in = g_y_in;
    const int rc = gj::launch(gj::k_adjoint_testing, gj::grid_for(gj::vec4_lanes(n, A.vec4), 2048), gj::kThreads, 0,
                              (hipStream_t)hip_stream, A);
    if (rc) return rc;
  }
  return gj::seed_sum_launch(R, (hipStream_t)hip_stream);
}

int gj_adjoint_transmission(int64_t n, const gj_agent_state* st, float now, const float* trans_bar,
                            const float* g_inf, float* grad_inf_out, float* grad_time_inout, void* stream) {
  if (n < 0) return GJ_E_RANGE;
  if (n == 0) return GJ_OK;
  if (const int rc = gj::check_profile_adjoint(st, trans_bar, grad_inf_out, grad_time_inout)) return rc;
  return gj::launch(gj::k_adjoint_transmission, gj::grid_for(n), gj::kThreads, 0, (hipStream_t)stream, n,
                    st->max_infectiousness, st->shape, st->rate, st->shift, st->infection_time, st->is_infected, now,
                    trans_bar, g_inf, grad_inf_out, grad_time_inout);
}

int gj_adjoint_transmission_params(int64_t n, const gj_agent_state* st, float now, const float* trans_bar,
                                   const float* g_inf, float* grad_inf_out, float* grad_time_inout,
                                   float* grad_max_infectiousness_out, float* grad_shape_out, float* grad_rate_out,
                                   float* grad_shift_out, void* stream) {
  if (n < 0) return GJ_E_RANGE;
  if (n == 0) return GJ_OK;
  if (const int rc = gj::check_profile_adjoint(st, trans_bar, grad_inf_out, grad_time_inout)) return rc;
  return gj::launch(gj::k_adjoint_transmission_params, gj::grid_for(n), gj::kThreads, 0, (hipStream_t)stream, n,
                    st->max_infectiousness, st->shape, st->rate, st->shift, st->infection_time, st->is_infected, now,
                    trans_bar, g_inf, grad_inf_out, grad_time_inout, grad_max_infectiousness_out, grad_shape_out,
                    grad_rate_out, grad_shift_out);
}

int gj_adjoint_beta_partial(int64_t n_venues, int32_t stride, int32_t nk, const float* cum_fwd, const float* cum_bwd,
                            const float* v_pcontact, const double* weights, const float* beta, const int32_t* cols,
                            double* partial, void* stream) {
  if (n_venues < 0 || stride < 1 || stride > GJ_MAX_NETS_PER_SET || nk < 0 || nk > stride) return GJ_E_RANGE;
  if (!partial || (nk > 0 && (!beta || !cols))) return GJ_E_NULL;
  if (n_venues == 0 || nk == 0) return GJ_OK;
  if (!cum_fwd || !cum_bwd || !v_pcontact) return GJ_E_NULL;
  gj::AdjBetaArgs A;
  A.n_venues = n_venues;
  A.stride = stride;
  A.nk = nk;
  A.cum_fwd = cum_fwd;
  A.cum_bwd = cum_bwd;
  A.v_pc = v_pcontact;
  A.weights = weights;
  for (int k = 0; k < GJ_MAX_NETS_PER_SET; ++k) {
    A.beta[k] = k < nk ? beta[k] : 0.0f;
    A.cols[k] = k < nk ? cols[k] : 0;
    if (k < nk && (cols[k] < 0 || cols[k] >= GJ_MAX_NETS)) return GJ_E_RANGE;
  }
  A.partial = partial;
  return gj::launch(gj::k_adjoint_beta_partial, GJ_ADJ_BETA_BLOCKS, gj::kAdjBetaThreads, 0, (hipStream_t)stream, A);
}

int gj_adjoint_beta_finish(int32_t n_cols, const double* partial, const float* scale, double* out, void* stream) {
  if (n_cols < 0 || n_cols > GJ_MAX_NETS) return GJ_E_RANGE;
  if (n_cols == 0) return GJ_OK;
  if (!partial || !scale || !out) return GJ_E_NULL;
  return gj::launch(gj::k_adjoint_beta_finish, 1, 64, 0, (hipStream_t)stream, n_cols, partial, scale, out);
}

int gj_symptoms_update(int64_t n, const uint8_t* agent_class, const float* new_infected, float* current_stage,
                       float* next_stage, float* time_to_next_stage, const gj_symptoms_params* params,
                       const float* progresses, const float* dwell, void* stream) {
  if (n < 0) return GJ_E_RANGE;
  if (n == 0) return GJ_OK;
  if (const int rc = gj::check_symptoms(agent_class, new_infected, current_stage, next_stage, time_to_next_stage, params,
                                        progresses, dwell))
    return rc;
  const gj::SymptomsArgs S = {*params, n, agent_class, new_infected, current_stage, next_stage, time_to_next_stage,
                              progresses, dwell};
  return gj::launch(gj::k_symptoms, gj::grid_for(n), gj::kThreads, 0, (hipStream_t)stream, S);
}

int gj_adjoint_symptoms(int64_t n, const uint8_t* agent_class, const float* new_infected,
                        const float* current_stage0, const float* next_stage0, const float* time_to_next_stage0,
                        const gj_symptoms_params* params, const float* progresses, const float* dwell,
                        const float* g_current, const float* g_next, const float* g_time, float* g_current_in,
                        float* g_next_in, float* g_time_in, float* g_new_infected, void* stream) {
  if (n < 0) return GJ_E_RANGE;
  if (n == 0) return GJ_OK;
  if (!g_current_in || !g_next_in || !g_new_infected) return GJ_E_NULL;
  if (const int rc = gj::check_symptoms(agent_class, new_infected, current_stage0, next_stage0, time_to_next_stage0,
                                        params, progresses, dwell))
    return rc;
  gj::SymptomsAdjointArgs S;
  S.P = *params;
  S.n = n;
  S.cls = agent_class;
  S.new_inf = new_infected;
  S.cur0 = current_stage0;
  S.nxt0 = next_stage0;
  S.ttn0 = time_to_next_stage0;
  S.progresses = progresses;
  S.dwell = dwell;
  S.g_cur = g_current;
  S.g_nxt = g_next;
  S.g_ttn = g_time;
  S.g_cur_in = g_current_in;
  S.g_nxt_in = g_next_in;
  S.g_ttn_in = g_time_in;
  S.g_new = g_new_infected;
  return gj::launch(gj::k_adjoint_symptoms, gj::grid_for(n), gj::kThreads, 0, (hipStream_t)stream, S);
}

int gj_step_stats(int64_t n, const uint8_t* agent_class, const float* is_infected, const float* current_stage,
                  int32_t n_bins, const int32_t* bin_edges, int32_t dead_stage, double* out, void* stream) {
  if (n < 0 || n_bins < 0 || n_bins > GJ_MAX_AGE_BINS) return GJ_E_RANGE;
  if (!out || (n_bins > 0 && !bin_edges)) return GJ_E_NULL;
  if (n == 0) return GJ_OK;
  if (!agent_class || !is_infected || !current_stage) return GJ_E_NULL;
  const gj::StatsArgs S = gj::stats_args(n, agent_class, is_infected, current_stage, n_bins, bin_edges, dead_stage, out,
                                         gj::aligned16(is_infected, current_stage));
  return gj::launch(gj::k_step_stats, gj::grid_for(gj::vec4_lanes(n, S.vec4), 2048), gj::kThreads, 0,
                    (hipStream_t)stream, S);
}

int gj_symptoms_step_stats(int64_t n, const uint8_t* agent_class, const float* new_infected, float* current_stage,
                           float* next_stage, float* time_to_next_stage, const gj_symptoms_params* params,
                           const float* progresses, const float* dwell, const float* is_infected, int32_t n_bins,
                           const int32_t* bin_edges, int32_t dead_stage, double* out, void* stream) {
  if (n < 0 || n_bins < 0 || n_bins > GJ_MAX_AGE_BINS) return GJ_E_RANGE;
  if (!out || (n_bins > 0 && !bin_edges)) return GJ_E_NULL;
  if (n == 0) return GJ_OK;
  if (!is_infected) return GJ_E_NULL;
  if (const int rc = gj::check_symptoms(agent_class, new_infected, current_stage, next_stage, time_to_next_stage, params,
                                        progresses, dwell))
    return rc;
  const gj::SymptomsArgs S = {*params, n, agent_class, new_infected, current_stage, next_stage, time_to_next_stage,
                              progresses, dwell};
  const gj::StatsArgs R =
      gj::stats_args(n, agent_class, is_infected, current_stage, n_bins, bin_edges, dead_stage, out,
                     gj::aligned16(new_infected, current_stage, next_stage, time_to_next_stage, is_infected));
  return gj::launch(gj::k_symptoms_stats, gj::grid_for(gj::vec4_lanes(n, R.vec4), 4096), gj::kThreads, 0,
                    (hipStream_t)stream, S, R);
}

int gj_group_stats(int64_t n, const int32_t* group, int32_t n_groups, const float* is_infected,
                   const float* current_stage, int32_t dead_stage, double* out, void* workspace, void* stream) {
  if (n < 0 || n_groups < 1 || n_groups > GJ_MAX_GROUPS) return GJ_E_RANGE;
  if (!out || !workspace) return GJ_E_NULL;
  if (n == 0) return GJ_OK;
  if (!group || !is_infected || !current_stage) return GJ_E_NULL;
  gj::GroupArgs S;
  S.n = n;
  S.group = group;
  S.inf = is_infected;
  S.stage = current_stage;
  S.n_groups = n_groups;
  S.dead = dead_stage;
  S.vec4 = gj::aligned16(group, is_infected, current_stage);
  S.ws = (gj::fx_t*)workspace;
  const int64_t units = S.vec4 ? (n >> 2) + 1 : n;
  const int rc =
      n_groups <= gj::kGroupLdsMax       // regimes (i) and (iii): a histogram in LDS per workgroup
          ? gj::launch(gj::k_group_stats<true>, gj::grid_for(units, gj::kGroupLdsBlocks, gj::kGroupLdsThreads),
                       gj::kGroupLdsThreads, (size_t)n_groups * 2 * sizeof(gj::fx_t), (hipStream_t)stream, S)
          // regime (ii): one global atomic per run of equal labels in a wave
          : gj::launch(gj::k_group_stats<false>, gj::grid_for(units, 2048), gj::kThreads, 0, (hipStream_t)stream, S);
  if (rc) return rc;
  return gj::launch(gj::k_group_finish, gj::grid_for(2 * (int64_t)n_groups), gj::kThreads, 0, (hipStream_t)stream,
                    n_groups, S.ws, out);
}

int gj_adjoint_group_stats(int64_t n, const int32_t* group, int32_t n_groups, const float* current_stage,
                           int32_t dead_stage, const float* g_cases, const float* g_deaths, float* grad_is_infected,
                           float* grad_stage, void* stream) {
  if (n < 0 || n_groups < 1 || n_groups > GJ_MAX_GROUPS) return GJ_E_RANGE;
  if (grad_stage && dead_stage == 0) return GJ_E_RANGE;      // (stage == dead) * stage / dead
  if (n == 0 || (!grad_is_infected && !grad_stage)) return GJ_OK;
  if (!group || (grad_stage && !current_stage)) return GJ_E_NULL;
  gj::GroupAdjArgs S;
  S.n = n;
  S.group = group;
  S.stage = current_stage;
  S.g_cases = g_cases;
  S.g_deaths = g_deaths;
  S.grad_inf = grad_is_infected;
  S.grad_stage = grad_stage;
  S.n_groups = n_groups;
  S.dead = dead_stage;
  S.vec4 = gj::aligned16(group, grad_is_infected, grad_stage, grad_stage ? current_stage : nullptr);   // (stage: read for grad_stage only)
  const int64_t blocks = gj::grid_for(gj::vec4_lanes(n, S.vec4), 2048);
  if (n_groups <= gj::kGroupAdjLdsMax)
    return gj::launch(gj::k_adjoint_group_stats<true>, blocks, gj::kThreads, (size_t)n_groups * 2 * sizeof(float),
                      (hipStream_t)stream, S);
  return gj::launch(gj::k_adjoint_group_stats<false>, blocks, gj::kThreads, 0, (hipStream_t)stream, S);
}

// the size checks gj_stage_stats and its adjoint share
static int check_stage_sizes(int64_t n, const int32_t* group, int32_t n_groups, int32_t n_stages) {
  if (n < 0 || n > GJ_STAGE_MAX_AGENTS || n_groups < 1 || n_groups > GJ_MAX_GROUPS) return GJ_E_RANGE;
  if (n_stages < 1 || n_stages > GJ_MAX_STAGES || (int64_t)n_groups * n_stages > INT32_MAX) return GJ_E_RANGE;
  if (!group && n_groups != 1) return GJ_E_RANGE;
  return GJ_OK;
}

int gj_stage_stats(int64_t n, const int32_t* group, int32_t n_groups, int32_t n_stages, const float* current_stage,
                   const float* prev_stage, int64_t* out, uint32_t* err, void* stream) {
  if (const int rc = check_stage_sizes(n, group, n_groups, n_stages)) return rc;
  if (!current_stage || !out || !err) return GJ_E_NULL;
  if (n == 0) return GJ_OK;
  gj::StageArgs S;
  S.n = n;
  S.group = group;
  S.stage = current_stage;
  S.prev = prev_stage;
  S.n_groups = n_groups;
  S.n_stages = n_stages;
  S.vec4 = gj::aligned16(group, current_stage, prev_stage);
  S.out = (unsigned long long*)out;
  S.err = err;
  const int64_t bins = (int64_t)n_groups * n_stages;
  const int64_t units = S.vec4 ? (n >> 2) + 1 : n;
  const size_t lds = (size_t)bins * 2 * sizeof(uint32_t);
  if (n_groups == 1) {      // regime (i); no lane takes more than kStageLaneLoads loads
    const int64_t lane_bound = gj::grid_for(units, 0, gj::kStageLdsThreads * gj::kStageLaneLoads);
    const int64_t blocks = std::max(gj::grid_for(units, gj::kStageLdsBlocks, gj::kStageLdsThreads), lane_bound);
    return gj::launch(gj::k_stage_stats<gj::kStageOne>, blocks, gj::kStageLdsThreads, lds, (hipStream_t)stream, S);
  }
  if (bins <= gj::kStageLdsBins)      // regime (ii)
    return gj::launch(gj::k_stage_stats<gj::kStageLds>, gj::grid_for(units, gj::kStageLdsBlocks, gj::kStageLdsThreads),
                      gj::kStageLdsThreads, lds, (hipStream_t)stream, S);
  return gj::launch(gj::k_stage_stats<gj::kStageGlobal>, gj::grid_for(units, gj::kStageGlobalBlocks), gj::kThreads, 0,
                    (hipStream_t)stream, S);      // regime (iii)
}

int gj_adjoint_stage_stats(int64_t n, const int32_t* group, int32_t n_groups, int32_t n_stages,
                           const float* current_stage, const float* prev_stage, const float* g_occupancy,
                           const float* g_entries, float* grad_stage, void* stream) {
  if (const int rc = check_stage_sizes(n, group, n_groups, n_stages)) return rc;
  if (!current_stage || !grad_stage) return GJ_E_NULL;
  if (n == 0) return GJ_OK;
  gj::StageAdjArgs S;
  S.n = n;
  S.group = group;
  S.stage = current_stage;
  S.prev = prev_stage;
  S.g_occ = g_occupancy;
  S.g_ent = g_entries;
  S.grad_stage = grad_stage;
  S.n_groups = n_groups;
  S.n_stages = n_stages;
  S.vec4 = gj::aligned16(group, current_stage, prev_stage, grad_stage);
  const int64_t bins = (int64_t)n_groups * n_stages;
  const int64_t blocks = gj::grid_for(gj::vec4_lanes(n, S.vec4), 2048);
  if (bins <= gj::kStageAdjLdsBins)
    return gj::launch(gj::k_adjoint_stage_stats<true>, blocks, gj::kThreads, (size_t)bins * 2 * sizeof(float),
                      (hipStream_t)stream, S);
  return gj::launch(gj::k_adjoint_stage_stats<false>, blocks, gj::kThreads, 0, (hipStream_t)stream, S);
}

int gj_location_stats(const gj_plan* plan, const gj_step_params* params, const gj_location_rows* rows,
                      const float* new_infected, const float* susceptibility0, const float* current_stage,
                      const int32_t* group, int32_t n_groups, const int32_t* cols, int32_t n_cols,
                      int32_t background_col, int64_t* out, uint32_t* err, void* stream) {
  int rc = gj::check_plan(plan);
  if (rc) return rc;
  gj::Groups G;
  rc = gj::group_networks(plan, params, &G);
  if (rc) return rc;
  if (!new_infected || !susceptibility0 || !out || !err) return GJ_E_NULL;
  if ((plan->n_sets > 0 && !rows) || (params->n_nets > 0 && !cols)) return GJ_E_NULL;
  if (params->has_quarantine && !current_stage) return GJ_E_NULL;
  if (n_groups < 1 || n_groups > GJ_MAX_GROUPS || (!group && n_groups != 1)) return GJ_E_RANGE;
  if (n_cols < 1 || n_cols > GJ_LOC_MAX_COLS || background_col < 0 || background_col >= n_cols) return GJ_E_RANGE;
  for (int i = 0; i < params->n_nets; ++i)
    if (cols[i] < 0 || cols[i] >= n_cols) return GJ_E_RANGE;
  gj::LocArgs A = {};
  for (int g = 0; g < G.n; ++g) {
    const gj_edge_set& E = plan->sets[G.set[g]];
    const gj_location_rows& R = rows[G.set[g]];
    if (R.a_rowptr && !R.a_venue && E.n_edges > 0) return GJ_E_NULL;
    const gj::NetGroup C = gj::classify_group(params, G, g);
    gj::LocSet& S = A.sets[g];
    S.rowptr = R.a_rowptr;
    S.venue = R.a_venue;
    S.cum = E.cum;
    S.n_edges = (int32_t)E.n_edges;
    S.n_venues = (int32_t)E.n_venues;
    S.stride = E.cum_stride;
    S.nk = C.nk;
    S.first = G.first[g];
    memcpy(S.mask, C.mask, sizeof(S.mask));
    memcpy(S.table, C.table, sizeof(S.table));
  }
  if (plan->n_agents == 0) return GJ_OK;
  A.n = plan->n_agents;
  A.nu = new_infected;
  A.s0 = susceptibility0;
  A.stage = params->has_quarantine ? current_stage : nullptr;
  A.group = group;
  A.cls = plan->agent_class;
  A.tables = plan->tables;
  A.out = (unsigned long long*)out;
  A.err = err;
  A.n_groups = n_groups;
  A.n_cols = n_cols;
  A.n_nets = params->n_nets;
  A.background = background_col;
  A.n_sets = G.n;
  A.has_q = params->has_quarantine ? 1 : 0;
  A.day_type = params->day_type;
  A.q_thr = params->q_threshold;
  for (int i = 0; i < params->n_nets; ++i) A.cols[i] = cols[i];
  const int64_t blocks = gj::grid_for(A.n, gj::kLocBlocks, gj::kLocLoads * gj::kWave);
  const int64_t bins = (int64_t)n_groups * n_cols;
  if (bins <= gj::kLocLdsBins)
    return gj::launch(gj::k_location_stats<true>, blocks, gj::kThreads, (size_t)bins * sizeof(unsigned long long),
                      (hipStream_t)stream, A);
  return gj::launch(gj::k_location_stats<false>, blocks, gj::kThreads, 0, (hipStream_t)stream, A);
}

// the sets of the step's networks as the infector kernels take them: the location kernel's, with p_contact, U and beta;
// and UG where the caller takes it (the infection-matrix launches: the scatter takes UG alone, the gather both)
enum { kInfU = 1, kInfUG = 2 };
static int infector_sets(const gj_plan* plan, const gj_step_params* params, const gj_location_rows* rows,
                         int64_t* const* U, gj::InfArgs* A, int64_t* const* UG = nullptr, int takes = kInfU) {
  int rc = gj::check_plan(plan);
  if (rc) return rc;
  gj::Groups G;
  rc = gj::group_networks(plan, params, &G);
  if (rc) return rc;
  if (plan->n_sets > 0 && !rows) return GJ_E_NULL;
  if (params->n_nets > 0 && (((takes & kInfU) && !U) || ((takes & kInfUG) && !UG))) return GJ_E_NULL;
  for (int g = 0; g < G.n; ++g) {
    const gj_edge_set& E = plan->sets[G.set[g]];
    const gj_location_rows& R = rows[G.set[g]];
    if (R.a_rowptr && !R.a_venue && E.n_edges > 0) return GJ_E_NULL;
    if ((takes & kInfU) && R.a_rowptr && E.n_venues > 0 && !U[G.set[g]]) return GJ_E_NULL;
    if ((takes & kInfUG) && R.a_rowptr && E.n_venues > 0 && !UG[G.set[g]]) return GJ_E_NULL;
    const gj::NetGroup C = gj::classify_group(params, G, g);
    gj::InfSet& S = A->sets[g];
    S.rowptr = R.a_rowptr;
    S.venue = R.a_venue;
    S.cum = E.cum;
    S.n_edges = (int32_t)E.n_edges;
    S.n_venues = (int32_t)E.n_venues;
    S.stride = E.cum_stride;
    S.nk = C.nk;
    S.first = G.first[g];
    memcpy(S.mask, C.mask, sizeof(S.mask));
    memcpy(S.table, C.table, sizeof(S.table));
    memcpy(S.beta, C.beta, sizeof(S.beta));
    S.pc = E.v_pcontact;
    S.U = (takes & kInfU) ? (unsigned long long*)U[G.set[g]] : nullptr;
    S.UG = (takes & kInfUG) ? (unsigned long long*)UG[G.set[g]] : nullptr;
  }
  A->n = plan->n_agents;
  A->cls = plan->agent_class;
  A->tables = plan->tables;
  A->n_nets = params->n_nets;
  A->n_sets = G.n;
  A->has_q = params->has_quarantine ? 1 : 0;
  A->day_type = params->day_type;
  A->q_thr = params->q_threshold;
  return GJ_OK;
}

int gj_infector_scatter(const gj_plan* plan, const gj_step_params* params, const gj_location_rows* rows,
                        const float* new_infected, const float* susceptibility0, const float* current_stage,
                        int64_t* const* U, int64_t* unattributed, int32_t* cohort, int32_t cohort_value, uint32_t* err,
                        void* stream) {
  gj::InfArgs A = {};
  if (const int rc = infector_sets(plan, params, rows, U, &A)) return rc;
  if (!new_infected || !susceptibility0 || !unattributed || !err) return GJ_E_NULL;
  if (params->has_quarantine && !current_stage) return GJ_E_NULL;
  if (plan->n_agents == 0) return GJ_OK;
  A.flag = new_infected;
  A.s0 = susceptibility0;
  A.stage = params->has_quarantine ? current_stage : nullptr;
  A.unattributed = (unsigned long long*)unattributed;
  A.cohort = cohort;
  A.cohort_value = cohort_value;
  A.err = err;
  return gj::launch(gj::k_infector_scatter<false>, gj::grid_for(A.n, gj::kLocBlocks, gj::kLocLoads * gj::kWave),
                    gj::kThreads, 0, (hipStream_t)stream, A);
}

int gj_infector_gather(const gj_plan* plan, const gj_step_params* params, const gj_location_rows* rows,
                       const float* transmission, const float* current_stage, int64_t* const* U, const int32_t* group,
                       int32_t n_groups, double* caused, int64_t* out, uint32_t* err, void* stream) {
  gj::InfArgs A = {};
  if (const int rc = infector_sets(plan, params, rows, U, &A)) return rc;
  if (!transmission || !err || (!caused && !out)) return GJ_E_NULL;
  if (params->has_quarantine && !current_stage) return GJ_E_NULL;
  if (n_groups < 1 || n_groups > GJ_MAX_GROUPS || (!group && n_groups != 1)) return GJ_E_RANGE;
  if (plan->n_agents == 0 || params->n_nets == 0) return GJ_OK;
  A.flag = transmission;
  A.stage = params->has_quarantine ? current_stage : nullptr;
  A.group = group;
  A.n_groups = n_groups;
  A.caused = caused;
  A.out = (unsigned long long*)out;
  A.err = err;
  const int64_t blocks = gj::grid_for(A.n, gj::kLocBlocks, gj::kLocLoads * gj::kWave);
  if (out && n_groups <= gj::kLocLdsBins)
    return gj::launch(gj::k_infector_gather<true>, blocks, gj::kThreads, (size_t)n_groups * sizeof(unsigned long long),
                      (hipStream_t)stream, A);
  return gj::launch(gj::k_infector_gather<false>, blocks, gj::kThreads, 0, (hipStream_t)stream, A);
}

// gj_infector_clear (n_groups == 0: U) and gj_infection_matrix_clear (UG, n_groups cells per column)
static int infector_clear(const gj_plan* plan, const gj_location_rows* rows, const float* new_infected, int64_t* const* U,
                          int32_t n_groups, void* stream) {
  const int rc = gj::check_plan(plan);
  if (rc) return rc;
  if (!new_infected || (plan->n_sets > 0 && (!rows || !U))) return GJ_E_NULL;
  gj::InfArgs A = {};
  A.n_groups = n_groups;
  for (int s = 0; s < plan->n_sets; ++s) {
    const gj_edge_set& E = plan->sets[s];
    if (!rows[s].a_rowptr || !U[s] || E.n_venues == 0) continue;      // no rows or no U: nothing of this set to clear
    if (!rows[s].a_venue && E.n_edges > 0) return GJ_E_NULL;
    gj::InfSet& S = A.sets[A.n_sets++];
    S.rowptr = rows[s].a_rowptr;
    S.venue = rows[s].a_venue;
    S.n_edges = (int32_t)E.n_edges;
    S.n_venues = (int32_t)E.n_venues;
    S.stride = E.cum_stride;
    (n_groups ? S.UG : S.U) = (unsigned long long*)U[s];
  }
  if (plan->n_agents == 0 || A.n_sets == 0) return GJ_OK;
  A.n = plan->n_agents;
  A.flag = new_infected;
  const int64_t blocks = gj::grid_for(A.n, gj::kLocBlocks, gj::kLocLoads * gj::kWave);
  if (n_groups) return gj::launch(gj::k_infector_clear<true>, blocks, gj::kThreads, 0, (hipStream_t)stream, A);
  return gj::launch(gj::k_infector_clear<false>, blocks, gj::kThreads, 0, (hipStream_t)stream, A);
}

int gj_infector_clear(const gj_plan* plan, const gj_location_rows* rows, const float* new_infected, int64_t* const* U,
                      void* stream) {
  return infector_clear(plan, rows, new_infected, U, 0, stream);
}

static int matrix_groups(const int32_t* group, int32_t n_groups) {
  return (n_groups < 1 || n_groups > GJ_MATRIX_MAX_GROUPS || (!group && n_groups != 1)) ? GJ_E_RANGE : GJ_OK;
}

int gj_infection_matrix_scatter(const gj_plan* plan, const gj_step_params* params, const gj_location_rows* rows,
                                const float* new_infected, const float* susceptibility0, const float* current_stage,
                                const int32_t* group, int32_t n_groups, int64_t* const* UG,
                                int64_t* unattributed_by_group, uint32_t* err, void* stream) {
  gj::InfArgs A = {};
  if (const int rc = infector_sets(plan, params, rows, nullptr, &A, UG, kInfUG)) return rc;
  if (!new_infected || !susceptibility0 || !err) return GJ_E_NULL;
  if (params->has_quarantine && !current_stage) return GJ_E_NULL;
  if (const int rc = matrix_groups(group, n_groups)) return rc;
  if (plan->n_agents == 0) return GJ_OK;
  A.flag = new_infected;
  A.s0 = susceptibility0;
  A.stage = params->has_quarantine ? current_stage : nullptr;
  A.group = group;
  A.n_groups = n_groups;
  A.unattributed = (unsigned long long*)unattributed_by_group;
  A.err = err;
  return gj::launch(gj::k_infector_scatter<true>, gj::grid_for(A.n, gj::kLocBlocks, gj::kLocLoads * gj::kWave),
                    gj::kThreads, 0, (hipStream_t)stream, A);
}

int gj_infection_matrix_gather(const gj_plan* plan, const gj_step_params* params, const gj_location_rows* rows,
                               const float* transmission, const float* current_stage, int64_t* const* U,
                               int64_t* const* UG, const int32_t* group, int32_t n_groups, int64_t* out, uint32_t* err,
                               void* stream) {
  static_assert(GJ_MATRIX_MAX_GROUPS * GJ_MATRIX_MAX_GROUPS <= GJ_LOC_LDS_BINS, "the matrix fits the LDS histogram");
  gj::InfArgs A = {};
  if (const int rc = infector_sets(plan, params, rows, U, &A, UG, kInfU | kInfUG)) return rc;
  if (!transmission || !out || !err) return GJ_E_NULL;
  if (params->has_quarantine && !current_stage) return GJ_E_NULL;
  if (const int rc = matrix_groups(group, n_groups)) return rc;
  if (plan->n_agents == 0 || params->n_nets == 0) return GJ_OK;
  A.flag = transmission;
  A.stage = params->has_quarantine ? current_stage : nullptr;
  A.group = group;
  A.n_groups = n_groups;
  A.out = (unsigned long long*)out;
  A.err = err;
  return gj::launch(gj::k_infector_gather<true, true>, gj::grid_for(A.n, gj::kLocBlocks, gj::kLocLoads * gj::kWave),
                    gj::kThreads, (size_t)n_groups * n_groups * sizeof(unsigned long long), (hipStream_t)stream, A);
}

int gj_infection_matrix_clear(const gj_plan* plan, const gj_location_rows* rows, const float* new_infected,
                              int64_t* const* UG, int32_t n_groups, void* stream) {
  if (n_groups < 1 || n_groups > GJ_MATRIX_MAX_GROUPS) return plan ? GJ_E_RANGE : GJ_E_NULL;
  return infector_clear(plan, rows, new_infected, UG, n_groups, stream);
}

int gj_infection_tree(const gj_plan* plan, const gj_step_params* params, const gj_location_rows* rows,
                      const gj_venue_rows* venue_rows, const float* new_infected, const float* susceptibility0,
                      const float* current_stage, const float* transmission, const int32_t* cols, int32_t n_cols,
                      int32_t background_col, uint64_t seed, uint64_t step, int64_t agent_offset, int32_t* infector,
                      int32_t* via, int32_t* venue, int32_t* row_of, int32_t row_value, int64_t* counts,
                      int64_t* unresolved, uint32_t* err, void* stream) {
  int rc = gj::check_plan(plan);
  if (rc) return rc;
  gj::Groups G;
  rc = gj::group_networks(plan, params, &G);
  if (rc) return rc;
  if (!new_infected || !susceptibility0 || !infector || !via || !venue || !row_of || !counts || !unresolved || !err)
    return GJ_E_NULL;
  if ((plan->n_sets > 0 && !rows) || (params->n_nets > 0 && (!cols || !transmission || !venue_rows))) return GJ_E_NULL;
  if (params->has_quarantine && !current_stage) return GJ_E_NULL;
  if (n_cols < 1 || n_cols > GJ_LOC_MAX_COLS || background_col < 0 || background_col >= n_cols) return GJ_E_RANGE;
  for (int i = 0; i < params->n_nets; ++i)
    if (cols[i] < 0 || cols[i] >= n_cols) return GJ_E_RANGE;
  if (agent_offset < 0 || agent_offset > (int64_t)INT32_MAX - plan->n_agents) return GJ_E_RANGE;
  static_assert(sizeof(gj::TreeArgs) <= 4096, "kernel arguments");
  gj::TreeArgs A = {};
  // the sets in the order of plan->sets - the canonical order of the pairs - whatever the order of the networks
  int order[GJ_MAX_SETS];
  for (int g = 0; g < G.n; ++g) order[g] = g;
  std::sort(order, order + G.n, [&](int x, int y) { return G.set[x] < G.set[y]; });
  for (int j = 0; j < G.n; ++j) {
    const int g = order[j];
    const gj_edge_set& E = plan->sets[G.set[g]];
    const gj_location_rows& R = rows[G.set[g]];
    const gj_venue_rows& V = venue_rows[G.set[g]];
    if (R.a_rowptr && !R.a_venue && E.n_edges > 0) return GJ_E_NULL;
    if (V.v_rowptr && !V.v_agent && E.n_edges > 0) return GJ_E_NULL;
    const gj::NetGroup C = gj::classify_group(params, G, g);
    gj::TreeSet& S = A.sets[j];
    S.rowptr = R.a_rowptr;
    S.venue = R.a_venue;
    S.cum = E.cum;
    S.n_edges = (int32_t)E.n_edges;
    S.n_venues = (int32_t)E.n_venues;
    S.stride = E.cum_stride;
    S.nk = C.nk;
    S.first = G.first[g];
    memcpy(S.mask, C.mask, sizeof(S.mask));
    memcpy(S.table, C.table, sizeof(S.table));
    S.v_rowptr = V.v_rowptr;
    S.v_agent = V.v_agent;
  }
  if (plan->n_agents == 0) return GJ_OK;
  A.n = plan->n_agents;
  A.flag = new_infected;
  A.s0 = susceptibility0;
  A.stage = params->has_quarantine ? current_stage : nullptr;
  A.tr = transmission;
  A.cls = plan->agent_class;
  A.tables = plan->tables;
  A.infector = infector;
  A.via = via;
  A.venue = venue;
  A.row_of = row_of;
  A.counts = (unsigned long long*)counts;
  A.unresolved = (unsigned long long*)unresolved;
  A.err = err;
  A.seed = seed;
  A.step = step;
  A.agent_offset = agent_offset;
  A.n_cols = n_cols;
  A.n_nets = params->n_nets;
  A.n_sets = G.n;
  A.has_q = params->has_quarantine ? 1 : 0;
  A.day_type = params->day_type;
  A.background = background_col;
  A.row_value = row_value;
  A.q_thr = params->q_threshold;
  for (int i = 0; i < params->n_nets; ++i) A.cols[i] = cols[i];
  return gj::launch(gj::k_infection_tree, gj::grid_for(A.n, gj::kLocBlocks, gj::kLocLoads * gj::kWave), gj::kThreads, 0,
                    (hipStream_t)stream, A);
}

int gj_step(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params, const gj_step_io* io,
            void* stream) {
  return gj_step_aux(plan, state, params, io, nullptr, stream);
}

int gj_step_aux(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params, const gj_step_io* io,
                const gj_aux* aux, void* stream) {
  int rc = gj::check_plan(plan);
  if (rc) return rc;
  gj::Groups G;
  rc = gj::group_networks(plan, params, &G);
  if (rc) return rc;
  rc = gj::check_state(plan, state, params);
  if (rc) return rc;
  rc = gj::do_transmission(plan, state, params, (hipStream_t)stream);
  if (rc) return rc;
  if (plan->tiled) {
    rc = gj::tiled_scatter(plan, state, params, G, (hipStream_t)stream);
    if (rc) return rc;
    rc = gj::tiled_venues(plan, state, params, G, 0, (hipStream_t)stream, aux);
    if (rc) return rc;
    return gj::tiled_agents(plan, state, params, G, io, 1, (hipStream_t)stream);
  }
  rc = gj::do_venue_reduce(plan, state, params, G, (hipStream_t)stream);
  if (rc) return rc;
  return gj::do_agent_gather(plan, state, params, G, io, 1, (hipStream_t)stream);
}

int gj_step_phase(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params,
                  const gj_step_io* io, int phase, void* stream) {
  return gj_step_phase_aux(plan, state, params, io, nullptr, phase, stream);
}

int gj_step_phase_aux(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params,
                      const gj_step_io* io, const gj_aux* aux, int phase, void* stream) {
  int rc = gj::check_plan(plan);
  if (rc) return rc;
  gj::Groups G;
  rc = gj::group_networks(plan, params, &G);
  if (rc) return rc;
  rc = gj::check_state(plan, state, params, /*full=*/phase == 0 || phase == 3);   // only a1 / a9 touch the infection state
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  switch (phase) {
    case 0: return gj::do_transmission(plan, state, params, st);
    case 1: return plan->tiled ? gj::tiled_scatter(plan, state, params, G, st)
                               : gj::do_venue_reduce(plan, state, params, G, st);
    case 2: return plan->tiled ? gj::tiled_venues(plan, state, params, G, 0, st, aux) : GJ_OK;
    case 3: return plan->tiled ? gj::tiled_agents(plan, state, params, G, io, 1, st)
                               : gj::do_agent_gather(plan, state, params, G, io, 1, st);
    case 4: return plan->tiled ? gj::tiled_agents(plan, state, params, G, io, 0, st)
                               : gj::do_agent_gather(plan, state, params, G, io, 0, st);
    case 5: return plan->tiled ? gj::tiled_venues(plan, state, params, G, 1, st, aux) : GJ_OK;
    case 6: return plan->tiled ? gj::tiled_venues(plan, state, params, G, 2, st, aux) : GJ_OK;
    case 7:   // 1 then 5 (A + B) in one call: the launch path of a partial-sum group
    case 8:   // 1 then 2 (A + B + C)
      if (!plan->tiled) return gj::do_venue_reduce(plan, state, params, G, st);
      rc = gj::tiled_scatter(plan, state, params, G, st);
      if (rc) return rc;
      return gj::tiled_venues(plan, state, params, G, phase == 7 ? 1 : 0, st, aux);
    default: return GJ_E_RANGE;
  }
}

namespace gj {
__global__ void k_clock_advance(gj_clock* clock, double delta_now) {
  const uint64_t step = clock->step + 1;
  clock->step = step;
  clock->now = (float)(clock->now0 + (double)(int64_t)(step - clock->step0) * delta_now);
}
}  // namespace gj

int gj_clock_advance(gj_clock* clock, double delta_now, void* stream) {
  if (!clock) return GJ_E_NULL;
  return gj::launch(gj::k_clock_advance, 1, 1, 0, (hipStream_t)stream, clock, delta_now);
}

int gj_pack_f32(int64_t n, const int32_t* index, const float* src, float* out, void* stream) {
  if (n < 0) return GJ_E_RANGE;
  if (n == 0) return GJ_OK;
  if (!index || !src || !out) return GJ_E_NULL;
  return gj::launch(gj::k_pack, gj::grid_for(n), gj::kThreads, 0, (hipStream_t)stream, n, index, src, out);
}

int gj_unpack_f32(int64_t n, const int32_t* index, const float* in, float* dst, void* stream) {
  if (n < 0) return GJ_E_RANGE;
  if (n == 0) return GJ_OK;
  if (!index || !in || !dst) return GJ_E_NULL;
  return gj::launch(gj::k_unpack, gj::grid_for(n), gj::kThreads, 0, (hipStream_t)stream, n, index, in, dst);
}

int gj_event_create(void** event) {
  if (!event) return GJ_E_NULL;
  hipEvent_t e;
  const hipError_t rc = hipEventCreate(&e);
  if (rc != hipSuccess) return (int)rc;
  *event = (void*)e;
  return GJ_OK;
}
int gj_event_record(void* event, void* stream) {
  if (!event) return GJ_E_NULL;
  return (int)hipEventRecord((hipEvent_t)event, (hipStream_t)stream);
}
int gj_event_elapsed_ms(void* start, void* stop, float* ms) {
  if (!start || !stop || !ms) return GJ_E_NULL;
  hipError_t rc = hipEventSynchronize((hipEvent_t)stop);
  if (rc != hipSuccess) return (int)rc;
  return (int)hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
}
int gj_event_destroy(void* event) {
  if (!event) return GJ_E_NULL;
  return (int)hipEventDestroy((hipEvent_t)event);
}

}  // extern "C"
