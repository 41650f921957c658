// The per-agent kernels beside the infection path, and their argument blocks: the symptoms update (f1), the per-step
// statistics by age bin and by agent group (f2), and the elementwise and seed adjoints (f3).  One lane per agent (or
// per four), no edge structure.  Included by gradjune_hip.hip, which holds their launches (C ABI: include/gradjune_hip.h).
#pragma once
#include "../../include/gradjune_hip.h"
#include "gj_device.h"
#include "gj_tiled.h"   // fx_t, to_fx, fx_max: the group statistics' fixed point

namespace gj {

// f1: disease-stage progression (reference grad_june/symptoms.py:204-247, 82-128), one lane per agent
struct SymptomsArgs {
  gj_symptoms_params P;
  int64_t n;
  const uint8_t* cls;
  const float* new_inf;
  float* cur;
  float* nxt;
  float* ttn;
  const float* progresses;
  const float* dwell;
};

__device__ __forceinline__ float dwell_sample(int kind, float loc, float scale, float z) {
  const float v = loc + scale * z;
  return kind == 1 ? __builtin_amdgcn_exp2f(v * 1.44269504088896341f) : v;      // LogNormal: exp on v_exp_f32
}
// The library's own draw for an agent at stage s that is due (no reference stream to reproduce: symptoms.py:82-128 draws
// torch.bernoulli + rsample): progress with the table's probability, dwell time = LogNormal / Normal of one Box-Muller
// normal.  On the hardware's transcendental units (v_log_f32, v_sqrt_f32, v_cos_f32 - whose argument is in revolutions -
// v_exp_f32): the draws of a wave's due agents were half of the fused symptoms launch with libm's logf / cosf / expf.
// ONE definition, shared by the update and its adjoint (which must replay the same draw).
__device__ __forceinline__ void stage_draw(const gj_symptoms_params& P, int64_t a, int s, int age, bool& onward, float& d) {
  uint32_t r[4];
  philox4x32_10((uint64_t)(P.agent_offset + a), P.step | (1ull << 63), P.seed, r);
  onward = u01(r[0]) < P.progress[s * 100 + age];
  const float ln_u = __builtin_amdgcn_logf(u01(r[1])) * 0.693147180559945309f;        // ln(u) = log2(u) * ln(2)
  const float z = __builtin_amdgcn_sqrtf(-2.0f * ln_u) * __builtin_amdgcn_cosf(u01(r[2]));   // cos(2 pi u)
  d = onward ? dwell_sample(P.next_kind[s], P.next_loc[s], P.next_scale[s], z)
             : dwell_sample(P.rec_kind[s], P.rec_loc[s], P.rec_scale[s], z);
}

// The update up to the draw, shared by the update and its adjoint (which recomputes the branch the agent took from the
// PRE-step state): the values after a new infection (x1, t1: next stage = exposed, due now) and after the move to the
// next stage (c1), the stage s the agent is then in and whether it is due a draw there.
struct SymptomsMove {
  float x1, t1, c1;
  bool moving, due;
  int s;
};
__device__ __forceinline__ SymptomsMove symptoms_move(const gj_symptoms_params& P, float nw, float c0, float x0,
                                                      float t0) {
  SymptomsMove M;
  M.x1 = x0 + nw * (2.0f - x0);
  M.t1 = t0 + nw * (P.time - t0);
  M.moving = (P.time >= M.t1) && (c0 < (float)(P.n_stages - 1));
  M.c1 = c0 - (c0 - M.x1) * (M.moving ? 1.0f : 0.0f);
  M.s = min(max((int)M.c1, 0), P.n_stages - 1);
  M.due = M.moving && M.s >= 2 && M.s <= P.n_stages - 2 && M.c1 == (float)M.s;
  return M;
}
// a due agent's outcome: the injected one, or the library's own draw
__device__ __forceinline__ void stage_outcome(const gj_symptoms_params& P, const float* progresses, const float* dwell,
                                              int64_t a, int s, int age, bool& onward, float& d) {
  if (progresses) {
    onward = progresses[a] != 0.0f;
    d = dwell[a];
  } else {
    stage_draw(P, a, s, age, onward, d);
  }
}

// One agent's stage update (symptoms.py:204-247, 82-128).  Returns true when any of the three values changed.
__device__ __forceinline__ bool symptoms_agent(const SymptomsArgs& S, int64_t a, float nw, int cls, float& cur,
                                               float& nx, float& tt) {
  const float cur0 = cur, nx0 = nx, tt0 = tt;
  const SymptomsMove M = symptoms_move(S.P, nw, cur, nx, tt);
  cur = M.c1;
  nx = M.x1;
  tt = M.t1;
  if (M.due) {
    bool onward;
    float d;
    stage_outcome(S.P, S.progresses, S.dwell, a, M.s, cls % 100, onward, d);
    if (onward) {
      nx = nx + 1.0f;
    } else {
      nx = nx - nx;
    }
    tt = tt + d;
  }
  // (bit comparison: a NaN that stays a NaN has not changed)
  return __float_as_uint(cur) != __float_as_uint(cur0) || __float_as_uint(nx) != __float_as_uint(nx0) ||
         __float_as_uint(tt) != __float_as_uint(tt0);
}

__global__ __launch_bounds__(kThreads) void k_symptoms(const SymptomsArgs S) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= S.n) return;
  float cur = S.cur[a], nx = S.nxt[a], tt = S.ttn[a];
  symptoms_agent(S, a, S.new_inf[a], (int)S.cls[a], cur, nx, tt);
  S.cur[a] = cur;
  S.nxt[a] = nx;
  S.ttn[a] = tt;
}

// f3: adjoint of k_symptoms w.r.t. the stage values and new_infected (oracle/gj_oracle.py:adjoint_symptoms).
// Recomputes the branch the agent took from the PRE-step state and the same randomness.
struct SymptomsAdjointArgs {
  gj_symptoms_params P;
  int64_t n;
  const uint8_t* cls;
  const float* new_inf;
  const float* cur0;
  const float* nxt0;
  const float* ttn0;
  const float* progresses;
  const float* dwell;
  const float* g_cur;
  const float* g_nxt;
  const float* g_ttn;
  float* g_cur_in;
  float* g_nxt_in;
  float* g_ttn_in;
  float* g_new;
};

__global__ __launch_bounds__(kThreads) void k_adjoint_symptoms(const SymptomsAdjointArgs S) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= S.n) return;
  const float time = S.P.time;
  const float nw = S.new_inf[a];
  const float x0 = S.nxt0[a], t0 = S.ttn0[a];
  const SymptomsMove M = symptoms_move(S.P, nw, S.cur0[a], x0, t0);
  const float m = M.moving ? 1.0f : 0.0f;
  float gc1 = S.g_cur ? S.g_cur[a] : 0.0f;
  float gx1 = S.g_nxt ? S.g_nxt[a] : 0.0f;
  const float gt1 = S.g_ttn ? S.g_ttn[a] : 0.0f;
  if (M.due) {
    const int s = M.s;
    bool onward;
    float d;
    stage_outcome(S.P, S.progresses, S.dwell, a, s, (int)(S.cls[a] % 100), onward, d);
    gc1 += gt1 * d / (float)s;              // time += dwell * (current == s) * current / s  (either branch)
    if (onward) {
      gc1 += gx1 / (float)s;                // next += (current == s) * current / s
    } else {
      gc1 -= gx1 * M.x1 / (float)s;         // next -= next * (current == s) * current / s
      gx1 = 0.0f;
    }
  }
  gx1 += gc1 * m;                           // current -= (current - next) * moving
  S.g_cur_in[a] = gc1 * (1.0f - m);
  S.g_nxt_in[a] = gx1 * (1.0f - nw);        // next += new_infected * (2 - next)
  if (S.g_ttn_in) S.g_ttn_in[a] = gt1 * (1.0f - nw);   // time += new_infected * (now - time)
  S.g_new[a] = gx1 * (2.0f - x0) + gt1 * (time - t0);
}

// f3: elementwise adjoints (see include/gradjune_hip.h)
__global__ __launch_bounds__(kThreads) void k_adjoint_sample(
    int64_t n, const float* __restrict__ susc0, const float* __restrict__ time0, const float* __restrict__ acc,
    const float* __restrict__ noise, uint64_t seed, uint64_t step, int64_t agent_offset, float now, float dt,
    const float* __restrict__ g_susc, const float* __restrict__ g_inf, const float* __restrict__ g_time,
    const float* __restrict__ g_new, float* __restrict__ x_out, float* __restrict__ grad_susc,
    float* __restrict__ grad_time) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;
  const float s0 = susc0[a];
  const float ac = acc[a];
  const float ts = s0 * ac;
  const bool inside = (ts >= 1e-6f) && (ts <= 100.0f);
  const float p = not_infected_prob(ts, dt);
  const float gs = g_susc ? g_susc[a] : 0.0f, gi = g_inf ? g_inf[a] : 0.0f, gt = g_time ? g_time[a] : 0.0f;
  const float gn = g_new ? g_new[a] : 0.0f;
  float e0, e1;
  sampler_draws(noise, n, a, seed, step, agent_offset, e0, e1);
  float y0, y1;
  sampler_softmax<float>(p, e0, e1, y0, y1);
  const float nu = sampler_decision(p, noise != nullptr, y0, y1, seed, step, agent_offset + a);
  const SampleAdjoint<float> r = sample_adjoint<float>(p, s0, time0[a], y0, y1, nu, now, gs, gi, gt, gn);
  const float ts_bar = inside ? r.nu_bar * r.dnu_dp * (-dt * p) : 0.0f;
  x_out[a] = s0 * ts_bar;
  grad_susc[a] = gs * r.h + ts_bar * ac;
  grad_time[a] = gt * (1.0f - nu);
}

// f3, the seed: adjoint of sampling with one probability per agent group followed by infect_people (include/gradjune_hip.h,
// gj_adjoint_seed).  Three launches.  (1) one lane per agent: the per-agent term c_a = -nu_bar * d nu / d p of
// d loss / d fraction[group[a]] (in fp64 from the fp32 inputs, into a workspace) and the elementwise outputs.
struct SeedAdjArgs {
  int64_t n;
  const float* p_not;       // [n_groups]
  const int32_t* group;     // [n] or NULL (every agent in group 0)
  int32_t n_groups;
  const float* susc0;
  const float* time0;
  const float* noise;
  uint64_t seed, step;
  int64_t agent_offset;
  float now;
  const float* g_susc;
  const float* g_inf;
  const float* g_time;
  const float* g_new;
  double* contrib;          // [n]
  float* grad_susc;         // [n] or NULL
  float* grad_time;         // [n] or NULL
};

__global__ __launch_bounds__(kThreads) void k_adjoint_seed_agents(const SeedAdjArgs S) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= S.n) return;
  const int32_t g = S.group ? S.group[a] : 0;
  const float s0 = S.susc0[a];
  const float gs = S.g_susc ? S.g_susc[a] : 0.0f, gt = S.g_time ? S.g_time[a] : 0.0f;
  if ((uint32_t)g >= (uint32_t)S.n_groups) {   // no group: not seeded (nu = 0), no term; the label is not an index
    S.contrib[a] = 0.0;
    if (S.grad_susc) S.grad_susc[a] = gs * ((s0 > 0.0f) ? 1.0f : ((s0 == 0.0f) ? 0.5f : 0.0f));
    if (S.grad_time) S.grad_time[a] = gt;
    return;
  }
  const float gi = S.g_inf ? S.g_inf[a] : 0.0f, gn = S.g_new ? S.g_new[a] : 0.0f;
  const float p = S.p_not[g];
  double e0, e1;                                                // (injected draws: the fp32 values; the library's own:
  sampler_draws(S.noise, S.n, a, S.seed, S.step, S.agent_offset, e0, e1);   //  exp_pair's products taken in fp64)
  float y0f = 0.0f, y1f = 0.0f;                                 // the decision is the forward's: taken in its arithmetic
  if (S.noise) sampler_softmax<float>(p, (float)e0, (float)e1, y0f, y1f);
  const float nu = sampler_decision(p, S.noise != nullptr, y0f, y1f, S.seed, S.step, S.agent_offset + a);
  double y0, y1;
  sampler_softmax<double>(p, e0, e1, y0, y1);
  const SampleAdjoint<double> r = sample_adjoint<double>(p, s0, S.time0[a], y0, y1, nu, S.now, gs, gi, gt, gn);
  S.contrib[a] = -(r.nu_bar * r.dnu_dp);       // d fraction = -d p
  if (S.grad_susc) S.grad_susc[a] = gs * (float)r.h;
  if (S.grad_time) S.grad_time[a] = gt * (1.0f - nu);
}

// (2) one WAVE per (group, chunk): the chunk's <= GJ_SEED_CHUNK terms, read through the label-sorted agent list, are
// added in fp64 - every lane its terms in list order, then the lanes by a butterfly - and written as partial[chunk].
// (3) one wave per group adds its chunks' partials the same way.  No atomics: the order of every sum is a function of
// the labels alone, so two launches give the same bits.  Every index read from the tables is checked before use.
struct SeedSumArgs {
  int64_t n, n_sorted, n_chunks;
  int32_t n_groups;
  const double* contrib;
  const int64_t* order;        // [n_sorted] or NULL (identity)
  const int64_t* seg_offsets;  // [n_groups + 1] or NULL ({0, n})
  const int64_t* chunk_first;  // [n_groups + 1] or NULL ({0, n_chunks})
  const int32_t* chunk_group;  // [n_chunks] or NULL (0)
  double* partial;             // [n_chunks]
  double* out;                 // [n_groups]
};

__global__ __launch_bounds__(kThreads) void k_adjoint_seed_chunks(const SeedSumArgs S) {
  const int64_t c = (int64_t)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (c >= S.n_chunks) return;                 // (whole waves leave: the shuffles below see full waves)
  const int32_t g = S.chunk_group ? S.chunk_group[c] : 0;
  double acc = 0.0;
  if ((uint32_t)g < (uint32_t)S.n_groups) {
    const int64_t k = c - (S.chunk_first ? S.chunk_first[g] : 0);
    const int64_t s0 = S.seg_offsets ? S.seg_offsets[g] : 0, s1 = S.seg_offsets ? S.seg_offsets[g + 1] : S.n;
    if (k >= 0 && s0 >= 0 && k <= (S.n_sorted - s0) / GJ_SEED_CHUNK) {
      const int64_t begin = s0 + k * GJ_SEED_CHUNK;
      int64_t end = begin + GJ_SEED_CHUNK;
      if (end > s1) end = s1;
      if (end > S.n_sorted) end = S.n_sorted;
      for (int64_t j = begin + lane; j < end; j += kWave) {
        const int64_t a = S.order ? S.order[j] : j;
        if ((uint64_t)a < (uint64_t)S.n) acc += S.contrib[a];
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) S.partial[c] = acc;
}

__global__ __launch_bounds__(kThreads) void k_adjoint_seed_finish(const SeedSumArgs S) {
  const int64_t g = (int64_t)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (g >= S.n_groups) return;
  int64_t c0 = S.chunk_first ? S.chunk_first[g] : 0, c1 = S.chunk_first ? S.chunk_first[g + 1] : S.n_chunks;
  if (c0 < 0) c0 = 0;
  if (c1 > S.n_chunks) c1 = S.n_chunks;
  double acc = 0.0;
  for (int64_t c = c0 + lane; c < c1; c += kWave) acc += S.partial[c];
  acc = wave_sum(acc);
  if (lane == 0) S.out[g] = acc;
}

// Vaccination (include/gradjune_hip.h, gj_vaccinate / gj_adjoint_vaccinate): streaming, per agent.  A campaign's uniform
// of an agent is infection_uniform(seed, stream, global id) - word (id & 3) of the block (id >> 2, stream) - so a lane
// that holds the four agents of an aligned quad of global ids computes ONE block (vaccine_uniforms4); a lane that holds
// one agent calls infection_uniform itself.  The per-age tables arrive by value and are staged in LDS, where a lane's
// age indexes them (300 floats; from the kernel arguments a per-lane index would go through scratch).
// ONE definition of the rule, shared by the update and its adjoint (which must take the update's decision).
__device__ __forceinline__ bool vaccine_newly(float u, float lo, float hi) { return lo <= u && u < hi; }

constexpr int kVaccineAges = 100, kVaccineTable = 3 * kVaccineAges;
static_assert(sizeof(gj_vaccinate_tables) == kVaccineTable * sizeof(float), "gj_vaccinate_tables: three packed tables");

// tab = thr_lo | thr_hi | factor; ends with a barrier
__device__ __forceinline__ void vaccine_stage_tables(const gj_vaccinate_tables& T, float* tab) {
  const float* src = reinterpret_cast<const float*>(&T);
  for (int i = threadIdx.x; i < kVaccineTable; i += blockDim.x) tab[i] = src[i];
  __syncthreads();
}
// one agent's decision and the factor its susceptibility is multiplied by (1 where it is not newly vaccinated)
__device__ __forceinline__ bool vaccine_agent(const float* tab, int cls, float u, float& factor) {
  const int age = cls % kVaccineAges;
  const bool nw = vaccine_newly(u, tab[age], tab[kVaccineAges + age]);
  factor = nw ? tab[2 * kVaccineAges + age] : 1.0f;
  return nw;
}
// the uniforms of the global ids g0 .. g0 + 3, g0 a multiple of 4: infection_uniform's, from one block
__device__ __forceinline__ void vaccine_uniforms4(uint64_t seed, uint64_t stream, int64_t g0, float (&u)[4]) {
  uint32_t r[4];
  philox4x32_10((uint64_t)g0 >> 2, stream, seed, r);
#pragma unroll
  for (int j = 0; j < 4; ++j) u[j] = u01(r[j]);
}

struct VaccinateArgs {
  gj_vaccinate_tables T;
  int64_t n;
  const uint8_t* cls;
  uint64_t seed, stream;
  int64_t agent_offset;
  float* susc;
  float* newly;                // [n] or NULL
  unsigned long long* count;   // [1] or NULL
  int32_t vec4;                // agent_offset % 4 == 0 and susc, newly 16-byte, cls 4-byte aligned
};

// Workgroups of 1024 lanes, at most 512 of them (the shape of k_group_stats' LDS form: the same waves per CU as 2048
// workgroups of 256), because every workgroup with a count ends in one atomic on ONE address, and those serialise: with
// 2048 workgroups the launch that moves 1 % of 10 M agents took 34 us, of which the atomics were 20.
constexpr int kVaccineThreads = 1024, kVaccineBlocks = 512;

__global__ __launch_bounds__(kVaccineThreads) void k_vaccinate(const VaccinateArgs S) {
  __shared__ float tab[kVaccineTable];
  __shared__ uint32_t part[kVaccineThreads / kWave];
  vaccine_stage_tables(S.T, tab);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint32_t cnt = 0;            // (a lane meets n / (lanes of the grid) agents: far below 2^32)
  int64_t first_scalar = 0;
  if (S.vec4) {
    const int64_t n4 = S.n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      // both loads issued before the Philox rounds
      const uint32_t cl = reinterpret_cast<const uint32_t*>(S.cls)[i];
      float4 s = reinterpret_cast<const float4*>(S.susc)[i];
      float u[4], f0, f1, f2, f3;
      vaccine_uniforms4(S.seed, S.stream, S.agent_offset + 4 * i, u);
      const bool n0 = vaccine_agent(tab, (int)(cl & 0xFF), u[0], f0);
      const bool n1 = vaccine_agent(tab, (int)((cl >> 8) & 0xFF), u[1], f1);
      const bool n2 = vaccine_agent(tab, (int)((cl >> 16) & 0xFF), u[2], f2);
      const bool n3 = vaccine_agent(tab, (int)(cl >> 24), u[3], f3);
      if (n0 || n1 || n2 || n3) {      // most steps move few agents: the array is read, not rewritten
        if (n0) s.x *= f0;
        if (n1) s.y *= f1;
        if (n2) s.z *= f2;
        if (n3) s.w *= f3;
        reinterpret_cast<float4*>(S.susc)[i] = s;
      }
      if (S.newly)
        reinterpret_cast<float4*>(S.newly)[i] =
            make_float4(n0 ? 1.0f : 0.0f, n1 ? 1.0f : 0.0f, n2 ? 1.0f : 0.0f, n3 ? 1.0f : 0.0f);
      cnt += (uint32_t)n0 + (uint32_t)n1 + (uint32_t)n2 + (uint32_t)n3;
    }
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < S.n; a += stride) {
    float f;
    const bool nw = vaccine_agent(tab, (int)S.cls[a], infection_uniform(S.seed, S.stream, S.agent_offset + a), f);
    if (nw) S.susc[a] = S.susc[a] * f;
    if (S.newly) S.newly[a] = nw ? 1.0f : 0.0f;
    cnt += (uint32_t)nw;
  }
  // the workgroup's count: a wave sum, the waves' sums through LDS, one integer atomic where it is not zero
  cnt = wave_sum(cnt);
  if (threadIdx.x % kWave == 0) part[threadIdx.x / kWave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0 && S.count) {
    unsigned long long v = 0;
    for (int w = 0; w < kVaccineThreads / kWave; ++w) v += part[w];
    if (v) atomicAdd(S.count, v);
  }
}

// The adjoint's per-agent launch: g_in and the term of d loss / d efficacy[band] into the workspace that the seed's two
// summing kernels (k_adjoint_seed_chunks, k_adjoint_seed_finish) then reduce in the order of the band's gj_seed_plan.
struct VaccinateAdjArgs {
  gj_vaccinate_tables T;
  int64_t n;
  const uint8_t* cls;
  uint64_t seed, stream;
  int64_t agent_offset;
  const float* susc0;
  const float* g_out;          // [n] or NULL (zeros)
  const int32_t* band;         // [n]
  int32_t n_bands;
  int32_t vec4;                // agent_offset % 4 == 0 and every array given 16-byte (cls: 4-byte) aligned
  double* contrib;             // [n]
  float* g_in;                 // [n] or NULL
};

// susceptibility' = susceptibility0 * factor, factor = 1 - efficacy[band] where newly: d / d efficacy = -susceptibility0.
// The product of two fp32 values is exact in fp64.  A label outside [0, n_bands) is no band: no term, never an index.
__device__ __forceinline__ void vaccine_adjoint_agent(const float* tab, int cls, float u, float s0, float g, int32_t band,
                                                      int32_t n_bands, double& c, float& gi) {
  float f;
  const bool nw = vaccine_agent(tab, cls, u, f);
  gi = g * f;
  c = (nw && (uint32_t)band < (uint32_t)n_bands) ? -((double)g * (double)s0) : 0.0;
}

__global__ __launch_bounds__(kThreads) void k_adjoint_vaccinate_agents(const VaccinateAdjArgs S) {
  __shared__ float tab[kVaccineTable];
  vaccine_stage_tables(S.T, tab);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t first_scalar = 0;
  if (S.vec4) {
    const int64_t n4 = S.n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const uint32_t cl = reinterpret_cast<const uint32_t*>(S.cls)[i];
      const float4 s = reinterpret_cast<const float4*>(S.susc0)[i];
      const float4 g = S.g_out ? reinterpret_cast<const float4*>(S.g_out)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      const int4 b = reinterpret_cast<const int4*>(S.band)[i];
      float u[4];
      vaccine_uniforms4(S.seed, S.stream, S.agent_offset + 4 * i, u);
      double c0, c1, c2, c3;
      float4 gi;
      vaccine_adjoint_agent(tab, (int)(cl & 0xFF), u[0], s.x, g.x, b.x, S.n_bands, c0, gi.x);
      vaccine_adjoint_agent(tab, (int)((cl >> 8) & 0xFF), u[1], s.y, g.y, b.y, S.n_bands, c1, gi.y);
      vaccine_adjoint_agent(tab, (int)((cl >> 16) & 0xFF), u[2], s.z, g.z, b.z, S.n_bands, c2, gi.z);
      vaccine_adjoint_agent(tab, (int)(cl >> 24), u[3], s.w, g.w, b.w, S.n_bands, c3, gi.w);
      reinterpret_cast<double2*>(S.contrib)[2 * i] = make_double2(c0, c1);
      reinterpret_cast<double2*>(S.contrib)[2 * i + 1] = make_double2(c2, c3);
      if (S.g_in) reinterpret_cast<float4*>(S.g_in)[i] = gi;
    }
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < S.n; a += stride) {
    double c;
    float gi;
    vaccine_adjoint_agent(tab, (int)S.cls[a], infection_uniform(S.seed, S.stream, S.agent_offset + a), S.susc0[a],
                          S.g_out ? S.g_out[a] : 0.0f, S.band[a], S.n_bands, c, gi);
    S.contrib[a] = c;
    if (S.g_in) S.g_in[a] = gi;
  }
}

// Waning immunity (include/gradjune_hip.h, gj_immunity_step / gj_adjoint_immunity): streaming, per agent, after a step.
// ONE definition of the rule, shared by the update and the numpy restatement the tests hold it to; the adjoint replays
// the update's decisions from its flags.
constexpr int kImmunityTable = 2 * kVaccineAges;
static_assert(sizeof(gj_immunity_tables) == kImmunityTable * sizeof(float), "gj_immunity_tables: two packed tables");
constexpr uint32_t kImmunityWaned = 1, kImmunityReinfected = 2;

// tab = cap | keep; ends with a barrier
__device__ __forceinline__ void immunity_stage_tables(const gj_immunity_tables& T, float* tab) {
  const float* src = reinterpret_cast<const float*>(&T);
  for (int i = threadIdx.x; i < kImmunityTable; i += blockDim.x) tab[i] = src[i];
  __syncthreads();
}
__device__ __forceinline__ bool immunity_wanes(const float* tab, int cls, float stage, float recovered, float nw) {
  return stage == recovered && !(nw != 0.0f) && tab[kVaccineAges + cls % kVaccineAges] != 1.0f;
}
// s' = cap - (cap - s) * keep: three fp32 operations (the build keeps them apart: -ffp-contract=off)
__device__ __forceinline__ float immunity_relax(const float* tab, int cls, float s) {
  const int age = cls % kVaccineAges;
  const float cap = tab[age];
  const float gap = cap - s;
  return cap - gap * tab[kVaccineAges + age];
}
// a newly infected agent that had an infection before: the step's increment is undone
__device__ __forceinline__ bool immunity_reinfected(float nw, float& inf) {
  const float before = inf - nw;
  if (!(before >= 1.0f)) return false;
  inf = before;
  return true;
}
// the agent's term of susc_sum_out: exact scaling and truncation; a NaN counts 0 (fmaxf returns the number)
__device__ __forceinline__ uint64_t immunity_fixed(float s) {
  return (uint64_t)(int64_t)(fminf(fmaxf(s, 0.0f), 4.0f) * 1073741824.0f);
}

struct ImmunityArgs {
  gj_immunity_tables T;
  int64_t n;
  const uint8_t* cls;
  const float* stage;
  float recovered;
  const float* new_inf;        // [n] or NULL (nobody)
  float* susc;
  float* inf;
  uint8_t* flags;              // [n] or NULL
  float* reinf;                // [n] or NULL
  unsigned long long* count;   // [1] or NULL
  unsigned long long* susc_sum;  // [1] or NULL
  int32_t vec4;                // the fp32 arrays given 16-byte, cls and flags 4-byte aligned
};

// k_vaccinate's shape: workgroups of 1024 lanes, at most 512 of them, one integer atomic per output and workgroup.
__global__ __launch_bounds__(kVaccineThreads) void k_immunity(const ImmunityArgs S) {
  __shared__ float tab[kImmunityTable];
  __shared__ uint32_t part_cnt[kVaccineThreads / kWave];
  __shared__ uint64_t part_sum[kVaccineThreads / kWave];
  immunity_stage_tables(S.T, tab);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool want_sum = S.susc_sum != nullptr;
  uint32_t cnt = 0;            // (a lane meets n / (lanes of the grid) agents: far below 2^32)
  uint64_t sum = 0;            // (at most 2^32 an agent)
  int64_t first_scalar = 0;
  if (S.vec4) {
    const int64_t n4 = S.n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const uint32_t cl = reinterpret_cast<const uint32_t*>(S.cls)[i];
      const float4 st = reinterpret_cast<const float4*>(S.stage)[i];
      const float4 nw = S.new_inf ? reinterpret_cast<const float4*>(S.new_inf)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      const int c0 = (int)(cl & 0xFF), c1 = (int)((cl >> 8) & 0xFF), c2 = (int)((cl >> 16) & 0xFF), c3 = (int)(cl >> 24);
      const bool w0 = immunity_wanes(tab, c0, st.x, S.recovered, nw.x), w1 = immunity_wanes(tab, c1, st.y, S.recovered, nw.y);
      const bool w2 = immunity_wanes(tab, c2, st.z, S.recovered, nw.z), w3 = immunity_wanes(tab, c3, st.w, S.recovered, nw.w);
      const bool any_w = w0 || w1 || w2 || w3;
      if (any_w || want_sum) {      // most agents are not recovered: their susceptibility is not read
        float4 s = reinterpret_cast<const float4*>(S.susc)[i];
        if (any_w) {
          if (w0) s.x = immunity_relax(tab, c0, s.x);
          if (w1) s.y = immunity_relax(tab, c1, s.y);
          if (w2) s.z = immunity_relax(tab, c2, s.z);
          if (w3) s.w = immunity_relax(tab, c3, s.w);
          reinterpret_cast<float4*>(S.susc)[i] = s;
        }
        if (want_sum) sum += immunity_fixed(s.x) + immunity_fixed(s.y) + immunity_fixed(s.z) + immunity_fixed(s.w);
      }
      bool r0 = false, r1 = false, r2 = false, r3 = false;
      if (nw.x != 0.0f || nw.y != 0.0f || nw.z != 0.0f || nw.w != 0.0f) {      // few lanes hold a new infection
        float4 f = reinterpret_cast<const float4*>(S.inf)[i];
        if (nw.x != 0.0f) r0 = immunity_reinfected(nw.x, f.x);
        if (nw.y != 0.0f) r1 = immunity_reinfected(nw.y, f.y);
        if (nw.z != 0.0f) r2 = immunity_reinfected(nw.z, f.z);
        if (nw.w != 0.0f) r3 = immunity_reinfected(nw.w, f.w);
        if (r0 || r1 || r2 || r3) reinterpret_cast<float4*>(S.inf)[i] = f;
      }
      if (S.flags)
        reinterpret_cast<uint32_t*>(S.flags)[i] =
            ((uint32_t)w0 | (uint32_t)r0 << 1) | ((uint32_t)w1 | (uint32_t)r1 << 1) << 8 |
            ((uint32_t)w2 | (uint32_t)r2 << 1) << 16 | ((uint32_t)w3 | (uint32_t)r3 << 1) << 24;
      if (S.reinf)
        reinterpret_cast<float4*>(S.reinf)[i] =
            make_float4(r0 ? 1.0f : 0.0f, r1 ? 1.0f : 0.0f, r2 ? 1.0f : 0.0f, r3 ? 1.0f : 0.0f);
      cnt += (uint32_t)r0 + (uint32_t)r1 + (uint32_t)r2 + (uint32_t)r3;
    }
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < S.n; a += stride) {
    const int cls = (int)S.cls[a];
    const float nw = S.new_inf ? S.new_inf[a] : 0.0f;
    const bool w = immunity_wanes(tab, cls, S.stage[a], S.recovered, nw);
    if (w || want_sum) {
      float s = S.susc[a];
      if (w) S.susc[a] = s = immunity_relax(tab, cls, s);
      if (want_sum) sum += immunity_fixed(s);
    }
    bool r = false;
    if (nw != 0.0f) {
      float f = S.inf[a];
      r = immunity_reinfected(nw, f);
      if (r) S.inf[a] = f;
    }
    if (S.flags) S.flags[a] = (uint8_t)((uint32_t)w | (uint32_t)r << 1);
    if (S.reinf) S.reinf[a] = r ? 1.0f : 0.0f;
    cnt += (uint32_t)r;
  }
  // the workgroup's sums: a wave sum, the waves' sums through LDS, one integer atomic per output where it is not zero
  cnt = wave_sum(cnt);
  sum = wave_sum(sum);
  if (threadIdx.x % kWave == 0) {
    part_cnt[threadIdx.x / kWave] = cnt;
    part_sum[threadIdx.x / kWave] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long c = 0, v = 0;
    for (int w = 0; w < kVaccineThreads / kWave; ++w) {
      c += part_cnt[w];
      v += part_sum[w];
    }
    if (S.count && c) atomicAdd(S.count, c);
    if (S.susc_sum && v) atomicAdd(S.susc_sum, v);
  }
}

// The adjoint's per-agent launch: the three per-agent gradients and the agent's terms of sum_A and sum_B into the
// workspace that the seed's two summing kernels then reduce, each in the order of the band's gj_seed_plan.
struct ImmunityAdjArgs {
  gj_immunity_tables T;
  int64_t n;
  const uint8_t* flags;
  const uint8_t* cls;
  const float* susc0;
  const float* g_susc;         // [n] or NULL (zeros)
  const float* g_inf;          // [n] or NULL (zeros)
  const int32_t* band;         // [n]
  int32_t n_bands;
  int32_t vec4;                // every array given 16-byte (flags, cls: 4-byte) aligned, contrib_b too
  double* contrib_a;           // [n]
  double* contrib_b;           // [n]
  float* g_susc_in;            // [n] or NULL
  float* g_inf_in;             // [n] or NULL
  float* g_new;                // [n] or NULL
};

// s' = cap - (cap - s0) * keep where waned: d / d s0 = keep, d / d keep = -(cap - s0), d / d cap = 1 - keep.
// cap - s0 is the forward's fp32 difference; its product with g is exact in fp64.  A label outside [0, n_bands) is no
// band: no term, never an index.
__device__ __forceinline__ void immunity_adjoint_agent(const float* tab, uint32_t flag, int cls, float s0, float gs,
                                                       float gi, int32_t band, int32_t n_bands, double& ca, double& cb,
                                                       float& gs_in, float& gn) {
  const int age = cls % kVaccineAges;
  const bool waned = (flag & kImmunityWaned) != 0;
  gs_in = waned ? gs * tab[kVaccineAges + age] : gs;
  gn = (flag & kImmunityReinfected) ? -gi : 0.0f;
  const bool term = waned && (uint32_t)band < (uint32_t)n_bands;
  const float gap = tab[age] - s0;
  ca = term ? (double)gs * (double)gap : 0.0;
  cb = term ? (double)gs : 0.0;
}

__global__ __launch_bounds__(kThreads) void k_adjoint_immunity_agents(const ImmunityAdjArgs S) {
  __shared__ float tab[kImmunityTable];
  immunity_stage_tables(S.T, tab);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t first_scalar = 0;
  if (S.vec4) {
    const int64_t n4 = S.n >> 2;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const uint32_t fl = reinterpret_cast<const uint32_t*>(S.flags)[i];
      const uint32_t cl = reinterpret_cast<const uint32_t*>(S.cls)[i];
      const float4 s = reinterpret_cast<const float4*>(S.susc0)[i];
      const float4 gs = S.g_susc ? reinterpret_cast<const float4*>(S.g_susc)[i] : zero;
      const float4 gi = S.g_inf ? reinterpret_cast<const float4*>(S.g_inf)[i] : zero;
      const int4 b = reinterpret_cast<const int4*>(S.band)[i];
      double a0, a1, a2, a3, b0, b1, b2, b3;
      float4 go, gn;
      immunity_adjoint_agent(tab, fl & 0xFF, (int)(cl & 0xFF), s.x, gs.x, gi.x, b.x, S.n_bands, a0, b0, go.x, gn.x);
      immunity_adjoint_agent(tab, (fl >> 8) & 0xFF, (int)((cl >> 8) & 0xFF), s.y, gs.y, gi.y, b.y, S.n_bands, a1, b1,
                             go.y, gn.y);
      immunity_adjoint_agent(tab, (fl >> 16) & 0xFF, (int)((cl >> 16) & 0xFF), s.z, gs.z, gi.z, b.z, S.n_bands, a2, b2,
                             go.z, gn.z);
      immunity_adjoint_agent(tab, fl >> 24, (int)(cl >> 24), s.w, gs.w, gi.w, b.w, S.n_bands, a3, b3, go.w, gn.w);
      reinterpret_cast<double2*>(S.contrib_a)[2 * i] = make_double2(a0, a1);
      reinterpret_cast<double2*>(S.contrib_a)[2 * i + 1] = make_double2(a2, a3);
      reinterpret_cast<double2*>(S.contrib_b)[2 * i] = make_double2(b0, b1);
      reinterpret_cast<double2*>(S.contrib_b)[2 * i + 1] = make_double2(b2, b3);
      if (S.g_susc_in) reinterpret_cast<float4*>(S.g_susc_in)[i] = go;
      if (S.g_inf_in) reinterpret_cast<float4*>(S.g_inf_in)[i] = gi;
      if (S.g_new) reinterpret_cast<float4*>(S.g_new)[i] = gn;
    }
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < S.n; a += stride) {
    double ca, cb;
    float go, gn;
    const float gi = S.g_inf ? S.g_inf[a] : 0.0f;
    immunity_adjoint_agent(tab, S.flags[a], (int)S.cls[a], S.susc0[a], S.g_susc ? S.g_susc[a] : 0.0f, gi, S.band[a],
                           S.n_bands, ca, cb, go, gn);
    S.contrib_a[a] = ca;
    S.contrib_b[a] = cb;
    if (S.g_susc_in) S.g_susc_in[a] = go;
    if (S.g_inf_in) S.g_inf_in[a] = gi;
    if (S.g_new) S.g_new[a] = gn;
  }
}

// psi(x) = d lgamma / dx (torch.digamma, the derivative torch's autograd gives lgamma), for the adjoint of the profile's
// 1 / Gamma(shape).  x < 0: reflection psi(x) = psi(1 - x) - pi / tan(pi x), NaN at the poles; x == 0: -inf (torch:
// copysign(inf, -x)).  x > 0: the recurrence psi(x) = psi(x + 1) - 1/x up to x >= 6, then the asymptotic series to
// x^-6 (truncation: next term 1/(240 x^8) < 2.6e-9 there).  The error is that of fp32 rounding of the sum: a few ulp
// of the largest term, i.e. ~1e-6 absolute for x >= 0.25 and a few ulp of 1/x below (x = 0.02: psi ~ -50, ~1e-5) -
// over inv_gamma's fast range (0.25, 16) and its libm fallback range alike.  NaN in, NaN out.  No libm: v_log_f32
// and (x < 0 only) v_sin/v_cos.
__device__ __forceinline__ float digamma(float x) {
  if (x == 0.0f) return copysignf(__builtin_inff(), -x);
  float refl = 0.0f;
  if (x < 0.0f) {
    const float r = x - truncf(x);                     // (-1, 0]; tan(pi x) = tan(pi r)
    if (r == 0.0f) return __builtin_nanf("");          // negative integer: a pole
    // v_sin_f32 / v_cos_f32 take revolutions: sin(pi r) = sin(2 pi * r / 2)
    refl = 3.14159265358979f * __builtin_amdgcn_cosf(0.5f * r) / __builtin_amdgcn_sinf(0.5f * r);
    x = 1.0f - x;
  }
  float acc = 0.0f;
  while (x < 6.0f) {                                   // (false for NaN)
    acc += 1.0f / x;
    x += 1.0f;
  }
  const float ix = 1.0f / x, ix2 = ix * ix;
  float s = ix2 * (1.0f / 252.0f);
  s = ix2 * (1.0f / 120.0f - s);
  s = ix2 * (1.0f / 12.0f - s);
  const float lnx = __builtin_amdgcn_logf(x) * 0.693147180559945309f;
  return lnx - 0.5f * ix - s - acc - refl;
}

// f3: the profile's adjoint, one body for two kernels.  k_adjoint_transmission (PARAMS = false): grad_inf = g_inf +
// trans_bar * d trans / d is_infected and grad_time -= trans_bar * d trans / d t.  k_adjoint_transmission_params adds
// the adjoint w.r.t. the profile's own per-agent parameters.  With T the profile, d = t - shift, u = d * rate:
//   dT/d max_inf = sign * aux * aux2 * is_infected   (not T / max_inf: max_inf == 0 is allowed)
//   dT/d shape   = T * (ln u - psi(shape))           (torch: pow'(exponent) = pow * ln(base), masked to 0 at base == 0
//                                                     with exponent >= 0; lgamma' = digamma)
//   dT/d rate    = T * (shape / rate - d)
//   dT/d shift   = T * (rate - (shape - 1) / d)      (= -dT/dt: the infection_time term shares it; d == 0 is taken apart
//                                                     from the division, see below)
// Each NULL output is neither computed nor written: a launch moves bytes only for the parameters that need a gradient.
// is_infected == 0 gives 0 in every output.
template <bool PARAMS>
__device__ __forceinline__ void adjoint_transmission_agent(
    int64_t n, const float* __restrict__ mx, const float* __restrict__ shp, const float* __restrict__ rt,
    const float* __restrict__ sh, const float* __restrict__ time0, const float* __restrict__ inf0, float now,
    const float* __restrict__ trans_bar, const float* __restrict__ g_inf, float* __restrict__ grad_inf,
    float* __restrict__ grad_time, float* __restrict__ grad_mx, float* __restrict__ grad_shp,
    float* __restrict__ grad_rt, float* __restrict__ grad_sh) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;
  const float s = shp[a], r = rt[a];
  const ProfileHead h = profile_head(s, r, sh[a], time0[a], now);
  const float base = mx[a] * h.sign * h.aux * h.aux2;        // d trans / d is_infected
  const float tb = trans_bar[a];                             // (loaded here: not held in a register across the profile)
  const float inf = inf0[a];
  float p_mx = 0.0f, p_shp = 0.0f, p_rt = 0.0f, dtdt = 0.0f;  // d trans / d parameter; d trans / d t = -dT/d shift
  if (inf != 0.0f) {
    const float T = base * inf;
    if (h.d != 0.0f) {
      dtdt = T * ((s - 1.0f) / h.d - r);
    } else {
      // t == shift exactly (a constant integer shape and a shift that is a multiple of the step: once per infected
      // agent): T * ((s - 1) / 0 - r) is T * (0 / 0) at shape 1 and 0 * inf at shape >= 2.  The derivative of the pow
      // as torch takes it, y * pow(base, y - 1) with a zero exponent y contributing 0: -r T at shape 1,
      // max_inf * sign / Gamma(2) * aux2 * is_infected * r at shape 2, 0 above; +-inf or NaN at a non-integer shape < 2.
      const float y = s - 1.0f;
      const float lead = (y == 0.0f) ? 0.0f : y * fast_pow(0.0f, y - 1.0f);
      dtdt = mx[a] * h.sign * inv_gamma(s) * h.aux2 * inf * r * lead - r * T;
    }
    if (PARAMS && grad_mx) p_mx = h.sign * h.aux * h.aux2 * inf;
    if (PARAMS && grad_shp) {
      const float u = h.d * r;
      const float lnu = (u == 0.0f && s >= 1.0f) ? 0.0f : __builtin_amdgcn_logf(u) * 0.693147180559945309f;
      p_shp = T * lnu - T * digamma(s);
    }
    if (PARAMS && grad_rt) p_rt = T * (s / r - h.d);
  }
  grad_inf[a] = (g_inf ? g_inf[a] : 0.0f) + tb * base;
  grad_time[a] = grad_time[a] - tb * dtdt;                   // d t / d infection_time = -1
  if (PARAMS && grad_mx) grad_mx[a] = tb * p_mx;
  if (PARAMS && grad_shp) grad_shp[a] = tb * p_shp;
  if (PARAMS && grad_rt) grad_rt[a] = tb * p_rt;
  if (PARAMS && grad_sh) grad_sh[a] = 0.0f - tb * dtdt;     // (0 - x: no -0 for the uninfected)
}

__global__ __launch_bounds__(kThreads) void k_adjoint_transmission(
    int64_t n, const float* __restrict__ mx, const float* __restrict__ shp, const float* __restrict__ rt,
    const float* __restrict__ sh, const float* __restrict__ time0, const float* __restrict__ inf0, float now,
    const float* __restrict__ trans_bar, const float* __restrict__ g_inf, float* __restrict__ grad_inf,
    float* __restrict__ grad_time) {
  adjoint_transmission_agent<false>(n, mx, shp, rt, sh, time0, inf0, now, trans_bar, g_inf, grad_inf, grad_time,
                                    nullptr, nullptr, nullptr, nullptr);
}
__global__ __launch_bounds__(kThreads) void k_adjoint_transmission_params(
    int64_t n, const float* __restrict__ mx, const float* __restrict__ shp, const float* __restrict__ rt,
    const float* __restrict__ sh, const float* __restrict__ time0, const float* __restrict__ inf0, float now,
    const float* __restrict__ trans_bar, const float* __restrict__ g_inf, float* __restrict__ grad_inf,
    float* __restrict__ grad_time, float* __restrict__ grad_mx, float* __restrict__ grad_shp,
    float* __restrict__ grad_rt, float* __restrict__ grad_sh) {
  adjoint_transmission_agent<true>(n, mx, shp, rt, sh, time0, inf0, now, trans_bar, g_inf, grad_inf, grad_time, grad_mx,
                                   grad_shp, grad_rt, grad_sh);
}

// f2: per-step result reductions (reference grad_june/runner.py:167,198-224), one streaming pass
struct StatsArgs {
  int64_t n;
  const uint8_t* cls;
  const float* inf;
  const float* stage;
  int32_t n_bins;
  int32_t edges[GJ_MAX_AGE_BINS + 1];
  int32_t dead;
  int32_t vec4;     // all three arrays 16-byte (cls: 4-byte) aligned
  double* out;
};

// A lane's sums over its agents - cases, cases per age bin, deaths - and the workgroup's reduction of them: a wave sum,
// the waves' sums through LDS in wave order, one atomicAdd per non-zero output.  One per kernel (finish owns the LDS).
struct AgeBins {
  static constexpr int kOut = GJ_MAX_AGE_BINS + 2;
  const StatsArgs& R;
  double acc[kOut];
  __device__ __forceinline__ explicit AgeBins(const StatsArgs& r) : R(r) {
#pragma unroll
    for (int k = 0; k < kOut; ++k) acc[k] = 0.0;
  }
  __device__ __forceinline__ void take(float inf, float stage, int cls) {
    const int age = cls % 100;
    acc[0] += inf;
#pragma unroll
    for (int b = 0; b < GJ_MAX_AGE_BINS; ++b)
      if (b < R.n_bins && age > R.edges[b] && age < R.edges[b + 1]) acc[1 + b] += inf;
    if (stage == (float)R.dead) acc[GJ_MAX_AGE_BINS + 1] += 1.0;
  }
  // four agents of one dword of classes
  __device__ __forceinline__ void take4(const float4& inf, const float4& stage, uint32_t cls) {
    take(inf.x, stage.x, (int)(cls & 0xFF));
    take(inf.y, stage.y, (int)((cls >> 8) & 0xFF));
    take(inf.z, stage.z, (int)((cls >> 16) & 0xFF));
    take(inf.w, stage.w, (int)(cls >> 24));
  }
  __device__ __forceinline__ void finish(double* out) {
    __shared__ double part[kThreads / kWave][kOut];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
#pragma unroll
    for (int k = 0; k < kOut; ++k) {
      const double v = wave_sum(acc[k]);
      if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kOut) {
      double v = 0.0;
      for (int w = 0; w < kThreads / kWave; ++w) v += part[w][threadIdx.x];
      const int k = threadIdx.x;
      int dst = -1;
      if (k == 0) dst = 0;
      else if (k <= GJ_MAX_AGE_BINS) dst = (k - 1 < R.n_bins) ? k : -1;
      else dst = 1 + R.n_bins;
      if (dst >= 0 && v != 0.0) atomicAdd(&out[dst], v);
    }
  }
};

__global__ __launch_bounds__(kThreads) void k_step_stats(const StatsArgs S) {
  AgeBins bins(S);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t first_scalar = 0;
  if (S.vec4) {   // 16-byte aligned arrays: four agents per lane and load (the scalar form is latency-bound)
    const int64_t n4 = S.n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
      bins.take4(reinterpret_cast<const float4*>(S.inf)[i], reinterpret_cast<const float4*>(S.stage)[i],
                 reinterpret_cast<const uint32_t*>(S.cls)[i]);
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < S.n; a += stride)
    bins.take(S.inf[a], S.stage[a], (int)S.cls[a]);
  bins.finish(S.out);
}

// f1 + f2 in one pass (gj_symptoms_step_stats): the stage update of four agents per lane, written back only where a
// value changed (early in an epidemic almost nobody moves: the three arrays are then read, not rewritten), and the
// Runner's reductions taken from the registers that hold the updated stages.
__global__ __launch_bounds__(kThreads) void k_symptoms_stats(const SymptomsArgs S, const StatsArgs R) {
  AgeBins bins(R);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t first_scalar = 0;
  if (R.vec4) {
    const int64_t n4 = S.n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      // all six loads issued before the first use
      const float4 nw = reinterpret_cast<const float4*>(S.new_inf)[i];
      float4 c = reinterpret_cast<const float4*>(S.cur)[i];
      float4 x = reinterpret_cast<const float4*>(S.nxt)[i];
      float4 t = reinterpret_cast<const float4*>(S.ttn)[i];
      const float4 f = reinterpret_cast<const float4*>(R.inf)[i];
      const uint32_t cl = reinterpret_cast<const uint32_t*>(S.cls)[i];
      bool ch = symptoms_agent(S, 4 * i, nw.x, (int)(cl & 0xFF), c.x, x.x, t.x);
      ch |= symptoms_agent(S, 4 * i + 1, nw.y, (int)((cl >> 8) & 0xFF), c.y, x.y, t.y);
      ch |= symptoms_agent(S, 4 * i + 2, nw.z, (int)((cl >> 16) & 0xFF), c.z, x.z, t.z);
      ch |= symptoms_agent(S, 4 * i + 3, nw.w, (int)(cl >> 24), c.w, x.w, t.w);
      if (ch) {
        reinterpret_cast<float4*>(S.cur)[i] = c;
        reinterpret_cast<float4*>(S.nxt)[i] = x;
        reinterpret_cast<float4*>(S.ttn)[i] = t;
      }
      bins.take4(f, c, cl);
    }
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < S.n; a += stride) {
    float cur = S.cur[a], nx = S.nxt[a], tt = S.ttn[a];
    const int cls = (int)S.cls[a];
    if (symptoms_agent(S, a, S.new_inf[a], cls, cur, nx, tt)) {
      S.cur[a] = cur;
      S.nxt[a] = nx;
      S.ttn[a] = tt;
    }
    bins.take(R.inf[a], cur, cls);
  }
  bins.finish(R.out);
}

// f2 by agent group (gj_group_stats): segmented sums of is_infected and of the deaths indicator over an int32 label.
// Summed as 64-bit integers (is_infected in 32.32 fixed point, deaths as a count), so every order of the additions
// gives the same bits.  Each lane carries ONE open run (label, two sums) across its agents; a run is closed when the
// lane meets another label.  Closing is done by the whole wave: the lanes that close the same label fold their sums
// with shuffles and one of them adds (two rounds, which is what a wave that straddles a boundary of sorted labels
// needs; lanes still open after them add on their own).  LDS = true: the adds go to this workgroup's histogram in LDS,
// which is added to the workspace at the end, one global atomic per non-zero accumulator.  LDS = false: the adds are
// global atomics on the workspace.  A workgroup owns a CONTIGUOUS share of the agents, so that sorted labels give it
// few groups.
constexpr int kGroupFxBits = 32;
constexpr int kGroupLdsMax = 4096;       // 2 * 8 B * 4096 = 64 KiB of LDS per workgroup: two workgroups per CU
constexpr int kGroupLdsThreads = 1024, kGroupLdsBlocks = 512;
constexpr int kGroupAdjLdsMax = 2048;    // gj_adjoint_group_stats stages 2 * 4 B * 2048 = 16 KiB per workgroup (above
                                         // that, filling the copy costs more than the gathers it saves)
constexpr uint32_t kGroupBadLabel = 1u, kGroupBadValue = 2u;    // GJ_GROUP_ERR_LABEL / GJ_GROUP_ERR_VALUE

struct GroupArgs {
  int64_t n;
  const int32_t* group;
  const float* inf;
  const float* stage;
  int32_t n_groups;
  int32_t dead;
  int32_t vec4;     // all three arrays 16-byte aligned
  fx_t* ws;         // [2 * n_groups] sums, then the error word
};

template <bool LDS>
__global__ __launch_bounds__(LDS ? kGroupLdsThreads : kThreads) void k_group_stats(const GroupArgs S) {
  extern __shared__ fx_t hist[];     // LDS: [2 * n_groups]
  const int G = S.n_groups;
  if (LDS) {
    for (int i = threadIdx.x; i < 2 * G; i += blockDim.x) hist[i] = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x % kWave;
  int run = -1;            // label of this lane's open run
  fx_t rc = 0, rd = 0;     // its sums: cases (fixed point), deaths (count)
  uint32_t err = 0;
  auto add = [&](int g, fx_t c, fx_t d) {
    fx_t* dst = LDS ? hist : S.ws;
    if (c) atomicAdd(&dst[g], c);
    if (d) atomicAdd(&dst[G + g], d);
  };
  // wave-convergent: closes the run of every lane with `closing` set
  auto close_runs = [&](bool closing) {
    closing = closing && run >= 0;
#pragma unroll 1
    for (int round = 0; round < 2; ++round) {
      const unsigned long long m = __ballot(closing);
      if (m == 0) return;
      const int leader = __ffsll((long long)m) - 1;
      const int label = __shfl(run, leader, kWave);
      const bool mine = closing && run == label;
      const fx_t c = wave_sum<fx_t>(mine ? rc : 0), d = wave_sum<fx_t>(mine ? rd : 0);
      if (lane == leader) add(label, c, d);
      if (mine) closing = false, run = -1, rc = 0, rd = 0;
    }
    if (closing) add(run, rc, rd), run = -1, rc = 0, rd = 0;
  };
  // wave-convergent: one agent per lane (`on` = this lane has one)
  auto take = [&](bool on, int g, float inf, float stage) {
    if (on && (uint32_t)g >= (uint32_t)G) err |= kGroupBadLabel, on = false;   // never an index: the agent is skipped
    const bool differs = on && g != run;
    if (__any(differs && run >= 0)) close_runs(differs);
    if (!on) return;
    run = g;
    const bool ok = fabsf(inf) <= fx_max<kGroupFxBits>();      // false for NaN too
    if (!ok) err |= kGroupBadValue;
    rc += to_fx<kGroupFxBits>(ok ? inf : 0.0f);
    rd += (stage == (float)S.dead) ? 1u : 0u;
  };
  // this workgroup's share, in units of four agents (vec4) or of one
  const int64_t units = S.vec4 ? (S.n >> 2) : S.n;
  const int64_t per = (units + gridDim.x - 1) / gridDim.x;
  const int64_t u0 = (int64_t)blockIdx.x * per, u1 = (u0 + per < units) ? u0 + per : units;
  for (int64_t base = u0; base < u1; base += blockDim.x) {     // (the same trip count for every lane of a wave)
    const int64_t i = base + threadIdx.x;
    const bool on = i < u1;
    if (S.vec4) {
      int4 g = make_int4(0, 0, 0, 0);
      float4 f = make_float4(0.f, 0.f, 0.f, 0.f), s = f;
      if (on) {
        g = reinterpret_cast<const int4*>(S.group)[i];
        f = reinterpret_cast<const float4*>(S.inf)[i];
        s = reinterpret_cast<const float4*>(S.stage)[i];
      }
      take(on, g.x, f.x, s.x);
      take(on, g.y, f.y, s.y);
      take(on, g.z, f.z, s.z);
      take(on, g.w, f.w, s.w);
    } else {
      take(on, on ? S.group[i] : 0, on ? S.inf[i] : 0.f, on ? S.stage[i] : 0.f);
    }
  }
  if (S.vec4 && blockIdx.x == gridDim.x - 1 && threadIdx.x < kWave) {     // the n % 4 agents behind the last float4
    const int64_t a = (units << 2) + threadIdx.x;
    const bool on = a < S.n;
    take(on, on ? S.group[a] : 0, on ? S.inf[a] : 0.f, on ? S.stage[a] : 0.f);
  }
  close_runs(true);
  if (err) atomicOr(reinterpret_cast<uint32_t*>(S.ws + 2 * (int64_t)G), err);
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * G; i += blockDim.x) {
      const fx_t v = hist[i];
      if (v) atomicAdd(&S.ws[i], v);
    }
  }
}

// out += the sums as doubles (once, so the rounding does not depend on any order); the sums are zeroed for the next call
__global__ __launch_bounds__(kThreads) void k_group_finish(int32_t n_groups, fx_t* ws, double* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * (int64_t)n_groups) return;
  const fx_t v = ws[i];
  if (v == 0) return;
  ws[i] = 0;
  out[i] += (i < n_groups) ? (double)(long long)v * (1.0 / (double)(1ull << kGroupFxBits)) : (double)v;
}

// adjoint of gj_group_stats: a gather through the labels
struct GroupAdjArgs {
  int64_t n;
  const int32_t* group;
  const float* stage;
  const float* g_cases;
  const float* g_deaths;
  float* grad_inf;
  float* grad_stage;
  int32_t n_groups;
  int32_t dead;
  int32_t vec4;
};

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_adjoint_group_stats(const GroupAdjArgs S) {
  extern __shared__ float staged[];     // LDS: g_cases [n_groups], g_deaths [n_groups]
  const int G = S.n_groups;
  const float* gc = S.g_cases;
  const float* gd = S.g_deaths;
  if (LDS) {
    for (int i = threadIdx.x; i < G; i += blockDim.x) {
      staged[i] = gc ? gc[i] : 0.0f;
      staged[G + i] = gd ? gd[i] : 0.0f;
    }
    __syncthreads();
    gc = staged;
    gd = staged + G;
  }
  const float dead = (float)S.dead;
  auto cases = [&](int g) { return ((uint32_t)g < (uint32_t)G && gc) ? gc[g] : 0.0f; };
  auto deaths = [&](int g, float st) {      // autograd of (stage == dead) * stage / dead: (g / dead) * mask
    const float v = ((uint32_t)g < (uint32_t)G && gd) ? gd[g] : 0.0f;
    return v / dead * (st == dead ? 1.0f : 0.0f);
  };
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t first_scalar = 0;
  if (S.vec4) {
    const int64_t n4 = S.n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const int4 g = reinterpret_cast<const int4*>(S.group)[i];
      if (S.grad_inf) reinterpret_cast<float4*>(S.grad_inf)[i] = make_float4(cases(g.x), cases(g.y), cases(g.z), cases(g.w));
      if (S.grad_stage) {
        const float4 s = reinterpret_cast<const float4*>(S.stage)[i];
        reinterpret_cast<float4*>(S.grad_stage)[i] =
            make_float4(deaths(g.x, s.x), deaths(g.y, s.y), deaths(g.z, s.z), deaths(g.w, s.w));
      }
    }
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < S.n; a += stride) {
    const int g = S.group[a];
    if (S.grad_inf) S.grad_inf[a] = cases(g);
    if (S.grad_stage) S.grad_stage[a] = deaths(g, S.stage[a]);
  }
}

// f2 by symptom stage (gj_stage_stats): a histogram of the agents over (group, stage) - the occupancy - and of those
// whose stage differs from the previous step's - the entries - as 64-bit counts.  Most agents sit in one or two stages,
// so one atomic per agent on the same address is the form to avoid.  kStageOne (one group): a lane counts in private
// 8-bit fields - stage s is byte s % 8 of the low (s < 8) or high word - which the host's grid keeps from overflowing
// (at most kStageLaneLoads loads of four agents per lane); the fields are added over the wave at the end.  kStageLds /
// kStageGlobal (labels): a lane carries one open run keyed on the bin g * n_stages + s, closed by the whole wave as in
// k_group_stats; the adds go to this workgroup's histogram of 32-bit counters in LDS, or to `out` as global atomics.
// kStageOne and kStageLds end by adding the histogram's non-zero counters to `out`, one 64-bit atomic each.
constexpr int kStageLdsBins = GJ_STAGE_LDS_BINS;       // 2 * 4 B * 8192 = 64 KiB of LDS per workgroup, as k_group_stats
constexpr int kStageLdsThreads = GJ_STAGE_LDS_THREADS, kStageLdsBlocks = GJ_STAGE_LDS_BLOCKS;
constexpr int kStageGlobalBlocks = GJ_STAGE_GLOBAL_BLOCKS;
constexpr int kStageLaneLoads = GJ_STAGE_LANE_LOADS;   // 63 loads * 4 agents = 252 < 256: an 8-bit field holds them
constexpr int kStageAdjLdsBins = GJ_STAGE_ADJ_LDS_BINS;   // the adjoint stages 2 * 4 B * 2048 = 16 KiB, as k_adjoint_group_stats
constexpr uint32_t kStageBadLabel = GJ_STAGE_ERR_LABEL, kStageBadStage = GJ_STAGE_ERR_STAGE;
static_assert(GJ_STAGE_GLOBAL_THREADS == kThreads && kStageLaneLoads * 4 < 256 && GJ_MAX_STAGES <= 16, "gj_stage_stats");
enum { kStageOne = 0, kStageLds = 1, kStageGlobal = 2 };

// The bin g * n_stages + s of one agent, or -1 for an agent that is skipped: a label outside [0, G) (never an index)
// or a stage that is not an integer value in [0, S) (false for NaN).  ONE definition, for the histogram and its adjoint.
__device__ __forceinline__ int stage_bin(int g, float stage, int G, int S, uint32_t& err) {
  const bool label = (uint32_t)g < (uint32_t)G;
  const bool value = stage >= 0.0f && stage < (float)S && stage == truncf(stage);
  if (!label) err |= kStageBadLabel;
  else if (!value) err |= kStageBadStage;
  return (label && value) ? g * S + (int)stage : -1;
}

struct StageArgs {
  int64_t n;
  const int32_t* group;       // [n] or NULL (every agent in group 0)
  const float* stage;
  const float* prev;          // [n] or NULL (no entries)
  int32_t n_groups, n_stages;
  int32_t vec4;               // every array given is 16-byte aligned
  unsigned long long* out;    // [2][n_groups][n_stages]
  uint32_t* err;
};

template <int MODE>
__global__ __launch_bounds__(MODE == kStageGlobal ? kThreads : kStageLdsThreads) void k_stage_stats(const StageArgs A) {
  extern __shared__ uint32_t stage_hist[];     // kStageOne, kStageLds: [2 * bins]
  const int G = A.n_groups, S = A.n_stages, bins = G * S;      // (bins <= INT32_MAX; the second plane is indexed in 64 bits)
  if (MODE != kStageGlobal) {
    for (int i = threadIdx.x; i < 2 * bins; i += blockDim.x) stage_hist[i] = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x % kWave;
  uint64_t occ_lo = 0, occ_hi = 0, ent_lo = 0, ent_hi = 0;     // kStageOne: this lane's counts, 8 bits per stage
  int run = -1;                                                // otherwise: the bin of this lane's open run
  uint32_t ro = 0, re = 0;                                     // and its counts: occupancy, entries
  uint32_t err = 0;
  auto add = [&](int b, uint32_t o, uint32_t e) {
    if (MODE == kStageGlobal) {
      if (o) atomicAdd(&A.out[b], (unsigned long long)o);
      if (e) atomicAdd(&A.out[(int64_t)bins + b], (unsigned long long)e);
    } else {
      if (o) atomicAdd(&stage_hist[b], o);
      if (e) atomicAdd(&stage_hist[bins + b], e);
    }
  };
  // wave-convergent: closes the run of every lane with `closing` set (k_group_stats' close_runs, on bins)
  auto close_runs = [&](bool closing) {
    closing = closing && run >= 0;
#pragma unroll 1
    for (int round = 0; round < 2; ++round) {
      const unsigned long long m = __ballot(closing);
      if (m == 0) return;
      const int leader = __ffsll((long long)m) - 1;
      const int bin = __shfl(run, leader, kWave);
      const bool mine = closing && run == bin;
      const uint32_t o = wave_sum<uint32_t>(mine ? ro : 0u), e = wave_sum<uint32_t>(mine ? re : 0u);
      if (lane == leader) add(bin, o, e);
      if (mine) closing = false, run = -1, ro = 0, re = 0;
    }
    if (closing) add(run, ro, re), run = -1, ro = 0, re = 0;
  };
  // one agent per lane (`on` = this lane has one); wave-convergent except in kStageOne
  auto take = [&](bool on, int g, float stage, float prev) {
    const int b = on ? stage_bin(g, stage, G, S, err) : -1;
    const bool entered = A.prev != nullptr && prev != stage;
    if (MODE == kStageOne) {                                   // (b = the stage, < 16)
      const uint64_t one = b >= 0 ? 1ull << ((b & 7) * 8) : 0ull;
      const uint64_t lo = b < 8 ? one : 0ull, hi = one ^ lo, e = entered ? ~0ull : 0ull;
      occ_lo += lo, occ_hi += hi, ent_lo += lo & e, ent_hi += hi & e;
      return;
    }
    const bool differs = b >= 0 && b != run;
    if (__any(differs && run >= 0)) close_runs(differs);
    if (b < 0) return;
    run = b;
    ro += 1u;
    re += entered ? 1u : 0u;
  };
  // this workgroup's share, in units of four agents (vec4) or of one
  const int64_t units = A.vec4 ? (A.n >> 2) : A.n;
  const int64_t per = (units + gridDim.x - 1) / gridDim.x;
  const int64_t u0 = (int64_t)blockIdx.x * per, u1 = (u0 + per < units) ? u0 + per : units;
  for (int64_t base = u0; base < u1; base += blockDim.x) {     // (the same trip count for every lane of a wave)
    const int64_t i = base + threadIdx.x;
    const bool on = i < u1;
    if (A.vec4) {
      int4 g = make_int4(0, 0, 0, 0);
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f), p = s;
      if (on) {
        if (A.group) g = reinterpret_cast<const int4*>(A.group)[i];
        s = reinterpret_cast<const float4*>(A.stage)[i];
        if (A.prev) p = reinterpret_cast<const float4*>(A.prev)[i];
      }
      take(on, g.x, s.x, p.x);
      take(on, g.y, s.y, p.y);
      take(on, g.z, s.z, p.z);
      take(on, g.w, s.w, p.w);
    } else {
      take(on, (on && A.group) ? A.group[i] : 0, on ? A.stage[i] : 0.f, (on && A.prev) ? A.prev[i] : 0.f);
    }
  }
  if (A.vec4 && blockIdx.x == gridDim.x - 1 && threadIdx.x < kWave) {     // the n % 4 agents behind the last float4
    const int64_t a = (units << 2) + threadIdx.x;
    const bool on = a < A.n;
    take(on, (on && A.group) ? A.group[a] : 0, on ? A.stage[a] : 0.f, (on && A.prev) ? A.prev[a] : 0.f);
  }
  if (MODE == kStageOne) {
#pragma unroll
    for (int s = 0; s < GJ_MAX_STAGES; ++s) {
      if (s >= S) continue;                                    // (S is uniform: whole waves skip)
      const int sh = (s & 7) * 8;
      const uint32_t o = wave_sum<uint32_t>((uint32_t)((s < 8 ? occ_lo : occ_hi) >> sh) & 0xFFu);
      const uint32_t e = wave_sum<uint32_t>((uint32_t)((s < 8 ? ent_lo : ent_hi) >> sh) & 0xFFu);
      if (lane == 0) add(s, o, e);
    }
  } else {
    close_runs(true);
  }
  if (err) atomicOr(A.err, err);
  if (MODE != kStageGlobal) {
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * bins; i += blockDim.x) {
      const uint32_t v = stage_hist[i];
      if (v) atomicAdd(&A.out[i], (unsigned long long)v);
    }
  }
}

// adjoint of gj_stage_stats: a gather through (label, stage)
struct StageAdjArgs {
  int64_t n;
  const int32_t* group;
  const float* stage;
  const float* prev;
  const float* g_occ;
  const float* g_ent;
  float* grad_stage;
  int32_t n_groups, n_stages;
  int32_t vec4;
};

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_adjoint_stage_stats(const StageAdjArgs A) {
  extern __shared__ float stage_staged[];     // LDS: g_occ [bins], g_ent [bins]
  const int G = A.n_groups, S = A.n_stages, bins = G * S;
  const float* go = A.g_occ;
  const float* ge = A.g_ent;
  if (LDS) {
    for (int i = threadIdx.x; i < bins; i += blockDim.x) {
      stage_staged[i] = go ? go[i] : 0.0f;
      stage_staged[bins + i] = ge ? ge[i] : 0.0f;
    }
    __syncthreads();
    go = stage_staged;
    ge = stage_staged + bins;
  }
  // autograd of (stage == s) * stage / s, for the occupancy and (masked by the constant prev != stage) for the entries
  auto grad = [&](int g, float stage, float prev) {
    uint32_t unused = 0;
    const int b = stage_bin(g, stage, G, S, unused);
    if (b < 0 || stage == 0.0f) return 0.0f;
    float v = go ? go[b] / stage : 0.0f;
    if (A.prev && ge && prev != stage) v += ge[b] / stage;
    return v;
  };
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t first_scalar = 0;
  if (A.vec4) {
    const int64_t n4 = A.n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const int4 g = A.group ? reinterpret_cast<const int4*>(A.group)[i] : make_int4(0, 0, 0, 0);
      const float4 s = reinterpret_cast<const float4*>(A.stage)[i];
      const float4 p = A.prev ? reinterpret_cast<const float4*>(A.prev)[i] : s;
      reinterpret_cast<float4*>(A.grad_stage)[i] =
          make_float4(grad(g.x, s.x, p.x), grad(g.y, s.y, p.y), grad(g.z, s.z, p.z), grad(g.w, s.w, p.w));
    }
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < A.n; a += stride) {
    const float s = A.stage[a];
    A.grad_stage[a] = grad(A.group ? A.group[a] : 0, s, A.prev ? A.prev[a] : s);
  }
}

}  // namespace gj
