// Device-side helpers shared by the gfx950 kernels: wave64 reductions, Philox4x32-10, the
// per-agent Gumbel-softmax decision (a8), the infection state update (a9) and the transmission profile (a1).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gj {

constexpr int kWave = 64;          // CDNA wavefront
constexpr int kThreads = 256;      // 4 waves per workgroup: one per SIMD of a CU
constexpr int kEdgesPerThread = 8; // STREAM block = 2048 edges = GJ_STREAM_EDGES

// Sum over the lanes of an aligned group of G lanes (G = 4, 16, 64); every lane gets the total
// of ITS group.  Butterfly order: run-to-run deterministic.  T: float, double or uint64_t.
template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
// the whole wave: THE butterfly every wave-wide sum of the library goes through
template <typename T>
__device__ __forceinline__ T wave_sum(T v) { return group_sum<kWave>(v); }

// ---- Philox4x32-10 (Salmon et al., SC'11), counter = (pair lo, pair hi, step lo, step hi), key = seed.
// One call yields the two Exponential(1) draws of each agent of a pair (see exp_pair).
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#ifndef GJ_PHILOX_MULHI
  // one 32x32->64 product per word pair (v_mad_u64_u32) instead of a mul_hi + mul_lo pair: half the quarter-rate
  // integer multiplies, which are what the sampler costs
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
  const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
#else
  const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]);
  const uint32_t lo0 = 0xD2511F53u * c[0];
  const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]);
  const uint32_t lo1 = 0xCD9E8D57u * c[2];
#endif
  const uint32_t n0 = hi1 ^ c[1] ^ k0;
  const uint32_t n2 = hi0 ^ c[3] ^ k1;
  c[0] = n0;
  c[1] = lo1;
  c[2] = n2;
  c[3] = lo0;
}

__device__ __forceinline__ void philox4x32_10(uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key,
                                              uint32_t (&out)[4]) {
  uint32_t c[4] = {(uint32_t)ctr_lo, (uint32_t)(ctr_lo >> 32), (uint32_t)ctr_hi,
                   (uint32_t)(ctr_hi >> 32)};
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c[0];
  out[1] = c[1];
  out[2] = c[2];
  out[3] = c[3];
}

// 23 random bits -> uniform in (0,1): (k + 0.5) * 2^-23 for k < 2^23 is exactly representable in fp32 (24 significant
// bits), so the result is never 0 or 1 and -log(u) is finite and positive.  (With 24 bits the largest value,
// 16777215.5, rounds up to 2^24 and the draw becomes exactly 1: an Exponential draw of 0, once per ~1.7e7 draws -
// about once per step of a 10 M-agent world.)
__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-7f; }

// ---- the library's own noise for a8 (no reference draw to reproduce) ---------------------------------------------
// The reference draws two Exponential(1) variates (e0, e1) per agent and infects iff log(1-p) - log(e1) > log(p) -
// log(e0), i.e. iff p < e0 / (e0 + e1).  For two iid exponentials theta = e0 / (e0 + e1) is Uniform(0,1) and
// INDEPENDENT of s = e0 + e1 ~ Gamma(2,1).  So:
//   forward : theta = one 23-bit uniform; infected iff p < theta.  One Philox4x32-10 block (four words) serves the FOUR
//             agents 4k .. 4k+3 of GLOBAL ids (counter = agent >> 2) - a quarter of the integer multiplies that are the
//             sampler's cost, no logarithm, no division.
//   backward: the straight-through softmax needs both draws: e0 = theta * s, e1 = (1 - theta) * s with s = -log(u1 u2)
//             from a second block (counter = agent >> 1, stream bit 62 set) - the same joint law as two iid draws,
//             and by construction the same decision as the forward's.
__device__ __forceinline__ float infection_uniform_from_block(const uint32_t (&r)[4], int which) {
  return u01(which == 0 ? r[0] : (which == 1 ? r[1] : (which == 2 ? r[2] : r[3])));
}
__device__ __forceinline__ float infection_uniform(uint64_t seed, uint64_t step, int64_t agent) {
  uint32_t r[4];
  philox4x32_10((uint64_t)agent >> 2, step, seed, r);
  return infection_uniform_from_block(r, (int)(agent & 3));
}
__device__ __forceinline__ float own_new_infected(float p, float theta) { return (p < theta) ? 1.0f : 0.0f; }
// (e0, e1) with e0 / (e0 + e1) == theta up to rounding: what k_adjoint_sample feeds the softmax derivative
__device__ __forceinline__ void exp_pair_parts(uint64_t seed, uint64_t step, int64_t agent, float& theta, float& s) {
  theta = infection_uniform(seed, step, agent);
  uint32_t r[4];
  philox4x32_10((uint64_t)agent >> 1, step | (1ull << 62), seed, r);
  const float u1 = u01((agent & 1) ? r[2] : r[0]), u2 = u01((agent & 1) ? r[3] : r[1]);
  s = -logf(u1) - logf(u2);
}
__device__ __forceinline__ void exp_pair(uint64_t seed, uint64_t step, int64_t agent, float& e0, float& e1) {
  float theta, s;
  exp_pair_parts(seed, step, agent, theta, s);
  e0 = theta * s;
  e1 = (1.0f - theta) * s;
}
// The same pair with the two products formed in fp64, where they are exact (24 x 24 bits; 1 - theta is exact in fp32):
// e0 / e1 == theta / (1 - theta) to fp64 rounding, so the softmax terms - which see the draws through log e0 - log e1
// only - do not depend on the last bit of logf in s.
__device__ __forceinline__ void exp_pair(uint64_t seed, uint64_t step, int64_t agent, double& e0, double& e1) {
  float theta, s;
  exp_pair_parts(seed, step, agent, theta, s);
  e0 = (double)theta * (double)s;
  e1 = (double)(1.0f - theta) * (double)s;
}

// a8: IsInfectedSampler.forward = F.gumbel_softmax(vstack(p, 1-p).log(), tau=0.1, hard=True, dim=0)
// (reference grad_june/infection.py:13-18).  e0/e1 are the Exponential(1) draws of rows 0/1.
// Returns the forward value 1 - (y_hard - y_soft + y_soft)[0], computed op for op.
__device__ __forceinline__ float gumbel_new_infected(float p, float e0, float e1) {
  const float l0 = logf(p);
  const float l1 = logf(1.0f - p);
  const float z0 = (l0 + (-logf(e0))) / 0.1f;
  const float z1 = (l1 + (-logf(e1))) / 0.1f;
  const float m = fmaxf(z0, z1);
  const float x0 = expf(z0 - m);
  const float x1 = expf(z1 - m);
  const float s = x0 + x1;
  const float y0 = x0 / s;
  const float y1 = x1 / s;
  const float h0 = (y1 > y0) ? 0.0f : 1.0f;  // argmax, ties -> row 0 (not infected)
  const float ret0 = (h0 - y0) + y0;
  return 1.0f - ret0;
}

// a9: GradJune.infect_people (reference grad_june/model.py:103-110).  torch.maximum passes a NaN through where fmaxf
// would swallow it: a NaN new_infected (a NaN probability, an injected draw of 0) or a NaN susceptibility leaves the
// susceptibility NaN like is_infected and infection_time, not 0.
__device__ __forceinline__ void infect(float nw, float now, float& susc, float& inf, float& t_inf) {
  const float x = susc - nw;
  susc = (x != x) ? x : fmaxf(0.0f, x);
  inf = inf + nw;
  t_inf = t_inf + nw * (now - t_inf);
}

// Adjoint of a8 + a9 for one agent, shared by k_adjoint_sample (a hot-path step, T = float) and k_adjoint_seed_agents
// (the seed, T = double): four pieces.
//  sampler_draws:    agent a's columns of `noise` ([2, n]) or, without it, exp_pair(seed, step, agent_offset + a)
//  sampler_decision: the decision nu the FORWARD took - in its arithmetic (fp32), by its rule: the argmax of the
//                    tau = 0.1 softmax for injected draws, p < theta for the library's own
//  sampler_softmax:  y0, y1 of the straight-through sampler's forward, in T
//  sample_adjoint:   given p (the probability of NOT being infected), the pre-state, y0, y1, nu and the gradients w.r.t.
//                    the outputs: h, the subgradient of max(0, susceptibility - nu) (a tie splits the gradient),
//                    nu_bar = d loss / d new_infected = g_inf + g_time * (now - time0) - g_susc * h + g_new
//                    and the straight-through derivative d nu / d p of the softmax
__device__ __forceinline__ float gj_log(float x) { return logf(x); }
__device__ __forceinline__ double gj_log(double x) { return log(x); }
__device__ __forceinline__ float gj_exp(float x) { return expf(x); }
__device__ __forceinline__ double gj_exp(double x) { return exp(x); }
__device__ __forceinline__ float gj_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double gj_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float gj_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double gj_abs(double x) { return fabs(x); }

template <typename T>
__device__ __forceinline__ void sampler_draws(const float* __restrict__ noise, int64_t n, int64_t a, uint64_t seed,
                                              uint64_t step, int64_t agent_offset, T& e0, T& e1) {
  if (noise) {
    e0 = noise[a];
    e1 = noise[n + a];
  } else {
    exp_pair(seed, step, agent_offset + a, e0, e1);
  }
}

// y0, y1 of the straight-through sampler's forward (same op sequence as gumbel_new_infected)
template <typename T>
__device__ __forceinline__ void sampler_softmax(T p, T e0, T e1, T& y0, T& y1) {
  const T tau = (T)0.1;
  const T z0 = (gj_log(p) + (-gj_log(e0))) / tau;
  const T z1 = (gj_log((T)1 - p) + (-gj_log(e1))) / tau;
  const T m = gj_max(z0, z1);
  const T x0 = gj_exp(z0 - m), x1 = gj_exp(z1 - m);
  y0 = x0 / (x0 + x1);
  y1 = x1 / (x0 + x1);
}

// (y0, y1: the FLOAT softmax terms; read for injected draws only)
__device__ __forceinline__ float sampler_decision(float p, bool injected, float y0, float y1, uint64_t seed,
                                                  uint64_t step, int64_t agent) {
  return injected ? ((y1 > y0) ? 1.0f : 0.0f)                                          // the forward's rule
                  : own_new_infected(p, infection_uniform(seed, step, agent));
}

template <typename T>
struct SampleAdjoint {
  T h, nu_bar, dnu_dp;
};
template <typename T>
__device__ __forceinline__ SampleAdjoint<T> sample_adjoint(T p, T s0, T t0, T y0, T y1, T nu, T now, T gs, T gi, T gt,
                                                           T gn) {
  SampleAdjoint<T> r;
  const T x = s0 - nu;                                       // torch.maximum(0, x): tie splits the gradient
  r.h = (x > (T)0) ? (T)1 : ((x == (T)0) ? (T)0.5 : (T)0);
  r.nu_bar = gi + gt * (now - t0) - gs * r.h + gn;
  r.dnu_dp = -(y0 * y1 / (T)0.1) * ((T)1 / p + (T)1 / ((T)1 - p));
  if (!(gj_abs(r.dnu_dp) < (T)3.0e38f)) r.dnu_dp = (T)0;     // p == 0 or 1: y0*y1 == 0 there
  return r;
}

// a7 (reference base.py:136-140): p = clamp(exp(-clamp(ts, 1e-6, 100) * dt), 0, 1).  torch.clamp passes a NaN
// through; fminf / fmaxf would swallow it (and turn a poisoned agent into "never infected").
__device__ __forceinline__ float clamp_keep_nan(float x, float lo, float hi) {
  return (x != x) ? x : fminf(fmaxf(x, lo), hi);
}
__device__ __forceinline__ float not_infected_prob(float ts, float dt) {
  return clamp_keep_nan(expf(-clamp_keep_nan(ts, 1e-6f, 100.0f) * dt), 0.0f, 1.0f);
}

__device__ __forceinline__ float sgnf(float x) { return (float)((0.0f < x) - (x < 0.0f)); }

// ---- a1: the transmission profile (reference grad_june/transmission.py:39-51) -----------------------------------
// The profile's transcendental part, exp(-lgamma(shape)) * pow(x, shape - 1) * exp(e), costs ~690 instructions with
// libm's lgammaf (~420) and powf (~200) - and a wave pays them for all 64 lanes whenever one lane holds an infected
// agent, which made k_transmission arithmetic-bound at the 5-25 % prevalence of the timed steps.  Round 3:
//   1 / Gamma(shape)  by the recurrence to [1, 2] and Abramowitz & Stegun 6.1.36 (degree 8, |eps| <= 3e-7 there; measured
//                     3.5e-7 relative in fp32), libm only for shapes outside (0.25, 16);
//   pow(x, y)         = exp2(y * log2(x)) on the hardware's v_log_f32 / v_exp_f32 (1 ulp each): the error of the
//                     exponent, |y log2 x| * 2^-23, is ~1e-6 relative in the result; 0 / inf at x == 0 as powf; x < 0: NaN for a
//                     non-integer y and +-|x|^y for an integer one, as powf / torch.pow;
//   exp(e)            = exp2(e * log2(e)): ~|e| * 1e-7.
// Together ~2e-6 relative against the reference's fp32 torch ops (themselves ~1e-7); the parity tests hold the
// transmissions to 2e-5.  ~60 instructions.
__device__ __forceinline__ float inv_gamma(float x) {
  if (!(x > 0.25f && x < 16.0f)) return expf(-lgammaf(x));        // (also NaN)
  float up = 1.0f, down = 1.0f;           // Gamma(x_in) = Gamma(x) * up / down
  while (x > 2.0f) {
    x -= 1.0f;
    up *= x;
  }
  while (x < 1.0f) {
    down *= x;
    x += 1.0f;
  }
  const float z = x - 1.0f;
  float g = 0.035868343f;
  g = g * z - 0.193527818f;
  g = g * z + 0.482199394f;
  g = g * z - 0.756704078f;
  g = g * z + 0.918206857f;
  g = g * z - 0.897056937f;
  g = g * z + 0.988205891f;
  g = g * z - 0.577191652f;
  g = g * z + 1.0f;                       // Gamma(1 + z), 0 <= z <= 1
  return down / (g * up);
}
__device__ __forceinline__ float fast_pow(float x, float y) {
  if (y == 0.0f) return 1.0f;             // powf(x, 0) == 1 for every x
  if (x < 0.0f) {
    // torch.pow / powf of a negative base: finite for an INTEGER exponent (sign by its parity), NaN otherwise.  A
    // constant integer shape with t < shift is the case that matters (transmission.py:45-49: sign == 0 there, and
    // 0 * finite == 0 where 0 * NaN would poison the venue sums).  Rare: not worth libm's powf in the
    // instruction stream of a launch that lives on its occupancy.
    const float yi = truncf(y);
    if (yi != y) return __builtin_nanf("");
    const float r = __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(-x));
    const float h = 0.5f * yi;
    return (truncf(h) != h) ? -r : r;     // odd exponent: the base's sign survives
  }
  return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x));      // v_exp_f32(y * v_log_f32(x))
}
// v_exp_f32 flushes a subnormal RESULT to 0 where expf underflows gradually.  Alone that is an absolute error below
// 2^-126; but next to a pow that has overflowed (shape 28, d * rate = 100: pow(100, 27) = inf, exp(-100) = 3.8e-44) it
// turns the reference's inf * 3.8e-44 = inf into inf * 0 = NaN.  Below 2^-126 the result is therefore taken as
// exp2(x + 32) * 2^-32 (the product is an ordinary multiply, which keeps subnormals); above, the multiply by 1 changes no bit.
__device__ __forceinline__ float fast_exp(float e) {
  const float x = e * 1.44269504088896341f;
  const bool tiny = x < -126.0f;
  return __builtin_amdgcn_exp2f(tiny ? x + 32.0f : x) * (tiny ? 2.3283064365386963e-10f : 1.0f);
}

// The head of the profile, shared by the update and its adjoints (which must give the update's bits):
// transmission = max_infectiousness * sign * aux * aux2 * is_infected, with t the time since infection and d = t - shift.
struct ProfileHead {
  float sign, aux, aux2, d, t;
};
__device__ __forceinline__ ProfileHead profile_head(float shp, float rt, float sh, float t_inf, float now) {
  ProfileHead h;
  h.t = now - t_inf;
  h.d = h.t - sh;
  h.sign = (sgnf(h.d + 1e-10f) + 1.0f) / 2.0f;
  h.aux = inv_gamma(shp) * fast_pow(h.d * rt, shp - 1.0f);
  h.aux2 = fast_exp((sh - h.t) * rt) * rt;
  return h;
}

}  // namespace gj
