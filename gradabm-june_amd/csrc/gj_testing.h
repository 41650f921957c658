// Testing (include/gradjune_hip.h, gj_testing_step / gj_adjoint_testing): one stand-alone per-agent launch BEFORE the
// step, on the stage the step starts from.  Nothing of gj_tiled.h is involved.
//   decide: an agent at or above the threshold whose infection has not been decided yet draws ONE Philox block of its
//           own - counter = global id, stream | bits(infection_time), key = seed - for whether the infection is found
//           (word 0 against the age's probability) and after how many days (word 1 against the cumulative shares).
//   report: a result that is due is taken off (result_time = +inf); a positive one is a confirmed case, and a complying
//           agent of an isolating policy stays away until `release`.
//   mask:   qstate[a] = 1 for !(stage < q_threshold), else 3 while now < isolate_until, else 0 - what the step then takes
//           in the place of the stage with the threshold 0.5, as it takes gj_contact_mask's.
// Most agents neither decide nor report: their lanes read the stage, the infection time, `decided`, `result_time` and the
// class, and write nothing but the optional per-agent outputs.  The rare paths - `positive`, `confirmed_time`,
// `isolate_until` - go through scalar loads and stores of the one agent.  Four agents per lane where the arrays are
// 16-byte aligned, one per lane otherwise; both forms call ONE per-agent function and give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gradjune_hip.h"
#include "gj_device.h"
#include "gj_agent.h"

namespace gj {

constexpr uint32_t kTestDecided = GJ_TESTING_DECIDED, kTestPositive = GJ_TESTING_POSITIVE, kTestDue = GJ_TESTING_DUE;
constexpr int kTestProb = 0, kTestCum = kVaccineAges, kTestDays = kVaccineAges + GJ_TESTING_MAX_DELAYS;
constexpr int kTestTable = kVaccineAges + 2 * GJ_TESTING_MAX_DELAYS;
static_assert(sizeof(gj_testing_tables) == (kTestTable + 2) * sizeof(float), "gj_testing_tables: three packed tables");

struct TestingArgs {
  gj_testing_tables T;
  int64_t n;
  const uint8_t* cls;
  const float* stage;
  const float* inf_time;
  uint32_t* decided;
  float* result_time;
  float* positive;
  float* isolate_until;        // [n], or NULL for a policy that does not isolate
  float* confirmed_time;
  float* newly;                // [n] or NULL
  float* qstate;               // [n] or NULL
  uint8_t* flags;              // [n] or NULL
  unsigned long long* counts;  // [2] or NULL: newly confirmed, decisions
  uint64_t seed, decide_stream, comply_stream;
  int64_t agent_offset;
  float threshold, q_threshold, now, release, compliance;
  int32_t active;
  int32_t vec4;                // the 4-byte arrays given 16-byte, cls and flags 4-byte aligned
};

// tab = probability | cumulative shares | days; ends with a barrier
__device__ __forceinline__ void testing_stage_tables(const gj_testing_tables& T, float* tab) {
  const float* src = reinterpret_cast<const float*>(&T);
  for (int i = threadIdx.x; i < kTestTable; i += blockDim.x) tab[i] = src[i];
  __syncthreads();
}

// ONE definition of the rule.  `dec`, `rt` and `iso` are the agent's loaded values and leave as its new ones; the caller
// stores dec where kTestDecided and rt where kTestDecided or kTestDue came back.  `iso` is read only under a mask.
__device__ __forceinline__ uint32_t testing_agent(const TestingArgs& A, const float* tab, int n_delays, int64_t a, int cls,
                                                  float stage, float it, uint32_t& dec, float& rt, float& iso) {
  uint32_t flags = 0;
  float pos = 0.0f;
  const uint32_t bits = __float_as_uint(it);
  if (A.active && !(stage < A.threshold) && bits != dec) {
    dec = bits;
    flags |= kTestDecided;
    uint32_t r[4];
    philox4x32_10((uint64_t)(A.agent_offset + a), A.decide_stream | bits, A.seed, r);
    pos = (u01(r[0]) < tab[kTestProb + cls % kVaccineAges]) ? 1.0f : 0.0f;
    const float u = u01(r[1]);
    int k = n_delays - 1;      // the last entry takes the remainder
    for (int j = 0; j < n_delays - 1; ++j)
      if (tab[kTestCum + j] > u) {
        k = j;
        break;
      }
    rt = A.now + tab[kTestDays + k];
    A.positive[a] = pos;
  }
  if (rt <= A.now) {
    if (!(flags & kTestDecided)) pos = A.positive[a];
    rt = __builtin_inff();
    flags |= kTestDue;
    if (pos != 0.0f) {
      A.confirmed_time[a] = A.now;
      if (A.isolate_until && infection_uniform(A.seed, A.comply_stream, A.agent_offset + a) < A.compliance) {
        A.isolate_until[a] = A.release;
        iso = A.release;
      }
    }
  }
  if (pos != 0.0f) flags |= kTestPositive;
  return flags;
}

__device__ __forceinline__ float testing_mask(const TestingArgs& A, float stage, float iso) {
  return !(stage < A.q_threshold) ? 1.0f : ((A.now < iso) ? 3.0f : 0.0f);
}
__device__ __forceinline__ bool testing_confirmed(uint32_t f) { return (f & (kTestDue | kTestPositive)) == (kTestDue | kTestPositive); }

// k_vaccinate's shape: workgroups of 1024 lanes, at most 512 of them, one integer atomic per count and workgroup.
__global__ __launch_bounds__(kVaccineThreads) void k_testing_step(const TestingArgs A) {
  __shared__ float tab[kTestTable];
  __shared__ uint32_t part_c[kVaccineThreads / kWave], part_d[kVaccineThreads / kWave];
  testing_stage_tables(A.T, tab);
  const int n_delays = A.T.n_delays;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool mask = A.qstate != nullptr;
  uint32_t confirmed = 0, decisions = 0;      // (a lane meets n / (lanes of the grid) agents: far below 2^32)
  int64_t first_scalar = 0;
  if (A.vec4) {
    const int64_t n4 = A.n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const uint32_t cl = reinterpret_cast<const uint32_t*>(A.cls)[i];
      const float4 st = reinterpret_cast<const float4*>(A.stage)[i];
      const float4 it = reinterpret_cast<const float4*>(A.inf_time)[i];
      uint4 dc = reinterpret_cast<const uint4*>(A.decided)[i];
      float4 rt = reinterpret_cast<const float4*>(A.result_time)[i];
      float4 iso = make_float4(0.f, 0.f, 0.f, 0.f);
      if (mask && A.isolate_until) iso = reinterpret_cast<const float4*>(A.isolate_until)[i];
      const uint32_t f0 = testing_agent(A, tab, n_delays, 4 * i, (int)(cl & 0xFF), st.x, it.x, dc.x, rt.x, iso.x);
      const uint32_t f1 = testing_agent(A, tab, n_delays, 4 * i + 1, (int)((cl >> 8) & 0xFF), st.y, it.y, dc.y, rt.y, iso.y);
      const uint32_t f2 = testing_agent(A, tab, n_delays, 4 * i + 2, (int)((cl >> 16) & 0xFF), st.z, it.z, dc.z, rt.z, iso.z);
      const uint32_t f3 = testing_agent(A, tab, n_delays, 4 * i + 3, (int)(cl >> 24), st.w, it.w, dc.w, rt.w, iso.w);
      const uint32_t any = f0 | f1 | f2 | f3;
      if (any & kTestDecided) reinterpret_cast<uint4*>(A.decided)[i] = dc;
      if (any & (kTestDecided | kTestDue)) reinterpret_cast<float4*>(A.result_time)[i] = rt;
      const bool c0 = testing_confirmed(f0), c1 = testing_confirmed(f1), c2 = testing_confirmed(f2), c3 = testing_confirmed(f3);
      if (A.newly)
        reinterpret_cast<float4*>(A.newly)[i] =
            make_float4(c0 ? 1.0f : 0.0f, c1 ? 1.0f : 0.0f, c2 ? 1.0f : 0.0f, c3 ? 1.0f : 0.0f);
      if (mask)
        reinterpret_cast<float4*>(A.qstate)[i] = make_float4(testing_mask(A, st.x, iso.x), testing_mask(A, st.y, iso.y),
                                                             testing_mask(A, st.z, iso.z), testing_mask(A, st.w, iso.w));
      if (A.flags) reinterpret_cast<uint32_t*>(A.flags)[i] = f0 | f1 << 8 | f2 << 16 | f3 << 24;
      confirmed += (uint32_t)c0 + (uint32_t)c1 + (uint32_t)c2 + (uint32_t)c3;
      decisions += (f0 & kTestDecided) + (f1 & kTestDecided) + (f2 & kTestDecided) + (f3 & kTestDecided);
    }
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < A.n; a += stride) {
    const float stage = A.stage[a];
    uint32_t dc = A.decided[a];
    float rt = A.result_time[a];
    float iso = (mask && A.isolate_until) ? A.isolate_until[a] : 0.0f;
    const uint32_t f = testing_agent(A, tab, n_delays, a, (int)A.cls[a], stage, A.inf_time[a], dc, rt, iso);
    if (f & kTestDecided) A.decided[a] = dc;
    if (f & (kTestDecided | kTestDue)) A.result_time[a] = rt;
    const bool c = testing_confirmed(f);
    if (A.newly) A.newly[a] = c ? 1.0f : 0.0f;
    if (mask) A.qstate[a] = testing_mask(A, stage, iso);
    if (A.flags) A.flags[a] = (uint8_t)f;
    confirmed += (uint32_t)c;
    decisions += f & kTestDecided;
  }
  // the workgroup's counts: a wave sum, the waves' sums through LDS, one integer atomic per count where it is not zero
  confirmed = wave_sum(confirmed);
  decisions = wave_sum(decisions);
  if (threadIdx.x % kWave == 0) {
    part_c[threadIdx.x / kWave] = confirmed;
    part_d[threadIdx.x / kWave] = decisions;
  }
  __syncthreads();
  if (threadIdx.x == 0 && A.counts) {
    unsigned long long c = 0, d = 0;
    for (int w = 0; w < kVaccineThreads / kWave; ++w) {
      c += part_c[w];
      d += part_d[w];
    }
    if (c) atomicAdd(&A.counts[0], c);
    if (d) atomicAdd(&A.counts[1], d);
  }
}

// The adjoint's per-agent launch: the cotangent an agent's y receives - from the later launches (g_y) and, where its
// result fell due in this one, from the row (g_row) - goes to the probability of its band and to its stage where the
// launch decided it, and back to the incoming y where it did not.  The per-band sums go through the seed's two summing
// kernels (k_adjoint_seed_chunks, k_adjoint_seed_finish) in the order of the band's gj_seed_plan.
struct TestingAdjArgs {
  int64_t n;
  const uint8_t* flags;
  const float* stage;
  const float* g_y;            // [n] or NULL (zeros)
  const float* g_row;          // [1] or NULL (zero)
  const int32_t* band;         // [n]
  int32_t n_bands;
  int32_t vec4;                // every array given 16-byte (flags: 4-byte) aligned
  double* contrib;             // [n]
  float* g_stage;              // [n] or NULL
  float* g_y_in;               // [n] or NULL
};

// y = hard * stage / stage.detach() where decided: d y / d stage = hard / stage, d y / d probability[band] := 1 (the
// straight-through estimator).  A label outside [0, n_bands) is no band: no term, never an index.
__device__ __forceinline__ void testing_adjoint_agent(uint32_t flag, float stage, float gy, float grow, int32_t band,
                                                      int32_t n_bands, double& c, float& gs, float& gy_in) {
  const float g = gy + ((flag & kTestDue) ? grow : 0.0f);
  const bool decided = (flag & kTestDecided) != 0;
  const float hard = (flag & kTestPositive) ? 1.0f : 0.0f;
  c = (decided && (uint32_t)band < (uint32_t)n_bands) ? (double)g : 0.0;
  gs = decided ? g * hard / stage : 0.0f;
  gy_in = decided ? 0.0f : g;
}

__global__ __launch_bounds__(kThreads) void k_adjoint_testing(const TestingAdjArgs A) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float grow = A.g_row ? A.g_row[0] : 0.0f;
  int64_t first_scalar = 0;
  if (A.vec4) {
    const int64_t n4 = A.n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const uint32_t fl = reinterpret_cast<const uint32_t*>(A.flags)[i];
      const float4 st = reinterpret_cast<const float4*>(A.stage)[i];
      const float4 gy = A.g_y ? reinterpret_cast<const float4*>(A.g_y)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      const int4 b = reinterpret_cast<const int4*>(A.band)[i];
      double c0, c1, c2, c3;
      float4 gs, gi;
      testing_adjoint_agent(fl & 0xFF, st.x, gy.x, grow, b.x, A.n_bands, c0, gs.x, gi.x);
      testing_adjoint_agent((fl >> 8) & 0xFF, st.y, gy.y, grow, b.y, A.n_bands, c1, gs.y, gi.y);
      testing_adjoint_agent((fl >> 16) & 0xFF, st.z, gy.z, grow, b.z, A.n_bands, c2, gs.z, gi.z);
      testing_adjoint_agent(fl >> 24, st.w, gy.w, grow, b.w, A.n_bands, c3, gs.w, gi.w);
      reinterpret_cast<double2*>(A.contrib)[2 * i] = make_double2(c0, c1);
      reinterpret_cast<double2*>(A.contrib)[2 * i + 1] = make_double2(c2, c3);
      if (A.g_stage) reinterpret_cast<float4*>(A.g_stage)[i] = gs;
      if (A.g_y_in) reinterpret_cast<float4*>(A.g_y_in)[i] = gi;
    }
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < A.n; a += stride) {
    double c;
    float gs, gi;
    testing_adjoint_agent(A.flags[a], A.stage[a], A.g_y ? A.g_y[a] : 0.0f, grow, A.band[a], A.n_bands, c, gs, gi);
    A.contrib[a] = c;
    if (A.g_stage) A.g_stage[a] = gs;
    if (A.g_y_in) A.g_y_in[a] = gi;
  }
}

}  // namespace gj
