// Contact quarantine (include/gradjune_hip.h, gj_contact_mark / gj_contact_mask): two stand-alone kernels that run BEFORE
// the step and hand it a per-agent mask in the place of current_stage.  Nothing of gj_tiled.h is involved.
//   mark: every index agent (!(stage < threshold)) raises until[v] of its venues in the traced sets to the launch's
//         release time.  The times are fp32 bit patterns of non-negative values, for which the unsigned integer order is
//         the float order: the max is an integer atomicMax - exact, and no order of the agents shows.
//   mask: qstate[a] = 1 for an index agent, 2 for a complying agent one of whose traced venues is still marked
//         (float(until[v]) > now), else 0.  The compliance uniform is the vaccination's kind of draw: one per agent for
//         the run, infection_uniform(seed, stream, global id).
// The lane that owns an agent walks its rows (a household row holds 1 to 5 edges); where a lane holds four agents the
// mask walks their rows as one range of the edge list (contact_mask_quad).  Both kernels read the stage coalesced, four
// agents per lane where the arrays are 16-byte aligned, and give the same bits in either form.  A row pointer or venue
// id outside its set is skipped - never an index - and sets kContactBadRows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gradjune_hip.h"
#include "gj_device.h"
#include "gj_agent.h"

namespace gj {

constexpr uint32_t kContactBadRows = GJ_CONTACT_ERR_ROWS;
constexpr int kContactBlocks = 2048;

struct ContactSet {
  const int32_t* rowptr;       // [n + 1]
  const int32_t* venue;        // [rowptr[n]]
  uint32_t* until;             // [n_venues]
  int32_t n_venues;
  uint32_t release;            // bits of the launch's fp32 release time (mark only)
};

// ONE definition of the index rule, the hot path's own: a NaN stage is an index case
__device__ __forceinline__ bool contact_index(float stage, float threshold) { return !(stage < threshold); }

// agent a's row of set S, checked against the set's edge count rowptr[n]: false (and the error bit) for a row outside it
__device__ __forceinline__ bool contact_row(const ContactSet& S, int64_t n, int64_t a, int32_t& r0, int32_t& r1,
                                            uint32_t& err) {
  r0 = S.rowptr[a], r1 = S.rowptr[a + 1];
  const int32_t n_edges = S.rowptr[n];
  if (r0 < 0 || r1 < r0 || r1 > n_edges) {
    err |= kContactBadRows;
    return false;
  }
  return true;
}

struct ContactMarkArgs {
  int64_t n;
  const float* stage;
  uint32_t* err;
  float threshold;
  int32_t n_sets;
  int32_t vec4;                // stage 16-byte aligned
  ContactSet sets[GJ_MAX_SETS];
};

__device__ __forceinline__ void contact_mark_agent(const ContactMarkArgs& A, int64_t a, uint32_t& err) {
  for (int s = 0; s < A.n_sets; ++s) {
    const ContactSet& S = A.sets[s];
    int32_t r0, r1;
    if (!contact_row(S, A.n, a, r0, r1, err)) continue;
    for (int32_t e = r0; e < r1; ++e) {
      const int32_t v = S.venue[e];
      if ((uint32_t)v >= (uint32_t)S.n_venues) { err |= kContactBadRows; continue; }
      atomicMax(&S.until[v], S.release);       // (result unused: a fire-and-forget integer max)
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_contact_mark(const ContactMarkArgs A) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t lane0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t err = 0;
  int64_t first_scalar = 0;
  if (A.vec4) {
    const int64_t n4 = A.n >> 2;
    for (int64_t i = lane0; i < n4; i += stride) {
      const float4 st = reinterpret_cast<const float4*>(A.stage)[i];
      if (contact_index(st.x, A.threshold)) contact_mark_agent(A, 4 * i, err);
      if (contact_index(st.y, A.threshold)) contact_mark_agent(A, 4 * i + 1, err);
      if (contact_index(st.z, A.threshold)) contact_mark_agent(A, 4 * i + 2, err);
      if (contact_index(st.w, A.threshold)) contact_mark_agent(A, 4 * i + 3, err);
    }
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + lane0; a < A.n; a += stride)
    if (contact_index(A.stage[a], A.threshold)) contact_mark_agent(A, a, err);
  if (err) atomicOr(A.err, err);
}

struct ContactMaskArgs {
  int64_t n;
  const float* stage;
  float* qstate;
  uint32_t* err;
  uint64_t seed, stream;
  int64_t agent_offset;
  float threshold, now, compliance;
  int32_t n_sets;
  int32_t vec4;                // agent_offset % 4 == 0 and stage, qstate 16-byte aligned
  ContactSet sets[GJ_MAX_SETS];
};

// whether a venue of agent a's row in set S is still marked at `now` (the whole row: what the error word reports depends
// on no order)
__device__ __forceinline__ bool contact_row_held(const ContactSet& S, int64_t n, int64_t a, float now, uint32_t& err) {
  int32_t r0, r1;
  if (!contact_row(S, n, a, r0, r1, err)) return false;
  bool held = false;
  for (int32_t e = r0; e < r1; ++e) {
    const int32_t v = S.venue[e];
    if ((uint32_t)v >= (uint32_t)S.n_venues) { err |= kContactBadRows; continue; }
    held |= __uint_as_float(S.until[v]) > now;
  }
  return held;
}

// one agent's state from its stage and its compliance uniform; only a complying agent that is no index case walks rows
__device__ __forceinline__ float contact_mask_agent(const ContactMaskArgs& A, int64_t a, float stage, float u,
                                                    uint32_t& err) {
  if (contact_index(stage, A.threshold)) return 1.0f;
  if (!(u < A.compliance)) return 0.0f;
  bool held = false;
  for (int s = 0; s < A.n_sets; ++s) held |= contact_row_held(A.sets[s], A.n, a, A.now, err);
  return held ? 2.0f : 0.0f;
}

// The quad form of the walk.  Agent by agent, a lane that holds four agents goes through twelve dependent loads (row
// pointers -> venue id -> until, four times over), and the launch is bound by that chain, not by bytes.  The rows of
// four consecutive agents are one contiguous range of the set's edge list, so the lane walks the range [rp[0], rp[4])
// kContactBatch edges at a time - the batch's venue ids are loaded together, then its until words - and credits an
// edge to the agent whose row holds it.  Edges of agents that walk no row are not loaded.  A quad whose five row
// pointers are not 0 <= rp[0] <= .. <= rp[4] <= edges falls back to the agent-by-agent walk, which skips and reports
// the bad rows of its walkers one by one; the result is the same bits either way.
constexpr int kContactBatch = 8;

__device__ __forceinline__ float4 contact_mask_quad(const ContactMaskArgs& A, int64_t i, const float4 st,
                                                    const float (&u)[4], uint32_t& err) {
  const float stage[4] = {st.x, st.y, st.z, st.w};
  bool index[4], walk[4], held[4];
  bool any = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    index[j] = contact_index(stage[j], A.threshold);
    walk[j] = !index[j] && u[j] < A.compliance;
    held[j] = false;
    any |= walk[j];
  }
  if (any) {
    for (int s = 0; s < A.n_sets; ++s) {
      const ContactSet& S = A.sets[s];
      int32_t rp[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) rp[j] = S.rowptr[4 * i + j];
      const int32_t n_edges = S.rowptr[A.n];
      if (rp[0] < 0 || rp[1] < rp[0] || rp[2] < rp[1] || rp[3] < rp[2] || rp[4] < rp[3] || rp[4] > n_edges) {
#pragma unroll
        for (int j = 0; j < 4; ++j)                  // the agent-by-agent walk of this set alone
          if (walk[j]) held[j] |= contact_row_held(S, A.n, 4 * i + j, A.now, err);
        continue;
      }
      for (int64_t base = rp[0]; base < rp[4]; base += kContactBatch) {
        int32_t v[kContactBatch];
        int owner[kContactBatch];
        bool on[kContactBatch];
#pragma unroll
        for (int k = 0; k < kContactBatch; ++k) {
          const int64_t e = base + k;
          owner[k] = (int)(e >= rp[1]) + (int)(e >= rp[2]) + (int)(e >= rp[3]);
          on[k] = e < rp[4] && ((owner[k] == 0 && walk[0]) || (owner[k] == 1 && walk[1]) ||
                                (owner[k] == 2 && walk[2]) || (owner[k] == 3 && walk[3]));
          v[k] = on[k] ? S.venue[e] : 0;
        }
        uint32_t t[kContactBatch];
#pragma unroll
        for (int k = 0; k < kContactBatch; ++k) {
          const bool inside = (uint32_t)v[k] < (uint32_t)S.n_venues;
          if (on[k] && !inside) err |= kContactBadRows;
          on[k] = on[k] && inside;
          t[k] = on[k] ? S.until[v[k]] : 0u;
        }
#pragma unroll
        for (int k = 0; k < kContactBatch; ++k) {
          const bool hit = on[k] && __uint_as_float(t[k]) > A.now;
#pragma unroll
          for (int j = 0; j < 4; ++j) held[j] |= hit && owner[k] == j;
        }
      }
    }
  }
  float q[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = index[j] ? 1.0f : (held[j] ? 2.0f : 0.0f);
  return make_float4(q[0], q[1], q[2], q[3]);
}

__global__ __launch_bounds__(kThreads) void k_contact_mask(const ContactMaskArgs A) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t lane0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t err = 0;
  int64_t first_scalar = 0;
  if (A.vec4) {
    const int64_t n4 = A.n >> 2;
    for (int64_t i = lane0; i < n4; i += stride) {
      const float4 st = reinterpret_cast<const float4*>(A.stage)[i];
      float u[4];
      vaccine_uniforms4(A.seed, A.stream, A.agent_offset + 4 * i, u);      // one Philox block serves the quad
      reinterpret_cast<float4*>(A.qstate)[i] = contact_mask_quad(A, i, st, u, err);
    }
    first_scalar = n4 << 2;
  }
  for (int64_t a = first_scalar + lane0; a < A.n; a += stride)
    A.qstate[a] = contact_mask_agent(A, a, A.stage[a], infection_uniform(A.seed, A.stream, A.agent_offset + a), err);
  if (err) atomicOr(A.err, err);
}

}  // namespace gj
