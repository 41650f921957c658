/*
 * gradjune_hip.h - C ABI of the MI355X (gfx950) infection message-passing library.
 *
 * This is the drop-in boundary for ONE path of GradABM-JUNE: the per-timestep infection
 * step.  The reference has no native code and no FFI for this path:
 * it runs as eager PyTorch + torch_geometric ops on the CPU.  Each entry point below
 * therefore names the reference PYTHON interface it replaces (paths relative to the
 * reference tree, file:line) - these are the call sites a maintainer re-binds with the
 * ctypes stub shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  No torch types, no C++ types.
 *   - Every pointer marked "device" is a HIP device pointer valid on the current device.
 *     Every buffer (inputs, outputs, workspace) is allocated and owned by the caller; the
 *     library never allocates, frees or retains device memory and keeps no global state,
 *     so it is re-entrant and one host thread per process/GPU may call it freely.
 *   - All launches are asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     legacy default stream).  No entry point synchronises, so calls may be captured into a
 *     hipGraph.
 *   - Return value: 0 = ok; negative = argument error (GJ_E_*); positive = hipError_t of a
 *     failed launch.  Nothing throws across the ABI.  gj_error_string() describes a code.
 *   - Index arrays are int32 (the reference's int64 COO is compiled once on the host into
 *     int32 CSR, see gj_plan below); all values are IEEE fp32, computed with FMA contraction
 *     off so that the op sequence matches the reference's ATen ops.
 */
#ifndef GRADJUNE_HIP_H
#define GRADJUNE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GJ_ABI_VERSION 7

#define GJ_MAX_SETS 12        /* distinct agent<->venue edge sets in a world (reference: 6)   */
#define GJ_MAX_NETS 16        /* infection networks active in one step (reference: <= 11)      */
#define GJ_MAX_NETS_PER_SET 8 /* networks sharing one edge set (reference: 6 leisure classes)  */
#define GJ_TABLE_SIZE 400     /* one leisure table: [day_type 2][sex 2][age 100] floats        */

/* error codes (negative) */
#define GJ_OK 0
#define GJ_E_NULL (-1)     /* required pointer is NULL                      */
#define GJ_E_RANGE (-2)    /* count / index out of the documented range     */
#define GJ_E_PLAN (-3)     /* inconsistent plan (sizes, strides, schedule)  */
#define GJ_E_NODEVICE (-4) /* no HIP device / wrong architecture            */

/* how a network derives its per-agent transmission / susceptibility from the raw values
 * (reference: grad_june/infection_networks/base.py:47-59,144-149;
 *             grad_june/infection_networks/leisure_network.py:61-85,107-120)           */
typedef enum gj_mask_kind {
  GJ_MASK_RAW = 0,      /* household: raw transmission / susceptibility, ignores quarantine */
  GJ_MASK_Q = 1,        /* q[a] * value                                                      */
  GJ_MASK_QL = 2,       /* q[a] * L[day, sex[a], age[a]] * value                             */
  GJ_MASK_QL_AGE75 = 3  /* as QL; susceptibility additionally * (age[a] > 75) (care_visit)   */
} gj_mask_kind;

/* One agent<->venue edge set, compiled once from the reference's COO
 * `data["attends_<set>"].edge_index` (int64 [2,E], row 0 agent, row 1 venue;
 * grad_june/june_world_loader/network_loader.py:30-44) into two int32 CSR views.
 * Edge order inside every CSR row is the COO order (stable sort), so sums taken in row
 * order reproduce the reference's scatter_add_ order.                                      */
typedef struct gj_edge_set {
  int64_t n_venues;
  int64_t n_edges;
  const int32_t* v_rowptr;  /* device [n_venues+1]  CSR by venue                            */
  const int32_t* v_agent;   /* device [n_edges]     agent of each edge, venue-major         */
  const float* v_pcontact;  /* device [n_venues]    clamp(1/(people-1),0,1), base.py:63-69  */
  const int32_t* a_rowptr;  /* device [n_agents+1]  CSR by agent                            */
  const int32_t* a_venue;   /* device [n_edges]     venue of each edge, agent-major         */
  float* cum;               /* device [n_venues*cum_stride] workspace: pass-1 out, pass-2 in */
  int32_t cum_stride;       /* floats per venue in `cum` (>= networks active on this set)   */
  int32_t _pad;
} gj_edge_set;

/* One workgroup's share of pass 1 (built on the host by the graph compiler).
 * kind 0: STREAM - venues [v0,v1) whose edges [e0,e1) (<= GJ_STREAM_EDGES) are staged through
 *         LDS and reduced with `lanes` (1,4,16 or 64) lanes per venue.
 * kind 1: LONG   - edges [e0,e1) of the single venue v0; the partial sum goes to
 *         partial[slot*cum_stride + k] and is combined in chunk order by a second kernel.  */
typedef struct gj_block {
  int32_t set;
  int32_t kind;
  int32_t v0, v1;
  int32_t e0, e1;
  int32_t slot;
  int32_t lanes;
} gj_block;

/* venue whose degree exceeds the stream capacity: partial slots [slot0,slot1) -> cum[v] */
typedef struct gj_long_row {
  int32_t set;
  int32_t v;
  int32_t slot0, slot1;
} gj_long_row;

#define GJ_STREAM_EDGES 2048 /* max edges of a STREAM block (256 threads x 8)               */

/* ---- tiled ("propagation-blocked") layout: the fast path of both passes -------------------
 * Agents are cut into n_slices slices of slice_agents consecutive agents; the venues of a set
 * into blocks of consecutive venues; edge (a, v) belongs to tile (slice(a), block(v)).  Every
 * random access of the two passes then hits LDS (a slice of transmissions / a block of venue
 * sums) and HBM only sees four coalesced streams per step (24 B per edge):
 *   A  one workgroup per slice :  val[block-major pos] = x_slice[a_la]
 *   B  one workgroup per block :  sums[e_lv] += val   (LDS integer atomics); cum = beta*p_contact*sums
 *   C  same workgroup (fused)  :  val[i] = cum[e_lv[i]]          (in place)
 *   D  one workgroup per slice :  acc[a_la] += val[block-major pos]; epilogue a7-a9
 * A tile is contiguous in both the slice-major (s, j) and the block-major (j, s) edge order.
 * Sums are accumulated with 64-bit fixed-point LDS atomics (resolution 2^-36 per venue, 2^-32 per agent).  The
 * reference has no window (its sums stay finite and the epilogue clamps them, base.py:136-138); here a TERM beyond
 * +-16384 (venue; less for sets with venues of > 4096 attendees, see max_venue_edges) / +-262144 (agent), or an
 * infinity, SATURATES its sum: the element reads back +-1e30, which every later stage carries to the epilogue's clamp
 * (exp(-100 dt): infected with certainty) while a zero factor - p_contact of an empty venue, susceptibility 0, a
 * quarantine mask - still gives 0, as in the reference.  A NaN term, or saturation in both directions, reads back NaN.
 * No sum can wrap: terms x attendees is bounded per set (max_venue_edges), edges per agent by 4096.
 * integer adds are order-independent, so results are bitwise reproducible from run to run, and
 * agree with the CSR path to fp32 rounding.                                                  */
typedef struct gj_tiled_set {
  int32_t n_blocks;          /* J: venue blocks of this set                                  */
  int32_t max_block_venues;  /* largest block of this set (sizes the LDS of phases B/C)      */
  int32_t desc_wide;         /* 0: chunk_desc holds 4, 1: 8 int32 per chunk (see chunk_desc); 2: no descriptors -
                                chunk_desc holds int32 [E], the block-major slot of every slice-major edge
                                (sets with tiles of a few edges)                                  */
  int32_t ell_k;             /* 0: pass 2 of this set runs through phases C + D.  2, 4 or 8: "direct"
                                form - phase C is skipped, phase D reads the venues' cum from an LDS
                                table through `ell` (sets with <= 65534 venues, see `ell`)        */
  const int32_t* blk_v0;     /* device [J+1]   venue range of block j                        */
  const int32_t* blk_e0;     /* device [J+1]   block-major SLOT range of block j; every block is
                                               padded to a multiple of 8 slots (16-byte accesses) */
  const uint16_t* e_lv;      /* device [slots] venue index local to its block, block-major;
                                               0xFFFF marks a pad slot                        */
  const uint8_t* e_cls;      /* device [slots] agent_class of the edge's agent, block-major
                                               (sets that carry leisure tables; else NULL)    */
  const uint16_t* a_la;      /* device [E]     agent index local to its slice, slice-major   */
  const int32_t* tile_sptr;  /* device [S*J+1] slice-major prefix: tile (s,j) = [sptr[s*J+j], sptr[s*J+j+1]) */
  const int32_t* tile_jpos;  /* device [S*J]   block-major start slot of tile (s,j)          */
  const int32_t* chunk_ptr;  /* device [S+1]   first 64-edge chunk of slice s's slice-major segment */
  const int32_t* chunk_desc; /* device [4*chunks] per 64-edge chunk: slot0, slot1, split|multi<<16, j0:
                                the first `split` edges map to block-major slots slot0.., the rest
                                (next non-empty tile) to slot1..; multi: spans > 2 tiles, lanes
                                resolve through tile_sptr/tile_jpos starting at block j0.
                                desc_wide (sets with small tiles): [8*chunks], base_0..base_5,
                                start_1|start_2<<8|start_3<<16|start_4<<24, start_5|multi<<8|j0<<9:
                                lanes [start_k, start_k+1) lie in one tile and map to slots
                                base_k + lane (start_0 = 0, unused segments start at 64);
                                multi: more than 6 tiles                                        */
  float* val;                /* device [slots] workspace: per-edge value (phase A->B, C->D)  */
  const uint16_t* ell;       /* device [ell_k / 2 planes][owned slices * slice_agents][2] or NULL: the venue
                                ids (whole-set numbering) of each OWNED agent's edges in COO order, columns in pairs (plane p holds an agent's edges 2p and
                                2p + 1), 0xFFFF = none.  Replaces a_la / val / chunk_desc reads of phase D and
                                all of phase C for this set: 2 * ell_k bytes per agent                    */
  /* "Run form" of ONE edge per owned agent (NULL pointers: none).  When the owned agents are ordered by their smallest
   * venue of this set (the household-major order of graph.locality_order; agents without an edge last), the agents
   * whose smallest venue is v are consecutive, and that "primary" edge (a, vmin(a)) needs no entry in the arrays
   * above: phase B reads the transmissions of block j's agents [run_blk_r0[j], run_blk_r0[j+1]) straight from the
   * per-agent array next to run_pv_blk (phase A has nothing to scatter for them); phase D stages the window
   * [run_win_lo[s], run_win_lo[s] + run_win_n[s]) of the venues' cum through LDS and reads it through run_pv_win
   * (phase C has nothing to write for them).  The set's other edges stay in the tiled arrays.                     */
  const uint16_t* run_pv_blk; /* device [owned slices * slice_agents] vmin(a) - blk_v0[block of vmin(a)], 0xFFFF = none */
  const uint16_t* run_pv_win; /* device [owned slices * slice_agents] vmin(a) - run_win_lo[slice of a], 0xFFFF = none    */
  const int32_t* run_blk_r0;  /* device [J+1]  first agent whose primary venue lies in block j (non-decreasing)        */
  const int32_t* run_win_lo;  /* device [owned slices] first venue of the slice's window                              */
  const int32_t* run_win_n;   /* device [owned slices] venues in the window (0: no primary edge in the slice)         */
  int32_t run_max_window;     /* max run_win_n (sizes the LDS table of phase D), <= 32768                             */
  int32_t run_tiled_edges;    /* with a run form: the edges the tiled arrays above hold (the set's n_edges minus the
                                 primary ones; may be 0 - every person lives in exactly one household)               */
  /* Pass 1 in the "direct" form (NULL: through phases A + B).  For a set in the direct form of pass 2 (ell_k != 0)
   * whose edges ALL belong to owned agents, the ELL rows serve pass 1 too: gj_tiled.presum_wgs workgroups each take a
   * contiguous range of owned agents, add every edge's term into an LDS table of 64-bit fixed-point sums per (venue,
   * network) and write it to presum[workgroup][venue][network]; a second launch adds the tables up and applies
   * beta * p_contact.  Exact (integer sums), so cum is the same bit for bit as through phases A + B.              */
  int64_t* presum;            /* device [presum_wgs][n_venues * cum_stride] workspace or NULL                         */
  const int32_t* multi_slots; /* device [n_multi * 64] or NULL: the block-major slots of the 64 edges of every chunk that spans
                                 more tiles than its descriptor has segments ("multi"); the descriptor's j0 field holds the
                                 chunk's row.  NULL: such a chunk's lanes walk tile_sptr / tile_jpos from block j0
                                 (rounds 1-3: ~50x the cost of a chunk - 1 % of them doubled phase A on a world with a
                                 geography).  ABI 6                                                                     */
  int32_t max_venue_edges;    /* edges of the set's LARGEST venue (run-form primaries included).  Bounds the terms of one
                                 venue sum: the window of a term is min(16384, 2^26 / next_pow2(max_venue_edges)), so that
                                 no sum can leave its 64 bits.  0 = not stated: 16384, no such guarantee (ABI 6)        */
  int32_t _pad_mve;
} gj_tiled_set;

typedef struct gj_tiled {
  int32_t n_slices;          /* S                                                            */
  int32_t slice_agents;      /* SA (multiple of 64, <= 19840: one slice of 8-byte sums + two flag bits per agent fits LDS) */
  int32_t direct_table_floats; /* 0: the direct form of pass 2 stages as many venue values through LDS at once
                                as fit; > 0: at most this many (tests: forces several groups)   */
  int32_t n_work;            /* entries of `work`                                            */
  const int32_t* work;       /* device [2*n_work] (set, block) pairs, heaviest first         */
  float* agent_scratch;      /* device [n_agents] workspace or NULL.  Non-NULL: phase D hands its
                                per-agent sums to a separate full-occupancy epilogue launch  */
  int32_t presum_wgs;        /* workgroups (= partial tables) of the direct form of pass 1, see gj_tiled_set.presum;
                                0: no set uses it                                                 */
  int32_t _pad_presum;
  gj_tiled_set sets[GJ_MAX_SETS];
} gj_tiled;

/* The compiled, immutable contact graph ("plan").  Host struct; arrays it points to are device
 * memory owned by the caller.                                                              */
typedef struct gj_plan {
  int64_t n_agents;           /* agents OWNED by this rank (all per-agent outputs)           */
  int64_t n_ext_agents;       /* owned + halo agents: length of transmission, q_transmission
                                 and agent_class, the arrays pass 1 gathers from (== n_agents
                                 on one GPU); v_agent indexes this extended range            */
  int32_t n_sets;
  int32_t n_blocks;           /* entries of `blocks`                                        */
  int32_t n_long_rows;        /* entries of `long_rows`                                     */
  int32_t n_partial_slots;    /* slots of `partial`                                         */
  gj_edge_set sets[GJ_MAX_SETS];
  const gj_block* blocks;     /* device [n_blocks]                                          */
  const gj_long_row* long_rows; /* device [n_long_rows]                                     */
  float* partial;             /* device [n_partial_slots * GJ_MAX_NETS_PER_SET] workspace   */
  const uint8_t* agent_class; /* device [n_ext_agents]  sex*100 + age  (0..199).  4-byte aligned and
                                 readable up to the next multiple of 4 agents when a leisure set is
                                 in the direct form (gj_tiled_set.ell): four classes are one load   */
  const float* tables;        /* device [n_tables * GJ_TABLE_SIZE] leisure tables           */
  int32_t n_tables;
  int32_t _pad;
  const gj_tiled* tiled;      /* HOST pointer or NULL.  Non-NULL: the passes run on the tiled
                                 layout and the CSR arrays of `sets` (v_rowptr, v_agent, a_rowptr,
                                 a_venue, blocks, long_rows) may be NULL                      */
} gj_plan;

/* One infection network active in this step
 * (reference: one InfectionNetwork module, base.py:11-87 / leisure_network.py:7-120).      */
typedef struct gj_network {
  float beta;          /* 10**log_beta * active SocialDistancing factors, fp32 (base.py:36-42) */
  int32_t set;         /* index into gj_plan.sets                                             */
  int32_t mask_kind;   /* gj_mask_kind                                                        */
  int32_t table;       /* index into gj_plan.tables, or -1                                    */
} gj_network;

/* The two scalars that change from one timestep to the next, in DEVICE memory: with gj_step_params.clock set, the
 * kernels read `now` and `step` from there instead of from the launch arguments, so a step captured once in a
 * hipGraph (kernels + the multi-GPU collectives) can be replayed for every following timestep of the same kind
 * (same networks, betas, duration) - gj_clock_advance is the graph's first node.                              */
typedef struct gj_clock {
  float now;      /* timer.now, days: what the kernels read                                        */
  float _pad;
  uint64_t step;  /* Philox stream id: timestep counter                                            */
  double now0;    /* (now0, step0): the origin the host set; gj_clock_advance derives               */
  uint64_t step0; /* now = (float)(now0 + (step - step0) * delta) - no accumulated rounding, the    */
                  /* same value an eager run computes on the host for that step (timer.py:92-95)    */
} gj_clock;

/* Scalars of one timestep.  `nets` MUST be in the reference's accumulation order
 * (activity hierarchy, grad_june/timer.py:14-26,139-157) with the networks of one edge set
 * adjacent; the kernels add the per-network terms in exactly this order.                   */
typedef struct gj_step_params {
  float now;            /* timer.now, days (timer.py:92-95)                                 */
  float delta_time;     /* timer.duration, days (timer.py:101-103)                          */
  int32_t day_type;     /* 0 weekday, 1 weekend (timer.py:84-90)                            */
  int32_t has_quarantine; /* 0: no quarantine-policy collection (mask is scalar 1.0)        */
  float q_threshold;    /* min stage_threshold over ACTIVE quarantine policies, +inf if none */
  int32_t n_nets;
  uint64_t seed;        /* Philox key (perf mode)                                           */
  uint64_t step;        /* Philox stream id: timestep counter                               */
  int64_t agent_offset; /* global id of local agent 0 (multi-GPU: partition-invariant RNG)  */
  int32_t transpose;    /* 0: forward.  1 (tiled layout, backward pass): the two passes run with the
                           pass-1 / pass-2 per-network weights exchanged - the adjoint of the
                           aggregation w.r.t. the transmissions (row f3)                      */
  int32_t _pad;
  gj_network nets[GJ_MAX_NETS];
  const gj_clock* clock; /* device pointer or NULL.  Non-NULL: `now` and `step` above are ignored, the kernels read
                            them from *clock (see gj_clock)                                                 */
} gj_step_params;

/* Per-agent state, all device fp32 [n_agents] unless noted.
 * (reference: data["agent"].*, grad_june/runner.py:72-90)                                  */
typedef struct gj_agent_state {
  const float* max_infectiousness; /* infection_parameters["max_infectiousness"]            */
  const float* shape;
  const float* rate;
  const float* shift;
  float* infection_time;
  float* is_infected;
  float* susceptibility;
  float* transmission;       /* out of a1; in of pass 1                                     */
  float* q_transmission;     /* workspace: qmask*transmission; may alias `transmission` when
                                has_quarantine == 0                                          */
  const float* current_stage; /* symptoms["current_stage"] as fp32 (NULL iff !has_quarantine) */
} gj_agent_state;

int gj_version(void);
const char* gj_error_string(int code);

/* GJ_OK when the CURRENT HIP device can run this library (a gfx950 / MI355X: the kernels are built for that
 * architecture only and size their workgroups for its 160 KiB of LDS per CU), GJ_E_NODEVICE otherwise.
 * The host mirror calls it once per process before the first launch (there is no other path to fall back to). */
int gj_check_device(void);

/* Which optional outputs / inputs the fused step uses. NULL = not wanted / not supplied.  */
typedef struct gj_step_io {
  float* not_infected_probs; /* out [n_agents] (a7), optional                               */
  float* new_infected;       /* out [n_agents] (a8), optional                               */
  const float* exp_noise;    /* in  [2*n_agents] Exponential(1) draws, row 0 = "not infected";
                                NULL = draw in-kernel with Philox4x32-10(seed, step, agent)  */
  float* trans_susc;         /* out [n_agents] pre-clamp sum over networks, optional (tests) */
  float* agent_sums;         /* out [n_agents] the same sum WITHOUT the agent's susceptibility factor (trans_susc =
                                susceptibility * agent_sums), optional: what a backward pass needs of the forward
                                (grad_june_amd/autograd.py keeps it instead of recomputing both passes).  Tiled
                                layout only: the CSR kernels multiply per term, as the reference does (GJ_E_PLAN) */
} gj_step_io;

/* a1 + a2: replaces TransmissionUpdater.forward (grad_june/transmission.py:38-51) and the
 * quarantine mask of QuarantinePolicies.apply (grad_june/policies/quarantine_policies.py:26-33).
 * Writes state->transmission and, when has_quarantine, state->q_transmission.              */
int gj_transmission_update(const gj_plan* plan, const gj_agent_state* state,
                           const gj_step_params* params, void* stream);

/* a2 alone: q_transmission[a] = (current_stage[a] < q_threshold) * transmission[a] for a
 * transmission vector the caller filled itself (the contract of InfectionNetworks.forward,
 * base.py:118-141, which reads data["agent"].transmission).  No-op when !has_quarantine.     */
int gj_quarantine_transmission(const gj_plan* plan, const gj_agent_state* state,
                               const gj_step_params* params, void* stream);

/* a3 + a4 + a5 (pass 1): replaces, for every active network, the first
 * `self.propagate(edge_index, x=transmissions, y=beta*p_contact)` of InfectionNetwork.forward
 * (grad_june/infection_networks/base.py:61-79).  Fills plan->sets[s].cum.                   */
int gj_venue_reduce(const gj_plan* plan, const gj_agent_state* state,
                    const gj_step_params* params, void* stream);

/* a4 + a6 + a7 (+ a8 + a9 when `sample` != 0): replaces the second propagate
 * (base.py:80-83), the sum over networks and clamp/exp/clamp of InfectionNetworks.forward
 * (base.py:118-141) and, fused, IsInfectedSampler.forward (grad_june/infection.py:13-18) and
 * GradJune.infect_people (grad_june/model.py:90-110).                                       */
int gj_agent_gather(const gj_plan* plan, const gj_agent_state* state,
                    const gj_step_params* params, const gj_step_io* io, int sample,
                    void* stream);

/* a8 + a9 alone on a given probability vector: replaces IsInfectedSampler.forward +
 * infect_people for callers that hold `not_infected_probs` (e.g. infect_fraction_of_people,
 * grad_june/infection.py:31-42).  The three state pointers may ALL be NULL: then only
 * `new_infected` is produced (IsInfectedSampler.forward alone).
 * new_infected is exactly 0 or 1 (a tie of the two softmax terms: 0), or NaN where torch gives NaN: a NaN
 * probability or an injected draw of 0.  An agent with new_infected == 0 keeps its state bits.  The others get
 * max(0, s - nu), i + nu, t + nu * (now - t) as separate fp32 operations; a NaN nu or a NaN susceptibility gives
 * a NaN susceptibility (torch.maximum), like is_infected and infection_time, in the fused step too.           */
int gj_sample_infect(int64_t n_agents, const float* not_infected_probs, const float* exp_noise,
                     uint64_t seed, uint64_t step, int64_t agent_offset, float now,
                     float* new_infected, float* susceptibility, float* is_infected,
                     float* infection_time, void* stream);

/* ---- row f1 ("next"): disease-stage progression, run right after the hot path each step -------
 * replaces SymptomsUpdater.forward + SymptomsSampler.sample_next_stage
 * (grad_june/symptoms.py:204-247, 82-128) as one fused per-agent kernel.                        */
#define GJ_MAX_STAGES 16
typedef struct gj_symptoms_params {
  int32_t n_stages;                 /* len(symptoms.stages), <= GJ_MAX_STAGES (reference: 8)     */
  int32_t _pad;
  const float* progress;            /* device [n_stages*100] P(progress | stage, age) (symptoms.py:39-51) */
  int32_t next_kind[GJ_MAX_STAGES]; /* dwell time before progressing: 0 none, 1 LogNormal, 2 Normal */
  float next_loc[GJ_MAX_STAGES];
  float next_scale[GJ_MAX_STAGES];
  int32_t rec_kind[GJ_MAX_STAGES];  /* dwell time before recovering                              */
  float rec_loc[GJ_MAX_STAGES];
  float rec_scale[GJ_MAX_STAGES];
  float time;                       /* timer.now                                                 */
  float _pad2;
  uint64_t seed, step;              /* Philox key / stream (when no noise is injected)           */
  int64_t agent_offset;
} gj_symptoms_params;

/* current_stage / next_stage / time_to_next_stage: device fp32 [n], updated in place.
 * progresses / dwell: optional injected randomness (device fp32 [n]): the torch.bernoulli outcome
 * and the stage-time sample each agent consumes; NULL = Philox4x32-10(seed, step, agent).       */
int gj_symptoms_update(int64_t n, const uint8_t* agent_class, const float* new_infected,
                       float* current_stage, float* next_stage, float* time_to_next_stage,
                       const gj_symptoms_params* params, const float* progresses, const float* dwell,
                       void* stream);

/* ---- row f2 ("next"): the Runner's per-step result reductions in one pass -----------------------
 * replaces, per timestep, `is_infected.sum()` (grad_june/runner.py:167), get_cases_by_age
 * (runner.py:217-224: one masked sum per age bin, OPEN intervals lo < age < hi) and the deaths
 * count of store_differentiable_deaths (runner.py:198-215).
 * out: device double [2 + n_bins], ZEROED by the caller:  out[0] = sum is_infected,
 * out[1 .. n_bins] = sum is_infected over each age bin, out[1 + n_bins] = #agents at `dead_stage`.
 * Accumulated in fp64 (exact for these integer-valued sums), so the result is order-independent. */
#define GJ_MAX_AGE_BINS 8
int gj_step_stats(int64_t n, const uint8_t* agent_class, const float* is_infected,
                  const float* current_stage, int32_t n_bins, const int32_t* bin_edges /* host [n_bins+1] */,
                  int32_t dead_stage, double* out, void* stream);

/* ---- rows f1 + f2 in ONE pass: gj_symptoms_update followed by gj_step_stats of the updated state -----------------
 * What the reference's time loop does after the hot path of every step (grad_june/model.py:141 then
 * runner.py:167-171): the stage progression, then the result reductions over the post-update is_infected /
 * current_stage.  One kernel, four agents per lane: the three symptom arrays are read once and written back only
 * where an agent's values changed, the reductions are taken from the registers that hold the updated stages.
 * Arguments as for the two calls it replaces; `out` (device double [2 + n_bins]) must be ZEROED by the caller.      */
int gj_symptoms_step_stats(int64_t n, const uint8_t* agent_class, const float* new_infected,
                           float* current_stage, float* next_stage, float* time_to_next_stage,
                           const gj_symptoms_params* params, const float* progresses, const float* dwell,
                           const float* is_infected, int32_t n_bins, const int32_t* bin_edges /* host [n_bins+1] */,
                           int32_t dead_stage, double* out, void* stream);

/* ---- row f2 by agent group: result series per area / super area / ethnicity / any integer label ------------------
 * restates, for every label at once, the masked sums of get_cases_by_ethnicity (grad_june/runner.py:235-242: one
 * [n] mask per group) and the deaths form of store_differentiable_deaths (runner.py:198-215) per group:
 *   out[g]            += sum over agents a with group[a] == g of is_infected[a]
 *   out[n_groups + g] += number of those agents with current_stage[a] == dead_stage
 * group: device int32 [n], labels in [0, n_groups).  out: device double [2 * n_groups]; the call ADDS to it, like
 * gj_step_stats.  workspace: device, GJ_GROUP_WORKSPACE_BYTES(n_groups) bytes, 8-byte aligned, ZEROED by the caller
 * before its first use; a call leaves the sums in it zero again, so it can be reused without clearing.
 * Order independence: is_infected is summed as a 64-bit integer in 32.32 fixed point (deaths as a count) and
 * converted to double once, so two launches - or any permutation of the agents together with their labels - give
 * the same bits.  A value is rounded to the nearest multiple of 2^-32 (exact for the model's 0 / 1 / 2); a group's
 * sum must stay below 2^31.  What cannot be summed that way never reaches another group: an agent whose label is
 * outside [0, n_groups) is skipped altogether (the label is never used as an index) and sets GJ_GROUP_ERR_LABEL in
 * the error word; an is_infected that is not finite or beyond +-2^18 adds 0 to its group and sets
 * GJ_GROUP_ERR_VALUE.  The error word is the uint32 at byte 16 * n_groups of the workspace; it is sticky until the
 * caller clears it, and the caller reads it when it wants to know (the Python binding raises).
 * Three regimes, chosen from n_groups:  (i) n_groups <= 4096: every workgroup keeps the 2 * n_groups accumulators
 * in LDS (at most 64 KiB, two workgroups per CU) and adds the non-zero ones to the workspace when it is done, one
 * 64-bit atomic each;  (ii) above that, the lanes of a wave fold their runs of equal labels and one lane issues one
 * global 64-bit atomic per run: labels that follow the geography cost one atomic per wave and boundary, shuffled
 * labels one per agent;  (iii) n_groups == 1 is regime (i) with a single run that is never closed before the end:
 * the national sums of gj_step_stats.  In every regime a workgroup reads a contiguous share of the agents.         */
#define GJ_MAX_GROUPS (1 << 28)
#define GJ_GROUP_WORKSPACE_BYTES(n_groups) (16 * (int64_t)(n_groups) + 8)
#define GJ_GROUP_ERR_LABEL 1u
#define GJ_GROUP_ERR_VALUE 2u
int gj_group_stats(int64_t n, const int32_t* group, int32_t n_groups, const float* is_infected,
                   const float* current_stage, int32_t dead_stage, double* out, void* workspace, void* stream);

/* adjoint of gj_group_stats (what autograd gives for the reference's forms above): the gather
 *   grad_is_infected[a] = g_cases[group[a]]
 *   grad_stage[a]       = g_deaths[group[a]] / dead_stage * (current_stage[a] == dead_stage)
 * g_cases / g_deaths: device fp32 [n_groups], NULL = zeros.  grad_is_infected / grad_stage: device fp32 [n], each
 * may be NULL: a NULL output is neither computed nor written (current_stage is read for grad_stage only).  An agent
 * whose label is outside [0, n_groups) gets 0.  Up to 2048 groups the two rows are staged in LDS once per workgroup. */
int gj_adjoint_group_stats(int64_t n, const int32_t* group, int32_t n_groups, const float* current_stage,
                           int32_t dead_stage, const float* g_cases, const float* g_deaths, float* grad_is_infected,
                           float* grad_stage, void* stream);

/* ---- row f2 by symptom stage: occupancy of every stage and the entries into it, nationally or by agent group ------
 * A pure addition to ABI 7.  What hospital data records - beds occupied, daily admissions - are the number of agents
 * in `severe` / `critical` and the entries into them; the reference reduces only the last stage to a series
 * (store_differentiable_deaths, runner.py:198-215).  For agent a with g = group[a] (0 when group is NULL) and
 * s = (int)current_stage[a]:
 *   out[0][g][s] += 1                                                      (occupancy)
 *   out[1][g][s] += 1  if prev_stage is given and prev_stage[a] != current_stage[a]   (a entered s during this step)
 * out: device int64 [2][n_groups][n_stages]; the call ADDS to it.  The counts are 64-bit integers: no order of the
 * agents, no grid and no regime changes a bit, and there is neither a workspace nor a finish launch.
 * Bad input never reaches a bin: an agent whose label is outside [0, n_groups) is skipped (the label is never used as
 * an index) and sets GJ_STAGE_ERR_LABEL in *err; a current_stage that is not an integer value in [0, n_stages) - NaN,
 * 2.5, -1, n_stages - is skipped and sets GJ_STAGE_ERR_STAGE.  *err (device uint32) is sticky until the caller clears it.
 * group: device int32 [n], or NULL = every agent in group 0 (n_groups must be 1).  prev_stage: device fp32 [n] or
 * NULL (plane 1 is then left alone).  n_groups * n_stages <= INT32_MAX; n <= GJ_STAGE_MAX_AGENTS.
 * One pass, 8 B per agent (12 with labels), a workgroup reads a CONTIGUOUS share of the agents; four agents per lane
 * and load when every array is 16-byte aligned.  Three regimes:
 *  (i)   n_groups == 1 (the national call, where most agents share one or two bins): every lane counts in private
 *        8-bit fields of four 64-bit registers, the lanes' counts are added by wave shuffles at the end and at most
 *        2 * n_stages 64-bit atomics per workgroup reach memory.  The grid is sized so that a lane takes at most
 *        GJ_STAGE_LANE_LOADS loads of four agents: a field cannot overflow.
 *  (ii)  n_groups * n_stages <= GJ_STAGE_LDS_BINS: a lane carries one open run keyed on the bin g * n_stages + s; the
 *        lanes of a wave that close the same bin fold their counts with shuffles and one adds to the workgroup's
 *        histogram of 32-bit counters in LDS (2 * 4 B * 8192 = 64 KiB at most), whose non-zero counters are added to
 *        `out` at the end, one 64-bit atomic each.
 *  (iii) above that: the same runs, one global 64-bit atomic per folded run.
 * (i) and (ii) launch at most GJ_STAGE_LDS_BLOCKS workgroups of GJ_STAGE_LDS_THREADS lanes ((i): more where the lane
 * bound asks for it), (iii) at most GJ_STAGE_GLOBAL_BLOCKS of GJ_STAGE_GLOBAL_THREADS.
 * Errors, returned before any device work: GJ_E_RANGE for n < 0 or > GJ_STAGE_MAX_AGENTS, n_groups outside
 * 1..GJ_MAX_GROUPS, n_stages outside 1..GJ_MAX_STAGES, n_groups * n_stages > INT32_MAX, group == NULL with
 * n_groups != 1; GJ_E_NULL for a NULL current_stage, out or err.                                                     */
#define GJ_STAGE_ERR_LABEL 1u
#define GJ_STAGE_ERR_STAGE 2u
#define GJ_STAGE_LDS_BINS 8192
#define GJ_STAGE_LDS_THREADS 1024
#define GJ_STAGE_LDS_BLOCKS 512
#define GJ_STAGE_GLOBAL_THREADS 256
#define GJ_STAGE_GLOBAL_BLOCKS 2048
#define GJ_STAGE_LANE_LOADS 63
#define GJ_STAGE_MAX_AGENTS ((int64_t)1 << 40)
int gj_stage_stats(int64_t n, const int32_t* group, int32_t n_groups, int32_t n_stages, const float* current_stage,
                   const float* prev_stage, int64_t* out, uint32_t* err, void* stream);

/* adjoint of gj_stage_stats.  The differentiable value of a count is the reference's own form for deaths
 * (store_differentiable_deaths, and mask_stage * current_stage / i in sample_next_stage): sum (stage == s) * stage / s;
 * the entry mask (prev != stage) is a constant.  With s = current_stage[a], g = group[a]:
 *   grad_stage[a] = g_occupancy[g][s] / s + (prev_stage[a] != current_stage[a] ? g_entries[g][s] / s : 0)    for s >= 1
 *   grad_stage[a] = 0                                              for s == 0, a bad label or a bad stage (as above)
 * Column 0 (`recovered`) is therefore a plain count with zero gradient: the reference's form divides by the stage id.
 * g_occupancy / g_entries: device fp32 [n_groups][n_stages], NULL = zeros.  grad_stage: device fp32 [n], written for
 * every agent.  A gather; up to GJ_STAGE_ADJ_LDS_BINS bins the two tables are staged in LDS once per workgroup.
 * Errors as for gj_stage_stats, with GJ_E_NULL for a NULL current_stage or grad_stage.                              */
#define GJ_STAGE_ADJ_LDS_BINS 2048
int gj_adjoint_stage_stats(int64_t n, const int32_t* group, int32_t n_groups, int32_t n_stages,
                           const float* current_stage, const float* prev_stage, const float* g_occupancy,
                           const float* g_entries, float* grad_stage, void* stream);

/* ---- row f2 by infection location: the step's new infections attributed to the networks they came through ---------
 * A pure addition to ABI 7.  Run AFTER a step, with the step's own `params`, while plan->sets[s].cum still holds the
 * step's per-venue sums cum_n[v] (column k of a set = its k-th network among the step's active networks, in the order
 * of params->nets).  For an agent a with new_infected[a] == 1 and every active network n, in fp64:
 *   t_n[a] = w_n[a] * susceptibility0[a] * sum over the edges (a, v) of n's edge set of cum_n[v]
 * w_n the receiving-side recipe of gj_mask_kind: 1 (RAW), q[a] (Q), q[a] * L_n[day_type][class[a]] (QL), that times
 * (age > 75) (QL_AGE75); q[a] = !has_quarantine || current_stage[a] < q_threshold.  This is what the reference's
 * InfectionNetwork.forward returns per network (infection_networks/base.py:61-84); T = sum_n t_n (in the order of
 * nets) is the pre-clamp trans_susc.  T finite and > 0: network n gets the share t_n / T of the infection.  Otherwise
 * the whole infection goes to `background_col`: the reference's probability floor (clamp(ts, 1e-6, ...), base.py:136)
 * infects agents nobody transmitted to.  A term that is NaN or negative counts as 0 and sets GJ_LOC_ERR_VALUE.
 * Shares are 64-bit integers in units of 1 / GJ_LOC_UNIT of an infection: c_n = floor(t_n / T * GJ_LOC_UNIT), the
 * remainder GJ_LOC_UNIT - sum c_n goes to the network with the largest t_n (lowest index on a tie), so every infection
 * adds exactly GJ_LOC_UNIT and out[g][.] sums to GJ_LOC_UNIT * (new infections of group g); no order of the agents, no
 * grid and no regime changes a bit.
 *   out[group[a]][cols[n]] += c_n          out: device int64 [n_groups][n_cols]; the call ADDS to it.
 * rows[s] (s < plan->n_sets): the set's edges as CSR by OWNED agent - a_rowptr device int32 [n_agents + 1], a_venue
 * device int32 [n_edges], venue ids in the set's own numbering - supplied by the caller because gj_edge_set's CSR arrays
 * are NULL on the tiled layout (a CSR plan may pass those).  a_rowptr == NULL: the set contributes nothing.
 * cols: HOST int32 [params->n_nets], the output column of active network i; several networks may share a column.
 * group: device int32 [n_agents] or NULL (n_groups must be 1).  current_stage: NULL iff !has_quarantine.
 * n_nets == 0 is valid: every infection goes to background_col (the seeding step).  n_agents == 0 launches nothing.
 * Bad input never reaches a bin: a label outside [0, n_groups) is skipped (never an index) and sets GJ_LOC_ERR_LABEL; a
 * new_infected that is neither 0 nor 1 is skipped and sets GJ_LOC_ERR_VALUE; a row pointer or venue id outside the set
 * is skipped and sets GJ_LOC_ERR_ROWS.  *err (device uint32) is sticky until the caller clears it.
 * One launch.  A lane reads new_infected for its agents (4 B per agent, coalesced, a workgroup takes a contiguous
 * share); a wave ballots 256 agents and hands the flagged ones to its four groups of 16 lanes, four agents at a time:
 * a group walks its agent's rows set by set with its lanes striding over the edges (8 B of row pointers per set, 4 B
 * per edge, the set's nk floats of cum per edge, at cache-line granularity), reduces in fp64 over the group - lane i
 * holds t_i - and adds the shares: into an LDS histogram when n_groups * n_cols <= GJ_LOC_LDS_BINS, flushed with one
 * 64-bit atomic per non-zero bin, else with global 64-bit atomics.  At most GJ_LOC_BLOCKS workgroups of 256.
 * Errors, returned before any device work: GJ_E_NULL for a NULL plan, params, rows (n_sets > 0), new_infected,
 * susceptibility0, out, err, cols (n_nets > 0), a NULL current_stage with has_quarantine, a_rowptr without a_venue;
 * GJ_E_RANGE for n_nets outside 0..GJ_MAX_NETS, n_groups outside 1..GJ_MAX_GROUPS, group == NULL with n_groups != 1,
 * n_cols outside 1..GJ_LOC_MAX_COLS, cols[i] or background_col outside [0, n_cols); and what gj_step returns for a
 * bad plan or bad networks.                                                                                          */
#define GJ_LOC_UNIT ((int64_t)1 << 30)
#define GJ_LOC_ERR_LABEL 1u
#define GJ_LOC_ERR_VALUE 2u
#define GJ_LOC_ERR_ROWS 4u
#define GJ_LOC_MAX_COLS 64
#define GJ_LOC_LDS_BINS 4096
#define GJ_LOC_BLOCKS 2048
typedef struct gj_location_rows {
  const int32_t* a_rowptr;  /* device [n_agents+1] or NULL: no rows, the set contributes nothing */
  const int32_t* a_venue;   /* device [n_edges]                                                   */
} gj_location_rows;
int gj_location_stats(const gj_plan* plan, const gj_step_params* params, const gj_location_rows* rows /* [plan->n_sets] */,
                      const float* new_infected, const float* susceptibility0, const float* current_stage,
                      const int32_t* group, int32_t n_groups, const int32_t* cols /* host [n_nets] */, int32_t n_cols,
                      int32_t background_col, int64_t* out, uint32_t* err, void* stream);

/* ---- row f2 by infector: the step's new infections attributed to the agents who transmitted ----------------------------
 * A pure addition to ABI 7: gj_location_stats carried one level further, through the venue.  Run at the same point -
 * AFTER a step, with its `params`, while plan->sets[s].cum holds the step's sums, current_stage is the stage the
 * quarantine mask was formed from and state->transmission is the step's - as two sparse passes over `rows`.
 * Notation: network i of params->nets lives on set s_i, column k_i of that set's cum, with beta_i; w_i[a] is the
 * receiving-side weight of gj_mask_kind exactly as gj_location_stats forms it, m_i[b] the transmitting-side one: 1 (RAW),
 * q[b] (Q), q[b] * L_i[day_type][class[b]] (QL and QL_AGE75: care_visit's age > 75 is on the receiving side only,
 * leisure_network.py:107-120).  U[s]: device int64 [n_venues][cum_stride] per set, HOST array [plan->n_sets] of device
 * pointers, all zero before pass 1 (gj_infector_clear, or a memset).
 *
 * gj_infector_scatter (pass 1).  For every agent a with new_infected[a] == 1: t_i and T = t_0 + t_1 + ... are exactly
 * gj_location_stats' values, and for every edge e of a's row in set s_i, at venue v_e, in fp64
 *   t_{i,e} = (w_i[a] * susceptibility0[a]) * cum_{s_i}[v_e][k_i]          (NaN or negative: 0, sets GJ_LOC_ERR_VALUE)
 * A network whose t_i is 0 - by its mask, or because gj_location_stats' rule refused it - has t_{i,e} = 0 at every edge.
 * T finite and > 0: u_{i,e} = floor(t_{i,e} / T * GJ_LOC_UNIT) (at most GJ_LOC_UNIT), and the remainder GJ_LOC_UNIT - sum u
 * goes to the pair with the largest t_{i,e}: the lowest i on a tie, then the lowest position in the row.  The remainder
 * is >= 0: every term is non-negative and at most GJ_MAX_NETS * 4096 of them reassociate in fp64, which moves the sum
 * by less than 2^-7 of a unit.  (Only a negative cum next to larger positive ones - reported as GJ_LOC_ERR_VALUE - can
 * make sum u exceed GJ_LOC_UNIT; nothing is taken back then.)  Every u is added to U[s_i][v_e][k_i] with a 64-bit integer
 * atomic, so no order of the agents or of the workgroups changes a bit of U, and U sums to GJ_LOC_UNIT * (attributed
 * infections).  Otherwise nothing is scattered and *unattributed (device int64; the call ADDS) counts the infection:
 * the decision that sends it to background_col in gj_location_stats, from the same values.
 * cohort (device int32 [n_agents], or NULL): cohort[a] = cohort_value for every a with new_infected[a] == 1.
 * n_nets == 0 is valid (the seeding step): every infection is unattributed, cohort is written, U may be NULL.
 *
 * gj_infector_gather (pass 2).  For every agent b with transmission[b] > 0, in fp64:
 *   credit[b] = sum_i sum over the edges e of b's row in s_i with U != 0 of
 *               U[s_i][v_e][k_i] / GJ_LOC_UNIT * beta_i * pc[v_e] * m_i[b] * transmission[b] / cum_{s_i}[v_e][k_i]
 * pc = gj_edge_set.v_pcontact; cum is read only where U != 0 - the few venues with a new infection - and a cum that is
 * not finite or <= 0 there cannot follow from pass 1: the pair is skipped and GJ_LOC_ERR_VALUE set; so is an agent whose
 * credit is not finite.  Then caused[b] += credit (caused: device fp64 [n_agents] or NULL) and out[group[b]] +=
 * llrint(credit * GJ_LOC_UNIT) (out: device int64 [n_groups] or NULL; integer adds, order-free).  caused and out are
 * separate so that several labellings can be summed from one step (one call with caused, the others without).
 * The credits of one venue sum to its U / GJ_LOC_UNIT only up to the fp32 roundings inside cum - cum is
 * fp32(beta * pc) * fp32(sum of m * transmission) - so a step's credits sum to its attributed infections approximately
 * (relative 2^-22 per venue at worst), not exactly; U itself and the counts are exact.
 * An agent with transmission <= 0 or NaN is untouched.  n_nets == 0 launches nothing.
 *
 * gj_infector_clear: U back to zero by the way it was filled - plain stores of 0 to every column of the venues that the
 * rows of the agents with new_infected != 0 name - instead of a memset of all of U.  Sets without rows or U are skipped.
 *
 * All three: rows as for gj_location_stats; n_agents == 0 launches nothing; one launch each, the launch shape of
 * gj_location_stats (a wave ballots 256 agents and hands the flagged ones to its four groups of 16 lanes, whose lanes
 * stride over the agent's edges); the gather adds through an LDS histogram up to GJ_LOC_LDS_BINS groups, and takes a
 * round of 256 agents with 16 or more infectious ones one agent per lane instead (late in an epidemic a third of the
 * agents transmit: four agents per wave at a time are then too few loads in flight).  The credit's terms are added in
 * fp64 in the order of the path taken - all non-negative, so the paths agree to 4096 * 2^-53 relative.  Bad input
 * never reaches memory: a label outside [0, n_groups) skips its agent (never an index) and sets GJ_LOC_ERR_LABEL; a
 * new_infected that is neither 0 nor 1 is skipped and sets GJ_LOC_ERR_VALUE; a row pointer or venue id outside its set is
 * skipped and sets GJ_LOC_ERR_ROWS.  *err (device uint32) is sticky until the caller clears it.
 * Errors, returned before any device work: what gj_location_stats returns for a bad plan, params or rows; GJ_E_NULL for
 * a NULL new_infected, susceptibility0, unattributed or err (scatter), transmission or err or both of caused and out
 * (gather), a NULL current_stage with has_quarantine, a NULL U with n_nets > 0 or U[s] of a set with rows, venues and an
 * active network; GJ_E_RANGE for n_groups outside 1..GJ_MAX_GROUPS or group == NULL with n_groups != 1.             */
int gj_infector_scatter(const gj_plan* plan, const gj_step_params* params, const gj_location_rows* rows /* [plan->n_sets] */,
                        const float* new_infected, const float* susceptibility0, const float* current_stage,
                        int64_t* const* U /* host [plan->n_sets] */, int64_t* unattributed, int32_t* cohort,
                        int32_t cohort_value, uint32_t* err, void* stream);
int gj_infector_gather(const gj_plan* plan, const gj_step_params* params, const gj_location_rows* rows /* [plan->n_sets] */,
                       const float* transmission, const float* current_stage, int64_t* const* U /* host [plan->n_sets] */,
                       const int32_t* group, int32_t n_groups, double* caused, int64_t* out, uint32_t* err, void* stream);
int gj_infector_clear(const gj_plan* plan, const gj_location_rows* rows /* [plan->n_sets] */, const float* new_infected,
                      int64_t* const* U /* host [plan->n_sets] */, void* stream);

/* ---- row f2 by pairs of groups: who infects whom ------------------------------------------------------------------------
 * A pure addition to ABI 7: the two passes above with the units kept apart by the group of the INFECTED agent, so that
 * pass 2 is a sum over pairs of groups.  G = n_groups <= GJ_MATRIX_MAX_GROUPS, so that G * G <= GJ_LOC_LDS_BINS.
 * UG[s]: device int64 [n_venues][cum_stride][G] per set, HOST array [plan->n_sets] of device pointers, all zero before
 * pass 1.  It sits beside U, which keeps its layout and its meaning; a step runs both scatters, from the same inputs.
 *
 * gj_infection_matrix_scatter: gj_infector_scatter's rule - the same kernel body: t_i, T, t_{i,e}, floors, remainder and
 * tie-break - with every u added to UG[s_i][v_e][k_i][group[a]] (64-bit integer atomics).  After both scatters of a step
 * the sum over g' of UG[s][v][k][g'] therefore equals U[s][v][k] exactly, in every cell.  An infection nobody
 * transmitted adds 1 to unattributed_by_group[group[a]] (device int64 [G], the call ADDS; may be NULL).  No cohort is
 * written and U is not touched.  n_nets == 0 is valid as for gj_infector_scatter (the seeding step): every infection is
 * counted in unattributed_by_group, UG may be NULL.
 *
 * gj_infection_matrix_gather: gj_infector_gather's walk, both forms of it.  For every agent b with transmission[b] > 0
 * and every edge of its rows where U[s_i][v_e][k_i] != 0 (read first; only there the G cells of UG are read), for every
 * g' with UG[s_i][v_e][k_i][g'] != 0, in fp64 and in the order of gj_infector_gather's term:
 *   out[group[b]][g'] += llrint(UG / GJ_LOC_UNIT * (beta_i * pc[v_e]) * (m_i[b] * transmission[b]) / cum * GJ_LOC_UNIT)
 * out: device int64 [G][G], [infector's group][infected's group]; the call ADDS.  Every term is rounded on its own - a
 * chain of correctly rounded fp64 products and quotients, then one round-to-nearest-even - and the sums are integers
 * (an LDS histogram of G * G bins, one global 64-bit atomic per non-zero bin at the end), so out is independent of the
 * order of the agents, of the workgroups and of which form of the walk took a round.  Against gj_infector_gather's
 * out[g] on the same inputs the row sum over g' differs by the roundings alone: half a unit per non-zero term of the
 * group's agents and half a unit per infectious agent of the group.  n_nets == 0 launches nothing.
 *
 * gj_infection_matrix_clear: UG back to zero by gj_infector_clear's walk: plain stores of 0 to the cum_stride * G cells
 * of every venue that the rows of the agents with new_infected != 0 name.
 *
 * All three: rows, launch shape and bad input as for the three above - a label outside [0, G) skips its agent (in the
 * scatter too: the infected agent's) and sets GJ_LOC_ERR_LABEL; a cum that is not finite or <= 0 where U != 0, or a term
 * that is not finite, skips the pair and sets GJ_LOC_ERR_VALUE; rows outside the set set GJ_LOC_ERR_ROWS.  n_agents == 0
 * launches nothing.  Errors, returned before any device work: as above, with GJ_E_NULL for a NULL UG (n_nets > 0) or
 * UG[s] of a set with rows, venues and an active network, and for a NULL out; GJ_E_RANGE for n_groups outside
 * 1..GJ_MATRIX_MAX_GROUPS or group == NULL with n_groups != 1.                                                        */
#define GJ_MATRIX_MAX_GROUPS 64
int gj_infection_matrix_scatter(const gj_plan* plan, const gj_step_params* params,
                                const gj_location_rows* rows /* [plan->n_sets] */, const float* new_infected,
                                const float* susceptibility0, const float* current_stage, const int32_t* group,
                                int32_t n_groups, int64_t* const* UG /* host [plan->n_sets] */,
                                int64_t* unattributed_by_group, uint32_t* err, void* stream);
int gj_infection_matrix_gather(const gj_plan* plan, const gj_step_params* params,
                               const gj_location_rows* rows /* [plan->n_sets] */, const float* transmission,
                               const float* current_stage, int64_t* const* U /* host [plan->n_sets] */,
                               int64_t* const* UG /* host [plan->n_sets] */, const int32_t* group, int32_t n_groups,
                               int64_t* out, uint32_t* err, void* stream);
int gj_infection_matrix_clear(const gj_plan* plan, const gj_location_rows* rows /* [plan->n_sets] */,
                              const float* new_infected, int64_t* const* UG /* host [plan->n_sets] */, int32_t n_groups,
                              void* stream);

/* ---- row f2 as a tree: one sampled infector per new infection ------------------------------------------------------------
 * A pure addition to ABI 7: where gj_infector_gather gives every infectious agent its EXPECTED share of the step's new
 * infections, gj_infection_tree draws ONE infector for each of them - who infected whom, where, and when.  Run at the
 * point where gj_infector_scatter runs - AFTER a step, with its `params`, while plan->sets[s].cum holds the step's sums,
 * current_stage is the stage the quarantine mask was formed from and `transmission` is the step's.  Notation as above.
 * For every agent a with new_infected[a] == 1:
 *
 * The draw.  One Philox4x32-10 block, counter (agent_offset + a, step | 1 << 60), key `seed` (bit 60 is a stream of its
 * own: bits 61, 62, 63 and the 1 << 40 counter are taken): r1 = word 0 & (2^30 - 1), R = word 2 | word 3 << 32.
 *
 * The (venue, network) pair.  t_i, T, t_{i,e} and u_{i,e} = min(floor(t_{i,e} / T * GJ_LOC_UNIT), GJ_LOC_UNIT) are exactly
 * gj_infector_scatter's values (the same device functions form them), and so is the best pair: the largest t_{i,e}, the
 * lowest i on a tie, then the lowest position in the row.  T not finite or not > 0: nobody transmitted - infector[a] =
 * -2, via[a] = background_col, venue[a] = -1.  Otherwise the pairs are ordered by edge set (the order of plan->sets), then
 * by position in a's row of that set, then by the network's column k_i; given = sum of u over all pairs; if r1 < given
 * the pair is the first whose inclusive prefix sum of u exceeds r1, otherwise it is the best pair - which is therefore
 * drawn with probability (u + GJ_LOC_UNIT - given) / GJ_LOC_UNIT: its cell of U.  All integers: no arrangement of the
 * lanes changes the choice.  via[a] = cols[i], venue[a] = v_e in the set's own numbering.
 *
 * The infector.  venue_rows[s] (s < plan->n_sets): the set's edges as CSR by venue - v_rowptr device int32
 * [n_venues + 1], v_agent device int32 [n_edges], OWNED agents, in a fixed order (DevicePlan.venue_rows: COO order inside
 * a row) - supplied by the caller like `rows`; a CSR plan may pass gj_edge_set's.  Over the members b of venue v, in row
 * order: b == a has weight 0; otherwise w_b = m_i[b] * transmission[b] in fp64 (the product of two fp32 values: exact),
 * NaN or <= 0: weight 0; W_b = min(floor(w_b * 2^36), 2^46) - 2^36 is the hot path's venue resolution; a saturated weight
 * sets GJ_LOC_ERR_VALUE.  S = sum of W_b in unsigned 64 bits: a venue row holds at most GJ_TREE_MAX_VENUE_ROW = 2^18
 * members (a longer one is refused where the rows are built, and counts as a bad row here), so S cannot wrap.  S == 0:
 * unresolved - infector[a] = -3, via and venue keep the pair, *unresolved (device int64; the call ADDS) counts it; it
 * happens only where every transmitter's weight is below 2^-36, or the set has no venue rows (v_rowptr == NULL).
 * Otherwise target = (R * S) >> 64 (the 128-bit product) and infector[a] = agent_offset + the first member whose
 * inclusive prefix sum of W exceeds target.  W_b / S is m_i[b] * transmission[b] over the venue's sum of them up to the
 * 2^-36 floor - b's share in gj_infector_gather's credit - so the expectation of the sample is the infector series.
 *
 * counts[via[a]] += 1 (device int64 [n_cols], exact; the call ADDS) and row_of[a] = row_value.  infector, via, venue,
 * row_of: device int32 [n_agents]; an agent with new_infected[a] == 0 is untouched (the caller starts infector at -1,
 * "never infected").  n_nets == 0 is valid (the seeding step): every infection gets -2 and background_col, venue_rows is
 * not read.  n_agents == 0 launches nothing.
 * Bad input never becomes an index: a new_infected that is neither 0 nor 1 is skipped and sets GJ_LOC_ERR_VALUE; a row
 * pointer or venue id of `rows` outside its set is skipped and sets GJ_LOC_ERR_ROWS; a venue row outside its set or
 * longer than GJ_TREE_MAX_VENUE_ROW counts as empty, a member outside [0, n_agents) has weight 0, and both set
 * GJ_LOC_ERR_ROWS.  *err (device uint32) is sticky until the caller clears it.
 * One launch, the launch shape of gj_location_stats: a group of 16 lanes per newly infected agent; the pairs are walked
 * once, in chunks of 16 positions with an exclusive scan over the group; the venue row twice (sum, then select), in
 * batches of 4 members per lane whose transmissions are loaded together - the mask's inputs are read for the members
 * that transmit only - by the agent's group, or, a row of more than 256 members, by the whole wave (one such row after
 * the other: a launch ends with its longest row); a row of one batch is not loaded again.  counts go through an LDS
 * histogram of n_cols bins.
 * Errors, returned before any device work: what gj_location_stats returns for a bad plan, params, rows, cols, n_cols or
 * background_col; GJ_E_NULL for a NULL new_infected, susceptibility0, infector, via, venue, row_of, counts, unresolved
 * or err, a NULL current_stage with has_quarantine, a NULL transmission or venue_rows with n_nets > 0, v_rowptr without
 * v_agent; GJ_E_RANGE for agent_offset < 0 or agent_offset + n_agents > INT32_MAX.                                        */
#define GJ_TREE_MAX_VENUE_ROW (1 << 18)
typedef struct gj_venue_rows {
  const int32_t* v_rowptr;  /* device [n_venues+1] or NULL: no rows, an infection through this set stays unresolved */
  const int32_t* v_agent;   /* device [n_edges]                                                                     */
} gj_venue_rows;
int gj_infection_tree(const gj_plan* plan, const gj_step_params* params, const gj_location_rows* rows /* [plan->n_sets] */,
                      const gj_venue_rows* venue_rows /* [plan->n_sets] */, const float* new_infected,
                      const float* susceptibility0, const float* current_stage, const float* transmission,
                      const int32_t* cols /* host [n_nets] */, int32_t n_cols, int32_t background_col, uint64_t seed,
                      uint64_t step, int64_t agent_offset, int32_t* infector, int32_t* via, int32_t* venue,
                      int32_t* row_of, int32_t row_value, int64_t* counts, int64_t* unresolved, uint32_t* err,
                      void* stream);

/* ---- row f3: adjoint (backward) of one hot-path step, forward-only kernels reused ---------------
 * The aggregation ts = susc * sum_n w_n * (M_n^T diag(beta_n p_contact) M_n)(m_n * transmission) is
 * self-adjoint up to the exchange of the masks m_n <-> w_n, so its backward is the same four tiled
 * phases run with gj_step_params.transpose = 1 on the vector susc0 * ts_bar.  What remains is
 * elementwise:
 * gj_adjoint_sample: through infect_people (model.py:103-110), the straight-through Gumbel-softmax
 *   (infection.py:13-18) and clamp/exp/clamp (base.py:136-140).  Inputs: the step's pre-state, `acc`
 *   (= pre-susceptibility sum, i.e. gj_agent_gather's trans_susc run with susceptibility == 1), the
 *   step's noise (or Philox key) and the gradients w.r.t. the step's outputs (NULL = zeros).
 *   Outputs: x_out = susc0 * ts_bar (input of the transposed passes), grad_susc_out (complete),
 *   grad_time_out = g_time * (1 - new_infected).
 *   Per agent, with the rules of gj_adjoint_seed below: ts = susc0 * acc and the clamp's mask 1e-6f <= ts <= 100f are
 *   taken in fp32 (ts_bar is 0 outside it and for a NaN ts); d nu / d p is 0 where it is not finite (p == 0 or 1
 *   after rounding, a NaN softmax: torch's autograd gives NaN there); the subgradient of max(0, susc0 - nu) is 0.5
 *   at the tie.  All in fp32: against fp64, ts_bar is good to about 2^-24 * (50 L + 10 (|ln p| + 2) / (1 - p)) relative,
 *   L the sum of the four |ln| of p, 1 - p and the two draws, and is 0 where y0 * y1 underflows fp32
 *   (tests/gj_sampler_ref.py: the bound, per agent; measured in tests/test_gpu_sampler_kernels.py).
 * gj_adjoint_transmission: through the transmission profile (transmission.py:39-51):
 *   grad_inf_out = g_inf + trans_bar * d trans/d is_infected;
 *   grad_time_inout += trans_bar * d trans/d infection_time.
 * gj_adjoint_transmission_params (ABI 7): the same two outputs, bit for bit, plus the gradients w.r.t. the profile's
 *   own per-agent parameters (the reference draws them with rsample, transmission.py:15-20, so a calibration can
 *   differentiate the distributions' loc / scale through them):  grad_<p>_out[a] = trans_bar[a] * d trans[a] / d p[a]
 *   with d = t - shift, u = d * rate:  d/d max_infectiousness = sign * aux * aux2 * is_infected,
 *   d/d shape = trans * (ln u - digamma(shape)), d/d rate = trans * (shape / rate - d),
 *   d/d shift = trans * (rate - (shape - 1) / d); 0 where is_infected == 0.  Each of the four outputs may be NULL:
 *   a NULL output is neither computed nor written.
 *   d == 0 (t == shift exactly; both entry points): d trans/d t is not taken through the division but as torch's
 *   autograd gives it, max_inf * sign / Gamma(shape) * aux2 * is_infected * rate * (shape - 1) * pow(0, shape - 2)
 *   - rate * trans with a zero exponent contributing 0: -rate * trans at shape 1, max_inf * rate^2 * is_infected at
 *   shape 2, 0 above - finite for every integer shape.                                                */
int gj_adjoint_sample(int64_t n, const float* susceptibility0, const float* infection_time0, const float* acc,
                      const float* exp_noise, uint64_t seed, uint64_t step, int64_t agent_offset, float now,
                      float delta_time, const float* g_susc, const float* g_inf, const float* g_time,
                      const float* g_new, float* x_out, float* grad_susc_out, float* grad_time_out,
                      void* stream);
int gj_adjoint_transmission(int64_t n, const gj_agent_state* state0, float now, const float* trans_bar,
                            const float* g_inf, float* grad_inf_out, float* grad_time_inout, void* stream);
int gj_adjoint_transmission_params(int64_t n, const gj_agent_state* state0, float now, const float* trans_bar,
                                   const float* g_inf, float* grad_inf_out, float* grad_time_inout,
                                   float* grad_max_infectiousness_out, float* grad_shape_out, float* grad_rate_out,
                                   float* grad_shift_out, void* stream);

/* gj_adjoint_seed: adjoint of the seed - gj_sample_infect on p_not[a] = p_not_by_group[group[a]] (the per-group
 * probability of NOT being an initial case, 1 - fraction) - w.r.t. each group's fraction.  A pure addition to ABI 7.
 * Per agent, with the rules of gj_adjoint_sample (one shared device function): the draws (e0, e1) from exp_noise or
 * exp_pair(seed, step, agent_offset + a); y0, y1 the tau = 0.1 softmax terms; nu the forward's decision; h the
 * subgradient of max(0, susceptibility0 - nu) (0.5 at the tie);
 *   nu_bar = g_inf + g_time * (now - infection_time0) - g_susc * h + g_new
 *   d nu / d p = -(y0 * y1 / 0.1) * (1/p + 1/(1-p)), 0 where that is not finite
 *   c_a = -nu_bar * d nu / d p                       (d fraction = -d p)
 *   grad_fraction[g] = sum over agents with group[a] == g of c_a                   (device double [n_groups])
 *   grad_susc_out[a] = g_susc * h,  grad_time_out[a] = g_time * (1 - nu)            (each may be NULL: not written)
 * g_* : device fp32 [n], NULL = zeros.  group: device int32 [n]; NULL = every agent in group 0 (n_groups must be 1,
 * `plan` is not read).  An agent whose label is outside [0, n_groups) was not seeded: it contributes nothing, its
 * nu is 0, and the label is never used as an index.
 * The sums are taken in fp64 without atomics, in an order fixed by the labels alone, so the same inputs give the same
 * bits from launch to launch: `plan` lists the agents with a valid label sorted by label (stable) and cuts every
 * group's segment into chunks of GJ_SEED_CHUNK agents; one wave adds a chunk (each lane its terms in list order,
 * then a butterfly over the lanes) into partial_workspace[chunk], then one wave per group adds its chunks the same
 * way.  The tables are built once per labelling (groups.SeedPlan); a kernel checks every index it reads from them.
 * Arithmetic: nu is taken in the forward's fp32 arithmetic, so it IS the forward's decision; h, nu_bar, d nu / d p
 * and c_a are evaluated in fp64 from the fp32 inputs.  (The logarithms' rounding errors are multiplied by 1 / tau = 10
 * on their way into y0 * y1: in fp32 a single agent's term is good to a few 1e-6 only, and underflows where fp64 does
 * not.)  Of the library's own draws, theta and s are fp32 as everywhere; e0 = theta * s and e1 = (1 - theta) * s are
 * formed in fp64, where the products are exact, so the last bit of s cancels in log e0 - log e1.
 * contrib_workspace: device double [n].  partial_workspace: device double [plan->n_chunks], or
 * [(n + GJ_SEED_CHUNK - 1) / GJ_SEED_CHUNK] when group is NULL.                                                  */
#define GJ_SEED_CHUNK 1024
typedef struct gj_seed_plan {
  int64_t n_sorted;            /* agents with a label in [0, n_groups)                                          */
  int64_t n_chunks;            /* sum over groups of ceil(size / GJ_SEED_CHUNK)                                 */
  const int64_t* order;        /* device [n_sorted]: agent indices, stable sort by label                        */
  const int64_t* seg_offsets;  /* device [n_groups + 1]: group g is order[seg_offsets[g] .. seg_offsets[g+1])   */
  const int64_t* chunk_first;  /* device [n_groups + 1]: group g owns chunks chunk_first[g] .. chunk_first[g+1] */
  const int32_t* chunk_group;  /* device [n_chunks]: the group of every chunk                                   */
} gj_seed_plan;
int gj_adjoint_seed(int64_t n, const float* p_not_by_group, const int32_t* group, int32_t n_groups,
                    const gj_seed_plan* plan, const float* susceptibility0, const float* infection_time0,
                    const float* exp_noise, uint64_t seed, uint64_t step, int64_t agent_offset, float now,
                    const float* g_susc, const float* g_inf, const float* g_time, const float* g_new,
                    double* contrib_workspace, double* partial_workspace, double* grad_fraction, float* grad_susc_out,
                    float* grad_time_out, void* stream);

/* ---- vaccination: an age-banded rollout that lowers susceptibility, differentiable in the efficacy ----------------
 * A pure addition to ABI 7 (not in the reference, whose policies never touch the susceptibility).  One campaign gives
 * every agent ONE uniform for the whole run, u = infection_uniform(seed, stream, agent_offset + a) - the forward
 * sampler's device function: word (id & 3) of the Philox block (id >> 2, stream), so a partitioned run decides as one
 * GPU does; the caller keeps `stream` apart from the step streams (policies.py: bit 61 set, the campaign's index
 * below).  A launch moves the agents of one slice of the rollout,
 *   newly = thr_lo[age] <= u && u < thr_hi[age]                 (age = agent_class % 100)
 *   susceptibility[a] *= factor[age]   where newly              (an fp32 multiply, in place; stored only where a lane's
 *                                                                 agents changed)
 * The three per-age tables are formed by the host, each value rounded once: a threshold is fp32(fp64(coverage[age]) *
 * ramp) and a factor fp32(1 - fp64(efficacy of the age's band)).  The kernel only compares and multiplies, so a numpy
 * restatement gives its bits (tests/gj_vaccination_ref.py).  Thresholds that rise from launch to launch make the
 * rollout monotone without per-agent state: the slices [lo, hi) of a run tile [0, final).  A NaN threshold moves
 * nobody.
 * newly_out:  device fp32 [n], 0 / 1, or NULL.   count_out: device int64 [1], the launch ADDS its number of newly
 * vaccinated agents (an integer atomic: exact in any order), or NULL.
 * Where agent_offset is a multiple of 4 and the arrays are 16-byte (agent_class: 4-byte) aligned, a lane takes four
 * consecutive agents, which share one Philox block; otherwise one agent per lane.  Both forms give the same bits.   */
typedef struct gj_vaccinate_tables {
  float thr_lo[100];           /* per age: the rollout reached u < thr_lo before this launch                    */
  float thr_hi[100];           /* ... and reaches u < thr_hi with it                                            */
  float factor[100];           /* per age: 1 - efficacy (1 for an age in no band)                               */
} gj_vaccinate_tables;
int gj_vaccinate(int64_t n, const uint8_t* agent_class, const gj_vaccinate_tables* tables /* host */, uint64_t seed,
                 uint64_t stream, int64_t agent_offset, float* susceptibility, float* newly_out, int64_t* count_out,
                 void* hip_stream);

/* gj_adjoint_vaccinate: adjoint of gj_vaccinate w.r.t. the incoming susceptibility and the efficacy of each band.
 * The decision inputs are the forward's and `newly` is the forward's rule (one shared device function);
 * susceptibility0: the PRE-update values; g_out: the cotangent of the updated susceptibility (device fp32 [n], NULL =
 * zeros); band: device int32 [n], each agent's efficacy band, or a label outside [0, n_bands) for none.
 *   g_in[a]          = g_out[a] * (newly ? factor[age] : 1)                                   (fp32; g_in may be NULL)
 *   grad_efficacy[b] = sum over agents with band[a] == b and newly of -g_out[a] * susceptibility0[a]
 *                                                                              (device double [n_bands]; d factor = -d efficacy)
 * The terms are formed in fp64 from the fp32 inputs (the products are exact) and summed without atomics in the order
 * `plan` fixes - a gj_seed_plan built on `band` (groups.SeedPlan), read exactly as gj_adjoint_seed reads it, through
 * the same two kernels - so two launches on the same inputs give the same bits.  An agent with no band contributes
 * nothing and its label is never used as an index.  contrib_workspace: device double [n]; partial_workspace: device
 * double [plan->n_chunks].                                                                                          */
int gj_adjoint_vaccinate(int64_t n, const uint8_t* agent_class, const gj_vaccinate_tables* tables /* host */,
                         uint64_t seed, uint64_t stream, int64_t agent_offset, const float* susceptibility0,
                         const float* g_out, const int32_t* band, int32_t n_bands, const gj_seed_plan* plan,
                         double* contrib_workspace, double* partial_workspace, double* grad_efficacy, float* g_in,
                         void* hip_stream);

/* ---- waning immunity: recovered agents become susceptible again, differentiable in half-life and residual ----------
 * A pure addition to ABI 7 (not in the reference, where an infected agent's susceptibility stays 0 for good).  One
 * launch AFTER a step and BEFORE the symptoms update, on the stage the step started from.  Per agent, with
 * age = agent_class % 100 and nu = new_infected[a] != 0 (new_infected NULL: nobody):
 *   reinfected = nu && is_infected[a] - new_infected[a] >= 1          (the agent had an infection before this one)
 *       is_infected[a] -= new_infected[a]      the step's increment is undone (exact in fp32), so is_infected stays the
 *                                               0 / 1 flag the transmission profile multiplies by
 *   waned = current_stage[a] == recovered_stage && !nu && keep[age] != 1
 *       susceptibility[a] = cap[age] - (cap[age] - susceptibility[a]) * keep[age]      three fp32 operations, no contraction
 *   everybody else: nothing is written.  A NaN stage is not recovered; a NaN susceptibility stays NaN; a value above cap
 *   relaxes downward; there is no clamp.
 * The two per-age tables are formed by the host, each value rounded once: keep = fp32(2^(-dt / half_life)) (1 for an
 * infinite half-life and for an age in no band) and cap = fp32(1 - fp64(fp32(residual_protection))).  From 0 at recovery
 * the susceptibility is cap * (1 - 2^(-(t - t_rec) / half_life)) whatever the step lengths.  The kernel only subtracts and
 * multiplies, so a numpy float32 restatement gives its bits (tests/gj_immunity_ref.py).
 * Optional outputs (each may be NULL: not written):
 *   flags_out       device uint8 [n]: bit 0 waned, bit 1 reinfected (what gj_adjoint_immunity replays)
 *   reinfected_out  device fp32 [n], 0 / 1
 *   count_out       device int64 [1]: the launch ADDS its number of reinfected agents
 *   susc_sum_out    device int64 [1]: the launch ADDS sum over agents of (int64)(fmin(fmax(s', 0), 4) * 2^30), s' the
 *                   susceptibility after the launch (NaN counts 0).  Scaling and truncation are exact and the sum is an
 *                   integer one: no order shows.  With it every agent's susceptibility is read.
 * susceptibility is loaded only where a lane holds a waning agent (or susc_sum_out is given) and stored only where a lane
 * changed it; is_infected is loaded only by lanes that hold a new infection.  Four agents per lane where the fp32 arrays
 * are 16-byte and agent_class / flags_out 4-byte aligned, one per lane otherwise; both forms give the same bits.      */
typedef struct gj_immunity_tables {
  float cap[100];              /* per age: 1 - residual_protection of the age's band (1 for an age in no band)      */
  float keep[100];             /* per age: 2^(-dt / half_life) (1: the age does not wane)                          */
} gj_immunity_tables;
int gj_immunity_step(int64_t n, const uint8_t* agent_class, const gj_immunity_tables* tables /* host */,
                     const float* current_stage, int32_t recovered_stage, const float* new_infected,
                     float* susceptibility, float* is_infected, uint8_t* flags_out, float* reinfected_out,
                     int64_t* count_out, int64_t* susc_sum_out, void* hip_stream);

/* gj_adjoint_immunity: adjoint of gj_immunity_step w.r.t. its three per-agent inputs and, per band, the two sums the
 * host turns into d loss / d half_life and d loss / d residual_protection.  flags: the forward's flags_out;
 * susceptibility0: the PRE-update values; g_susc / g_inf: the cotangents of the updated arrays (device fp32 [n], NULL =
 * zeros); band: device int32 [n], or a label outside [0, n_bands) for none.
 *   g_susc_in[a] = waned ? g_susc[a] * keep[age] : g_susc[a]       g_inf_in[a] = g_inf[a]
 *   g_new[a]     = reinfected ? -g_inf[a] : 0                       (fp32; each of the three may be NULL: not written)
 *   sum_A[b] = sum over waned agents of band b of g_susc[a] * (cap[age] - susceptibility0[a])     (device double [n_bands])
 *   sum_B[b] = sum over waned agents of band b of g_susc[a]                                      (device double [n_bands])
 * so that, with keep = 2^(-dt / h):  d loss / d h = -sum_A * keep * ln 2 * dt / h^2,  d loss / d r = -sum_B * (1 - keep).
 * cap - susceptibility0 is the forward's fp32 difference; its product with g_susc is formed in fp64, where the product
 * of two fp32 values is exact.  The terms are summed without atomics in the order `plan` fixes, through gj_adjoint_seed's
 * two summing kernels, once for each sum: two launches on the same inputs give the same bits.  An agent with no band
 * contributes nothing and its label is never used as an index.  contrib_workspace: device double [2 * n] (A's terms,
 * then B's); partial_workspace: device double [2 * plan->n_chunks].                                                   */
int gj_adjoint_immunity(int64_t n, const uint8_t* flags, const uint8_t* agent_class,
                        const gj_immunity_tables* tables /* host */, const float* susceptibility0, const float* g_susc,
                        const float* g_inf, const int32_t* band, int32_t n_bands, const gj_seed_plan* plan,
                        double* contrib_workspace, double* partial_workspace, double* sum_A, double* sum_B,
                        float* g_susc_in, float* g_inf_in, float* g_new, void* hip_stream);

/* ---- contact quarantine: the household and venue contacts of symptomatic agents stay away ----------------------------
 * A pure addition to ABI 7 (not in the reference, whose Quarantine isolates the symptomatic agent alone).  Two launches
 * BEFORE a step turn its current_stage into a per-agent mask `qstate` that the step then takes in the place of the stage,
 * with q_threshold = 0.5; the step's kernels do not change.  Per traced edge set the caller keeps one uint32 per venue,
 * `until`: the fp32 bit pattern of the time up to which the venue's members are held, 0 = never marked.  The values are
 * non-negative, so their order as unsigned integers is their order as floats.
 *   gj_contact_mark:  for every agent a with !(current_stage[a] < stage_threshold)  (a NaN stage is an index case, as in
 *                     the step), every set s and every venue v of a in s:  until_s[v] = max(until_s[v], bits(release_s))
 *                     - an unsigned integer atomic max: exact, and no order of the agents shows.  release_s =
 *                     fp32(now + days_s) is formed once by the host; only index agents walk their rows.
 *   gj_contact_mask:  qstate[a] = 1   if !(current_stage[a] < q_threshold)                              (index case)
 *                               = 2   else if u < compliance and float(until_s[v]) > now for a venue v of a in a set s
 *                               = 0   otherwise                                                         (free)
 *                     u = infection_uniform(seed, stream, agent_offset + a): ONE uniform per agent for the whole run, as
 *                     gj_vaccinate draws it; the caller keeps `stream` apart from the other streams (policies.py: bit 59
 *                     set, the policy's index below).  Index agents and agents that do not comply walk no row.
 * The kernels only compare, so a numpy restatement gives their bits (tests/gj_contact_ref.py).  The stage is read
 * coalesced, four agents per lane where the per-agent arrays are 16-byte aligned (mask: and agent_offset is a multiple of
 * 4, the quad then shares one Philox block), one per lane otherwise; both forms give the same bits.
 * a_rowptr / a_venue: the set's edges as CSR by owned agent (gj_location_rows' arrays); a_venue holds a_rowptr[n]
 * entries.  Bad input never becomes an index: a row that is negative, decreasing or beyond a_rowptr[n], and a venue id
 * outside [0, n_venues), is skipped and sets GJ_CONTACT_ERR_ROWS.  *err (device uint32) is sticky until the caller
 * clears it.
 * Returns GJ_E_RANGE for n < 0, agent_offset < 0, n_sets outside 1 .. GJ_MAX_SETS, an n_venues outside 0 .. INT32_MAX
 * and (mark) a release that is negative or NaN; GJ_E_NULL for a NULL `sets`, `err`, array of a set, or per-agent array
 * with n > 0 - all before any device work.  n == 0 launches nothing.                                                    */
#define GJ_CONTACT_ERR_ROWS 4u
typedef struct gj_contact_set {
  const int32_t* a_rowptr;     /* device [n + 1]: the set's edges as CSR by owned agent (gj_location_rows' arrays) */
  const int32_t* a_venue;      /* device [edges]                                                                  */
  uint32_t* until;             /* device [n_venues]                                                               */
  int64_t n_venues;
  float release;               /* fp32(now + days) of this launch (gj_contact_mask does not read it)              */
} gj_contact_set;
int gj_contact_mark(int64_t n, const float* current_stage, float stage_threshold,
                    const gj_contact_set* sets /* host */, int32_t n_sets, uint32_t* err, void* stream);
int gj_contact_mask(int64_t n, const float* current_stage, float q_threshold,
                    const gj_contact_set* sets /* host */, int32_t n_sets, float now, float compliance,
                    uint64_t seed, uint64_t stream, int64_t agent_offset, float* qstate, uint32_t* err,
                    void* hip_stream);

/* ---- testing: confirmed cases with a reporting delay, isolation on a positive result ------------------------------------
 * A pure addition to ABI 7 (not in the reference, whose Quarantine finds every symptomatic agent at once).  One launch
 * BEFORE a step, on the current_stage the step starts from, keeps five per-agent arrays (20 B an agent, the caller's):
 *   decided        uint32  bits of the infection_time the agent's decision was made for      (start: 0xFFFFFFFF)
 *   result_time    fp32    when the result is due                                            (start: +inf)
 *   positive       fp32    0 / 1                                                             (start: 0)
 *   isolate_until  fp32    end of the isolation; NULL for a policy that does not isolate     (start: 0)
 *   confirmed_time fp32    when the case was confirmed                                       (start: -1, never)
 * Per agent, with age = agent_class % 100 and g = agent_offset + a, in this order:
 *   decide  if active && !(current_stage[a] < stage_threshold) && bits(infection_time[a]) != decided[a]   (a NaN stage
 *           qualifies, as in the step; 0.0 and -0.0 are two infections):
 *             decided[a] = bits(infection_time[a]);  r = Philox4x32-10(counter = (g, decide_stream | bits), key = seed)
 *             - ONE block per decision, the agent's own: the counter's low half is g itself, not g >> 2, because the
 *             decision takes two words;  positive[a] = u01(r[0]) < probability[age];  d = days[k], k the first entry
 *             with cum[k] > u01(r[1]), the last entry where there is none;  result_time[a] = now + d  (one fp32 add)
 *   report  if result_time[a] <= now:  result_time[a] = +inf, and where positive[a]: the case is newly confirmed,
 *           confirmed_time[a] = now, and, where isolate_until is given and infection_uniform(seed, comply_stream, g) <
 *           compliance (ONE uniform per agent for the whole run, as gj_contact_mask draws it),  isolate_until[a] =
 *           isolate_release - fp32(now + days), formed once by the host.  A delay of 0 reports in the deciding launch.
 *   mask    where qstate_out is given:  qstate[a] = 1 if !(current_stage[a] < q_threshold), else 3 if now <
 *           isolate_until[a], else 0 - what the step then takes in the place of the stage with q_threshold = 0.5.
 * The three tables are formed by the host, each value rounded once; the kernel compares and adds once, so a numpy
 * restatement gives its bits (tests/gj_testing_ref.py).  Nothing is stored where nothing changed.
 * Optional outputs (each may be NULL: not written):
 *   newly_confirmed_out  device fp32 [n], 0 / 1
 *   qstate_out           device fp32 [n]; needs isolate_until
 *   flags_out            device uint8 [n]: GJ_TESTING_DECIDED | GJ_TESTING_POSITIVE (the value of `positive` of an agent
 *                        that decided or reported) | GJ_TESTING_DUE - what gj_adjoint_testing replays
 *   counts_out           device int64 [2]: the launch ADDS its newly confirmed cases to [0] and its decisions to [1]
 * Four agents per lane where the 4-byte arrays are 16-byte and agent_class / flags_out 4-byte aligned, one per lane
 * otherwise; both forms give the same bits.
 * Returns GJ_E_RANGE for n < 0, agent_offset < 0, n_delays outside 1 .. GJ_TESTING_MAX_DELAYS, a `now` that is negative
 * or NaN and a decide_stream with any of its low 32 bits set; GJ_E_NULL for a NULL `tables`, a NULL required array with
 * n > 0, and qstate_out without isolate_until - all before any device work.  n == 0 launches nothing.                */
#define GJ_TESTING_MAX_DELAYS 16
#define GJ_TESTING_DECIDED 1u
#define GJ_TESTING_POSITIVE 2u
#define GJ_TESTING_DUE 4u
typedef struct gj_testing_tables {
  float probability[100];                 /* per age: the chance that an infection is found (0 for an age in no band) */
  float delay_cum[GJ_TESTING_MAX_DELAYS]; /* cumulative shares of the delays, fp32 each                               */
  float delay_days[GJ_TESTING_MAX_DELAYS];
  int32_t n_delays;
  int32_t _pad;
} gj_testing_tables;
int gj_testing_step(int64_t n, const uint8_t* agent_class, const gj_testing_tables* tables /* host */,
                    const float* current_stage, const float* infection_time, float stage_threshold, int32_t active,
                    float now, float q_threshold, float isolate_release, float compliance, uint64_t seed,
                    uint64_t decide_stream, uint64_t comply_stream, int64_t agent_offset, uint32_t* decided,
                    float* result_time, float* positive, float* isolate_until, float* confirmed_time,
                    float* newly_confirmed_out, float* qstate_out, uint8_t* flags_out, int64_t* counts_out,
                    void* hip_stream);

/* gj_adjoint_testing: adjoint of one gj_testing_step, whose `positive` travels on the graph as y: a deciding agent's
 * y = hard * stage / stage.detach() (the reference's own form for deaths), everybody else's y is the incoming one, and
 * the launch's row is sum over due agents of y.  flags: the forward's flags_out; g_y: the cotangent of the outgoing y
 * (device fp32 [n], NULL = zeros); g_row: the cotangent of the row (device fp32 [1], NULL = zero); band: device int32
 * [n], each agent's probability band, or a label outside [0, n_bands) for none.  With g = g_y[a] + (due ? *g_row : 0):
 *   g_stage[a] = decided ? g * hard / current_stage[a] : 0        g_y_in[a] = decided ? 0 : g       (fp32; each may be NULL)
 *   grad_probability[b] = sum over deciding agents of band b of g      (device double [n_bands]; d y / d probability := 1
 *                         for every deciding agent, positive or negative: a straight-through estimator whose sum is the
 *                         exact derivative of the expected count)
 * The terms are summed in fp64 without atomics in the order `plan` fixes, through gj_adjoint_seed's two summing kernels:
 * two launches on the same inputs give the same bits.  contrib_workspace: device double [n]; partial_workspace: device
 * double [plan->n_chunks].                                                                                            */
int gj_adjoint_testing(int64_t n, const uint8_t* flags, const float* current_stage, const float* g_y, const float* g_row,
                       const int32_t* band, int32_t n_bands, const gj_seed_plan* plan, double* contrib_workspace,
                       double* partial_workspace, double* grad_probability, float* g_stage, float* g_y_in,
                       void* hip_stream);

/* d loss / d log_beta of the networks on ONE edge set, from the forward's and the transposed passes' per-venue sums:
 *   col0 + k :  ln(10) * scale * sum_v [p_contact[v] > 0]  cum_fwd[v][k] * cum_bwd[v][k] / (beta[k] * p_contact[v]) * weight[v]
 * (reference: autograd through base.py:36-42,78-83; `weights` - fp64 [n_venues] or NULL = 1 - is a rank's share of
 * each venue in a multi-GPU run).  Two launches, deterministic: gj_adjoint_beta_partial ADDS every workgroup's fp64
 * partial sums into partial[GJ_ADJ_BETA_BLOCKS][GJ_MAX_NETS] (zeroed by the caller before a step's first set; a twin
 * network on the second half of a split set adds into its network's column), gj_adjoint_beta_finish sums the rows in
 * order into out[0 .. n_cols) and applies ln(10) * *scale (a device float: the power of two the cotangent was
 * normalised by).  beta[k] == 0 contributes 0.                                                                   */
#define GJ_ADJ_BETA_BLOCKS 256
int gj_adjoint_beta_partial(int64_t n_venues, int32_t stride, int32_t nk, const float* cum_fwd, const float* cum_bwd,
                            const float* v_pcontact, const double* weights, const float* beta /* host [nk] */,
                            const int32_t* cols /* host [nk] */, double* partial, void* stream);
int gj_adjoint_beta_finish(int32_t n_cols, const double* partial, const float* scale, double* out, void* stream);

/* gj_adjoint_symptoms: adjoint of gj_symptoms_update - what makes a loss on the symptom stages (the
 * deaths series, grad_june/runner.py:198-215; test/unit/test_runner.py:82-90 and
 * test_symptoms.py:208-231 assert the gradient exists) differentiable w.r.t. log_beta.  Inputs: the
 * PRE-update current / next stage and time_to_next_stage, new_infected, the SAME params (time, seed,
 * step) or the same injected `progresses` + `dwell`, and the gradients w.r.t. the updated current /
 * next stage / time (each may be NULL = 0).  Outputs ([n] each; g_time_in may be NULL): gradients
 * w.r.t. the incoming current stage, next stage, time_to_next_stage and w.r.t. new_infected.  The
 * gradient paths are those of symptoms.py:98,105-124,231-236: next += new*(2-next), time +=
 * new*(now-time), current -= (current-next)*mask, and the value-1 factor (current==i)*current/i on
 * the +1 / -next updates of next_stage and on the dwell time added to time_to_next_stage.          */
int gj_adjoint_symptoms(int64_t n, const uint8_t* agent_class, const float* new_infected,
                        const float* current_stage0, const float* next_stage0, const float* time_to_next_stage0,
                        const gj_symptoms_params* params, const float* progresses, const float* dwell,
                        const float* g_current, const float* g_next, const float* g_time, float* g_current_in,
                        float* g_next_in, float* g_time_in, float* g_new_infected, void* stream);

/* The production step: a1..a9 = the middle of GradJune.forward (grad_june/model.py:125-138)
 * as three dependent launches on `stream` (+1 when the plan has long rows).                */
int gj_step(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params,
            const gj_step_io* io, void* stream);

/* One launch group of gj_step at a time, for per-kernel timing (bench.py brackets each with HIP
 * events): phase 0 = transmission; 1 = pass-1 front (tiled: phase A scatter; CSR: venue reduce);
 * 2 = tiled phases B+C (CSR: nothing); 3 = pass-2 + epilogue + decision + state update.
 * Calling phases 0,1,2,3 in order is exactly gj_step.  Diagnostic variants: 4 = phase 3 without
 * the decision/state update (probabilities only); 5 / 6 = the tiled venue launch split into its
 * B half (sums -> cum) and its C half (cum -> per-edge values) - the multi-GPU step all-reduces
 * cum between the two; 7 = phases 1 then 5, 8 = phases 1 then 2, in one call.                  */
int gj_step_phase(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params,
                  const gj_step_io* io, int phase, void* stream);

/* Narrower copies of arrays the step streams, built ONCE from data that stays the same from step to step (the contact
 * graph).  Every pointer may be NULL: that stream is then read in its original form.
 * A NULL `aux` is gj_step / gj_step_phase exactly; no result depends on it, bit for bit.  A pure addition to ABI 7.
 *   e_lv8[s]           device uint8 [slots of set s, rounded up to 8] = gj_tiled_set.e_lv in one byte per slot, 0xFF
 *                      for the pad value 0xFFFF (gj_narrow_venue_ids), 8-byte aligned.  Only for a set whose every
 *                      block holds at most 255 venues (max_block_venues <= 255, else GJ_E_PLAN): the venue launch of
 *                      the forward step reads it instead of e_lv.  Every other reader keeps the 16-bit array. */
typedef struct gj_aux {
  const uint8_t* e_lv8[GJ_MAX_SETS];
} gj_aux;
int gj_step_aux(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params,
                const gj_step_io* io, const gj_aux* aux, void* stream);
int gj_step_phase_aux(const gj_plan* plan, const gj_agent_state* state, const gj_step_params* params,
                      const gj_step_io* io, const gj_aux* aux, int phase, void* stream);

/* clock->step += 1; clock->now = (float)(now0 + (step - step0) * delta_now), in double: a step length that is not a
 * power of two (hours / 24) does not drift over the replays.  One tiny launch on `stream` (the first node of a
 * captured step).                                                                                                 */
int gj_clock_advance(gj_clock* clock, double delta_now, void* stream);

/* Multi-GPU halo exchange helpers (one process per GPU; the all-to-all itself is issued by
 * the host through torch.distributed/RCCL between the two calls).
 * pack:   out[i] = src[index[i]]            for i < n      (send buffer of owned agents)
 * unpack: dst[index[i]] = in[i]             for i < n      (halo slots of remote agents)   */
int gj_pack_f32(int64_t n, const int32_t* index, const float* src, float* out, void* stream);
int gj_unpack_f32(int64_t n, const int32_t* index, const float* in, float* dst, void* stream);

/* ================= graph compile on the device ("native graph compile") =================
 * The tiled layout of ONE edge set (the arrays of gj_tiled_set) built in HBM from the reference's data format:
 * the unsorted COO `data["attends_<set>"].edge_index` (int64 [2, E]; grad_june/ has no compile step of its own -
 * torch_geometric walks this COO on every propagate, infection_networks/base.py:78-80).  Same arrays, bit for bit, as
 * the numpy specification grad_june_amd/tiling.py (build_tiled, wide_descriptors, build_ell), which documents them.
 * Kernels: key construction, rocPRIM radix sort / scans (hipcub), scatter of the 16-bit local indices, chunk
 * descriptors.  The library allocates nothing: the caller passes every output at its upper-bound size and one
 * workspace (gj_compile_workspace_bytes), reads `counts` (device int32[GJ_COMPILE_COUNTS]) after a stage and trims.
 *   1. gj_compile_blocks        venue degrees, range checks, the venue blocks         -> counts[GJ_CC_BLOCKS] = J
 *   2. gj_compile_tiles         everything else, with 4-word chunk descriptors        -> SLOTS, CHUNKS, MULTI
 *   3. gj_compile_wide_descriptors   (optional) the 8-word descriptor format for sets with small tiles
 *   4. gj_compile_ell_degrees / gj_compile_ell    the ELL rows of the direct form of pass 2
 * counts[GJ_CC_ERROR] != 0 after a stage: 1 agent index out of range, 2 venue index out of range, 3 more venue
 * blocks than blk_cap, 4 wide descriptor field overflow, 5 an owned agent has more edges than ell_k columns (the
 * entry is skipped, nothing is written outside the table).                                                        */
#define GJ_COMPILE_COUNTS 16
#define GJ_CC_BLOCKS 0       /* J: venue blocks                                                        */
#define GJ_CC_SLOTS 1        /* length of the block-major arrays (every block padded to 8 slots)       */
#define GJ_CC_CHUNKS 2       /* 64-edge chunks of the slice-major order                                */
#define GJ_CC_MULTI 3        /* chunks that span more than two tiles (share > 5 %: use wide descriptors; else rows, gj_compile_multi_slots) */
#define GJ_CC_OWNED_EDGES 4  /* edges whose agent is owned (< n_agents)                                */
#define GJ_CC_MAX_DEGREE 5   /* largest number of edges of one owned agent                             */
#define GJ_CC_ERROR 7
#define GJ_CC_RUN_PRIMARY 8   /* gj_compile_runs_pick: owned agents with an edge = primary edges               */
#define GJ_CC_RUN_UNSORTED 9  /* != 0: the owned agents are NOT ordered by their smallest venue - no run form  */
#define GJ_CC_RUN_WINDOW 10   /* venues in the widest slice window                                            */
#define GJ_CC_WIDE_MULTI 11   /* gj_compile_wide_descriptors: chunks that span more than six tiles (share > 2 %:
                                 use gj_compile_explicit_slots)                                             */

typedef struct gj_compile_set {
  const int64_t* agent;        /* [n_edges] edge_index[0]: agent ids, owned then halo, < n_ext_agents            */
  const int64_t* venue;        /* [n_edges] edge_index[1]: venue ids < n_venues                                  */
  const uint8_t* agent_class;  /* [owned + halo agents] or NULL; non-NULL: e_cls is written (leisure sets)        */
  int64_t n_edges;             /* < 2^30                                                                         */
  int64_t n_agents;            /* owned agents (the ELL rows)                                                    */
  int64_t n_ext_agents;        /* owned + halo agents, <= n_slices * slice_agents                                */
  int32_t n_venues;
  int32_t n_slices, slice_agents;   /* S, SA <= 65536                                                            */
  int32_t sv_max, eb_target;        /* venues per block <= 65536, edges per block aimed for                      */
  int32_t n_blocks;                 /* J, as stage 1 returned it (stage 1 itself: ignored)                       */
} gj_compile_set;

typedef struct gj_compile_out {       /* device buffers at their upper-bound sizes, see gj_compile_capacity      */
  int32_t* blk_e0;       /* [J + 1]                                                                              */
  uint16_t* e_lv;        /* [slots_cap]   0xFFFF = pad                                                            */
  uint8_t* e_cls;        /* [slots_cap] or NULL                                                                   */
  uint16_t* a_la;        /* [n_edges]                                                                             */
  int32_t* tile_sptr;    /* [S * J + 1]                                                                           */
  int32_t* tile_jpos;    /* [S * J]                                                                               */
  int32_t* chunk_ptr;    /* [S + 1]                                                                               */
  int32_t* chunk_desc;   /* [chunks_cap * 4]                                                                      */
  int64_t slots_cap, chunks_cap;
} gj_compile_out;

/* Upper bounds for the caller's allocations: blocks (before stage 1), slots and chunks (J known or not).          */
int gj_compile_capacity(const gj_compile_set* set, int64_t* blk_cap, int64_t* slots_cap, int64_t* chunks_cap);
/* Bytes of workspace that suffice for every stage of this set (J = set->n_blocks, or its upper bound when 0).      */
int gj_compile_workspace_bytes(const gj_compile_set* set, int64_t* bytes);
int gj_compile_blocks(const gj_compile_set* set, int32_t* blk_v0 /* [blk_cap + 1] */, int32_t blk_cap,
                      int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);
int gj_compile_tiles(const gj_compile_set* set, const int32_t* blk_v0, const gj_compile_out* out, int32_t* counts,
                     void* workspace, int64_t workspace_bytes, void* stream);
int gj_compile_wide_descriptors(const gj_compile_set* set, const gj_compile_out* out, int32_t n_chunks,
                                int32_t* desc8 /* [n_chunks * 8] */, int32_t* counts, void* stream);
/* degree[a] (int32 [n_agents + 1], caller-owned) = edges of owned agent a; counts[OWNED_EDGES], counts[MAX_DEGREE]. */
int gj_compile_ell_degrees(const gj_compile_set* set, int32_t* degree, int32_t* counts, void* stream);
/* ell: uint16 [ell_k / 2 planes][rows][2] (gj_tiled_set.ell), rows = owned slices * slice_agents; `degree` as
 * returned by gj_compile_ell_degrees; ell_k >= counts[GJ_CC_MAX_DEGREE] (checked per entry: counts[GJ_CC_ERROR] = 5
 * when an agent does not fit; `counts` may be NULL).                                                               */
int gj_compile_ell(const gj_compile_set* set, int32_t ell_k, int64_t rows, const int32_t* degree, uint16_t* ell,
                   void* workspace, int64_t workspace_bytes, int32_t* counts, void* stream);

/* (optional, after gj_compile_tiles) the explicit-slot form of a set with tiles of a few edges: slots[i] (int32 [E]) = the
 * block-major slot of slice-major edge i; gj_tiled_set.desc_wide = 2 and chunk_desc = slots.                       */
int gj_compile_explicit_slots(const gj_compile_set* set, const gj_compile_out* out, int32_t* slots, void* stream);
/* (after gj_compile_tiles / gj_compile_wide_descriptors, for a set NOT in the explicit-slot form) the chunks a descriptor
 * cannot express - counts[GJ_CC_MULTI] of the 4-word form, counts[GJ_CC_WIDE_MULTI] of the 8-word form = `n_multi` - get
 * a row of 64 explicit slots each, in chunk order (gj_tiled_set.multi_slots, int32 [n_multi * 64], caller-owned; lanes
 * past a chunk's end: 0), and their descriptors the row number in the j0 field.  `desc` = the descriptors in use
 * ([n_chunks * 4] or, `wide` != 0, [n_chunks * 8]); workspace >= 2 * (n_chunks + 1) * 4 bytes + 64 KiB.
 * Specification: tiling.attach_multi_slots.  (ABI 6; before, such a chunk's lanes walked the tile tables.)              */
int gj_compile_multi_slots(const gj_compile_set* set, const gj_compile_out* out, int32_t n_chunks, int32_t wide,
                           int32_t* desc, int32_t n_multi, int32_t* multi_slots, int32_t* counts, void* workspace,
                           int64_t workspace_bytes, void* stream);
/* (after the compile, for a set whose every block holds at most 255 venues) gj_aux.e_lv8:
 * e_lv8[i] = e_lv[i] == 0xFFFF ? 0xFF : (uint8_t)e_lv[i] for i < n_slots.  The caller decides eligibility from blk_v0. */
int gj_narrow_venue_ids(int64_t n_slots, const uint16_t* e_lv, uint8_t* e_lv8, void* stream);

/* ---- run form of the set that orders the agents (gj_tiled_set.run_*; specification: tiling.split_primary_runs /
 * finish_run_form).  Three steps around the compile of the set's remaining edges:
 *   gj_compile_runs_pick   vmin[a] (int32 [n_agents], 0x7FFFFFFF = no edge), pick[a] (COO position of the agent's
 *                          primary edge: the first edge to its smallest venue), keep[e] (uint8 [E]: 1 = the edge stays
 *                          in the tiled arrays), the slices' windows (int32 [owned slices] each) and
 *                          counts[RUN_PRIMARY / RUN_UNSORTED / RUN_WINDOW / OWNED_EDGES] - the caller decides;
 *   gj_compile_runs_rest   the kept edges, compacted in COO order (int64 [E - primary] each) - the input of
 *                          gj_compile_blocks / _tiles for this set;
 *   gj_compile_runs_index  once the venue blocks are known: run_pv_blk, run_pv_win (uint16 [rows]), run_blk_r0.     */
int gj_compile_runs_pick(const gj_compile_set* set, int32_t* vmin, int32_t* pick, uint8_t* keep, int32_t* win_lo,
                         int32_t* win_n, int32_t* counts, void* stream);
int gj_compile_runs_rest(const gj_compile_set* set, const uint8_t* keep, int64_t* agent_out, int64_t* venue_out,
                         void* workspace, int64_t workspace_bytes, int32_t* counts, void* stream);
int gj_compile_runs_index(const gj_compile_set* set, const int32_t* vmin, const int32_t* blk_v0, int32_t n_blocks,
                          int64_t rows, const int32_t* win_lo, uint16_t* pv_blk, uint16_t* pv_win, int32_t* blk_r0,
                          void* stream);

/* Average device time of the last-timed dominant kernel is measured by the caller with
 * hipEvents; these two helpers let a ctypes caller do that on the stream it launches on
 * (torch.cuda.Event only sees torch's current stream).                                      */
int gj_event_create(void** event);
int gj_event_record(void* event, void* stream);
int gj_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop`       */
int gj_event_destroy(void* event);

#ifdef __cplusplus
}
#endif
#endif /* GRADJUNE_HIP_H */
