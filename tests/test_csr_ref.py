"""CPU: the restatement of the CSR layout's two passes (tests/gj_csr_ref.py) checked without a device, on the worlds of
tests/test_gpu_csr_kernels.py:

  * where every block sums with one lane and no venue is long, it IS torch's CPU scatter_add_ in COO order, bit for bit
    (the claim of plan.py's docstring), per venue and per agent;
  * on dyadic inputs it equals the float64 sums exactly, in every block form: which edges and which factors enter;
  * on general inputs it lies inside bounds that follow from float32 alone;
  * the facts about build_schedule that it relies on and that tests/test_plan_host.py does not already assert.
"""
import numpy as np
import pytest
import torch

import gj_csr_ref as RC
import test_gpu_csr_kernels as G
from grad_june_amd import _native as N
from grad_june_amd.plan import LONG_CHUNK, MAX_ROWS_PER_BLOCK, NetworkSpec, build_schedule, compile_plan

F32 = np.float32
U = 2.0 ** -24           # unit roundoff of float32, round to nearest


def test_constants_are_the_library_s():
    assert (RC.STREAM_EDGES, RC.MAX_SETS, RC.MAX_NETS, RC.MAX_NETS_PER_SET, RC.TABLE_SIZE) == (
        N.GJ_STREAM_EDGES, N.GJ_MAX_SETS, N.GJ_MAX_NETS, N.GJ_MAX_NETS_PER_SET, N.GJ_TABLE_SIZE)
    assert (RC.MASK_RAW, RC.MASK_Q, RC.MASK_QL, RC.MASK_QL_AGE75) == (N.MASK_RAW, N.MASK_Q, N.MASK_QL, N.MASK_QL_AGE75)
    assert RC.THREADS * 8 == N.GJ_STREAM_EDGES and LONG_CHUNK % (4 * RC.THREADS) == 0


def test_every_form_is_reached_on_the_host_plans():
    G.forms_reached()


def test_ordered_sums_add_one_after_the_other():
    rng = np.random.default_rng(1)
    t = rng.uniform(0.0, 1.0, 5000).astype(np.float32)
    first, count = np.array([0, 7, 100, 4000, 4999, 10]), np.array([7, 93, 3000, 999, 1, 0])
    got = RC.ordered_sums(t, first, count)
    for f, c, g in zip(first, count, got):
        want = np.cumsum(t[f:f + c], dtype=np.float32)[-1] if c else F32(0.0)       # cumsum on float32 is sequential
        assert RC.bits(g) == RC.bits(want)
    assert RC.bits(got[2]) != RC.bits(np.sum(t[100:3100]))                          # np.sum adds pairwise: another value
    lanes = RC.ordered_sums(t, 20 + np.arange(4), RC.strided_counts(np.array([11]), 4)[0], 4)
    for lane in range(4):
        assert RC.bits(lanes[lane]) == RC.bits(np.cumsum(t[20 + lane:31:4], dtype=np.float32)[-1])
    assert RC.strided_counts(np.array([0, 1, 4, 5, 1025]), 4).tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1], [2, 1, 1, 1],
                                                                           [257, 256, 256, 256]]
    p = rng.uniform(0.0, 1.0, (3, 4)).astype(np.float32)
    want = (p[:, 0] + p[:, 2]) + (p[:, 1] + p[:, 3])                                # off = 2, then off = 1, as lane 0 sees it
    assert np.array_equal(RC.bits(RC.butterfly(p)), RC.bits(want))


# ---- torch's order --------------------------------------------------------------------------------------------------------
def test_one_lane_blocks_have_torch_s_scatter_add_order():
    """A world whose blocks all sum with one lane: cum per venue and trans_susc per agent (one plain network) equal
    torch's own CPU scatter_add_ over the COO lists, bit for bit."""
    rng = np.random.default_rng(5)
    A, V = 4000, 3000
    deg = rng.integers(0, 7, V)
    venue = rng.permutation(np.repeat(np.arange(V), deg))
    agent = rng.integers(0, A, len(venue))
    people = deg + rng.integers(0, 3, V)
    host = compile_plan(A, {"school": {"agent": agent, "venue": venue, "people": people}}, age=np.zeros(A, np.int64),
                        sex=np.zeros(A, np.int64), layout="csr")
    assert len(host.long_rows) == 0 and (host.blocks[:, 7] == 1).all() and len(host.blocks) > 3
    specs = [NetworkSpec("school", "school", N.MASK_Q)]
    beta = 0.87
    groups = RC.groups_of(RC.launch_nets(specs, ["school"], {"school": beta}, host.set_index), [1])
    x = np.where(rng.random(A) < 0.5, 0.0, rng.uniform(2.0 ** -10, 1.0, A)).astype(np.float32)
    susc = rng.choice([0.0, 0.4, 1.0], A).astype(np.float32)
    kw = dict(has_q=False, q_thr=np.inf, day_type=0)
    cum = RC.restate_cum(host, groups, None, x, stage_ext=np.ones(A, np.float32), **kw)["school"]
    ts = RC.ts_of_agents(host, groups, None, {"school": cum}, susc=susc, stage=np.ones(A, np.float32), **kw)
    tv, ta = torch.from_numpy(venue), torch.from_numpy(agent)
    y = torch.tensor(beta, dtype=torch.float32) * torch.from_numpy(host.sets[0].v_pcontact)
    want = torch.zeros(V).scatter_add_(0, tv, torch.from_numpy(x)[ta] * y[tv])
    assert np.array_equal(RC.bits(cum[:, 0]), RC.bits(want.numpy())) and want.max() > 0
    want_ts = torch.zeros(A).scatter_add_(0, ta, want[tv] * torch.from_numpy(susc)[ta])
    assert np.array_equal(RC.bits(ts), RC.bits(want_ts.numpy())) and want_ts.max() > 0


# ---- dyadic inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", G.EVERY)
def test_dyadic_inputs_are_summed_exactly(key):
    """Transmissions m * 2^-10 (m = 1 ... 3), p_contact 1, 1/2, 1/4, 1/8 (`people` 2, 3, 5, 9), beta 1/2, 1 or 2, table
    entries and susceptibilities 0, 1/2 or 1: every term is a whole number of 2^-15 (pass 1) and every partial sum of a
    venue stays below 2^24 of them (at most 24 581 terms of at most 3 x 2 x 2^4 units), so no product and no add rounds
    and the order cannot matter: cum equals the float64 sum, in every block form.  The terms of pass 2 are whole numbers
    of 2^-17 and an agent's sum stays below 2^24 of them in these worlds (asserted: the float64 sum is a float32)."""
    w = G.world_of(key)
    host = G.host_of(key, "dyadic")
    x = G.dyadic_vector(key)
    assert set(np.unique(x * 2.0 ** 10).tolist()) <= {0.0, 1.0, 2.0, 3.0}
    for name, p in w["variants"]["dyadic"]["people"].items():
        assert set(p.tolist()) <= {2, 3, 5, 9}
    for li, launch in enumerate(w["launches"]):
        groups, tables = G.launch_of(key, "dyadic", launch)
        kw = dict(has_q=launch["has_q"], q_thr=G.Q_THR, day_type=launch["day_type"])
        cums, ts = G.restated(key, "dyadic", li, x, cache="dyadic")
        exact = RC.cum_float64(host, groups, tables, x, stage_ext=w["stage_ext"], **kw)
        assert set(exact) == set(cums)
        for name, (s, _, _) in exact.items():
            assert np.array_equal(cums[name].astype(np.float64), s), (key, li, name)
            if host.sets[host.set_index[name]].n_edges > 50 and w["n_agents"] > 1:
                assert s.max() > 0
        ts64, _, _ = RC.ts_float64(host, groups, tables, cums, susc=w["variants"]["dyadic"]["susc"], stage=w["stage_ext"], **kw)
        assert np.array_equal(ts64.astype(np.float32).astype(np.float64), ts64)
        assert np.array_equal(ts.astype(np.float64), ts64), (key, li)
        assert ts64.max() > 0 or w["n_agents"] == 1


# ---- general inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", G.EVERY)
def test_general_inputs_stay_inside_the_float32_bounds(key):
    """u = 2^-24.  A venue's cum is the float32 sum of n terms fp32(x * y) - on a table set fp32(fp32(tab * src) * y) - of
    the float32 inputs src, tab and y = fp32(beta * p_contact); the float64 sum is of the exact products x * y.  A term
    carries at most two roundings and goes through at most n - 1 adds, whatever the order (fewer in the lane and thread
    trees), each of which rounds a partial sum of magnitude <= S = sum |terms| (1 + O(u)):

        |cum - sum| <= ((1 + u)^(n + 1) - 1) S <= (n + 2) u S

    (the last step: (n + 1) u / (1 - (n + 1) u) <= (n + 2) u while (n + 1)(n + 2) u <= 1, n <= 4 094; a long venue's terms
    go through at most 8192 / 256 + 6 + 4 + slots <= 50 adds instead of n - 1.)  The values of G.general_vector and the
    tables keep every product normal, so no absolute term is needed.  An agent's trans_susc is the float32 sum of N terms
    fp32(cum * w), w = fp32(fp32(q * tab) * susc) [* 0 or 1] with q in {0, 1}: two roundings per term again, and N - 1
    rounding adds over the per-network sums and their sum (adding +0.0 is exact): (N + 2) u S with its own N and S, against
    the float64 sum of cum * (q * tab * susc * [age > 75]) over the float32 cum values that pass 2 reads."""
    w = G.world_of(key)
    host = G.host_of(key, "general")
    x = G.general_vector(key)
    for li, launch in enumerate(w["launches"]):
        groups, tables = G.launch_of(key, "general", launch)
        kw = dict(has_q=launch["has_q"], q_thr=G.Q_THR, day_type=launch["day_type"])
        cums, ts = G.restated(key, "general", li, x, cache="general")
        exact = RC.cum_float64(host, groups, tables, x, stage_ext=w["stage_ext"], **kw)
        for name, (s, s_abs, n) in exact.items():
            err = np.abs(cums[name].astype(np.float64) - s)
            bound = (n[:, None] + 2) * U * s_abs
            assert (err <= bound).all(), (key, li, name, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err > 0).any() or host.sets[host.set_index[name]].n_edges < 50 or w["n_agents"] == 1     # (sums do round)
        ts64, ts_abs, n = RC.ts_float64(host, groups, tables, cums, susc=w["variants"]["general"]["susc"],
                                        stage=w["stage_ext"], **kw)
        err = np.abs(ts.astype(np.float64) - ts64)
        assert (err <= (n + 2) * U * ts_abs).all(), (key, li)


@pytest.mark.parametrize("key", ["lanes", "long", "nets"])
def test_a_probed_venue_is_a_single_product(key):
    """Where exactly one term of a venue is non-zero, cum is that product in every block form: fp32(fp32(tab * x) * y) -
    adding +0.0 changes nothing.  Most venues of every probe vector are such venues."""
    w = G.world_of(key)
    host = G.host_of(key)
    single = 0
    for j in range(G.N_PROBES):
        x = G.probe_vector(key, j)
        cums, _ = G.restated(key, "general", 0, x, cache=f"probe-{j}")
        groups, tables = G.launch_of(key, "general", w["launches"][0])
        for g in groups:
            s = host.sets[g.set]
            src = RC.source(x, w["stage_ext"], G.Q_THR, w["launches"][0]["has_q"], g.raw)
            ve = np.repeat(np.arange(s.n_venues), np.diff(s.v_rowptr))
            for k in range(g.nk):
                xe = src[s.v_agent]
                if g.leisure:
                    xe = RC.f32_mul(tables[g.table[k]][w["launches"][0]["day_type"]][host.agent_class[s.v_agent]], xe)
                term = RC.f32_mul(xe, RC.f32_mul(g.beta[k], s.v_pcontact)[ve])
                nz = np.bincount(ve, weights=(term != 0), minlength=s.n_venues)
                one = np.flatnonzero(nz == 1)
                value = np.zeros(s.n_venues, dtype=np.float32)
                np.add.at(value, ve[term != 0], term[term != 0])          # (one term per venue of `one`: no sum)
                assert np.array_equal(RC.bits(cums[s.name][one, k]), RC.bits(value[one])), (key, j, s.name, k)
                single += len(one)
    assert single >= (10 if key == "long" else 100), single      # (the long world has sixteen venues)


# ---- the schedule -----------------------------------------------------------------------------------------------------------
def test_schedule_facts_the_restatement_relies_on():
    """Of build_schedule, beyond what tests/test_plan_host.py asserts (every venue covered once, lanes in {1, 4, 16, 64},
    a STREAM block's edge range is its venues'): the chunks of a long row tile [rp[v], rp[v + 1]) in slot order, in steps
    of LONG_CHUNK; a long row's slots are consecutive and no two rows share one; a STREAM block has 1 ... 2 048 rows."""
    for rp in (np.concatenate([[0], np.cumsum(G.BIG)]), np.concatenate([[0], np.cumsum(G.LEI)]),
               G.host_of("lanes").sets[0].v_rowptr, G.host_of("nets").sets[3].v_rowptr):
        blocks, long_rows, n_slots = build_schedule(np.asarray(rp, dtype=np.int32), 3, slot_base=5)
        RC.check_schedule(np.asarray(rp, dtype=np.int64), blocks, long_rows)
        deg = np.diff(rp)
        assert sorted(long_rows[:, 1].tolist()) == np.flatnonzero(deg > N.GJ_STREAM_EDGES).tolist()
        used = []
        for (sid, v, s0, s1) in long_rows.tolist():
            chunks = blocks[(blocks[:, 1] == 1) & (blocks[:, 2] == v)]
            chunks = chunks[np.argsort(chunks[:, 6])]
            assert chunks[:, 6].tolist() == list(range(s0, s1)) and s1 - s0 == -(-deg[v] // LONG_CHUNK)
            assert chunks[0, 4] == rp[v] and chunks[-1, 5] == rp[v + 1] and (chunks[1:, 4] == chunks[:-1, 5]).all()
            assert ((chunks[:-1, 5] - chunks[:-1, 4]) == LONG_CHUNK).all() and (chunks[:, 7] == 64).all()
            used += list(range(s0, s1))
        assert sorted(used) == list(range(5, 5 + n_slots))
        stream = blocks[blocks[:, 1] == 0]
        rows = stream[:, 3] - stream[:, 2]
        assert (rows >= 1).all() and (rows <= MAX_ROWS_PER_BLOCK).all() and (blocks[:, 0] == 3).all()
