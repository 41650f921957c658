"""The restatement of pass 2 (tests/gj_pass2_ref.py) - what tests/test_gpu_pass2_kernels.py holds the device to bit for
bit - checked on the CPU so that a wrong restatement cannot hide: against float64 sums from the edge lists within a
bound derived from the number formats, against tiling's emulations (the direct form bitwise), and its roundings, window,
flags and venue-group rule on hand-computed cases."""

import numpy as np
import pytest
import torch

import gj_pass2_ref as R
import gj_testlib as L
from grad_june_amd import tiling as TL
from grad_june_amd.plan import compile_plan
from test_gpu_random_worlds import random_world
from test_transposed_reference import june769_case

F32 = np.float32


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def f32_of(b):
    return np.ascontiguousarray(b).view(np.float32)


def random_cum(rng, V, stride, signed):
    """Magnitudes spread over 2^-30 ... 2^10, a fifth exact zeros."""
    c = np.exp2(rng.uniform(-30.0, 10.0, (V, stride)))
    if signed:
        c *= rng.choice([-1.0, 1.0], (V, stride))
    c[rng.random((V, stride)) < 0.2] = 0.0
    return c.astype(np.float32)


def world_case(world, tables, rng):
    """Every configured network active, a random signed cum per set, random stages and susceptibilities."""
    specs = L.network_specs(world, tables)
    if not specs:
        return None
    active = [s.name for s in specs]
    stride = {}
    for s in specs:
        stride[s.edge_set] = stride.get(s.edge_set, 0) + 1
    cums = {es: random_cum(rng, len(world["edge_sets"][es]["people"]), k, signed=True) for es, k in stride.items()}
    A = world["n_agents"]
    return dict(specs=specs, active=active, cums=cums, stage=rng.integers(1, 7, A).astype(np.float32),
                susc=rng.choice([0.0, 0.4, 1.0], A).astype(np.float32))


def host_plan(world, **kw):
    es = {k: {kk: vv.numpy() for kk, vv in v.items()} for k, v in world["edge_sets"].items()}
    return compile_plan(world["n_agents"], es, age=world["age"].numpy(), sex=world["sex"].numpy(), layout="tiled", **kw)


def check_against_fp64(world, tables, rng, what):
    """The three forms (workspace; direct with one group; direct with several) x quarantine x direction against the
    float64 sums, every agent within its bound.  Returns (direct sets seen, most venue groups of one set)."""
    case = world_case(world, tables, rng)
    if case is None:
        return 0, 0
    A = world["n_agents"]
    age, sex = world["age"].numpy(), world["sex"].numpy()
    forms = R.forms_of_plan(host_plan(world, runs=False))
    n_direct = sum(f["form"] == "direct" for f in forms.values())
    most = 0
    for use_forms, dtf in ((None, 0), (forms, 0), (forms, 24)):
        groups = R.groups_of(world["edge_sets"], case["specs"], case["active"], case["cums"], use_forms)
        direct = [g for g in groups if g["form"] == "direct" and len(g["agent"])]
        for g, (_, gv) in zip(direct, R.venue_groups([g["cum"].shape for g in direct], dtf)):
            most = max(most, -(-g["cum"].shape[0] // gv))
        for has_q in (False, True):
            for transpose in (0, 1):
                kw = dict(age=age, sex=sex, day_type=transpose, transpose=transpose, stage=case["stage"], q_thr=4.0,
                          has_quarantine=has_q)
                sums, ts = R.restate(A, groups, susceptibility=case["susc"], direct_table_floats=dtf, **kw)
                want, bound = R.fp64_sums(A, groups, **kw)
                got = f32_of(sums).astype(np.float64)
                bad = ~(np.abs(got - want) <= bound)
                assert not bad.any(), (what, use_forms is not None, dtf, has_q, transpose, int(np.argmax(bad)),
                                       got[bad][:3], want[bad][:3], bound[bad][:3])
                assert np.array_equal(ts, bits(case["susc"] * f32_of(sums)))
                assert np.abs(want).max() > 0
    return n_direct, most


def test_restatement_against_fp64_on_the_reference_world():
    case = june769_case(0, False)
    n_direct, most = check_against_fp64(case["world"], case["tables"], np.random.default_rng(5), "769")
    assert n_direct >= 2 and most >= 4


@pytest.mark.parametrize("seed", range(20))
def test_restatement_against_fp64_on_random_worlds(seed):
    rng = np.random.default_rng(7000 + seed)
    world = random_world(rng)
    tables = {n: torch.from_numpy(rng.random((2, 2, 100)).astype(np.float32)) for n in L.LEISURE + ("care_visit",)
              if rng.random() < 0.8}
    check_against_fp64(world, tables, rng, f"seed {seed}")


def test_random_draws_reach_the_direct_form_and_several_groups():
    seen, most = 0, 0
    for seed in range(20):
        rng = np.random.default_rng(7000 + seed)
        world = random_world(rng)
        forms = R.forms_of_plan(host_plan(world, runs=False))
        seen += sum(f["form"] == "direct" for f in forms.values())
        most = max([most] + [len(world["edge_sets"][n]["people"]) // 24 for n, f in forms.items() if f["form"] == "direct"])
    assert seen >= 5 and most >= 4


# ---- against the specification in tiling.py ----------------------------------------------------------------------------
def spec_world(rng, A=700, V=45, K=8):
    deg = rng.integers(0, K + 1, A)
    deg[rng.random(A) < 0.3] = 0
    deg[5] = K
    agent = np.repeat(np.arange(A), deg)
    rng.shuffle(agent)
    venue = rng.integers(0, V, len(agent))
    age, sex = rng.integers(0, 100, A), rng.integers(0, 2, A)
    return agent, venue, age, sex


@pytest.mark.parametrize("gv", [None, 7])
@pytest.mark.parametrize("leisure", [False, True], ids=["plain", "leisure"])
def test_a_single_direct_set_is_the_emulation_bit_for_bit(leisure, gv):
    """tiling.emulate_direct_pass2 on tiling.build_ell's rows == the restatement from the edge lists: K = 8 (four
    planes), one group and groups of 7 venues (direct_table_floats = 7 x stride: the launch rule then gives 7)."""
    rng = np.random.default_rng(31)
    A, V, sa = 700, 45, 64
    agent, venue, age, sex = spec_world(rng, A, V)
    stride = 3 if leisure else 2
    cum = random_cum(rng, V, stride, signed=True)
    tabs = [rng.random((2, 2, 100)).astype(np.float32) for _ in range(3)]
    nets = [(tabs[0], False), (tabs[1], True), (tabs[2], False)] if leisure else [(None, False)]
    ell, K = TL.build_ell(agent, venue, A, -(-A // sa), sa)
    assert K == 8
    g = R.make_group(agent, venue, cum, nets, raw=False, form="direct", ell_k=K)
    dtf = 0 if gv is None else 7 * stride
    assert R.venue_groups([(V, stride)], dtf) == [(0, V if gv is None else 7)]
    for transpose in (0, 1):
        got, _ = R.restate(A, [g], age=age, sex=sex, day_type=1, transpose=transpose, susceptibility=np.ones(A, F32),
                           direct_table_floats=dtf)
        weights = cls = None
        if leisure:
            cls = (sex * 100 + age).astype(np.uint8)
            weights = np.stack([(t[1].reshape(200) * ((np.arange(200) % 100 > 75) if (a75 and not transpose) else 1.0)
                                 ).astype(np.float32) for t, a75 in nets])
        want = TL.emulate_direct_pass2(ell, cum if leisure else cum[:, :1], A, weights=weights, agent_class=cls,
                                       group_venues=gv)
        assert np.array_equal(got, bits(want)), (transpose, int(np.argmax(got != bits(want))))
        assert np.abs(want).max() > 0


def test_the_item_order_is_not_the_coo_order():
    """1.0, 2^-24, 2^-24 in COO order is ((1 + 2^-24) + 2^-24) = 1 in float32 (a tie to even, twice).  The items add
    something else: with the large term in the second venue group the small ones meet first, 1 + 2^-23; and over two
    planes of one group the pairs are summed first, (1 + 0) + (2^-24 + 2^-24) = 1 + 2^-23."""
    one, tiny = F32(1.0), F32(2.0 ** -24)
    assert (one + tiny) + tiny == one
    kw = dict(age=np.zeros(1, int), sex=np.zeros(1, int), day_type=0, transpose=0, susceptibility=np.ones(1, F32))
    cum = np.zeros((12, 1), dtype=np.float32)
    cum[9], cum[0], cum[1] = one, tiny, tiny
    # edges in COO order to venues 9, 0, 1: plane 0 = (venue 9, venue 0), plane 1 = (venue 1, -)
    g = R.make_group(np.zeros(3, int), [9, 0, 1], cum, [(None, False)], raw=False, form="direct", ell_k=4)
    assert f32_of(R.restate(1, [g], **kw)[0])[0] == one                              # one group: (1 + tiny), + tiny
    assert R.venue_groups([(12, 1)], 8) == [(0, 8)]
    # groups of 8 venues: venues 0 and 1 (tiny, then tiny: 2^-23) before venue 9
    assert f32_of(R.restate(1, [g], direct_table_floats=8, **kw)[0])[0] == one + F32(2.0 ** -23)
    # one group, COO order 1, 0, tiny, tiny over two planes
    cum[2] = 0.0
    g = R.make_group(np.zeros(4, int), [9, 2, 0, 1], cum, [(None, False)], raw=False, form="direct", ell_k=4)
    assert ((one + F32(0)) + tiny) + tiny == one
    assert f32_of(R.restate(1, [g], **kw)[0])[0] == one + F32(2.0 ** -23)


def test_a_single_workspace_set_is_the_emulation_within_the_fixed_point_bound():
    rng = np.random.default_rng(32)
    A, V, sa = 700, 45, 64
    agent, venue, age, sex = spec_world(rng, A, V)
    S = -(-A // sa)
    cls = (sex * 100 + age).astype(np.uint8)
    t = TL.build_tiled("x", agent, venue, V, np.ones(V, F32), S, sa, agent_class=cls, sv_max=16, eb_target=256)
    terms = np.bincount(agent, minlength=A)
    for tab in (None, rng.random((2, 2, 100)).astype(np.float32)):
        cum = random_cum(rng, V, 1, signed=True)
        g = R.make_group(agent, venue, cum, [(tab, False)], raw=False)
        got, _ = R.restate(A, [g], age=age, sex=sex, day_type=0, transpose=0, susceptibility=np.ones(A, F32))
        want = TL.emulate_pass2(t, cum[:, 0], A, sa, weight_table=None if tab is None else tab[0].reshape(200))
        err = np.abs(f32_of(got).astype(np.float64) - want.astype(np.float64))
        assert (err <= terms * R.FX_AGENT_HALF + 2 * R.U32 * np.abs(want)).all()
        assert np.abs(want).max() > 0


# ---- roundings -----------------------------------------------------------------------------------------------------------
def test_rint_is_the_magic_number_conversion():
    rng = np.random.default_rng(33)
    x = np.concatenate([
        (rng.standard_normal(200000) * np.exp2(rng.uniform(-40, 18, 200000))).astype(np.float32),
        ((2 * np.arange(-2000, 2000) + 1) * 2.0 ** -33).astype(np.float32),            # ties
        np.array([0.0, -0.0, 262144.0, -262144.0, 2.0 ** -33, 2.0 ** -34, -2.0 ** -33, 1e-45, 2.0 ** -126], dtype=np.float32)])
    x = x[R.in_window(x)]
    assert len(x) > 200000
    assert np.array_equal(R.to_fx(x), R.to_fx_magic(x))
    assert R.to_fx(np.array([262144.0], F32))[0] == 1 << 50


def one_agent(values, raw=False, **kw):
    """An agent whose entries of one workspace set are ``values``: its sum as a float32."""
    n = len(values)
    g = R.make_group(np.zeros(n, int), np.arange(n), np.asarray(values, dtype=np.float32).reshape(n, 1), [(None, False)], raw=raw)
    args = dict(age=np.zeros(1, int), sex=np.zeros(1, int), day_type=0, transpose=0, susceptibility=np.ones(1, F32))
    args.update(kw)
    return f32_of(R.restate(1, [g], **args)[0])[0]


def test_ties_round_to_even():
    tie = lambda j: F32((2 * j + 1) * 2.0 ** -33)
    assert [int(R.to_fx(np.array([tie(j)]))[0]) for j in range(4)] == [0, 2, 2, 4]
    assert one_agent([tie(0)]) == 0.0 and one_agent([tie(1)]) == F32(2.0 ** -31)
    assert one_agent([tie(j) for j in range(4)]) == F32(8 * 2.0 ** -32)             # the exact sum is 16 * 2^-33 too ...
    assert one_agent([tie(0), tie(2)]) == F32(2 * 2.0 ** -32)                       # ... here it is 6 * 2^-33 = 3 * 2^-32
    assert one_agent([-tie(1), -tie(2)]) == F32(-4 * 2.0 ** -32)
    # a small term next to a large one survives: the sum is exact, only the read-back rounds
    assert one_agent([1.0, 2.0 ** -30]) == F32(1.0)
    assert one_agent([1.0, 2.0 ** -24]) == F32(1.0)                                   # a tie, to even
    assert one_agent([1.0, 2.0 ** -24, 2.0 ** -30]) == F32(1.0 + 2.0 ** -23)          # above the tie: only exact sums see it


def test_the_window_edge_and_the_flag_table():
    edge = F32(262144.0)
    above = np.nextafter(edge, F32(np.inf))
    big, nan, inf = F32(1e30), F32(np.nan), F32(np.inf)
    assert one_agent([edge]) == edge and one_agent([-edge, 1.0]) == F32(-262143.0)
    assert one_agent([above]) == big and one_agent([-above, 1.0]) == -big
    for v in (3e5, 1e30, inf):
        assert one_agent([v, 7.0]) == big and one_agent([-v, 7.0]) == -big
        assert np.isnan(one_agent([v, -v]))
    assert np.isnan(one_agent([nan])) and np.isnan(one_agent([nan, 3e5]))
    assert one_agent([1e-45, -0.0]) == 0.0
    # quarantine: the masked sum becomes 0 and a single flag is cleared; a NaN stays; a raw set is not touched
    q = dict(stage=np.array([5.0], F32), q_thr=4.0, has_quarantine=True)
    assert one_agent([3e5, 7.0], **q) == 0.0 and one_agent([-inf], **q) == 0.0 and one_agent([7.0], **q) == 0.0
    assert np.isnan(one_agent([nan], **q)) and np.isnan(one_agent([3e5, -3e5], **q))
    assert one_agent([3e5, 7.0], raw=True, **q) == big and one_agent([7.0], raw=True, **q) == 7.0
    assert one_agent([3e5, 7.0], stage=np.array([3.0], F32), q_thr=4.0, has_quarantine=True) == big
    # the raw set is added after the zeroing: the household term survives
    masked = R.make_group([0], [0], np.array([[3e5]], F32), [(None, False)], raw=False)
    house = R.make_group([0], [0], np.array([[2.5]], F32), [(None, False)], raw=True)
    kw = dict(age=np.zeros(1, int), sex=np.zeros(1, int), day_type=0, transpose=0, **q)
    for order in ([masked, house], [house, masked]):
        sums, ts = R.restate(1, order, susceptibility=np.array([0.4], F32), **kw)
        assert f32_of(sums)[0] == 2.5 and f32_of(ts)[0] == F32(0.4) * F32(2.5)
    # susceptibility 0: times 1e30 gives 0, times NaN gives NaN
    z = np.zeros(1, F32)
    assert f32_of(R.restate(1, [masked], age=[0], sex=[0], day_type=0, transpose=0, susceptibility=z)[1])[0] == 0.0
    poisoned = R.make_group([0], [0], np.array([[np.nan]], F32), [(None, False)], raw=False)
    assert np.isnan(f32_of(R.restate(1, [poisoned], age=[0], sex=[0], day_type=0, transpose=0, susceptibility=z)[1])[0])
    # the direct form has no window: 3e5 is added as it is
    d = R.make_group([0, 0], [0, 1], np.array([[3e5], [-1.0]], F32), [(None, False)], raw=False, form="direct", ell_k=2)
    assert f32_of(R.restate(1, [d], age=[0], sex=[0], day_type=0, transpose=0, susceptibility=np.ones(1, F32))[0])[0] == F32(299999.0)


# ---- the venue-group rule --------------------------------------------------------------------------------------------------
def test_venue_group_rule_on_hand_computed_cases():
    """budget = 40960 - 2 * 1600 - 2 * 64 = 37632 floats.  Tables (V, stride): a = (10, 1), b = (5, 3), c = (100, 1),
    d = (30, 1), e = (20, 3), big = (20000, 3) = 60000 floats."""
    assert R.BUDGET == 37632
    a, b, c, d, e, big = (10, 1), (5, 3), (100, 1), (30, 1), (20, 3), (20000, 3)
    # no knob: cap0 = the largest table (100), cap1 = the rest; a in region 0, b in 1, c back in 0 - every table whole
    assert R.venue_groups([a, b, c], 0) == [(0, 10), (1, 5), (0, 100)]
    # 24: cap0 = cap1 = 24; alternation as before, c (100 > 24) in groups of 24
    assert R.venue_groups([a, b, c], 24) == [(0, 10), (1, 5), (0, 24)]
    assert R.venue_groups([a, b, c], 40) == [(0, 10), (1, 5), (0, 40)]
    # region 0 only: nothing that follows a region-0 table fits region 1 (24 floats)
    assert R.venue_groups([c, d, e], 24) == [(0, 24), (0, 24), (0, 8)]             # e: 24 // 3
    assert R.venue_groups([c, d, e], 40) == [(0, 40), (1, 30), (0, 13)]            # d fits region 1; e (60 > 40): 40 // 3
    # alternation 0 1 0 1 with tables that fit; a set behind a region-1 set always returns to region 0
    assert R.venue_groups([a, a, a, a, c], 0) == [(0, 10), (1, 10), (0, 10), (1, 10), (0, 100)]
    # a table larger than the budget: cap0 = 37632 -> 12544 venues of stride 3 per group; cap1 = 0, so no region 1
    assert R.venue_groups([big, a], 0) == [(0, 12544), (0, 10)]
    assert R.venue_groups([a, big], 0) == [(0, 10), (0, 12544)]
    # the knob never takes cap0 below 8 floats (one venue of eight networks)
    assert R.venue_groups([c], 3) == [(0, 8)]
    assert R.venue_groups([], 24) == []
    with pytest.raises(ValueError):
        R.venue_groups([(10, 16)], 8)                                              # not one venue of stride 16 in 8 floats


def test_ell_columns_and_primary_edges():
    agent = np.array([2, 0, 2, 1, 2, 0])
    venue = np.array([7, 3, 5, 4, 5, 3])
    assert R.ell_columns(agent, 4).tolist() == [0, 0, 1, 0, 2, 1]
    ell, K = TL.build_ell(agent, venue, 4, 1, 64)
    rows = TL.ell_rows(ell)
    col = R.ell_columns(agent, 4)
    assert K == 4 and all(rows[a, c] == v for a, v, c in zip(agent, venue, col))
    # the first edge in COO order to the agent's smallest venue (tiling.split_primary_runs keeps the others)
    assert R.primary_edges(agent, venue, 4).tolist() == [False, True, True, True, False, False]
    a_s, v_s = np.sort(agent), venue[np.argsort(agent, kind="stable")]        # smallest venues 3, 4, 5: ordered
    rf = TL.split_primary_runs(a_s, v_s, 3, 8, 64, min_share=0.0)
    assert rf is not None and np.array_equal(~rf.keep, R.primary_edges(a_s, v_s, 3))
