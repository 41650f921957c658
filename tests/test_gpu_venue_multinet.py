"""GPU: pass 1 of the venue launch on a set that carries several networks, `cum` per (venue, network) BIT FOR BIT.

Phase B of csrc/gj_tiled.h sums a multi-network set in one pass per group of eight slots (multi_sums): the class
weights of all networks from one or two 16-byte LDS reads, the run structure once, an LDS atomic only where a run of
one venue ends.  None of that may change a bit of `cum`, so every case here is held to a numpy restatement of the
arithmetic itself - not to another path of the library:

    term = fp32(w * x)                       w: the network's table entry of the agent's class (transposed: times age > 75
                                             for a care-visit kind of network), x: the agent's transmission
    fx   = rint(term * 2^36) as int64        (a term beyond the set's window, an infinity or a NaN raises flags instead)
    sum  = exact integer sum per venue
    s    = fp32(fp64(sum) * 2^-36);  +-1e30 with one flag, NaN with both (two flags per sum)
    cum  = fp32(fp32(beta * p_contact) * s)

Worlds of 11 264 - 16 001 agents with one leisure set of more than 8 192 edges (several venue blocks), nk in
{1, 2, 3, 6, 8}, both values of `transpose`:
  * runs-of-1:   no two neighbouring slots of a tile share a venue - every atomic is a real one;
  * short-runs:  venues of 2 - 20 consecutive agents - runs that end inside a lane's eight slots;
  * one-venue:   one venue holds every agent (the wave-uniform path; its run crosses lanes, groups and tiles), venues of
                 700 agents next to it in further blocks.
A NaN, +-inf and +-3e4 are then placed inside a run and at a run's end (the slots are found from the plan's own arrays)."""
import numpy as np
import pytest
import torch

import gj_pass1_ref as R1
from grad_june_amd import _native as N
from grad_june_amd.engine import AgentBuffers, InfectionEngine
from grad_june_amd.plan import DevicePlan, NetworkSpec, _host, compile_plan

pytestmark = pytest.mark.gpu

SET = "leisure"
NKS = [1, 2, 3, 6, 8]
WORLDS = ["runs-of-1", "short-runs", "one-venue"]
SATURATED = np.float32(1.0e30)


# ---- worlds ------------------------------------------------------------------------------------------------------------
def make_world(kind):
    rng = np.random.default_rng(WORLDS.index(kind) + 11)
    if kind == "runs-of-1":
        # slices of 1024 agents; within a slice every edge of a family goes to another venue
        A = 11 * 1024
        a = np.arange(A)
        agent = np.concatenate([a, a[5:]])            # (five edges fewer: a block then ends in pad slots)
        venue = np.concatenate([a % 1024, 1024 + (7 * a[5:]) % 1024])
    elif kind == "short-runs":
        A = 16001
        agent, venue, v0 = [], [], 0
        for shift in (0, 5):                      # two families of groups of 2 - 20 consecutive agents
            sizes = []
            while sum(sizes) < A - shift:
                sizes.append(int(rng.integers(2, 21)))
            ids = np.repeat(np.arange(len(sizes)), sizes)[: A - shift]
            agent.append(np.arange(shift, A))
            venue.append(v0 + ids)
            v0 += len(sizes)
        agent, venue = np.concatenate(agent), np.concatenate(venue)
    else:
        A = 12345
        a = np.arange(A)
        agent = np.concatenate([a, a])
        venue = np.concatenate([np.zeros(A, dtype=np.int64), 1 + a // 700])
    perm = rng.permutation(len(agent))
    agent, venue = agent[perm].astype(np.int64), venue[perm].astype(np.int64)
    V = int(venue.max()) + 1
    people = np.bincount(venue, minlength=V).astype(np.int64) + 1           # p_contact = 1 / attendees
    age = rng.integers(0, 100, A)
    age[::5] = rng.integers(76, 100, len(age[::5]))                         # enough agents beyond 75 for the transposed mask
    sex = rng.integers(0, 2, A)
    # transmissions: zeros and values in [2^-10, 1] (no product below the normal range)
    x = np.where(rng.random(A) < 0.3, 0.0, rng.uniform(2.0 ** -10, 1.0, A)).astype(np.float32)
    return dict(kind=kind, A=A, V=V, agent=agent, venue=venue, people=people, age=age, sex=sex, x=x)


_WORLDS, _ENGINES = {}, {}


def world_of(kind):
    if kind not in _WORLDS:
        _WORLDS[kind] = make_world(kind)
    return _WORLDS[kind]


def networks_of(nk):
    """nk leisure networks: tables in [0.6, 1] (so that 3e4 * w leaves every window), every third one of the care-visit
    kind (its receiving side carries the age > 75 mask - the side that `transpose` moves into pass 1)."""
    rng = np.random.default_rng(100 + nk)
    names = [f"net{k}" for k in range(nk)]
    kinds = [N.MASK_QL_AGE75 if k % 3 == 1 else N.MASK_QL for k in range(nk)]
    tables = [rng.uniform(0.6, 1.0, (2, 2, 100)).astype(np.float32) for _ in range(nk)]
    betas = {n: float(np.float32(0.37 * (k + 1))) for k, n in enumerate(names)}
    return names, kinds, tables, betas


def engine_of(kind, nk, device):
    if (kind, nk) not in _ENGINES:
        w = world_of(kind)
        names, kinds, tables, _ = networks_of(nk)
        es = {SET: {"agent": w["agent"], "venue": w["venue"], "people": w["people"]}}
        host = compile_plan(w["A"], es, age=w["age"], sex=w["sex"], layout="tiled", nets_per_set={SET: nk}, eb_target=8192,
                            direct=False)
        specs = [NetworkSpec(n, SET, k, t) for n, k, t in zip(names, kinds, tables)]
        _ENGINES[(kind, nk)] = InfectionEngine(DevicePlan(host, specs, device))
    return _ENGINES[(kind, nk)]


# ---- the restatement ---------------------------------------------------------------------------------------------------
def term_limit_bits(max_venue_edges):
    """The set's window: 2^14 while its largest venue has at most 4 096 edges, else the power of two
    that keeps edges x window below 2^26.  (tests/gj_pass1_ref.py holds the rule.)"""
    return R1.term_limit_bits(max_venue_edges)


def restate(w, nk, day_type, transpose, x):
    """{network index: cum [V] float32}, and the venues with a flagged sum, per network: tests/gj_pass1_ref.py on this
    file's one set (every network of it active)."""
    names, kinds, tables, betas = networks_of(nk)
    with np.errstate(all="ignore"):
        pc = np.clip(np.float32(1.0) / (w["people"] - 1).astype(np.float32), np.float32(0.0), np.float32(1.0))
    nets = [(betas[n], t, k == N.MASK_QL_AGE75, False) for n, k, t in zip(names, kinds, tables)]
    cum, flagged = R1.restate_set(w["agent"], w["venue"], pc, nets, x, age=w["age"], sex=w["sex"], day_type=day_type,
                                  transpose=transpose)
    return ([np.ascontiguousarray(cum[:, k]).view(np.float32) for k in range(nk)],
            [np.ascontiguousarray(flagged[:, k]) for k in range(nk)])


def launch(engine, nk, day_type, transpose, x, device, phase=8):
    names, _, _, betas = networks_of(nk)
    A = engine.plan.host.n_agents
    p = engine.params(now=1.0, delta_time=1.0, day_type=day_type, active=names, betas=betas)
    p.transpose = transpose
    xs = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
    bufs = AgentBuffers(engine.plan, susceptibility=torch.ones(A, device=device), transmission=xs)
    out = torch.zeros(A, device=device)
    engine.step_phase(bufs, p, engine.io(trans_susc=out), phase)
    torch.cuda.synchronize()
    return engine.plan.cum_of(SET).cpu().numpy().copy()


def assert_same_bits(got, want, what):
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f"{what}: NaN at other venues"
    same = (got.view(np.uint32) == want.view(np.uint32)) | nan_w
    if not same.all():
        i = int(np.argmax(~same))
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} venues differ; first at {i}: got {got[i]!r}, "
                             f"want {want[i]!r}")


# ---- 1. finite worlds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", NKS)
@pytest.mark.parametrize("kind", WORLDS)
def test_cum_per_venue_and_network_bit_for_bit(device, kind, nk):
    w = world_of(kind)
    engine = engine_of(kind, nk, device)
    t = engine.plan.host.sets[0].tiled
    blk_e0, e_lv = _host(t.blk_e0).astype(np.int64), _host(t.e_lv)
    assert len(w["agent"]) > 8192 and t.n_blocks >= 3
    assert any(e_lv[e - 1] == 0xFFFF for e in blk_e0[1:]), "no block ends in pad slots"
    if kind == "runs-of-1":
        real = e_lv[:-1] != 0xFFFF
        assert not (real & (e_lv[1:] == e_lv[:-1])).any()
    if kind == "one-venue":       # a wave's 512 slots within one venue, and a run that crosses tiles
        lv0 = (e_lv[: blk_e0[1] // 512 * 512] == 0).reshape(-1, 512)
        assert lv0.all(axis=1).sum() >= 8 and int(np.diff(_host(t.blk_v0))[0]) == 1
    for transpose in (0, 1):
        day_type = transpose          # (both day types over the two directions)
        want, flagged = restate(w, nk, day_type, transpose, w["x"])
        assert not any(f.any() for f in flagged)
        got = launch(engine, nk, day_type, transpose, w["x"], device)
        assert got.shape == (w["V"], nk)
        for k in range(nk):
            assert np.abs(want[k]).max() > 0
            assert_same_bits(np.ascontiguousarray(got[:, k]), want[k], f"{kind} nk={nk} transpose={transpose} network {k}")
        if transpose and nk >= 2:     # the mask is in pass 1 only when transposed
            assert not np.array_equal(want[1], restate(w, nk, day_type, 0, w["x"])[0][1])


# ---- 2. values that cannot be summed -----------------------------------------------------------------------------------
def special_slots(engine, w, device):
    """Two agents with an edge of the set in distinct venues: one whose slot lies INSIDE a run of its lane's eight slots
    (the neighbours on both sides belong to the same venue), one whose slot ENDS a run of two slots or more.  The slots'
    agents are read from the workspace after a scatter of the agents' own numbers."""
    t = engine.plan.host.sets[0].tiled
    e_lv = _host(t.e_lv).astype(np.int64)
    launch(engine, engine.plan.c.sets[0].cum_stride, 0, 0, np.arange(1, w["A"] + 1, dtype=np.float32), device, phase=1)
    val = engine.plan.keep[0]["val"].cpu().numpy()[: len(e_lv)]
    p = np.arange(len(e_lv))
    real = e_lv != 0xFFFF
    prev_same = np.zeros(len(e_lv), dtype=bool)
    next_same = np.zeros(len(e_lv), dtype=bool)
    prev_same[1:] = (e_lv[1:] == e_lv[:-1]) & (p[1:] % 8 > 0)
    next_same[:-1] = (e_lv[:-1] == e_lv[1:]) & (p[:-1] % 8 < 7)
    inside = np.flatnonzero(real & prev_same & next_same)
    end = np.flatnonzero(real & prev_same & ~next_same)
    assert len(inside) and len(end)
    s_in = int(inside[len(inside) // 2])
    blk = np.searchsorted(_host(t.blk_e0), [s_in], side="right")[0]
    other = end[(np.searchsorted(_host(t.blk_e0), end, side="right") != blk) | (e_lv[end] != e_lv[s_in])]
    s_end = int(other[len(other) // 3])
    a_in, a_end = int(val[s_in]) - 1, int(val[s_end]) - 1
    assert 0 <= a_in < w["A"] and 0 <= a_end < w["A"] and a_in != a_end
    return a_in, a_end


@pytest.mark.parametrize("nk", [3, 6])
@pytest.mark.parametrize("kind", ["short-runs", "one-venue"])
def test_terms_that_cannot_be_summed_inside_and_at_the_end_of_a_run(device, kind, nk):
    w = world_of(kind)
    engine = engine_of(kind, nk, device)
    a_in, a_end = special_slots(engine, w, device)
    for value in (np.nan, np.inf, -np.inf, 3.0e4, -3.0e4):
        x = w["x"].copy()
        x[a_in] = x[a_end] = value
        for transpose in (0, 1):
            want, flagged = restate(w, nk, 0, transpose, x)
            # both agents' venues are flagged in the network without a mask (w >= 0.6: 3e4 w > 2^14)
            for a in (a_in, a_end):
                assert flagged[0][w["venue"][w["agent"] == a]].all()
            got = launch(engine, nk, 0, transpose, x, device)
            for k in range(nk):
                assert_same_bits(np.ascontiguousarray(got[:, k]), want[k],
                                 f"{kind} nk={nk} value={value} transpose={transpose} network {k}")
