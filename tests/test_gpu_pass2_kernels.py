"""GPU: pass 2 of the tiled step per agent - phase C + phase D of csrc/gj_tiled.h (k_tile_venues mode 0 / 2,
k_tile_agents, k_tile_epilogue) - BIT FOR BIT against the numpy restatement tests/gj_pass2_ref.py, in every form.

Pass 1 is pinned to its arithmetic by test_gpu_pass1_kernels.py (every form, against tests/gj_pass1_ref.py) and, for a
leisure set in the workspace form, by test_gpu_venue_multinet.py / test_gpu_venue_lv8.py; pass 2 was compared with
other things only (the oracle at rtol 2e-5, float64 sums within a bound, itself across geometries).  Here `agent_sums`
and `trans_susc` of EVERY agent are compared as uint32 (NaN by position) with the restatement, which works from the edge
lists alone and which tests/test_pass2_ref.py checks on the CPU.

Drive A - pass 2 alone on a given cum: the chosen arrays are written into plan.cum_of(set) in place, step_phase 6
(phase C, reads cum from memory), step_phase 4 (phase D without the decision).
Drive B - pass 2 as the step runs it: quarantine_transmission, step_phase 8, cum read back (the restatement takes the
device's own cum), step_phase 4; day type 0 with the forward direction, 1 with the transposed one.

Worlds (the smallest at which the code paths differ):
  W-small  1 003 agents: slices of 64 give 16 slices with a tail of 43 agents, n % 4 = 3.  Six sets: household (raw,
           degree 1 but for a few duplicated edges), company (degree <= 2: K = 2, one plane), school (degree <= 8: four
           planes), leisure (three networks, one of the age > 75 kind; degree <= 4), university (degree up to 30: never
           direct), care_home (no edge).  A third and more of the agents have no edge in each set; duplicated (agent,
           venue) pairs; `people` differs from the degree.
  W-quads  43 847 agents, the same six kinds of set (~220 000 edges: the direct form of a K = 8 set needs two edges per
           agent): slices of 4 160 agents (a lane's second quad exists for 16 lanes only) and of 19 840 (the maximum:
           all five quads, a partial last slice of 4 167 agents).
  W-run    W-small renumbered household-major, the household set in the run form.

The forms are asserted on the plans' own fields (test_every_form_is_reached)."""
import math

import numpy as np
import pytest
import torch

import gj_pass2_ref as R
import gj_testlib as L
from grad_june_amd import _native as N
from grad_june_amd import tiling as TL
from grad_june_amd.engine import AgentBuffers, InfectionEngine
from grad_june_amd.plan import DevicePlan, NetworkSpec, compile_plan
from test_gpu_random_worlds import random_layout, random_world
from test_gpu_run_form import household_major

pytestmark = pytest.mark.gpu

F32 = np.float32
Q_THR = 4.0
SETS = ["household", "company", "school", "leisure", "university", "care_home"]
# (name, edge set, kind): the launch order of the sets is school, university, company, care_home, leisure, household
NETWORKS = [("school", "school", N.MASK_Q), ("university", "university", N.MASK_Q), ("company", "company", N.MASK_Q),
            ("care_home", "care_home", N.MASK_Q), ("pub", "leisure", N.MASK_QL), ("care_visit", "leisure", N.MASK_QL_AGE75),
            ("gym", "leisure", N.MASK_QL), ("household", "household", N.MASK_RAW)]
ACTIVE = [n for n, _, _ in NETWORKS]
BETAS = {n: float(np.float32(0.5 + 0.37 * i)) for i, n in enumerate(ACTIVE)}
STRIDE = {"household": 1, "company": 1, "school": 1, "leisure": 3, "university": 1, "care_home": 1}


# ---- worlds --------------------------------------------------------------------------------------------------------------
def degrees(rng, A, share, lo, hi):
    deg = np.where(rng.random(A) < share, rng.integers(lo, hi + 1, A), 0)
    deg[int(rng.integers(0, A))] = hi
    return deg


def make_world(A, seed):
    rng = np.random.default_rng(seed)
    n_v = {"household": max(8, A // 3), "company": max(60, A // 40), "school": max(50, A // 60), "leisure": max(8, A // 150),
           "university": max(80, A // 100), "care_home": 5}
    deg = {"household": (rng.random(A) < 0.7).astype(np.int64), "company": degrees(rng, A, 0.5, 1, 2),
           "school": degrees(rng, A, 0.42, 2, 8), "leisure": degrees(rng, A, 0.55, 1, 4),
           "university": degrees(rng, A, 0.02 if A > 5000 else 0.06, 1, 30), "care_home": np.zeros(A, dtype=np.int64)}
    sets = {}
    for s in SETS:
        agent = np.repeat(np.arange(A), deg[s])
        venue = rng.integers(0, n_v[s], len(agent))
        if s in ("company", "school", "leisure") and len(agent):       # duplicated (agent, venue) pairs
            second = np.flatnonzero(agent[1:] == agent[:-1]) + 1
            dup = second[rng.random(len(second)) < 0.1]
            venue[dup] = venue[dup - 1]
        if s == "household":                                            # a few agents with their household edge twice
            twice = rng.choice(len(agent), max(3, len(agent) // 50), replace=False)
            agent, venue = np.concatenate([agent, agent[twice]]), np.concatenate([venue, venue[twice]])
        perm = rng.permutation(len(agent))
        agent, venue = agent[perm], venue[perm]
        people = np.bincount(venue, minlength=n_v[s]) + rng.integers(0, 3, n_v[s])      # not the degree
        sets[s] = {"agent": agent.astype(np.int64), "venue": venue.astype(np.int64), "people": people.astype(np.int64)}
    age = rng.integers(0, 100, A)
    age[::4] = rng.integers(76, 100, len(age[::4]))
    tables = {n: np.where(rng.random((2, 2, 100)) < 0.1, 0.0, rng.random((2, 2, 100))).astype(np.float32)
              for n, es, _ in NETWORKS if es == "leisure"}
    return dict(n_agents=A, age=age, sex=rng.integers(0, 2, A), edge_sets=sets, tables=tables,
                stage=rng.integers(1, 7, A).astype(np.float32),
                susc=rng.choice([0.0, 0.4, 1.0], A).astype(np.float32),
                specs=[NetworkSpec(n, es, kind, tables.get(n)) for n, es, kind in NETWORKS])


def renumbered_household_major(w):
    hh = w["edge_sets"]["household"]
    order, new_of = household_major(hh["agent"], hh["venue"], w["n_agents"])
    sets = {k: dict(v, agent=new_of[v["agent"]]) for k, v in w["edge_sets"].items()}
    return dict(w, age=w["age"][order], sex=w["sex"][order], stage=w["stage"][order], susc=w["susc"][order], edge_sets=sets)


_WORLDS, _HOSTS, _ENGINES, _WANT = {}, {}, {}, {}


def world_of(key):
    if key not in _WORLDS:
        if key == "small":
            _WORLDS[key] = make_world(1003, 41)
        elif key == "quads":
            _WORLDS[key] = make_world(43847, 42)
        else:
            _WORLDS[key] = renumbered_household_major(world_of("small"))
    return _WORLDS[key]


# ---- layouts ---------------------------------------------------------------------------------------------------------------
SMALL = dict(sv_max=64, eb_target=512)
TINY = dict(sv_max=16, eb_target=64)
# world, slice_agents (None: the default choice), compile_plan arguments, DevicePlan arguments
LAYOUTS = {
    "ws-narrow": ("small", 64, dict(SMALL, desc_wide=False, direct=False, runs=False), {}),
    "ws-wide": ("small", 64, dict(SMALL, desc_wide=True, direct=False, runs=False), {}),
    "ws-tiny-wide": ("small", 64, dict(TINY, desc_wide=True, desc_explicit=False, direct=False, runs=False), {}),
    "ws-explicit": ("small", 64, dict(TINY, desc_explicit=True, direct=False, runs=False), {}),
    "ws-pad16": ("small", None, dict(direct=False, runs=False, tile_pad=16), {}),
    "ws-split-no-lv8": ("small", 64, dict(SMALL, direct=False, runs=False), dict(split_epilogue=True, lv8=False)),
    "direct": ("small", 64, dict(runs=False), {}),
    "direct-split": ("small", 64, dict(runs=False), dict(split_epilogue=True)),
    "direct-12": ("small", 64, dict(runs=False), dict(direct_table_floats=12)),
    "direct-24": ("small", 64, dict(SMALL, runs=False), dict(direct_table_floats=24)),
    "direct-40-split": ("small", 64, dict(runs=False), dict(direct_table_floats=40, split_epilogue=True)),
    "direct-some": ("small", 64, dict(SMALL, runs=False, direct=("school", "leisure")), dict(lv8=False)),
    "direct-presum": ("small", 64, dict(SMALL, runs=False, presum=True), dict(direct_table_floats=24)),
    "run": ("run", 64, dict(SMALL, runs=("household",)), {}),
    "run-ws": ("run", 64, dict(SMALL, runs=("household",), direct=False), dict(split_epilogue=True)),
    "quads-ws-4160": ("quads", 4160, dict(direct=False, runs=False), {}),
    "quads-direct-4160": ("quads", 4160, dict(runs=False), {}),
    "quads-ws-19840": ("quads", 19840, dict(direct=False, runs=False), {}),
    "quads-direct-19840": ("quads", 19840, dict(runs=False), dict(direct_table_floats=4000)),
}
ALL = list(LAYOUTS)


def host_of(layout):
    if layout not in _HOSTS:
        wkey, sa, kw, _ = LAYOUTS[layout]
        w = world_of(wkey)
        kw = dict(kw)
        if sa is not None:
            kw["slices"] = (-(-w["n_agents"] // sa), sa)
        _HOSTS[layout] = compile_plan(w["n_agents"], w["edge_sets"], age=w["age"], sex=w["sex"], layout="tiled",
                                      nets_per_set={"leisure": 3}, **kw)
    return _HOSTS[layout]


def engine_of(layout, device):
    if layout not in _ENGINES:
        w = world_of(LAYOUTS[layout][0])
        _ENGINES[layout] = InfectionEngine(DevicePlan(host_of(layout), w["specs"], device, **LAYOUTS[layout][3]))
    return _ENGINES[layout]


def dtf_of(layout):
    return LAYOUTS[layout][3].get("direct_table_floats", 0)


def forms_seen(layout):
    host = host_of(layout)
    f = set()
    for s in host.sets:
        t = s.tiled
        if t.n_edges == 0 and t.runs is None and not t.ell_k:
            continue
        f.add("direct" if t.ell_k else ("run" if t.runs is not None else "workspace"))
        if not t.ell_k:
            f.add("explicit" if t.slot_idx is not None and t.n_edges > 0 else ("wide" if t.desc_wide else "narrow"))
            if t.multi_slots is not None and len(t.multi_slots):
                f.add("multi_slots")
            if t.n_edges > len(world_of(LAYOUTS[layout][0])["edge_sets"][s.name]["agent"]):
                f.add("tile_pad")
        if t.presum:
            f.add("presum")
        if t.ell_k:
            f.add(f"K={t.ell_k}")
    return f


def test_every_form_is_reached(device):
    """On the plans' own fields: workspace form with narrow, wide and explicit-slot descriptors, multi_slots rows and
    tiles padded to 16; direct with one group, with several groups in both LDS regions, for some sets only; the run
    form; the split epilogue; presum; the one-byte venue ids on and off; the slice extents of the W-quads world."""
    seen = set()
    for layout in ALL:
        seen |= forms_seen(layout)
    assert seen >= {"workspace", "direct", "run", "narrow", "wide", "explicit", "multi_slots", "tile_pad", "presum", "K=2",
                    "K=4", "K=8"}, seen
    forms = {k: R.forms_of_plan(host_of(k)) for k in ALL}
    assert {n for n, f in forms["direct"].items() if f["form"] == "direct"} == {"household", "company", "school", "leisure"}
    assert {n for n, f in forms["direct-some"].items() if f["form"] == "direct"} == {"school", "leisure"}
    assert forms["run"]["household"]["form"] == "run" and forms["run"]["school"]["form"] == "direct"
    assert forms["run-ws"]["household"]["form"] == "run" and forms["run-ws"]["school"]["form"] == "workspace"
    assert all(f["form"] == "workspace" for k in ALL if "ws-" in k and k != "run-ws" for f in forms[k].values())
    # venue groups: one group each without the knob; with 24 / 40 floats several groups, both regions in use
    w = world_of("small")
    order = ["school", "company", "leisure", "household"]                          # launch order of the direct sets
    tables = [(len(w["edge_sets"][s]["people"]), STRIDE[s]) for s in order]
    assert [gv for _, gv in R.venue_groups(tables, 0)] == [V for V, _ in tables]
    for knob in (24, 40):
        rule = R.venue_groups(tables, knob)
        assert {r for r, _ in rule} == {0, 1} and sum(gv < V for (_, gv), (V, _) in zip(rule, tables)) >= 3, rule
    assert all(gv < V for (_, gv), (V, _) in zip(R.venue_groups(tables, 12), tables))      # leisure too: 12 // 3 of its 8 venues
    for k in ALL:
        e = engine_of(k, device)
        assert e.plan.tiled_c.direct_table_floats == dtf_of(k)
        assert (e.plan.agent_scratch is not None) == bool(LAYOUTS[k][3].get("split_epilogue"))
        assert any(t is not None for t in e.plan.lv8) == (LAYOUTS[k][3].get("lv8") is not False)
    # slices: a tail of 43 agents; 1 040 quads per slice (16 lanes with a second quad); the maximum, last slice partial
    assert (host_of("direct").n_slices, host_of("direct").slice_agents, 1003 - 15 * 64, 1003 % 4) == (16, 64, 43, 3)
    assert host_of("quads-ws-4160").slice_agents // 4 - 1024 == 16
    assert (host_of("quads-ws-19840").slice_agents, 43847 - 2 * 19840) == (TL.SA_MAX, 4167)
    assert sum(len(v["agent"]) for v in world_of("quads")["edge_sets"].values()) > 150_000


# ---- driving the engine ----------------------------------------------------------------------------------------------------
def params_of(engine, day_type, transpose, has_q):
    p = engine.params(now=1.0, delta_time=1.0, day_type=day_type, active=ACTIVE, betas=BETAS, has_quarantine=has_q,
                      q_threshold=Q_THR if has_q else math.inf)
    p.transpose = transpose
    return p


def offset_buffer(n, device, offset, fill=float("nan")):
    """[n] floats that start `offset` floats into a 16-byte aligned allocation."""
    big = torch.full((n + 8,), fill, device=device)
    assert big.data_ptr() % 16 == 0
    return big[offset:offset + n]


def outputs(engine, w, p, device, x=None, susc=None, stage=None, want=("trans_susc", "agent_sums", "probs"), offset=0):
    """(buffers, io, the output tensors by name)"""
    A = w["n_agents"]
    s = offset_buffer(A, device, offset)
    s.copy_(torch.from_numpy(w["susc"] if susc is None else susc))
    st = torch.from_numpy(w["stage"] if stage is None else stage).to(device)
    xs = torch.zeros(A, device=device) if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
    bufs = AgentBuffers(engine.plan, susceptibility=s, transmission=xs, current_stage=st)
    out = {k: offset_buffer(A, device, offset) for k in want}
    io = engine.io(trans_susc=out.get("trans_susc"), agent_sums=out.get("agent_sums"), not_infected_probs=out.get("probs"))
    if offset:
        assert all(t.data_ptr() % 16 == 4 * offset for t in list(out.values()) + [s])
    return bufs, io, out


def write_cums(engine, cums):
    """The chosen arrays into plan.cum_of(set), in place."""
    for name, c in cums.items():
        dst = engine.plan.cum_of(name)
        assert tuple(dst.shape) == c.shape
        dst.copy_(torch.from_numpy(c))


def drive_a(engine, w, cums, device, *, day_type, transpose, has_q, **kw):
    write_cums(engine, cums)
    p = params_of(engine, day_type, transpose, has_q)
    bufs, io, out = outputs(engine, w, p, device, **kw)
    engine.step_phase(bufs, p, io, 6)
    engine.step_phase(bufs, p, io, 4)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def drive_b(engine, edge_sets, w, x, device, *, active, betas, day_type, transpose, has_q, q_thr=Q_THR):
    p = engine.params(now=1.0, delta_time=1.0, day_type=day_type, active=active, betas=betas, has_quarantine=has_q,
                      q_threshold=q_thr if has_q else math.inf)
    p.transpose = transpose
    bufs, io, out = outputs(engine, w, p, device, x=x, want=("trans_susc", "agent_sums"))
    engine.quarantine_transmission(bufs, p)
    engine.step_phase(bufs, p, io, 8)
    torch.cuda.synchronize()
    cums = {name: engine.plan.cum_of(name).cpu().numpy().copy() for name in edge_sets}
    engine.step_phase(bufs, p, io, 4)
    torch.cuda.synchronize()
    return cums, {k: v.cpu().numpy() for k, v in out.items()}


def assert_bits(got, want_bits, groups, what):
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want_bits).view(np.float32)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    same = (nan_g & nan_w) | (~nan_g & ~nan_w & (got.view(np.uint32) == want_bits))
    if not same.all():
        i = int(np.argmax(~same))
        sets = [f"{g['name']}[{g['form']}] x{int((g['agent'] == i).sum())}" for g in groups if (g["agent"] == i).any()]
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} agents differ; first agent {i} (sets {sets}): "
                             f"got {got[i]!r} ({got.view(np.uint32)[i]:#010x}), want {want[i]!r} ({want_bits[i]:#010x})")


def groups_for(layout, w, cums, specs=None, active=None):
    return R.groups_of(w["edge_sets"], specs or w["specs"], active or ACTIVE, cums, R.forms_of_plan(host_of(layout)))


def restated(layout, w, cums, *, day_type, transpose, has_q, susc=None, stage=None, key=None):
    """The restatement, computed once per (arithmetic, inputs) and shared by the layouts that give the same arithmetic
    (every workspace layout of a world)."""
    forms = R.forms_of_plan(host_of(layout))
    k = None
    if key is not None:
        k = (key, LAYOUTS[layout][0], tuple(sorted((n, f["form"], f["ell_k"], f["run_window"]) for n, f in forms.items())),
             dtf_of(layout) if any(f["form"] != "workspace" for f in forms.values()) else 0, day_type, transpose, has_q)
        if k in _WANT:
            return _WANT[k]
    groups = groups_for(layout, w, cums)
    res = (groups,) + R.restate(w["n_agents"], groups, age=w["age"], sex=w["sex"], day_type=day_type, transpose=transpose,
                                susceptibility=w["susc"] if susc is None else susc,
                                stage=w["stage"] if stage is None else stage, q_thr=Q_THR, has_quarantine=has_q,
                                direct_table_floats=dtf_of(layout))
    if k is not None:
        _WANT[k] = res
    return res


def check(layout, device, cums, what, *, day_type, transpose, has_q, susc=None, stage=None, key=None, **kw):
    w = world_of(LAYOUTS[layout][0])
    groups, sums, ts = restated(layout, w, cums, day_type=day_type, transpose=transpose, has_q=has_q, susc=susc, stage=stage,
                                key=key)
    got = drive_a(engine_of(layout, device), w, cums, device, day_type=day_type, transpose=transpose, has_q=has_q, susc=susc,
                  stage=stage, **kw)
    what = f"{layout} {what} day {day_type} transpose {transpose} quarantine {has_q}"
    assert_bits(got["agent_sums"], sums, groups, what + " agent_sums")
    assert_bits(got["trans_susc"], ts, groups, what + " trans_susc")
    return got, (groups, sums, ts)


def random_cums(w, seed, signed):
    """Magnitudes spread over 2^-30 ... 2^10 (a tenth exact zeros): forward positive, transposed signed."""
    rng = np.random.default_rng(seed)
    out = {}
    for s in SETS:
        shape = (len(w["edge_sets"][s]["people"]), STRIDE[s])
        c = np.exp2(rng.uniform(-30.0, 10.0, shape))
        if signed:
            c *= rng.choice([-1.0, 1.0], shape)
        c[rng.random(shape) < 0.1] = 0.0
        out[s] = c.astype(np.float32)
    return out


_CUMS = {}


def cums_of(wkey, transpose):
    if (wkey, transpose) not in _CUMS:
        _CUMS[(wkey, transpose)] = random_cums(world_of(wkey), 900 + transpose, signed=bool(transpose))
    return _CUMS[(wkey, transpose)]


# ---- 1. finite -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ALL)
def test_finite_cum_every_agent_bit_for_bit(device, layout):
    wkey = LAYOUTS[layout][0]
    w = world_of(wkey)
    assert set(np.unique(w["susc"])) == {F32(0.0), F32(0.4), F32(1.0)}
    for has_q in (False, True):
        for transpose in (0, 1):
            cums = cums_of(wkey, transpose)
            got, (groups, sums, ts) = check(layout, device, cums, "finite", day_type=transpose, transpose=transpose,
                                            has_q=has_q, key="finite")
            assert np.isfinite(got["agent_sums"]).all() and np.abs(got["agent_sums"]).max() > 1
            quarantined = ~(w["stage"] < Q_THR)
            assert 100 < quarantined.sum() < w["n_agents"] - 100
    # the same bits whether or not the outputs are requested together
    e = engine_of(layout, device)
    alone = {k: drive_a(e, w, cums, device, day_type=1, transpose=1, has_q=True, want=(k,))[k]
             for k in ("agent_sums", "trans_susc", "probs")}
    for k in alone:
        assert np.array_equal(alone[k].view(np.uint32), got[k].view(np.uint32)), (layout, k)


SAME_ARITHMETIC = [("ws-narrow", "ws-split-no-lv8"), ("direct", "direct-split")]      # fused, split: every set in the same form


@pytest.mark.parametrize("fused,split", SAME_ARITHMETIC)
def test_split_and_fused_epilogue(device, fused, split):
    """k_tile_epilogue gives what the epilogue inside k_tile_agents gives: agent_sums, trans_susc and the probabilities
    bit for bit."""
    w = world_of("small")
    for has_q in (False, True):
        for transpose in (0, 1):
            cums = cums_of("small", transpose)
            kw = dict(day_type=transpose, transpose=transpose, has_q=has_q)
            a = drive_a(engine_of(fused, device), w, cums, device, **kw)
            b = drive_a(engine_of(split, device), w, cums, device, **kw)
            for k in ("agent_sums", "trans_susc", "probs"):
                assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (fused, split, k, has_q, transpose)
            assert np.isfinite(a["probs"]).all() and a["probs"].min() < 1.0


# ---- 2. roundings ------------------------------------------------------------------------------------------------------------
def edges_of(w, s, a):
    """The venues of agent a's edges of set s, in COO order."""
    es = w["edge_sets"][s]
    return es["venue"][es["agent"] == a]


def find_agent(w, s, used, k, pred=lambda a, v: True):
    """An agent of set s - the one with the fewest edges - none of whose venues is in use, whose first k venues (COO
    order) occur once among its venues, and for which pred(agent, venues) holds.  All its venues become used."""
    es = w["edge_sets"][s]
    deg = np.bincount(es["agent"], minlength=w["n_agents"])
    for a in np.argsort(deg, kind="stable"):
        if deg[a] < k:
            continue
        v = edges_of(w, s, a)
        if all((v == x).sum() == 1 for x in v[:k]) and not (set(v.tolist()) & used) and pred(int(a), v):
            used |= set(v.tolist())
            return int(a), v[:k]
    raise AssertionError(f"no such agent in {s}")


def zero_cums(w):
    return {s: np.zeros((len(w["edge_sets"][s]["people"]), STRIDE[s]), dtype=np.float32) for s in SETS}


ROUNDING_LAYOUTS = ["ws-narrow", "ws-explicit", "ws-pad16", "direct", "direct-12", "direct-24", "direct-40-split",
                    "direct-some"]
TINY_TERM = F32(2.0 ** -24)


def rounding_case(w):
    """cum is zero but for the venues of chosen agents, which therefore receive exactly these terms (in COO order):
      ties    (2j + 1) 2^-33, j = 0..3: rint gives 0, 2, 2, 4 (half away from zero would give 1, 2, 3, 4)
      small   1.0, 2^-30
      above   1.0, 2^-24, 2^-30: above the tie of the read-back only if the small term is still there
      three   1.0, 2^-24, 2^-24 with the large term in a venue >= 40 and the small ones in venues < 12 (school): with
              venue groups of 12, 24 or 40 the small terms meet first
      planes  1.0, 0, 2^-24, 2^-24: two planes of a K = 8 set (school)
    in university (always the workspace form) and in school (direct in the direct layouts)."""
    cums = zero_cums(w)
    tie = lambda j: F32((2 * j + 1) * 2.0 ** -33)
    chosen = {}
    for s in ("university", "school"):
        used = set()
        c = cums[s][:, 0]
        plant = [("ties", [tie(0), tie(1), tie(2), tie(3)], None), ("small", [1.0, 2.0 ** -30], None),
                 ("above", [1.0, TINY_TERM, 2.0 ** -30], None)]
        if s == "school":
            plant += [("three", [1.0, TINY_TERM, TINY_TERM], lambda a, v: v[0] >= 40 and v[1] < 12 and v[2] < 12),
                      ("planes", [1.0, 0.0, TINY_TERM, TINY_TERM], None)]
        other = w["edge_sets"]["school" if s == "university" else "university"]["agent"]      # (not in the other planted set)
        for case, values, pred in plant:
            a, v = find_agent(w, s, used, len(values),
                              lambda a, v: not (other == a).any() and (pred is None or pred(a, v)))
            c[v] = values
            chosen[s, case] = a
    return cums, chosen


@pytest.mark.parametrize("layout", ROUNDING_LAYOUTS)
def test_roundings(device, layout):
    w = world_of("small")
    cums, chosen = rounding_case(w)
    one, up = F32(1.0), F32(1.0 + 2.0 ** -23)
    got, (groups, sums, ts) = check(layout, device, cums, "roundings", day_type=0, transpose=0, has_q=False, key="roundings",
                                    susc=np.ones(1003, F32))
    # what the restatement says of the chosen agents, hand-computed (the device equals it bit for bit: check)
    want = sums.view(np.float32)
    form = {g["name"]: g["form"] for g in groups}
    several = dtf_of(layout) in (12, 24, 40)
    for (s, case), a in chosen.items():
        if form[s] == "workspace":     # exact sums, one rounding: 1 + 2^-24 + 2^-24 = 1 + 2^-23 whatever the order
            expect = {"ties": F32(8 * 2.0 ** -32), "small": one, "above": up, "three": up, "planes": up}[case]
        else:                          # float32 in item order
            expect = {"ties": F32(16 * 2.0 ** -33), "small": one, "above": None if several else one, "three": up if several else one,
                      "planes": None if several else up}[case]
        assert expect is None or want[a] == expect, (layout, s, case, a, want[a], expect)
    assert {form["university"], form["school"]} == ({"workspace"} if layout.startswith("ws-") else {"workspace", "direct"})


def test_the_venue_group_size_is_the_one_geometry_input_that_changes_bits(device):
    """direct_table_floats (a test knob) changes the order of a direct set's float32 additions: the agent of
    rounding_case whose large term lies in a later venue group reads 1 with one group and 1 + 2^-23 with groups of 24
    venues, on the device.  (Slices, blocks, descriptors, presum and the one-byte ids do not change a bit: the layouts
    of one form share one restatement in test_finite_cum_every_agent_bit_for_bit.)"""
    w = world_of("small")
    cums, chosen = rounding_case(w)
    a = chosen["school", "three"]
    kw = dict(day_type=0, transpose=0, has_q=False, susc=np.ones(1003, F32))
    one_group = drive_a(engine_of("direct", device), w, cums, device, **kw)["agent_sums"]
    groups_24 = drive_a(engine_of("direct-24", device), w, cums, device, **kw)["agent_sums"]
    assert one_group[a] == F32(1.0) and groups_24[a] == F32(1.0 + 2.0 ** -23)


# ---- 3. what cannot be summed ------------------------------------------------------------------------------------------------
EDGE = F32(262144.0)
ABOVE = np.nextafter(EDGE, F32(np.inf))
BIG = F32(1e30)
SPECIALS = [EDGE, ABOVE, F32(3e5), F32(-3e5), BIG, -BIG, F32(np.inf), F32(-np.inf), F32(np.nan), F32(1e-45), F32(-0.0)]
SPECIAL_LAYOUTS = {"university": ["ws-narrow", "ws-explicit", "direct", "run"],                # masked, always workspace
                   "household": ["ws-narrow", "ws-split-no-lv8", "direct", "run", "run-ws"],   # the raw set, in three forms
                   "school": ["ws-narrow", "direct", "direct-24", "direct-40-split", "run"]}   # masked; direct where it can
HOUSE_TERM = F32(2.5)


def special_case(w, s):
    """A finite positive base cum, one special value in each of eleven venues of set s that no chosen agent attends, and
    chosen agents (the venues they attend in s are theirs alone among the chosen):
      both      two venues of the set with +3e5 and -3e5 (household: one venue with +3e5); not quarantined
      sat       quarantined, +1e30 from the set, a household whose cum is 2.5, susceptibility 0.4
      nan       quarantined, a NaN from the set
      zero_sat  susceptibility 0 against 1e30;   zero_nan  susceptibility 0 against a NaN (neither quarantined)."""
    cums = random_cums(w, 77, signed=False)
    stage, susc = w["stage"].copy(), w["susc"].copy()
    used, chosen, planted = set(), {}, set()
    c = cums[s][:, 0]
    hh = w["edge_sets"]["household"]
    in_hh = np.bincount(hh["agent"], minlength=w["n_agents"]) > 0
    n_both = 1 if s == "household" else 2
    for name, values, st, su, pred in [("both", [3e5, -3e5][:n_both], 1.0, 1.0, None),
                                       ("sat", [1e30], 5.0, 0.4, lambda a, v: in_hh[a]),
                                       ("nan", [np.nan], 5.0, 1.0, None), ("zero_sat", [1e30], 1.0, 0.0, None),
                                       ("zero_nan", [np.nan], 1.0, 0.0, None)]:
        a, v = find_agent(w, s, used, len(values), pred or (lambda a, v: True))
        c[v] = values
        planted |= set(v.tolist())
        chosen[name] = a
        stage[a], susc[a] = st, su
    if s != "household":
        cums["household"][edges_of(w, "household", chosen["sat"]), 0] = HOUSE_TERM
    attended = np.unique(w["edge_sets"][s]["venue"])
    free = [int(x) for x in attended if x not in used]          # venue ids of the world's own list
    assert len(free) >= len(SPECIALS)
    special_venues = {}
    for x, value in zip(free, SPECIALS):
        c[x] = value
        special_venues[x] = value
    return cums, stage, susc, chosen, special_venues, planted | set(special_venues)


@pytest.mark.parametrize("placed,layout", [(s, l) for s, ls in SPECIAL_LAYOUTS.items() for l in ls])
def test_values_that_cannot_be_summed(device, placed, layout):
    w = world_of(LAYOUTS[layout][0])
    cums, stage, susc, chosen, special_venues, altered = special_case(w, placed)
    es = w["edge_sets"][placed]
    raw = placed == "household"
    for transpose in (0, 1):
        got, (groups, sums, ts) = check(layout, device, cums, f"specials in {placed}", day_type=0, transpose=transpose,
                                        has_q=True, susc=susc, stage=stage)
        want, want_ts = sums.view(np.float32), ts.view(np.float32)
        form = {g["name"]: g["form"] for g in groups}[placed]
        # what the restatement says of the chosen agents (each has one edge of the set per planted venue, so in the run
        # form these are primary edges: the direct arithmetic)
        windowed = form == "workspace"
        a = chosen["both"]
        if windowed:
            assert (want[a] == BIG) if raw else np.isnan(want[a])            # +flag and -flag from two venues: NaN
        else:
            assert np.isfinite(want[a]) and abs(want[a]) < 4e5                 # the direct form adds +-3e5 as they are
        a = chosen["sat"]
        n_house = len(edges_of(w, "household", a))
        assert stage[a] >= Q_THR and n_house >= 1
        assert want[a] == (BIG if raw else HOUSE_TERM * F32(n_house))          # flag cleared, the household term survives
        assert want_ts[a] == F32(0.4) * want[a]
        assert np.isnan(want[chosen["nan"]]) == (windowed or raw)             # a NaN stays; a masked direct set is not taken
        assert want[chosen["zero_sat"]] == BIG and want_ts[chosen["zero_sat"]] == 0.0
        assert np.isnan(want[chosen["zero_nan"]]) and np.isnan(want_ts[chosen["zero_nan"]])
        # the agents that attend exactly one special venue of the set (once), found from the edge lists, not quarantined
        hits = 0
        deg = np.bincount(es["agent"], minlength=w["n_agents"])
        n_special = np.bincount(es["agent"][np.isin(es["venue"], list(altered))], minlength=w["n_agents"])
        for x, value in special_venues.items():
            for a in np.unique(es["agent"][es["venue"] == x]):
                if n_special[a] != 1 or (stage[a] >= Q_THR and not raw) or a in chosen.values():
                    continue
                direct_edge = (not windowed) and (form == "direct" or deg[a] == 1)
                if not windowed and not direct_edge:
                    continue
                hits += 1
                if np.isnan(value):
                    assert np.isnan(want[a])
                elif windowed and abs(value) > EDGE:
                    assert want[a] == (BIG if value > 0 else -BIG), (x, value, a, want[a])
                elif abs(value) <= EDGE:
                    assert np.isfinite(want[a]) and want[a] >= value - F32(1.0)     # 262144 itself is added
                elif abs(value) == F32(3e5):
                    assert np.isfinite(want[a]) and abs(want[a] - value) < 1e5      # added as it is
        assert hits >= 1


# ---- 4. alignment ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ws-narrow", "direct-24", "direct-40-split", "run", "quads-direct-4160"])
def test_outputs_at_a_four_byte_offset(device, layout):
    """Outputs and susceptibility one float into larger buffers (io_vec4 == 0: guarded scalar accesses): the same bits."""
    wkey = LAYOUTS[layout][0]
    w = world_of(wkey)
    cums = cums_of(wkey, 1)
    aligned, _ = check(layout, device, cums, "aligned", day_type=1, transpose=1, has_q=True, key="finite")
    shifted, _ = check(layout, device, cums, "offset 4 bytes", day_type=1, transpose=1, has_q=True, key="finite", offset=1)
    for k in aligned:
        assert np.array_equal(aligned[k].view(np.uint32), shifted[k].view(np.uint32)), (layout, k)


# ---- drive B on the worlds above ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ws-narrow", "ws-split-no-lv8", "direct", "direct-presum", "direct-some", "run",
                                    "quads-ws-19840", "quads-direct-4160"])
def test_pass2_as_the_step_runs_it(device, layout):
    w = world_of(LAYOUTS[layout][0])
    A = w["n_agents"]
    rng = np.random.default_rng(12)
    engine = engine_of(layout, device)
    for transpose in (0, 1):
        x = np.where(rng.random(A) < 0.3, 0.0, rng.uniform(2.0 ** -10, 1.0, A))
        if transpose:
            x *= rng.choice([-1.0, 1.0], A)
        for has_q in (False, True):
            cums, got = drive_b(engine, SETS, w, x.astype(np.float32), device, active=ACTIVE, betas=BETAS, day_type=transpose,
                                transpose=transpose, has_q=has_q)
            assert all(np.isfinite(c).all() for c in cums.values()) and np.abs(cums["leisure"]).max() > 0
            groups, sums, ts = restated(layout, w, cums, day_type=transpose, transpose=transpose, has_q=has_q)
            what = f"{layout} drive B transpose {transpose} quarantine {has_q}"
            assert_bits(got["agent_sums"], sums, groups, what + " agent_sums")
            assert_bits(got["trans_susc"], ts, groups, what + " trans_susc")
            assert np.abs(got["agent_sums"]).max() > 0


# ---- 5. random worlds ----------------------------------------------------------------------------------------------------------
def random_draw(seed):
    """A draw of random_world / random_layout that has a network and a tiled layout (further draws of the same stream
    until it does: no seed is skipped)."""
    rng = np.random.default_rng(8000 + seed)
    while True:
        world = random_world(rng)
        tables = {n: torch.from_numpy(rng.random((2, 2, 100)).astype(np.float32)) for n in L.LEISURE + ("care_visit",)
                  if rng.random() < 0.8}
        specs = L.network_specs(world, tables)
        if specs:
            break
    A = world["n_agents"]
    active = [s.name for s in specs if rng.random() < 0.8] or [specs[0].name]
    betas = {n: float(np.float32(rng.uniform(0.1, 40.0))) for n in active}
    layout = random_layout(rng, A)
    while layout[0] == "csr":
        layout = random_layout(rng, A)
    return dict(world=world, tables=tables, specs=specs, active=active, betas=betas, kw=layout[1],
                stage=rng.integers(1, 7, A).astype(np.float32), susc=rng.choice([0.0, 0.4, 1.0], A).astype(np.float32),
                has_q=bool(rng.random() < 0.5), q_thr=float(rng.choice([2.0, 3.0, 4.0])), rng=rng)


@pytest.mark.parametrize("seed", range(40))
def test_pass2_on_random_worlds(device, seed):
    """The forward counterpart of test_transposed_passes_on_random_worlds, without a tolerance: drive B, both
    directions, every agent bit for bit."""
    d = random_draw(seed)
    world, rng = d["world"], d["rng"]
    A = world["n_agents"]
    engine = L.make_engine(world, d["tables"], device, layout="tiled", **d["kw"])
    forms = R.forms_of_plan(engine.plan.host)
    w = dict(n_agents=A, susc=d["susc"], stage=d["stage"])
    sets = {k: {kk: vv.numpy() for kk, vv in v.items()} for k, v in world["edge_sets"].items()}
    for transpose in (0, 1):
        x = np.where(rng.random(A) < 0.3, 0.0, rng.uniform(2.0 ** -10, 1.0, A))
        if transpose:
            x *= rng.choice([-1.0, 1.0], A)
        cums, got = drive_b(engine, list(sets), w, x.astype(np.float32), device, active=d["active"], betas=d["betas"],
                            day_type=transpose, transpose=transpose, has_q=d["has_q"], q_thr=d["q_thr"])
        groups = R.groups_of(sets, d["specs"], d["active"], cums, forms)
        sums, ts = R.restate(A, groups, age=world["age"].numpy(), sex=world["sex"].numpy(), day_type=transpose,
                             transpose=transpose, susceptibility=d["susc"], stage=d["stage"], q_thr=d["q_thr"],
                             has_quarantine=d["has_q"])
        what = f"seed {seed}: {A} agents, active {d['active']}, q {d['has_q']} {d['q_thr']}, {d['kw']}, transpose {transpose}"
        assert_bits(got["agent_sums"], sums, groups, what + " agent_sums")
        assert_bits(got["trans_susc"], ts, groups, what + " trans_susc")
