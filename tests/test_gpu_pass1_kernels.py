"""GPU: pass 1 of the tiled step per venue - k_tile_scatter, phase B of k_tile_venues, k_tile_presum and k_presum_reduce
of csrc/gj_tiled.h - BIT FOR BIT against the numpy restatement tests/gj_pass1_ref.py, in every form.

Pass 1 is exact by design (fixed-point terms, integer adds, two fixed roundings), so `cum` of EVERY venue of EVERY active
network is compared as uint32 (NaN by position) with the restatement, which works from the edge lists alone and which
tests/test_pass1_ref.py checks on the CPU.  There is no tolerance in this file.

Drive: the transmissions into the buffers, quarantine_transmission, step_phase 7 (phase A, then phase B with the cum
write-out; the presum launches where a set takes them), synchronize, plan.cum_of(set) of every set.

Sentinel: every cum buffer is filled with 123.0 before every drive.  What the code does, and what is asserted: column k
of a set's cum belongs to the k-th of the set's ACTIVE networks; the columns behind them, and every column of a set
without an active network, are not written and keep the sentinel.  An active set without an edge is written: +0.0 in
every venue, as is every venue nobody attends.

Worlds: those of tests/test_gpu_pass2_kernels.py (every layout of its ALL) and the ones below, each the smallest at
which its code path exists (test_every_form_is_reached asserts the paths on the plans' own fields):
  W-uniform    9 001 agents, slices of 1 024.  school: venue 0 holds agents 0 ... 4 999 (whole 512-slot windows of one
               venue - the wave-uniform sum - and the set's window is 2^13), the rest go to venues of 2 - 20; university:
               8 200 venues cut into a block of 8 197 (a second trip of the cum write-out) and one of 3; household in
               small venues.  Venues nobody attends, `people` of 0, 1 and 2.
  W-halo       W-small / W-run cut at 960 owned agents + 43 halo agents that attend owned venues.
  W-primary    1 003 agents who all have a household edge, household-major: the run form with every agent primary.
  W-presum     9 001 agents, three presum sets in one launch (K = 2, K = 8, a leisure set of two networks), 3 workgroups.
  W-batch2     13 001 agents, one presum workgroup (the ctypes field set after construction): 3 251 quads > 3 x 1 024.
  W-tables     135 173 agents with one edge each: 34 presum workgroups, a second trip of the reduce loop.
  W-wrap       20 000 agents in one venue (test_large_venue_sums_saturate_and_never_wrap), presum=True."""
import functools
import hashlib
import math

import numpy as np
import pytest
import torch

import gj_pass1_ref as R1
import test_gpu_pass2_kernels as P2
from grad_june_amd import _native as N
from grad_june_amd import tiling as TL
from grad_june_amd.engine import InfectionEngine
from grad_june_amd.plan import DevicePlan, NetworkSpec, _host, compile_plan
from test_gpu_pass2_kernels import ALL, LAYOUTS, assert_bits, engine_of, forms_seen, host_of, outputs, params_of

pytestmark = pytest.mark.gpu

F32 = np.float32
Q_THR = P2.Q_THR
SENTINEL = F32(123.0)
PLAIN = [("school", "school", N.MASK_Q), ("university", "university", N.MASK_Q), ("company", "company", N.MASK_Q),
         ("household", "household", N.MASK_RAW)]
LEISURE2 = [("pub", "leisure", N.MASK_QL), ("care_visit", "leisure", N.MASK_QL_AGE75)]


# ---- worlds --------------------------------------------------------------------------------------------------------------
def groups_of_consecutive(rng, n, lo, hi):
    """Venue ids 0, 0, .., 1, 1, .. of n consecutive agents in groups of lo - hi, and the number of groups."""
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(lo, hi + 1)))
    return np.repeat(np.arange(len(sizes)), sizes)[:n].astype(np.int64), len(sizes)


def edge_set(rng, agent, venue, V, odd=True, shuffle=True):
    """A set with `people` = attendees + 0 .. 2, three further venues that nobody attends (`people` 0, 1, 2) and - with
    `odd` - `people` of 0, 1, 2 on the attended venues 1, 2, 3 as well (p_contact 0, 1, 1)."""
    agent, venue = np.asarray(agent, dtype=np.int64), np.asarray(venue, dtype=np.int64)
    if shuffle:
        perm = rng.permutation(len(agent))
        agent, venue = agent[perm], venue[perm]
    people = np.bincount(venue, minlength=V) + rng.integers(0, 3, V)
    people = np.concatenate([people, [0, 1, 2]])
    if odd:
        people[1:4] = [0, 1, 2]
    return {"agent": agent, "venue": venue, "people": people.astype(np.int64)}


def finish_world(rng, A, sets, networks, n_ext=None):
    n_ext = A if n_ext is None else n_ext
    age = rng.integers(0, 100, n_ext)
    age[::4] = rng.integers(76, 100, len(age[::4]))
    tables = {n: np.where(rng.random((2, 2, 100)) < 0.1, 0.0, rng.random((2, 2, 100))).astype(np.float32)
              for n, es, _ in networks if es == "leisure"}
    networks = [t for t in networks if t[1] in sets]
    active = [n for n, _, _ in networks]
    stage = rng.integers(1, 7, n_ext).astype(np.float32)
    return dict(n_agents=A, n_ext=n_ext, age=age, sex=rng.integers(0, 2, n_ext), edge_sets=sets, tables=tables,
                stage=stage[:A], stage_ext=stage, susc=rng.choice([0.0, 0.4, 1.0], A).astype(np.float32),
                specs=[NetworkSpec(n, es, kind, tables.get(n)) for n, es, kind in networks], active=active,
                betas={n: float(np.float32(0.5 + 0.37 * i)) for i, n in enumerate(active)})


def uniform_world():
    rng = np.random.default_rng(51)
    A = 9001
    rest, n_rest = groups_of_consecutive(rng, A - 5000, 2, 20)
    school = edge_set(rng, np.arange(A), np.concatenate([np.zeros(5000, np.int64), 1 + rest]), 1 + n_rest)
    # university: 8 200 venues, one or two attendees each, some nobody's; 8 203 with the three of edge_set
    uni_v = rng.permutation(A) % 8197
    university = edge_set(rng, np.arange(A), uni_v, 8197)
    hh, n_hh = groups_of_consecutive(rng, A, 1, 5)
    household = edge_set(rng, np.arange(A), hh, n_hh, shuffle=False)
    return finish_world(rng, A, {"school": school, "university": university, "household": household}, PLAIN)


def halo_world(base):
    """W-small (or W-run) with the agents from 960 on as halo agents: their edges stay (they attend owned venues), and
    twenty of them get one more household edge each, so that the household set has halo edges in either numbering."""
    w = P2.world_of(base)
    rng = np.random.default_rng(61)
    hh = w["edge_sets"]["household"]
    more_a = rng.choice(np.arange(960, 1003), 20, replace=False)
    more_v = rng.integers(0, len(hh["people"]), 20)
    at = rng.choice(len(hh["agent"]), 20, replace=False)
    sets = dict(w["edge_sets"], household=dict(hh, agent=np.insert(hh["agent"], at, more_a),
                                               venue=np.insert(hh["venue"], at, more_v)))
    stage = np.concatenate([w["stage"][:960], rng.integers(1, 7, 43).astype(np.float32)])
    return dict(w, n_agents=960, n_ext=1003, edge_sets=sets, stage=stage[:960], stage_ext=stage, susc=w["susc"][:960],
                active=list(P2.ACTIVE), betas=dict(P2.BETAS))


def primary_world():
    rng = np.random.default_rng(71)
    A = 1003
    hh, n_hh = groups_of_consecutive(rng, A, 1, 5)
    twice = rng.choice(A, 40, replace=False)                       # a second household edge, to a later household
    agent = np.concatenate([np.arange(A), twice])
    venue = np.concatenate([hh, np.minimum(hh[twice] + rng.integers(0, 9, 40), n_hh - 1)])
    household = edge_set(rng, agent, venue, n_hh)
    deg = P2.degrees(rng, A, 0.5, 1, 2)
    a = np.repeat(np.arange(A), deg)
    company = edge_set(rng, a, rng.integers(0, 60, len(a)), 60)
    return finish_world(rng, A, {"household": household, "company": company}, PLAIN)


def presum_world():
    rng = np.random.default_rng(81)
    A = 9001
    sets = {}
    for name, (share, lo, hi, V) in {"company": (0.6, 1, 2, 205), "school": (0.7, 2, 8, 150), "leisure": (0.6, 1, 4, 61)}.items():
        a = np.repeat(np.arange(A), P2.degrees(rng, A, share, lo, hi))
        sets[name] = edge_set(rng, a, rng.integers(0, V, len(a)), V)
    return finish_world(rng, A, sets, PLAIN[:3] + LEISURE2)


def one_edge_world(A, V, seed):
    rng = np.random.default_rng(seed)
    company = edge_set(rng, np.arange(A), rng.integers(0, V, A), V)
    return finish_world(rng, A, {"company": company}, PLAIN)


def wrap_world():
    n = 20_000
    rng = np.random.default_rng(91)
    school = {"agent": np.arange(n, dtype=np.int64), "venue": np.zeros(n, dtype=np.int64), "people": np.array([n])}
    w = finish_world(rng, n, {"school": school}, PLAIN)
    return dict(w, betas={"school": 0.5})


WORLDS = {"uniform": uniform_world, "halo-small": lambda: halo_world("small"), "halo-run": lambda: halo_world("run"),
          "primary": primary_world, "presum": presum_world, "batch2": lambda: one_edge_world(13001, 300, 101),
          "tables": lambda: one_edge_world(135173, 2000, 102), "wrap": wrap_world}
_WORLDS, _HOSTS, _ENGINES, _WANT = {}, {}, {}, {}


def world_of(key):
    if key in ("small", "quads", "run"):
        return dict(P2.world_of(key), n_ext=P2.world_of(key)["n_agents"], stage_ext=P2.world_of(key)["stage"],
                    active=list(P2.ACTIVE), betas=dict(P2.BETAS))
    if key not in _WORLDS:
        _WORLDS[key] = WORLDS[key]()
    return _WORLDS[key]


# ---- cases: the layouts of the pass-2 file, and the forms they lack ----------------------------------------------------------
SMALL, TINY = P2.SMALL, P2.TINY
# world, slice_agents (None: the default choice), compile_plan arguments, DevicePlan arguments, tweak
MORE = {
    "walk-narrow": ("small", 64, dict(SMALL, desc_wide=False, direct=False, runs=False), {}, "no-rows"),
    "walk-wide": ("small", 64, dict(TINY, desc_wide=True, desc_explicit=False, direct=False, runs=False), {}, "no-rows"),
    "quads-ws-19840-blocks": ("quads", 19840, dict(direct=False, runs=False, desc_wide=False, eb_target=2048), {}, None),
    "uniform-ws": ("uniform", 1024, dict(direct=False, runs=False, sv_max=8197), {}, None),
    "uniform-run": ("uniform", 1024, dict(direct=False, runs=("household",), sv_max=8197), {}, None),
    "halo-ws": ("halo-small", 64, dict(SMALL, direct=False, runs=False), {}, None),
    "halo-run": ("halo-run", 64, dict(SMALL, runs=("household",)), {}, None),
    "primary-run": ("primary", 64, dict(SMALL, runs=("household",), direct=False), {}, None),
    "presum-3": ("presum", None, dict(runs=False, presum=True), {}, None),
    "presum-batch2": ("batch2", None, dict(runs=False, presum=True), {}, "one-workgroup"),
    "presum-34": ("tables", None, dict(runs=False, presum=True), {}, None),
    "presum-wrap": ("wrap", None, dict(presum=True), {}, None),
}
CASES = dict({k: v + (None,) for k, v in LAYOUTS.items()}, **MORE)
EVERY = list(CASES)


def case_host(case):
    if case in LAYOUTS:
        return host_of(case)
    if case not in _HOSTS:
        wkey, sa, kw, _, tweak = CASES[case]
        w = world_of(wkey)
        kw = dict(kw)
        if sa is not None:
            kw["slices"] = (-(-w["n_ext"] // sa), sa)
        with pytest.MonkeyPatch.context() as m:
            if tweak == "no-rows":          # chunks that a descriptor cannot express walk the tile tables
                m.setattr(TL, "build_tiled", functools.partial(TL.build_tiled, multi_rows=False))
            _HOSTS[case] = compile_plan(w["n_agents"], w["edge_sets"], age=w["age"], sex=w["sex"], layout="tiled",
                                        n_ext_agents=w["n_ext"],
                                        nets_per_set={"leisure": sum(sp.edge_set == "leisure" for sp in w["specs"])}, **kw)
    return _HOSTS[case]


def case_engine(case, device):
    if case in LAYOUTS:
        return engine_of(case, device)
    if case not in _ENGINES:
        w = world_of(CASES[case][0])
        plan = DevicePlan(case_host(case), w["specs"], device, **CASES[case][3])
        if CASES[case][4] == "one-workgroup":      # the table buffer is sized for more
            assert plan.tiled_c.presum_wgs > 1
            plan.tiled_c.presum_wgs = 1
        _ENGINES[case] = InfectionEngine(plan)
    return _ENGINES[case]


def tiled_of(case, name):
    host = case_host(case)
    return host.sets[host.set_index[name]].tiled


def rules_of(case):
    return {s.name: "presum" for s in case_host(case).sets if s.tiled.presum and s.tiled.ell_k and s.n_edges > 0}


# ---- the restatement, the drive, the comparison ---------------------------------------------------------------------------------
def transmissions(w, seed, signed):
    """Zeros (about 30 %) and values in [2^-10, 1] - no product is then denormal; the transposed direction takes them
    with random signs."""
    rng = np.random.default_rng(seed)
    x = np.where(rng.random(w["n_ext"]) < 0.3, 0.0, rng.uniform(2.0 ** -10, 1.0, w["n_ext"]))
    if signed:
        x *= rng.choice([-1.0, 1.0], w["n_ext"])
    return x.astype(np.float32)


def restated(case, x, *, day_type, transpose, has_q, active=None, key=None):
    """{set: (cum bits [V, nk], flagged [V, nk])}.  The restatement does not know the geometry: with `key` it is
    computed once per (world, rule of each set, inputs) and shared by the cases of that world."""
    wkey = CASES[case][0]
    w = world_of(wkey)
    host = case_host(case)
    rules = rules_of(case)
    k = None
    if key is not None:       # (the inputs are part of the key: a hit is the restatement of exactly this drive)
        k = (key, wkey, tuple(sorted(rules)), day_type, transpose, has_q, tuple(active or w["active"]),
             hashlib.sha1(np.ascontiguousarray(x, dtype=np.float32).tobytes()).hexdigest())
        if k in _WANT:
            return _WANT[k]
    for s in host.sets:                                   # the window's input, as the plan has it
        v = w["edge_sets"][s.name]["venue"]
        assert s.max_venue_edges == (int(np.bincount(v).max()) if len(v) else 0)
    want = R1.restate(w["edge_sets"], {s.name: s.v_pcontact for s in host.sets}, w["specs"], active or w["active"],
                      w["betas"], x, rules=rules, age=w["age"], sex=w["sex"], stage=w["stage_ext"], q_thr=Q_THR,
                      has_quarantine=has_q, day_type=day_type, transpose=transpose)
    if k is not None:
        _WANT[k] = want
    return want


def drive(case, x, device, *, day_type, transpose, has_q, phase=7, active=None):
    """{set: cum [V, stride]} after step_phase `phase` on the transmissions x, every cum buffer pre-filled."""
    w = world_of(CASES[case][0])
    engine = case_engine(case, device)
    for c in engine.plan.cum:
        c.fill_(float(SENTINEL))
    if active is None and case in LAYOUTS:
        p = params_of(engine, day_type, transpose, has_q)
    else:
        p = engine.params(now=1.0, delta_time=1.0, day_type=day_type, active=active or w["active"], betas=w["betas"],
                          has_quarantine=has_q, q_threshold=Q_THR if has_q else math.inf)
        p.transpose = transpose
    bufs, io, _ = outputs(engine, w, p, device, x=x, want=("trans_susc", "agent_sums"))
    if has_q and w["n_ext"] > w["n_agents"]:         # the halo agents' q * x comes from the ranks that own them
        q = engine.q_transmission_buffer()
        halo = slice(w["n_agents"], w["n_ext"])
        q[halo] = torch.from_numpy(R1.source(x, w["stage_ext"], Q_THR, True, False)[halo]).to(device)
    engine.quarantine_transmission(bufs, p)
    engine.step_phase(bufs, p, io, phase)
    torch.cuda.synchronize()
    return {name: engine.plan.cum_of(name).cpu().numpy().copy() for name in w["edge_sets"]}


def compare(got, want, what):
    """Every venue of every active network as uint32; the columns behind the active networks and the sets without one
    keep the sentinel."""
    for name, cum in got.items():
        nk = want[name][0].shape[1] if name in want else 0
        if nk:
            assert cum.shape[0] == want[name][0].shape[0] and cum.shape[1] >= nk
            assert_bits(np.ascontiguousarray(cum[:, :nk]).ravel(), np.ascontiguousarray(want[name][0]).ravel(), [],
                        f"{what} cum of {name} [venue * {nk} + network]")
        assert (cum[:, nk:].view(np.uint32) == SENTINEL.view(np.uint32)).all(), f"{what}: {name} behind its networks"


def check(case, x, device, what, *, day_type, transpose, has_q, key=None, phase=7, active=None):
    want = restated(case, x, day_type=day_type, transpose=transpose, has_q=has_q, key=key, active=active)
    got = drive(case, x, device, day_type=day_type, transpose=transpose, has_q=has_q, phase=phase, active=active)
    compare(got, want, f"{case} {what} day {day_type} transpose {transpose} quarantine {has_q} phase {phase}")
    return got, want


# ---- the forms ---------------------------------------------------------------------------------------------------------------------
def scatter_branches(host):
    """{branch: [(set, slice)]} of scatter_set for the sets phase A scatters through descriptors.  csrc/gj_tiled.h:
    kLongSegmentChunks = 384, kNtTileEdges = GJ_NT_TILE_EDGES = 1024, kWave = 64; a set with narrow descriptors takes
      "nt"     n_chunks >= 384 and n_chunks * 64 >= 1024 * J     16-chunk batches, non-temporal stores
      "long"   n_chunks >= 384 and not that                      16-chunk batches
      "short"  n_chunks < 384                                    8-chunk batches
    and a set with wide descriptors always the last."""
    out = {"nt": [], "long": [], "short": []}
    for s in host.sets:
        t = s.tiled
        if t.n_edges == 0 or t.slot_idx is not None or t.presum:
            continue
        for sl, n in enumerate(np.diff(_host(t.chunk_ptr).astype(np.int64))):
            if n == 0:
                continue
            if not t.desc_wide and n >= 384:
                out["nt" if 64 * n >= 1024 * t.n_blocks else "long"].append((s.name, sl))
            else:
                out["short"].append((s.name, sl))
    return out


def wave_windows(t, j, lv):
    """The 512-slot windows of block j as a wave of phase B reads them (64 lanes x 8 slots from the block's first
    slot): (windows that hold local venue lv only, windows that hold it and something else)."""
    e0, e1 = int(_host(t.blk_e0)[j]), int(_host(t.blk_e0)[j + 1])
    e = _host(t.e_lv)[e0:e1].astype(np.int64)
    pure = mixed = 0
    for p in range(0, len(e), 512):
        win = e[p:p + 512]
        has = (win == lv).any()
        pure += int(has and len(win) == 512 and (win == lv).all())
        mixed += int(has and not (win == lv).all())
    return pure, mixed


def slot_agents(host, name):
    """The agent of every block-major slot of a set (-1: a pad slot), from the plan's slice-major arrays."""
    t = host.sets[host.set_index[name]].tiled
    S, J, SA = t.n_slices, t.n_blocks, host.slice_agents
    sptr, jpos, a_la = _host(t.tile_sptr).astype(np.int64), _host(t.tile_jpos).astype(np.int64), _host(t.a_la).astype(np.int64)
    e_lv = _host(t.e_lv)
    agents = np.full(len(e_lv), -1, dtype=np.int64)
    for s in range(S):
        for j in range(J):
            a, b = sptr[s * J + j], sptr[s * J + j + 1]
            agents[jpos[s * J + j]:jpos[s * J + j] + (b - a)] = s * SA + a_la[a:b]
    agents[e_lv.astype(np.int64) == 0xFFFF] = -1
    return agents


def test_every_form_is_reached(device):
    """(a) the forms of the pass-2 file's layouts, as that file asserts them; (b) each row of the table of forms that
    those layouts lack, on the plans' own arrays."""
    seen = set()
    for layout in ALL:
        seen |= forms_seen(layout)
    assert seen >= {"workspace", "direct", "run", "narrow", "wide", "explicit", "multi_slots", "tile_pad", "presum", "K=2",
                    "K=4", "K=8"}, seen
    assert tiled_of("direct-presum", "school").presum and case_engine("direct-presum", device).plan.tiled_c.direct_table_floats == 24
    assert {host_of(k).slice_agents for k in ALL} >= {64, 4160, 19840}
    assert any(t is not None for t in case_engine("direct", device).plan.lv8)
    assert not any(t is not None for t in case_engine("direct-some", device).plan.lv8)
    # the table walk: no rows of explicit slots, most chunks beyond their descriptor
    for case, wide in (("walk-narrow", False), ("walk-wide", True)):
        walks = {s.name: TL.walk_share(s.tiled) for s in case_host(case).sets if s.n_edges}
        assert all(s.tiled.multi_slots is None and s.tiled.slot_idx is None for s in case_host(case).sets)
        assert all(bool(s.tiled.desc_wide) == wide for s in case_host(case).sets if s.n_edges)
        assert max(walks.values()) > 0.5 and sum(v > 0.5 for v in walks.values()) >= 2, walks
    # phase A's three batch forms
    branches = {k: scatter_branches(case_host(k)) for k in ("quads-ws-19840", "quads-ws-4160", "quads-ws-19840-blocks")}
    assert branches["quads-ws-19840"]["nt"] and branches["quads-ws-4160"]["short"], branches
    assert branches["quads-ws-19840-blocks"]["long"], {k: len(v) for k, v in branches["quads-ws-19840-blocks"].items()}
    # both sources in one launch, a partial last slice: household reads x, the others q * x (quarantine on), 1003 = 15 * 64 + 43
    # Under quarantine the two source arrays differ at agents who attend a household (scattered from x) and a school
    # (scattered from q * x), and phase A scatters both sets in ws-narrow: one launch, two passes over its slices.
    w = world_of("small")
    x = transmissions(w, 300, signed=False)
    differ = R1.bits(R1.source(x, w["stage_ext"], Q_THR, True, False)) != R1.bits(x)
    attends = {n: np.bincount(w["edge_sets"][n]["agent"], minlength=w["n_ext"]) > 0 for n in ("household", "school")}
    assert (differ & attends["household"] & attends["school"]).sum() >= 20
    kinds = {sp.edge_set: sp.mask_kind for sp in w["specs"]}
    assert kinds["household"] == N.MASK_RAW and kinds["school"] == N.MASK_Q and kinds["leisure"] == N.MASK_QL
    for n in ("household", "school", "leisure"):
        t = tiled_of("ws-narrow", n)
        assert t.n_edges > 0 and not t.presum and t.runs is None and len(_host(t.a_la)) == len(w["edge_sets"][n]["agent"])
    # the wave-uniform venue of a plain set, the window of 2^13, the cum write-out in two trips
    w = world_of("uniform")
    host = case_host("uniform-ws")
    t = tiled_of("uniform-ws", "school")
    assert t.e_cls is None and not t.ell_k and t.runs is None
    pure, mixed = wave_windows(t, 0, 0)
    assert pure >= 1 and mixed >= 1, (pure, mixed)
    mve = host.sets[host.set_index["school"]].max_venue_edges
    assert mve == 5000 and R1.term_limit_bits(mve) == int(F32(2.0 ** 13).view(np.uint32))
    sizes = np.diff(_host(tiled_of("uniform-ws", "university").blk_v0))
    assert sizes.max() > 8 * 1024 and 1 <= sizes.min() <= 7, sizes          # kCumBatch x 1 024 venues per trip
    for name in ("school", "university", "household"):
        es, pc = w["edge_sets"][name], host.sets[host.set_index[name]].v_pcontact
        assert list(es["people"][-3:]) == [0, 1, 2] and list(pc[-3:]) == [0.0, 1.0, 1.0]
        assert list(es["people"][1:4]) == [0, 1, 2] and list(pc[1:4]) == [0.0, 1.0, 1.0]
        assert not np.isin(np.arange(len(pc) - 3, len(pc)), es["venue"]).any() and np.isin([1, 2, 3], es["venue"]).all()
    # halo agents
    for case in ("halo-ws", "halo-run"):
        host, w = case_host(case), world_of(CASES[case][0])
        assert (host.n_agents, host.n_ext_agents, host.n_agents % host.slice_agents) == (960, 1003, 0)
        for s in host.sets:
            a = w["edge_sets"][s.name]["agent"]
            if len(a) == 0:
                continue
            n_halo = int((a >= 960).sum())
            assert n_halo >= (10 if s.name != "university" else 0) and not s.tiled.presum, (case, s.name)
            agents = slot_agents(host, s.name)
            assert int((agents >= 960).sum()) == n_halo, (case, s.name)      # every halo edge has its slot
    assert tiled_of("halo-run", "household").runs is not None and tiled_of("halo-run", "school").ell_k
    assert all(s.tiled.runs is None and not s.tiled.ell_k for s in case_host("halo-ws").sets)
    # the run form with every agent primary
    rf = tiled_of("primary-run", "household").runs
    r0 = _host(rf.blk_r0).astype(np.int64)
    assert r0[-1] == 1003 and 1003 % 8 != 0 and len(r0) - 1 >= 3 and (r0[1:-1] % 8 != 0).any(), r0
    assert rf.n_primary == 1003 and tiled_of("primary-run", "household").n_edges == 40
    assert tiled_of("uniform-run", "household").runs.n_primary == 9001
    # presum: three sets in one launch over three workgroups, the reduce's waves straddle sets
    host, plan = case_host("presum-3"), case_engine("presum-3", device).plan
    # agents per workgroup: the launch layer's rule, which the plan does not expose - tiled_presum in
    # csrc/gradjune_hip.hip: apw = ceil(n_agents / presum_wgs), rounded up to a multiple of 64
    assert plan.tiled_c.presum_wgs == 3 and -(-(-(-9001 // 3)) // 64) * 64 == 3008 and 9001 - 2 * 3008 == 2985 and 2985 % 4
    assert {s.name: (bool(s.tiled.presum), s.tiled.ell_k) for s in host.sets} == {"company": (True, 2), "school": (True, 8),
                                                                                 "leisure": (True, 4)}
    entries = [host.sets[host.set_index[n]].n_venues * k for n, k in (("school", 1), ("company", 1), ("leisure", 2))]   # launch order
    assert plan.c.sets[host.set_index["leisure"]].cum_stride == 2 and all(e % 64 for e in np.cumsum(entries)[:-1]), entries
    plan = case_engine("presum-batch2", device).plan
    assert plan.tiled_c.presum_wgs == 1 and -(-13001 // 4) > 3 * 1024 and tiled_of("presum-batch2", "company").presum
    assert plan.keep[0]["presum"].numel() == 4 * (300 + 3)
    assert case_engine("presum-34", device).plan.tiled_c.presum_wgs == 34 and tiled_of("presum-34", "company").presum


# ---- 1. finite transmissions, every case ----------------------------------------------------------------------------------------
def empty_venues(w):
    return {name: np.setdiff1d(np.arange(len(es["people"])), es["venue"]) for name, es in w["edge_sets"].items()}


@pytest.mark.parametrize("case", EVERY)
def test_cum_of_every_venue_bit_for_bit(device, case):
    """Forward (the values as they are) and transposed (random signs), quarantine off and on, day type 0 with the
    forward and 1 with the transposed direction and the other way round under quarantine."""
    wkey = CASES[case][0]
    w = world_of(wkey)
    for transpose in (0, 1):
        x = transmissions(w, 300 + transpose, signed=bool(transpose))
        for has_q in (False, True):
            day_type = transpose ^ int(has_q)
            got, want = check(case, x, device, "finite", day_type=day_type, transpose=transpose, has_q=has_q, key="finite")
            for name, (cum, flagged) in want.items():
                assert not flagged.any() and np.isfinite(R1.f32_of(cum)).all()
                if len(w["edge_sets"][name]["agent"]):
                    assert np.abs(R1.f32_of(cum)).max() > 0
                assert (got[name][empty_venues(w)[name]][:, :cum.shape[1]].view(np.uint32) == 0).all()     # +0.0
    assert 100 < (~(w["stage_ext"] < Q_THR)).sum() < w["n_ext"] - 100
    if "care_home" in w["edge_sets"]:                 # an active set without an edge is written: +0.0 everywhere
        assert len(w["edge_sets"]["care_home"]["agent"]) == 0 and (got["care_home"].view(np.uint32) == 0).all()


PHASE8 = ["ws-narrow", "ws-explicit", "direct", "direct-presum", "run", "quads-ws-4160", "uniform-ws", "halo-run"]


@pytest.mark.parametrize("case", PHASE8)
def test_phase_c_does_not_touch_cum(device, case):
    w = world_of(CASES[case][0])
    x = transmissions(w, 301, signed=True)
    kw = dict(day_type=1, transpose=1, has_q=True)
    after7, _ = check(case, x, device, "phase 7", key="phase 8", **kw)
    after8, _ = check(case, x, device, "phase 8", key="phase 8", phase=8, **kw)
    for name in after7:
        assert np.array_equal(after7[name].view(np.uint32), after8[name].view(np.uint32)), (case, name)


SOME_ACTIVE = ["university", "company", "pub", "gym", "household"]      # no school, no care_home, leisure without its second network


@pytest.mark.parametrize("case", ["ws-narrow", "direct", "direct-presum", "run"])
def test_what_is_not_active_keeps_the_sentinel(device, case):
    """Column k of cum is the k-th ACTIVE network of the set: with care_visit off, gym moves to column 1 and column 2
    keeps the sentinel, as does every venue of a set without an active network (school; care_home, which has no edge)."""
    w = world_of(CASES[case][0])
    x = transmissions(w, 302, signed=False)
    got, want = check(case, x, device, "some active", day_type=0, transpose=0, has_q=True, active=SOME_ACTIVE)
    assert set(want) == {"university", "company", "leisure", "household"} and want["leisure"][0].shape[1] == 2
    sentinel = SENTINEL.view(np.uint32)
    assert (got["school"].view(np.uint32) == sentinel).all() and (got["care_home"].view(np.uint32) == sentinel).all()
    assert (got["leisure"][:, 2].view(np.uint32) == sentinel).all() and not (got["leisure"][:, :2] == SENTINEL).any()
    # gym in column 1 is what it is in column 2 with every network active (the same beta, table and kind)
    everything, _ = check(case, x, device, "all active", day_type=0, transpose=0, has_q=True)
    assert np.array_equal(got["leisure"][:, 1].view(np.uint32), everything["leisure"][:, 2].view(np.uint32))


# ---- 2. values that cannot be summed ---------------------------------------------------------------------------------------------
def run_positions(lv, real):
    """Positions inside a run of equal venues within a group of eight (both neighbours the same venue) and positions
    that end a run of two or more; `real`: the positions that hold an edge."""
    p = np.arange(len(lv))
    prev_same, next_same = np.zeros(len(lv), dtype=bool), np.zeros(len(lv), dtype=bool)
    prev_same[1:] = (lv[1:] == lv[:-1]) & (p[1:] % 8 > 0)
    next_same[:-1] = (lv[:-1] == lv[1:]) & (p[:-1] % 8 < 7)
    return np.flatnonzero(real & prev_same & next_same), np.flatnonzero(real & prev_same & ~next_same)


def special_agents(case, name, how):
    """Agents of set `name` by where the plan puts their term:
      slots    (workspace form) a slot inside a run of its lane's eight slots, and one that ends a run
      primary  (run form) a primary agent inside a run of its group of eight agents, and one that ends a run
      uniform  an agent of venue 0 inside a window that a wave sums as one venue, the one whose slot ends venue 0's run
               in the window that venue 0 shares, and one of another venue of that window
      rows     (presum) an agent of the first workgroup and the last agent with an edge (the last workgroup)
    plus - where the world has one - an attendee of a venue whose p_contact is 0."""
    host = case_host(case)
    w = world_of(CASES[case][0])
    t = tiled_of(case, name)
    es = w["edge_sets"][name]
    if how == "slots":
        agents = slot_agents(host, name)
        blk = np.searchsorted(_host(t.blk_e0).astype(np.int64), np.arange(len(agents)), side="right")
        inside, end = run_positions(_host(t.e_lv).astype(np.int64) + 65536 * blk, agents >= 0)
        chosen = [int(agents[inside[len(inside) // 2]]), int(agents[end[len(end) // 3]])]
    elif how == "primary":
        vmin = _host(t.runs.vmin).astype(np.int64)       # agent a is a slot of its group of eight; equal vmin: one block, one run
        inside, end = run_positions(vmin, vmin != TL.NO_VENUE)
        chosen = [int(inside[len(inside) // 2]), int(end[len(end) // 3])]
    elif how == "uniform":
        agents = slot_agents(host, name)
        e = _host(t.e_lv).astype(np.int64)
        e0 = int(_host(t.blk_e0)[0])
        wins = [(p, e[p:p + 512]) for p in range(e0, int(_host(t.blk_e0)[1]), 512)]
        pure = next(p for p, win in wins if len(win) == 512 and (win == 0).all())
        mixed = next(p for p, win in wins if (win == 0).any() and not (win == 0).all())
        last0 = mixed + int(np.flatnonzero(e[mixed:mixed + 512] == 0).max())
        other = mixed + int(np.flatnonzero((e[mixed:mixed + 512] != 0) & (e[mixed:mixed + 512] != 0xFFFF)).min())
        chosen = [int(agents[pure + 8 * 17 + 3]), int(agents[last0]), int(agents[other])]
    else:
        with_edge = np.unique(es["agent"])
        chosen = [int(with_edge[len(with_edge) // 7]), int(with_edge[-1])]
    pc = host.sets[host.set_index[name]].v_pcontact
    zero = np.flatnonzero(pc[es["venue"]] == 0)
    if len(zero):
        chosen.append(int(es["agent"][zero[0]]))
    assert len(set(chosen)) == len(chosen) and all(0 <= a < w["n_ext"] for a in chosen)
    return chosen


def special_input(w, chosen, value, transpose):
    x = transmissions(w, 310 + transpose, signed=bool(transpose))
    x[chosen] = value
    return x


# case, the set the agents are chosen in, how
SPECIALS = [("ws-narrow", "university", "slots"), ("ws-narrow", "leisure", "slots"), ("ws-explicit", "school", "slots"),
            ("walk-wide", "school", "slots"), ("uniform-ws", "household", "slots"), ("uniform-ws", "school", "uniform"),
            ("halo-ws", "school", "slots"), ("run", "household", "primary"), ("primary-run", "household", "primary"),
            ("uniform-run", "household", "primary"), ("direct-presum", "school", "rows"), ("presum-3", "company", "rows"),
            ("presum-3", "leisure", "rows"), ("presum-batch2", "company", "rows")]


@pytest.mark.parametrize("case,name,how", SPECIALS)
def test_values_that_cannot_be_summed(device, case, name, how):
    """A NaN, +-inf, +-3e4, the set's window itself and the next float32 above it (negative values only transposed) at
    the chosen agents.  Default rule: +-1e30 x beta x p_contact with one flag, NaN with both, 0.0 where p_contact is 0;
    presum: NaN, also where p_contact is 0.  The window itself is summed."""
    w = world_of(CASES[case][0])
    host = case_host(case)
    s = host.sets[host.set_index[name]]
    es = w["edge_sets"][name]
    chosen = special_agents(case, name, how)
    presum = rules_of(case).get(name) == "presum"
    raw = name == "household"
    window = R1.f32_of(np.array([R1.term_limit_bits(s.max_venue_edges)], dtype=np.uint32))[0]
    above = np.nextafter(window, F32(np.inf))
    beta = R1.nets_of(w["specs"], w["active"], w["betas"], name)[0][0]
    if CASES[case][0] in ("uniform", "primary", "presum"):      # these worlds have attended venues with p_contact 0
        assert any(s.v_pcontact[v] == 0 for a in chosen for v in es["venue"][es["agent"] == a])
    for transpose in (0, 1):
        values = [F32(np.nan), F32(np.inf), F32(3.0e4), window, above]
        if transpose:
            values += [F32(-np.inf), F32(-3.0e4), -window, -above]
        for value in values:
            x = special_input(w, chosen, value, transpose)
            has_q = bool(np.isnan(value))                 # (q * NaN is a NaN: a quarantined agent's NaN stays)
            got, want = check(case, x, device, f"{value!r} at {chosen}", day_type=0, transpose=transpose, has_q=has_q)
            if s.tiled.e_cls is not None:                 # a class weight in [0, 1) stands between x and the term:
                continue                                  # the equality with the restatement is the whole check
            cum, flagged = want[name]
            wf = R1.f32_of(cum)[:, 0]
            for a in chosen:
                for v in np.unique(es["venue"][es["agent"] == a]):
                    bp = F32(F32(beta) * s.v_pcontact[v])
                    if abs(value) == window:              # the window itself is summed
                        assert not flagged[v, 0] and np.isfinite(wf[v])
                    elif presum or np.isnan(value):
                        assert flagged[v, 0] and np.isnan(wf[v]) and np.isnan(got[name][v, 0])
                    elif bp == 0:
                        assert flagged[v, 0] and wf[v] == 0.0 and got[name][v, 0] == 0.0
                    else:
                        assert flagged[v, 0] and wf[v] == F32(bp * F32(math.copysign(1.0e30, value)))
            if abs(value) == window:
                assert np.isfinite(wf).all()


# ---- 3. the rounding of a term ------------------------------------------------------------------------------------------------------
def small_terms(w, seed, signed):
    """A float32 of 2^-13 or more is a whole number of 2^-36: the values of `transmissions` reach the rounding of to_fx
    only through a leisure set's class weight.  These do in every set: magnitudes spread over 2^-45 ... 2^-12, and
    every fifth value an odd multiple of 2^-37 - a tie, which rint takes to the even neighbour."""
    rng = np.random.default_rng(seed)
    n = w["n_ext"]
    x = np.exp2(rng.uniform(-45.0, -12.0, n))
    x[::5] = (2 * rng.integers(0, 64, len(x[::5])) + 1) * 2.0 ** -37
    if signed:
        x *= rng.choice([-1.0, 1.0], n)
    return x.astype(np.float32)


@pytest.mark.parametrize("case", ["ws-narrow", "direct-presum", "run", "uniform-ws", "uniform-run", "halo-run", "primary-run",
                                  "presum-3", "presum-batch2"])
def test_terms_below_the_resolution_round_half_to_even(device, case):
    w = world_of(CASES[case][0])
    for transpose in (0, 1):
        x = small_terms(w, 320 + transpose, signed=bool(transpose))
        got, want = check(case, x, device, "small terms", day_type=transpose, transpose=transpose, has_q=bool(transpose))
        assert not any(flagged.any() for _, flagged in want.values())
        ties = np.abs(x[::5]).astype(np.float64) * 2.0 ** 37
        assert (ties == np.rint(ties)).all() and (ties % 2 == 1).all()


# ---- 4. the two roundings of from_fx ---------------------------------------------------------------------------------------------
def double_rounding_input(case, name):
    """(x, venue): zero but for attendees of one venue of a plain set - 2^19 / window terms of the set's window, one of
    2^-5 and one of 2^-36.  The exact sum 2^19 + 2^-5 + 2^-36 loses its last term on the way to float64 and then lies
    on a tie of float32: s = 524288.0; rounded once it would be 524288.0625."""
    w = world_of(CASES[case][0])
    host = case_host(case)
    s = host.sets[host.set_index[name]]
    es = w["edge_sets"][name]
    window = float(R1.f32_of(np.array([R1.term_limit_bits(s.max_venue_edges)], dtype=np.uint32))[0])
    n_big = int(2.0 ** 19 / window)
    pair = es["agent"] * s.n_venues + es["venue"]                        # agents with ONE edge to the venue
    _, inverse, count = np.unique(pair, return_inverse=True, return_counts=True)
    ok = (count[inverse] == 1) & (s.v_pcontact[es["venue"]] > 0)
    venue = int(np.argmax(np.bincount(es["venue"][ok], minlength=s.n_venues)))
    agents = es["agent"][ok & (es["venue"] == venue)]
    assert len(agents) >= n_big + 2, (case, name, len(agents))
    x = np.zeros(w["n_ext"], dtype=np.float32)
    x[agents[:n_big]] = window
    x[agents[n_big]], x[agents[n_big + 1]] = 2.0 ** -5, 2.0 ** -36
    return x, venue


ROUNDINGS = [("uniform-ws", "school"), ("run", "school"), ("halo-ws", "school"), ("direct-presum", "school"),
             ("presum-3", "company"), ("quads-ws-4160", "university")]


@pytest.mark.parametrize("case,name", ROUNDINGS)
def test_the_two_roundings_of_the_read_back(device, case, name):
    host = case_host(case)
    s = host.sets[host.set_index[name]]
    w = world_of(CASES[case][0])
    x, venue = double_rounding_input(case, name)
    beta = R1.nets_of(w["specs"], w["active"], w["betas"], name)[0][0]
    bp = F32(F32(beta) * s.v_pcontact[venue])
    got, want = check(case, x, device, "double rounding", day_type=0, transpose=0, has_q=False)
    twice, once = F32(bp * F32(524288.0)), F32(bp * F32(524288.0625))
    assert twice != once and R1.f32_of(want[name][0])[venue, 0] == twice and got[name][venue, 0] == twice


# ---- 5. the wrap -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("term", [1000.0, 10000.0])
def test_presum_sums_of_a_large_venue_never_wrap(device, term):
    """20 000 attendees of ONE venue with a transmission of 1 000 / 10 000 each, presum=True.  Every workgroup's table
    stays inside the 64 bits; the sum of the five tables does not for 10 000: 2e8 x 2^36 > 2^63.  Presum takes the set's
    term window (2^26 / 32 768 = 2 048) as phase B does, so 1 000 is summed exactly and 10 000 reads back NaN (presum's
    one-flag rule) - never a finite value that is not the sum.  (Before the window was handed to k_tile_presum the
    terms of 10 000 passed its fixed check |x| <= 16 384 and cum read back negative.)"""
    case = "presum-wrap"
    host = case_host(case)
    t = host.sets[0].tiled
    assert t.presum and t.ell_k == 2 and host.sets[0].max_venue_edges == 20_000
    assert case_engine(case, device).plan.tiled_c.presum_wgs == 5
    assert R1.term_limit_bits(20_000) == int(F32(2048.0).view(np.uint32))
    x = np.full(20_000, term, dtype=np.float32)
    got, want = check(case, x, device, f"term {term}", day_type=0, transpose=0, has_q=False)
    value, wanted = got["school"][0, 0], R1.f32_of(want["school"][0])[0, 0]
    print(f"term {term}: cum {value!r}, restatement {wanted!r}")
    if term == 1000.0:
        assert wanted == F32(F32(0.5) * host.sets[0].v_pcontact[0]) * F32(2.0e7) and value == wanted
    else:
        assert np.isnan(wanted) and np.isnan(value)
