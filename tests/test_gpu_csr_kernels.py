"""GPU: the two passes of the CSR layout per venue and per agent - k_venue_reduce, k_combine_long and the sum loop of
k_agent_gather of csrc/gradjune_hip.hip - BIT FOR BIT against the numpy restatement tests/gj_csr_ref.py.

The library is built with -ffp-contract=off and group_sum is a fixed butterfly: every sum of these kernels is a fixed
sequence of float32 multiplies and adds, which the restatement repeats from the plan's own arrays (tests/test_csr_ref.py
checks it on the CPU: against torch's scatter_add_, against float64 on dyadic inputs and inside the float32 bounds).
`cum` of EVERY venue of EVERY active network and `trans_susc` of EVERY owned agent are compared as uint32, NaN by position.
There is no tolerance in this file.

Drive: the cum buffers filled with 123.0, the transmissions into the buffer, quarantine_transmission, step_phase 1
(k_venue_reduce + k_combine_long), synchronize, plan.cum_of(set) of every set; then step_phase 4 (k_agent_gather without
sampling) and trans_susc.  The columns behind a set's active networks and the sets without one keep the sentinel.

Worlds, each the smallest at which its paths exist (test_every_form_is_reached asserts them on the plans' own fields);
every world in a "general" variant (`people` = attendance + 0 .. 2 with 0, 1 and 2 on attended venues, random tables with
zeros, susceptibility 0 / 0.4 / 1) and a "dyadic" one (same edges; tests/test_csr_ref.py says why it is exact):
  lanes        one set per lane width (block mean degree <= 6, <= 24, <= 96, > 96): a block of exactly 2 048 edges, one of
               2 048 venues, one of one edge, a 64-lane block with a venue of one edge and one of none, a one-lane block with
               a venue of 1 500 edges among single-edge venues, venues nobody attends (first, last, after a long venue)
  long         a plain set with venues of 2 048, 2 049, 8 192, 8 193, 8 192 + 1 023 / 1 024 / 1 025 and 3 x 8 192 + 5 edges
               (first and last venue long, two long venues adjacent) and a leisure set with rows of 1, 2 and 4 slots
  nets         a leisure set of 8 networks (care_visit among them) with STREAM and LONG venues, launched with 8, 2 and 1
               of them (a single QL network: the multi-network branch with nk == 1), a set without an active network, a
               plain set with TWO networks and a long venue, quarantine on and off, both day types, the household set raw
  agents-N     N = 1, 255, 256, 257, 1 003 owned agents + halo agents that attend owned venues; agents without an edge in
               one set or in any, one agent with 300 edges
Transmission vectors per world: dyadic (on the dyadic variant), general random with most entries 0, eight one-hot probe
vectors (one attendee per venue, at row position 0, the last, either side of the lane count and of 256 / 1 024 / 8 192)
and one with an inf and a NaN."""
import math

import numpy as np
import pytest
import torch

import gj_csr_ref as RC
from grad_june_amd import _native as N
from grad_june_amd.engine import AgentBuffers, InfectionEngine
from grad_june_amd.plan import LONG_CHUNK, MAX_ROWS_PER_BLOCK, DevicePlan, NetworkSpec, compile_plan

pytestmark = pytest.mark.gpu

F32 = np.float32
Q_THR = 4.0
SENTINEL = F32(123.0)
LEISURE8 = ["pub", "gym", "grocery", "visit", "care_visit", "cinema", "park", "club"]
N_PROBES = 8


# ---- worlds --------------------------------------------------------------------------------------------------------------
def edges_of(rng, degs, pool):
    """COO lists of a set whose venue v has degs[v] attendees, drawn from `pool` WITH replacement (so there are duplicated
    (agent, venue) pairs), in shuffled order (the plan's stable sort then has something to keep)."""
    degs = np.asarray(degs, dtype=np.int64)
    venue = np.repeat(np.arange(len(degs)), degs)
    agent = rng.choice(np.asarray(pool, dtype=np.int64), len(venue))
    perm = rng.permutation(len(venue))
    return {"agent": agent[perm].astype(np.int64), "venue": venue[perm].astype(np.int64), "n_venues": len(degs)}


def finish_world(rng, A, n_ext, sets, nets, launches):
    """nets: (name, set, kind) in the plan's order; launches: dict(active, has_q, day_type)."""
    age = rng.integers(0, 100, n_ext)
    age[::5], age[1::5] = 75, 76
    stage = rng.integers(1, 7, n_ext).astype(np.float32)
    variants = {}
    for variant in ("general", "dyadic"):
        people, tables = {}, {}
        for name, es in sets.items():
            V = es["n_venues"]
            if variant == "general":
                p = np.bincount(es["venue"], minlength=V) + rng.integers(0, 3, V)
                attended = np.unique(es["venue"])
                p[attended[len(attended) // 2:][:3]] = [0, 1, 2][:len(attended[len(attended) // 2:][:3])]
            else:
                p = rng.choice([2, 3, 5, 9], V)
            people[name] = p.astype(np.int64)
        for n, _, kind in nets:
            if kind >= N.MASK_QL:
                t = rng.random((2, 2, 100))
                tables[n] = (np.where(rng.random((2, 2, 100)) < 0.1, 0.0, t) if variant == "general"
                             else rng.choice([0.0, 0.5, 1.0], (2, 2, 100))).astype(np.float32)
        susc = rng.choice([0.0, 0.4, 1.0] if variant == "general" else [0.0, 0.5, 1.0], A).astype(np.float32)
        betas = {n: float(F32(0.5 + 0.37 * i)) if variant == "general" else 2.0 ** (i % 3 - 1) for i, (n, _, _) in enumerate(nets)}
        variants[variant] = dict(people=people, tables=tables, susc=susc, betas=betas)
    return dict(n_agents=A, n_ext=n_ext, age=age, sex=rng.integers(0, 2, n_ext), stage_ext=stage, sets=sets, nets=nets,
                launches=launches, variants=variants)


def lanes_world():
    rng = np.random.default_rng(1101)
    A = 3000
    pool = np.arange(A)
    d = rng.integers(0, 2, MAX_ROWS_PER_BLOCK)
    d[0] = 0
    s1 = np.concatenate([d, [1] * 150, [1500], [1] * 150, [2049], [0, 1], [2049], [1, 0]])
    s4 = np.concatenate([[16] * 128, [5, 3, 4, 0, 8], rng.integers(7, 25, 80)])
    s16 = np.concatenate([[15, 16, 17, 31, 32, 33, 0, 1], rng.integers(25, 97, 40)])
    s64 = [300, 63, 64, 65, 127, 128, 129, 500, 255, 256, 257, 1800, 1000, 1, 0, 900, 400, 97, 700]
    sets = {"s1": edges_of(rng, s1, pool), "s4": edges_of(rng, s4, pool), "s16": edges_of(rng, s16, pool),
            "s64": edges_of(rng, s64, pool)}
    nets = [("n1", "s1", N.MASK_RAW), ("n4", "s4", N.MASK_Q), ("n16", "s16", N.MASK_Q), ("n64", "s64", N.MASK_Q)]
    active = [n for n, _, _ in nets]
    return finish_world(rng, A, A, sets, nets, [dict(active=active, has_q=True, day_type=0),
                                                dict(active=active[::-1], has_q=False, day_type=1)])


BIG = [2049, 3, 2048, LONG_CHUNK, LONG_CHUNK + 1, 0, LONG_CHUNK + 1023, 5, LONG_CHUNK + 1024, LONG_CHUNK + 1025, 7,
       3 * LONG_CHUNK + 5]
LEI = [2049, LONG_CHUNK + 1, 2, 3 * LONG_CHUNK + 5]


def long_world():
    rng = np.random.default_rng(1102)
    A = 6000
    sets = {"big": edges_of(rng, BIG, np.arange(A)), "lei": edges_of(rng, LEI, np.arange(A))}
    nets = [("plain", "big", N.MASK_Q), ("pub", "lei", N.MASK_QL), ("care_visit", "lei", N.MASK_QL_AGE75)]
    return finish_world(rng, A, A, sets, nets, [dict(active=["plain", "pub", "care_visit"], has_q=True, day_type=1),
                                                dict(active=["care_visit", "pub", "plain"], has_q=False, day_type=0)])


def nets_world():
    rng = np.random.default_rng(1103)
    A = 2500
    pool = np.arange(A)
    sets = {"household": edges_of(rng, rng.integers(1, 6, 600), pool),
            "school": edges_of(rng, rng.integers(0, 40, 60), pool),
            "company": edges_of(rng, rng.integers(0, 10, 100), pool),
            "leisure": edges_of(rng, np.concatenate([[3, 2100, 0, 40, 1, 700, 9, 2, 2], rng.integers(0, 30, 40)]), pool),
            "dual": edges_of(rng, [5, 2500, 12, 0, 300], pool)}
    nets = ([("school", "school", N.MASK_Q), ("company", "company", N.MASK_Q)]
            + [(n, "leisure", N.MASK_QL_AGE75 if n == "care_visit" else N.MASK_QL) for n in LEISURE8]
            + [("dual_a", "dual", N.MASK_Q), ("dual_b", "dual", N.MASK_Q), ("household", "household", N.MASK_RAW)])
    launches = [dict(active=["school"] + LEISURE8 + ["dual_a", "dual_b", "household"], has_q=True, day_type=0),
                dict(active=["household", "pub", "care_visit"], has_q=False, day_type=1),
                dict(active=["gym", "school"], has_q=True, day_type=1),
                dict(active=["care_visit", "dual_b"], has_q=False, day_type=0)]
    return finish_world(rng, A, A, sets, nets, launches)


def agents_world(A):
    rng = np.random.default_rng(1200 + A)
    n_ext = A + (43 if A > 1000 else 5)
    halo = np.arange(A, n_ext)
    owned = np.arange(A)
    some = owned[(owned % 7 != 3) | (owned == 0)]                   # the others have no edge at all
    Vh, Vs, Vl = max(2, A // 3), max(1, A // 20), max(3, A // 10)

    def coo(agent, V):
        agent = np.asarray(agent, dtype=np.int64)
        perm = rng.permutation(len(agent))
        return {"agent": agent[perm], "venue": rng.integers(0, V, len(agent))[perm].astype(np.int64), "n_venues": V + 2}

    in_school = some[some % 3 != 1]
    in_leisure = some[some % 2 == 0]
    sets = {"household": coo(np.concatenate([some, halo, halo]), Vh),
            "school": coo(np.concatenate([np.repeat(in_school, rng.integers(1, 3, len(in_school))), halo]), Vs),
            "leisure": coo(np.concatenate([np.repeat(in_leisure, rng.integers(0, 4, len(in_leisure))), np.zeros(300, np.int64),
                                           np.repeat(halo, 3)]), Vl)}
    nets = [("school", "school", N.MASK_Q), ("pub", "leisure", N.MASK_QL), ("care_visit", "leisure", N.MASK_QL_AGE75),
            ("household", "household", N.MASK_RAW)]
    active = [n for n, _, _ in nets]
    return finish_world(rng, A, n_ext, sets, nets, [dict(active=active, has_q=True, day_type=0),
                                                    dict(active=active[::-1][:1] + active[:3], has_q=False, day_type=1)])


AGENT_COUNTS = (1, 255, 256, 257, 1003)
WORLDS = dict({"lanes": lanes_world, "long": long_world, "nets": nets_world},
              **{f"agents-{A}": (lambda A=A: agents_world(A)) for A in AGENT_COUNTS})
EVERY = list(WORLDS)
_WORLDS, _HOSTS, _ENGINES, _WANT = {}, {}, {}, {}


def world_of(key):
    if key not in _WORLDS:
        _WORLDS[key] = WORLDS[key]()
    return _WORLDS[key]


def specs_of(key, variant):
    w = world_of(key)
    return [NetworkSpec(n, es, kind, w["variants"][variant]["tables"].get(n)) for n, es, kind in w["nets"]]


def host_of(key, variant="general"):
    if (key, variant) not in _HOSTS:
        w = world_of(key)
        es = {name: {"agent": s["agent"], "venue": s["venue"], "people": w["variants"][variant]["people"][name]}
              for name, s in w["sets"].items()}
        _HOSTS[key, variant] = compile_plan(w["n_agents"], es, age=w["age"], sex=w["sex"], layout="csr",
                                            n_ext_agents=w["n_ext"])
    return _HOSTS[key, variant]


def engine_of(key, variant, device):
    if (key, variant) not in _ENGINES:
        _ENGINES[key, variant] = InfectionEngine(DevicePlan(host_of(key, variant), specs_of(key, variant), device))
    return _ENGINES[key, variant]


# ---- transmission vectors ------------------------------------------------------------------------------------------------
def general_vector(key, seed=0):
    """Most entries 0, the others in [2^-10, 1]: no product is then denormal."""
    w = world_of(key)
    rng = np.random.default_rng(2000 + seed)
    x = np.where(rng.random(w["n_ext"]) < 0.7, 0.0, rng.uniform(2.0 ** -10, 1.0, w["n_ext"])).astype(np.float32)
    x[[0, -1]] = 0.37, 0.81           # (the smallest world has six agents)
    return x


def dyadic_vector(key):
    w = world_of(key)
    rng = np.random.default_rng(2100)
    x = np.where(rng.random(w["n_ext"]) < 0.75, 0.0, rng.integers(1, 4, w["n_ext"]) * 2.0 ** -10).astype(np.float32)
    x[[0, -1]] = 3 * 2.0 ** -10
    return x


def block_lanes(host, sid):
    """lanes of the block that holds each venue of set `sid` (a long venue: 0)."""
    out = np.zeros(host.sets[sid].n_venues, dtype=np.int64)
    for b in host.blocks[(host.blocks[:, 0] == sid) & (host.blocks[:, 1] == 0)]:
        out[b[2]:b[3]] = b[7]
    return out


def probe_positions(d, G):
    """Row positions worth a probe in a venue of d edges whose block sums with G lanes (0: a long venue)."""
    pos = ([0, d - 1, 255, 256, 1023, 1024, LONG_CHUNK - 1, LONG_CHUNK] if G == 0
           else [0, d - 1, max(G, 4) - 1, max(G, 4), max(G, 4) + 1, 255, 256, 257])
    return [min(max(p, 0), d - 1) for p in pos]


def probe_vector(key, j):
    """One attendee per venue non-zero: venue v of every set at the (v + j)-th of its probe positions.  Where no other
    attendee of the venue was chosen by another venue, cum is a single product, whatever the order."""
    w, host = world_of(key), host_of(key)
    rng = np.random.default_rng(2200 + j)
    x = np.zeros(w["n_ext"], dtype=np.float32)
    for sid, s in enumerate(host.sets):
        lanes = block_lanes(host, sid)
        deg = np.diff(s.v_rowptr)
        for v in np.flatnonzero(deg):
            p = probe_positions(int(deg[v]), int(lanes[v]))[(v + j) % N_PROBES]
            x[s.v_agent[s.v_rowptr[v] + p]] = F32(rng.uniform(0.25, 1.0))
    return x


def special_vector(key):
    """The general vector with an inf and a NaN: (x, [(set, venue)] that must not be finite)."""
    host = host_of(key)
    x = general_vector(key, seed=7)
    first, last = host.sets[0], host.sets[-1]
    e_inf = first.n_edges // 2
    a_inf = int(first.v_agent[e_inf])
    others = np.flatnonzero(last.v_agent != a_inf)                               # (another agent's edges)
    e_nan = int(others[len(others) // 3])
    a_nan = int(last.v_agent[e_nan])
    x[a_inf], x[a_nan] = np.inf, np.nan
    at = [(first.name, int(np.searchsorted(first.v_rowptr, e_inf, side="right") - 1)),
          (last.name, int(np.searchsorted(last.v_rowptr, e_nan, side="right") - 1))]
    return x, at


def vectors_of(key):
    """[(name, variant, x)]"""
    out = [("dyadic", "dyadic", dyadic_vector(key)), ("general", "general", general_vector(key))]
    out += [(f"probe-{j}", "general", probe_vector(key, j)) for j in range(N_PROBES)]
    out.append(("inf-nan", "general", special_vector(key)[0]))
    return out


# ---- the restatement, the drive, the comparison -----------------------------------------------------------------------------
def launch_of(key, variant, launch):
    """(groups, tables) of a launch as the restatement takes them."""
    w, host = world_of(key), host_of(key, variant)
    specs = specs_of(key, variant)
    nets = RC.launch_nets(specs, launch["active"], w["variants"][variant]["betas"], host.set_index)
    return RC.groups_of(nets, RC.strides_of(specs, host.set_index)), RC.tables_of(specs)


def restated(key, variant, li, x, cache=None, susc=None):
    """({set: cum [V, nk]}, trans_susc [A]) of launch `li` of the world on the transmissions x."""
    if cache is not None and (key, variant, li, cache) in _WANT:
        return _WANT[key, variant, li, cache]
    w, host = world_of(key), host_of(key, variant)
    launch = w["launches"][li]
    groups, tables = launch_of(key, variant, launch)
    kw = dict(has_q=launch["has_q"], q_thr=Q_THR, day_type=launch["day_type"])
    cums = RC.restate_cum(host, groups, tables, x, stage_ext=w["stage_ext"], **kw)
    ts = RC.ts_of_agents(host, groups, tables, cums, susc=w["variants"][variant]["susc"] if susc is None else susc,
                         stage=w["stage_ext"], **kw)
    if cache is not None:
        _WANT[key, variant, li, cache] = (cums, ts)
    return cums, ts


def params_of(engine, w, variant, launch):
    return engine.params(now=1.0, delta_time=1.0, day_type=launch["day_type"], active=launch["active"],
                         betas=w["variants"][variant]["betas"], has_quarantine=launch["has_q"],
                         q_threshold=Q_THR if launch["has_q"] else math.inf)


def buffers_of(engine, w, variant, x, device, **more):
    A = w["n_agents"]
    susc = torch.from_numpy(w["variants"][variant]["susc"].copy()).to(device)
    stage = torch.from_numpy(w["stage_ext"][:A].copy()).to(device)
    xs = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
    return AgentBuffers(engine.plan, susceptibility=susc, transmission=xs, current_stage=stage, **more)


def write_halo_q(engine, w, x, launch, device):
    """q * x of the halo agents comes from the ranks that own them: written here, as the restatement takes it."""
    if launch["has_q"] and w["n_ext"] > w["n_agents"]:
        halo = slice(w["n_agents"], w["n_ext"])
        engine.q_transmission_buffer()[halo] = torch.from_numpy(RC.source(x, w["stage_ext"], Q_THR, True, False)[halo]).to(device)


def read_cums(engine, w):
    return {name: engine.plan.cum_of(name).cpu().numpy().copy() for name in w["sets"]}


def drive(key, variant, li, x, device, entry="phases"):
    """({set: cum [V, stride]}, trans_susc [A]); entry "phases": step_phase 1 and 4, "standalone": gj_venue_reduce and
    gj_agent_gather."""
    w = world_of(key)
    launch = w["launches"][li]
    engine = engine_of(key, variant, device)
    for c in engine.plan.cum:
        c.fill_(float(SENTINEL))
    p = params_of(engine, w, variant, launch)
    bufs = buffers_of(engine, w, variant, x, device)
    ts = torch.full((w["n_agents"],), float("nan"), device=device)
    probs = torch.full((w["n_agents"],), float("nan"), device=device)
    io = engine.io(trans_susc=ts, not_infected_probs=probs)
    write_halo_q(engine, w, x, launch, device)
    engine.quarantine_transmission(bufs, p)
    if entry == "phases":
        engine.step_phase(bufs, p, io, 1)
    else:
        engine.venue_reduce(bufs, p)
    torch.cuda.synchronize()
    cums = read_cums(engine, w)
    if entry == "phases":
        engine.step_phase(bufs, p, io, 4)
    else:
        engine.agent_gather(bufs, p, io, sample=False)
    torch.cuda.synchronize()
    return cums, ts.cpu().numpy()


def assert_same_bits(got, want, what, unit):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    same = (nan_g & nan_w) | (~nan_g & ~nan_w & (got.view(np.uint32) == want.view(np.uint32)))
    if not same.all():
        i = np.unravel_index(int(np.argmax(~same)), same.shape)
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} differ; first at {unit} {tuple(int(t) for t in i)}: "
                             f"got {got[i]!r} ({got.view(np.uint32)[i]:#010x}), want {want[i]!r} ({want.view(np.uint32)[i]:#010x})")


def compare(key, got_cums, got_ts, want_cums, want_ts, what):
    """Every venue of every active network and every owned agent as uint32; what is not written keeps the sentinel."""
    for name, cum in got_cums.items():
        nk = want_cums[name].shape[1] if name in want_cums else 0
        if nk:
            assert_same_bits(cum[:, :nk], want_cums[name], f"{what}: cum of set {name}", "(venue, network)")
        assert (cum[:, nk:].view(np.uint32) == SENTINEL.view(np.uint32)).all(), f"{what}: set {name} behind its {nk} networks"
    assert_same_bits(got_ts, want_ts, f"{what}: trans_susc", "agent")


# ---- the forms -----------------------------------------------------------------------------------------------------------
def forms_reached():
    """Each path of the kernels exists in the worlds, on the plans' own fields."""
    hosts = {k: host_of(k) for k in EVERY}
    blocks = np.concatenate([h.blocks for h in hosts.values()])
    stream = blocks[blocks[:, 1] == 0]
    edges, rows = stream[:, 5] - stream[:, 4], stream[:, 3] - stream[:, 2]
    assert set(stream[:, 7].tolist()) == {1, 4, 16, 64}
    assert (edges == N.GJ_STREAM_EDGES).any() and ((edges == N.GJ_STREAM_EDGES) & (rows > 1)).any()        # a full block
    full_rows = stream[rows == MAX_ROWS_PER_BLOCK]
    assert len(full_rows) and (full_rows[:, 7] == 1).all() and MAX_ROWS_PER_BLOCK // 256 == 8             # 8 trips of the row loop
    assert (edges == 1).any()
    lanes = hosts["lanes"]
    for sid, (name, G) in enumerate((("s1", 1), ("s4", 4), ("s16", 16), ("s64", 64))):
        b = lanes.blocks[(lanes.blocks[:, 0] == sid) & (lanes.blocks[:, 1] == 0)]
        assert lanes.sets[sid].name == name and (b[:, 7] == G).sum() >= 1, (name, b[:, 7])
    s1, s64 = lanes.sets[0], lanes.sets[3]
    d1, d64 = np.diff(s1.v_rowptr), np.diff(s64.v_rowptr)
    b1 = lanes.blocks[(lanes.blocks[:, 0] == 0) & (lanes.blocks[:, 1] == 0)]
    b64 = lanes.blocks[(lanes.blocks[:, 0] == 3) & (lanes.blocks[:, 1] == 0)]
    assert any(b[7] == 1 and d1[b[2]:b[3]].max() == 1500 and (d1[b[2]:b[3]] == 1).sum() == 300 for b in b1)
    assert any(b[7] == 64 and (d64[b[2]:b[3]] == 1).any() and (d64[b[2]:b[3]] == 0).any() for b in b64)
    assert any(b[5] - b[4] == 1 for b in b1)                                                             # a block of one edge
    long_v = lanes.long_rows[lanes.long_rows[:, 0] == 0][:, 1]
    assert d1[0] == 0 and d1[-1] == 0 and len(long_v) == 2 and d1[long_v[0] + 1] == 0                    # nobody's venues
    for name in ("s1", "s4", "s16", "s64"):
        s = lanes.sets[lanes.set_index[name]]
        people = world_of("lanes")["variants"]["general"]["people"][name]
        att = np.diff(s.v_rowptr) > 0
        assert {0, 1, 2} <= set(people[att].tolist()) and set(s.v_pcontact[att & (people <= 2)].tolist()) == {0.0, 1.0}
        pairs = s.v_agent.astype(np.int64) * s.n_venues + np.repeat(np.arange(s.n_venues), np.diff(s.v_rowptr))
        assert len(np.unique(pairs)) < len(pairs)                                                          # duplicated pairs
    # long rows of 1, 2 and 4 slots; chunk lengths on either side of the 4 x 256 unroll; a chunk of one edge
    lg = hosts["long"]
    for sid in (0, 1):
        slots = lg.long_rows[lg.long_rows[:, 0] == sid]
        assert {1, 2, 4} <= set((slots[:, 3] - slots[:, 2]).tolist())
    plain = lg.blocks[(lg.blocks[:, 0] == 0) & (lg.blocks[:, 1] == 1)]
    chunk = plain[:, 5] - plain[:, 4]
    assert {1, 1023, 1024, 1025, 2049, LONG_CHUNK} <= set(chunk.tolist()) and (chunk < 1024).any() and (chunk > 1024).any()
    db = np.diff(lg.sets[0].v_rowptr)
    assert db.tolist() == BIG and db[0] > N.GJ_STREAM_EDGES and db[-1] > N.GJ_STREAM_EDGES and (db[3:5] > N.GJ_STREAM_EDGES).all()
    alone = lg.blocks[(lg.blocks[:, 0] == 0) & (lg.blocks[:, 1] == 0) & (lg.blocks[:, 5] - lg.blocks[:, 4] == 2048)]
    assert len(alone) == 1 and alone[0, 3] - alone[0, 2] == 1 and alone[0, 7] == 64                        # 2 048 edges: STREAM
    assert world_of("long")["nets"][0][2] == N.MASK_Q and world_of("long")["nets"][1][2] == N.MASK_QL
    # the leisure set of 8 networks: STREAM and LONG blocks; the plain set of two with a long venue
    nw, wn = hosts["nets"], world_of("nets")
    lei, dual = nw.set_index["leisure"], nw.set_index["dual"]
    assert sum(es == "leisure" for _, es, _ in wn["nets"]) == N.GJ_MAX_NETS_PER_SET == 8
    assert sum(n in LEISURE8 for n in wn["launches"][0]["active"]) == 8
    for sid in (lei, dual):
        kinds = set(nw.blocks[nw.blocks[:, 0] == sid][:, 1].tolist())
        assert kinds == {0, 1}, (sid, kinds)
    groups = {li: launch_of("nets", "general", launch)[0] for li, launch in enumerate(wn["launches"])}
    by_set = lambda li: {g.set: g for g in groups[li]}
    assert by_set(0)[lei].nk == 8 and by_set(1)[lei].nk == 2 and by_set(2)[lei].nk == 1 and by_set(3)[lei].nk == 1
    assert by_set(2)[lei].mask == [N.MASK_QL] and by_set(3)[lei].mask == [N.MASK_QL_AGE75]
    assert by_set(0)[dual].nk == 2 and not by_set(0)[dual].leisure and by_set(3)[dual].nk == 1
    assert all(nw.set_index["company"] not in by_set(li) for li in groups)                               # never active
    assert by_set(0)[nw.set_index["household"]].raw and not by_set(0)[nw.set_index["school"]].raw
    assert {launch["has_q"] for launch in wn["launches"]} == {True, False}
    assert {launch["day_type"] for launch in wn["launches"]} == {0, 1}
    assert {75, 76} <= set(wn["age"].tolist()) and 100 < (wn["stage_ext"] < Q_THR).sum() < wn["n_agents"] - 100
    assert all((t == 0).any() for t in wn["variants"]["general"]["tables"].values())
    # agents
    for A in AGENT_COUNTS:
        h, w = hosts[f"agents-{A}"], world_of(f"agents-{A}")
        assert h.n_agents == A and h.n_ext_agents > A
        degs = np.stack([np.diff(s.a_rowptr) for s in h.sets])
        assert degs.shape == (3, A) and degs[:, 0].sum() >= 300
        for s in h.sets:
            assert (s.v_agent >= A).any() and np.diff(s.v_rowptr)[-2:].sum() == 0        # halo attendees; nobody's venues
        if A > 1:
            assert ((degs == 0).any(axis=0) & (degs.sum(axis=0) > 0)).any() and (degs.sum(axis=0) == 0).any()
            assert {0.0, F32(0.4), 1.0} <= set(w["variants"]["general"]["susc"].tolist())


def test_every_form_is_reached(device):
    forms_reached()


# ---- 1. every world, every vector, every launch ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", EVERY)
def test_cum_and_trans_susc_bit_for_bit(device, key):
    w = world_of(key)
    for name, variant, x in vectors_of(key):
        for li in range(len(w["launches"])):
            want_cums, want_ts = restated(key, variant, li, x, cache=name)
            got_cums, got_ts = drive(key, variant, li, x, device)
            compare(key, got_cums, got_ts, want_cums, want_ts, f"{key} / {name} / launch {li} {w['launches'][li]}")
            if name == "general" and w["n_agents"] > 1:          # (not vacuous; the world of one agent has a few edges)
                assert all(np.isfinite(c).all() and c.max() > 0 for c in want_cums.values()) and want_ts.max() > 0
            if name == "inf-nan":
                for set_name, v in special_vector(key)[1]:
                    if set_name in want_cums:
                        assert not np.isfinite(want_cums[set_name][v]).any() and not np.isfinite(got_cums[set_name][v, 0])


@pytest.mark.parametrize("key", EVERY)
def test_dyadic_inputs_equal_the_float64_sums(device, key):
    """On the dyadic variant every product and every partial sum is exact (tests/test_csr_ref.py): the DEVICE's cum and
    trans_susc equal the float64 sums, whatever the order - this pins which edges and which factors enter."""
    w = world_of(key)
    host = host_of(key, "dyadic")
    x = dyadic_vector(key)
    for li, launch in enumerate(w["launches"]):
        got_cums, got_ts = drive(key, "dyadic", li, x, device)
        groups, tables = launch_of(key, "dyadic", launch)
        kw = dict(has_q=launch["has_q"], q_thr=Q_THR, day_type=launch["day_type"])
        exact = RC.cum_float64(host, groups, tables, x, stage_ext=w["stage_ext"], **kw)
        for name, (s, _, _) in exact.items():
            assert np.array_equal(got_cums[name][:, :s.shape[1]].astype(np.float64), s), (key, li, name)
        ts64, _, _ = RC.ts_float64(host, groups, tables, got_cums, susc=w["variants"]["dyadic"]["susc"], stage=w["stage_ext"], **kw)
        assert np.array_equal(got_ts.astype(np.float64), ts64), (key, li)


# ---- 2. the other entry points ---------------------------------------------------------------------------------------------
def test_standalone_entry_points(device):
    """gj_venue_reduce and gj_agent_gather on the nets world: the same two comparisons."""
    key = "nets"
    w = world_of(key)
    x = general_vector(key)
    for li in range(len(w["launches"])):
        want_cums, want_ts = restated(key, "general", li, x, cache="general")
        got_cums, got_ts = drive(key, "general", li, x, device, entry="standalone")
        compare(key, got_cums, got_ts, want_cums, want_ts, f"{key} / stand-alone / launch {li}")


def test_fused_step(device):
    """gj_step on the nets world, sampling on with injected noise: the transmissions are the step's own (read back after
    it: nothing behind k_transmission writes them), cum and trans_susc are compared with the restatement on the
    susceptibility from BEFORE the step, which the state update then changes."""
    key, variant = "nets", "general"
    w = world_of(key)
    A = w["n_agents"]
    rng = np.random.default_rng(2300)
    engine = engine_of(key, variant, device)
    for li, launch in enumerate(w["launches"]):
        for c in engine.plan.cum:
            c.fill_(float(SENTINEL))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        infected = (rng.random(A) < 0.3).astype(np.float32)
        state = dict(max_infectiousness=dev(rng.uniform(0.1, 1.0, A)), shape=dev(rng.uniform(1.0, 3.0, A)),
                     rate=dev(rng.uniform(0.5, 2.0, A)), shift=dev(rng.uniform(0.0, 0.4, A)),
                     infection_time=dev(5.0 - rng.uniform(0.5, 4.0, A)), is_infected=dev(infected))
        bufs = buffers_of(engine, w, variant, np.zeros(A, np.float32), device, **state)
        susc_before = bufs.tensors["susceptibility"].cpu().numpy().copy()
        p = engine.params(now=5.0, delta_time=1.0, day_type=launch["day_type"], active=launch["active"],
                          betas=w["variants"][variant]["betas"], has_quarantine=launch["has_q"],
                          q_threshold=Q_THR if launch["has_q"] else math.inf)
        ts, new = torch.full((A,), float("nan"), device=device), torch.full((A,), float("nan"), device=device)
        noise = dev(rng.exponential(1.0, 2 * A))
        engine.step(bufs, p, engine.io(trans_susc=ts, new_infected=new, exp_noise=noise))
        torch.cuda.synchronize()
        x = bufs.tensors["transmission"].cpu().numpy()
        assert np.isfinite(x).all() and (x > 0).sum() > 100 and np.array_equal(x != 0, infected != 0)
        want_cums, want_ts = restated(key, variant, li, x, susc=susc_before)
        compare(key, read_cums(engine, w), ts.cpu().numpy(), want_cums, want_ts, f"{key} / gj_step / launch {li}")
        changed = bufs.tensors["susceptibility"].cpu().numpy() != susc_before
        assert changed.any() and not (changed & (new.cpu().numpy() == 0)).any()
