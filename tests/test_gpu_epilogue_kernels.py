"""GPU: the end of the step - a7 not_infected_prob, a8 gumbel_new_infected / own_new_infected, a9 infect - per agent,
INSIDE the step, in each of its four implementations: the stand-alone k_sample_infect, the tail of k_agent_gather (CSR),
k_tile_epilogue (the tiled step's split form) and agents_ts_to_lds / agents_epilogue / agents_tail of k_tile_agents (the
fused form, which bench.py times).  test_gpu_pass2_kernels.py stops in front of the decision (step_phase 4); this file
drives step_phase 6, then step_phase 3, with the full state, on a cum of its choosing.

References: pass 2 (trans_susc) is tests/gj_pass2_ref.py bit for bit; p is held to K x the bound of
gj_sampler_ref.prob_reference (derived from the number formats; K = 2 K_REF = 1: the bound itself); the decision is the
fp64 decision of gj_sampler_ref.forward_decision on the p THE DEVICE WROTE wherever rounding cannot flip it, torch's
value (oracle.sample_infected) where p or a draw rules, and in every point what gj_sample_infect returns for the same
(p, draws): four kernels, one rule; the state is gj_sampler_ref.infect_unfused bit for bit.  With the library's own
draws the decision is p < theta with theta from tests/gj_philox_ref.py, exactly.

Worlds (test_gpu_pass2_kernels.py's, and one more):
  W-own    the 1 003 agents of W-small, each with ONE household edge to a venue of its own (V = A); only `household` is
           active, so cum[a] sets agent a's ts up to pass 2's fixed-point grid.  It carries gj_sampler_ref.step_points.
  W-small, W-run, W-quads with cums spread so that ts * dt spans the sampler's core range.

Measured on an MI355X (K = 1.0), max err / bound of p per form:
  W-own, the 10 030 agents of its ten launches (step_points at dt = 0.25, 1, 2; the edges at dt = 0.01): 0.453 in each of
  fused-ws, fused-direct, split-ws, split-direct, split-run, run, fused-ws-unaligned and csr (ts = 100 at dt = 1, the
  subnormal p: the fp32 restatement's own worst point and value, tests/test_sampler_ref.py);
  random cums at dt = 0.3: fused-ws, fused-direct, split-ws, split-direct, fused-ws-unaligned 0.675; split-run, run 0.638;
  csr 0.655 (its ts is another sum); second-quad and second-quad-unaligned 0.707, five-quads 0.807 (43 847 agents each).
Unsafe points: 0 of the 10 030 per form on W-own (tests/test_sampler_ref.py: 0.27 % of the step points once p is 2 ulp
off), 0 of 1 003 and of 43 847 on the random worlds; so none decided otherwise than fp64.  The cap is 1 %.
"""
import functools

import numpy as np
import pytest
import torch

import gj_oracle as O
import gj_pass2_ref as R2
import gj_philox_ref as PH
import gj_sampler_ref as R
import test_gpu_pass2_kernels as P2
from grad_june_amd import _native as N
from grad_june_amd.engine import AgentBuffers, InfectionEngine, StepClock
from grad_june_amd.plan import DevicePlan, compile_plan
from test_gpu_sampler_kernels import bits, dev, same_bits, same_bits_nan_as_class

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = -77.0
NOW = R.UPDATE_NOW                                # a full mantissa
SEED, STEP = 0x1234_5678_9ABC, (1 << 32) + 41     # a step above 2^32
OFFSETS = (0, 1, 2, 3, (1 << 33) + 7)             # every value of mis = (agent_offset + base) & 3, and an offset above 2^32
RANDOM_DT = 0.3                                   # (not a float32 number: ts * dt rounds)
HOUSEHOLD = ["household"]
EVERYONE, NOBODY = (1e30, 1e-30), (1e-30, 1e30)   # draw pairs that decide a p in (0, 1) whatever it is


# ---- W-own and the layouts ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def own_world():
    w = P2.world_of("small")
    one = np.arange(w["n_agents"], dtype=np.int64)
    household = {"agent": one, "venue": one.copy(), "people": np.full(len(one), 2, dtype=np.int64)}
    return dict(w, edge_sets=dict(w["edge_sets"], household=household))


def world_for(wkey):
    return own_world() if wkey == "own" else P2.world_of(wkey)


# (form, layout of test_gpu_pass2_kernels.py, float offset of every io and state array inside its buffer); W-own takes
# the layouts of W-small / W-run: the same plan arguments on its edge sets
TILED_FORMS = {"fused-ws": ("ws-narrow", 0), "fused-direct": ("direct", 0), "split-ws": ("ws-split-no-lv8", 0),
               "split-direct": ("direct-split", 0), "split-run": ("run-ws", 0), "run": ("run", 0),
               "fused-ws-unaligned": ("ws-narrow", 1)}
QUAD_FORMS = {"second-quad": ("quads-ws-4160", 0), "five-quads": ("quads-direct-19840", 0),
              "second-quad-unaligned": ("quads-ws-4160", 1)}
OWN_FORMS = list(TILED_FORMS) + ["csr"]
STEP_FORMS = list(TILED_FORMS) + list(QUAD_FORMS) + ["csr"]

_OWN_HOSTS, _ENGINES = {}, {}


def form_of(form, own):
    """(world key, layout or None for the CSR plan, offset)"""
    if form == "csr":
        return ("own" if own else "small"), None, 0
    layout, offset = {**TILED_FORMS, **QUAD_FORMS}[form]
    return ("own" if own else P2.LAYOUTS[layout][0]), layout, offset


def host_for(wkey, layout):
    if wkey != "own":
        return P2.host_of(layout)
    if layout not in _OWN_HOSTS:
        w = own_world()
        _, sa, kw, _ = P2.LAYOUTS[layout]
        _OWN_HOSTS[layout] = compile_plan(w["n_agents"], w["edge_sets"], age=w["age"], sex=w["sex"], layout="tiled",
                                          nets_per_set={"leisure": 3}, slices=(-(-w["n_agents"] // sa), sa), **kw)
    return _OWN_HOSTS[layout]


def engine_for(wkey, layout, device):
    if layout is not None and wkey != "own":
        return P2.engine_of(layout, device)
    if (wkey, layout) not in _ENGINES:
        w = world_for(wkey)
        if layout is None:
            host = compile_plan(w["n_agents"], w["edge_sets"], age=w["age"], sex=w["sex"], layout="csr")
            _ENGINES[wkey, layout] = InfectionEngine(DevicePlan(host, w["specs"], device))
        else:
            plan = DevicePlan(host_for(wkey, layout), w["specs"], device, **P2.LAYOUTS[layout][3])
            _ENGINES[wkey, layout] = InfectionEngine(plan)
    return _ENGINES[wkey, layout]


def test_every_form_is_reached(device):
    """On the plans' own fields: W-own's household set in the workspace, direct and run forms, fused and split; slices of
    64 with a tail of 43 agents and n % 4 = 3; W-quads with a lane's second quad (4 160) and with all five quads and a
    partial last slice (19 840); the CSR plans hold no tiled arrays; the unaligned forms are one float off 16 bytes."""
    own = own_world()
    hh = own["edge_sets"]["household"]
    assert own["n_agents"] == 1003 and np.array_equal(hh["agent"], np.arange(1003)) and np.array_equal(hh["venue"], hh["agent"])
    want = {"fused-ws": ("workspace", False), "fused-direct": ("direct", False), "split-ws": ("workspace", True),
            "split-direct": ("direct", True), "split-run": ("run", True), "run": ("run", False),
            "fused-ws-unaligned": ("workspace", False)}
    for form, (hh_form, split) in want.items():
        for is_own in (True, False):
            wkey, layout, offset = form_of(form, is_own)
            host = host_for(wkey, layout)
            assert R2.forms_of_plan(host)["household"]["form"] == hh_form, (form, is_own)
            assert (host.n_slices, host.slice_agents, 1003 - 15 * 64, 1003 % 4) == (16, 64, 43, 3)
            e = engine_for(wkey, layout, device)
            assert (e.plan.agent_scratch is not None) == split, (form, is_own)
            assert offset == (1 if "unaligned" in form else 0)
    assert R2.forms_of_plan(P2.host_of("run-ws"))["school"]["form"] == "workspace"
    assert R2.forms_of_plan(P2.host_of("run"))["school"]["form"] == "direct"
    assert P2.host_of("quads-ws-4160").slice_agents // 4 - 1024 == 16                    # 16 lanes hold a second quad
    h = P2.host_of("quads-direct-19840")
    assert (h.slice_agents, h.n_slices, 43847 - 2 * 19840) == (19840, 3, 4167) and 19840 // 4 > 4 * 1024      # m_run reaches 4
    assert any(f["form"] == "direct" for f in R2.forms_of_plan(h).values())
    for wkey in ("own", "small"):
        e = engine_for(wkey, None, device)
        assert e.plan.host.layout == "csr" and e.plan.host.slice_agents == 0
    b = P2.offset_buffer(8, device, 1)
    assert b.data_ptr() % 16 == 4


# ---- the drive -----------------------------------------------------------------------------------------------------------------
def pre_state(A):
    """gj_sampler_ref.forward_state, with a NaN that carries a payload, -0.0 and a subnormal number planted in is_infected
    and infection_time of every 17th agent"""
    st = R.forward_state(A)
    odd = np.array([0x7FC01234, 0x80000000, 0x00000001], dtype=np.uint32).view(F32)
    inf, time = st["inf"].copy(), st["time"].copy()
    at = np.arange(3, A, 17)
    inf[at] = odd[np.arange(len(at)) % 3]
    time[at] = odd[(np.arange(len(at)) + 1) % 3]
    return {"susc": st["susc"], "inf": inf, "time": time, "now": NOW}


def sample_alone(device, p, noise, seed=0, step=0, agent_offset=0):
    """gj_sample_infect on (p, noise) without a state: new_infected"""
    pd = dev(p, device)
    nd = None if noise is None else dev(np.concatenate(noise).astype(F32), device)
    out = torch.full((len(p),), SENTINEL, device=device)
    N.check(N.load().gj_sample_infect(len(p), N.ptr(pd), N.ptr(nd), seed, step, agent_offset, NOW, N.ptr(out), None, None, None,
                                      N.current_stream()), "gj_sample_infect")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def drive(engine, w, device, *, cums, st, dt, active, noise=None, offset=0, phase=3, drop=(), seed=0, step=0,
          agent_offset=0, now=NOW, clock=None):
    """The chosen cum in place, step_phase 6 (phase C), then step_phase `phase` (3: the whole of phase D; 4: without the
    decision) with the full state and every output but those in ``drop``; a CSR plan: agent_gather.  Returns the outputs
    and the post-state on the CPU."""
    A = w["n_agents"]
    P2.write_cums(engine, cums)
    p = engine.params(now=now, delta_time=dt, day_type=0, active=active, betas=P2.BETAS, seed=seed, step=step,
                      agent_offset=agent_offset)
    p.transpose = 0
    if clock is not None:
        p.clock = clock.ptr

    def buf(v, n=A, fill=float("nan")):
        t = P2.offset_buffer(n, device, offset, fill)
        if v is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=F32)))
        assert t.data_ptr() % 16 == 4 * offset
        return t

    state = {k: buf(st[k]) for k in ("susc", "inf", "time")}
    bufs = AgentBuffers(engine.plan, susceptibility=state["susc"], is_infected=state["inf"], infection_time=state["time"],
                        transmission=torch.zeros(engine.plan.host.n_ext_agents, device=device),
                        current_stage=torch.from_numpy(w["stage"]).to(device))
    out = {k: buf(None, fill=SENTINEL) for k in ("probs", "new", "ts") if k not in drop}
    nz = None if noise is None else buf(np.concatenate(noise), n=2 * A)
    io = engine.io(not_infected_probs=out.get("probs"), new_infected=out.get("new"), trans_susc=out.get("ts"), exp_noise=nz)
    if engine.plan.host.layout == "csr":
        engine.agent_gather(bufs, p, io, sample=phase == 3)
    else:
        engine.step_phase(bufs, p, io, 6)
        engine.step_phase(bufs, p, io, phase)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in {**out, **state}.items()}
    return got


def assert_state(got, st, new, what):
    """3.  infect_unfused(pre-state, new_infected) bit for bit, NaN as a class; nu == 0 keeps every bit; a NaN decision
    makes all three NaN"""
    want = R.infect_unfused(st, new)
    kept = new == 0
    assert kept.any()
    for k, wv in zip(("susc", "inf", "time"), want):
        assert same_bits(got[k][kept], st[k][kept]), (what, k, "nu == 0 changed bits")
        assert same_bits_nan_as_class(got[k][~kept], wv[~kept]), (what, k, int(np.argmax(bits(got[k]) != bits(wv))))
    nan = np.isnan(new)
    assert all(np.isnan(got[k][nan]).all() for k in ("susc", "inf", "time")), what


STATS = {}


def check_injected(device, got, probs4, st, noise, dt, what, form):
    """1. (p), 2. and 3. of one launch with injected draws; returns the launch's figures"""
    e0, e1 = noise
    ts, p, new = got["ts"], got["probs"], got["new"]
    assert same_bits_nan_as_class(p, probs4), (what, "p differs from step_phase 4's")
    p64, bound = R.prob_reference(ts, dt)
    q, ok = R.excess(p, p64, bound)
    assert ok.all(), (what, [(int(i), float(ts[i]), float(p[i]), float(p64[i])) for i in np.nonzero(~ok)[0][:8]])
    assert np.array_equal(np.isnan(p), np.isnan(ts)), what
    v, i = R.worst(q)
    assert v <= R.K, (what, i, float(ts[i]), float(p[i]), float(p64[i]))
    share, unsafe, safe, ruled, nu64 = R.unsafe_share(p, e0, e1)
    assert share <= R.MAX_UNSAFE_SHARE, (what, share)
    assert same_bits(new[safe], nu64[safe].astype(F32)), (what, np.nonzero(safe & (new != nu64))[0][:8].tolist())
    assert np.isin(new[unsafe], (0.0, 1.0)).all(), what
    oracle = O.sample_infected(torch.from_numpy(p), torch.from_numpy(np.stack([e0, e1]))).numpy()
    assert same_bits_nan_as_class(new[ruled], oracle[ruled]), what
    alone = sample_alone(device, p, noise)
    assert same_bits_nan_as_class(new, alone), (what, "not gj_sample_infect's", np.nonzero(bits(new) != bits(alone))[0][:8].tolist())
    assert_state(got, st, new, what)
    s = STATS.setdefault(form, {"worst": 0.0, "points": 0, "unsafe": 0, "otherwise": 0})
    s["worst"] = max(s["worst"], v)
    s["points"] += len(p)
    s["unsafe"] += int(unsafe.sum())
    s["otherwise"] += int((new[unsafe] != nu64[unsafe]).sum())
    return dict(ruled=ruled, safe=safe, unsafe=unsafe, nu64=nu64, worst=(v, i))


def report(form):
    s = STATS[form]
    print(f"{form}: {s['points']} points, max err / bound of p {s['worst']:.3f}, unsafe {s['unsafe']}, "
          f"of which decided otherwise than fp64: {s['otherwise']}")


# ---- W-own: the step points ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def own_rounds(dt):
    """The launches that carry step_points(dt) on W-own: the agents with a non-zero susceptibility take the points in
    order, a launch's other agents a ts in the core and random draws.  Per launch (cum [A, 1], e0, e1, kinds)."""
    A = 1003
    st = pre_state(A)
    sp = R.step_points(dt, grid=dt in R.STEP_DTS)
    carriers = np.flatnonzero(st["susc"] != 0)
    g = np.random.default_rng(int(1000 * dt) + 7)
    rounds = []
    for lo in range(0, sp["n"], len(carriers)):
        n = min(len(carriers), sp["n"] - lo)
        ts = (g.uniform(0.01, 5.0, A) / dt).astype(F32)
        e0, e1 = g.exponential(size=A).astype(F32), g.exponential(size=A).astype(F32)
        kinds = ["filler"] * A
        at = carriers[:n]
        ts[at], e0[at], e1[at] = sp["ts"][lo:lo + n], sp["e0"][lo:lo + n], sp["e1"][lo:lo + n]
        for a, k in zip(at, sp["kinds"][lo:lo + n]):
            kinds[a] = k
        cum = np.array([R.acc_for(t, s) if s != 0 else t for t, s in zip(ts, st["susc"])], dtype=F32).reshape(A, 1)
        rounds.append((cum, e0, e1, kinds))
    return rounds


def own_restated(layout, cum, susc):
    """(groups, trans_susc bits) of W-own; the CSR step: the one product fl(cum * susc), added to 0"""
    w = own_world()
    if layout is None:
        with np.errstate(all="ignore"):
            ts = ((cum[:, 0] * susc).astype(F32) + F32(0.0)).astype(F32)
        return [], np.ascontiguousarray(ts).view(np.uint32)
    groups = R2.groups_of(w["edge_sets"], w["specs"], HOUSEHOLD, {"household": cum}, R2.forms_of_plan(host_for("own", layout)))
    _, ts = R2.restate(w["n_agents"], groups, age=w["age"], sex=w["sex"], day_type=0, transpose=0, susceptibility=susc,
                       direct_table_floats=P2.dtf_of(layout))
    return groups, ts


@pytest.mark.parametrize("form", OWN_FORMS)
def test_step_points_every_agent(device, form):
    """1. - 3. on W-own with gj_sampler_ref.step_points at dt = 0.25, 1, 2 and the edges at dt = 0.01: every form."""
    wkey, layout, offset = form_of(form, own=True)
    w = world_for(wkey)
    engine = engine_for(wkey, layout, device)
    st = pre_state(w["n_agents"])
    seen = set()
    for dt in R.STEP_DTS + R.EDGE_DTS[:1]:
        for r, (cum, e0, e1, kinds) in enumerate(own_rounds(dt)):
            what = f"{form} dt {dt} launch {r}"
            kw = dict(cums={"household": cum}, st=st, dt=dt, active=HOUSEHOLD, noise=(e0, e1), offset=offset)
            probs4 = drive(engine, w, device, phase=4, **kw)["probs"]
            got = drive(engine, w, device, **kw)
            groups, ts_bits = own_restated(layout, cum, st["susc"])
            P2.assert_bits(got["ts"], ts_bits, groups, what + " trans_susc")
            res = check_injected(device, got, probs4, st, (e0, e1), dt, what, form)
            # the named points are what they are named for, on the p the device wrote
            k = {name: np.array([x == name for x in kinds]) & (st["susc"] != 0) for name in set(kinds)}
            p, new = got["probs"], got["new"]
            for name in ("ts_nan", "draw0"):
                if name in k and k[name].any():
                    assert res["ruled"][k[name]].all() and np.isnan(new[k[name]]).all(), (what, name)
                    seen.add(name)
            if k.get("ts_nan") is not None and k["ts_nan"].any():
                assert np.isnan(p[k["ts_nan"]]).all()
            if "ts_hi" in k and k["ts_hi"].any():
                hi = p[k["ts_hi"]]
                if dt == 2.0:
                    assert (hi == 0).all() and (new[k["ts_hi"]] == 1).all()
                    seen.add("p_zero")
                if dt == 1.0:
                    assert ((hi > 0) & (hi < R.FLT_MIN)).all()
                    seen.add("p_subnormal")
            if "ts_lo" in k and k["ts_lo"].any() and dt == 0.01:
                assert (p[k["ts_lo"]] == 1).all() and (bits(new[k["ts_lo"]]) == 0).all()
                seen.add("p_one")
            if "ts_neg" in k and k["ts_neg"].any():
                neg = p[k["ts_neg"]]                                          # clamped to 1e-6: one value, just below 1
                assert (got["ts"][k["ts_neg"]] <= 0).all() and (bits(neg) == bits(neg)[0]).all() and 0.99 < neg[0] <= 1
                seen.add("ts_neg")
            if "ts_sat" in k and k["ts_sat"].any() and layout is not None and "ws" in form:
                assert (np.abs(got["ts"][k["ts_sat"]]) >= 1e29).all()          # the saturated sum, read back
                seen.add("saturated")
            if "draw_sub" in k and k["draw_sub"].any():
                assert np.isfinite(new[k["draw_sub"]]).all()
                seen.add("draw_sub")
    assert seen >= {"ts_nan", "draw0", "p_zero", "p_subnormal", "p_one", "ts_neg", "draw_sub"}, seen
    assert ("saturated" in seen) == (layout is not None and "ws" in form)
    report(form)


# ---- W-small, W-run, W-quads ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def core_cums(wkey):
    """cum log-uniform in [1e-3, 4] (a tenth exact zeros): with up to ~40 terms per agent ts * dt spans the core range;
    one household's cum is a NaN"""
    w = world_for(wkey)
    g = np.random.default_rng(77)
    out = {}
    for s in P2.SETS:
        shape = (len(w["edge_sets"][s]["people"]), P2.STRIDE[s])
        c = np.exp(g.uniform(np.log(1e-3), np.log(4.0), shape))
        c[g.random(shape) < 0.1] = 0.0
        out[s] = c.astype(F32)
    out["household"][w["edge_sets"]["household"]["venue"][0], 0] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def random_noise(A):
    """Exponential draws; a draw of 0 for every 97th agent (a NaN decision), a subnormal draw for every 101st"""
    g = np.random.default_rng(A)
    e0, e1 = g.exponential(size=A).astype(F32), g.exponential(size=A).astype(F32)
    e0[5::97] = 0.0
    e1[7::101] = 1e-40
    return e0, e1


def world_restated(wkey, layout, st):
    """(groups, trans_susc bits) of a world with every network active"""
    w = world_for(wkey)
    if layout is None:
        return None
    groups, _, ts = P2.restated(layout, w, core_cums(wkey), day_type=0, transpose=0, has_q=False, susc=st["susc"],
                                key="epilogue")
    return groups, ts


@pytest.mark.parametrize("form", STEP_FORMS)
def test_random_worlds_every_agent(device, form):
    """1. - 3. on W-small, W-run and W-quads, every network active: a lane's second quad, m_run up to 4 with a partial
    last slice, the guarded scalar accesses, and NaN decisions (a draw of 0, a NaN cum) in every quad position."""
    wkey, layout, offset = form_of(form, own=False)
    w = world_for(wkey)
    A = w["n_agents"]
    engine = engine_for(wkey, layout, device)
    st, noise, cums = pre_state(A), random_noise(A), core_cums(wkey)
    kw = dict(cums=cums, st=st, dt=RANDOM_DT, active=P2.ACTIVE, noise=noise, offset=offset)
    probs4 = drive(engine, w, device, phase=4, **kw)["probs"]
    got = drive(engine, w, device, **kw)
    restated = world_restated(wkey, layout, st)
    if restated is not None:
        P2.assert_bits(got["ts"], restated[1], restated[0], form + " trans_susc")
    res = check_injected(device, got, probs4, st, noise, RANDOM_DT, form, form + " (random)")
    x = got["ts"].astype(np.float64) * RANDOM_DT
    live = st["susc"] != 0
    assert ((x >= 0.01) & (x <= 5.0))[live].mean() > 0.5 and (x[live] > 5.0).any() and (x[live] < 0.01).any()
    new = got["new"]
    assert (new == 1).sum() > A // 20 and (new == 0).sum() > A // 20
    nan = np.isnan(new)
    assert nan.sum() >= A // 97 and np.isnan(got["probs"]).any()
    if layout is not None:                    # a NaN decision in every position j of a quad, and in a lane's later quads
        sa = P2.host_of(layout).slice_agents
        local = np.flatnonzero(nan) % sa
        assert set((local % 4).tolist()) == {0, 1, 2, 3}
        assert (local // 4096).max() == (sa - 1) // 4096                      # (quad m of a lane holds agents 4096 m ...)
    report(form + " (random)")


# ---- 4. masks and the deferred update ------------------------------------------------------------------------------------------
def flat_cums(wkey, value, own):
    w = world_for(wkey)
    sets = HOUSEHOLD if own else P2.SETS
    return {s: np.full((len(w["edge_sets"][s]["people"]), P2.STRIDE[s]), value, dtype=F32) for s in sets}


MASK_FORMS = [("fused-ws", True), ("fused-direct", True), ("fused-ws-unaligned", True), ("split-ws", True), ("csr", True),
              ("second-quad", False), ("five-quads", False), ("second-quad-unaligned", False)]


@pytest.mark.parametrize("form,own", MASK_FORMS, ids=[f for f, _ in MASK_FORMS])
def test_everyone_infected_and_exactly_one_per_slice(device, form, own):
    """Every agent infected - p == 0 at dt = 2 for every agent with an edge and a susceptibility, draws that infect the
    others - sets every bit of every lane's mask: up to 20 deferred updates per lane.  Then exactly one agent per slice,
    in its first quad, in its last quad, and the last agent (the tail quad of the last slice): everyone else keeps
    every bit."""
    wkey, layout, offset = form_of(form, own)
    w = world_for(wkey)
    A = w["n_agents"]
    engine = engine_for(wkey, layout, device)
    st = pre_state(A)
    active = HOUSEHOLD if own else P2.ACTIVE
    everyone = (np.full(A, EVERYONE[0], dtype=F32), np.full(A, EVERYONE[1], dtype=F32))
    got = drive(engine, w, device, cums=flat_cums(wkey, 1000.0, own), st=st, dt=2.0, active=active, noise=everyone,
                offset=offset)
    assert (bits(got["new"]) == bits(np.ones(A, F32))).all(), form
    if own:
        assert (got["probs"][st["susc"] != 0] == 0).all()
    else:
        assert (got["probs"] == 0).mean() > 0.5
    for k, wv in zip(("susc", "inf", "time"), R.infect_unfused(st, np.ones(A, F32))):
        assert same_bits_nan_as_class(got[k], wv), (form, k, int(np.argmax(bits(got[k]) != bits(wv))))
    sa = host_for(wkey, layout).slice_agents if layout is not None else 64
    starts = np.arange(0, A, sa)
    n_local = np.minimum(sa, A - starts)
    chosen_sets = {"first quad": starts + 1, "last quad": starts + 4 * ((n_local + 3) // 4 - 1), "last agent": starts + n_local - 1}
    assert chosen_sets["last agent"][-1] == A - 1 and (A - 1) % 4 != 3           # the tail quad: n_ok < 4
    for name, chosen in chosen_sets.items():
        mask = np.zeros(A, dtype=bool)
        mask[chosen] = True
        e0 = np.where(mask, F32(EVERYONE[0]), F32(NOBODY[0])).astype(F32)
        e1 = np.where(mask, F32(EVERYONE[1]), F32(NOBODY[1])).astype(F32)
        got = drive(engine, w, device, cums=flat_cums(wkey, 0.5, own), st=st, dt=2.0, active=active, noise=(e0, e1),
                    offset=offset)
        assert ((got["probs"] > 0) & (got["probs"] < 1)).all()
        assert same_bits(got["new"], mask.astype(F32)), (form, name, np.flatnonzero(got["new"] != mask)[:8].tolist())
        assert_state(got, st, got["new"], f"{form} one per slice, {name}")


# ---- 5. optional outputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fused-ws", "fused-direct", "fused-ws-unaligned", "split-ws", "run", "second-quad", "csr"])
def test_optional_outputs(device, form):
    """Each of new_infected, not_infected_probs, trans_susc NULL in turn: the same state bits and the same other
    outputs; step_phase 4 leaves the state and a sentinel-filled new_infected untouched."""
    wkey, layout, offset = form_of(form, own=False)
    w = world_for(wkey)
    A = w["n_agents"]
    engine = engine_for(wkey, layout, device)
    st, noise = pre_state(A), random_noise(A)
    kw = dict(cums=core_cums(wkey), st=st, dt=RANDOM_DT, active=P2.ACTIVE, noise=noise, offset=offset)
    full = drive(engine, w, device, **kw)
    assert (full["new"] == 1).sum() > A // 20 and np.isnan(full["new"]).any()
    for name in ("new", "probs", "ts"):
        part = drive(engine, w, device, drop=(name,), **kw)
        assert name not in part
        for k, v in part.items():
            assert same_bits_nan_as_class(v, full[k]), (form, "without " + name, k)
    only = drive(engine, w, device, phase=4, **kw)
    assert (only["new"] == SENTINEL).all()
    for k in ("susc", "inf", "time"):
        assert same_bits(only[k], st[k]), (form, k)
    for k in ("probs", "ts"):
        assert same_bits_nan_as_class(only[k], full[k]), (form, k)


# ---- 6. the library's own draws ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", STEP_FORMS)
def test_own_draws_every_agent(device, form):
    """exp_noise NULL: new_infected == (p < theta) on the p the device wrote, theta = gj_philox_ref.infection_uniform(seed,
    step, agent_offset + a) - exact, no tie tolerance - for every agent_offset mod 4 and one above 2^32, a step above
    2^32; the post-state follows 3.; a NaN p decides 0 (the one documented difference from the injected mode) in the
    step and in gj_sample_infect."""
    wkey, layout, offset = form_of(form, own=False)
    w = world_for(wkey)
    A = w["n_agents"]
    engine = engine_for(wkey, layout, device)
    st = pre_state(A)
    agents = np.arange(A, dtype=np.uint64)
    for agent_offset in OFFSETS:
        got = drive(engine, w, device, cums=core_cums(wkey), st=st, dt=RANDOM_DT, active=P2.ACTIVE, offset=offset, seed=SEED,
                    step=STEP, agent_offset=agent_offset)
        p, new = got["probs"], got["new"]
        theta = PH.infection_uniform(SEED, STEP, np.uint64(agent_offset) + agents)
        with np.errstate(invalid="ignore"):
            want = (p < theta).astype(F32)
        what = f"{form} agent_offset {agent_offset}"
        assert same_bits(new, want), (what, np.flatnonzero(new != want)[:8].tolist())
        nan = np.isnan(p)
        assert nan.any() and (bits(new[nan]) == 0).all(), what
        assert (new == 1).sum() > A // 20 and (new == 0).sum() > A // 20
        assert same_bits(sample_alone(device, p, None, SEED, STEP, agent_offset), new), what
        assert_state(got, st, new, what)
        if agent_offset == 0:          # another step, another offset: other decisions
            other = PH.infection_uniform(SEED, STEP & 0xFFFFFFFF, agents)
            assert ((p < other) != (p < theta)).sum() > A // 50
    restated = world_restated(wkey, layout, st)
    if restated is not None:
        P2.assert_bits(got["ts"], restated[1], restated[0], form + " trans_susc")


# ---- 7. the device clock -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fused-ws", "fused-direct", "split-ws", "split-direct", "second-quad", "csr"])
def test_device_clock(device, form):
    """params.clock set: decisions follow the clock's step and infection_time the clock's now, bit for bit, whatever the
    scalar fields say."""
    wkey, layout, offset = form_of(form, own=False)
    w = world_for(wkey)
    A = w["n_agents"]
    engine = engine_for(wkey, layout, device)
    st = pre_state(A)
    clock = StepClock(device)
    clock.set(NOW, STEP)
    got = drive(engine, w, device, cums=core_cums(wkey), st=st, dt=RANDOM_DT, active=P2.ACTIVE, seed=SEED, step=7, now=99.0,
                agent_offset=3, clock=clock)
    assert clock.read() == (float(F32(NOW)), STEP)
    p, new = got["probs"], got["new"]
    agents = np.uint64(3) + np.arange(A, dtype=np.uint64)
    with np.errstate(invalid="ignore"):
        want = (p < PH.infection_uniform(SEED, STEP, agents)).astype(F32)
        scalar = (p < PH.infection_uniform(SEED, 7, agents)).astype(F32)
    assert same_bits(new, want) and (want != scalar).sum() > A // 50
    assert_state(got, st, new, form)                                            # (pre_state's now is the clock's)
    wrong = R.infect_unfused(dict(st, now=99.0), new)[2]
    assert (bits(wrong) != bits(got["time"]))[(new == 1) & ~np.isnan(st["time"])].all()
