"""GPU: the venue launch reading the local venue of a slot from one byte (gj_aux.e_lv8) instead of two.

A set whose every venue block holds at most 255 venues gets `e_lv8`: the same integers as `e_lv` in a narrower field,
0xFF for the pad value.  Phase B (and phase C of a set that is not in the direct form) widens a group's eight bytes to
the sixteen it read before; everything behind that is unchanged, so `cum`, the per-slot values of phase C and a whole
step may not differ in a single bit between the two forms, and `cum` is held to the numpy restatement of the
arithmetic itself (tests/test_gpu_venue_multinet.py, module docstring)."""
import numpy as np
import pytest
import torch

import bench as B
from grad_june_amd import _native as N
from grad_june_amd.benchrun import SingleGpuHotPath
from grad_june_amd.engine import AgentBuffers, InfectionEngine
from grad_june_amd.plan import DevicePlan, NetworkSpec, _host, compile_plan, narrow_venue_ids
from grad_june_amd.synthetic import make_world
from test_gpu_venue_multinet import SATURATED, assert_same_bits, term_limit_bits

pytestmark = pytest.mark.gpu

A = 6000                     # 8 slices of 768 agents
EB_TARGET = 4096
NKS = [1, 2, 3, 8]
SETS = ["household", "school", "university", "leisure"]


# ---- the world -----------------------------------------------------------------------------------------------------------
def make_sets():
    """household  a // 3 for everybody (the run form takes these edges), a second household for every seventh agent (the
                  edges that stay in the tiled arrays);
    school        600 venues of 4 agents: the venue limit cuts the blocks - 255, 255 and 90 venues (256, 256, 88);
    university    one venue that holds everybody (a block of ONE venue: every wave's 512 slots are that venue), then
                  venues of 700 (blocks of five);
    leisure       one venue that holds everybody and venues of 2 - 20 consecutive agents: runs that end inside a lane's
                  eight slots, several networks per slot."""
    rng = np.random.default_rng(5)
    a = np.arange(A, dtype=np.int64)
    sets = {}
    second = a[::7]
    second = second[second // 3 + 11 < A // 3]       # (a later household: the agents stay ordered by their smallest one)
    sets["household"] = (np.concatenate([a, second]), np.concatenate([a // 3, second // 3 + 11]))
    members = rng.permutation(A)[:2400]
    sets["school"] = (members, np.arange(2400) // 4)
    sets["university"] = (np.concatenate([a, a]), np.concatenate([np.zeros(A, dtype=np.int64), 1 + a // 700]))
    sizes = []
    while sum(sizes) < A:
        sizes.append(int(rng.integers(2, 21)))
    sets["leisure"] = (np.concatenate([a, a]), np.concatenate([np.zeros(A, dtype=np.int64),
                                                                1 + np.repeat(np.arange(len(sizes)), sizes)[:A]]))
    out = {}
    for name, (agent, venue) in sets.items():
        if name != "household":                      # (the run form needs the household edges in agent order)
            perm = rng.permutation(len(agent))
            agent, venue = agent[perm], venue[perm]
        out[name] = {"agent": agent.astype(np.int64), "venue": venue.astype(np.int64),
                     "people": np.bincount(venue).astype(np.int64) + 1}
    age = rng.integers(0, 100, A)
    sex = rng.integers(0, 2, A)
    x = np.where(rng.random(A) < 0.3, 0.0, rng.uniform(2.0 ** -10, 1.0, A)).astype(np.float32)
    return dict(sets=out, age=age, sex=sex, x=x)


def networks_of(nk):
    """(names in accumulation order, specs, betas, {set: [per-agent weight of each of its networks]})."""
    rng = np.random.default_rng(200 + nk)
    w = world()
    names, specs, betas, weights = [], [], {}, {s: [] for s in SETS}
    for name in ("school", "university"):
        names.append(name)
        specs.append(NetworkSpec(name, name, N.MASK_Q))
        weights[name].append(np.ones(A, dtype=np.float32))
    for k in range(nk):
        table = rng.uniform(0.6, 1.0, (2, 2, 100)).astype(np.float32)
        names.append(f"leisure{k}")
        specs.append(NetworkSpec(f"leisure{k}", "leisure", N.MASK_QL_AGE75 if k % 3 == 1 else N.MASK_QL, table))
        weights["leisure"].append(table[0, w["sex"], w["age"]])
    names.append("household")
    specs.append(NetworkSpec("household", "household", N.MASK_RAW))
    weights["household"].append(np.ones(A, dtype=np.float32))
    for i, n in enumerate(names):
        betas[n] = float(np.float32(0.29 * (i + 1)))
    return names, specs, betas, weights


_CACHE = {}


def world():
    if "world" not in _CACHE:
        _CACHE["world"] = make_sets()
    return _CACHE["world"]


def engines_of(nk, sv_max, device):
    """(16-bit ids, 8-bit ids where a set is eligible): two engines on ONE compiled plan."""
    key = (nk, sv_max)
    if key not in _CACHE:
        w = world()
        _, specs, _, _ = networks_of(nk)
        host = compile_plan(A, w["sets"], age=w["age"], sex=w["sex"], layout="tiled", nets_per_set={"leisure": nk},
                            eb_target=EB_TARGET, sv_max=sv_max, direct=False,
                            runs=("household",))
        _CACHE[key] = tuple(InfectionEngine(DevicePlan(host, specs, device, lv8=on))
                            for on in (False, True))
    return _CACHE[key]


# ---- the restatement (tests/test_gpu_venue_multinet.py, for any set) ---------------------------------------------------
def restate(es, weights, betas, x):
    """[cum [V] float32 of each network of the set]."""
    a, v = es["agent"], es["venue"]
    V = len(es["people"])
    with np.errstate(all="ignore"):
        pc = np.clip(np.float32(1.0) / (es["people"] - 1).astype(np.float32), np.float32(0.0), np.float32(1.0))
    limit = term_limit_bits(int(np.bincount(v).max()))
    cum = []
    for wk, beta in zip(weights, betas):
        with np.errstate(all="ignore"):
            term = (wk[a] * x[a]).astype(np.float32)
            ok = (term.view(np.uint32) & 0x7FFFFFFF) <= limit
            sums = np.zeros(V, dtype=np.int64)
            np.add.at(sums, v[ok], np.rint(term[ok].astype(np.float64) * 2.0 ** 36).astype(np.int64))
            pos, neg = np.zeros(V, dtype=bool), np.zeros(V, dtype=bool)
            pos[v[~ok & ~(term < 0)]] = True
            neg[v[~ok & ~(term > 0)]] = True
            s = (sums.astype(np.float64) * 2.0 ** -36).astype(np.float32)
            s = np.where(pos & neg, np.float32(np.nan), np.where(pos, SATURATED, np.where(neg, -SATURATED, s)))
            cum.append(((np.float32(beta) * pc).astype(np.float32) * s).astype(np.float32))
    return cum


def launch(engine, nk, x, device):
    """Phases A + B + C on the transmissions x: ({set: cum [V, networks]}, {set: the per-slot values phase C wrote})."""
    names, _, betas, _ = networks_of(nk)
    p = engine.params(now=1.0, delta_time=1.0, day_type=0, active=names, betas=betas)
    xs = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
    bufs = AgentBuffers(engine.plan, susceptibility=torch.ones(A, device=device), transmission=xs)
    engine.step_phase(bufs, p, engine.io(), 8)
    torch.cuda.synchronize()
    plan = engine.plan
    return ({s: plan.cum_of(s).cpu().numpy().copy() for s in SETS},
            {s: plan.keep[plan.host.set_index[s]]["val"].cpu().numpy().copy() for s in SETS})


def check_cum(nk, sv_max, x, device, what):
    w = world()
    names, _, betas, weights = networks_of(nk)
    off, on = engines_of(nk, sv_max, device)
    cum_off, val_off = launch(off, nk, x, device)
    cum_on, val_on = launch(on, nk, x, device)
    for s in SETS:
        mine = [n for n in names if (n if not n.startswith("leisure") else "leisure") == s]
        want = restate(w["sets"][s], weights[s], [betas[n] for n in mine], x)
        assert cum_on[s].shape == (len(w["sets"][s]["people"]), len(mine))
        for k in range(len(mine)):
            assert_same_bits(np.ascontiguousarray(cum_on[s][:, k]), want[k], f"{what}: {mine[k]}, 8-bit ids")
            assert_same_bits(np.ascontiguousarray(cum_off[s][:, k]), want[k], f"{what}: {mine[k]}, 16-bit ids")
        # phase C read the same ids: every slot's value (pad slots hold 0 in both)
        assert np.array_equal(val_on[s].view(np.uint32), val_off[s].view(np.uint32)), f"{what}: {s}, phase C"
    return cum_on


# ---- 1. cum with and without the 8-bit ids --------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", NKS)
def test_cum_with_8_bit_ids_bit_for_bit(device, nk):
    off, on = engines_of(nk, 255, device)
    host = on.plan.host
    nv = {s: np.diff(_host(host.sets[host.set_index[s]].tiled.blk_v0)) for s in SETS}
    # what the world was built for
    assert list(nv["school"]) == [255, 255, 90]                          # blocks of exactly 255 venues
    assert nv["university"][0] == 1 and len(nv["leisure"]) >= 3          # a block of one venue; several leisure blocks
    assert host.sets[host.set_index["household"]].tiled.runs is not None and host.sets[0].tiled.n_edges > 0
    for s in SETS:                                                       # every set is eligible, and only `on` has the array
        i = host.set_index[s]
        assert nv[s].max() <= 255 and on.plan.lv8[i] is not None and on.aux.e_lv8[i]
        assert off.plan.lv8[i] is None and not off.aux.e_lv8[i]
        t = host.sets[i].tiled
        e_lv, blk_e0 = _host(t.e_lv).view(np.uint16), _host(t.blk_e0).astype(np.int64)
        assert any(e_lv[e - 1] == 0xFFFF and e_lv[e - 8] != 0xFFFF for e in blk_e0[1:]), f"{s}: no group is partly pad slots"
    for s, least in (("university", 8), ("leisure", 1)):                # waves whose 512 slots are the venue of everybody
        t = host.sets[host.set_index[s]].tiled
        e_lv, e1 = _host(t.e_lv).view(np.uint16), int(_host(t.blk_e0)[1])
        assert (e_lv[: e1 // 512 * 512] == 0).reshape(-1, 512).all(axis=1).sum() >= least, s
    x = world()["x"]
    cum = check_cum(nk, 255, x, device, f"nk={nk}")
    assert all(np.abs(c).max() > 0 for c in cum.values())
    # values that cannot be summed: a NaN, infinities and terms outside every window, in every set
    rng = np.random.default_rng(nk)
    for value in (np.nan, np.inf, -np.inf, 3.0e4, -3.0e4):
        xv = x.copy()
        xv[rng.choice(A, 3, replace=False)] = value
        check_cum(nk, 255, xv, device, f"nk={nk} value={value}")


def test_a_block_of_256_venues_keeps_the_16_bit_ids(device):
    off, on = engines_of(2, 256, device)
    host = on.plan.host
    i = host.set_index["school"]
    assert list(np.diff(_host(host.sets[i].tiled.blk_v0))) == [256, 256, 88]
    assert on.plan.lv8[i] is None and not on.aux.e_lv8[i]               # not eligible: the field stays NULL
    assert on.plan.lv8[host.set_index["leisure"]] is not None           # (the other sets of the plan are)
    check_cum(2, 256, world()["x"], device, "256 venues")


# ---- 2. the device kernel and its numpy specification ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_device_and_host_narrowing_agree(device, seed):
    w = make_world("c3", n_agents=3000 + 517 * seed, seed=seed, infected_fraction=0.05)
    for dev in (None, device):                                           # the plan compiled with numpy and on the device
        host = compile_plan(w["n_agents"], w["edge_sets"], age=w["age"], sex=w["sex"], layout="tiled", eb_target=2048,
                            sv_max=255, device=dev)
        plan = DevicePlan(host, B.network_specs(w), device)
        torch.cuda.synchronize()
        seen = 0
        for i, s in enumerate(host.sets):
            if plan.lv8[i] is None:
                continue
            want = narrow_venue_ids(s.tiled.e_lv)
            got = plan.lv8[i].cpu().numpy()
            assert got.dtype == np.uint8 and len(got) == -(-len(want) // 8) * 8
            assert np.array_equal(got[: len(want)], want), s.name
            assert (got[len(want):] == 0xFF).all()
            e16 = _host(s.tiled.e_lv).view(np.uint16)
            assert np.array_equal(want == 0xFF, e16 == 0xFFFF) and np.array_equal(want[want != 0xFF], e16[e16 != 0xFFFF])
            seen += (want == 0xFF).any() and (want != 0xFF).any()
        assert seen >= 3


# ---- 3. a whole step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [None, False], ids=["direct-auto", "direct-off"])
@pytest.mark.parametrize("preset", ["c3", "june"])
def test_a_whole_step_bit_for_bit(device, preset, direct):
    """Three production steps (Philox noise) on a 60 000-agent world of the benchmark's shape: every output and every
    state array equal with the 8-bit ids on and off.  direct=False: the eligible sets take pass 2 through phase C,
    which reads the ids too."""
    key = ("step-world", preset)
    if key not in _CACHE:
        _CACHE[key] = make_world(preset, n_agents=60_000, seed=21, infected_fraction=0.05)
    w = _CACHE[key]
    w = dict(w, state={k: v.copy() for k, v in w["state"].items()})
    specs, betas = B.network_specs(w), B.betas_of(w)
    runs = [SingleGpuHotPath(w, specs, betas, device, seed=9, layout="tiled", lv8=on, direct=direct,
                             quarantine_threshold=4.0) for on in (False, True)]
    off, on = runs
    eligible = [s.name for i, s in enumerate(on.engine.plan.host.sets) if on.engine.plan.lv8[i] is not None]
    assert "leisure" in eligible and len(eligible) >= 2, eligible
    assert all(t is None for t in off.engine.plan.lv8)
    if direct is False:
        assert all(s.tiled.ell_k == 0 for s in on.engine.plan.host.sets)
    for step in range(3):
        for r in runs:
            r.step()
        torch.cuda.synchronize()
        for k in off.state:
            assert torch.equal(off.state[k].view(torch.int32), on.state[k].view(torch.int32)), (step, k)
        assert torch.equal(off.probs.view(torch.int32), on.probs.view(torch.int32)), step
        assert torch.equal(off.new_infected, on.new_infected), step
        for i, s in enumerate(on.engine.plan.host.sets):
            assert torch.equal(off.engine.plan.cum[i].view(torch.int32), on.engine.plan.cum[i].view(torch.int32)), (step, s.name)
    assert float(on.new_infected.sum()) > 0
