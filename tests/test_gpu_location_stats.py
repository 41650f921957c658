"""GPU: gj_location_stats against the numpy restatement (tests/gj_location_ref.py).  The tests fill the plan's ``cum``
workspaces themselves, so no step needs to run.

Bit-equal case: ``cum``, the leisure tables and ``s0`` are multiples of 2^-8 in [0, 4].  An agent has at most 130 + 8
edges per set, so a sum stays below 2^10 with 8 fractional bits (18 bits), times a table value and s0 (10 bits each):
38 bits - every fp64 product and sum is exact in any order, only the correctly rounded division t_n / T rounds, and
``out`` must equal the restatement bit for bit.

General inputs: per (group, column) within ``(n_cols + 1) * count(group)`` units of 2^-30 - one unit of floor per column
and agent, plus a remainder of fewer than n_cols units that may land on another column on a near-tie; row sums exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import gj_location_ref as R
import gj_testlib as L
from grad_june_amd import _native as N
from grad_june_amd.groups import LocationError, LocationStats

pytestmark = pytest.mark.gpu

GUARD = 8
SENTINEL = -(1 << 40) - 777
LEISURE = ("pub", "gym", "care_visit")
ACTIVE = ["company", "pub", "gym", "care_visit", "household"]       # `school` is in the plan and absent from nets
THRESHOLD = 4.0
LONG_ROW = 130       # edges of agent 0 in `company`: the wave-stride loop wraps twice and leaves a partial pass


def make_world(A, seed=0):
    """Four edge sets: household (one edge for most agents), company (agent 0: LONG_ROW edges), school, leisure (0 - 3
    edges).  Every seventh agent (a % 7 == 6) has no edge in any set."""
    rng = np.random.default_rng(1000 + A + seed)
    lonely = (np.arange(A) % 7 == 6) & (A > 1)
    sets = {}

    def add(name, agent, n_venues):
        agent = np.asarray(agent, dtype=np.int64)
        agent = agent[~lonely[agent]]
        agent = agent[rng.permutation(len(agent))]                   # COO order: not sorted by agent
        if len(agent) == 0:
            agent = np.zeros(1, dtype=np.int64)
        venue = rng.integers(0, n_venues, len(agent))
        people = np.bincount(venue, minlength=n_venues) + 1
        sets[name] = {"agent": torch.from_numpy(agent), "venue": torch.from_numpy(venue), "people": torch.from_numpy(people)}

    everyone = np.arange(A)
    add("household", everyone, max(1, A // 3))
    add("company", np.concatenate((np.zeros(LONG_ROW, dtype=np.int64), everyone[rng.random(A) < 0.5])), max(2, A // 4))
    add("school", everyone[rng.random(A) < 0.3], max(1, A // 50))
    add("leisure", np.repeat(everyone, rng.integers(0, 4, A)), 5)
    age = rng.integers(0, 100, A)
    if A >= 63:
        age[:8] = [76, 75, 90, 10, 99, 74, 80, 30]
    world = {"n_agents": A, "age": torch.from_numpy(age), "sex": torch.from_numpy(rng.integers(0, 2, A)), "edge_sets": sets}
    tables = {n: torch.from_numpy((rng.integers(0, 1025, (2, 2, 100)) / 256.0).astype(np.float32)) for n in LEISURE}
    return world, tables


def exact_values(rng, shape):
    return (rng.integers(0, 1025, shape) / 256.0).astype(np.float32)


def engine_and_cum(world, tables, device, layout, cum):
    """The engine, its ``cum`` workspaces filled from ``cum`` = {set: float32 [V, stride]}."""
    eng = L.make_engine(world, tables, device, layout=layout)
    for s, values in cum.items():
        dst = eng.plan.cum_of(s)
        assert tuple(dst.shape) == values.shape, (s, dst.shape, values.shape)
        dst.copy_(torch.from_numpy(values))
    return eng


def draw_cum(world, rng, draw=exact_values):
    return {s: draw(rng, (len(es["people"]), 3 if s == "leisure" else 1)) for s, es in world["edge_sets"].items()}


def edges_of(world):
    return {s: (es["agent"], es["venue"]) for s, es in world["edge_sets"].items()}


def terms_of(world, tables, active, cum, s0, stage, day_type):
    """[n_nets, A] by the restatement; column k of a set = the k-th of ITS networks among ``active``."""
    q = None if stage is None else (stage < np.float32(THRESHOLD)).astype(np.float64)
    per_set, by_name = {}, {}
    for name in active:
        s = L.edge_set_name(name)
        by_name[name] = cum[s][:, per_set.get(s, 0)]
        per_set[s] = per_set.get(s, 0) + 1
    return R.step_terms(world, {k: v.numpy() for k, v in tables.items()}, active, by_name, s0, day_type, q)


def launch(eng, world, device, active, nu, s0, stage, group, G, cols, n_cols, background, day_type=0, base=None,
           check=True):
    """out [G, n_cols] (int64, numpy) after one launch on top of ``base`` (zeros), the guards around it verified, and
    the error word."""
    p = eng.params(now=1.0, delta_time=1.0, day_type=day_type, active=active, betas=dict.fromkeys(active, 1.0),
                   has_quarantine=stage is not None, q_threshold=THRESHOLD)
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
    stats = LocationStats(dev(group, np.int32), G, [f"c{i}" for i in range(n_cols)], device=device)
    buf = torch.full((G * n_cols + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=device)
    stats.out = buf[GUARD: GUARD + G * n_cols].view(1, G, n_cols)
    if base is None:
        stats.out.zero_()
    else:
        stats.out.copy_(torch.from_numpy(base).view(1, G, n_cols))
    stats.add(eng.plan, p, dev(nu, np.float32), dev(s0, np.float32), dev(stage, np.float32),
              active=[f"c{c}" for c in cols], background=f"c{background}", edges=edges_of(world))
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), "wrote outside out"
    err = int(stats.err.item())
    if check:
        stats.check()
    return stats.out[0].cpu().numpy(), err


def as_array(out):
    return np.array(out, dtype=np.int64)


def state(A, rng):
    s0 = exact_values(rng, A)
    s0[rng.random(A) < 0.2] = 0.0
    stage = rng.integers(1, 8, A).astype(np.float32)                 # below, at and above the threshold of 4
    return s0, stage


# ---- 1. bit for bit ---------------------------------------------------------------------------------------------------------
CASES = [(1, "csr"), (1, "tiled"), (63, "tiled"), (64, "tiled"), (65, "tiled"), (257, "tiled"), (1000, "tiled")]


@pytest.mark.parametrize("G", [1, 3, 5000])
@pytest.mark.parametrize("A,layout", CASES)
def test_kernel_equals_the_restatement_bit_for_bit(device, A, layout, G):
    world, tables = make_world(A)
    rng = np.random.default_rng(A * 13 + G)
    cum = draw_cum(world, rng)
    eng = engine_and_cum(world, tables, device, layout, cum)
    assert (eng.plan.c.sets[0].a_rowptr is not None) == (layout == "csr")      # csr: the plan's own rows are reused
    s0, stage = state(A, rng)
    group = None if G == 1 else rng.integers(0, G, A)
    n = len(ACTIVE)
    assert (G * (n + 1) <= N.GJ_LOC_LDS_BINS) == (G < 5000)                     # both accumulation regimes
    draws = {"some": (rng.random(A) < 0.3).astype(np.float32), "none": np.zeros(A, np.float32),
             "all": np.ones(A, np.float32)}
    for day_type in (0, 1):
        terms = terms_of(world, tables, ACTIVE, cum, s0, stage, day_type)
        for what, nu in draws.items():
            base = rng.integers(-5, 1 << 40, (G, n + 1))
            got, err = launch(eng, world, device, ACTIVE, nu, s0, stage, group, G, list(range(n)), n + 1, n, day_type, base)
            want, want_err = R.location_stats(terms, nu, group, G, list(range(n)), n + 1, n)
            assert err == want_err == 0
            assert np.array_equal(got - base, as_array(want)), (what, day_type)
            assert int((got - base).sum()) == R.U * int(nu.sum())
            if what == "none":
                assert np.array_equal(got, base)                                  # out untouched
    # fewer networks, shared and permuted columns, no quarantine; and no network at all (the seeding step)
    few = ["company", "pub", "care_visit", "household"]
    terms = terms_of(world, tables, few, cum, s0, None, 0)
    got, err = launch(eng, world, device, few, draws["all"], s0, None, group, G, [2, 0, 0, 1], 4, 3)
    want, _ = R.location_stats(terms, draws["all"], group, G, [2, 0, 0, 1], 4, 3)
    assert err == 0 and np.array_equal(got, as_array(want))
    got, err = launch(eng, world, device, [], draws["some"], s0, stage, group, G, [], 2, 1)
    want, _ = R.location_stats(np.zeros((0, A)), draws["some"], group, G, [], 2, 1)
    assert err == 0 and np.array_equal(got, as_array(want))
    assert int(got[:, 1].sum()) == R.U * int(draws["some"].sum()) and not got[:, 0].any()


def test_what_each_mask_does_to_an_infection(device):
    """Directly, on the 257-agent world: care_visit gives nothing to agents of 75 or under; an agent at or above the
    quarantine threshold is attributed to the household alone; s0 == 0 goes to background; so does an agent without an
    edge; the agent with LONG_ROW company edges gets all of them."""
    A = 257
    world, tables = make_world(A)
    rng = np.random.default_rng(3)
    cum = {s: v + np.float32(1 / 256) for s, v in draw_cum(world, rng).items()}          # no zero sum by chance
    for t in tables.values():
        t += 1 / 256
    eng = engine_and_cum(world, tables, device, "tiled", cum)
    age = world["age"].numpy()
    n = len(ACTIVE)
    col = {name: i for i, name in enumerate(ACTIVE)}
    ones = np.ones(A, np.float32)
    low = np.full(A, 1.0, np.float32)
    leisure_goers = np.bincount(world["edge_sets"]["leisure"]["agent"].numpy(), minlength=A) > 0
    has_home = np.bincount(world["edge_sets"]["household"]["agent"].numpy(), minlength=A) > 0

    def run(mask, s0=ones, stage=low):
        nu = mask.astype(np.float32)
        got, err = launch(eng, world, device, ACTIVE, nu, s0, stage, None, 1, list(range(n)), n + 1, n)
        assert err == 0 and got.sum() == R.U * int(mask.sum())
        return got[0]

    young = run((age <= 75) & leisure_goers)
    assert young[col["care_visit"]] == 0 and young[col["pub"]] > 0 and young[col["gym"]] > 0
    old = run((age > 75) & leisure_goers)
    assert ((age > 75) & leisure_goers).sum() >= 3 and old[col["care_visit"]] > 0
    high = np.full(A, THRESHOLD, np.float32)
    high[::2] = THRESHOLD + 2
    quarantined = run(np.ones(A, bool), stage=high)
    assert quarantined[col["household"]] == R.U * int(has_home.sum())
    assert quarantined[n] == R.U * int((~has_home).sum()) and not quarantined[: col["household"]].any()
    immune = run(np.ones(A, bool), s0=np.zeros(A, np.float32))
    assert immune[n] == R.U * A and not immune[:n].any()
    lonely = np.arange(A) % 7 == 6
    assert run(lonely)[n] == R.U * int(lonely.sum())
    only0 = np.zeros(A, bool)
    only0[0] = True
    es = world["edge_sets"]["company"]
    rows0 = es["venue"].numpy()[es["agent"].numpy() == 0]
    assert len(rows0) >= LONG_ROW
    single = run(only0)
    terms = terms_of(world, tables, ACTIVE, cum, ones, low, 0)
    assert terms[col["company"], 0] == cum["company"][rows0, 0].astype(np.float64).sum()
    want, _ = R.location_stats(terms, only0.astype(np.float32), None, 1, list(range(n)), n + 1, n)
    assert np.array_equal(single, as_array(want)[0]) and single[col["company"]] > 0


# ---- 2. no order of the agents changes a bit ------------------------------------------------------------------------------
def generic_values(rng, shape):
    return (rng.random(shape) * rng.choice([1e-3, 1.0, 50.0], shape)).astype(np.float32)


@pytest.mark.parametrize("G", [3, 5000])
def test_permuting_the_agents_gives_identical_bits(device, G):
    A = 1000
    world, tables = make_world(A)
    rng = np.random.default_rng(17 + G)
    cum = draw_cum(world, rng, generic_values)
    s0, stage = rng.random(A).astype(np.float32), rng.integers(1, 8, A).astype(np.float32)
    nu = (rng.random(A) < 0.4).astype(np.float32)
    group = rng.integers(0, G, A)
    n = len(ACTIVE)
    eng = engine_and_cum(world, tables, device, "tiled", cum)
    once, err = launch(eng, world, device, ACTIVE, nu, s0, stage, group, G, list(range(n)), n + 1, n)
    assert err == 0 and once.sum() == R.U * int(nu.sum())
    perm = rng.permutation(A)                     # new id of agent a: perm[a]; the COO order of every set stays
    inverse = np.argsort(perm)
    moved = dict(world, age=world["age"][inverse], sex=world["sex"][inverse], edge_sets={
        s: dict(es, agent=torch.from_numpy(perm)[es["agent"]]) for s, es in world["edge_sets"].items()})
    eng2 = engine_and_cum(moved, tables, device, "tiled", cum)
    again, err = launch(eng2, moved, device, ACTIVE, nu[inverse], s0[inverse], stage[inverse], group[inverse], G,
                        list(range(n)), n + 1, n)
    assert err == 0 and again.tobytes() == once.tobytes()


# ---- 3. general inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3, 5000])
def test_general_inputs_within_the_floor_and_remainder_bound(device, G):
    A = 1000
    world, tables = make_world(A, seed=1)
    rng = np.random.default_rng(29 + G)
    cum = draw_cum(world, rng, generic_values)
    # saturated venues, and what must never reach a bin as a share: NaN and negative sums (far from cancelling)
    cum["company"][:60, 0] = 1e30
    cum["household"][0, 0], cum["household"][1, 0] = np.nan, -1e6
    cum["leisure"][0, 1], cum["leisure"][1, 2] = np.nan, -1e6
    eng = engine_and_cum(world, tables, device, "tiled", cum)
    s0, stage = rng.random(A).astype(np.float32), rng.integers(1, 8, A).astype(np.float32)
    s0[rng.random(A) < 0.1] = 0.0
    nu = (rng.random(A) < 0.5).astype(np.float32)
    group = None if G == 1 else rng.integers(0, G, A)
    n = len(ACTIVE)
    terms = terms_of(world, tables, ACTIVE, cum, s0, stage, 1)
    want, want_err = R.location_stats(terms, nu, group, G, list(range(n)), n + 1, n)
    assert want_err == R.ERR_VALUE
    got, err = launch(eng, world, device, ACTIVE, nu, s0, stage, group, G, list(range(n)), n + 1, n, day_type=1, check=False)
    assert err == N.GJ_LOC_ERR_VALUE
    g = np.zeros(A, np.int64) if group is None else group
    count = np.bincount(g[nu == 1], minlength=G)
    assert np.array_equal(got.sum(1), R.U * count)                               # row sums: exact
    worst = np.abs(got - as_array(want)).max(1)
    print("largest deviation per group, in units of 2^-30:", int(worst.max()), "bound per infection:", n + 2)
    assert np.all(worst <= (n + 2) * count)
    saturated = np.isin(np.arange(A), world["edge_sets"]["company"]["agent"].numpy()[
        world["edge_sets"]["company"]["venue"].numpy() < 60])
    assert (saturated & (nu == 1) & (s0 > 0) & (stage < THRESHOLD)).sum() >= 3    # 1e30 took part
    # bad labels and values are skipped and reported, the others are counted as before
    if group is not None:
        bad_nu, bad_group = nu.copy(), group.copy()
        at = np.nonzero(nu == 1)[0][:3]
        bad_nu[at[0]], bad_nu[at[1]], bad_group[at[2]] = 0.5, np.nan, G
        got2, err2 = launch(eng, world, device, ACTIVE, bad_nu, s0, stage, bad_group, G, list(range(n)), n + 1, n,
                            day_type=1, check=False)
        keep_nu = nu.copy()
        keep_nu[at] = 0.0
        only, _ = launch(eng, world, device, ACTIVE, keep_nu, s0, stage, group, G, list(range(n)), n + 1, n, day_type=1,
                         check=False)
        assert err2 == N.GJ_LOC_ERR_VALUE | N.GJ_LOC_ERR_LABEL
        assert np.array_equal(got2, only)


def test_the_error_word_is_sticky_and_check_raises_once(device):
    A = 65
    world, tables = make_world(A)
    rng = np.random.default_rng(5)
    eng = engine_and_cum(world, tables, device, "tiled", draw_cum(world, rng))
    p = eng.params(now=1.0, delta_time=1.0, day_type=0, active=ACTIVE, betas=dict.fromkeys(ACTIVE, 1.0))
    stats = LocationStats(torch.full((A,), 9, dtype=torch.int32), 3, ACTIVE + ["background"], device=device)
    ones = torch.ones(A, device=device)
    stats.add(eng.plan, p, ones, ones, None, active=ACTIVE, edges=edges_of(world))
    stats.add(eng.plan, p, torch.zeros(A, device=device), ones, None, active=ACTIVE)     # a clean launch keeps the word
    assert int(stats.err.item()) == N.GJ_LOC_ERR_LABEL and not bool(stats.out.any())
    with pytest.raises(LocationError, match="label"):
        stats.check()
    stats.check()
    assert stats.values().shape == (1, 3, len(ACTIVE) + 1) and stats.values().dtype == torch.float32


# ---- 4. argument errors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["csr", "tiled"])
def test_argument_errors_are_returned_before_any_device_work(device, layout):
    A = 65
    world, tables = make_world(A)
    rng = np.random.default_rng(7)
    eng = engine_and_cum(world, tables, device, layout, draw_cum(world, rng))
    lib = N.load()
    n = len(ACTIVE)
    ones = torch.ones(A, device=device)
    out = torch.full((3 * (n + 1),), SENTINEL, dtype=torch.int64, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    labels = torch.zeros(A, dtype=torch.int32, device=device)
    rows = eng.plan.location_rows(edges_of(world))
    good = dict(plan=C.byref(eng.plan.c), params=None, rows=rows, nu=N.ptr(ones), s0=N.ptr(ones), stage=None,
                group=N.ptr(labels), n_groups=3, cols=(C.c_int32 * n)(*range(n)), n_cols=n + 1, background=n,
                out=N.ptr(out), err=N.ptr(err))

    def params(**kw):
        kw = dict(dict(now=1.0, delta_time=1.0, day_type=0, active=ACTIVE, betas=dict.fromkeys(ACTIVE, 1.0)), **kw)
        return eng.params(**kw)

    def call(p=None, **change):
        a = dict(good, **change)
        if a["params"] is None:
            a["params"] = C.byref(p if p is not None else params())
        return lib.gj_location_stats(a["plan"], a["params"], a["rows"], a["nu"], a["s0"], a["stage"], a["group"],
                                     a["n_groups"], a["cols"], a["n_cols"], a["background"], a["out"], a["err"],
                                     N.current_stream())

    E_NULL, E_RANGE = -1, -2
    for name in ("plan", "rows", "nu", "s0", "out", "err", "cols"):
        assert call(**{name: None}) == E_NULL, name
    assert lib.gj_location_stats(good["plan"], None, rows, good["nu"], good["s0"], None, good["group"], 3, good["cols"],
                                 n + 1, n, good["out"], good["err"], None) == E_NULL
    assert call(params(has_quarantine=True, q_threshold=4.0)) == E_NULL            # quarantine without a stage
    assert call(params(has_quarantine=True, q_threshold=4.0), stage=N.ptr(ones)) == 0
    out.fill_(SENTINEL)
    err.zero_()
    p = params()
    p.n_nets = N.GJ_MAX_NETS + 1
    assert call(p) == E_RANGE
    p.n_nets = -1
    assert call(p) == E_RANGE
    for change in (dict(n_groups=0), dict(n_groups=N.GJ_MAX_GROUPS + 1), dict(group=None), dict(n_cols=0),
                   dict(n_cols=N.GJ_LOC_MAX_COLS + 1), dict(background=-1), dict(background=n + 1),
                   dict(cols=(C.c_int32 * n)(0, 1, n + 1, 2, 3)), dict(cols=(C.c_int32 * n)(0, -1, 1, 2, 3))):
        assert call(**change) == E_RANGE, change
    half = (N.LocationRows * N.GJ_MAX_SETS)()
    for i in range(N.GJ_MAX_SETS):
        half[i].a_rowptr = rows[i].a_rowptr
    assert call(rows=half) == E_NULL                                               # row pointers without venues
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and int(err.item()) == 0                  # nothing was launched
    assert call(group=None, n_groups=1) == 0 and call() == 0
    none = (N.LocationRows * N.GJ_MAX_SETS)()                                      # no rows at all: everything is background
    out.zero_()
    assert call(rows=none) == 0
    torch.cuda.synchronize()
    got = out.view(3, n + 1).cpu().numpy()
    assert got[0, n] == R.U * A and got.sum() == R.U * A and int(err.item()) == 0


def test_an_empty_world_launches_nothing(device):
    lib = N.load()
    plan, p = N.Plan(), N.StepParams()
    out = torch.full((2,), SENTINEL, dtype=torch.int64, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    one = torch.ones(1, device=device)
    assert lib.gj_location_stats(C.byref(plan), C.byref(p), None, N.ptr(one), N.ptr(one), None, None, 1, None, 2, 1,
                                 N.ptr(out), N.ptr(err), N.current_stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
