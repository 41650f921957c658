"""GPU: gj_infection_tree against the numpy restatement (tests/gj_tree_ref.py), on the worlds of
tests/test_gpu_location_stats.py: agent 0's 130-edge row (several chunks of 16 positions and a partial one), a 3-network
set, leisure venues of some hundred members (long venue rows), agents without edges.  The tests fill the plan's ``cum``
workspaces and the transmissions themselves, so no step needs to run.

Bit-equal case: ``cum``, the leisure tables, ``s0`` and ``transmission`` are multiples of 2^-8 in [0, 4] - the argument of
test_gpu_location_stats.py: every fp64 product and sum is exact in any order, only the correctly rounded divisions round,
and the weights m * transmission * 2^36 are integers - so every output must equal the restatement exactly.

General inputs: T reassociates, so a share u may differ by a unit and with it, rarely, a choice; what holds for every
choice is asserted instead."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gj_infector_ref as I
import gj_tree_ref as T
from grad_june_amd import _native as N
from grad_june_amd.groups import InfectionTree, InfectionTreeError
from test_gpu_location_stats import (ACTIVE, CASES, GUARD, THRESHOLD, draw_cum, edges_of, engine_and_cum, exact_values,
                                     generic_values, make_world, state)

pytestmark = pytest.mark.gpu

BETAS = {"company": 0.75, "pub": 0.5, "gym": 1.25, "care_visit": 2.0, "household": 1.5, "school": 1.0}
FEW = ["company", "pub", "care_visit", "household"]
COLUMNS = ACTIVE + ["background", "seed"]
ROWS = 8
PER_AGENT = ("infector", "via", "venue", "infected_row")


class Harness:
    """An engine with its ``cum`` filled and an InfectionTree whose outputs sit between sentinels."""

    def __init__(self, world, tables, device, layout, cum):
        self.world, self.tables, self.device, self.cum, self.A = world, tables, device, cum, world["n_agents"]
        self.eng = engine_and_cum(world, tables, device, layout, cum)
        self.set_order = [s.name for s in self.eng.plan.host.sets]
        self.tree = tr = InfectionTree(self.A, COLUMNS, device=device, n_rows=ROWS)
        self.guards = []
        for name, dtype, fill, sentinel in [(k, torch.int32, -1, -777777) for k in PER_AGENT] + [
                ("counts", torch.int64, 0, -(1 << 40) - 777), ("unresolved", torch.int64, 0, -(1 << 40) - 777)]:
            shape = getattr(tr, name).shape
            buf = torch.full((getattr(tr, name).numel() + 2 * GUARD,), sentinel, dtype=dtype, device=device)
            view = buf[GUARD: -GUARD]
            view.fill_(fill)
            self.guards.append((buf, sentinel))
            setattr(tr, name, view.view(shape))

    def params(self, active, stage, day_type=0):
        return self.eng.params(now=1.0, delta_time=1.0, day_type=day_type, active=active, betas=BETAS,
                               has_quarantine=stage is not None, q_threshold=THRESHOLD)

    def dev(self, a, dt=np.float32):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)

    def intact(self):
        torch.cuda.synchronize()
        for buf, sentinel in self.guards:
            assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[-GUARD:] == sentinel).all()), "wrote outside an output"

    def record(self, active, nu, s0, stage, tr, day_type=0, row=0, seed=1, step=0, background="background"):
        self.tree.record(self.eng.plan, self.params(active, stage, day_type), self.dev(nu), self.dev(s0), self.dev(stage),
                         self.dev(tr), active=active, background=background, row=row, edges=edges_of(self.world),
                         seed=seed, step=step)
        self.intact()
        return self.outputs()

    def outputs(self):
        t = self.tree
        out = {k: getattr(t, k).cpu().numpy().copy() for k in PER_AGENT + ("counts", "unresolved")}
        out["err"] = int(t.err.item())
        return out

    def nets(self, active, stage, day_type=0):
        q = None if stage is None else (stage < np.float32(THRESHOLD)).astype(np.float64)
        return I.step_nets(self.world, self.tables, active, BETAS, day_type, q)

    def edges(self):
        return {s: (a.numpy(), v.numpy()) for s, (a, v) in edges_of(self.world).items()}

    def restated(self, want, active, nu, s0, stage, tr, day_type, row, seed, step, background="background"):
        """The restatement's outputs after this step, on top of ``want`` (None: a fresh run)."""
        cols = [COLUMNS.index(n) for n in active]
        step_out = T.infection_tree(self.nets(active, stage, day_type), self.edges(), self.cum, s0, nu, tr, cols, len(COLUMNS),
                                    COLUMNS.index(background), seed, step, self.A, self.set_order, row_value=row)
        if want is None:
            want = dict(infector=np.full(self.A, -1, np.int32), via=np.full(self.A, -1, np.int32),
                        venue=np.full(self.A, -1, np.int32), infected_row=np.full(self.A, -1, np.int32),
                        counts=np.zeros((ROWS, len(COLUMNS)), np.int64), unresolved=np.zeros(ROWS, np.int64), err=0)
        hit = step_out["row_of"] >= 0
        for k in ("infector", "via", "venue"):
            want[k][hit] = step_out[k][hit]
        want["infected_row"][hit] = row
        want["counts"][row] += step_out["counts"]
        want["unresolved"][row] += step_out["unresolved"]
        want["err"] |= step_out["err"]
        return want


def transmissions(A, rng, draw=exact_values):
    """Zero for about 70 % of the agents: venues without a transmitter leave an infection unresolved."""
    tr = draw(rng, A)
    tr[rng.random(A) < 0.7] = 0.0
    return tr


def same(got, want):
    return all(np.array_equal(got[k], want[k]) for k in PER_AGENT + ("counts", "unresolved")) and got["err"] == want["err"]


# ---- 1. bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,layout", CASES)
def test_the_tree_equals_the_restatement_exactly(device, A, layout):
    world, tables = make_world(A)
    rng = np.random.default_rng(A * 17 + 5)
    cum = draw_cum(world, rng)
    h = Harness(world, tables, device, layout, cum)
    assert h.set_order[0] == "household" and ACTIVE[-1] == "household"      # the sets' order is not the networks'
    s0, stage = state(A, rng)
    tr = transmissions(A, rng)
    draws = {"some": (rng.random(A) < 0.3).astype(np.float32), "none": np.zeros(A, np.float32),
             "all": np.ones(A, np.float32)}
    want = None
    steps = [(0, "some", stage, 11, 3), (1, "all", stage, 11, 4), (0, "none", stage, 11, 5), (1, "some", None, 12, 3),
             (0, "all", None, (1 << 63) + 9, (1 << 40) - 1)]
    for row, (day_type, what, stg, seed, step) in enumerate(steps):
        nu = draws[what]
        want = h.restated(want, ACTIVE, nu, s0, stg, tr, day_type, row, seed, step)
        got = h.record(ACTIVE, nu, s0, stg, tr, day_type, row=row, seed=seed, step=step)
        assert want["err"] == 0 and same(got, want), (what, day_type)
        assert int(got["counts"][row].sum()) == int(nu.sum())
        assert int(got["unresolved"][row]) == int((got["infector"][nu == 1] == T.UNRESOLVED).sum())
    if A >= 63:
        assert want["unresolved"].sum() > 0 and (want["infector"] >= 0).any() and (want["infector"] == T.NOBODY).any()
    # fewer networks (care_visit moves to column 1 of its set); and no network at all (the seeding step)
    want = h.restated(want, FEW, draws["all"], s0, stage, tr, 0, 5, 1, 1)
    got = h.record(FEW, draws["all"], s0, stage, tr, 0, row=5, seed=1, step=1)
    assert same(got, want)
    want = h.restated(want, [], draws["some"], s0, None, None, 0, 7, 1, 2, background="seed")
    got = h.record([], draws["some"], s0, None, None, 0, row=7, seed=1, step=2, background="seed")
    assert same(got, want)
    assert int(got["counts"][7, COLUMNS.index("seed")]) == int(draws["some"].sum())
    assert (got["infector"][draws["some"] == 1] == T.NOBODY).all()
    offspring = h.tree.offspring().cpu().numpy()
    assert offspring.dtype == np.int64 and np.array_equal(
        offspring, np.bincount(got["infector"][got["infector"] >= 0], minlength=A))


def test_agent_offset_moves_the_counter_and_the_ids(device):
    A = 257
    world, tables = make_world(A)
    rng = np.random.default_rng(77)
    cum = draw_cum(world, rng)
    h = Harness(world, tables, device, "tiled", cum)
    s0, stage = state(A, rng)
    tr, nu = transmissions(A, rng), np.ones(A, np.float32)
    offset = 1 << 20
    cols = [COLUMNS.index(n) for n in ACTIVE]
    want = T.infection_tree(h.nets(ACTIVE, stage), h.edges(), cum, s0, nu, tr, cols, len(COLUMNS),
                            COLUMNS.index("background"), 5, 6, A, h.set_order, agent_offset=offset, row_value=2)
    t, plan = h.tree, h.eng.plan
    lib = N.load()
    p, d_nu, d_s0, d_stage, d_tr = h.params(ACTIVE, stage), h.dev(nu), h.dev(s0), h.dev(stage), h.dev(tr)
    rc = lib.gj_infection_tree(
        C.byref(plan.c), C.byref(p), plan.location_rows(edges_of(world)),
        plan.venue_rows(edges_of(world)), N.ptr(d_nu), N.ptr(d_s0), N.ptr(d_stage), N.ptr(d_tr),
        (C.c_int32 * len(cols))(*cols), len(COLUMNS), COLUMNS.index("background"), 5, 6, offset, N.ptr(t.infector),
        N.ptr(t.via), N.ptr(t.venue), N.ptr(t.infected_row), 2, N.ptr(t.counts[2]), N.ptr(t.unresolved[2:]),
        N.ptr(t.err), N.current_stream())
    assert rc == 0
    h.intact()
    got = h.outputs()
    assert got["err"] == 0 and (got["infector"] >= offset).any()
    for k, name in (("infector", "infector"), ("via", "via"), ("venue", "venue"), ("infected_row", "row_of")):
        assert np.array_equal(got[k], want[name]), k
    assert np.array_equal(got["counts"][2], want["counts"]) and int(got["unresolved"][2]) == want["unresolved"]


# ---- 2. general inputs -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general_case():
    A = 1000
    world, tables = make_world(A, seed=1)
    rng = np.random.default_rng(41)
    cum = draw_cum(world, rng, generic_values)
    s0, stage = rng.random(A).astype(np.float32), rng.integers(1, 8, A).astype(np.float32)
    s0[rng.random(A) < 0.1] = 0.0
    nu = (rng.random(A) < 0.5).astype(np.float32)
    tr = transmissions(A, rng, generic_values)
    return dict(A=A, world=world, tables=tables, cum=cum, s0=s0, stage=stage, nu=nu, tr=tr)


def check_every_choice(h, c, got, nets, day_type):
    """What holds for every choice, whatever the roundings of T."""
    members = T.venue_members(h.edges(), {s: v.shape[0] for s, v in c["cum"].items()})
    rows = I.rows_of(h.edges(), c["A"])
    by_column = {COLUMNS.index(n): i for i, n in enumerate(ACTIVE)}
    flagged = np.nonzero(c["nu"] == 1)[0]
    for a in flagged:
        b, col, v = int(got["infector"][a]), int(got["via"][a]), int(got["venue"][a])
        if b == T.NOBODY:
            assert col == COLUMNS.index("background") and v == -1
            continue
        net = nets[by_column[col]]
        assert v in rows[net.set][a]
        assert net.w[a] * float(c["s0"][a]) * float(c["cum"][net.set][v, net.column]) > 0      # t_ie > 0
        if b == T.UNRESOLVED:
            W, _ = T.weights_of(members[net.set][v], a, net.m, c["tr"])
            assert sum(W) == 0
            continue
        assert b != a and b in members[net.set][v]
        assert T.weights_of([b], a, net.m, c["tr"])[0][0] > 0
    assert int(got["counts"].sum()) == len(flagged)
    assert np.array_equal(got["infected_row"] >= 0, c["nu"] == 1)
    assert (got["infector"][c["nu"] == 0] == T.NEVER).all()
    assert int(got["unresolved"].sum()) == int((got["infector"] == T.UNRESOLVED).sum())


def test_general_inputs_every_choice_is_a_possible_one_and_launches_agree(device):
    c = general_case()
    h = Harness(c["world"], c["tables"], device, "tiled", c["cum"])
    got = h.record(ACTIVE, c["nu"], c["s0"], c["stage"], c["tr"], day_type=1, row=1, seed=21, step=8)
    assert got["err"] == 0
    nets = h.nets(ACTIVE, c["stage"], 1)
    check_every_choice(h, c, got, nets, 1)
    assert (got["infector"] >= 0).sum() > 50 and (got["infector"] == T.UNRESOLVED).sum() > 0
    print("infectors drawn:", int((got["infector"] >= 0).sum()), "unresolved:", int(got["unresolved"].sum()),
          "nobody transmitted:", int((got["infector"] == T.NOBODY).sum()))
    # a second launch of the same step writes the same tree
    h2 = Harness(c["world"], c["tables"], device, "tiled", c["cum"])
    again = h2.record(ACTIVE, c["nu"], c["s0"], c["stage"], c["tr"], day_type=1, row=1, seed=21, step=8)
    assert all(again[k].tobytes() == got[k].tobytes() for k in PER_AGENT + ("counts", "unresolved"))


def test_renumbering_the_other_agents_gives_the_same_tree(device):
    """The draw is keyed by the infected agent's id, so an infected agent that is renumbered draws anew; the agents who
    are NOT newly infected - every possible infector among them - are renumbered at random here (the COO order of every
    set stays), which moves them to other lanes, waves and workgroups of the walk: the tree is the same, name for name."""
    c = general_case()
    A, world, nu = c["A"], c["world"], c["nu"]
    h = Harness(world, c["tables"], device, "tiled", c["cum"])
    once = h.record(ACTIVE, nu, c["s0"], c["stage"], c["tr"], day_type=1, seed=21, step=8)
    rng = np.random.default_rng(99)
    perm = np.arange(A)                           # new id of agent a: perm[a]
    others = np.nonzero(nu == 0)[0]
    perm[others] = others[rng.permutation(len(others))]
    inverse = np.argsort(perm)
    moved = dict(world, age=world["age"][inverse], sex=world["sex"][inverse], edge_sets={
        s: dict(es, agent=torch.from_numpy(perm)[es["agent"]]) for s, es in world["edge_sets"].items()})
    h2 = Harness(moved, c["tables"], device, "tiled", c["cum"])
    again = h2.record(ACTIVE, nu[inverse], c["s0"][inverse], c["stage"][inverse], c["tr"][inverse], day_type=1, seed=21,
                      step=8)
    assert np.array_equal(nu[inverse], nu)
    named = np.where(once["infector"] >= 0, perm[np.maximum(once["infector"], 0)], once["infector"])
    assert np.array_equal(again["infector"], named) and (once["infector"] >= 0).sum() > 50
    assert (named != once["infector"]).sum() > 20
    for k in ("via", "venue", "infected_row", "counts", "unresolved"):
        assert np.array_equal(again[k], once[k]), k


# ---- 3. bad input ----------------------------------------------------------------------------------------------------------
def test_bad_values_and_rows_are_skipped_and_reported(device):
    A = 257
    world, tables = make_world(A)
    rng = np.random.default_rng(9)
    cum = draw_cum(world, rng)
    s0, stage = state(A, rng)
    tr = transmissions(A, rng)
    nu = (rng.random(A) < 0.5).astype(np.float32)
    # a new_infected of 2 or NaN: the agent is skipped, the others get what they get without it
    at = np.nonzero(nu == 1)[0][:2]
    bad_nu, keep_nu = nu.copy(), nu.copy()
    bad_nu[at[0]], bad_nu[at[1]] = 2.0, np.nan
    keep_nu[at] = 0.0
    h = Harness(world, tables, device, "tiled", cum)
    got = h.record(ACTIVE, bad_nu, s0, stage, tr)
    assert got["err"] == N.GJ_LOC_ERR_VALUE
    with pytest.raises(InfectionTreeError, match="neither 0 nor 1"):
        h.tree.check()
    h.tree.check()                                                                 # raised once
    h2 = Harness(world, tables, device, "tiled", cum)
    only = h2.record(ACTIVE, keep_nu, s0, stage, tr)
    assert only["err"] == 0 and all(np.array_equal(got[k], only[k]) for k in PER_AGENT + ("counts", "unresolved"))
    assert (got["infector"][at] == T.NEVER).all() and (got["infected_row"][at] == -1).all()
    # a saturated weight (m * transmission >= 2^10) is taken at 2^46 and reported
    big = tr.copy()
    big[tr > 0] = 2048.0
    h3 = Harness(world, tables, device, "tiled", cum)
    got = h3.record(ACTIVE, nu, s0, None, big)
    want = h3.restated(None, ACTIVE, nu, s0, None, big, 0, 0, 1, 0)
    assert got["err"] == want["err"] == N.GJ_LOC_ERR_VALUE and same(got, want)
    # rows outside their set - an agent's row pointer, a venue id, a venue's row pointer, a member: skipped and reported,
    # nothing written out of bounds
    hr = Harness(world, tables, device, "tiled", cum)
    plan = hr.eng.plan
    plan.location_rows(edges_of(world))
    plan.venue_rows(edges_of(world))
    first = plan.host.set_index["household"]
    rowptr, venue = plan._location_rows_keep[first]
    v_rowptr, v_agent = plan._venue_rows_keep[first]
    assert plan._venue_rows[first].v_rowptr == v_rowptr.data_ptr()
    ones = np.ones(A, np.float32)
    clean = hr.record(ACTIVE, ones, s0, stage, tr)
    assert clean["err"] == 0
    v_agent[::5] = A + 3
    v_agent[1::7] = -2
    v_rowptr[3] = v_rowptr[-1] + 100000
    got = hr.record(ACTIVE, ones, s0, stage, tr, row=1)
    assert got["err"] == N.GJ_LOC_ERR_ROWS
    assert ((got["infector"] >= -3) & (got["infector"] < A)).all()
    hr.tree.err.zero_()
    rowptr[5] = -3
    rowptr[40] = rowptr[-1] + 100000
    venue[int(rowptr[100].item())] = plan.host.sets[first].n_venues + 7
    got = hr.record(ACTIVE, ones, s0, stage, tr, row=2)
    assert got["err"] & N.GJ_LOC_ERR_ROWS
    with pytest.raises(InfectionTreeError, match="outside its edge set"):
        hr.tree.check()
    assert int(got["counts"][2].sum()) == A


@pytest.mark.parametrize("layout", ["csr", "tiled"])
def test_argument_errors_are_returned_before_any_device_work(device, layout):
    A = 65
    world, tables = make_world(A)
    rng = np.random.default_rng(3)
    h = Harness(world, tables, device, layout, draw_cum(world, rng))
    plan, lib, t = h.eng.plan, N.load(), h.tree
    ones = torch.ones(A, device=device)
    n = len(ACTIVE)
    cols = (C.c_int32 * n)(*range(n))
    p, pq = h.params(ACTIVE, None), h.params(ACTIVE, np.ones(A, np.float32))
    good = dict(plan=C.byref(plan.c), params=C.byref(p), rows=plan.location_rows(edges_of(world)),
                venue_rows=plan.venue_rows(edges_of(world)), nu=N.ptr(ones), s0=N.ptr(ones), stage=None, tr=N.ptr(ones),
                cols=cols, n_cols=len(COLUMNS), background=n, seed=1, step=2, offset=0, infector=N.ptr(t.infector),
                via=N.ptr(t.via), venue=N.ptr(t.venue), row_of=N.ptr(t.infected_row), row=3, counts=N.ptr(t.counts[3]),
                unresolved=N.ptr(t.unresolved[3:]), err=N.ptr(t.err))

    def call(**change):
        a = dict(good, **change)
        return lib.gj_infection_tree(a["plan"], a["params"], a["rows"], a["venue_rows"], a["nu"], a["s0"], a["stage"],
                                     a["tr"], a["cols"], a["n_cols"], a["background"], a["seed"], a["step"], a["offset"],
                                     a["infector"], a["via"], a["venue"], a["row_of"], a["row"], a["counts"],
                                     a["unresolved"], a["err"], N.current_stream())

    E_NULL, E_RANGE = -1, -2
    for name in ("plan", "params", "rows", "venue_rows", "nu", "s0", "tr", "cols", "infector", "via", "venue", "row_of",
                 "counts", "unresolved", "err"):
        assert call(**{name: None}) == E_NULL, name
    assert call(params=C.byref(pq)) == E_NULL                                      # quarantine without a stage
    half = (N.VenueRows * N.GJ_MAX_SETS)()
    for i in range(N.GJ_MAX_SETS):
        half[i].v_rowptr = good["venue_rows"][i].v_rowptr
    assert call(venue_rows=half) == E_NULL                                         # row pointers without members
    for change in (dict(n_cols=0), dict(n_cols=N.GJ_LOC_MAX_COLS + 1), dict(background=-1), dict(background=len(COLUMNS)),
                   dict(cols=(C.c_int32 * n)(0, 1, len(COLUMNS), 2, 3)), dict(offset=-1), dict(offset=(1 << 31) - A)):
        assert call(**change) == E_RANGE, change
    bad = h.params(ACTIVE, None)
    bad.n_nets = N.GJ_MAX_NETS + 1
    assert call(params=C.byref(bad)) == E_RANGE
    h.intact()
    assert int(t.err.item()) == 0 and bool((t.infector == -1).all()) and not t.counts.any() and not t.unresolved.any()
    # ... and the good call goes through; a set without venue rows leaves its infections unresolved
    assert call() == 0 and call(offset=(1 << 31) - 1 - A) == 0
    h.intact()
    assert bool((t.infected_row == 3).all()) and int(t.counts[3].sum()) == 2 * A
    none = (N.VenueRows * N.GJ_MAX_SETS)()
    t.reset(ROWS)
    assert call(venue_rows=none, infector=N.ptr(t.infector), via=N.ptr(t.via), venue=N.ptr(t.venue),
                row_of=N.ptr(t.infected_row), counts=N.ptr(t.counts[3]), unresolved=N.ptr(t.unresolved[3:])) == 0
    torch.cuda.synchronize()
    assert not bool((t.infector >= 0).any()) and int(t.unresolved[3]) == int((t.infector == T.UNRESOLVED).sum()) > 0


def test_an_empty_world_launches_nothing(device):
    lib = N.load()
    plan, p = N.Plan(), N.StepParams()
    out = torch.full((2,), -777777, dtype=torch.int32, device=device)
    big = torch.full((2,), -(1 << 40), dtype=torch.int64, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    one = torch.ones(1, device=device)
    assert lib.gj_infection_tree(C.byref(plan), C.byref(p), None, None, N.ptr(one), N.ptr(one), None, None, None, 2, 1, 0,
                                 0, 0, N.ptr(out), N.ptr(out), N.ptr(out), N.ptr(out), 0, N.ptr(big), N.ptr(big),
                                 N.ptr(err), N.current_stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == -777777).all()) and bool((big == -(1 << 40)).all()) and int(err.item()) == 0
