"""GPU: gj_infector_scatter / gj_infector_gather / gj_infector_clear against the numpy restatement
(tests/gj_infector_ref.py), on the worlds of tests/test_gpu_location_stats.py.  The tests fill the plan's ``cum``
workspaces and the transmissions themselves, so no step needs to run.

Bit-equal case: ``cum``, the leisure tables and ``s0`` are multiples of 2^-8 in [0, 4] - the argument of
test_gpu_location_stats.py: every fp64 product and sum is exact in any order, only the correctly rounded divisions round
- so ``U``, ``unattributed`` and ``infected_row`` must equal the restatement bit for bit.

General inputs: the sum of ``U`` is exact; a cell is within (edges of new infections touching the venue + n_nets) units of
the restatement: one unit of floor per edge, and a remainder that a different T - the terms reassociate - can move by as
much.  ``caused`` is within 1e-12 relative (non-negative terms, fewer than 4096 of them per set: 4096 * 2^-53 = 4.5e-13),
the group sums within one unit per infectious agent of the group (one llrint each)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gj_infector_ref as I
from grad_june_amd import _native as N
from grad_june_amd.groups import InfectorError, InfectorStats
from test_gpu_location_stats import (ACTIVE, CASES, GUARD, SENTINEL, THRESHOLD, draw_cum, edges_of, engine_and_cum,
                                     generic_values, make_world, state)

pytestmark = pytest.mark.gpu

BETAS = {"company": 0.75, "pub": 0.5, "gym": 1.25, "care_visit": 2.0, "household": 1.5, "school": 1.0}
FEW = ["company", "pub", "care_visit", "household"]
ROWS = 8


def guarded(n, dtype, fill, device):
    """(buffer with GUARD sentinels on both sides, the view between them filled with ``fill``)."""
    sentinel = SENTINEL if dtype != torch.int32 else -777777
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=device)
    view = buf[GUARD: GUARD + n]
    view.fill_(fill)
    return buf, view, sentinel


class Harness:
    """An engine with its ``cum`` filled, ``U`` between sentinels, and an InfectorStats whose outputs sit between
    sentinels too."""

    def __init__(self, world, tables, device, layout, cum, labels=None, G=1):
        self.world, self.tables, self.device, self.cum, self.A = world, tables, device, cum, world["n_agents"]
        self.eng = engine_and_cum(world, tables, device, layout, cum)
        plan = self.eng.plan
        self.guards = []
        units = []
        for i, s in enumerate(plan.host.sets):
            shape = (max(1, s.n_venues), int(plan.c.sets[i].cum_stride))
            buf, view, sentinel = guarded(shape[0] * shape[1], torch.int64, 0, device)
            self.guards.append((buf, sentinel))
            units.append(view.view(shape))
        plan._infector_units = (units, (C.c_void_p * N.GJ_MAX_SETS)(*[u.data_ptr() for u in units]))
        self.pc = {s.name: plan.keep[i]["v_pc"].cpu().numpy() for i, s in enumerate(plan.host.sets)}
        labellings = {} if labels is None else {"g": (torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)), G)}
        self.key = None if labels is None else "g"
        self.stats = st = InfectorStats(self.A, labellings, device=device, n_rows=ROWS)
        for name, dtype, fill in (("caused", torch.float64, 0), ("infected_row", torch.int32, -1),
                                  ("unattributed", torch.int64, 0)):
            buf, view, sentinel = guarded(getattr(st, name).numel(), dtype, fill, device)
            self.guards.append((buf, sentinel))
            setattr(st, name, view)
        for key in list(st.out):
            buf, view, sentinel = guarded(st.out[key].numel(), torch.int64, 0, device)
            self.guards.append((buf, sentinel))
            st.out[key] = view.view(ROWS, -1)

    def params(self, active, stage, day_type=0):
        return self.eng.params(now=1.0, delta_time=1.0, day_type=day_type, active=active, betas=BETAS,
                               has_quarantine=stage is not None, q_threshold=THRESHOLD)

    def dev(self, a, dt=np.float32):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)

    def intact(self):
        torch.cuda.synchronize()
        for buf, sentinel in self.guards:
            assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[-GUARD:] == sentinel).all()), "wrote outside an output"

    def units(self):
        plan = self.eng.plan
        return {s.name: plan.infector_units()[0][i][: s.n_venues].cpu().numpy() for i, s in enumerate(plan.host.sets)}

    def set_units(self, units):
        plan = self.eng.plan
        for i, s in enumerate(plan.host.sets):
            plan.infector_units()[0][i][: s.n_venues].copy_(torch.from_numpy(units[s.name]))

    def scatter(self, active, nu, s0, stage, day_type=0, row=0):
        self.stats.scatter(self.eng.plan, self.params(active, stage, day_type), self.dev(nu), self.dev(s0), self.dev(stage),
                           row=row, edges=edges_of(self.world))
        self.intact()
        return self.units(), int(self.stats.unattributed.sum().item()), int(self.stats.err.item())

    def gather(self, active, tr, stage, day_type=0):
        self.stats.gather(self.eng.plan, self.params(active, stage, day_type), self.dev(tr), self.dev(stage),
                          edges=edges_of(self.world))
        self.intact()
        return (self.stats.caused.cpu().numpy(), {k: v[0].cpu().numpy() for k, v in self.stats.out.items()},
                int(self.stats.err.item()))

    def nets(self, active, stage, day_type=0):
        q = None if stage is None else (stage < np.float32(THRESHOLD)).astype(np.float64)
        return I.step_nets(self.world, self.tables, active, BETAS, day_type, q)

    def edges(self):
        return {s: (a.numpy(), v.numpy()) for s, (a, v) in edges_of(self.world).items()}


def same_units(got, want):
    return all(np.array_equal(got[s], want[s]) for s in want)


# ---- 1. bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,layout", CASES)
def test_scatter_equals_the_restatement_bit_for_bit(device, A, layout):
    world, tables = make_world(A)
    rng = np.random.default_rng(A * 13 + 1)
    cum = draw_cum(world, rng)
    h = Harness(world, tables, device, layout, cum)
    s0, stage = state(A, rng)
    draws = {"some": (rng.random(A) < 0.3).astype(np.float32), "none": np.zeros(A, np.float32),
             "all": np.ones(A, np.float32)}
    lost_so_far, row_of, lost_in = 0, np.full(A, -1, np.int32), np.zeros(ROWS, np.int64)
    for row, (day_type, what) in enumerate([(0, "some"), (1, "all"), (0, "none"), (1, "some"), (0, "all")]):
        nu = draws[what]
        want, lost, want_err, _ = I.scatter(h.nets(ACTIVE, stage, day_type), h.edges(), cum, s0, nu, A)
        got, got_lost, err = h.scatter(ACTIVE, nu, s0, stage, day_type, row=row)
        lost_so_far += lost
        lost_in[row] = lost
        row_of[nu == 1] = row
        assert err == want_err == 0
        assert same_units(got, want), (what, day_type)
        assert got_lost == lost_so_far and np.array_equal(h.stats.unattributed.cpu().numpy(), lost_in)
        assert sum(int(u.sum()) for u in got.values()) == I.U * (int(nu.sum()) - lost)
        assert np.array_equal(h.stats.infected_row.cpu().numpy(), row_of)
        h.stats.clear(h.eng.plan)
        assert not any(u.any() for u in h.units().values())
    assert A == 1 or lost_so_far > 0
    # fewer networks (care_visit moves to column 1 of its set), no quarantine; and no network at all (the seeding step)
    want, lost, _, _ = I.scatter(h.nets(FEW, None), h.edges(), cum, s0, draws["all"], A)
    got, got_lost, err = h.scatter(FEW, draws["all"], s0, None)
    assert err == 0 and same_units(got, want) and got_lost == lost_so_far + lost
    h.stats.clear(h.eng.plan)
    row_of[:] = 0
    got, got_lost, err = h.scatter([], draws["some"], s0, stage, row=7)
    assert err == 0 and not any(u.any() for u in got.values())
    assert got_lost == lost_so_far + lost + int(draws["some"].sum())
    row_of[draws["some"] == 1] = 7
    assert np.array_equal(h.stats.infected_row.cpu().numpy(), row_of)


# ---- 2. general inputs -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general_case():
    """The 1000-agent world with generic sums - saturated venues, a NaN and a negative sum - and the restatement's pass 1."""
    A = 1000
    world, tables = make_world(A, seed=1)
    rng = np.random.default_rng(31)
    cum = draw_cum(world, rng, generic_values)
    cum["company"][:60, 0] = 1e30
    cum["household"][0, 0], cum["household"][1, 0] = np.nan, -1e6
    cum["leisure"][0, 1], cum["leisure"][1, 2] = np.nan, -1e6
    s0, stage = rng.random(A).astype(np.float32), rng.integers(1, 8, A).astype(np.float32)
    s0[rng.random(A) < 0.1] = 0.0
    nu = (rng.random(A) < 0.5).astype(np.float32)
    q = (stage < np.float32(THRESHOLD)).astype(np.float64)
    nets = I.step_nets(world, tables, ACTIVE, BETAS, 1, q)
    edges = {s: (a.numpy(), v.numpy()) for s, (a, v) in edges_of(world).items()}
    want = I.scatter(nets, edges, cum, s0, nu, A)
    return dict(A=A, world=world, tables=tables, cum=cum, s0=s0, stage=stage, nu=nu, want=want)


def test_scatter_on_general_inputs_sums_exactly_and_stays_within_the_floor_bound(device):
    c = general_case()
    want, lost, want_err, touched = c["want"]
    assert want_err == I.ERR_VALUE and lost > 0
    h = Harness(c["world"], c["tables"], device, "tiled", c["cum"])
    got, got_lost, err = h.scatter(ACTIVE, c["nu"], c["s0"], c["stage"], day_type=1)
    assert err == N.GJ_LOC_ERR_VALUE and got_lost == lost
    assert sum(int(u.sum()) for u in got.values()) == I.U * (int(c["nu"].sum()) - lost)      # exact
    worst = 0
    for s, u in got.items():
        diff = np.abs(u - want[s]).max(1)
        worst = max(worst, int(diff.max()))
        assert np.all(diff <= touched[s] + len(ACTIVE)), s
        assert (u >= 0).all() and not u[touched[s] == 0].any()
    print("largest deviation of a cell of U from the restatement, in units of 2^-30:", worst)
    with pytest.raises(InfectorError, match="NaN / negative"):
        h.stats.check()
    # 5. a second launch of the same step gives the same bits
    h.stats.clear(h.eng.plan)
    again, _, _ = h.scatter(ACTIVE, c["nu"], c["s0"], c["stage"], day_type=1)
    assert all(again[s].tobytes() == got[s].tobytes() for s in got)
    # clearing by the walk zeroes what the step touched - which is all that is not zero
    h.stats.clear_by = "walk"
    h.stats.clear(h.eng.plan, h.dev(c["nu"]))
    h.intact()
    assert not any(u.any() for u in h.units().values())


# ---- 3. gather -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gather_case(A, exact):
    world, tables = make_world(A)
    rng = np.random.default_rng(A * 7 + 3)
    cum = draw_cum(world, rng) if exact else {s: v + np.float32(1e-4) for s, v in draw_cum(world, rng, generic_values).items()}
    s0, stage = state(A, rng)
    nu = (rng.random(A) < 0.4).astype(np.float32) if A > 1 else np.ones(1, np.float32)
    q = (stage < np.float32(THRESHOLD)).astype(np.float64)
    edges = {s: (a.numpy(), v.numpy()) for s, (a, v) in edges_of(world).items()}
    nets = I.step_nets(world, tables, ACTIVE, BETAS, 1, q)
    units, _, _, _ = I.scatter(nets, edges, cum, s0, nu, A)
    tr = (rng.random(A) * rng.choice([0.0, 0.0, 1e-3, 1.0], A)).astype(np.float32)
    tr[0] = 0.5                                                        # the agent with the long row transmits
    return dict(A=A, world=world, tables=tables, cum=cum, stage=stage, units=units, tr=tr, nets=nets, edges=edges)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("G", [1, 3, 5000])
@pytest.mark.parametrize("A,layout", CASES)
def test_gather_agrees_with_the_restatement(device, A, layout, G, sparse):
    """``sparse``: every twentieth agent transmits - fewer than the 16 of 256 from which the kernel takes a round one
    agent per lane; otherwise about half of them do, and it does."""
    c = gather_case(A, exact=A in (1, 64, 257))
    if sparse:
        c = dict(c, tr=np.where(np.arange(A) % 20 == 0, np.maximum(c["tr"], np.float32(0.25)), np.float32(0)))
        assert (c["tr"].reshape(-1)[:256] > 0).sum() < 16
    rng = np.random.default_rng(A + G)
    group = None if G == 1 else rng.integers(0, G, A)
    h = Harness(c["world"], c["tables"], device, layout, c["cum"], group, G)
    assert (G <= N.GJ_LOC_LDS_BINS) == (G < 5000)                                 # both accumulation regimes
    h.set_units(c["units"])
    base = np.where(c["tr"] == 0, rng.random(A), 0.0)                             # something to leave untouched
    h.stats.caused.copy_(torch.from_numpy(base))
    want, want_out, want_err = I.gather(c["nets"], c["edges"], c["cum"], h.pc, c["units"], c["tr"], A, group, G)
    assert want_err == 0 and (want.sum() > 0 or A == 1 or (sparse and A < 257))     # (a handful of transmitters)
    caused, out, err = h.gather(ACTIVE, c["tr"], c["stage"], day_type=1)
    assert err == 0
    assert np.array_equal(caused[c["tr"] == 0], base[c["tr"] == 0])                # untouched
    credit = np.where(c["tr"] == 0, 0.0, caused)
    assert np.all(np.abs(credit - want) <= 1e-12 * want)
    g = np.zeros(A, np.int64) if group is None else group
    infectious = np.bincount(g[c["tr"] > 0], minlength=G)
    assert np.all(np.abs(out[h.key] - np.array(want_out, dtype=np.int64)) <= infectious)
    assert int(out[None][0]) == int(out[h.key].sum())                             # the same credits, the same llrint
    assert abs(int(out[None][0]) - int(np.sum(want_out))) <= infectious.sum()
    # a second launch adds: to caused once more, to the group sums the same integers
    caused2, out2, _ = h.gather(ACTIVE, c["tr"], c["stage"], day_type=1)
    assert np.array_equal(np.where(c["tr"] == 0, 0.0, caused2), 2 * credit)        # 5. the same bits twice
    assert np.array_equal(caused2[c["tr"] == 0], base[c["tr"] == 0])
    assert np.array_equal(out2[h.key], 2 * out[h.key])
    assert same_units(h.units(), c["units"])                                       # U is read only


# ---- 4. refusals and error bits -------------------------------------------------------------------------------------------
def test_bad_labels_values_and_rows_are_skipped_and_reported(device):
    A, G = 257, 3
    c = gather_case(A, exact=False)
    rng = np.random.default_rng(9)
    group = rng.integers(0, G, A)
    nu = (rng.random(A) < 0.5).astype(np.float32)
    s0 = np.ones(A, np.float32)
    # a new_infected of 2 or NaN: the agent is skipped, the others are scattered as before
    h = Harness(c["world"], c["tables"], device, "tiled", c["cum"], group, G)
    at = np.nonzero(nu == 1)[0][:2]
    bad_nu, keep_nu = nu.copy(), nu.copy()
    bad_nu[at[0]], bad_nu[at[1]] = 2.0, np.nan
    keep_nu[at] = 0.0
    got, lost, err = h.scatter(ACTIVE, bad_nu, s0, c["stage"])
    rows = h.stats.infected_row.cpu().numpy()
    assert err == N.GJ_LOC_ERR_VALUE and np.array_equal(rows == 0, keep_nu == 1)
    h.stats.clear(h.eng.plan)
    h.stats.err.zero_()
    only, only_lost, err = h.scatter(ACTIVE, keep_nu, s0, c["stage"])
    assert err == 0 and same_units(got, only) and only_lost == 2 * lost
    # a bad label: the agent is skipped - as if it did not transmit - and the label is never an index
    tr = c["tr"]
    b = int(np.nonzero(tr > 0)[0][3])
    bad_group = group.copy()
    bad_group[b] = G
    hb = Harness(c["world"], c["tables"], device, "tiled", c["cum"], bad_group, G)
    hb.set_units(only)
    caused, out, err = hb.gather(ACTIVE, tr, c["stage"])
    assert err == N.GJ_LOC_ERR_LABEL
    with pytest.raises(InfectorError, match="label"):
        hb.stats.check()
    hb.stats.check()                                                               # raised once
    quiet = tr.copy()
    quiet[b] = 0.0
    h.stats.caused.zero_()
    _, out_quiet, err = h.gather(ACTIVE, quiet, c["stage"])
    assert err == 0 and np.array_equal(out["g"], out_quiet["g"])
    # a row pointer outside its set, and a venue id outside it: skipped, reported, nothing written out of bounds
    hr = Harness(c["world"], c["tables"], device, "tiled", c["cum"], group, G)
    plan = hr.eng.plan
    plan.location_rows(edges_of(c["world"]))
    first = plan.host.set_index["household"]
    rowptr, venue = plan._location_rows_keep[first]
    assert plan._location_rows[first].a_rowptr == rowptr.data_ptr()
    rowptr[5] = -3
    rowptr[40] = rowptr[-1] + 100000
    venue[int(rowptr[100].item())] = plan.host.sets[first].n_venues + 7
    _, _, err = hr.scatter(ACTIVE, np.ones(A, np.float32), s0, c["stage"])
    assert err & N.GJ_LOC_ERR_ROWS
    hr.stats.err.zero_()
    _, _, err = hr.gather(ACTIVE, np.ones(A, np.float32), c["stage"])
    assert err & N.GJ_LOC_ERR_ROWS
    hr.stats.clear_by = "walk"
    hr.stats.clear(plan, hr.dev(np.ones(A, np.float32)))
    hr.intact()


@pytest.mark.parametrize("layout", ["csr", "tiled"])
def test_argument_errors_are_returned_before_any_device_work(device, layout):
    A = 65
    c = gather_case(A, exact=False)
    h = Harness(c["world"], c["tables"], device, layout, c["cum"], np.zeros(A, np.int64), 3)
    plan, lib = h.eng.plan, N.load()
    ones = torch.ones(A, device=device)
    rows, U = plan.location_rows(edges_of(c["world"])), plan.infector_units()[1]
    st = h.stats
    p = h.params(ACTIVE, None)
    pq = h.params(ACTIVE, np.ones(A, np.float32))
    good_s = dict(plan=C.byref(plan.c), params=C.byref(p), rows=rows, nu=N.ptr(ones), s0=N.ptr(ones), stage=None, U=U,
                  lost=N.ptr(st.unattributed), cohort=N.ptr(st.infected_row), value=5, err=N.ptr(st.err))
    good_g = dict(plan=C.byref(plan.c), params=C.byref(p), rows=rows, tr=N.ptr(ones), stage=None, U=U,
                  group=N.ptr(st.labels["g"]), G=3, caused=N.ptr(st.caused), out=N.ptr(st.out["g"]), err=N.ptr(st.err))

    def scatter(**change):
        a = dict(good_s, **change)
        return lib.gj_infector_scatter(a["plan"], a["params"], a["rows"], a["nu"], a["s0"], a["stage"], a["U"], a["lost"],
                                       a["cohort"], a["value"], a["err"], N.current_stream())

    def gather(**change):
        a = dict(good_g, **change)
        return lib.gj_infector_gather(a["plan"], a["params"], a["rows"], a["tr"], a["stage"], a["U"], a["group"], a["G"],
                                      a["caused"], a["out"], a["err"], N.current_stream())

    E_NULL, E_RANGE = -1, -2
    for name in ("plan", "params", "rows", "nu", "s0", "U", "lost", "err"):
        assert scatter(**{name: None}) == E_NULL, name
    for name in ("plan", "params", "rows", "tr", "U", "err"):
        assert gather(**{name: None}) == E_NULL, name
    assert gather(caused=None, out=None) == E_NULL
    assert scatter(params=C.byref(pq)) == E_NULL and gather(params=C.byref(pq)) == E_NULL      # quarantine without a stage
    holes = (C.c_void_p * N.GJ_MAX_SETS)()                                       # a set with rows and networks but no U
    assert scatter(U=holes) == E_NULL and gather(U=holes) == E_NULL
    for change in (dict(G=0), dict(G=N.GJ_MAX_GROUPS + 1), dict(group=None)):
        assert gather(**change) == E_RANGE, change
    bad = h.params(ACTIVE, None)
    bad.n_nets = N.GJ_MAX_NETS + 1
    assert scatter(params=C.byref(bad)) == E_RANGE and gather(params=C.byref(bad)) == E_RANGE
    for args in ((None, rows, N.ptr(ones), U), (C.byref(plan.c), None, N.ptr(ones), U),
                 (C.byref(plan.c), rows, None, U), (C.byref(plan.c), rows, N.ptr(ones), None)):
        assert lib.gj_infector_clear(*args, N.current_stream()) == E_NULL
    h.intact()
    assert int(st.err.item()) == 0 and not st.unattributed.any() and bool((st.infected_row == -1).all())
    assert not any(u.any() for u in h.units().values()) and not st.caused.any() and not st.out["g"].any()
    # ... and the good calls go through: cohort is optional, so are caused and out (one of them)
    assert scatter(cohort=None) == 0 and bool((st.infected_row == -1).all())
    assert scatter() == 0 and bool((st.infected_row == 5).all())
    assert gather(caused=None) == 0 and gather(out=None) == 0 and gather(group=None, G=1, out=N.ptr(st.out[None])) == 0
    assert lib.gj_infector_clear(C.byref(plan.c), rows, N.ptr(ones), U, N.current_stream()) == 0
    h.intact()
    assert not any(u.any() for u in h.units().values())


def test_an_empty_world_launches_nothing(device):
    lib = N.load()
    plan, p = N.Plan(), N.StepParams()
    out = torch.full((2,), SENTINEL, dtype=torch.int64, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    one = torch.ones(1, device=device)
    assert lib.gj_infector_scatter(C.byref(plan), C.byref(p), None, N.ptr(one), N.ptr(one), None, None, N.ptr(out), None,
                                   0, N.ptr(err), N.current_stream()) == 0
    assert lib.gj_infector_gather(C.byref(plan), C.byref(p), None, N.ptr(one), None, None, None, 1, None, N.ptr(out),
                                  N.ptr(err), N.current_stream()) == 0
    assert lib.gj_infector_clear(C.byref(plan), None, N.ptr(one), None, N.current_stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and int(err.item()) == 0
