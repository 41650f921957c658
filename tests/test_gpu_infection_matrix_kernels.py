"""GPU: gj_infection_matrix_scatter / gj_infection_matrix_gather / gj_infection_matrix_clear against the numpy restatement
(tests/gj_matrix_ref.py), with the harness of tests/test_gpu_infector_stats.py on the worlds of
tests/test_gpu_location_stats.py.  The tests fill ``cum``, ``U`` / ``UG`` and the transmissions themselves, so no step
needs to run; every output sits between sentinels.

Scatter: on the exact-valued inputs (multiples of 2^-8: the argument of test_gpu_location_stats.py) ``UG`` and the
unattributed counts equal the restatement bit for bit; on generic inputs ``UG`` sums over the groups to the device's own
``U`` in every cell - both launches form the same t_i, T and floors - and the totals per group are exact.

Gather: ``out`` equals the restatement's integers EXACTLY, on exact and on generic inputs.  Every term is
UG / 2^30 * (beta * pc) * (m * tr) / cum * 2^30: a chain of correctly rounded fp64 products and quotients in a fixed order
with no addition that could be contracted into a product, then one round-to-nearest-even; the sums are integers.

Marginals: the sum over g' of out[g][g'] is within (non-zero terms of group g) / 2 + (infectious agents of g) / 2 units of
gj_infector_gather's out[g] on the same inputs: one half-unit rounding per term against one per agent."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gj_infector_ref as I
import gj_matrix_ref as M
from grad_june_amd import _native as N
from grad_june_amd.groups import InfectorError, InfectorStats
from test_gpu_infector_stats import BETAS, ROWS, Harness, guarded, same_units
from test_gpu_location_stats import (ACTIVE, CASES, SENTINEL, THRESHOLD, draw_cum, edges_of, generic_values, make_world,
                                     state)

pytestmark = pytest.mark.gpu

GROUPS = [1, 3, N.GJ_MATRIX_MAX_GROUPS]


class MatrixHarness(Harness):
    """The infector harness with a labelling "g" that has a matrix: ``UG`` between sentinels on the plan, the statistics
    object's ``matrix`` and ``unattributed_by`` between sentinels too."""

    def __init__(self, world, tables, device, layout, cum, labels, G, matrix_clear="walk"):
        labels = np.zeros(world["n_agents"], np.int64) if labels is None else labels
        super().__init__(world, tables, device, layout, cum, labels, G)
        plan, self.G = self.eng.plan, G
        by_group = []
        for i, s in enumerate(plan.host.sets):
            shape = (max(1, s.n_venues), int(plan.c.sets[i].cum_stride), G)
            buf, view, sentinel = guarded(shape[0] * shape[1] * G, torch.int64, 0, device)
            self.guards.append((buf, sentinel))
            by_group.append(view.view(shape))
        assert getattr(plan, "_infection_matrix_units", None) is None
        plan._infection_matrix_units = {"g": (by_group, (C.c_void_p * N.GJ_MAX_SETS)(*[u.data_ptr() for u in by_group]))}
        old = self.stats
        self.stats = st = InfectorStats(self.A, {"g": (old.labels["g"], G)}, device=device, n_rows=ROWS, matrices=["g"],
                                        matrix_clear=matrix_clear)
        for name in ("caused", "infected_row", "unattributed", "out"):                 # (already between sentinels)
            setattr(st, name, getattr(old, name))
        for name in ("matrix", "unattributed_by"):
            buf, view, sentinel = guarded(getattr(st, name)["g"].numel(), torch.int64, 0, device)
            self.guards.append((buf, sentinel))
            getattr(st, name)["g"] = view.view(getattr(st, name)["g"].shape)

    def by_group(self):
        plan = self.eng.plan
        return {s.name: plan.infection_matrix_units("g", self.G)[0][i][: s.n_venues].cpu().numpy()
                for i, s in enumerate(plan.host.sets)}

    def set_by_group(self, UG):
        """``UG`` on the plan, and its sums over the groups as ``U``."""
        plan = self.eng.plan
        for i, s in enumerate(plan.host.sets):
            plan.infection_matrix_units("g", self.G)[0][i][: s.n_venues].copy_(torch.from_numpy(UG[s.name]))
        self.set_units({s: u.sum(-1) for s, u in UG.items()})

    def matrix_scatter(self, active, nu, s0, stage, day_type=0, row=0):
        self.stats.matrix_scatter(self.eng.plan, self.params(active, stage, day_type), self.dev(nu), self.dev(s0),
                                  self.dev(stage), row=row, edges=edges_of(self.world))
        self.intact()
        return self.by_group(), self.stats.unattributed_by["g"].cpu().numpy(), int(self.stats.err.item())

    def matrix_gather(self, active, tr, stage, day_type=0, row=0):
        self.stats.matrix_gather(self.eng.plan, self.params(active, stage, day_type), self.dev(tr), self.dev(stage), row=row,
                                 edges=edges_of(self.world))
        self.intact()
        return self.stats.matrix["g"][row].cpu().numpy(), int(self.stats.err.item())


def labels_for(A, G, seed=0):
    return np.random.default_rng(A * 31 + G + seed).integers(0, G, A)


# ---- 1. scatter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("A,layout", CASES)
def test_scatter_equals_the_restatement_bit_for_bit(device, A, layout, G):
    world, tables = make_world(A)
    rng = np.random.default_rng(A * 13 + 1)
    cum = draw_cum(world, rng)
    group = labels_for(A, G)
    h = MatrixHarness(world, tables, device, layout, cum, group, G)
    s0, stage = state(A, rng)
    draws = {"some": (rng.random(A) < 0.3).astype(np.float32), "all": np.ones(A, np.float32)}
    lost_in = np.zeros((ROWS, G), np.int64)
    for row, (day_type, what, clear) in enumerate([(0, "some", "walk"), (1, "all", "memset"), (1, "some", "walk")]):
        nu = draws[what]
        want, lost, want_err = M.scatter_by_group(h.nets(ACTIVE, stage, day_type), h.edges(), cum, s0, nu, A, group, G)
        got, got_lost, err = h.matrix_scatter(ACTIVE, nu, s0, stage, day_type, row=row)
        lost_in[row] = lost
        assert err == want_err == 0
        assert same_units(got, want), (what, day_type)
        assert np.array_equal(got_lost, lost_in)
        # the device's own U from the same inputs: UG sums to it cell by cell
        units, _, _ = h.scatter(ACTIVE, nu, s0, stage, day_type, row=row)
        assert all(np.array_equal(got[s].sum(-1), units[s]) for s in units)
        # both ways of clearing leave UG all zero (and the sentinels intact)
        h.stats.matrix_clear_by = clear
        h.stats.matrix_clear(h.eng.plan, h.dev(nu), edges=edges_of(world))
        h.stats.clear(h.eng.plan)
        h.intact()
        assert not any(u.any() for u in h.by_group().values()), clear
    assert A == 1 or lost_in.sum() > 0
    # no network at all (the seeding step): every infection is counted by its group, nothing is scattered
    cohorts = h.stats.infected_row.cpu().numpy().copy()
    got, got_lost, err = h.matrix_scatter([], draws["some"], s0, stage, row=7)
    assert err == 0 and not any(u.any() for u in got.values())
    assert np.array_equal(got_lost[7], np.bincount(group[draws["some"] == 1], minlength=G))
    assert np.array_equal(h.stats.infected_row.cpu().numpy(), cohorts) and (cohorts != 7).all()      # it writes no cohort


@functools.lru_cache(maxsize=None)
def general_case():
    """The 1000-agent world with generic sums - saturated venues, a NaN and a negative sum."""
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
    return dict(A=A, world=world, tables=tables, cum=cum, s0=s0, stage=stage, nu=nu)


@pytest.mark.parametrize("G", [3, N.GJ_MATRIX_MAX_GROUPS])
def test_scatter_on_general_inputs_sums_to_the_devices_own_units_exactly(device, G):
    c = general_case()
    A, group = c["A"], labels_for(c["A"], G)
    h = MatrixHarness(c["world"], c["tables"], device, "tiled", c["cum"], group, G)
    got, lost_by, err = h.matrix_scatter(ACTIVE, c["nu"], c["s0"], c["stage"], day_type=1)
    units, lost, err_units = h.scatter(ACTIVE, c["nu"], c["s0"], c["stage"], day_type=1)
    assert err == err_units == N.GJ_LOC_ERR_VALUE and lost > 0
    for s, u in units.items():                                                     # cell by cell, exactly
        assert (got[s] >= 0).all() and np.array_equal(got[s].sum(-1), u), s
    new = np.bincount(group[c["nu"] == 1], minlength=G)                            # the totals per group are exact
    for g in range(G):
        assert sum(int(u[:, :, g].sum()) for u in got.values()) + I.U * int(lost_by[0, g]) == I.U * int(new[g]), g
    assert int(lost_by[0].sum()) == lost
    with pytest.raises(InfectorError, match="NaN / negative"):
        h.stats.check()
    # a second launch of the same step gives the same bytes
    h.stats.matrix_clear(h.eng.plan, h.dev(c["nu"]))
    h.intact()
    assert not any(u.any() for u in h.by_group().values())
    again, _, _ = h.matrix_scatter(ACTIVE, c["nu"], c["s0"], c["stage"], day_type=1)
    assert all(again[s].tobytes() == got[s].tobytes() for s in got)
    h.stats.matrix_clear_by = "memset"
    h.stats.matrix_clear(h.eng.plan, h.dev(c["nu"]))
    h.intact()
    assert not any(u.any() for u in h.by_group().values())


# ---- 2. gather ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gather_case(A, G, exact):
    """A world, its sums, the restatement's ``UG`` of a step and transmissions for about half of the agents."""
    world, tables = make_world(A)
    rng = np.random.default_rng(A * 7 + 3)
    cum = draw_cum(world, rng) if exact else {s: v + np.float32(1e-4) for s, v in draw_cum(world, rng, generic_values).items()}
    s0, stage = state(A, rng)
    nu = (rng.random(A) < 0.4).astype(np.float32) if A > 1 else np.ones(1, np.float32)
    group = labels_for(A, G)
    q = (stage < np.float32(THRESHOLD)).astype(np.float64)
    edges = {s: (a.numpy(), v.numpy()) for s, (a, v) in edges_of(world).items()}
    nets = I.step_nets(world, tables, ACTIVE, BETAS, 1, q)
    UG, _, _ = M.scatter_by_group(nets, edges, cum, s0, nu, A, group, G)
    tr = (rng.random(A) * rng.choice([0.0, 0.0, 1e-3, 1.0], A)).astype(np.float32)
    tr[0] = 0.5                                                        # the agent with the long row transmits
    return dict(A=A, G=G, world=world, tables=tables, cum=cum, stage=stage, UG=UG, tr=tr, nets=nets, edges=edges,
                group=group)


def sparse_transmissions(c):
    """Every twentieth agent transmits: fewer than the 16 of 256 from which the kernel takes a round one agent per lane."""
    tr = np.where(np.arange(c["A"]) % 20 == 0, np.maximum(c["tr"], np.float32(0.25)), np.float32(0))
    assert (tr[:256] > 0).sum() < 16
    return tr


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("A,layout", CASES)
def test_gather_equals_the_restatement_exactly(device, A, layout, G, sparse):
    c = gather_case(A, G, exact=A in (1, 64, 257))
    tr = sparse_transmissions(c) if sparse else c["tr"]
    h = MatrixHarness(c["world"], c["tables"], device, layout, c["cum"], c["group"], G)
    h.set_by_group(c["UG"])
    units = h.units()
    want = np.array(M.matrix(c["nets"], c["edges"], c["cum"], h.pc, c["UG"], tr, A, c["group"], G), dtype=np.int64)
    assert want.sum() > 0 or A == 1 or (sparse and A < 257)
    got, err = h.matrix_gather(ACTIVE, tr, c["stage"], day_type=1)
    assert err == 0
    assert np.array_equal(got, want)
    # a second launch doubles out; U and UG are read only; caused and the group sums are not written
    again, _ = h.matrix_gather(ACTIVE, tr, c["stage"], day_type=1)
    assert np.array_equal(again, 2 * want)
    assert same_units(h.by_group(), c["UG"]) and same_units(h.units(), units)
    assert not h.stats.caused.any() and not h.stats.out["g"].any() and not h.stats.matrix["g"][1:].any()
    # the marginals against gj_infector_gather on the same inputs: one rounding per term against one per agent
    _, out, err = h.gather(ACTIVE, tr, c["stage"], day_type=1)
    assert err == 0
    terms, infectious = np.zeros(G, np.int64), np.bincount(c["group"][tr > 0], minlength=G)
    for _, g, _, value in M.matrix_terms(c["nets"], c["edges"], c["cum"], h.pc, c["UG"], tr, A, c["group"], G):
        terms[g] += value != 0
    assert np.all(2 * np.abs(got.sum(1) - out["g"]) <= terms + infectious)


@pytest.mark.parametrize("A,G", [(257, 3), (1000, N.GJ_MATRIX_MAX_GROUPS)])
def test_both_forms_of_the_walk_give_the_same_integers(device, A, G):
    """The agents without an edge (a % 7 == 6) transmit too: a seventh of every round, so the kernel takes it one agent
    per lane - and they add no term, so ``out`` must be what the groups of lanes gave."""
    c = gather_case(A, G, exact=False)
    sparse = sparse_transmissions(c)
    dense = np.where(np.arange(A) % 7 == 6, np.float32(0.5), sparse)
    assert (dense[:256] > 0).sum() >= 16 and not np.isin(np.nonzero(np.arange(A) % 7 == 6)[0], c["edges"]["household"][0]).any()
    out = []
    for tr in (sparse, dense):
        h = MatrixHarness(c["world"], c["tables"], device, "tiled", c["cum"], c["group"], G)
        h.set_by_group(c["UG"])
        got, err = h.matrix_gather(ACTIVE, tr, c["stage"], day_type=1)
        assert err == 0 and got.sum() > 0
        out.append(got)
    assert out[0].tobytes() == out[1].tobytes()


def permuted(world, order):
    """The world with agent a renamed order[a]; the COO order of the edges stays."""
    to = torch.from_numpy(order)
    sets = {s: dict(es, agent=to[es["agent"]]) for s, es in world["edge_sets"].items()}
    inverse = torch.from_numpy(np.argsort(order))
    return dict(world, age=world["age"][inverse], sex=world["sex"][inverse], edge_sets=sets)


@pytest.mark.parametrize("A,G", [(257, 3), (1000, N.GJ_MATRIX_MAX_GROUPS)])
def test_permuting_the_agents_changes_no_bit(device, A, G):
    c = gather_case(A, G, exact=False)
    order = np.random.default_rng(5).permutation(A)
    inverse = np.argsort(order)
    out = []
    for world, pick in ((c["world"], np.arange(A)), (permuted(c["world"], order), inverse)):
        h = MatrixHarness(world, c["tables"], device, "tiled", c["cum"], c["group"][pick], G)
        h.set_by_group(c["UG"])
        got, err = h.matrix_gather(ACTIVE, c["tr"][pick], c["stage"][pick], day_type=1)
        assert err == 0 and got.sum() > 0
        out.append(got)
    assert out[0].tobytes() == out[1].tobytes()


# ---- 3. refusals and error bits -----------------------------------------------------------------------------------------------
def test_bad_labels_values_and_rows_are_skipped_and_reported(device):
    A, G = 257, 3
    c = gather_case(A, G, exact=False)
    rng = np.random.default_rng(9)
    nu = (rng.random(A) < 0.5).astype(np.float32)
    s0 = np.ones(A, np.float32)
    # scatter: a bad label skips the infected agent - as if it were not infected - and is never an index
    a = int(np.nonzero(nu == 1)[0][2])
    bad_group, keep_nu = c["group"].copy(), nu.copy()
    bad_group[a], keep_nu[a] = G, 0.0
    hb = MatrixHarness(c["world"], c["tables"], device, "tiled", c["cum"], bad_group, G)
    got, lost, err = hb.matrix_scatter(ACTIVE, nu, s0, c["stage"])
    assert err == N.GJ_LOC_ERR_LABEL
    with pytest.raises(InfectorError, match="label"):
        hb.stats.check()
    h = MatrixHarness(c["world"], c["tables"], device, "tiled", c["cum"], c["group"], G)
    only, only_lost, err = h.matrix_scatter(ACTIVE, keep_nu, s0, c["stage"])
    assert err == 0 and same_units(got, only) and np.array_equal(lost, only_lost)
    # gather: a bad label skips the transmitting agent
    b = int(np.nonzero(c["tr"] > 0)[0][3])
    bad_group = c["group"].copy()
    bad_group[b] = -1
    hb = MatrixHarness(c["world"], c["tables"], device, "tiled", c["cum"], bad_group, G)
    hb.set_by_group(c["UG"])
    got, err = hb.matrix_gather(ACTIVE, c["tr"], c["stage"], day_type=1)
    assert err == N.GJ_LOC_ERR_LABEL
    quiet = c["tr"].copy()
    quiet[b] = 0.0
    h.set_by_group(c["UG"])
    want, err = h.matrix_gather(ACTIVE, quiet, c["stage"], day_type=1)
    assert err == 0 and np.array_equal(got, want)
    # a NaN cum under a cell with units: the pair is skipped and reported
    agent, venue = c["edges"]["household"]
    attended = np.bincount(venue[c["tr"][agent] > 0], minlength=len(c["cum"]["household"])) > 0
    v = int(np.nonzero((c["UG"]["household"].sum((1, 2)) > 0) & attended)[0][0])      # units there, and someone transmits
    nan_cum = {s: x.copy() for s, x in c["cum"].items()}
    nan_cum["household"][v, 0] = np.nan
    hn = MatrixHarness(c["world"], c["tables"], device, "tiled", nan_cum, c["group"], G)
    hn.set_by_group(c["UG"])
    got, err = hn.matrix_gather(ACTIVE, c["tr"], c["stage"], day_type=1)
    assert err == N.GJ_LOC_ERR_VALUE
    assert np.array_equal(got, np.array(M.matrix(c["nets"], c["edges"], nan_cum, hn.pc, c["UG"], c["tr"], A, c["group"], G)))
    # a row pointer outside its set, and a venue id outside it: skipped, reported, nothing written out of bounds
    hr = MatrixHarness(c["world"], c["tables"], device, "tiled", c["cum"], c["group"], G)
    plan = hr.eng.plan
    plan.location_rows(edges_of(c["world"]))
    first = plan.host.set_index["household"]
    rowptr, venue = plan._location_rows_keep[first]
    rowptr[5] = -3
    rowptr[40] = rowptr[-1] + 100000
    venue[int(rowptr[100].item())] = plan.host.sets[first].n_venues + 7
    _, _, err = hr.matrix_scatter(ACTIVE, np.ones(A, np.float32), s0, c["stage"])
    assert err & N.GJ_LOC_ERR_ROWS
    hr.stats.err.zero_()
    hr.set_by_group(c["UG"])
    _, err = hr.matrix_gather(ACTIVE, np.ones(A, np.float32), c["stage"])
    assert err & N.GJ_LOC_ERR_ROWS
    hr.stats.matrix_clear(plan, hr.dev(np.ones(A, np.float32)))
    hr.intact()


@pytest.mark.parametrize("layout", ["csr", "tiled"])
def test_argument_errors_are_returned_before_any_device_work(device, layout):
    A, G = 65, 3
    c = gather_case(A, G, exact=False)
    h = MatrixHarness(c["world"], c["tables"], device, layout, c["cum"], c["group"], G)
    plan, lib, st = h.eng.plan, N.load(), h.stats
    ones = torch.ones(A, device=device)
    rows, U = plan.location_rows(edges_of(c["world"])), plan.infector_units()[1]
    UG = plan.infection_matrix_units("g", G)[1]
    p, pq = h.params(ACTIVE, None), h.params(ACTIVE, np.ones(A, np.float32))
    good_s = dict(plan=C.byref(plan.c), params=C.byref(p), rows=rows, nu=N.ptr(ones), s0=N.ptr(ones), stage=None,
                  group=N.ptr(st.labels["g"]), G=G, UG=UG, lost=N.ptr(st.unattributed_by["g"]), err=N.ptr(st.err))
    good_g = dict(plan=C.byref(plan.c), params=C.byref(p), rows=rows, tr=N.ptr(ones), stage=None, U=U, UG=UG,
                  group=N.ptr(st.labels["g"]), G=G, out=N.ptr(st.matrix["g"]), err=N.ptr(st.err))

    def scatter(**change):
        a = dict(good_s, **change)
        return lib.gj_infection_matrix_scatter(a["plan"], a["params"], a["rows"], a["nu"], a["s0"], a["stage"], a["group"],
                                               a["G"], a["UG"], a["lost"], a["err"], N.current_stream())

    def gather(**change):
        a = dict(good_g, **change)
        return lib.gj_infection_matrix_gather(a["plan"], a["params"], a["rows"], a["tr"], a["stage"], a["U"], a["UG"],
                                              a["group"], a["G"], a["out"], a["err"], N.current_stream())

    def clear(plan_=C.byref(plan.c), rows_=rows, nu=N.ptr(ones), UG_=UG, G_=G):
        return lib.gj_infection_matrix_clear(plan_, rows_, nu, UG_, G_, N.current_stream())

    E_NULL, E_RANGE = -1, -2
    for name in ("plan", "params", "rows", "nu", "s0", "UG", "err"):
        assert scatter(**{name: None}) == E_NULL, name
    for name in ("plan", "params", "rows", "tr", "U", "UG", "out", "err"):
        assert gather(**{name: None}) == E_NULL, name
    assert scatter(params=C.byref(pq)) == E_NULL and gather(params=C.byref(pq)) == E_NULL      # quarantine without a stage
    holes = (C.c_void_p * N.GJ_MAX_SETS)()                                       # a set with rows and networks but no UG
    assert scatter(UG=holes) == E_NULL and gather(UG=holes) == E_NULL and gather(U=holes) == E_NULL
    for change in (dict(G=0), dict(G=N.GJ_MATRIX_MAX_GROUPS + 1), dict(group=None)):
        assert scatter(**change) == E_RANGE and gather(**change) == E_RANGE, change
    bad = h.params(ACTIVE, None)
    bad.n_nets = N.GJ_MAX_NETS + 1
    assert scatter(params=C.byref(bad)) == E_RANGE and gather(params=C.byref(bad)) == E_RANGE
    assert clear(plan_=None) == E_NULL and clear(rows_=None) == E_NULL and clear(nu=None) == E_NULL and clear(UG_=None) == E_NULL
    assert clear(G_=0) == E_RANGE and clear(G_=N.GJ_MATRIX_MAX_GROUPS + 1) == E_RANGE
    h.intact()
    assert int(st.err.item()) == 0 and not st.unattributed_by["g"].any() and not st.matrix["g"].any()
    assert not any(u.any() for u in h.by_group().values()) and not any(u.any() for u in h.units().values())
    # ... and the good calls go through: the unattributed counts are optional
    assert scatter(lost=None) == 0 and not st.unattributed_by["g"].any()
    assert scatter() == 0 and gather() == 0 and clear() == 0
    h.intact()
    assert not any(u.any() for u in h.by_group().values())


def test_an_empty_world_launches_nothing(device):
    lib = N.load()
    plan, p = N.Plan(), N.StepParams()
    out = torch.full((2,), SENTINEL, dtype=torch.int64, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    one = torch.ones(1, device=device)
    assert lib.gj_infection_matrix_scatter(C.byref(plan), C.byref(p), None, N.ptr(one), N.ptr(one), None, None, 1, None,
                                           N.ptr(out), N.ptr(err), N.current_stream()) == 0
    assert lib.gj_infection_matrix_gather(C.byref(plan), C.byref(p), None, N.ptr(one), None, None, None, None, 1,
                                          N.ptr(out), N.ptr(err), N.current_stream()) == 0
    assert lib.gj_infection_matrix_clear(C.byref(plan), None, N.ptr(one), None, 1, N.current_stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and int(err.item()) == 0
