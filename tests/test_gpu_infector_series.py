"""GPU: the infector series through the step and the Runner, on the bundled 769-agent world.

The run records, at every step, what the two kernels were launched with - the plan's ``cum`` workspaces, the step's
transmissions, the pre-step susceptibility, the stage and the new infections - and the numpy restatement
(tests/gj_infector_ref.py) is driven from those: its ``U`` per step, its credits, their sums by area and by cohort.

Bounds, per row and group, in units of 2^-30 of an infection: a cell of ``U`` deviates from the restatement by at most
(edges of new infections touching its venue + n_nets) units (tests/test_gpu_infector_stats.py), the agents of a venue share
a cell's deviation with weights that sum to 1, and every infectious agent adds one llrint: the sum of the cell bounds
over the step's touched venues + the infectious agents of the group + 1 (the fp64 reassociation, 1e-12 relative of at most
a few hundred infections, is below 2^-30 * 2^30 = 1 unit).  R is a mean of float32 conversions: 1e-6 relative.

Conservation (the credits of a step sum to its attributed infections only up to the fp32 roundings inside ``cum``):
measured with the fp64 restatement on the captured ``cum`` of this run, the largest residual of a row is 3.986e-07
infections (rows of up to 21 attributed infections; RESIDUAL_MEASURED, rounded up); 4x that is asserted of the kernels'
series, taken from its integer units (the float32 results round the residual away)."""
import numpy as np
import pytest
import torch

import gj_infector_ref as I
import gj_location_ref as R
from grad_june_amd import _native as N
from grad_june_amd.groups import InfectorStats
from test_gpu_location_series import PARENT_KEYS, _differentiable, _params, _run

pytestmark = pytest.mark.gpu

U = N.GJ_LOC_UNIT
RESIDUAL_MEASURED = 4.0e-07   # infections per row, by the restatement on this run's cum; see the module docstring
NEW_KEYS = {"infections_caused_per_timestep", "infections_unattributed_per_timestep", "reproduction_number_per_timestep",
            "infections_caused_by_area", "reproduction_number_by_area"}


def _capture(log):
    """Record what every InfectorStats.record is called with; returns the method to put back."""
    real = InfectorStats.record

    def record(self, plan, params, new_infected, susceptibility0, current_stage, transmission, row=0, edges=None):
        f = lambda t: None if t is None else t.detach().cpu().numpy().copy()
        log.append(dict(plan=plan, params=type(params).from_buffer_copy(params), row=row, nu=f(new_infected),
                        s0=f(susceptibility0), stage=f(current_stage), tr=f(transmission),
                        cum={s.name: plan.cum_of(s.name).cpu().numpy().copy() for s in plan.host.sets}))
        return real(self, plan, params, new_infected, susceptibility0, current_stage, transmission, row=row, edges=edges)

    InfectorStats.record = record
    return real


@pytest.fixture(scope="module")
def with_keys(device):
    log = []
    real = _capture(log)
    try:
        runner, res, inf = _run(_params(device, infectors_to_save=True, locations_to_save=True))
    finally:
        InfectorStats.record = real
    return runner, res, inf, log


@pytest.fixture(scope="module")
def restated(with_keys):
    """The restatement of every recorded step: per row the national and by-area sums (units), the bound of a group sum,
    the unattributed count and the residual of the fp64 credits; over the run ``caused`` and ``infected_row``."""
    runner, res, _, log = with_keys
    A = runner.n_agents
    data = runner.data
    plan = log[0]["plan"]
    cls = plan.agent_class[:A].cpu().numpy().astype(np.int64)
    age = cls % 100
    tables = plan.tables.cpu().numpy().reshape(-1, N.GJ_TABLE_SIZE) if plan.tables is not None else None
    names = [s.name for s in plan.host.sets]
    edges = {s: tuple(data["attends_" + s].edge_index.cpu().numpy()) for s in names if "attends_" + s in data}
    pc = {s.name: plan.keep[i]["v_pc"].cpu().numpy() for i, s in enumerate(plan.host.sets)}
    area = runner._infectors().labels["area"].cpu().numpy().astype(np.int64)
    G = runner._infectors().n_groups["area"]
    caused, infected_row, rows = np.zeros(A), np.full(A, -1, np.int64), {}
    for rec in log:
        p = rec["params"]
        q = np.ones(A) if not p.has_quarantine else (rec["stage"] < np.float32(p.q_threshold)).astype(np.float64)
        nets, per_set = [], {}
        for i in range(p.n_nets):
            n = p.nets[i]
            s = names[n.set]
            row = None if n.table < 0 else tables[n.table, p.day_type * 200 + cls]
            nets.append(I.Net(s, per_set.get(s, 0), float(n.beta), R.mask_weight(n.mask_kind, q, row, age),
                              R.mask_weight(min(n.mask_kind, R.MASK_QL), q, row, age)))
            per_set[s] = per_set.get(s, 0) + 1
        units, lost, err, touched = I.scatter(nets, edges, rec["cum"], rec["s0"], rec["nu"], A)
        assert err == 0
        infected_row[rec["nu"] == 1] = rec["row"]
        out = dict(lost=lost, new=int(rec["nu"].sum()), national=0, area=[0] * G, bound=np.ones(G, np.int64), residual=0.0,
                   cells=0)
        if p.n_nets:
            credit, by_area, err = I.gather(nets, edges, rec["cum"], pc, units, rec["tr"][:A], A, area, G)
            assert err == 0
            caused += credit
            cells = sum(int((touched[n.set][touched[n.set] > 0] + len(nets)).sum()) for n in nets)
            out.update(national=sum(by_area), area=by_area, residual=abs(credit.sum() - (out["new"] - lost)), cells=cells,
                       bound=cells + np.bincount(area[rec["tr"][:A] > 0], minlength=G) + 1)
        rows[rec["row"]] = out
    return dict(rows=rows, caused=caused, infected_row=infected_row, area=area, G=G)


def test_series_agree_with_the_restatement(with_keys, restated, tmp_path):
    runner, res, inf, log = with_keys
    assert NEW_KEYS <= set(res) and len(log) == len(res["dates"])
    T, G, st = len(res["dates"]), restated["G"], runner._infectors()
    nat, by_area = st.out[None][:T, 0].cpu().numpy(), st.out["area"][:T].cpu().numpy()
    assert np.array_equal(by_area.sum(1), nat)                                     # the same credits, the same llrint
    worst = 0
    for r in range(T):
        want = restated["rows"][r]
        dev = np.abs(by_area[r] - np.array(want["area"], dtype=np.int64))
        worst = max(worst, int(dev.max()))
        assert np.all(dev <= want["bound"]), (r, dev, want["bound"])
        assert abs(int(nat[r]) - want["national"]) <= want["bound"].sum()
    print("largest deviation of a by-area sum from the restatement, units of 2^-30:", worst)
    assert nat[0] == 0 and nat[1:].sum() > 50 * U
    assert np.array_equal(res["infections_caused_per_timestep"].cpu().numpy(), (nat / float(U)).astype(np.float32))
    assert np.array_equal(res["infections_caused_by_area"].cpu().numpy(), (by_area / float(U)).astype(np.float32))
    # per agent: the offspring distribution
    caused = runner.data["agent"]["infections_caused"].cpu().numpy()
    row = runner.data["agent"]["infected_row"].cpu().numpy()
    assert np.array_equal(row, restated["infected_row"])
    # an agent's credit moves with the cells of U it shares in: by no more than all the cells' bounds together
    slack = sum(restated["rows"][r]["cells"] for r in range(T)) / float(U)
    print("caused: largest deviation from the restatement", np.abs(caused - restated["caused"]).max(), "slack", slack)
    assert np.all(np.abs(caused - restated["caused"]) <= 1e-12 * restated["caused"] + slack)
    assert abs(caused.sum() - nat.sum() / U) <= 1e-6 * caused.sum()
    daily = res["daily_cases_per_timestep"].cpu().numpy().astype(np.int64)
    assert np.array_equal(np.bincount(row[row >= 0], minlength=T), daily)
    # R by cohort: the mean of caused over the agents infected in a row (and of an area); NaN for an empty cohort
    for key, labels, n_groups in ((None, np.zeros_like(row), 1), ("area", restated["area"], G)):
        got = res["reproduction_number_per_timestep" if key is None else "reproduction_number_by_area"].cpu().numpy()
        got = got.reshape(T, n_groups)
        for r in range(T):
            for g in range(n_groups):
                cohort = (row == r) & (labels == g)
                if not cohort.any():
                    assert np.isnan(got[r, g]), (r, g)
                else:
                    want = restated["caused"][cohort].sum() / cohort.sum()
                    # (+ the credits' slack above, and gj_group_stats' fixed point: 2^-33 per value)
                    assert abs(got[r, g] - want) <= 1e-6 * want + slack + 2.0 ** -33, (key, r, g, got[r, g], want)
    R_t = res["reproduction_number_per_timestep"].cpu().numpy()
    print("R by cohort (right-censored at the end):", np.round(R_t, 3))
    assert R_t[0] > 0 and (np.isnan(R_t[-1]) or R_t[-1] == 0)                      # the last cohort has not transmitted yet
    # the CSVs
    import pandas as pd

    runner.save_path = tmp_path
    runner.save_results(res, inf)
    flat = pd.read_csv(tmp_path / "results_infectors.csv")
    assert list(flat.columns) == ["date", "series", "value"] and len(flat) == 3 * T
    assert list(flat["series"][:3]) == ["infections_caused", "infections_unattributed", "reproduction_number"]
    assert np.array_equal(flat["value"].to_numpy()[0::3].astype(np.float32), res["infections_caused_per_timestep"].cpu().numpy())
    long = pd.read_csv(tmp_path / "results_infectors_by_area.csv")
    assert list(long.columns) == ["date", "area", "infections_caused", "reproduction_number"] and len(long) == T * G
    assert np.array_equal(long["infections_caused"].to_numpy().astype(np.float32).reshape(T, G),
                          res["infections_caused_by_area"].cpu().numpy())


def test_unattributed_is_the_location_series_background_and_seed(with_keys, restated):
    runner, res, _, _ = with_keys
    T = len(res["dates"])
    loc = runner._locations()[None].out[:T, 0].cpu().numpy()
    col = {k: i for i, k in enumerate(runner.location_keys)}
    lost = runner._infectors().unattributed[:T].cpu().numpy()
    assert np.array_equal(U * lost, loc[:, col["background"]] + loc[:, col["seed"]])      # exactly, in every row
    assert np.array_equal(res["infections_unattributed_per_timestep"].cpu().numpy(), lost.astype(np.float64))
    assert lost[0] == res["daily_cases_per_timestep"][0].item() > 0                  # row 0: the seeds
    assert [restated["rows"][r]["lost"] for r in range(T)] == lost.tolist()


def test_the_credits_of_a_row_sum_to_its_attributed_infections(with_keys, restated):
    """Conservation: measured with the fp64 restatement on the captured ``cum`` of this run, see the module docstring."""
    runner, res, _, _ = with_keys
    T = len(res["dates"])
    measured = max(restated["rows"][r]["residual"] for r in range(T))
    attributed = np.array([restated["rows"][r]["new"] - restated["rows"][r]["lost"] for r in range(T)])
    caused = runner._infectors().out[None][:T, 0].cpu().numpy() / float(U)          # fp64: exact for these sizes
    got = np.abs(caused - attributed)
    print(f"conservation residual per row: restatement max {measured:.3e}, kernels max {got.max():.3e} infections; "
          f"attributed per row up to {attributed.max()}")
    assert 0 < measured <= RESIDUAL_MEASURED                                        # the recorded figure is this run's
    assert got.max() > 0 and np.all(got <= 4 * RESIDUAL_MEASURED)


def test_the_key_changes_no_other_result(device, with_keys):
    runner, res, inf, _ = with_keys
    lib = N.load()
    calls = []
    real = {name: getattr(lib, name) for name in ("gj_infector_scatter", "gj_infector_gather", "gj_infector_clear")}
    try:
        for name, fn in real.items():
            setattr(lib, name, (lambda fn: lambda *a: (calls.append(1), fn(*a))[1])(fn))
        plain_runner, plain, plain_inf = _run(_params(device, locations_to_save=True))
    finally:
        for name, fn in real.items():
            setattr(lib, name, fn)
    assert calls == []                                                              # off: never launched
    assert plain_runner._infectors() is None and plain_runner.model.infector_stats is None
    plan = plain_runner.model._engine(plain_runner.data, torch.device(device)).plan
    assert getattr(plan, "_infector_units", None) is None                           # ... and nothing allocated
    assert "infections_caused" not in plain_runner.data["agent"]
    assert set(res) - set(plain) == NEW_KEYS and PARENT_KEYS <= set(plain)
    for key, value in plain.items():
        assert value == res[key] if key == "dates" else torch.equal(value, res[key]), key
    assert torch.equal(plain_inf, inf)


def test_a_differentiable_run_keeps_every_gradient_bit(device):
    days = 8
    runner, res, grads = _differentiable(_params(device, days=days, infectors_to_save=True))
    _, plain, plain_grads = _differentiable(_params(device, days=days))
    assert sum(g is not None and float(g) != 0.0 for g in grads) >= 5
    for a, b in zip(grads, plain_grads):
        assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes())
    for key in NEW_KEYS:
        assert key not in plain and not res[key].requires_grad and res[key].grad_fn is None
    for key, value in plain.items():
        assert value == res[key] if key == "dates" else torch.equal(value.detach(), res[key].detach()), key
    # the same series as the plain (in-place) run of the same configuration
    _, same, _ = _run(_params(device, days=days, infectors_to_save=True))
    for key in NEW_KEYS:      # (NaN: an empty cohort)
        assert torch.equal(torch.nan_to_num(same[key], nan=-1.0), torch.nan_to_num(res[key], nan=-1.0)), key
