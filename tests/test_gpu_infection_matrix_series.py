"""GPU: the who-infects-whom matrix through the step and the Runner, on the bundled 769-agent world, by the binned
labelling ``age_band: {attribute: age, bins: [0, 18, 65, 100]}``.

The run records, at every step, what the kernels were launched with (as tests/test_gpu_infector_series.py does: the plan's
``cum`` workspaces, the transmissions, the pre-step susceptibility, the stage, the new infections) and, between the
scatters and the gathers, the plan's ``UG``.  The numpy restatement (tests/gj_matrix_ref.py) is driven from those.

Exact, in integer units of 2^-30 of an infection: the matrix equals the restatement's pass 2 on the step's ``cum`` and
``UG`` (every term a fixed chain of correctly rounded fp64 operations and one rounding to an integer; integer sums);
``UG`` sums per group, with the unattributed counts, to the group's new infections; the unattributed counts by group sum
to the national count.  ``UG`` itself is held to the restatement's pass 1 within the floor bound of
tests/test_gpu_infector_stats.py - (edges of new infections touching the venue + n_nets) units per venue.

Marginals: the row sums (by infector) are within (non-zero terms + infectious agents of the group) / 2 units of
``infections_caused_by_age_band``.  The column sums (by infected) conserve the attributed infections of the band only up
to the fp32 roundings inside ``cum``: measured with the fp64 restatement on the captured ``cum`` of this run, the largest
residual of a (row, band) is 2.943e-07 infections (up to 12 attributed infections per row and band; RESIDUAL_MEASURED,
rounded up); 4x that is asserted of the kernels' series, taken from its integer units."""
import numpy as np
import pytest
import torch

import gj_infector_ref as I
import gj_location_ref as R
import gj_matrix_ref as M
from grad_june_amd import _native as N
from grad_june_amd.groups import InfectorStats
from test_gpu_infector_series import _capture
from test_gpu_location_series import _differentiable, _params, _run

pytestmark = pytest.mark.gpu

U = N.GJ_LOC_UNIT
BANDS = {"age_band": {"attribute": "age", "bins": [0, 18, 65, 100]}}
KEYS = ["0-18", "18-65", "65-100"]
NEW_KEYS = {"infection_matrix_by_age_band", "infections_unattributed_by_age_band"}
RESIDUAL_MEASURED = 3.0e-07   # infections per (row, band), by the restatement on this run's cum; see the module docstring


def _capture_units(log):
    """Record the plan's ``UG`` at every InfectorStats.matrix_gather: after the scatters, before the clears."""
    real = InfectorStats.matrix_gather

    def matrix_gather(self, plan, params, transmission, current_stage, row=0, edges=None):
        G = self.n_groups["age_band"]
        log[row] = {s.name: plan.infection_matrix_units("age_band", G)[0][i][: s.n_venues].cpu().numpy().copy()
                    for i, s in enumerate(plan.host.sets)}
        return real(self, plan, params, transmission, current_stage, row=row, edges=edges)

    InfectorStats.matrix_gather = matrix_gather
    return real


@pytest.fixture(scope="module")
def with_key(device):
    log, units = [], {}
    real, real_gather = _capture(log), _capture_units(units)
    try:
        runner, res, inf = _run(_params(device, groups_to_save=[BANDS], infectors_to_save=True,
                                        infection_matrices_to_save=["age_band"]))
    finally:
        InfectorStats.record, InfectorStats.matrix_gather = real, real_gather
    return runner, res, inf, log, units


@pytest.fixture(scope="module")
def restated(with_key):
    """Per recorded step: the restatement's pass 1 (UG, unattributed by band, the floor bound per venue) and its pass 2 on
    the DEVICE's UG (the matrix, the non-zero terms by the infector's band)."""
    runner, res, _, log, units = with_key
    A, data, plan = runner.n_agents, runner.data, log[0]["plan"]
    cls = plan.agent_class[:A].cpu().numpy().astype(np.int64)
    age = cls % 100
    tables = plan.tables.cpu().numpy().reshape(-1, N.GJ_TABLE_SIZE) if plan.tables is not None else None
    names = [s.name for s in plan.host.sets]
    edges = {s: tuple(data["attends_" + s].edge_index.cpu().numpy()) for s in names if "attends_" + s in data}
    pc = {s.name: plan.keep[i]["v_pc"].cpu().numpy() for i, s in enumerate(plan.host.sets)}
    band = runner._infectors().labels["age_band"].cpu().numpy().astype(np.int64)
    G = runner._infectors().n_groups["age_band"]
    rows = {}
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
        UG, lost, err = M.scatter_by_group(nets, edges, rec["cum"], rec["s0"], rec["nu"], A, band, G)
        assert err == 0
        touched = I.scatter(nets, edges, rec["cum"], rec["s0"], rec["nu"], A)[3]
        out = dict(UG=UG, lost=lost, new=np.bincount(band[rec["nu"] == 1], minlength=G), touched=touched, n_nets=len(nets),
                   matrix=np.zeros((G, G), np.int64), terms=np.zeros(G, np.int64), infectious=np.zeros(G, np.int64))
        if p.n_nets:
            tr = rec["tr"][:A]
            for _, g, h, value in M.matrix_terms(nets, edges, rec["cum"], pc, units[rec["row"]], tr, A, band, G):
                out["matrix"][g, h] += value
                out["terms"][g] += value != 0
            out["infectious"] = np.bincount(band[tr > 0], minlength=G)
        rows[rec["row"]] = out
    return dict(rows=rows, band=band, G=G)


def test_the_matrix_equals_the_restatement_exactly(with_key, restated):
    runner, res, _, log, units = with_key
    T, G, st = len(res["dates"]), restated["G"], runner._infectors()
    assert NEW_KEYS <= set(res) and len(log) == T and sorted(units) == list(range(1, T))
    assert runner.group_keys["age_band"].tolist() == KEYS and G == 3
    got = st.matrix["age_band"][:T].cpu().numpy()
    for r in range(T):
        assert np.array_equal(got[r], restated["rows"][r]["matrix"]), r
    assert got.sum() > 50 * U and (got.sum(0) > 0).all()                            # every pair of bands occurs
    values = res["infection_matrix_by_age_band"]
    assert values.dtype == torch.float32 and tuple(values.shape) == (T, G, G)
    assert np.array_equal(values.cpu().numpy(), (got / float(U)).astype(np.float32))


def test_the_units_by_band_are_the_steps_new_infections(with_key, restated):
    """Exactly per band; and cell by cell within the floor bound of the restatement's pass 1."""
    runner, res, _, log, units = with_key
    T, G = len(res["dates"]), restated["G"]
    lost_by = runner._infectors().unattributed_by["age_band"][:T].cpu().numpy()
    worst = 0
    for r in range(1, T):
        want = restated["rows"][r]
        for g in range(G):
            assert sum(int(u[:, :, g].sum()) for u in units[r].values()) + U * int(lost_by[r, g]) == U * int(want["new"][g])
        for s, u in units[r].items():
            dev = np.abs(u - want["UG"][s]).max((1, 2))
            worst = max(worst, int(dev.max()))
            assert np.all(dev <= want["touched"][s] + want["n_nets"]), (r, s)
        assert np.array_equal(lost_by[r], want["lost"])
    print("largest deviation of a cell of UG from the restatement, in units of 2^-30:", worst)


def test_unattributed_by_band_sums_to_the_national_count_and_row_0_is_the_seeding_step(with_key, restated):
    runner, res, _, log, _ = with_key
    T, st = len(res["dates"]), runner._infectors()
    by_band = res["infections_unattributed_by_age_band"]
    assert by_band.dtype == torch.float64 and tuple(by_band.shape) == (T, 3)
    assert torch.equal(by_band.sum(1), res["infections_unattributed_per_timestep"])
    assert np.array_equal(by_band.cpu().numpy(), st.unattributed_by["age_band"][:T].cpu().numpy().astype(np.float64))
    # row 0: the matrix is zero and the seeds are counted by their band
    seeds = np.bincount(restated["band"][log[0]["nu"] == 1], minlength=3)
    assert log[0]["row"] == 0 and seeds.sum() == res["daily_cases_per_timestep"][0].item() > 0
    assert not res["infection_matrix_by_age_band"][0].any() and np.array_equal(by_band[0].cpu().numpy(), seeds)
    assert np.array_equal(res["daily_cases_by_age_band"][0].cpu().numpy(), seeds)


def test_the_marginals(with_key, restated):
    runner, res, _, _, _ = with_key
    T, st = len(res["dates"]), runner._infectors()
    matrix = st.matrix["age_band"][:T].cpu().numpy()
    # by infector: one half-unit rounding per term against one per agent
    caused = st.out["age_band"][:T].cpu().numpy()
    for r in range(T):
        want = restated["rows"][r]
        assert np.all(2 * np.abs(matrix[r].sum(1) - caused[r]) <= want["terms"] + want["infectious"]), r
    # by infected: the attributed infections of the band, up to the fp32 roundings inside cum
    daily = res["daily_cases_by_age_band"].cpu().numpy().astype(np.int64)
    lost = st.unattributed_by["age_band"][:T].cpu().numpy()
    assert np.array_equal(daily, np.stack([restated["rows"][r]["new"] for r in range(T)]))
    attributed = daily - lost
    measured = max(np.abs(restated["rows"][r]["matrix"].sum(0) / float(U) - attributed[r]).max() for r in range(T))
    got = np.abs(matrix.sum(1) / float(U) - attributed)                             # fp64: exact for these sizes
    print(f"conservation residual per (row, band): restatement max {measured:.3e}, kernels max {got.max():.3e} infections; "
          f"attributed per (row, band) up to {attributed.max()}")
    assert 0 < measured <= RESIDUAL_MEASURED                                        # the recorded figure is this run's
    assert got.max() > 0 and np.all(got <= 4 * RESIDUAL_MEASURED)


def test_the_csvs(with_key, tmp_path):
    import pandas as pd

    runner, res, inf, _, _ = with_key
    T, G = len(res["dates"]), 3
    runner.save_path = tmp_path
    runner.save_results(res, inf)
    long = pd.read_csv(tmp_path / "results_infection_matrix_by_age_band.csv")
    assert list(long.columns) == ["date", "infector", "infected", "infections"] and len(long) == T * G * G
    assert list(long["infector"][: G * G]) == [k for k in KEYS for _ in range(G)] and list(long["infected"][: G * G]) == KEYS * G
    assert np.array_equal(long["infections"].to_numpy().astype(np.float32).reshape(T, G, G),
                          res["infection_matrix_by_age_band"].cpu().numpy())
    by_band = pd.read_csv(tmp_path / "results_infectors_by_age_band.csv")
    assert list(by_band.columns) == ["date", "age_band", "infections_caused", "reproduction_number", "infections_unattributed"]
    assert np.array_equal(by_band["infections_unattributed"].to_numpy().reshape(T, G),
                          res["infections_unattributed_by_age_band"].cpu().numpy())
    flat = pd.read_csv(tmp_path / "results_by_age_band.csv")
    assert list(flat["age_band"][:G]) == KEYS                                       # a binned labelling is an ordinary one


def test_the_key_changes_no_other_result(device, with_key):
    runner, res, inf, _, _ = with_key
    lib = N.load()
    calls = []
    names = ("gj_infection_matrix_scatter", "gj_infection_matrix_gather", "gj_infection_matrix_clear")
    real = {name: getattr(lib, name) for name in names}
    try:
        for name, fn in real.items():
            setattr(lib, name, (lambda fn: lambda *a: (calls.append(1), fn(*a))[1])(fn))
        plain_runner, plain, plain_inf = _run(_params(device, groups_to_save=[BANDS], infectors_to_save=True))
    finally:
        for name, fn in real.items():
            setattr(lib, name, fn)
    assert calls == []                                                              # off: never launched
    st = plain_runner._infectors()
    assert plain_runner.matrices_saved == [] and st.matrix == {} and st.unattributed_by == {}
    plan = plain_runner.model._engine(plain_runner.data, torch.device(device)).plan
    assert not getattr(plan, "_infection_matrix_units", None)                       # ... and no UG on the plan
    with_plan = runner.model._engine(runner.data, torch.device(device)).plan
    assert list(with_plan._infection_matrix_units) == ["age_band"]
    assert not any(bool(u.any()) for u in with_plan._infection_matrix_units["age_band"][0])      # zero between steps
    assert set(res) - set(plain) == NEW_KEYS
    for key, value in plain.items():      # (NaN: an empty cohort of the reproduction numbers)
        same = value == res[key] if key == "dates" else torch.equal(torch.nan_to_num(value, nan=-1.0),
                                                                    torch.nan_to_num(res[key], nan=-1.0))
        assert same, key
    assert torch.equal(plain_inf, inf)


def test_a_differentiable_run_keeps_every_gradient_bit(device):
    days, groups = 8, ["area", BANDS]
    keys = dict(groups_to_save=groups, infectors_to_save=True)
    runner, res, grads = _differentiable(_params(device, days=days, infection_matrices_to_save=["age_band"], **keys))
    _, plain, plain_grads = _differentiable(_params(device, days=days, **keys))
    assert sum(g is not None and float(g) != 0.0 for g in grads) >= 5
    for a, b in zip(grads, plain_grads):
        assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes())
    for key in NEW_KEYS:
        assert key not in plain and not res[key].requires_grad and res[key].grad_fn is None
    for key, value in plain.items():
        same = value == res[key] if key == "dates" else torch.equal(torch.nan_to_num(value.detach(), nan=-1.0),
                                                                    torch.nan_to_num(res[key].detach(), nan=-1.0))
        assert same, key
    # the same series as the plain (in-place) run of the same configuration
    _, same, _ = _run(_params(device, days=days, infection_matrices_to_save=["age_band"], **keys))
    for key in NEW_KEYS:
        assert torch.equal(same[key], res[key]), key
    assert res["infection_matrix_by_age_band"].sum() > 5
