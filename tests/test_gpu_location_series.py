"""GPU: the infection-location series through the step and the Runner.

Teacher-forced: every recorded step of the golden fixtures is run through ``gj_step`` from its recorded pre-state and
noise, then attributed by ``gj_location_stats`` from the ``cum`` workspaces the step left behind; the shares must equal
the fixture's own ``ts/<network>`` shares within ``RTOL * (new infections)`` per column (tests/test_location_ref.py).

Runner: on the bundled 769-agent world.  The series are integers in units of 2^-30 of an infection
(``LocationStats.out``), so "sums exactly" is asserted on them; the float32 ``results`` are those integers / 2^30, each
rounded once (relative 2^-24), which is what their sums are held to."""
import itertools

import numpy as np
import pytest
import torch

import gj_testlib as L
from grad_june_amd import _native as N
from grad_june_amd.groups import LocationStats
from test_location_ref import C100, RTOL, reference_shares

pytestmark = pytest.mark.gpu

U = N.GJ_LOC_UNIT


# ---- teacher-forced steps -----------------------------------------------------------------------------------------------------
def attribute_step(npz, prefix, engine, world, device):
    from grad_june_amd.engine import AgentBuffers

    rec = L.step_record(npz, prefix)
    sc = L.step_scalars(rec)
    st = L.device_state(L.pre_state(rec), device)
    A = engine.plan.host.n_agents
    active = sc["active"]
    has_q = sc["quarantine_thresholds"] is not None
    p = engine.params(now=sc["now"], delta_time=sc["delta_time"], day_type=sc["day_type"], active=active,
                      betas=sc["betas"], has_quarantine=has_q, q_threshold=L.q_threshold(sc["quarantine_thresholds"]))
    s0 = st["susceptibility"].clone()
    bufs = AgentBuffers(engine.plan, max_infectiousness=st["max_infectiousness"], shape=st["shape"], rate=st["rate"],
                        shift=st["shift"], infection_time=st["infection_time"], is_infected=st["is_infected"],
                        susceptibility=st["susceptibility"], transmission=st["transmission"],
                        current_stage=st["current_stage"])
    new = torch.empty(A, device=device)
    noise = torch.from_numpy(rec["exp_noise"]).to(device).contiguous()
    engine.step(bufs, p, engine.io(new_infected=new, exp_noise=noise))
    assert np.array_equal(new.cpu().numpy(), rec["new_infected"]), prefix + "the recorded decisions"
    stats = LocationStats(None, 1, active + ["background"], device=device)
    edges = {s: (es["agent"], es["venue"]) for s, es in world["edge_sets"].items()}
    stats.add(engine.plan, p, new, s0, st["current_stage"] if has_q else None, active=active, edges=edges)
    stats.check(prefix)
    row = stats.out[0, 0].cpu().numpy()
    want, background, count = reference_shares(rec, active)
    assert int(row.sum()) == U * count, prefix
    assert background == 0 and row[-1] == 0, prefix
    got = row[:-1] / float(U)
    assert np.all(np.abs(got - want) <= RTOL * count), (prefix, np.abs(got - want).max())
    return count


@pytest.mark.parametrize("layout", ["csr", "tiled"])
def test_c100_policy_variants(device, layout):
    npz = L.load_npz("c100.npz")
    world = L.world_from(npz)
    eng = L.make_engine(world, None, device, layout=layout)
    assert sum(attribute_step(npz, v + "/", eng, world, device) for v in C100) >= 50


@pytest.mark.parametrize("name", ["june769.npz", "june769_hot.npz", "synth10k.npz"])
def test_reference_trajectories(device, name):
    npz = L.load_npz(name)
    world, tables = L.world_from(npz), L.tables_from(npz)
    eng = L.make_engine(world, tables, device, layout="tiled")
    total = sum(attribute_step(npz, f"step{i}/", eng, world, device) for i in range(int(npz["n_steps"])))
    assert total >= {"june769.npz": 5, "june769_hot.npz": 300, "synth10k.npz": 30}[name]


# ---- the Runner on the bundled world ---------------------------------------------------------------------------------------
DAYS = 20
NETWORKS = ["household", "company", "school", "pub", "gym", "grocery", "visit", "cinema", "university", "care_visit",
            "care_home"]
PARENT_KEYS = {"dates", "cases_per_timestep", "daily_cases_per_timestep", "deaths_per_timestep", "cases_by_age_18",
               "cases_by_age_65", "cases_by_age_100", "cases_by_area", "daily_cases_by_area", "deaths_by_area"}
WINDOW = ("2022-02-03", "2022-02-06")


def _params(device, days=DAYS, **extra):
    from grad_june_amd.defaults import default_parameters

    p = default_parameters(str(device))
    p["timer"]["total_days"] = days
    p["infection_seed"]["log_fraction_initial_cases"] = -1.3
    for n in p["networks"]:
        p["networks"][n]["log_beta"] += 0.6
    p["groups_to_save"] = ["area"]
    p.update(extra)
    return p


def _runner(params, seed=21):
    import grad_june_amd as G
    from grad_june_amd import infection

    torch.manual_seed(seed)
    infection._philox_step = itertools.count(1 << 40)
    return G.Runner.from_parameters(params)


def _run(params):
    runner = _runner(params)
    with torch.no_grad():
        results, is_infected = runner()
    return runner, results, is_infected


@pytest.fixture(scope="module")
def with_key(device):
    return _run(_params(device, locations_to_save=True))


@pytest.fixture(scope="module")
def without_key(device):
    return _run(_params(device))


def _units(runner, key, T):
    return runner._locations()[key].out[:T].cpu().numpy()


def test_runner_series(device, with_key, without_key, tmp_path):
    runner, res, inf = with_key
    _, plain, inf_plain = without_key
    assert set(plain) == PARENT_KEYS                                  # without the key: exactly the parent's result keys
    for key, value in plain.items():                                  # ... and nothing that existed changes by a bit
        assert value == res[key] if key == "dates" else torch.equal(value, res[key]), key
    assert torch.equal(inf_plain, inf)
    assert set(res) - set(plain) == {"infections_by_location", "infections_by_location_by_area"}
    assert runner.location_keys == list(runner.model.infection_networks.networks) + ["background", "seed"]
    assert sorted(runner.location_keys[:-2]) == sorted(NETWORKS)
    T, Lc = len(res["dates"]), len(runner.location_keys)
    nat, by_area = res["infections_by_location"], res["infections_by_location_by_area"]
    assert nat.shape == (T, Lc) and by_area.shape == (T, 3, Lc)
    assert nat.dtype == by_area.dtype == torch.float32 and not nat.requires_grad
    daily = res["daily_cases_per_timestep"].cpu().numpy().astype(np.int64)
    assert daily.sum() > 100
    units, units_area = _units(runner, None, T), _units(runner, "area", T)
    assert np.array_equal(units[:, 0].sum(1), U * daily)              # every row sums to the day's new cases, exactly
    assert np.array_equal(units_area.sum(1), units[:, 0])             # by area sums to the nation, exactly
    daily_area = res["daily_cases_by_area"].cpu().numpy().astype(np.int64)
    assert np.array_equal(units_area.sum(2), U * daily_area)
    assert np.array_equal(nat.cpu().numpy(), (units[:, 0] / float(U)).astype(np.float32))
    assert np.array_equal(by_area.cpu().numpy(), (units_area / float(U)).astype(np.float32))
    assert np.all(np.abs(nat.double().sum(1).cpu().numpy() - daily) <= 2.0 ** -23 * daily)
    seed = runner.location_keys.index("seed")                         # row 0: the seeding step
    assert units[0, 0, seed] == U * daily[0] > 0 and units[0].sum() == U * daily[0]
    assert not units[1:, 0, seed].any()
    col = {k: i for i, k in enumerate(runner.location_keys)}
    totals = dict(zip(runner.location_keys, np.round(nat.sum(0).cpu().numpy(), 1)))
    print("infections by location over the run:", totals)
    assert all(totals[k] > 1 for k in ("household", "company", "school"))
    weekend = [i for i, d in enumerate(res["dates"]) if i and d.weekday() >= 5]
    assert weekend and not units[weekend][:, 0, [col["company"], col["school"], col["university"]]].any()   # inactive: zeros
    # the CSVs round-trip
    import pandas as pd

    runner.save_path = tmp_path
    runner.save_results(res, inf)
    flat = pd.read_csv(tmp_path / "results_by_location.csv")
    assert list(flat.columns) == ["date", "location", "infections"]
    assert list(flat["location"][:Lc]) == runner.location_keys
    assert np.array_equal(flat["infections"].to_numpy().astype(np.float32).reshape(T, Lc), nat.cpu().numpy())
    long = pd.read_csv(tmp_path / "results_by_location_by_area.csv")
    assert list(long.columns) == ["date", "area", "location", "infections"]
    assert np.array_equal(long["infections"].to_numpy().astype(np.float32).reshape(T, 3, Lc), by_area.cpu().numpy())
    assert list(long["area"][: 3 * Lc : Lc]) == list(runner.group_keys["area"])
    assert list(pd.read_csv(tmp_path / "results_by_area.csv").columns) == ["date", "area", "cases", "daily_cases", "deaths"]


def test_a_closed_venue_gives_a_zero_column_for_exactly_its_dates(device, with_key):
    _, open_res, _ = with_key
    policies = {"close_venue": {"close_venue": {"start_date": WINDOW[0], "end_date": WINDOW[1], "names": ["household"]}}}
    params = _params(device, locations_to_save=True)
    params["policies"] = dict(params["policies"], **policies)
    runner, res, _ = _run(params)
    col = runner.location_keys.index("household")
    T = len(res["dates"])
    units = _units(runner, None, T)[:, 0]
    closed = np.array([WINDOW[0] <= d.strftime("%Y-%m-%d") < WINDOW[1] for d in res["dates"]])
    assert closed.sum() == 3 and not closed[0]
    assert not units[closed, col].any()
    assert units[closed].sum() > 0                                      # the other networks went on
    first = int(np.nonzero(closed)[0][0])
    assert np.array_equal(units[:first], _units(with_key[0], None, T)[:first, 0])      # before the window: the open run
    assert units[1:first, col].sum() > 0 and units[first + 3:, col].sum() > 0
    assert np.array_equal(units.sum(1), U * res["daily_cases_per_timestep"].cpu().numpy().astype(np.int64))


def _differentiable(params):
    runner = _runner(params)
    nets = runner.model.infection_networks.networks
    for n in nets.values():
        n.log_beta = torch.nn.Parameter(n.log_beta.detach().clone())
    results, _ = runner()
    betas = [n.log_beta for n in nets.values()]
    T = len(results["dates"])
    w = torch.linspace(0.5, 1.5, T, device=results["cases_per_timestep"].device)
    loss = (w * results["cases_per_timestep"]).sum() + results["deaths_per_timestep"].sum() + \
        results["cases_by_area"][:, 1].sum()
    grads = torch.autograd.grad(loss, betas, allow_unused=True)
    return runner, results, [None if g is None else g.detach().cpu().numpy() for g in grads]


def test_a_differentiable_run_records_the_series_without_a_gradient(device):
    days = 10
    runner, res, grads = _differentiable(_params(device, days=days, locations_to_save=True))
    _, plain, plain_grads = _differentiable(_params(device, days=days))
    assert sum(g is not None and float(g) != 0.0 for g in grads) >= 5
    for a, b in zip(grads, plain_grads):                               # the key changes no gradient by a bit
        assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes())
    assert res["cases_per_timestep"].requires_grad
    for key in ("infections_by_location", "infections_by_location_by_area"):
        assert key not in plain and not res[key].requires_grad and res[key].grad_fn is None
    T = len(res["dates"])
    units = _units(runner, None, T)[:, 0]
    daily = res["daily_cases_per_timestep"].detach().cpu().numpy().astype(np.int64)
    assert np.array_equal(units.sum(1), U * daily) and daily[1:].sum() > 20
    # the same series as the plain (in-place) run of the same configuration
    _, same, _ = _run(_params(device, days=days, locations_to_save=True))
    assert torch.equal(same["infections_by_location_by_area"], res["infections_by_location_by_area"])


def test_without_the_key_the_kernel_is_never_launched(device, monkeypatch):
    lib = N.load()
    real, calls = lib.gj_location_stats, []

    def counting(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(lib, "gj_location_stats", counting)
    runner, res, _ = _run(_params(device, days=5))
    assert calls == [] and "infections_by_location" not in res
    assert runner.model.location_stats is None and runner._locations() == {}
    _run(_params(device, days=5, locations_to_save=True))
    assert len(calls) == 2 * (5 + 1)                                    # the nation and by area, the seed and five steps
