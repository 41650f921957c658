"""CPU: the infection-location attribution restated in numpy (tests/gj_location_ref.py) against the reference's own
numbers - the golden fixtures record ``ts/<network>`` and ``new_infected`` for every step - and the host logic of the
series: the column order, the YAML key, what a partitioned run answers, and a Runner without the key.

Tolerance of a share: ``RTOL * (new infections of the step)`` per column, RTOL the 2e-5 tests/test_gpu_golden_parity.py
asserts for the per-agent ``ts``: perturbing every t_n by a relative RTOL moves t_n / T by at most RTOL / 2 (the share
x / (x + y) has d share = share * (1 - share) * (dx / x - dy / y), and share * (1 - share) <= 1 / 4)."""
import numpy as np
import pytest

import gj_location_ref as R
import gj_testlib as L

RTOL = 2e-5
C100 = ["closed", "distancing", "quarantine", "quarantine_mixed", "plain_t3"]


def fixture_steps():
    for name in ("june769.npz", "june769_hot.npz", "synth10k.npz"):
        npz = L.load_npz(name)
        for i in range(int(npz["n_steps"])):
            yield name, f"step{i}/", npz
    npz = L.load_npz("c100.npz")
    for v in C100:
        yield "c100.npz", v + "/", npz


def reference_shares(rec, active):
    """sum_a nu[a] * ts_n[a] / sum_n ts_n[a] per network from the fixture's own per-agent terms (float64), and the
    number of infected agents whose terms sum to 0 (background)."""
    nu = rec["new_infected"].astype(np.float64)
    ts = np.stack([rec["ts/" + n].astype(np.float64) for n in active])
    T = ts.sum(0)
    hit = nu > 0.5
    background = int((hit & ~(T > 0)).sum())
    ok = hit & (T > 0)
    return (ts[:, ok] / T[ok]).sum(1), background, int(hit.sum())


def restated(npz, prefix):
    world, tables = L.world_from(npz), {k: v.numpy() for k, v in L.tables_from(npz).items()}
    rec = L.step_record(npz, prefix)
    sc = L.step_scalars(rec)
    active = sc["active"]
    qmask = None
    if sc["quarantine_thresholds"] is not None:
        qmask = (rec["pre/current_stage"] < np.float32(L.q_threshold(sc["quarantine_thresholds"]))).astype(np.float64)
        if "qmask" in rec:
            assert np.array_equal(qmask, rec["qmask"])
    terms = R.step_terms(world, tables, active, {n: rec["cum/" + n] for n in active}, rec["pre/susceptibility"],
                         sc["day_type"], qmask)
    n = len(active)
    out, err = R.location_stats(terms, rec["new_infected"], None, 1, list(range(n)), n + 1, n)
    return rec, active, out[0], err


def test_shares_equal_the_references_own_terms_on_every_recorded_step():
    seen, splits = 0, {}
    for name, prefix, npz in fixture_steps():
        rec, active, row, err = restated(npz, prefix)
        want, background, count = reference_shares(rec, active)
        assert err == 0, (name, prefix)
        assert sum(row) == R.U * count, (name, prefix)                       # every infection adds exactly one unit
        assert background == 0 and row[-1] == 0, (name, prefix, "a background infection")
        got = np.array([v / R.U for v in row[:-1]])
        assert np.all(np.abs(got - want) <= RTOL * count), (name, prefix, np.abs(got - want).max())
        splits[(name, prefix)] = (count, dict(zip(active, got)))
        seen += 1
    assert seen == 15 + 15 + 7 + len(C100)
    # the splits are not trivial
    count, hot = splits[("june769_hot.npz", "step0/")]
    assert count == 45
    for network, share in (("household", 21.1), ("company", 12.5), ("school", 7.2), ("university", 3.0)):
        assert abs(hot[network] - share) < 0.06, (network, hot[network])
    for variant in ("closed/", "quarantine/"):
        count, split = splits[("c100.npz", variant)]
        assert count > 0 and split["household"] == count                     # household-only, to the unit


def test_shares_rule():
    U = R.U
    assert R.shares([]) == ([], U, 0)                                        # no active network (the seeding step)
    assert R.shares([0.0, 0.0]) == ([0, 0], U, 0)                            # nobody transmitted: background
    assert R.shares([3.0]) == ([U], 0, 0)
    assert R.shares([1.0, 1.0]) == ([U // 2, U // 2], 0, 0)
    c, bg, err = R.shares([1.0, 1.0, 1.0])                                   # the remainder: lowest index on a tie
    assert (c, bg, err) == ([U // 3 + 1, U // 3, U // 3], 0, 0)
    c, bg, err = R.shares([1.0, 2.0, 4.0])                                   # ... else the largest term
    assert c == [U // 7, 2 * U // 7, U - U // 7 - 2 * U // 7] and sum(c) == U
    assert R.shares([float("nan"), 2.0]) == ([0, U], 0, R.ERR_VALUE)         # NaN / negative: 0, and reported
    assert R.shares([-1.0, 2.0]) == ([0, U], 0, R.ERR_VALUE)
    assert R.shares([float("nan")]) == ([0], U, R.ERR_VALUE)
    assert R.shares([float("inf"), 1.0]) == ([0, 0], U, 0)                   # T not finite: background
    assert R.shares([1e308, 1e308]) == ([0, 0], U, 0)


def test_bad_agents_never_reach_a_bin():
    terms = np.array([[1.0, 1.0, 1.0, 1.0, 1.0], [3.0, 0.0, 1.0, 1.0, 1.0]])
    nu = np.array([1.0, 1.0, 0.5, np.nan, 1.0])
    out, err = R.location_stats(terms, nu, np.array([0, 1, 0, 0, 7]), 2, [1, 0], 3, 2)
    assert err == (R.ERR_VALUE | R.ERR_LABEL)
    assert out == [[3 * R.U // 4, R.U // 4, 0], [0, R.U, 0]]


# ---- host logic -------------------------------------------------------------------------------------------------------------
def test_column_order_and_yaml_key():
    from grad_june_amd.groups import location_keys, locations_to_save

    assert location_keys(["household", "school", "pub"]) == ["household", "school", "pub", "background", "seed"]
    assert location_keys([]) == ["background", "seed"]
    with pytest.raises(ValueError, match="shadow"):
        location_keys(["household", "seed"])
    assert locations_to_save(None) is False and locations_to_save(False) is False and locations_to_save(True) is True
    for bad in ("yes", 1, ["household"]):
        with pytest.raises(ValueError, match="true or false"):
            locations_to_save(bad)


STAGES = ["recovered", "susceptible", "exposed", "infectious", "symptomatic", "severe", "critical", "dead"]
NETWORKS = ["household", "company", "school"]


class _Model:
    """What Runner.__init__ reads of a model."""
    device = "cpu"

    class symptoms_updater:
        class symptoms_sampler:
            stages = STAGES

    class infection_networks:
        networks = dict.fromkeys(NETWORKS)


def _runner(cls=None, **kw):
    import torch

    from grad_june_amd.graph import HeteroData
    from grad_june_amd.runner import Runner

    cls = cls or Runner
    data = HeteroData()
    ag = data["agent"]
    ag.id, ag.age, ag.sex = torch.arange(6), torch.tensor([5, 20, 30, 70, 80, 40]), torch.zeros(6, dtype=torch.long)
    ag.area = ["a", "b", "a", "b", "a", "c"]
    for k in Runner._STATE:
        ag[k] = torch.zeros(6)
    ag.symptoms = {k: torch.ones(6) for k in Runner._SYMPTOMS}
    return cls(model=_Model(), data=data, timer=None, log_fraction_initial_cases=-2.0, save_path="unused",
               parameters={}, **kw)


def test_runner_takes_the_key_at_construction_and_from_the_yaml(monkeypatch):
    from grad_june_amd import runner as RN

    plain = _runner()
    assert plain.locations_saved is False and plain.location_keys == []
    assert plain._locations() == {}                                  # absent: nothing to allocate, clone or launch
    on = _runner(locations=True, groups=["area"])
    assert on.locations_saved is True and on.location_keys == NETWORKS + ["background", "seed"]
    with pytest.raises(ValueError, match="true or false"):
        _runner(locations="all")
    data = plain.data
    monkeypatch.setattr(RN.Runner, "get_data", staticmethod(lambda params: data))
    monkeypatch.setattr(RN.GradJune, "from_parameters", classmethod(lambda cls, params: _Model()))
    monkeypatch.setattr(RN.Timer, "from_parameters", classmethod(lambda cls, params: None))
    params = {"infection_seed": {"log_fraction_initial_cases": -2.0}, "save_path": "unused"}
    assert RN.Runner.from_parameters(dict(params)).locations_saved is False
    assert RN.Runner.from_parameters(dict(params, locations_to_save=False)).locations_saved is False
    assert RN.Runner.from_parameters(dict(params, locations_to_save=True)).location_keys == NETWORKS + ["background", "seed"]


def test_a_partitioned_run_refuses_the_key():
    from grad_june_amd.distributed_api import DistributedRunner

    params = {"infection_seed": {"log_fraction_initial_cases": -2.0}, "save_path": "unused", "locations_to_save": True}
    with pytest.raises(NotImplementedError, match="partitioned"):
        DistributedRunner.from_parameters(params)                    # before a world is loaded or a device is touched
    with pytest.raises(NotImplementedError, match="partitioned"):
        _runner(DistributedRunner, locations=True)
    assert _runner(DistributedRunner).locations_saved is False


def test_the_model_has_the_sink_and_it_is_off():
    import inspect

    from grad_june_amd.model import GradJune

    assert "self.location_stats = None" in inspect.getsource(GradJune.__init__)
