"""CPU: the restatement of the infector attribution (tests/gj_infector_ref.py) against its own definition, and the host
logic of the ``infectors_to_save`` key.  The GPU tests hold the kernels to this restatement."""
import math

import numpy as np
import pytest

import gj_infector_ref as I
import gj_location_ref as R
from test_location_ref import _Model, _runner as _location_runner


def small_world(A=40, seed=0, exact=True):
    """Two edge sets - `home` (one network) and `leisure` (three networks, 5 venues) - on A agents; every seventh agent
    has no edge."""
    rng = np.random.default_rng(seed)
    lonely = np.arange(A) % 7 == 6
    agents = np.arange(A)[~lonely]
    home = (rng.permutation(agents), None)
    home = (home[0], rng.integers(0, max(1, A // 3), len(home[0])))
    going = rng.permutation(np.repeat(agents, rng.integers(0, 4, len(agents))))
    edges = {"home": home, "leisure": (going, rng.integers(0, 5, len(going)))}
    draw = (lambda shape: rng.integers(0, 1025, shape) / 256.0) if exact else (lambda shape: rng.random(shape) * 3.0)
    cum = {"home": draw((max(1, A // 3), 1)).astype(np.float32), "leisure": draw((5, 3)).astype(np.float32)}
    pc = {s: (rng.random(c.shape[0]) * 0.5 + 0.01).astype(np.float32) for s, c in cum.items()}
    age = rng.integers(0, 100, A)
    table = draw((3, A))
    q = (rng.random(A) < 0.8).astype(np.float64)
    nets = [I.Net("home", 0, 0.5, np.ones(A), np.ones(A))]
    for k in range(3):
        m = q * table[k]
        nets.append(I.Net("leisure", k, 0.25 * (k + 1), m * (age > 75) if k == 2 else m, m))      # k == 2: care_visit
    s0 = draw(A)
    s0[rng.random(A) < 0.2] = 0.0
    return dict(A=A, edges=edges, cum=cum, pc=pc, nets=nets, s0=s0, age=age, q=q)


@pytest.mark.parametrize("exact", [True, False])
def test_units_sum_to_the_attributed_infections_exactly(exact):
    w = small_world(exact=exact, seed=3)
    nu = (np.random.default_rng(1).random(w["A"]) < 0.6).astype(np.float32)
    units, lost, err, touched = I.scatter(w["nets"], w["edges"], w["cum"], w["s0"], nu, w["A"])
    assert err == 0 and 0 < lost < nu.sum()
    assert sum(int(u.sum()) for u in units.values()) == I.U * (int(nu.sum()) - lost)
    assert all((u >= 0).all() for u in units.values())
    assert all(not u[touched[s] == 0].any() for s, u in units.items())      # only venues a new infection attends


def test_the_decision_is_the_location_series_decision():
    w = small_world(seed=5)
    rows = I.rows_of(w["edges"], w["A"])
    ones = np.ones(w["A"], np.float32)
    lost = 0
    for a in range(w["A"]):
        t = I.location_terms(w["nets"], rows, w["cum"], w["s0"], a)
        _, background, _ = R.shares(t)
        only = np.zeros(w["A"], np.float32)
        only[a] = 1.0
        units, un, _, _ = I.scatter(w["nets"], w["edges"], w["cum"], w["s0"], only, w["A"])
        assert un == (1 if background else 0), a
        assert sum(int(u.sum()) for u in units.values()) == (0 if background else I.U)
        # per network, the units scattered are the location series' shares up to the floors of the edges
        share, _, _ = R.shares(t)
        for i, net in enumerate(w["nets"]):
            got = int(units[net.set][:, net.column].sum())
            assert abs(got - share[i]) <= len(rows[net.set][a]) * len(w["nets"]) + len(w["nets"]), (a, i)
        lost += un
    assert 0 < lost < w["A"]
    assert I.scatter(w["nets"], w["edges"], w["cum"], w["s0"], ones, w["A"])[1] == lost


def test_the_remainder_goes_to_the_largest_term_lowest_network_then_lowest_position():
    A = 1
    edges = {"x": (np.zeros(3, np.int64), np.array([2, 0, 1])), "y": (np.zeros(1, np.int64), np.array([0]))}
    one = np.ones(A)
    nets = [I.Net("x", 0, 1.0, one, one), I.Net("x", 1, 1.0, one, one), I.Net("y", 0, 1.0, one, one)]
    # seven equal terms: x col 0 at venues 2, 0, 1; x col 1 at the same; y at venue 0.  2^30 = 7 * 153391689 + 1
    cum = {"x": np.ones((3, 2), np.float32), "y": np.ones((1, 1), np.float32)}
    units, lost, err, _ = I.scatter(nets, edges, cum, np.ones(1), np.ones(1, np.float32), A)
    f = I.U // 7
    assert lost == 0 and err == 0 and I.U - 7 * f == 1
    assert units["x"].tolist() == [[f, f], [f, f], [f + 1, f]] and units["y"].tolist() == [[f]]      # position 0 is venue 2
    cum["x"][1, 1] = 2.0                      # a strictly largest term takes it wherever it is
    units, _, _, _ = I.scatter(nets, edges, cum, np.ones(1), np.ones(1, np.float32), A)
    f = I.U // 8
    assert units["x"].tolist() == [[f, f], [f, 2 * f], [f, f]] and I.U == 8 * f
    cum["y"][0, 0] = 2.0                      # a tie of two largest: the lower network
    units, _, _, _ = I.scatter(nets, edges, cum, np.ones(1), np.ones(1, np.float32), A)
    f = I.U // 9
    rest = I.U - 9 * f
    assert rest > 0 and units["x"][1, 1] == 2 * f + rest and units["y"][0, 0] == 2 * f


def test_care_visit_masks_the_receiving_side_only():
    A = 2                                      # agent 0: 80 years old, agent 1: 30; both visit venue 0
    edges = {"leisure": (np.array([0, 1]), np.array([0, 0]))}
    age = np.array([80, 30])
    m = np.array([0.5, 0.25])
    nets = [I.Net("leisure", 0, 2.0, m * (age > 75), m)]
    cum = {"leisure": np.array([[0.125]], np.float32)}
    pc = {"leisure": np.array([0.5], np.float32)}
    s0 = np.ones(A)
    units, lost, _, _ = I.scatter(nets, edges, cum, s0, np.array([0, 1], np.float32), A)
    assert lost == 1 and not units["leisure"].any()                 # the young visitor cannot be infected there
    units, lost, _, _ = I.scatter(nets, edges, cum, s0, np.array([1, 0], np.float32), A)
    assert lost == 0 and units["leisure"][0, 0] == I.U
    credit, out, err = I.gather(nets, edges, cum, pc, units, np.array([0.0, 0.5], np.float32), A)
    # ... but transmits there: 1 * (2 * 0.5) * (0.25 * 0.5) / 0.125
    assert err == 0 and credit.tolist() == [0.0, 1.0] and out == [I.U]


def test_an_agent_without_edges_and_a_step_without_networks():
    w = small_world(seed=7)
    lonely = np.zeros(w["A"], np.float32)
    lonely[6] = lonely[13] = 1.0
    units, lost, err, _ = I.scatter(w["nets"], w["edges"], w["cum"], np.ones(w["A"]), lonely, w["A"])
    assert lost == 2 and err == 0 and not any(u.any() for u in units.values())
    nu = np.ones(w["A"], np.float32)
    nu[3], nu[4] = 2.0, np.nan
    units, lost, err, _ = I.scatter([], w["edges"], w["cum"], w["s0"], nu, w["A"])      # the seeding step
    assert lost == w["A"] - 2 and err == I.ERR_VALUE and not any(u.any() for u in units.values())
    credit, out, err = I.gather([], w["edges"], w["cum"], w["pc"], units, np.ones(w["A"], np.float32), w["A"])
    assert not credit.any() and out == [0] and err == 0


def test_credits_of_a_venue_sum_to_its_units_when_cum_is_the_exact_sum():
    """cum = beta * pc * sum of m * transmission in fp64 (no fp32 rounding inside): the credits conserve the infections
    to fp64 rounding.  (The kernels' cum carries fp32 roundings; tests/test_gpu_infector_series.py measures what they cost.)"""
    w = small_world(A=60, seed=11, exact=False)
    A, nets = w["A"], w["nets"]
    rng = np.random.default_rng(2)
    tr = (rng.random(A) * (rng.random(A) < 0.4)).astype(np.float32)
    cum = {s: np.zeros(c.shape) for s, c in w["cum"].items()}
    for net in nets:
        agent, venue = w["edges"][net.set]
        np.add.at(cum[net.set][:, net.column], venue, (net.m * tr)[agent])
        cum[net.set][:, net.column] *= float(np.float32(net.beta)) * w["pc"][net.set].astype(np.float64)
    nu = ((tr == 0) & (rng.random(A) < 0.7)).astype(np.float32)
    units, lost, err, _ = I.scatter(nets, w["edges"], cum, np.ones(A), nu, A)
    credit, out, err2 = I.gather(nets, w["edges"], cum, w["pc"], units, tr, A, group=np.arange(A) % 3, n_groups=3)
    attributed = int(nu.sum()) - lost
    assert err == err2 == 0 and attributed >= 5
    assert abs(credit.sum() - attributed) <= 1e-12 * attributed
    assert not credit[tr == 0].any()
    assert abs(sum(out) - I.U * attributed) <= (tr > 0).sum()
    for g in range(3):
        assert abs(out[g] - credit[np.arange(A) % 3 == g].sum() * I.U) <= (tr > 0).sum()


# ---- host logic -------------------------------------------------------------------------------------------------------------
def _runner(cls=None, **kw):
    return _location_runner(cls, **kw)


def test_yaml_key():
    from grad_june_amd.groups import infectors_to_save

    assert infectors_to_save(None) is False and infectors_to_save(False) is False and infectors_to_save(True) is True
    assert infectors_to_save(np.bool_(True)) is True
    for bad in ("yes", 1, 0, ["household"], "true"):
        with pytest.raises(ValueError, match="true or false"):
            infectors_to_save(bad)


def test_runner_takes_the_key_at_construction_and_from_the_yaml(monkeypatch):
    from grad_june_amd import runner as RN

    plain = _runner()
    assert plain.infectors_saved is False and plain._infectors() is None      # absent: nothing to allocate or launch
    assert _runner(infectors=True, groups=["area"]).infectors_saved is True
    with pytest.raises(ValueError, match="true or false"):
        _runner(infectors="all")
    data = plain.data
    monkeypatch.setattr(RN.Runner, "get_data", staticmethod(lambda params: data))
    monkeypatch.setattr(RN.GradJune, "from_parameters", classmethod(lambda cls, params: _Model()))
    monkeypatch.setattr(RN.Timer, "from_parameters", classmethod(lambda cls, params: None))
    params = {"infection_seed": {"log_fraction_initial_cases": -2.0}, "save_path": "unused"}
    assert RN.Runner.from_parameters(dict(params)).infectors_saved is False
    assert RN.Runner.from_parameters(dict(params, infectors_to_save=False)).infectors_saved is False
    on = RN.Runner.from_parameters(dict(params, infectors_to_save=True))
    assert on.infectors_saved is True and on.locations_saved is False


def test_a_partitioned_run_refuses_the_key():
    from grad_june_amd.distributed_api import DistributedRunner

    params = {"infection_seed": {"log_fraction_initial_cases": -2.0}, "save_path": "unused", "infectors_to_save": True}
    with pytest.raises(NotImplementedError, match="partitioned"):
        DistributedRunner.from_parameters(params)                    # before a world is loaded or a device is touched
    with pytest.raises(NotImplementedError, match="partitioned"):
        _runner(DistributedRunner, infectors=True)
    assert _runner(DistributedRunner).infectors_saved is False


def test_the_model_has_the_sink_and_it_is_off():
    import inspect

    from grad_june_amd.model import GradJune

    assert "self.infector_stats = None" in inspect.getsource(GradJune.__init__)


def test_argument_errors_do_not_need_a_gpu():
    """A NULL plan is refused before anything touches the device, by all three entry points."""
    from grad_june_amd import _native as N

    lib = N.load()
    assert lib.gj_infector_scatter(None, None, None, None, None, None, None, None, None, 0, None, None) == -1
    assert lib.gj_infector_gather(None, None, None, None, None, None, None, 1, None, None, None, None) == -1
    assert lib.gj_infector_clear(None, None, None, None, None) == -1
    assert math.log2(N.GJ_LOC_UNIT) == 30 and I.U == N.GJ_LOC_UNIT
    assert (I.ERR_LABEL, I.ERR_VALUE, I.ERR_ROWS) == (N.GJ_LOC_ERR_LABEL, N.GJ_LOC_ERR_VALUE, N.GJ_LOC_ERR_ROWS)
