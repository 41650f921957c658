"""GPU: the ContactQuarantine policy through the model and the Runner, on the bundled 769-agent world (355 households,
745 household edges).  The mask of a step against the numpy restatement (tests/gj_contact_ref.py) and the step's
probabilities against the float64 sparse passes fed that mask; compliance 0 against a plain Quarantine, bit for bit;
compliance 1 household by household over the days; the result series; the differentiable run; the location series; and
the partitioned run's refusal."""
import itertools

import numpy as np
import pytest
import torch

import gj_contact_ref as R
import gj_testlib as L

pytestmark = pytest.mark.gpu

THRESHOLD = 4
WINDOW = ("2022-02-04", "2022-02-10")       # rows 3 .. 8 of a run that starts on 2022-02-01


def _params(device, days=12, window=("2022-02-01", "2022-03-01"), contacts=None, compliance=1.0, threshold=THRESHOLD,
            plain=False, **extra):
    from grad_june_amd.defaults import default_parameters

    p = default_parameters(str(device))
    p["timer"]["total_days"] = days
    p["infection_seed"]["log_fraction_initial_cases"] = -1.3
    for n in p["networks"]:
        p["networks"][n]["log_beta"] += 0.6
    where = {"start_date": window[0], "end_date": window[1], "stage_threshold": threshold}
    if plain:
        p["policies"]["quarantine"] = {"quarantine": where}
    else:
        p["policies"]["quarantine"] = {"contact_quarantine": dict(where, contacts=contacts or {"household": 14},
                                                                  compliance=compliance)}
    p.update(extra)
    return p


def _runner(params, seed=21):
    import grad_june_amd as G
    from grad_june_amd import infection

    torch.manual_seed(seed)
    infection._philox_step = itertools.count(1 << 40)
    return G.Runner.from_parameters(params)


def _recording(runner):
    """Keeps a copy of the mask every step hands the hot path (None for a step without an active ContactQuarantine)."""
    qp = runner.model.policies.quarantine_policies
    real, seen = qp.contact_step, []

    def contact_step(*args, **kwargs):
        q = real(*args, **kwargs)
        seen.append(None if q is None else q.detach().clone())
        return q

    qp.contact_step = contact_step
    return seen


def _households(runner):
    ei = runner.data["attends_household"].edge_index.cpu().numpy()
    return ei[0], ei[1], len(runner.data["household"]["people"])


def _seeded(runner):
    """The runner after its seeding step, the timer on the first step's date."""
    runner.timer.reset()
    runner.model.policies.reset()
    runner.restore_initial_data()
    runner.set_initial_cases()
    next(runner.timer)
    return runner.data, runner.timer, runner.model


def _world_of(runner):
    data = runner.data
    world = {"n_agents": runner.n_agents, "age": data["agent"].age.cpu(), "sex": data["agent"].sex.cpu(), "edge_sets": {}}
    for s in L.EDGE_SETS:
        if "attends_" + s in data:
            ei = data["attends_" + s].edge_index.cpu()
            world["edge_sets"][s] = {"agent": ei[0], "venue": ei[1], "people": data[s]["people"].cpu()}
    tables = {}
    for name, net in runner.model.infection_networks.networks.items():
        spec = net.spec()
        if spec.table is not None:
            tables[name] = torch.from_numpy(np.asarray(spec.table, dtype=np.float32).reshape(2, 2, 100))
    return world, tables


def test_the_steps_mask_and_probabilities(device):
    """(a) One step with a handful of symptomatic agents: ``quarantine_mask`` equals the restatement's mask, and the
    step's not_infected_probs agree with gj_testlib.sparse_passes_fp64 fed that mask within rtol 2e-5, atol 1e-9 - the
    tolerance tests/test_gpu_api.py holds a plain Quarantine's probabilities to (measured on MI355X: max |dp| = 4.9e-8,
    printed with -s)."""
    runner = _runner(_params(device, compliance=0.7))
    n = runner.n_agents
    assert n == 769
    with torch.no_grad():
        data, timer, model = _seeded(runner)
        agent, venue, n_households = _households(runner)
        assert n_households == 355 and len(agent) == 745
        stage = data["agent"].symptoms["current_stage"].clone()
        infected = torch.nonzero(data["agent"].is_infected > 0.5).flatten()[:6]
        stage[infected] = torch.tensor([4, 4, 5, 6, 4, 7], device=stage.device, dtype=stage.dtype)[: len(infected)]
        data["agent"].symptoms["current_stage"] = stage
        s0 = data["agent"].susceptibility.detach().clone().cpu().numpy().astype(np.float64)
        model.rng_seed = 0xC0FFEE
        new, probs = model.hot_path(data, timer, want_probs=True)
    qp = model.policies.quarantine_policies
    rowptr, by_agent = R.csr_by_agent(agent, venue, n)
    sets = [{"rowptr": rowptr, "venue": by_agent, "until": np.zeros(n_households, np.uint32), "days": 14.0}]
    st = stage.cpu().numpy().astype(np.float32)
    (until,), _ = R.mark(st, THRESHOLD, sets, timer.now)
    u = R.uniforms(0xC0FFEE, R.stream_of(0), 0, n)
    q_ref, _ = R.mask(st, THRESHOLD, [dict(sets[0], until=until)], timer.now, 0.7, u)
    assert np.array_equal(qp.qstate.cpu().numpy(), q_ref)
    assert (q_ref == 1.0).sum() == len(infected) and 0 < (q_ref == 2.0).sum()
    cases = infected.cpu().numpy()
    housemates = np.zeros(n, dtype=bool)
    housemates[agent[np.isin(venue, venue[np.isin(agent, cases)])]] = True
    housemates[cases] = False
    assert np.array_equal(q_ref == 2.0, housemates & (u < np.float32(0.7))) and housemates.sum() >= 3
    mask_ref = (q_ref < 0.5).astype(np.float32)
    assert np.array_equal(qp.quarantine_mask.cpu().numpy(), mask_ref)
    assert qp.launch_threshold == 0.5 and qp.threshold == THRESHOLD
    assert np.array_equal(qp._contact[0]["until"][0].cpu().numpy().view(np.uint32), until)
    # the step computed what the reference computes under that mask
    world, tables = _world_of(runner)
    active = [net.name for net in model.infection_networks.active_networks(timer, model.policies)]
    betas = {net: model.infection_networks.networks[net].beta_value(model.policies, timer) for net in active}
    x = data["agent"].transmission.cpu().numpy()
    assert (x > 0).sum() >= len(infected)
    ref = L.sparse_passes_fp64(world, active, betas, tables, 0 if timer.day_type == "weekday" else 1, mask_ref, x,
                               transpose=False)
    p_ref = np.exp(-np.clip(ref["out"] * s0, 1e-6, 100.0) * timer.duration)
    got = probs.cpu().numpy()
    print("max |dp| =", float(np.abs(got - p_ref).max()))
    assert np.allclose(got, p_ref, rtol=2e-5, atol=1e-9)
    # ... and not what it computes under the index cases' mask alone
    plain = L.sparse_passes_fp64(world, active, betas, tables, 0 if timer.day_type == "weekday" else 1,
                                 (st < THRESHOLD).astype(np.float32), x, transpose=False)
    assert not np.allclose(got, np.exp(-np.clip(plain["out"] * s0, 1e-6, 100.0) * timer.duration), rtol=2e-5, atol=1e-9)
    qp.check()


def _differentiable_run(params):
    runner = _runner(params)
    net = runner.model.infection_networks.networks["household"]
    net.log_beta = torch.nn.Parameter(net.log_beta.detach().clone())
    seen = _recording(runner) if runner.model.policies.quarantine_policies.contact_policies else None
    results, is_infected = runner()
    T = len(results["dates"])
    w = torch.linspace(0.5, 1.5, T, device=results["cases_per_timestep"].device)
    ((w * results["cases_per_timestep"]).sum() + results["deaths_per_timestep"].sum()).backward()
    return runner, results, is_infected, net.log_beta.grad.detach().cpu().numpy(), seen


def test_compliance_zero_is_a_plain_quarantine_bit_for_bit(device):
    """(b) Nobody complies: every result of a full run and d loss / d log_beta equal, bit for bit, the same
    configuration with a plain ``quarantine`` of the same window and threshold (3: index cases from the first days)."""
    kw = dict(days=10, window=WINDOW, threshold=3)
    runner, res, inf, grad, seen = _differentiable_run(_params(device, compliance=0.0, **kw))
    _, plain, inf_plain, grad_plain, _ = _differentiable_run(_params(device, plain=True, **kw))
    assert set(res) - set(plain) == {"quarantined_index_per_timestep", "quarantined_contacts_per_timestep"}
    for key, value in plain.items():
        assert value == res[key] if key == "dates" else torch.equal(value, res[key]), key
    assert torch.equal(inf, inf_plain)
    assert grad.tobytes() == grad_plain.tobytes() and float(grad) != 0.0
    assert int(res["quarantined_index_per_timestep"].sum()) > 0 and int(res["quarantined_contacts_per_timestep"].sum()) == 0
    assert sum(q is not None for q in seen) == 6 and all(not (q == 2.0).any() for q in seen if q is not None)


def test_households_are_held_for_the_days_and_then_released(device):
    """(c) Everybody complies, 3 days: while an agent is symptomatic every other member of its household is a contact;
    they remain so for 3 days after its stage drops, and are free at the first step with now >= release."""
    runner = _runner(_params(device, contacts={"household": 3}))
    with torch.no_grad():
        data, timer, model = _seeded(runner)
        agent, venue, _ = _households(runner)
        sizes = np.bincount(venue)
        homes = np.nonzero(sizes >= 3)[0][:4]                        # four households of three or more
        cases = np.array([agent[venue == h][0] for h in homes])
        others = np.setdiff1d(agent[np.isin(venue, homes)], cases)
        outside = np.setdiff1d(np.arange(runner.n_agents), agent[np.isin(venue, homes)])
        assert len(others) >= 8
        qp = model.policies.quarantine_policies
        states = {}
        for step in range(7):                                         # now = 1 .. 7; symptomatic at now = 1 and 2
            stage = torch.ones(runner.n_agents, device=device)
            if timer.now <= 2:
                stage[torch.from_numpy(cases).to(device)] = 5.0
            data["agent"].symptoms["current_stage"] = stage
            model.hot_path(data, timer)
            states[timer.now] = qp.qstate.cpu().numpy().copy()
            next(timer)
    release = 2 + 3
    for now, q in states.items():
        assert (q[outside] == 0.0).all(), now
        assert (q[cases] == (1.0 if now <= 2 else 2.0 if now < release else 0.0)).all(), now
        assert (q[others] == (2.0 if now < release else 0.0)).all(), now
    assert sorted(states) == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    qp.check()


@pytest.fixture(scope="module")
def series_run(device):
    """A run whose window covers rows 3 .. 8, by area, locations saved, the masks recorded; shared, never modified."""
    runner = _runner(_params(device, window=WINDOW, threshold=3, compliance=0.8, groups_to_save=["area"],
                             locations_to_save=True))
    seen = _recording(runner)
    from grad_june_amd import infection

    with torch.no_grad():
        first = runner()
        masks = list(seen)
        # the same key AND the same streams again: the steps', the symptoms' and the seeding's counters go on counting
        runner.model.n_steps, runner.model.symptoms_updater.n_calls = 0, 0
        infection._philox_step = itertools.count(1 << 40)
        second = runner()
    return runner, first, masks, second


def test_runner_series(device, series_run, tmp_path):
    """(d) By-group rows sum to the national row exactly; both series are counts of the per-step mask; rows outside the
    window are zero; a second run of the same runner gives the same results (``reset`` clears ``until``)."""
    runner, (res, inf), masks, (again, inf_again) = series_run
    T = len(res["dates"])
    index, contacts = res["quarantined_index_per_timestep"], res["quarantined_contacts_per_timestep"]
    assert index.shape == contacts.shape == (T,) and index.dtype == contacts.dtype == torch.int64
    assert not index.requires_grad
    by_index, by_contacts = res["quarantined_index_by_area"], res["quarantined_contacts_by_area"]
    assert by_index.shape == by_contacts.shape == (T, 3) and by_index.dtype == torch.int64
    assert torch.equal(by_index.sum(1), index) and torch.equal(by_contacts.sum(1), contacts)
    assert len(masks) == T - 1
    area = runner.data["agent"].group_labels["area"].cpu().numpy()
    inside = np.array([WINDOW[0] <= d.strftime("%Y-%m-%d") < WINDOW[1] for d in res["dates"]])
    assert inside.sum() == 6 and not inside[0]
    for row in range(T):
        q = masks[row - 1] if row else None
        assert (q is not None) == bool(inside[row]), row
        for value, nat, by in ((1.0, index, by_index), (2.0, contacts, by_contacts)):
            want = np.zeros(3, dtype=np.int64) if q is None else np.bincount(area[q.cpu().numpy() == value], minlength=3)
            assert np.array_equal(by[row].cpu().numpy(), want) and int(nat[row]) == want.sum(), (row, value)
    assert int(index[inside].sum()) > 0 and int(contacts[inside].sum()) > 0
    assert int(contacts[inside][0]) > 0 or int(index[inside][0]) == 0      # (what a stale ``until`` would change first)
    for key, value in res.items():
        assert value == again[key] if key == "dates" else torch.equal(value, again[key]), key
    assert torch.equal(inf, inf_again)
    import pandas as pd

    runner.save_path = tmp_path
    runner.save_results(res, inf)
    flat = pd.read_csv(tmp_path / "results.csv")
    assert np.array_equal(flat["quarantined_contacts_per_timestep"].to_numpy(), contacts.cpu().numpy())
    long = pd.read_csv(tmp_path / "results_by_area.csv")
    assert np.array_equal(long["quarantined_index"].to_numpy().reshape(T, 3), by_index.cpu().numpy())


def test_location_series_still_sum_to_the_daily_cases(device, series_run):
    """(f) With the policy on, every row of the infection-location series sums to the day's new cases, exactly."""
    runner, (res, _), _, _ = series_run
    T = len(res["dates"])
    units = runner._locations()[None].out[:T].cpu().numpy()
    daily = res["daily_cases_per_timestep"].cpu().numpy().astype(np.int64)
    assert daily[1:].sum() > 20 and np.array_equal(units[:, 0].sum(1), (1 << 30) * daily)


def test_a_differentiable_run_hands_the_step_the_same_mask(device):
    """(e) Step by step the differentiable run's ``qstate`` is the no_grad run's."""
    kw = dict(days=8, window=("2022-02-02", "2022-02-08"), threshold=3, compliance=0.8)
    _, res, _, grad, seen = _differentiable_run(_params(device, **kw))
    runner = _runner(_params(device, **kw))
    plain_seen = _recording(runner)
    with torch.no_grad():
        runner()
    assert len(seen) == len(plain_seen) == 8 and np.isfinite(grad).all() and float(grad) != 0.0
    active = 0
    for a, b in zip(seen, plain_seen):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        active += a is not None and bool((a == 2.0).any())
    assert active >= 3


def test_an_unknown_edge_set_is_a_key_error_at_the_first_step(device):
    runner = _runner(_params(device, days=3, contacts={"household": 14, "barracks": 7}))
    with torch.no_grad(), pytest.raises(KeyError, match="barracks"):
        runner()


def test_a_partitioned_run_refuses_the_policy(device):
    """(g)"""
    from grad_june_amd.distributed_api import DistributedRunner

    with pytest.raises(NotImplementedError, match="contact_quarantine.*partitioned run"):
        DistributedRunner.from_parameters(_params(device), rank=0, world_size=2, collectives=False)
