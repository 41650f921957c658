"""GPU: the Testing policy in the whole model, on the 769-agent world for 30 days.  The Runner with the ``testing`` key
against the same model without it, where the test itself applies the rule with torch ops (on the same Philox uniforms) at
the launch's place - every series, the per-agent state and the step's mask per step, bit for bit - the invariants of
tests/test_testing.py on the run itself, runs that must change nothing, the closed-form gradient of the probability,
``log_beta.grad`` through the confirmed series against float64 autograd, and two gloo ranks against one GPU."""
import datetime
import itertools

import numpy as np
import pytest
import torch

import gj_philox_ref as P
import gj_testing_ref as R
from grad_june_amd import _native as N

pytestmark = pytest.mark.gpu

DAYS, LOG_FRACTION, LOG_BETA_SHIFT = 30, -2.0, 1.0
THRESHOLD = 4      # symptomatic
PROBABILITY = {"0-18": 0.3, "18-65": 0.5, "65-100": 0.8}
DELAY = {1: 0.2, 2: 0.5, 3: 0.3}
#: the run starts 2022-02-01: two steps before the window, and a week of results arriving after it
WINDOW = {"start_date": "2022-02-03", "end_date": "2022-02-24"}
TESTING = dict(WINDOW, stage_threshold=THRESHOLD, probability=PROBABILITY, delay=DELAY,
               isolation={"days": 5, "compliance": 0.8})
WHOLE_RUN = {"start_date": "2022-02-01", "end_date": "2023-01-01"}


def _params(device, testing=None, days=DAYS, groups=None, quarantine=None):
    from grad_june_amd.defaults import default_parameters

    p = default_parameters(str(device))
    p["timer"]["total_days"] = days
    p["infection_seed"]["log_fraction_initial_cases"] = LOG_FRACTION
    for n in p["networks"]:
        p["networks"][n]["log_beta"] += LOG_BETA_SHIFT
    if testing is not None:
        p["policies"]["testing"] = {"testing": testing}
    if quarantine is not None:
        p["policies"]["quarantine"] = {"quarantine": quarantine}
    if groups:
        p["groups_to_save"] = list(groups)
    return p


def _fresh_runner(device, seed=21, cls=None, **kw):
    import grad_june_amd as G
    from grad_june_amd import infection

    torch.manual_seed(seed)
    infection._philox_step = itertools.count(1 << 40)
    return (cls or G.Runner).from_parameters(_params(device, **kw))


def _run(runner, grad=False, seed=21):
    from grad_june_amd import infection

    torch.manual_seed(seed)
    infection._philox_step = itertools.count(1 << 40)      # the seeding's Philox stream: the same for every run
    with torch.set_grad_enabled(grad):
        return runner()


def _log_beta_parameters(runner):
    nets = runner.model.infection_networks.networks
    for net in nets.values():
        net.log_beta = torch.nn.Parameter(net.log_beta.detach().clone())
    return [net.log_beta for net in nets.values()]


def _policy(runner):
    return runner.model.policies.testing_policies.policies[0]


class Emulation:
    """The rule restated with torch ops on a model WITHOUT the key, at the launch's place: ``QuarantinePolicies.apply`` is
    wrapped, and after it the emulation decides, reports and - with isolation - leaves its mask in ``qstate``, where the
    step reads it.  The uniforms are the restatement's (tests/gj_philox_ref.py), of the deciding agents alone.  ``y`` is
    float64 on the graph: ``hard * stage / stage.detach()`` plus an exact zero that carries ``d / d probability = 1``;
    ``probability`` is a float64 leaf [B]."""

    def __init__(self, runner, testing):
        import grad_june_amd.policies as GP

        self.runner, self.dev = runner, runner.device
        self.parsed = GP.Testing(**testing)
        self.table = torch.from_numpy(R.probability_table(testing["probability"]) if isinstance(testing["probability"], dict)
                                      else np.full(100, testing["probability"], np.float32)).to(self.dev)
        cum, days = R.delay_tables(testing.get("delay", 0))
        self.cum, self.days = torch.from_numpy(cum).to(self.dev), torch.from_numpy(days).to(self.dev)
        self.probability = self.parsed.probability.double().to(self.dev).requires_grad_(True)
        self.age = runner.data["agent"].age.to(self.dev).long()
        self.band = torch.tensor(self.parsed.band_of_age, device=self.dev)[self.age]
        qp = runner.model.policies.quarantine_policies
        real = qp.apply

        def apply(symptom_stages, timer):
            real(symptom_stages=symptom_stages, timer=timer)
            self(qp, symptom_stages, timer)

        qp.apply = apply
        self.reset()

    def reset(self):
        n, dev = self.age.numel(), self.dev
        self.started = False
        self.decided = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.result_time = torch.full((n,), float("inf"), device=dev)
        self.y = torch.zeros(n, dtype=torch.float64, device=dev)
        self.isolate_until = torch.zeros(n, device=dev)
        self.confirmed_time = torch.full((n,), -1.0, device=dev)
        self.rows, self.confirmed, self.decisions, self.isolating, self.masks = [], [0], [0], [0], []
        self.by_band_decided = torch.zeros(3, dtype=torch.int64)

    def __call__(self, qp, stage, timer):
        active = self.parsed.is_active(timer.date)
        self.started = self.started or active
        if not self.started:
            self.confirmed.append(0), self.decisions.append(0), self.isolating.append(0), self.masks.append(None)
            self.rows.append(torch.zeros((), dtype=torch.float64, device=self.dev))
            return
        model, dev = self.runner.model, self.dev
        seed = model.rng_seed if model.rng_seed is not None else torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
        now = torch.tensor(timer.now, dtype=torch.float32, device=dev)
        st = stage.detach().float()
        bits = self.runner.data["agent"].infection_time.detach().float().contiguous().view(torch.int32)
        deciding = ~(st < float(self.parsed.stage_threshold)) & (bits != self.decided) & bool(active)
        idx = torch.nonzero(deciding)[:, 0]
        u0, u1 = R.decision_words(seed, R.decide_stream(0), idx.cpu().numpy().astype(np.uint64),
                                  bits[idx].cpu().numpy().view(np.uint32))
        u0, u1 = torch.from_numpy(u0).to(dev), torch.from_numpy(u1).to(dev)
        hard = (u0 < self.table[self.age[idx]]).double()
        k = (self.cum[None, :-1] <= u1[:, None]).sum(1)      # the first entry whose threshold exceeds u
        self.decided[idx] = bits[idx]
        self.result_time[idx] = now + self.days[k]      # one float32 add
        s64 = stage.double()[idx]
        p = self.probability[self.band[idx].clamp(min=0)]
        in_band = (self.band[idx] >= 0).double()
        y = self.y.clone()
        y[idx] = hard * s64 / s64.detach() + (p - p.detach()) * in_band
        self.y = y
        due = self.result_time <= now
        self.result_time[due] = float("inf")
        newly = due & (self.y.detach() != 0)
        self.rows.append((due.double() * self.y).sum())
        self.confirmed_time[newly] = now
        self.confirmed.append(int(newly.sum())), self.decisions.append(int(deciding.sum()))
        self.by_band_decided += torch.bincount(self.band[idx].cpu(), minlength=3)
        mask = None
        if self.parsed.isolates:
            who = torch.nonzero(newly)[:, 0]
            u = (P.infection_uniform(seed, R.comply_stream(0), who.cpu().numpy().astype(np.uint64)) if len(who)
                 else np.zeros(0, np.float32))
            comply = torch.from_numpy(u).to(dev) < torch.tensor(self.parsed.compliance, dtype=torch.float32, device=dev)
            release = torch.tensor(timer.now + self.parsed.isolation_days, dtype=torch.float64).to(torch.float32).to(dev)
            self.isolate_until[who[comply]] = release
            mask = torch.where(~(st < qp.threshold), 1.0, torch.where(now < self.isolate_until, 3.0, 0.0)).float()
            qp.qstate = mask
        self.isolating.append(0 if mask is None else int((mask == 3).sum()))
        self.masks.append(mask)


def _spy_on_masks(runner):
    """The mask and the stage of every ``Policies.test`` of the runner's model, in order."""
    policies, seen = runner.model.policies, {"masks": [], "stages": []}
    real = policies.test

    def test(data, timer, **kw):
        seen["stages"].append(data["agent"]["symptoms"]["current_stage"].detach().clone())
        real(data, timer, **kw)
        q = policies.quarantine_policies.qstate
        seen["masks"].append(None if q is None else q.clone())

    policies.test = test
    return seen


_STATE = ("susceptibility", "is_infected", "infection_time")
_SYMPTOMS = ("current_stage", "next_stage", "time_to_next_stage")


def _same_run(res_a, inf_a, a, res_b, inf_b, b):
    assert res_a["dates"] == res_b["dates"] and len(res_b) >= 6
    for k, v in res_b.items():
        if k != "dates":
            assert torch.equal(res_a[k].detach(), v.detach()), k
    assert torch.equal(inf_a, inf_b)
    for k in _STATE:
        assert torch.equal(a.data["agent"][k].detach(), b.data["agent"][k].detach()), k
    for k in _SYMPTOMS:
        assert torch.equal(a.data["agent"]["symptoms"][k].detach(), b.data["agent"]["symptoms"][k].detach()), k


def test_runner_against_the_torch_op_emulation(device, tmp_path):
    """Every result series of the emulated run and the final per-agent state, bit for bit; the new series, the policy's
    per-agent state and the step's mask in every step against the emulation's own.  The floors of tests/test_testing.py
    hold on the run itself, so the comparison is not an empty one; a plain Quarantine over the window's first days puts
    value 1 into the mask."""
    import pandas as pd

    quarantine = {"start_date": "2022-02-03", "end_date": "2022-02-12", "stage_threshold": THRESHOLD}
    a = _fresh_runner(device, testing=TESTING, groups=["area"], quarantine=quarantine)
    b = _fresh_runner(device, groups=["area"], quarantine=quarantine)
    hook, seen = Emulation(b, TESTING), _spy_on_masks(a)
    (res_a, inf_a), (res_b, inf_b) = _run(a), _run(b)
    _same_run(res_a, inf_a, a, res_b, inf_b, b)
    T = len(res_a["dates"])
    assert T == DAYS + 1 == len(hook.confirmed)
    # floors
    tp = a.model.policies.testing_policies
    state = tp.state(0)
    decided = state["decided"] != -1
    positives, decisions = int((state["positive"] != 0).sum()), int(decided.sum())
    print("decisions", decisions, "positives", positives, "confirmed", sum(hook.confirmed), "by band",
          hook.by_band_decided.tolist(), "isolating agent-steps", sum(hook.isolating))
    assert positives >= 40 and decisions - positives >= 40 and hook.by_band_decided.min() >= 3
    assert decisions == sum(hook.decisions) == int(a._confirmed_series[:T, 1].sum())
    # the new series
    national = res_a["confirmed_cases_per_timestep"]
    assert national.dtype == torch.int64 and national.tolist() == hook.confirmed and national[0] == 0
    assert 0 < national.sum() <= positives and not national[:3].any()      # nothing before the window, and a delay >= 1
    assert national[23:].sum() > 0      # results keep arriving after the window (its last active step is row 22)
    by_area = res_a["confirmed_cases_by_area"]
    assert by_area.dtype == torch.int64 and by_area.shape == (T, len(a.group_keys["area"]))
    assert torch.equal(by_area.sum(1), national) and (by_area.sum(0) > 0).sum() >= 2
    assert res_a["isolating_per_timestep"].tolist() == hook.isolating and sum(hook.isolating) > 0
    assert torch.equal(res_a["isolating_by_area"].sum(1), res_a["isolating_per_timestep"])
    assert "quarantined_index_per_timestep" not in res_a
    # the per-agent state, and the mask of every step
    assert torch.equal(state["decided"], hook.decided) and torch.equal(state["result_time"], hook.result_time)
    assert torch.equal(state["positive"], hook.y.detach().float())
    assert torch.equal(tp.isolate_until, hook.isolate_until) and torch.equal(tp.confirmed_time, hook.confirmed_time)
    assert len(seen["masks"]) == len(hook.masks) == DAYS
    values = set()
    for got, ref in zip(seen["masks"], hook.masks):
        assert (got is None) == (ref is None)
        if ref is not None:
            assert torch.equal(got, ref)
            values |= set(ref.unique().tolist())
    assert values == {0.0, 1.0, 3.0} and seen["masks"][0] is None and seen["masks"][-1] is not None
    confirmed_time = a.data["agent"]["confirmed_time"]
    index = a.data["agent"].original_index.to(device).long() if "original_index" in a.data["agent"] else torch.arange(a.n_agents, device=device)
    assert torch.equal(confirmed_time[index], hook.confirmed_time) and int((confirmed_time >= 0).sum()) == int(national.sum())
    # isolation reaches the step: everybody found at once and held for the rest of the run changes the epidemic
    plain, _ = _run(_fresh_runner(device))
    held, _ = _run(_fresh_runner(device, testing=dict(WHOLE_RUN, stage_threshold=THRESHOLD, probability=1, delay=0,
                                                      isolation={"days": DAYS})))
    print("cases at the end: no policy", float(plain["cases_per_timestep"][-1]), "this run", float(res_a["cases_per_timestep"][-1]),
          "everybody held", float(held["cases_per_timestep"][-1]))
    assert "confirmed_cases_per_timestep" not in plain
    assert not torch.equal(plain["cases_per_timestep"], held["cases_per_timestep"])
    a.save_path = tmp_path / "out"
    a.save_results(res_a, inf_a)
    df = pd.read_csv(tmp_path / "out" / "results.csv")
    assert df["confirmed_cases_per_timestep"].tolist() == national.tolist()
    assert df["isolating_per_timestep"].tolist() == hook.isolating
    areas = pd.read_csv(tmp_path / "out" / "results_by_area.csv")
    assert areas["confirmed_cases"].tolist() == by_area.reshape(-1).tolist()
    assert areas["isolating"].tolist() == res_a["isolating_by_area"].reshape(-1).tolist()
    lines = pd.read_csv(tmp_path / "out" / "results_confirmed.csv")
    assert list(lines.columns) == ["agent", "date"] and len(lines) == int(national.sum())
    when = confirmed_time.cpu().numpy()
    first = lines.iloc[0]
    assert first["date"].startswith(str((res_a["dates"][0] + datetime.timedelta(days=float(when[first["agent"]]))).date()))


def test_full_ascertainment_without_delay_counts_everybody_at_the_threshold(device):
    """probability 1, delay 0, the window the whole run: the cumulative confirmed count at row k equals the number of
    agents seen at or above the threshold by the launches of the rows up to k - the stages the rows before k left - and
    the rows by group sum to the national row."""
    a = _fresh_runner(device, testing=dict(WHOLE_RUN, stage_threshold=THRESHOLD, probability=1, delay=0), groups=["area"])
    seen = _spy_on_masks(a)
    res, _ = _run(a)
    at = torch.stack(seen["stages"]) >= THRESHOLD      # [launch, agent]; launch j belongs to row j + 1
    reached = torch.cummax(at.long(), 0).values.sum(1)
    national = res["confirmed_cases_per_timestep"]
    assert torch.cumsum(national, 0)[1:].tolist() == reached.tolist() and national[0] == 0 and reached[-1] >= 80
    assert torch.equal(res["confirmed_cases_by_area"].sum(1), national)
    assert "isolating_per_timestep" not in res and all(m is None for m in seen["masks"])


def test_two_windows_and_a_contact_quarantine_after_them(device):
    """Numbered windows: the first isolates, the second does not; both report into one series, the first's isolations
    outlast its window, and a ContactQuarantine that is active later overrides the mask in its own steps."""
    p = _params(device, testing={
        1: {"start_date": "2022-02-03", "end_date": "2022-02-12", "stage_threshold": THRESHOLD, "probability": 1, "delay": 0,
            "isolation": {"days": 6}},
        2: {"start_date": "2022-02-12", "end_date": "2022-02-18", "stage_threshold": THRESHOLD, "probability": 0.5,
            "delay": 1}})
    p["policies"]["quarantine"] = {"contact_quarantine": {"start_date": "2022-02-16", "end_date": "2022-02-23",
                                                          "stage_threshold": THRESHOLD, "contacts": {"household": 7}}}
    import grad_june_amd as G

    runner = G.Runner.from_parameters(p)
    res, _ = _run(runner)
    confirmed, isolating = res["confirmed_cases_per_timestep"], res["isolating_per_timestep"]
    index, contacts = res["quarantined_index_per_timestep"], res["quarantined_contacts_per_timestep"]
    print("confirmed", confirmed.tolist(), "isolating", isolating.tolist(), "index", index.tolist())
    # rows: 2022-02-01 is row 0; a window [start, end) holds the rows start .. end - 1
    # (the windows' rows: 2 .. 10, 11 .. 16, and the ContactQuarantine's 15 .. 21)
    assert not confirmed[:2].any() and confirmed[2:11].sum() > 0 and confirmed[12:18].sum() > 0 and not confirmed[19:].any()
    first = int(torch.nonzero(confirmed)[0])
    assert 2 <= first <= 9 and not isolating[:first].any() and (isolating[first:first + 6] > 0).all()      # six days each
    assert not isolating[15:22].any() and (index[15:22] > 0).all() and contacts[15:22].sum() > 0      # the ContactQuarantine's mask
    assert not index[:15].any() and not index[22:].any() and not contacts[:15].any()
    tp = runner.model.policies.testing_policies
    first, second = tp.state(0), tp.state(1)
    assert (first["decided"] != -1).sum() > 0 and (second["decided"] != -1).sum() > 0
    assert (first["positive"] != 0).sum() == (first["decided"] != -1).sum()      # probability 1
    assert 0 < (second["positive"] != 0).sum() < (second["decided"] != -1).sum()
    assert 0 < int((tp.confirmed_time >= 0).sum()) <= int(confirmed.sum())


@pytest.mark.parametrize("which", ["no-isolation", "probability-0"])
def test_runs_that_must_change_nothing(device, which, monkeypatch):
    """A Testing without ``isolation``, and one with isolation that finds nobody (probability 0): every other result
    series, the final state and ``log_beta.grad`` are the bits of the run without the policy, which itself calls no
    gj_testing* symbol and allocates nothing."""
    lib = N.load()
    calls = []

    def spy(name):
        real = getattr(lib, name)

        def wrapped(*args):
            calls.append(name)
            return real(*args)

        return wrapped

    for name in ("gj_testing_step", "gj_adjoint_testing"):
        monkeypatch.setattr(lib, name, spy(name))
    testing = dict(TESTING)
    if which == "no-isolation":
        del testing["isolation"]
    else:
        testing["probability"] = 0
    days = 14

    def loss(res):
        return res["cases_per_timestep"].sum() + res["deaths_per_timestep"].sum()

    for grad in (False, True):
        plain = _fresh_runner(device, days=days)
        lb_ref = _log_beta_parameters(plain) if grad else None
        ref, ref_inf = _run(plain, grad)
        assert calls == [] and plain.model.policies.testing_policies.isolate_until is None
        assert not any(k.startswith(("confirmed", "isolating")) for k in ref)
        runner = _fresh_runner(device, days=days, testing=testing)
        lb = _log_beta_parameters(runner) if grad else None
        res, inf = _run(runner, grad)
        assert "gj_testing_step" in calls      # (the loss below does not read the confirmed series: no adjoint launch)
        _same_run(res, inf, runner, ref, ref_inf, plain)
        if which == "no-isolation":
            assert res["confirmed_cases_per_timestep"].sum() > 0 and "isolating_per_timestep" not in res
        else:
            assert not res["confirmed_cases_per_timestep"].any() and not res["isolating_per_timestep"].any()
        if grad:
            loss(ref).backward()
            loss(res).backward()
            assert lb_ref[0].grad is not None and lb_ref[0].grad != 0
            for pa, pb in zip(lb, lb_ref):
                assert torch.equal(pa.grad, pb.grad), (pa.grad, pb.grad)
        calls.clear()


def test_closed_form_gradient_of_the_probability(device):
    """A fixed delay and the loss ``confirmed_cases_per_timestep.sum()``: ``probability.grad[b]`` is the number of
    decisions in band b whose result fell due within the run, exactly - every decision counts 1, positive or negative."""
    testing = dict(TESTING, delay=2)
    a = _fresh_runner(device, testing=testing)
    policy = _policy(a)
    policy.probability = torch.nn.Parameter(policy.probability.detach().clone())
    res, _ = _run(a, grad=True)
    series = res["confirmed_cases_per_timestep"]
    assert series.requires_grad and series.dtype == torch.float32
    series.sum().backward()
    state = a.model.policies.testing_policies.state(0)
    reported = (state["decided"] != -1) & torch.isinf(state["result_time"])
    pending = (state["decided"] != -1) & ~torch.isinf(state["result_time"])
    band = torch.tensor(policy.band_of_age, device=device)[a.data["agent"].age.to(device).long()]
    expected = torch.bincount(band[reported], minlength=3).tolist()
    print("probability.grad", policy.probability.grad.tolist(), "expected", expected, "pending", int(pending.sum()))
    assert policy.probability.grad.tolist() == [float(v) for v in expected] and min(expected) >= 3
    # the same run without a gradient gives the same counts
    b = _fresh_runner(device, testing=testing)
    plain, _ = _run(b)
    assert plain["confirmed_cases_per_timestep"].tolist() == series.detach().tolist()


#: measured on MI355X (printed with -s): the largest relative difference between log_beta.grad through the kernels and
#: autograd's through the float64 torch ops on this world, over its 10 non-zero gradients, is 0.0 - the emulation's
#: float64 quotient ``g * hard / stage`` rounded to float32 is the kernel's float32 quotient for every deciding agent of
#: the run, and behind the stage both runs go through the same symptoms, sampler and profile adjoints.  The tolerance is
#: four times the measured value, the project's convention: here that is equality
MEASURED_GRADIENT_AGREEMENT = 0.0
#: ``probability.grad`` is a float32 parameter's: autograd adds the launches' float64 sums into it in float32, one
#: rounding of at most 2^-24 relative per launch (all terms are positive)
PROBABILITY_GRADIENT_TOLERANCE = DAYS * 2.0 ** -24
WEIGHTS = (0.5, 1.5)


def _weighted(series):
    # (float32 weights for either dtype of the series: the float64 emulation sums the same numbers)
    return (series * torch.linspace(*WEIGHTS, series.numel(), device=series.device).to(series.dtype)).sum()


def test_log_beta_gradient_through_the_confirmed_series(device):
    """``log_beta`` parameters and the probability as an nn.Parameter, the loss a weighted sum of the confirmed series
    alone: ``log_beta.grad`` and ``probability.grad`` against float64 autograd through the emulation's torch ops.
    Measured on MI355X: the largest relative difference over the 10 non-zero ``log_beta`` gradients was 0.0, so the test
    holds them to equality (four times the measured value); ``probability.grad`` to the float32 accumulation's bound."""
    a = _fresh_runner(device, testing=TESTING)
    b = _fresh_runner(device)
    hook = Emulation(b, TESTING)
    policy = _policy(a)
    policy.probability = torch.nn.Parameter(policy.probability.detach().clone())
    lb_a, lb_b = _log_beta_parameters(a), _log_beta_parameters(b)
    (res_a, _), (res_b, _) = _run(a, grad=True), _run(b, grad=True)
    for k in ("cases_per_timestep", "deaths_per_timestep"):
        assert torch.equal(res_a[k].detach(), res_b[k].detach()), k
    confirmed_b = torch.stack([torch.zeros((), dtype=torch.float64, device=device), *hook.rows])
    assert res_a["confirmed_cases_per_timestep"].detach().tolist() == confirmed_b.detach().tolist() == hook.confirmed
    _weighted(res_a["confirmed_cases_per_timestep"]).backward()
    _weighted(confirmed_b).backward()
    worst, nonzero = 0.0, 0
    for pa, pb in zip(lb_a, lb_b):
        assert pa.grad is not None and pb.grad is not None
        g, r = float(pa.grad), float(pb.grad)
        assert (g == 0.0) == (r == 0.0), (g, r)
        if r != 0.0:
            nonzero += 1
            worst = max(worst, abs(g - r) / abs(r))
    got, ref = policy.probability.grad.double().cpu(), hook.probability.grad.cpu()
    print("log_beta.grad through the confirmed series: largest relative difference", worst, "non-zero", nonzero,
          "probability.grad", got.tolist(), ref.tolist())
    assert nonzero >= 2 and (ref > 0).all()
    assert ((got - ref).abs() <= PROBABILITY_GRADIENT_TOLERANCE * ref).all(), (got, ref)
    assert worst <= 4 * MEASURED_GRADIENT_AGREEMENT, worst


# ---- two ranks ----------------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, R_, port, out):
    import os

    import torch.distributed as dist

    import grad_june_amd as G
    from grad_june_amd import infection
    from grad_june_amd.distributed_api import DistributedRunner

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=R_)
    try:
        testing = {k: v for k, v in TESTING.items() if k != "isolation"}      # (a partitioned run refuses the isolation)
        params = lambda: _params("cuda:0", testing=testing, groups=["area"])

        def run(runner):
            policy = _policy(runner)
            policy.probability = torch.nn.Parameter(policy.probability.detach().clone())
            results, _ = runner()
            _weighted(results["confirmed_cases_per_timestep"]).backward()
            return results, policy.probability.grad.tolist()

        torch.manual_seed(33)
        res, grads = run(DistributedRunner.from_parameters(params()))
        gathered = [None] * R_
        dist.all_gather_object(gathered, grads)
        assert gathered[0] == gathered[1], "every rank holds the whole gradient"
        if rank == 0:
            torch.manual_seed(33)
            infection._philox_step = itertools.count(1 << 40)
            ref_res, ref = run(G.Runner.from_parameters(params()))
            for k in ("cases_per_timestep", "confirmed_cases_per_timestep", "confirmed_cases_by_area"):
                assert torch.equal(res[k].detach().cpu(), ref_res[k].detach().cpu()), k
            assert ref_res["confirmed_cases_per_timestep"].sum() > 0
            assert all(v != 0.0 for v in ref) and grads == pytest.approx(ref, rel=1e-6), (grads, ref)
            with pytest.raises(NotImplementedError, match="isolation"):
                DistributedRunner.from_parameters(_params("cuda:0", testing=TESTING))
            out[0] = 1
    finally:
        dist.destroy_process_group()


def test_two_ranks_reproduce_the_single_gpu_series_and_probability_gradient(device):
    import os

    import torch.multiprocessing as mp

    out = mp.get_context("spawn").Array("i", [0])
    mp.spawn(_two_rank_worker, args=(2, 29900 + os.getpid() % 90, out), nprocs=2, join=True)
    assert out[0] == 1
