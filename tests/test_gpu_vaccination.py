"""GPU: the Vaccination policy.  gj_vaccinate and gj_adjoint_vaccinate against their numpy restatement
(tests/gj_vaccination_ref.py) over the shapes at which the kernels change form, then the whole model: the Runner with the
policy against the same model without it, where the test itself multiplies the susceptibility with torch ops before every
step - series and final state bit for bit, d loss / d efficacy against autograd through the torch ops - the dose series,
a config without the policy, and two gloo ranks against one GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import gj_vaccination_ref as V
from grad_june_amd import _native as N

pytestmark = pytest.mark.gpu

SEED, CAMPAIGN = 0x7654321, 3
COVERAGE = {"18-65": 0.6, "65-100": 0.9}                  # ages below 18: a gap
EFFICACY = {"65-100": 0.6, "30-65": 0.8}                  # ages 18-29: covered, but in no efficacy band
#: (coverage of every age or None = COVERAGE, lo, hi): nobody, everybody, a middle slice
SLICES = [(None, 0.3, 0.3), (1.0, 0.0, 1.0), (None, 0.25, 0.7)]


def _coverage_tables(coverage, lo, hi):
    from grad_june_amd.utils import parse_age_probabilities

    cov = [coverage] * 100 if coverage is not None else parse_age_probabilities(COVERAGE)
    band = [int(b) for b in parse_age_probabilities({k: i for i, k in enumerate(EFFICACY)}, fill_value=-1)]
    return V.tables(cov, band, np.array(list(EFFICACY.values()), dtype=np.float32), lo, hi), band


def _c_tables(tabs):
    t = N.VaccinateTables()
    for dst, src in zip((t.thr_lo, t.thr_hi, t.factor), tabs):
        dst[:] = [float(v) for v in src]
    return t


def _dev(a, device, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)


def _agents(n, rng):
    """(agent classes sex * 100 + age, ages, susceptibility): every age 0 .. 99 met where n allows, some agents at 0."""
    age = rng.integers(0, 100, n)
    cls = (rng.integers(0, 2, n) * 100 + age).astype(np.uint8)
    susc = np.where(rng.random(n) < 0.6, 1.0, rng.random(n)).astype(np.float32)
    susc[2::5] = 0.0
    return cls, age, susc


def _vaccinate(device, cls, susc, tabs, offset, want_newly=True, count_start=None):
    n = len(cls)
    s, k = _dev(susc, device), _dev(cls, device)
    newly = torch.full((n,), float("nan"), device=device) if want_newly else None
    count = None if count_start is None else torch.tensor([count_start], dtype=torch.int64, device=device)
    N.check(N.load().gj_vaccinate(n, N.ptr(k), _c_tables(tabs), SEED, V.stream_of(CAMPAIGN), offset, N.ptr(s),
                                  N.ptr(newly), N.ptr(count), N.current_stream()), "gj_vaccinate")
    torch.cuda.synchronize()
    return (s.cpu().numpy(), None if newly is None else newly.cpu().numpy(), None if count is None else int(count.item()))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1003, 9001])
def test_kernel_against_the_restatement(device, n):
    """Updated susceptibility and newly_out bit for bit, count_out exact and added onto a non-zero start, NULL outputs
    accepted (9001: several workgroups of 1024 lanes in either form).  agent_offset 0 and 8 (four agents per lane, one Philox block) and 5 (one agent per lane: an odd offset
    moves the blocks' boundaries); ages in bands and in gaps; agents at susceptibility 0; the three slices."""
    rng = np.random.default_rng(100 + n)
    cls, age, susc = _agents(n, rng)
    moved = 0
    for (coverage, lo, hi), offset in itertools.product(SLICES, (0, 5, 8)):
        tabs, _ = _coverage_tables(coverage, lo, hi)
        u = V.uniforms(SEED, V.stream_of(CAMPAIGN), offset, n)
        ref_s, ref_new = V.vaccinate(susc, age, tabs, u)
        got_s, got_new, count = _vaccinate(device, cls, susc, tabs, offset, count_start=1000)
        assert np.array_equal(got_s.view(np.int32), ref_s.view(np.int32)), (coverage, lo, hi, offset)
        assert np.array_equal(got_new, ref_new.astype(np.float32))
        assert count == 1000 + int(ref_new.sum())
        only_s, none_new, none_count = _vaccinate(device, cls, susc, tabs, offset, want_newly=False)
        assert none_new is None and none_count is None and np.array_equal(only_s.view(np.int32), ref_s.view(np.int32))
        if lo == hi:
            assert not ref_new.any() and np.array_equal(got_s.view(np.int32), susc.view(np.int32))
        if coverage == 1.0:
            assert ref_new.all()
        moved += int(ref_new.sum())
    assert moved >= 3 * n


def test_a_run_of_slices_moves_every_agent_once(device):
    """In place, launch after launch, as the policy drives it: the slices' masks are disjoint and their union is the
    [0, final) slice's; the susceptibility after the run is the one launch's."""
    rng = np.random.default_rng(7)
    n = 1003
    cls, age, susc = _agents(n, rng)
    ramps = [0.0, 0.2, 0.2, 0.55, 1.0]
    s, seen = susc, np.zeros(n)
    for lo, hi in zip(ramps, ramps[1:]):
        s, new, _ = _vaccinate(device, cls, s, _coverage_tables(None, lo, hi)[0], 8)
        seen += new
    once_s, once_new, _ = _vaccinate(device, cls, susc, _coverage_tables(None, 0.0, 1.0)[0], 8)
    assert np.array_equal(seen, once_new) and 0 < once_new.sum() < n
    assert np.array_equal(s.view(np.int32), once_s.view(np.int32))


def _adjoint(device, cls, susc0, g_out, band, n_bands, tabs, offset, want_g_in=True):
    from grad_june_amd.groups import SeedPlan

    n = len(cls)
    lab = _dev(band, device, np.int32)
    plan = SeedPlan(lab, n_bands, device=device)
    contrib = torch.full((max(1, n),), float("nan"), dtype=torch.float64, device=device)
    partial = torch.full((max(1, plan.n_chunks),), float("nan"), dtype=torch.float64, device=device)
    out = torch.full((n_bands,), float("nan"), dtype=torch.float64, device=device)
    g_in = torch.full((n,), float("nan"), device=device) if want_g_in else None
    keep = [_dev(cls, device), _dev(susc0, device), _dev(g_out, device)]
    N.check(N.load().gj_adjoint_vaccinate(n, N.ptr(keep[0]), _c_tables(tabs), SEED, V.stream_of(CAMPAIGN), offset,
                                          N.ptr(keep[1]), N.ptr(keep[2]), N.ptr(lab), n_bands, C.byref(plan.c),
                                          N.ptr(contrib), N.ptr(partial), N.ptr(out), N.ptr(g_in), N.current_stream()),
            "gj_adjoint_vaccinate")
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if g_in is None else g_in.cpu().numpy(), plan


def _check_adjoint(device, cls, age, susc0, g_out, band, n_bands, nonempty=True):
    """Every slice, offset 0 / 5 / 8, g_out given and NULL: per band |kernel - float64 restatement| <= 1e-6 * sum |c_a|
    (the bound gj_adjoint_seed is held to: the fp32 factor is the only rounding upstream of the fp64 sum), two launches
    the same bits, g_in the restatement's bit for bit."""
    n = len(cls)
    total = 0.0
    for (coverage, lo, hi), offset, given in itertools.product(SLICES, (0, 5, 8), (True, False)):
        tabs, _ = _coverage_tables(coverage, lo, hi)
        u = V.uniforms(SEED, V.stream_of(CAMPAIGN), offset, n)
        g = g_out if given else None
        ref = V.adjoint(susc0, g, age, band, n_bands, tabs, u)
        got, g_in, _ = _adjoint(device, cls, susc0, g, band, n_bands, tabs, offset)
        again, none_in, _ = _adjoint(device, cls, susc0, g, band, n_bands, tabs, offset, want_g_in=False)
        assert none_in is None and np.array_equal(got.view(np.int64), again.view(np.int64)), "two launches differ"
        err, bound = np.abs(got - ref["grad_efficacy"]), 1e-6 * ref["abs_sum"]
        assert np.all(err <= bound), (coverage, lo, hi, offset, given, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.array_equal(g_in.view(np.int32), ref["g_in"].view(np.int32))
        if not given:
            assert not got.any() and not g_in.any()
        total += float(ref["abs_sum"].sum())
    assert total > 0 or not nonempty


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1003])
def test_adjoint_against_the_restatement(device, n):
    """The bands as the policy forms them (each agent's age's band; ages 18-29 and some agents by hand have none)."""
    rng = np.random.default_rng(200 + n)
    cls, age, susc0 = _agents(n, rng)
    g_out = rng.standard_normal(n).astype(np.float32)
    band = np.asarray(_coverage_tables(None, 0.0, 1.0)[1])[age]
    band[3::7] = [-1, 2, 2 ** 31 - 1][n % 3]                  # labels outside [0, 2): no band, never an index
    _check_adjoint(device, cls, age, susc0, g_out, band, 2, nonempty=n > 1)      # (one agent: its age may be in a gap)


@pytest.mark.parametrize("which", ["one-2500", "mixed", "mixed-sorted"])
def test_adjoint_bands_of_several_chunks(device, which):
    """Bands that span several (band, chunk) partials of GJ_SEED_CHUNK = 1024 agents: one band of 2500 (3 chunks), and
    sizes 3000, 1, 0, 1025, 1024, 950, 2049 - shuffled and sorted - next to 500 agents with no band."""
    rng = np.random.default_rng(len(which))
    if which == "one-2500":
        n_bands, band = 1, np.zeros(2500, dtype=np.int64)
    else:
        sizes = [3000, 1, 0, 1025, 1024, 950, 2049]
        n_bands = len(sizes)
        band = rng.permutation(np.concatenate((np.repeat(np.arange(n_bands), sizes), np.full(500, -1))))
        if which == "mixed-sorted":
            band = np.sort(band)
    n = len(band)
    cls, age, susc0 = _agents(n, rng)
    g_out = rng.standard_normal(n).astype(np.float32)
    _, _, plan = _adjoint(device, cls, susc0, g_out, band, n_bands, _coverage_tables(1.0, 0.0, 1.0)[0], 0)
    sizes = np.bincount(band[band >= 0], minlength=n_bands)
    assert plan.n_chunks == int(np.ceil(sizes / N.GJ_SEED_CHUNK).sum()) and plan.n_sorted == int(sizes.sum())
    _check_adjoint(device, cls, age, susc0, g_out, band, n_bands)


# ---- the whole model ----------------------------------------------------------------------------------------------------
#: the timer starts on 2022-02-01: campaign 0 straddles the run (ramp 0.5 at the first step, 1 from day 3 on), campaign 1
#: is an empty window inside it (everybody it covers at once, on day 2)
CAMPAIGNS = {1: {"start_date": "2022-01-30", "end_date": "2022-02-04", "coverage": COVERAGE, "efficacy": EFFICACY},
             2: {"start_date": "2022-02-03", "end_date": "2022-02-03", "coverage": 0.3, "efficacy": 0.5}}
DONE_BEFORE = {"start_date": "2022-01-10", "end_date": "2022-01-20", "coverage": COVERAGE, "efficacy": EFFICACY}


def _params(device, vaccination=None, days=4, groups=None, save_path=None):
    from grad_june_amd.defaults import default_parameters

    p = default_parameters(str(device))
    p["timer"]["total_days"] = days
    p["infection_seed"]["log_fraction_initial_cases"] = -1.2
    for n in p["networks"]:
        p["networks"][n]["log_beta"] += 0.6
    p["policies"] = dict(p.get("policies") or {})
    if vaccination is not None:
        p["policies"]["vaccination"] = {"vaccination": vaccination}
    if groups:
        p["groups_to_save"] = list(groups)
    if save_path is not None:
        p["save_path"] = str(save_path)
    return p


def _fresh_runner(device, seed=21, cls=None, **kw):
    import grad_june_amd as G
    from grad_june_amd import infection

    torch.manual_seed(seed)
    infection._philox_step = itertools.count(1 << 40)
    return (cls or G.Runner).from_parameters(_params(device, **kw))


def _log_beta_parameters(runner):
    nets = runner.model.infection_networks.networks
    for net in nets.values():
        net.log_beta = torch.nn.Parameter(net.log_beta.detach().clone())
    return [net.log_beta for net in nets.values()]


class Emulation:
    """The policy restated with torch ops, as a forward pre-hook of a model WITHOUT it: before every ``model(data,
    timer)`` the susceptibility is multiplied by ``where(newly, 1 - eff[band], 1)`` with ``newly`` from the numpy
    restatement.  ``eff``: one float32 tensor per campaign (a leaf, for the gradient tests)."""

    def __init__(self, runner, campaigns, seed, agent_offset=0, leaf_susceptibility=False):
        from grad_june_amd.policies import Vaccination

        self.runner, self.seed, self.offset = runner, seed, agent_offset
        self.policies = [Vaccination(**w) for w in campaigns]          # parsing only: coverage, bands, ramp
        self.eff = [p.efficacy.clone().to(runner.device).requires_grad_(True) for p in self.policies]
        self.age = runner.data["agent"].age.cpu().numpy().astype(np.int64)
        self.masks, self.leaf, self.leaf_susceptibility = [], None, leaf_susceptibility
        runner.model.register_forward_pre_hook(self)

    def reset(self):
        self.applied = [0.0] * len(self.policies)
        self.masks, self.total = [], np.zeros(len(self.policies), dtype=np.int64)

    def __call__(self, model, args):
        data, timer = args[0], args[1]
        ag, dev, n = data["agent"], self.runner.device, len(self.age)
        for c, p in enumerate(self.policies):
            hi = V.ramp(timer.date, p.start_date, p.end_date)
            if not hi > self.applied[c]:
                continue
            tabs = V.tables(p.coverage, p.band_of_age, p.efficacy.numpy(), self.applied[c], hi)
            newly = V.newly(V.uniforms(self.seed, V.stream_of(c), self.offset, n), self.age, *tabs[:2])
            self.applied[c] = hi
            self.masks.append(newly)
            self.total[c] += int(newly.sum())
            band = torch.tensor(p.band_of_age, device=dev)[torch.from_numpy(self.age).to(dev)]
            factor = torch.where(band >= 0, 1.0 - self.eff[c][band.clamp(min=0)], torch.ones((), device=dev))
            w = torch.where(torch.from_numpy(newly).to(dev), factor, torch.ones((), device=dev))
            self.s0 = ag.susceptibility.detach().clone()
            ag.susceptibility = ag.susceptibility * w
            if self.leaf_susceptibility:      # the updated susceptibility as a per-agent leaf: its .grad is g_s
                self.leaf = ag.susceptibility = ag.susceptibility.detach().requires_grad_(True)
                self.newly, self.band = newly, band.cpu().numpy()


def _run_pair(device, campaigns, grad, leaf=False, groups=None):
    """(results and is_infected of run A, the Runner with the policy; of run B, the emulation; A's runner; B's hook)."""
    a = _fresh_runner(device, vaccination=dict(enumerate(campaigns, 1)), groups=groups)
    b = _fresh_runner(device, groups=groups)
    hook = Emulation(b, campaigns, seed=21, leaf_susceptibility=leaf)
    params_a = params_b = None
    if grad:
        for policy in a.model.policies.vaccination_policies.policies:
            policy.efficacy = torch.nn.Parameter(policy.efficacy.detach().clone())
        params_a, params_b = _log_beta_parameters(a), _log_beta_parameters(b)
    from grad_june_amd import infection

    out = []
    for runner in (a, b):
        torch.manual_seed(21)
        infection._philox_step = itertools.count(1 << 40)      # the seeding's Philox stream: the same for both
        hook.reset()
        with torch.set_grad_enabled(grad):
            out.append(runner())
    return out[0], out[1], a, hook, params_a, params_b


def test_runner_against_the_torch_op_emulation(device):
    """Every result series of the run without the policy and the final is_infected, bit for bit; the masks of the newly
    vaccinated are non-empty on more than one step (the comparison is not vacuous) and the epidemic differs from the
    unvaccinated one."""
    (res_a, inf_a), (res_b, inf_b), a, hook, _, _ = _run_pair(device, list(CAMPAIGNS.values()), grad=False)
    assert sum(1 for m in hook.masks if m.any()) >= 3 and len(hook.masks) >= 4
    assert res_a["dates"] == res_b["dates"] and len(res_b) >= 6
    for k, v in res_b.items():
        if k != "dates":
            assert torch.equal(res_a[k], v), k
    assert torch.equal(inf_a, inf_b)
    assert res_a["vaccine_doses_by_campaign"][-1].tolist() == hook.total.tolist() and hook.total.min() > 0
    with torch.no_grad():
        plain, _ = _fresh_runner(device)()
    assert not torch.equal(plain["cases_per_timestep"], res_a["cases_per_timestep"])
    # a second forward of the same runner starts again from nothing applied (the doses depend on the run's key and the
    # dates alone, not on the steps' streams, which go on counting)
    with torch.no_grad():
        res_again, _ = a()
    assert torch.equal(res_again["vaccine_doses_by_campaign"], res_a["vaccine_doses_by_campaign"])


def _loss(results):
    return results["cases_per_timestep"].sum() + results["deaths_per_timestep"].sum()


def test_gradients_against_autograd_through_the_emulation(device):
    """d loss / d efficacy of run A (gj_adjoint_vaccinate) against run B's (torch ops) at the project's gradient-parity
    tolerance, rel 2e-5 (abs 1e-7); d loss / d log_beta bit for bit.  Measured on MI355X: the largest relative
    difference over the three efficacies was 8.2e-8 (printed with -s)."""
    (res_a, _), (res_b, _), a, hook, lb_a, lb_b = _run_pair(device, list(CAMPAIGNS.values()), grad=True)
    assert res_a["cases_per_timestep"].requires_grad
    assert torch.equal(res_a["cases_per_timestep"].detach(), res_b["cases_per_timestep"].detach())
    _loss(res_a).backward()
    _loss(res_b).backward()
    worst = 0.0
    for policy, eff in zip(a.model.policies.vaccination_policies.policies, hook.eff):
        got, ref = policy.efficacy.grad.cpu().tolist(), eff.grad.cpu().tolist()
        assert len(got) == len(ref) and all(r != 0.0 for r in ref), (got, ref)
        for g, r in zip(got, ref):
            worst = max(worst, abs(g - r) / abs(r))
            assert g == pytest.approx(r, rel=2e-5, abs=1e-7), (got, ref)
    print("efficacy gradients: largest relative difference", worst)
    for pa, pb in zip(lb_a, lb_b):
        assert pa.grad is not None and pa.grad != 0 and torch.equal(pa.grad, pb.grad), (pa.grad, pb.grad)


def test_gradient_of_a_campaign_that_finished_before_the_first_step(device):
    """Everybody the campaign covers is vaccinated in the first step.  With the updated susceptibility a per-agent leaf
    in run B, g_s = its .grad, grad_efficacy[b] = -sum g_s[a] * s0[a] over the vaccinated agents of band b, within 1e-6 *
    sum |g_s[a] * s0[a]| (s0, the susceptibility before the update, is 1 but for the seeded agents, where it is 0: the
    sum is -sum g_s[a] over the vaccinated agents that were still susceptible)."""
    (res_a, _), (res_b, _), a, hook, _, _ = _run_pair(device, [DONE_BEFORE], grad=True, leaf=True)
    assert len(hook.masks) == 1 and hook.masks[0].sum() > 100
    assert torch.equal(res_a["cases_per_timestep"].detach(), res_b["cases_per_timestep"].detach())
    _loss(res_a).backward()
    _loss(res_b).backward()
    g_s, s0 = hook.leaf.grad.double().cpu().numpy(), hook.s0.double().cpu().numpy()
    assert set(np.unique(s0)) <= {0.0, 1.0}
    got = a.model.policies.vaccination_policies[0].efficacy.grad.double().cpu().numpy()
    for b in range(2):
        mine = hook.newly & (hook.band == b)
        ref, scale = -(g_s[mine] * s0[mine]).sum(), np.abs(g_s[mine] * s0[mine]).sum()
        assert scale > 0 and abs(got[b] - ref) <= 1e-6 * scale, (b, got[b], ref, scale)


def test_dose_series(device, tmp_path):
    """By-group rows and by-campaign rows sum to the national series exactly; it starts at zero, never falls and ends at
    the restatement's count; save_results writes the columns."""
    import pandas as pd

    (res, inf), _, a, hook, _, _ = _run_pair(device, list(CAMPAIGNS.values()), grad=False, groups=["area"])
    national = res["vaccine_doses_per_timestep"]
    T = len(res["dates"])
    assert national.shape == (T,) and res["vaccine_doses_by_campaign"].shape == (T, 2)
    assert res["vaccine_doses_by_area"].shape == (T, len(a.group_keys["area"]))
    assert national[0] == 0 and (torch.diff(national) >= 0).all() and national[-1] == int(hook.total.sum()) > 0
    assert torch.equal(res["vaccine_doses_by_area"].sum(1), national)
    assert torch.equal(res["vaccine_doses_by_campaign"].sum(1), national)
    assert torch.equal(national, national.round()) and not national.requires_grad
    assert (res["vaccine_doses_by_area"][-1] > 0).sum() >= 2
    a.save_path = tmp_path / "out"
    a.save_results(res, inf)
    df = pd.read_csv(tmp_path / "out" / "results.csv")
    assert df["vaccine_doses_per_timestep"].tolist() == national.tolist()
    assert df["vaccine_doses_campaign_1"].tolist() == res["vaccine_doses_by_campaign"][:, 1].tolist()
    by_area = pd.read_csv(tmp_path / "out" / "results_by_area.csv")
    assert by_area["vaccine_doses"].tolist() == res["vaccine_doses_by_area"].reshape(-1).tolist()
    # a differentiable run records the same counts
    (res_g, _), _, _, _, _, _ = _run_pair(device, list(CAMPAIGNS.values()), grad=True, groups=["area"])
    assert torch.equal(res_g["vaccine_doses_by_area"], res["vaccine_doses_by_area"])
    assert torch.equal(res_g["vaccine_doses_by_campaign"], res["vaccine_doses_by_campaign"])


def test_no_policy_launches_nothing_and_coverage_zero_changes_nothing(device, monkeypatch):
    lib = N.load()
    calls = []

    def spy(name):
        real = getattr(lib, name)

        def wrapped(*args):
            calls.append(name)
            return real(*args)

        return wrapped

    monkeypatch.setattr(lib, "gj_vaccinate", spy("gj_vaccinate"))
    monkeypatch.setattr(lib, "gj_adjoint_vaccinate", spy("gj_adjoint_vaccinate"))
    plain = _fresh_runner(device)
    assert plain._campaigns() is None
    with torch.no_grad():
        ref, ref_inf = plain()
    lb = _log_beta_parameters(plain)
    torch.manual_seed(21)
    _loss(plain()[0]).backward()                              # a differentiable run: neither entry either
    assert calls == [] and lb[0].grad is not None
    assert not any(k.startswith("vaccine") for k in ref) and plain.model.policies.vaccination_policies.doses is None
    nobody = dict(CAMPAIGNS[1], coverage=0.0)
    zero = _fresh_runner(device, vaccination={1: nobody})
    with torch.no_grad():
        res, inf = zero()
    assert calls and set(calls) == {"gj_vaccinate"}
    assert torch.equal(inf, ref_inf) and not res["vaccine_doses_per_timestep"].any()
    for k, v in ref.items():
        if k != "dates":
            assert torch.equal(res[k], v), k


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
        params = lambda: _params("cuda:0", vaccination=CAMPAIGNS, groups=["area"])

        def run(runner):
            policies = runner.model.policies.vaccination_policies.policies
            for policy in policies:
                policy.efficacy = torch.nn.Parameter(policy.efficacy.detach().clone())
            results, _ = runner()
            c = results["cases_per_timestep"]
            loss = (c * torch.linspace(0.5, 1.5, c.numel(), device=c.device)).sum() + results["deaths_per_timestep"].sum()
            loss.backward()
            return results, [policy.efficacy.grad.tolist() for policy in policies]

        torch.manual_seed(33)
        res, grads = run(DistributedRunner.from_parameters(params()))
        gathered = [None] * R_
        dist.all_gather_object(gathered, grads)
        assert gathered[0] == gathered[1], "every rank holds the whole gradient"
        if rank == 0:
            torch.manual_seed(33)
            infection._philox_step = itertools.count(1 << 40)
            ref_res, ref = run(G.Runner.from_parameters(params()))
            for k in ("cases_per_timestep", "deaths_per_timestep", "cases_by_area", "vaccine_doses_per_timestep",
                      "vaccine_doses_by_campaign", "vaccine_doses_by_area"):
                assert torch.equal(res[k].detach().cpu(), ref_res[k].detach().cpu()), k
            assert ref_res["vaccine_doses_by_campaign"][-1].min() > 0
            for a, b in zip(sum(grads, []), sum(ref, [])):
                assert b != 0.0 and a == pytest.approx(b, rel=2e-5, abs=1e-7), (grads, ref)
            out[0] = 1
    finally:
        dist.destroy_process_group()


def test_two_ranks_reproduce_the_single_gpu_series_and_efficacy_gradients(device):
    import os

    import torch.multiprocessing as mp

    out = mp.get_context("spawn").Array("i", [0])
    mp.spawn(_two_rank_worker, args=(2, 29700 + os.getpid() % 90, out), nprocs=2, join=True)
    assert out[0] == 1
