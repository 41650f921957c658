"""GPU: seeding by agent group.  gj_adjoint_seed against its float64 restatement (tests/gj_seed_ref.py) over the shapes
at which the reduction changes form, ``infect_fraction_by_group`` against the scalar seed bit for bit, the reference's
recorded gradients w.r.t. the log fractions (tests/golden/grads_seed.npz) through the whole model, and the Runner /
DistributedRunner with a seed that requires a gradient."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import gj_seed_ref as R
import gj_testlib as L
from grad_june_amd import _native as N

pytestmark = pytest.mark.gpu

SEED, STEP, NOW = 0x1234567, 9, 1.5
G_NAMES = ("g_susc", "g_inf", "g_time", "g_new")
#: which of the four cotangents a variant passes (the others are NULL = zeros)
GIVEN = [G_NAMES, ("g_inf", "g_time"), ("g_inf",), ("g_susc", "g_time", "g_new")]


def _case(n, kind, rng, labels=None, G=None):
    if labels is not None:
        pass
    elif kind == "1null":
        G, labels = 1, None
    elif kind == "2":
        G, labels = 2, rng.integers(0, 2, n)
    elif kind == "7e":                                    # seven groups, group 3 empty
        G, labels = 7, rng.choice([0, 1, 2, 4, 5, 6], n)
    else:                                                 # every agent its own group
        G, labels = n, rng.permutation(n)
    d = {"G": G, "labels": labels, "p_not": (1.0 - rng.uniform(0.03, 0.4, G)).astype(np.float32),
         "susc0": np.where(rng.random(n) < 0.7, 1.0, rng.random(n)).astype(np.float32),
         "time0": rng.random(n).astype(np.float32), "e": rng.exponential(size=(2, n)).astype(np.float32)}
    d["susc0"][::5] = 0.0
    for k in G_NAMES:
        d[k] = rng.standard_normal(n).astype(np.float32)
    return d


def _dev(a, device, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)


def _launch(device, d, labels, given, injected, offset, want_outputs=True, ones_time=False):
    """One gj_adjoint_seed call; returns (grad_fraction, grad_susc_out, grad_time_out) as numpy."""
    from grad_june_amd.groups import SeedPlan

    n, G = len(d["susc0"]), d["G"]
    lab = _dev(labels, device, np.int32)
    plan = None if lab is None else SeedPlan(lab, G, device=device)
    g = {k: _dev(d[k], device) if k in given else None for k in G_NAMES}
    if ones_time:
        g = dict.fromkeys(G_NAMES)
        g["g_time"] = torch.ones(n, device=device)
    n_chunks = plan.n_chunks if plan is not None else (n + N.GJ_SEED_CHUNK - 1) // N.GJ_SEED_CHUNK
    contrib = torch.empty(max(1, n), dtype=torch.float64, device=device)
    partial = torch.full((max(1, n_chunks),), float("nan"), dtype=torch.float64, device=device)
    out = torch.full((G,), float("nan"), dtype=torch.float64, device=device)
    gs, gt = ((torch.empty(n, device=device), torch.empty(n, device=device)) if want_outputs else (None, None))
    keep = [_dev(d["p_not"], device), _dev(d["susc0"], device), _dev(d["time0"], device),
            _dev(d["e"], device) if injected else None]
    N.check(N.load().gj_adjoint_seed(n, N.ptr(keep[0]), N.ptr(lab), G, C.byref(plan.c) if plan is not None else None,
                                     N.ptr(keep[1]), N.ptr(keep[2]), N.ptr(keep[3]), SEED, STEP, offset, NOW,
                                     N.ptr(g["g_susc"]), N.ptr(g["g_inf"]), N.ptr(g["g_time"]), N.ptr(g["g_new"]),
                                     N.ptr(contrib), N.ptr(partial), N.ptr(out), N.ptr(gs), N.ptr(gt),
                                     N.current_stream()), "gj_adjoint_seed")
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if gs is None else gs.cpu().numpy(), None if gt is None else gt.cpu().numpy()


def _forward_decisions(device, d, labels, injected, offset):
    n = len(d["susc0"])
    p = d["p_not"][np.zeros(n, dtype=np.int64) if labels is None else labels]
    probs, noise = _dev(p, device), (_dev(d["e"], device) if injected else None)
    new = torch.empty(n, device=device)
    N.check(N.load().gj_sample_infect(n, N.ptr(probs), N.ptr(noise), SEED, STEP, offset, NOW, N.ptr(new), None, None, None,
                                      N.current_stream()), "gj_sample_infect")
    return new.cpu().numpy() > 0.5


@pytest.mark.parametrize("injected", [True, False], ids=["injected", "philox"])
@pytest.mark.parametrize("kind", ["1null", "2", "7e", "n"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1003])
def test_kernel_against_the_restatement(device, n, kind, injected):
    """Per group: |kernel - float64 restatement| <= 1e-6 * sum |c_a| over the group; two launches give the same bits;
    the decisions the adjoint took are gj_sample_infect's.  Shuffled and sorted labels, agent_offset 0 and 5 (the Philox
    blocks serve 4 and 2 agents: an odd offset moves their boundaries), some cotangents NULL."""
    rng = np.random.default_rng(1000 * n + len(kind))
    d = _case(n, kind, rng)
    variants = itertools.product((False, True), (0, 5))
    for v, (sort, offset) in enumerate(variants):
        labels = d["labels"]
        if labels is not None and sort:
            labels = np.sort(labels)
        given = GIVEN[v]
        if injected:
            e0, e1, theta = d["e"][0], d["e"][1], None
        else:
            e0, e1, theta = R.library_draws(SEED, STEP, offset, n)
        ref = R.seed_adjoint(d["p_not"], labels, d["G"], d["susc0"], d["time0"], NOW, e0, e1, theta,
                             **{k: d[k] for k in given})
        got, gs, gt = _launch(device, d, labels, given, injected, offset)
        again, _, _ = _launch(device, d, labels, given, injected, offset, want_outputs=False)
        assert np.array_equal(got.view(np.int64), again.view(np.int64)), "two launches differ"
        err, bound = np.abs(got - ref["grad_fraction"]), 1e-6 * ref["abs_sum"]
        assert np.all(err <= bound), (sort, offset, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.any(ref["abs_sum"] > 0)
        # the decisions: grad_time_out = g_time * (1 - nu) with g_time = 1
        _, _, one_minus_nu = _launch(device, d, labels, (), injected, offset, ones_time=True)
        fwd = _forward_decisions(device, d, labels, injected, offset)
        assert np.array_equal(one_minus_nu == 0.0, fwd) and np.all((one_minus_nu == 0.0) | (one_minus_nu == 1.0))
        assert np.array_equal(fwd, ref["nu"] > 0.5)
        assert np.array_equal(gs, ref["grad_susc"].astype(np.float32))
        assert np.array_equal(gt, ref["grad_time"].astype(np.float32))


def _chunked_labels(which, rng):
    """(n, G, labels) with groups of more than one chunk of GJ_SEED_CHUNK = 1024 agents, sizes no multiple of it."""
    if which == "null-2500":                      # no labels: 3 chunks, the last of 452
        return 2500, 1, None
    if which == "one-70001":                      # one labelled group of 69 chunks: more than a wave of partials
        return 70001, 1, np.zeros(70001, dtype=np.int64)
    sizes = [3000, 1, 0, 1025, 1024, 950, 2049]   # 3, 1, 0, 2, 1, 1, 3 chunks
    return sum(sizes), len(sizes), rng.permutation(np.repeat(np.arange(len(sizes)), sizes))


@pytest.mark.parametrize("injected", [True, False], ids=["injected", "philox"])
@pytest.mark.parametrize("which", ["null-2500", "one-70001", "mixed"])
def test_groups_of_several_chunks_against_the_restatement(device, which, injected):
    """The same checks where a group spans several (group, chunk) partials: chunk offsets k > 0, the clamp of a group's
    last chunk, the finish kernel adding several partials per group (more than 64 of them for one-70001), next to groups
    of one agent, of exactly one chunk and of none."""
    from grad_june_amd.groups import SeedPlan

    rng = np.random.default_rng(len(which))
    n, G, labels0 = _chunked_labels(which, rng)
    d = _case(n, None, rng, labels=labels0 if labels0 is not None else np.zeros(n, dtype=np.int64), G=G)
    if labels0 is not None:
        plan = SeedPlan(torch.from_numpy(labels0.astype(np.int32)), G, device=device)
        sizes = np.bincount(labels0, minlength=G)
        assert plan.n_chunks == int(np.ceil(sizes / N.GJ_SEED_CHUNK).sum()) and plan.n_chunks > G - 1
    for v, (sort, offset) in enumerate(itertools.product((False, True), (0, 5))):
        labels = labels0
        if labels is not None and sort:
            labels = np.sort(labels)
        given = GIVEN[v]
        e0, e1, theta = (d["e"][0], d["e"][1], None) if injected else R.library_draws(SEED, STEP, offset, n)
        ref = R.seed_adjoint(d["p_not"], labels, G, d["susc0"], d["time0"], NOW, e0, e1, theta, **{k: d[k] for k in given})
        got, gs, gt = _launch(device, d, labels, given, injected, offset)
        again, _, _ = _launch(device, d, labels, given, injected, offset, want_outputs=False)
        assert np.array_equal(got.view(np.int64), again.view(np.int64)), "two launches differ"
        err, bound = np.abs(got - ref["grad_fraction"]), 1e-6 * ref["abs_sum"]
        assert np.all(err <= bound), (sort, offset, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all((ref["abs_sum"] > 0) == (np.bincount(np.zeros(n, int) if labels is None else labels, minlength=G) > 0))
        assert np.array_equal(gs, ref["grad_susc"].astype(np.float32))
        assert np.array_equal(gt, ref["grad_time"].astype(np.float32))


@pytest.mark.parametrize("injected", [True, False], ids=["injected", "philox"])
def test_label_out_of_range_contributes_nothing(device, injected):
    rng = np.random.default_rng(4)
    n = 257
    d = _case(n, "7e", rng)
    labels = d["labels"].copy()
    labels[[0, 100, 256]] = [-1, 7, 2 ** 31 - 1]
    e0, e1, theta = (d["e"][0], d["e"][1], None) if injected else R.library_draws(SEED, STEP, 0, n)
    ref = R.seed_adjoint(d["p_not"], labels, 7, d["susc0"], d["time0"], NOW, e0, e1, theta, **{k: d[k] for k in G_NAMES})
    got, gs, gt = _launch(device, d, labels, G_NAMES, injected, 0)
    assert np.all(np.abs(got - ref["grad_fraction"]) <= 1e-6 * ref["abs_sum"])
    assert np.array_equal(gs, ref["grad_susc"].astype(np.float32)) and np.array_equal(gt, ref["grad_time"].astype(np.float32))
    assert np.array_equal(gt[[0, 100, 256]], d["g_time"][[0, 100, 256]])                  # not seeded: nu = 0


# ---- infect_fraction_by_group against the scalar seed ------------------------------------------------------------------
class _T:
    now = 2.0


def _seed_data(G, n, device):
    d = G.HeteroData()
    ag = d["agent"]
    ag.id = torch.arange(n)
    rng = np.random.default_rng(8)
    ag.susceptibility = torch.from_numpy(np.where(rng.random(n) < 0.8, 1.0, 0.0).astype(np.float32)).to(device)
    ag.is_infected = (1.0 - ag.susceptibility).clone()
    ag.infection_time = torch.from_numpy(rng.random(n).astype(np.float32)).to(device)
    return d


@pytest.mark.parametrize("grad", [False, True], ids=["plain", "node"])
@pytest.mark.parametrize("injected", [True, False], ids=["injected", "philox"])
def test_equal_fractions_are_the_scalar_seed_bit_for_bit(device, injected, grad):
    import grad_june_amd as G
    from grad_june_amd import infection

    n, fraction = 1003, 10.0 ** torch.tensor(-0.7)
    noise = torch.empty(2, n).exponential_(generator=torch.Generator().manual_seed(3)) if injected else None
    labels = torch.from_numpy(np.random.default_rng(2).integers(0, 3, n).astype(np.int32))
    torch.manual_seed(11)
    results = []
    for by_group in (False, True):
        data = _seed_data(G, n, device)
        infection._philox_step = itertools.count(77)                       # the same Philox key for both
        if by_group:
            fr = fraction.repeat(3).requires_grad_(grad)
            with torch.set_grad_enabled(grad):
                new = infection.infect_fraction_by_group(data, _T(), None, fr, labels, device, exp_noise=noise)
            assert new.requires_grad == grad and data["agent"].is_infected.requires_grad == grad
        else:
            with torch.no_grad():
                new = infection.infect_fraction_of_people(data, _T(), None, fraction, device, exp_noise=noise)
        ag = data["agent"]
        results.append([t.detach().cpu() for t in (new, ag.susceptibility, ag.is_infected, ag.infection_time)])
    assert results[0][0].sum() > 50
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_bad_labels_and_shapes_are_refused(device):
    import grad_june_amd as G
    from grad_june_amd import infection

    data = _seed_data(G, 10, device)
    with pytest.raises(ValueError):
        infection.infect_fraction_by_group(data, _T(), None, torch.tensor([0.1, 0.2]), None, device)
    with pytest.raises(ValueError):
        infection.infect_fraction_by_group(data, _T(), None, torch.tensor([0.1, 0.2]), torch.full((10,), 2), device)
    with pytest.raises(ValueError):
        infection.infect_fraction_by_group(data, _T(), None, torch.tensor(0.1), None, device)


# ---- the reference's recorded gradients through the whole model ---------------------------------------------------------
SYM = ("current_stage", "next_stage", "time_to_next_stage")


@pytest.mark.parametrize("case", ["s1", "s2"])
def test_golden_gradients_wrt_the_log_fractions(device, case):
    """grads_seed.npz: the seed (national / three area groups) and 4 steps with the reference's draws injected.  The
    states are the recorded ones exactly; d loss / d log_fraction and d loss / d log_beta match the reference's autograd
    under the criterion of test_gradients.py::test_hip_backward_matches_reference."""
    import grad_june_amd as G
    from grad_june_amd import infection
    from grad_june_amd.defaults import default_parameters
    from test_gradients import _hetero, step_info

    pre = case + "/"
    sub = {k[len(pre):]: v for k, v in L.load_npz("grads_seed.npz").items() if k.startswith(pre)}
    world = L.world_from(sub)
    names = str(sub["networks"]).split(",")
    params = default_parameters(str(device))
    for n in params["networks"]:
        params["networks"][n]["log_beta"] += 0.7
    model, timer = G.GradJune.from_parameters(params), G.Timer.from_parameters(params)
    start = {"state0/" + k[len("seed/pre/"):]: v for k, v in sub.items() if k.startswith("seed/pre/") and "/sym/" not in k}
    data = _hetero(G, start, world, device)
    ag = data["agent"]
    ag.symptoms = {k: torch.from_numpy(sub["seed/pre/sym/" + k]).to(device) for k in SYM}
    for n in names:
        net = model.infection_networks.networks[n]
        net.log_beta = torch.nn.Parameter(net.log_beta.detach().clone())
    log_fraction = torch.nn.Parameter(torch.from_numpy(sub["seed/log_fraction"]).clone())
    labels = None if case == "s1" else torch.from_numpy(sub["seed/labels"])
    assert timer.now == float(sub["seed/now"])
    new = infection.infect_fraction_by_group(data, timer, model.symptoms_updater, 10.0 ** log_fraction, labels, device,
                                             exp_noise=torch.from_numpy(sub["seed/exp_noise"]))
    assert new.requires_grad and np.array_equal(new.detach().cpu().numpy(), sub["seed/new_infected"])
    for k in ("susceptibility", "is_infected", "infection_time"):
        assert np.array_equal(ag[k].detach().cpu().numpy(), sub["state0/" + k]), k
    sym = model.symptoms_updater(data, timer, new, progresses=torch.from_numpy(sub["seed/sym/progresses"]),
                                 dwell=torch.from_numpy(sub["seed/sym/dwell"]))
    for k in SYM:
        assert np.array_equal(sym[k].detach().cpu().numpy(), sub["state0/sym/" + k]), k
    series = []
    for i in range(int(sub["n_steps"])):
        s = step_info(sub, i)
        next(timer)
        assert timer.now == s["now"]
        new, _ = model.hot_path(data, timer, exp_noise=s["noise"])
        assert np.array_equal(ag.is_infected.detach().cpu().numpy(), s["is_infected"]), i
        sym = model.symptoms_updater(data, timer, new, progresses=torch.from_numpy(sub[f"step{i}/sym/progresses"]),
                                     dwell=torch.from_numpy(sub[f"step{i}/sym/dwell"]))
        for k in SYM:
            assert np.array_equal(sym[k].detach().cpu().numpy(), sub[f"step{i}/sym/post/{k}"]), (i, k)
        series.append(ag.is_infected.sum())
    plist = [log_fraction] + [model.infection_networks.networks[n].log_beta for n in names]
    for tag, loss in (("last", series[-1]), ("series", torch.stack(series).sum())):
        grads = torch.autograd.grad(loss, plist, retain_graph=True, allow_unused=True)
        got_f, ref_f = grads[0].detach().cpu().numpy(), sub[f"grad_{tag}/log_fraction"]
        print(case, tag, "log_fraction", got_f.tolist(), ref_f.tolist())
        for g in range(len(ref_f)):
            assert float(got_f[g]) == pytest.approx(float(ref_f[g]), rel=2e-5, abs=1e-7), (tag, g, got_f, ref_f)
        for n, g in zip(names, grads[1:]):
            got, ref = (0.0 if g is None else float(g)), float(sub[f"grad_{tag}/{n}"])
            assert got == pytest.approx(ref, rel=2e-5, abs=1e-7), (tag, n, got, ref)


# ---- the Runner ----------------------------------------------------------------------------------------------------------
def _runner_params(device, by=None, days=5, series=True, locality=None, save_path=None):
    from grad_june_amd.defaults import default_parameters

    p = default_parameters(str(device))
    p["timer"]["total_days"] = days
    p["infection_seed"]["log_fraction_initial_cases"] = -1.2
    for n in p["networks"]:
        p["networks"][n]["log_beta"] += 0.6
    if by:
        p["infection_seed"]["by"] = by
        if series:
            p["groups_to_save"] = [by]
    if locality:
        p["system"]["locality_order"] = locality
    if save_path is not None:
        p["save_path"] = str(save_path)
    return p


def _fresh_runner(device, seed=21, **kw):
    import grad_june_amd as G
    from grad_june_amd import infection

    torch.manual_seed(seed)
    infection._philox_step = itertools.count(1 << 40)
    return G.Runner.from_parameters(_runner_params(device, **kw))


def test_runner_gradient_wrt_the_fraction_of_every_area(device):
    grads = []
    for _ in range(2):
        runner = _fresh_runner(device, by="area")
        G_ = len(runner.group_keys["area"])
        assert runner.seed_group == "area" and G_ >= 3 and tuple(runner.log_fraction_initial_cases.shape) == (G_,)
        runner.log_fraction_initial_cases = torch.nn.Parameter(torch.linspace(-1.4, -0.8, G_))
        results, _ = runner()
        by_area = results["cases_by_area"]
        assert by_area.requires_grad and by_area.shape[1] == G_
        torch.nn.functional.mse_loss(by_area, torch.zeros_like(by_area)).backward()
        g = runner.log_fraction_initial_cases.grad
        assert g.shape == (G_,) and torch.isfinite(g).all() and (g != 0).all(), g
        grads.append(g.clone())
    assert torch.equal(grads[0], grads[1]), "a second identical run gives other bits"


def test_runner_with_a_scalar_parameter_runs_and_yields_a_gradient(device):
    runner = _fresh_runner(device)
    assert runner.seed_group is None
    runner.log_fraction_initial_cases = torch.nn.Parameter(torch.tensor(-1.2))
    results, _ = runner()
    results["cases_per_timestep"].sum().backward()
    g = runner.log_fraction_initial_cases.grad
    assert g.shape == () and torch.isfinite(g) and g != 0


def test_runner_without_a_gradient_takes_the_scalar_path_and_by_group_equals_it(device):
    """Plain config: no labelling, the scalar launch.  ``by: area`` with no group listed seeds every area with the same
    fraction: the same decisions and the same series, bit for bit, with and without grad mode."""
    plain = _fresh_runner(device)
    assert plain.seed_group is None and plain.group_keys == {} and not isinstance(plain.log_fraction_initial_cases, torch.Tensor)
    with torch.no_grad():
        ref, ref_inf = plain()
    grouped = _fresh_runner(device, by="area")
    with torch.no_grad():
        res, inf = grouped()
    again = _fresh_runner(device, by="area")
    res2, inf2 = again()                                         # grad mode on, nothing requires a gradient
    assert ref["cases_per_timestep"][0] > 20
    for r, i in ((res, inf), (res2, inf2)):
        assert torch.equal(i, ref_inf)
        for k in ("cases_per_timestep", "deaths_per_timestep", "cases_by_age_65"):
            assert torch.equal(r[k], ref[k]), k
        assert torch.equal(r["cases_by_area"].sum(1), ref["cases_per_timestep"])


@pytest.mark.parametrize("locality", [None, "household"], ids=["file-order", "locality-order"])
def test_seeding_by_a_labelling_that_has_no_result_series(device, tmp_path, locality):
    """``infection_seed.by: area`` without ``groups_to_save``: the labelling is seeded by and nothing else - no
    ``cases_by_area`` series, ``save_results`` writes the national file only - with and without a gradient, and with the
    agents renumbered by ``system.locality_order`` (the labels are encoded before and carried along)."""
    kw = dict(by="area", series=False, locality=locality, save_path=tmp_path / "out")
    runner = _fresh_runner(device, **kw)
    G_ = len(runner.group_keys["area"])
    assert runner.seed_group == "area" and runner._groups() == {}
    with torch.no_grad():
        results, is_infected = runner()
    assert not any(k.endswith("_by_area") for k in results) and results["cases_per_timestep"][0] > 20
    assert is_infected.sum() == results["cases_per_timestep"][-1]
    runner.save_results(results, is_infected)
    assert sorted(f.name for f in (tmp_path / "out").iterdir()) == ["results.csv", "results_is_infected.csv"]
    # the file-order run of the same labelling with series seeds the same agents: the labels travel with the agents
    if locality is None:
        with_series = _fresh_runner(device, by="area")
        with torch.no_grad():
            ref, ref_inf = with_series()
        assert torch.equal(ref["cases_per_timestep"], results["cases_per_timestep"]) and torch.equal(ref_inf, is_infected)
    runner = _fresh_runner(device, **kw)
    runner.log_fraction_initial_cases = torch.nn.Parameter(torch.linspace(-1.4, -0.8, G_))
    results, is_infected = runner()
    assert not any(k.endswith("_by_area") for k in results)
    results["cases_per_timestep"].sum().backward()
    g = runner.log_fraction_initial_cases.grad
    assert g.shape == (G_,) and torch.isfinite(g).all() and (g != 0).all(), g
    runner.save_results(results, is_infected)


def test_plain_config_seeds_through_the_scalar_call_with_the_old_arguments(device, monkeypatch):
    """The reference's scalar-only config: ``set_initial_cases`` makes the one call it has always made -
    ``infect_fraction_of_people(fraction=10.0 ** log_fraction, agent_offset=0)`` with the fraction a Python float - and
    never enters the by-group function."""
    from grad_june_amd import infection
    from grad_june_amd import runner as RN

    runner = _fresh_runner(device)
    calls = []
    real = RN.infect_fraction_of_people

    def spy(**kw):
        calls.append(kw)
        return real(**kw)

    def refuse(*a, **kw):
        raise AssertionError("the plain config entered infect_fraction_by_group")

    monkeypatch.setattr(RN, "infect_fraction_of_people", spy)
    monkeypatch.setattr(infection, "infect_fraction_by_group", refuse)
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            runner()
    assert len(calls) == 2
    for kw in calls:
        assert sorted(kw) == ["agent_offset", "data", "device", "fraction", "symptoms_updater", "timer"]
        assert type(kw["fraction"]) is float and kw["fraction"] == 10.0 ** -1.2 and kw["agent_offset"] == 0
        assert kw["data"] is runner.data and kw["timer"] is runner.timer and kw["device"] == runner.device
        assert kw["symptoms_updater"] is runner.model.symptoms_updater


# ---- two ranks ----------------------------------------------------------------------------------------------------------
def _seed_grad_worker(rank, R_, port, out):
    import os

    import torch.distributed as dist

    import grad_june_amd as G
    from grad_june_amd import infection
    from grad_june_amd.distributed_api import DistributedRunner

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=R_)
    try:
        def run(runner):
            G_ = len(runner.group_keys["area"])
            runner.log_fraction_initial_cases = torch.nn.Parameter(torch.linspace(-1.4, -0.8, G_))
            results, _ = runner()
            c = results["cases_per_timestep"]
            loss = (c * torch.linspace(0.5, 1.5, c.numel(), device=c.device)).sum() + (results["cases_by_area"] ** 2).mean()
            loss.backward()
            return results, runner.log_fraction_initial_cases.grad.tolist()

        torch.manual_seed(33)
        res, grads = run(DistributedRunner.from_parameters(_runner_params("cuda:0", by="area", days=4)))
        gathered = [None] * R_
        dist.all_gather_object(gathered, grads)
        assert gathered[0] == gathered[1], "every rank holds the whole gradient"
        if rank == 0:
            torch.manual_seed(33)
            infection._philox_step = itertools.count(1 << 40)
            ref_res, ref = run(G.Runner.from_parameters(_runner_params("cuda:0", by="area", days=4)))
            assert torch.equal(res["cases_per_timestep"].detach().cpu(), ref_res["cases_per_timestep"].detach().cpu())
            assert all(g != 0.0 for g in ref)
            for a, b in zip(grads, ref):
                assert a == pytest.approx(b, rel=2e-5, abs=1e-7), (grads, ref)
            out[0] = 1
    finally:
        dist.destroy_process_group()


def test_two_ranks_reproduce_the_single_gpu_fraction_gradients(device):
    import os

    import torch.multiprocessing as mp

    out = mp.get_context("spawn").Array("i", [0])
    mp.spawn(_seed_grad_worker, args=(2, 29500 + os.getpid() % 90, out), nprocs=2, join=True)
    assert out[0] == 1
