"""GPU: result series by agent group - gj_group_stats / gj_adjoint_group_stats against numpy and torch indexing, the
autograd node GroupSeriesRow against the oracle's autograd, and the Runner's cases_by_<name> / deaths_by_<name> on the
bundled 769-agent world, on one GPU and on two ranks.

The forward sums are 64-bit integers (is_infected in 32.32 fixed point, deaths as a count): for the model's integer
values every comparison is `array_equal`, and no order of the agents may change a bit."""
import itertools

import numpy as np
import pytest
import torch

from grad_june_amd import _native as N
from grad_june_amd.groups import GroupLabelError, GroupStats

pytestmark = pytest.mark.gpu

DEAD = 7
LDS_MAX = 4096           # largest n_groups of the LDS regime (include/gradjune_hip.h)
RESOLUTION = 2.0 ** -32  # of the fixed-point format the cases are summed in
GUARD = 8
SENTINEL = -12345.5


def offset_tensor(array, device, offset):
    """The array on the device, its base pointer `offset` elements behind an allocation's (1: the scalar path)."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=device)
    buf[offset:].copy_(t)
    return buf[offset:]


def run_group_stats(device, group, G, inf, stage, offset=0, check=True):
    """(cases [G], deaths [G]) in fp64, with guard elements around `out` verified untouched."""
    stats = GroupStats(offset_tensor(group.astype(np.int32), device, offset), G)
    assert stats.labels.data_ptr() % 16 == (4 * offset) % 16
    buf = torch.full((2 * G + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=device)
    out = buf[GUARD: GUARD + 2 * G]
    out.zero_()
    stats.add(offset_tensor(inf.astype(np.float32), device, offset), offset_tensor(stage.astype(np.float32), device, offset),
              DEAD, out)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), "wrote outside out"
    assert int(stats.workspace[: 2 * G].abs().max()) == 0, "the workspace's sums are left zero for the next call"
    if check:
        stats.check()
    return host[GUARD: GUARD + G], host[GUARD + G: GUARD + 2 * G], stats


def expected(group, G, inf, stage):
    return (np.bincount(group, weights=inf.astype(np.float64), minlength=G),
            np.bincount(group, weights=(stage == DEAD).astype(np.float64), minlength=G))


def label_patterns(rng, n, G):
    yield "sorted", np.sort(rng.integers(0, G, n))
    yield "shuffled", rng.integers(0, G, n)
    yield "all equal", np.full(n, G - 1)
    yield "some empty", np.minimum(rng.integers(0, max(1, G // 2), n) * 2, G - 1)     # odd groups have nobody


@pytest.mark.parametrize("G", [1, 2, 769, LDS_MAX, LDS_MAX + 1, 1 << 20])
@pytest.mark.parametrize("n", [1, 63, 64, 1_000_003])
def test_kernel_equals_numpy_exactly(device, n, G):
    rng = np.random.default_rng(n * 31 + G)
    inf = rng.integers(0, 3, n).astype(np.float32)              # is_infected is additive: 0, 1 or 2
    stage = rng.integers(1, DEAD + 1, n).astype(np.float32)
    for (what, group), offset in itertools.product(label_patterns(rng, n, G), (0, 1)):
        cases, deaths, _ = run_group_stats(device, group, G, inf, stage, offset)
        want_c, want_d = expected(group, G, inf, stage)
        assert np.array_equal(cases, want_c), (what, offset)
        assert np.array_equal(deaths, want_d), (what, offset)
        assert cases.sum() == inf.sum(dtype=np.float64) and deaths.sum() == (stage == DEAD).sum()


@pytest.mark.parametrize("G", [1, 769, LDS_MAX + 1])
def test_fractional_values_within_the_fixed_point_resolution(device, G):
    """Every value is rounded to the nearest multiple of 2^-32 before it is added (an error of at most half of that) and
    the integer sum is exact, so a group's sum is within (2^-32 / 2) * its size of the true sum.  The assertion uses the
    issue's bound, the resolution times the largest group size; the fp64 reference's own rounding (1e-16 relative) is far
    below it."""
    n = 1_000_003
    rng = np.random.default_rng(G)
    inf = (rng.random(n) * 2.0).astype(np.float32)
    stage = rng.integers(1, DEAD + 1, n).astype(np.float32)
    group = np.sort(rng.integers(0, G, n))
    cases, deaths, _ = run_group_stats(device, group, G, inf, stage)
    want_c, want_d = expected(group, G, inf, stage)
    bound = RESOLUTION * np.bincount(group, minlength=G).max()
    err = np.abs(cases - want_c).max()
    print(f"G={G}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.array_equal(deaths, want_d)


@pytest.mark.parametrize("G", [1, 769, LDS_MAX + 1, 1 << 20])
def test_order_of_the_agents_cannot_change_a_bit(device, G):
    n = 1_000_003
    rng = np.random.default_rng(7 + G)
    inf = (rng.random(n) * 2.0).astype(np.float32)              # fractional: an fp sum WOULD depend on the order
    stage = rng.integers(1, DEAD + 1, n).astype(np.float32)
    group = np.sort(rng.integers(0, G, n))
    first = run_group_stats(device, group, G, inf, stage)[:2]
    again = run_group_stats(device, group, G, inf, stage)[:2]
    perm = rng.permutation(n)
    permuted = run_group_stats(device, group[perm], G, inf[perm], stage[perm])[:2]
    scalar = run_group_stats(device, group[perm], G, inf[perm], stage[perm], offset=1)[:2]
    for other in (again, permuted, scalar):
        assert first[0].tobytes() == other[0].tobytes() and first[1].tobytes() == other[1].tobytes()


def test_the_call_adds_to_out_and_the_workspace_is_reusable(device):
    rng = np.random.default_rng(3)
    n, G = 5000, 11
    group, inf = rng.integers(0, G, n), rng.integers(0, 3, n).astype(np.float32)
    stage = rng.integers(1, DEAD + 1, n).astype(np.float32)
    stats = GroupStats(torch.from_numpy(group.astype(np.int32)).to(device), G)
    out = torch.zeros(2 * G, dtype=torch.float64, device=device)
    for _ in range(3):
        stats.add(torch.from_numpy(inf).to(device), torch.from_numpy(stage).to(device), DEAD, out)
    stats.check()
    want_c, want_d = expected(group, G, inf, stage)
    assert np.array_equal(out.cpu().numpy(), 3 * np.concatenate((want_c, want_d)))


@pytest.mark.parametrize("G", [5, LDS_MAX + 1])
def test_a_label_out_of_range_is_skipped_and_reported(device, G):
    """A bad ARGUMENT to a kernel written never to index with it: the agent is left out, every other sum is exact,
    nothing outside `out` is written and the binding raises."""
    rng = np.random.default_rng(G)
    n = 10_000
    group = rng.integers(0, G, n)
    inf = rng.integers(0, 3, n).astype(np.float32)
    stage = rng.integers(1, DEAD + 1, n).astype(np.float32)
    bad = rng.choice(n, 40, replace=False)
    group[bad] = np.resize(np.array([-1, G, G + 1, 2 ** 31 - 1, -2 ** 31, 1 << 24]), 40)
    for offset in (0, 1):
        cases, deaths, stats = run_group_stats(device, group, G, inf, stage, offset, check=False)   # (checks the guards)
        with pytest.raises(GroupLabelError, match="label outside"):
            stats.check()
        stats.check()                                               # reported once: the word was cleared
        ok = np.ones(n, dtype=bool)
        ok[bad] = False
        want_c, want_d = expected(group[ok], G, inf[ok], stage[ok])
        assert np.array_equal(cases, want_c) and np.array_equal(deaths, want_d)
    # the adjoint: such an agent gets no gradient, and no row is read with its label
    stats = GroupStats(torch.from_numpy(group.astype(np.int32)).to(device), G)
    g = torch.arange(1, G + 1, dtype=torch.float32, device=device)
    grad_inf, grad_stage = stats.gather(torch.full((n,), float(DEAD), device=device), DEAD, g, g)
    assert (grad_inf[torch.from_numpy(bad).to(device)] == 0).all() and (grad_stage[torch.from_numpy(bad).to(device)] == 0).all()
    assert torch.equal(grad_inf[torch.from_numpy(ok).to(device)], g[torch.from_numpy(group[ok]).to(device)])


def test_a_value_that_cannot_be_summed_stays_in_its_group(device):
    rng = np.random.default_rng(5)
    n, G = 4096, 16
    group = rng.integers(0, G, n)
    inf = rng.integers(0, 3, n).astype(np.float32)
    stage = rng.integers(1, DEAD + 1, n).astype(np.float32)
    spoiled = inf.copy()
    spoiled[[10, 20, 30]] = [np.nan, np.inf, -1e30]
    cases, deaths, stats = run_group_stats(device, group, G, spoiled, stage, check=False)
    with pytest.raises(GroupLabelError, match="not finite"):
        stats.check()
    inf[[10, 20, 30]] = 0.0                                          # counted as 0, every other agent as it is
    want_c, want_d = expected(group, G, inf, stage)
    assert np.array_equal(cases, want_c) and np.array_equal(deaths, want_d)


# ---- the adjoint kernel alone --------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 7, 2048, 2049, 1 << 20])
@pytest.mark.parametrize("n", [1, 63, 1_000_003])
def test_adjoint_is_a_gather(device, n, G):
    rng = np.random.default_rng(n + G)
    for offset in (0, 1):
        group = offset_tensor(rng.integers(0, G, n).astype(np.int32), device, offset)
        stage = offset_tensor(rng.integers(DEAD - 1, DEAD + 1, n).astype(np.float32), device, offset)
        stats = GroupStats(group, G)
        gc = torch.from_numpy(rng.normal(size=G).astype(np.float32)).to(device)
        gd = torch.from_numpy(rng.normal(size=G).astype(np.float32)).to(device)
        idx = group.long()
        want_inf = gc[idx]
        # autograd of (stage == dead) * stage / dead, as the header states it: an IEEE division (numpy's; torch divides a
        # device tensor by a host scalar by multiplying with the rounded reciprocal, one ulp away)
        want_stage = torch.from_numpy(gd[idx].cpu().numpy() / np.float32(DEAD) * (stage == DEAD).cpu().numpy()).to(device)
        got_inf, got_stage = stats.gather(stage, DEAD, gc, gd)
        assert torch.equal(got_inf, want_inf) and torch.equal(got_stage, want_stage)
        got_inf, got_stage = stats.gather(stage, DEAD, gc, None)    # g_deaths == NULL
        assert torch.equal(got_inf, want_inf) and torch.equal(got_stage, torch.zeros_like(want_stage))
        got_inf, got_stage = stats.gather(stage, DEAD, None, gd)    # g_cases == NULL
        assert torch.equal(got_inf, torch.zeros_like(want_inf)) and torch.equal(got_stage, want_stage)
        assert stats.gather(stage, DEAD, gc, gd, want_inf=False)[0] is None
        assert stats.gather(stage, DEAD, gc, gd, want_stage=False)[1] is None


def test_node_against_torch_autograd_on_the_dense_form(device):
    from grad_june_amd.autograd import GroupSeriesRow

    rng = np.random.default_rng(11)
    n, G = 3001, 13
    group = torch.from_numpy(rng.integers(0, G, n)).to(device)
    stats = GroupStats(group, G)
    inf = torch.from_numpy(rng.integers(0, 3, n).astype(np.float32)).to(device).requires_grad_()
    stage = torch.from_numpy(rng.integers(DEAD - 1, DEAD + 1, n).astype(np.float32)).to(device).requires_grad_()
    wc = torch.from_numpy(rng.normal(size=G).astype(np.float32)).to(device)
    wd = torch.from_numpy(rng.normal(size=G).astype(np.float32)).to(device)
    cases, deaths = GroupSeriesRow.apply({"stats": stats, "dead": DEAD}, inf, stage)
    dense_c = torch.zeros(G, device=device).index_add(0, group, inf)
    dense_d = torch.zeros(G, device=device).index_add(0, group, (stage == DEAD) * stage / DEAD)
    assert torch.equal(cases, dense_c) and torch.equal(deaths, dense_d)
    got = torch.autograd.grad((cases * wc).sum() + (deaths * wd).sum(), [inf, stage])
    want = torch.autograd.grad((dense_c * wc).sum() + (dense_d * wd).sum(), [inf, stage])
    assert torch.equal(got[0], want[0])
    # (g / dead here, g * fl(1 / dead) in torch's division by a host scalar: one fp32 ulp)
    assert torch.allclose(got[1], want[1], rtol=2.0 ** -22, atol=0.0) and bool((got[1] != 0).any())
    assert torch.equal(got[1] == 0, want[1] == 0)
    only_cases = torch.autograd.grad(GroupSeriesRow.apply({"stats": stats, "dead": DEAD}, inf, stage.detach())[0].sum(), inf)
    assert torch.equal(only_cases[0], torch.ones(n, device=device))


# ---- gradients through the hot path against the oracle's autograd ------------------------------------------------------
N_DRAWS = 12


def _one_draw(device, seed):
    """One draw of tests/test_gpu_random_worlds.py::test_random_world_gradients_against_oracle_autograd (the same seeds
    and the same consumption of its generator, so the same worlds and the same Gumbel ties), with GroupSeriesRow on the
    state after each of the three steps.  Returns None where that test skips, else the number of comparisons made."""
    import gj_oracle as O
    import grad_june_amd as G
    from grad_june_amd.autograd import GroupSeriesRow
    from grad_june_amd.defaults import default_parameters
    from grad_june_amd.synthetic import edge_set_of
    from test_gpu_random_worlds import JUNE_NETWORKS, _hetero, random_state, random_world

    rng = np.random.default_rng(9000 + seed)
    world = random_world(rng)
    A = world["n_agents"]
    names = [n for n in JUNE_NETWORKS if edge_set_of(n) in world["edge_sets"] and rng.random() < 0.8]
    if not names:
        return None
    params = default_parameters(str(device))
    params["networks"] = {n: {"log_beta": float(rng.uniform(-0.3, 1.2))} for n in names}
    params["policies"] = {"interaction": {}}
    thr = None
    if rng.random() < 0.5:
        thr = float(rng.choice([3.0, 4.0]))
        params["policies"]["quarantine"] = {
            "quarantine": {1: {"start_date": "2022-01-01", "end_date": "2022-12-31", "stage_threshold": thr}}}
    model = G.GradJune.from_parameters(params)
    acts = (tuple(names),)
    timer = G.Timer(initial_day="2022-02-01", total_days=10, weekday_step_duration=(24,), weekend_step_duration=(24,),
                    weekday_activities=acts, weekend_activities=acts)
    state = random_state(rng, A, 0.0)
    data = _hetero(G, world, state, device)
    for n in names:
        net = model.infection_networks.networks[n]
        net.log_beta = torch.nn.Parameter(net.log_beta.detach().clone())
    tables = {n: model.infection_networks.networks[n].leisure_probabilities.detach().cpu()
              for n in names if edge_set_of(n) == "leisure"}
    mult = {n: torch.ones((), requires_grad=True) for n in names}
    st = {k: v.clone() for k, v in state.items()}
    # the labels and weights come from a generator of their own: the draw above stays the existing test's
    own = np.random.default_rng(77000 + seed)
    n_groups = (1, 7, A)[seed % 3]
    group = torch.from_numpy(own.integers(0, n_groups, A))
    w = torch.from_numpy(own.normal(size=n_groups).astype(np.float32))
    env = {"stats": GroupStats(group.to(device), n_groups), "dead": DEAD}
    hip_rows, ref_rows, hip_plain = [], [], []
    for i in range(3):
        next(timer)
        noise = O.draw_exp_noise(A, generator=torch.Generator().manual_seed(100 * seed + i))
        betas = {n: float(model.infection_networks[n].beta_value(model.policies, timer)) for n in names}
        model.hot_path(data, timer, exp_noise=noise)
        ag = data["agent"]
        hip_rows.append(GroupSeriesRow.apply(env, ag.is_infected, ag.symptoms["current_stage"])[0])
        hip_plain.append(ag.is_infected.sum())
        out = O.hot_path_step(world, st, now=timer.now, delta_time=timer.duration,
                              day_type=0 if timer.day_type == "weekday" else 1, active=names,
                              betas={n: torch.tensor(np.float32(betas[n])) * mult[n] for n in names},
                              leisure_tables=tables, quarantine_thresholds=None if thr is None else [thr], exp_noise=noise)
        for k in ("susceptibility", "is_infected", "infection_time"):
            st[k] = out[k]
        ref_rows.append(torch.zeros(n_groups).index_add(0, group, out["is_infected"]))
        if not np.array_equal(ag.is_infected.detach().cpu().numpy(), out["is_infected"].detach().numpy()):
            return None                                   # a decision at a Gumbel tie differs: not the same function
        assert torch.equal(hip_rows[-1].detach().cpu(), ref_rows[-1].detach())
    env["stats"].check()
    ps = [model.infection_networks.networks[n].log_beta for n in names]
    compared = 0
    hip, ref = (torch.stack(hip_rows) * w.to(device)).sum(), (torch.stack(ref_rows) * w).sum()
    ones, plain = torch.stack(hip_rows).sum(), torch.stack(hip_plain).sum()
    if not hip.requires_grad:                             # nobody infectious meets anybody susceptible: no graph
        assert not ref.requires_grad or all(g is None or float(g) == 0.0 for g in torch.autograd.grad(
            ref, list(mult.values()), retain_graph=True, allow_unused=True))
        return 0
    grad = lambda y, xs: [0.0 if g is None else float(g) for g in torch.autograd.grad(y, xs, retain_graph=True,
                                                                                      allow_unused=True)]
    got = grad(hip, ps)
    want = [g * np.log(10.0) for g in grad(ref, [mult[n] for n in names])]
    scale = max(1e-6, max(abs(x) for x in want))
    for n, a, b in zip(names, got, want):
        print(f"seed {seed} G={n_groups} {n}: hip {a:.6e} oracle {b:.6e} bound {1e-3 * scale + 1e-6:.2e}")
        assert abs(a - b) <= 1e-3 * scale + 1e-6, (seed, n_groups, n, a, b, scale)
        compared += 1
    # w == 1: the gradients of is_infected.sum() on the same graph
    got1, want1 = grad(ones, ps), grad(plain, ps)
    scale1 = max(1e-6, max(abs(x) for x in want1))
    for n, a, b in zip(names, got1, want1):
        assert abs(a - b) <= 1e-3 * scale1 + 1e-6, (seed, "w == 1", n, a, b, scale1)
    return compared


def test_gradients_by_group_against_oracle_autograd(device):
    """loss = sum_t sum_g w[g] * cases_by_group[t, g] through three chained `hot_path` steps, G in {1, 7, A}; on the
    oracle's side the same loss via index_add.  Bound: 1e-3 of the largest gradient of the draw + 1e-6, the skip rule
    and the seeds of the existing test (so the skipped draws are exactly those it skips)."""
    ran = [_one_draw(device, seed) for seed in range(N_DRAWS)]
    skipped = [s for s, r in enumerate(ran) if r is None]
    print(f"{N_DRAWS} draws, skipped {skipped}, comparisons {[r for r in ran if r is not None]}")
    assert N_DRAWS - len(skipped) >= N_DRAWS / 2, skipped
    assert sum(r for r in ran if r) >= 10


def test_deaths_row_through_the_symptoms_step(device):
    """The world of tests/test_symptoms.py::test_symptoms_differentiable (a hard Gumbel-softmax on a parameter, mortality 1,
    100 steps): deaths by group through GroupSeriesRow against the reference's form
    ((stage == dead) * stage / dead, summed per group with index_add) on the SAME graph.  That test asks for a finite
    gradient; here the two must agree to fp32 rounding of a sum of 100 terms (1e-5 relative)."""
    import grad_june_amd as G
    from grad_june_amd.autograd import GroupSeriesRow
    from grad_june_amd.defaults import default_parameters

    torch.manual_seed(0)
    params = default_parameters(str(device))
    su = G.SymptomsUpdater.from_parameters(params)
    su.symptoms_sampler.stage_transition_probabilities[2:, :] = 1.0
    timer = G.Timer.from_parameters(params)
    n, n_groups = 100, 6
    d = G.HeteroData()
    d["agent"].id = torch.arange(n, device=device)
    d["agent"].age = torch.randint(0, 100, (n,), device=device)
    d["agent"].sex = torch.zeros(n, dtype=torch.long, device=device)
    d["agent"].symptoms = {"current_stage": torch.ones(n, device=device), "next_stage": torch.ones(n, device=device),
                           "time_to_next_stage": torch.zeros(n, device=device)}
    beta = torch.nn.Parameter(torch.tensor(10.0, device=device))
    probs = 1 - torch.exp(-beta) * torch.ones(n, device=device)
    new_infected = torch.nn.functional.gumbel_softmax(probs, tau=0.1, hard=True)
    symptoms = su(data=d, timer=timer, new_infected=new_infected)
    for _ in range(100):
        next(timer)
        symptoms = su(data=d, timer=timer, new_infected=torch.zeros(n, device=device))
    dead = int(su.stages_ids[-1])
    stage = symptoms["current_stage"]
    assert stage.requires_grad and int((stage == dead).sum()) > 0
    group = torch.arange(n, device=device) % n_groups
    w = torch.linspace(0.5, 2.0, n_groups, device=device)
    stats = GroupStats(group, n_groups)
    _, deaths = GroupSeriesRow.apply({"stats": stats, "dead": dead}, torch.zeros(n, device=device), stage)
    dense = torch.zeros(n_groups, device=device).index_add(0, group, (stage == dead) * stage / dead)
    assert torch.equal(deaths, dense)
    got, = torch.autograd.grad((deaths * w).sum(), beta, retain_graph=True)
    want, = torch.autograd.grad((dense * w).sum(), beta, retain_graph=True)
    print(f"d deaths / d beta: node {float(got):.8e} dense {float(want):.8e}")
    assert torch.isfinite(got) and float(want) != 0.0
    assert float(got) == pytest.approx(float(want), rel=1e-5)


# ---- the Runner on the bundled world ---------------------------------------------------------------------------------
def _params(device, **extra):
    from grad_june_amd.defaults import default_parameters

    p = default_parameters(str(device))
    p["timer"]["total_days"] = 12
    p["infection_seed"]["log_fraction_initial_cases"] = -1.3
    for n in p["networks"]:
        p["networks"][n]["log_beta"] += 0.6
    p.update(extra)
    return p


def _run(params, **kw):
    import grad_june_amd as G
    from grad_june_amd import infection

    torch.manual_seed(21)
    infection._philox_step = itertools.count(1 << 40)
    runner = G.Runner.from_parameters(params) if not kw else G.Runner(
        model=G.GradJune.from_parameters(params), data=G.Runner.get_data(params), timer=G.Timer.from_parameters(params),
        log_fraction_initial_cases=params["infection_seed"]["log_fraction_initial_cases"], save_path=params["save_path"],
        parameters=params, **kw)
    with torch.no_grad():
        results, is_infected = runner()
    return runner, results, is_infected


def test_runner_series_by_area_and_ethnicity(device, tmp_path):
    plain_runner, plain, plain_inf = _run(_params(device))
    assert plain_runner.group_keys == {} and not any("_by_area" in k or "_by_ethnicity" in k for k in plain)
    runner, res, inf = _run(_params(device, groups_to_save=["area", "ethnicity"]))
    for key, value in plain.items():                           # nothing that existed changes by a bit
        assert value == res[key] if key == "dates" else torch.equal(value, res[key]), key
    assert torch.equal(plain_inf, inf)
    T = len(res["dates"])
    assert T > 10 and float(res["cases_per_timestep"][-1]) > float(res["cases_per_timestep"][0]) > 0
    for name, G in (("area", 3), ("ethnicity", 17)):
        cases, daily, deaths = res[f"cases_by_{name}"], res[f"daily_cases_by_{name}"], res[f"deaths_by_{name}"]
        assert cases.shape == daily.shape == deaths.shape == (T, G) and cases.dtype == torch.float32
        assert torch.equal(cases.sum(1), res["cases_per_timestep"])
        assert torch.equal(deaths.sum(1), res["deaths_per_timestep"])
        assert torch.equal(daily.sum(1), res["daily_cases_per_timestep"])
        assert torch.equal(daily[0], cases[0]) and torch.equal(daily[1:], cases[1:] - cases[:-1])
    assert list(runner.group_keys["ethnicity"]) == list(runner.ethnicities)
    assert torch.equal(res["cases_by_ethnicity"][-1], runner.get_cases_by_ethnicity(runner.data))
    assert float(res["cases_by_ethnicity"][-1].sum()) > 0
    # the long-format files next to results.csv
    import pandas as pd

    runner.save_path = tmp_path
    runner.save_results(res, inf)
    flat = pd.read_csv(tmp_path / "results.csv")
    assert "cases_per_timestep" in flat.columns and not any("_by_area" in c for c in flat.columns)
    by_area = pd.read_csv(tmp_path / "results_by_area.csv")
    assert list(by_area.columns) == ["date", "area", "cases", "daily_cases", "deaths"] and len(by_area) == 3 * T
    assert by_area["area"][:3].tolist() == list(runner.group_keys["area"])
    assert np.array_equal(by_area["cases"].to_numpy().reshape(T, 3), res["cases_by_area"].cpu().numpy())


def test_runner_age_bins_as_a_label_dict(device):
    import grad_june_amd as G

    params = _params(device)
    age = G.Runner.get_data(params)["agent"].age.cpu().numpy()
    edges = [0, 18, 65, 100]
    label = np.full(age.shape, 3, dtype=np.int64)              # an age ON an edge is in no (open) interval: column 3
    for b in range(3):
        label[(age > edges[b]) & (age < edges[b + 1])] = b
    assert (label == 3).any()
    runner, res, _ = _run(params, groups={"age_band": label})
    assert runner.group_keys["age_band"].tolist() == [0, 1, 2, 3]
    for b, key in enumerate((18, 65, 100)):
        assert torch.equal(res["cases_by_age_band"][:, b], res[f"cases_by_age_{key:02d}"]), key
    assert torch.equal(res["cases_by_age_band"].sum(1), res["cases_per_timestep"])


def test_runner_labels_follow_locality_order(device):
    params = _params(device, groups_to_save=["area", "ethnicity"])
    params["system"]["locality_order"] = "household"
    runner, res, _ = _run(params)
    ag = runner.data["agent"]
    assert "original_index" in ag and not torch.equal(ag.original_index.cpu(), torch.arange(769))
    assert np.array_equal(runner.group_keys["area"][ag.group_labels["area"].cpu().numpy()], np.asarray(ag.area))
    assert torch.equal(res["cases_by_ethnicity"][-1], runner.get_cases_by_ethnicity(runner.data))
    assert torch.equal(res["cases_by_area"].sum(1), res["cases_per_timestep"])
    inf = ag.is_infected.cpu().numpy()
    want = [inf[np.asarray(ag.area) == k].sum() for k in runner.group_keys["area"]]
    assert res["cases_by_area"][-1].cpu().tolist() == want and sum(want) > 0


def test_runner_differentiable_series_by_area(device):
    """Every log_beta a Parameter: the group series stay on the graph, equal the non-differentiable run's values and sum
    to the national series; a loss on cases_by_area and deaths_by_area reaches the parameters."""
    import grad_june_amd as G
    from grad_june_amd import infection

    params = _params(device, groups_to_save=["area"])
    params["timer"]["total_days"] = 6
    _, plain, _ = _run(params)
    torch.manual_seed(21)
    infection._philox_step = itertools.count(1 << 40)
    runner = G.Runner.from_parameters(params)
    nets = runner.model.infection_networks.networks
    for n in nets.values():
        n.log_beta = torch.nn.Parameter(n.log_beta.detach().clone())
    res, _ = runner()
    assert res["cases_by_area"].requires_grad and res["deaths_by_area"].requires_grad
    assert torch.equal(res["cases_by_area"].detach(), plain["cases_by_area"])
    assert torch.equal(res["deaths_by_area"].detach(), plain["deaths_by_area"])
    target = plain["cases_by_area"] * 0.9
    loss = ((res["cases_by_area"] - target) ** 2).mean() + res["deaths_by_area"].sum()
    national = torch.autograd.grad(res["cases_per_timestep"].sum(), [n.log_beta for n in nets.values()],
                                   retain_graph=True, allow_unused=True)
    by_area = torch.autograd.grad(res["cases_by_area"].sum(), [n.log_beta for n in nets.values()],
                                  retain_graph=True, allow_unused=True)
    scale = max(abs(float(g)) for g in national if g is not None)
    assert scale > 0
    for a, b in zip(by_area, national):
        assert (a is None) == (b is None)
        if a is not None:
            assert abs(float(a) - float(b)) <= 1e-3 * scale + 1e-6
    loss.backward()
    grads = [n.log_beta.grad for n in nets.values() if n.log_beta.grad is not None]
    assert len(grads) >= 5 and all(torch.isfinite(g) for g in grads) and any(float(g) != 0.0 for g in grads)


# ---- two ranks ---------------------------------------------------------------------------------------------------------
def _group_worker(rank, R, port, out):
    """DistributedRunner with groups_to_save on two ranks (gloo), plain and differentiable, against the single-GPU Runner."""
    import os

    import torch.distributed as dist

    import grad_june_amd as G
    from grad_june_amd import infection
    from grad_june_amd.defaults import default_parameters
    from grad_june_amd.distributed_api import DistributedRunner

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=R)
    try:
        def params():
            p = default_parameters("cuda:0")
            p["timer"]["total_days"] = 6
            p["infection_seed"]["log_fraction_initial_cases"] = -1.3
            for n in p["networks"]:
                p["networks"][n]["log_beta"] += 0.6
            p["policies"]["quarantine"] = {
                "quarantine": {1: {"start_date": "2022-02-03", "end_date": "2022-02-20", "stage_threshold": 4}}}
            p["groups_to_save"] = ["area", "ethnicity"]
            return p

        def run(runner, differentiable):
            nets = runner.model.infection_networks.networks
            if not differentiable:
                with torch.no_grad():
                    return runner()[0], None
            for n in nets.values():
                n.log_beta = torch.nn.Parameter(n.log_beta.detach().clone())
            results, _ = runner()
            w = torch.linspace(0.5, 1.5, 3, device=results["cases_by_area"].device)
            loss = (results["cases_by_area"] * w).sum() + 3.0 * results["deaths_by_ethnicity"][:, ::2].sum()
            loss.backward()
            return results, {k: (None if n.log_beta.grad is None else float(n.log_beta.grad)) for k, n in nets.items()}

        for differentiable in (False, True):
            torch.manual_seed(33)
            infection._philox_step = itertools.count(1 << 40)        # the seeding stream of a fresh process
            runner = DistributedRunner.from_parameters(params())
            assert len(runner.group_keys["area"]) == 3 and len(runner.group_keys["ethnicity"]) == 17   # of the WHOLE world
            assert runner.data["agent"].group_labels["area"].numel() == runner.n_agents < 769
            res, grads = run(runner, differentiable)
            gathered = [None] * R
            dist.all_gather_object(gathered, grads)
            assert gathered[0] == gathered[1], "every rank holds the whole gradient"
            if rank == 0:
                torch.manual_seed(33)
                infection._philox_step = itertools.count(1 << 40)
                ref_res, ref = run(G.Runner.from_parameters(params()), differentiable)
                for name in ("area", "ethnicity"):
                    for what in ("cases", "daily_cases", "deaths"):
                        key = f"{what}_by_{name}"
                        assert torch.equal(res[key].detach().cpu(), ref_res[key].detach().cpu()), (differentiable, key)
                assert torch.equal(res["cases_by_area"].detach().sum(1).cpu(), ref_res["cases_per_timestep"].detach().cpu())
                if differentiable:
                    nonzero = 0
                    for k, g in ref.items():
                        if g is None:
                            assert grads[k] is None, k
                            continue
                        # (the tolerance of test_two_ranks_gradients_match_single_gpu: one sum order differs)
                        assert grads[k] == pytest.approx(g, rel=2e-5, abs=1e-7), (k, grads[k], g)
                        nonzero += g != 0.0
                    assert nonzero >= 5
                    out[0] = 1
    finally:
        dist.destroy_process_group()


def test_two_ranks_group_series_match_single_gpu(device):
    import os

    import torch.multiprocessing as mp

    R = 2
    out = mp.get_context("spawn").Array("i", [0])
    mp.spawn(_group_worker, args=(R, 29500 + os.getpid() % 90, out), nprocs=R, join=True)
    assert out[0] == 1
