"""GPU: the symptom-stage series - gj_stage_stats / gj_adjoint_stage_stats against numpy and torch autograd, on the
reference's own 90-day record, and the Runner's <stage>_per_timestep / new_<stage>_per_timestep / *_by_<name> on the
bundled 769-agent world: plain, differentiable, and on two ranks.

The counts are 64-bit integers: every comparison of a series is `array_equal`, and no order of the agents, no alignment
and no regime may change a bit."""
import itertools

import numpy as np
import pytest
import torch

import gj_testlib as L
from grad_june_amd import _native as N
from grad_june_amd.groups import StageLabelError, StageStats

pytestmark = pytest.mark.gpu

STAGES = ["recovered", "susceptible", "exposed", "infectious", "symptomatic", "severe", "critical", "dead"]
GUARD = 8
SENTINEL = -(1 << 40) - 12345


def lds_boundary(S):
    """Largest n_groups (> 1) of the LDS regime for S stages (include/gradjune_hip.h, regime (ii))."""
    return N.GJ_STAGE_LDS_BINS // S


def n_two_loads(G, S):
    """The smallest n at which, with the grid gj_stage_stats really launches, a lane makes a second load in the
    four-agents-per-lane path (and so in the scalar path, which has four times the units): the grid is at its cap of
    blocks * threads lanes, and one unit more than one per lane makes the first workgroup's share one longer than its
    lanes.  (n_groups == 1 keeps GJ_STAGE_LDS_BLOCKS workgroups up to GJ_STAGE_LANE_LOADS loads per lane.)"""
    if G is None or G == 1 or G * S <= N.GJ_STAGE_LDS_BINS:
        lanes = N.GJ_STAGE_LDS_BLOCKS * N.GJ_STAGE_LDS_THREADS
    else:
        lanes = N.GJ_STAGE_GLOBAL_BLOCKS * N.GJ_STAGE_GLOBAL_THREADS
    return 4 * (lanes + 1)


def offset_tensor(array, device, offset):
    """The array on the device, its base pointer `offset` elements behind an allocation's (1: the scalar path)."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=device)
    buf[offset:].copy_(t)
    return buf[offset:]


def run_stage_stats(device, group, G, S, stage, prev, offset=0, base=None, check=True, calls=1):
    """out [2, G, S] (int64, on the device) after `calls` launches on top of `base` (zeros), the guard elements around
    it verified untouched; and the StageStats."""
    labels = None if group is None else offset_tensor(group.astype(np.int32), device, offset)
    stats = StageStats(labels, G, S, device=device)
    cur = offset_tensor(stage.astype(np.float32), device, offset)
    assert cur.data_ptr() % 16 == (4 * offset) % 16
    prv = None if prev is None else offset_tensor(prev.astype(np.float32), device, offset)
    buf = torch.full((2 * G * S + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=device)
    out = buf[GUARD: GUARD + 2 * G * S]
    if base is None:
        out.zero_()
    else:
        out.copy_(torch.from_numpy(base.reshape(-1)))
    for _ in range(calls):
        stats.add(cur, prv, out)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), "wrote outside out"
    if check:
        stats.check()
    return out.reshape(2, G, S), stats


def same_counts(out, want):
    """np.array_equal of the device's counts and numpy's.  Above 2^22 counters (n_groups = 2^20) the two are compared
    through their non-zero entries - positions and values, which is the same statement - so that a case does not move
    hundreds of MiB to the host per launch."""
    if out.numel() <= 1 << 22:
        return np.array_equal(out.cpu().numpy(), want)
    flat, want = out.reshape(-1), want.reshape(-1)
    at = torch.nonzero(flat).reshape(-1)
    want_at = np.nonzero(want)[0]
    return np.array_equal(at.cpu().numpy(), want_at) and np.array_equal(flat[at].cpu().numpy(), want[want_at])


def expected(group, G, S, stage, prev):
    """np.bincount on group * S + stage over the agents with a label in [0, G) and an integer stage in [0, S)."""
    g = np.zeros(stage.shape, np.int64) if group is None else group.astype(np.int64)
    with np.errstate(invalid="ignore"):
        ok = (g >= 0) & (g < G) & (stage >= 0) & (stage < S) & (stage == np.trunc(stage))
    bins = g[ok] * S + stage[ok].astype(np.int64)
    occ = np.bincount(bins, minlength=G * S)
    ent = np.zeros(G * S, np.int64) if prev is None else np.bincount(bins[prev[ok] != stage[ok]], minlength=G * S)
    return np.stack((occ, ent)).reshape(2, G, S).astype(np.int64)


def label_patterns(rng, n, G):
    yield "sorted", np.sort(rng.integers(0, G, n))
    yield "shuffled", rng.integers(0, G, n)
    yield "all equal", np.full(n, G - 1)
    yield "some empty", np.minimum(rng.integers(0, max(1, G // 2), n) * 2, G - 1)     # odd groups have nobody


def stage_draws(rng, n, S):
    yield "contended", np.where(rng.random(n) < 0.9, 1, rng.integers(0, S, n)).astype(np.float32)   # 90 % in stage 1
    yield "uniform", rng.integers(0, S, n).astype(np.float32)


def previous(rng, stage, S):
    """A previous stage that differs for a random third of the agents."""
    return np.where(rng.random(stage.shape) < 1.0 / 3.0, (stage + 1 + rng.integers(0, S - 1, stage.shape)) % S,
                    stage).astype(np.float32)


G_CASES = ["null", 1, 3, 1250, "lds", "lds+1", 1 << 20]


def _groups_of(case, S):
    return {"null": None, "lds": lds_boundary(S), "lds+1": lds_boundary(S) + 1}.get(case, case)


def _sweep():
    for S, case in itertools.product((3, 8, 16), G_CASES):
        for n in (1, 63, 64, 65, 4099):
            yield pytest.param(n, case, S, id=f"n{n}-G{case}-S{S}")
        if case in ("null", 1250, "lds+1"):
            yield pytest.param("two loads", case, S, id=f"two-loads-G{case}-S{S}")


# ---- 1. exactness --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,case,S", list(_sweep()))
def test_kernel_equals_numpy_exactly(device, n, case, S):
    G = _groups_of(case, S)
    if n == "two loads":
        n = n_two_loads(G, S)
        assert 2_000_000 < n < 4_000_000
    rng = np.random.default_rng(n * 31 + S * 7 + (0 if G is None else G))
    patterns = [("no labels", None)] if G is None else list(label_patterns(rng, n, G))
    for (dist, stage), (what, group), offset in itertools.product(list(stage_draws(rng, n, S)), patterns, (0, 1)):
        prev = previous(rng, stage, S)
        got, _ = run_stage_stats(device, group, G or 1, S, stage, prev, offset)
        want = expected(group, G or 1, S, stage, prev)
        assert same_counts(got, want), (dist, what, offset)
        assert int(got[0].sum()) == n and int(got[1].sum()) == (prev != stage).sum()
    # without a previous stage the second plane is left alone
    got, _ = run_stage_stats(device, patterns[0][1], G or 1, S, stage, None)
    assert same_counts(got, expected(patterns[0][1], G or 1, S, stage, None)) and not bool(got[1].any())


def test_national_call_where_the_lane_bound_sizes_the_grid(device):
    """Regime (i) counts in 8-bit fields per lane; what keeps a field from overflowing is the grid: above
    GJ_STAGE_LDS_BLOCKS * GJ_STAGE_LDS_THREADS * GJ_STAGE_LANE_LOADS units the host launches more workgroups, so that no
    lane takes more than GJ_STAGE_LANE_LOADS loads.  One misaligned (scalar-path) call just above that size, where the
    lanes take 63 loads each, with nearly everybody in one stage."""
    S = 8
    cap = N.GJ_STAGE_LDS_BLOCKS * N.GJ_STAGE_LDS_THREADS * N.GJ_STAGE_LANE_LOADS
    n = cap + N.GJ_STAGE_LDS_THREADS * N.GJ_STAGE_LANE_LOADS + 1          # 514 workgroups
    rng = np.random.default_rng(8)
    stage = np.where(rng.random(n) < 0.97, 1, rng.integers(0, S, n)).astype(np.float32)
    prev = np.where(rng.random(n) < 0.5, 0, stage).astype(np.float32)
    got, _ = run_stage_stats(device, None, 1, S, stage, prev, offset=1)
    assert same_counts(got, expected(None, 1, S, stage, prev))
    assert int(got[0].sum()) == n


# ---- 2. the call adds; no order changes a bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["null", 1, 37, "lds", "lds+1"])
def test_the_call_adds_and_the_order_of_the_agents_cannot_change_a_bit(device, case):
    n, S = 20011, 8
    G = _groups_of(case, S)
    rng = np.random.default_rng(11 + (0 if G is None else G))
    stage = next(stage_draws(rng, n, S))[1]
    prev = previous(rng, stage, S)
    group = None if G is None else np.sort(rng.integers(0, G, n))
    counts = expected(group, G or 1, S, stage, prev)
    base = rng.integers(-5, 1 << 40, counts.shape)
    once, _ = run_stage_stats(device, group, G or 1, S, stage, prev, base=base)
    twice, _ = run_stage_stats(device, group, G or 1, S, stage, prev, base=base, calls=2)
    once, twice = once.cpu().numpy(), twice.cpu().numpy()
    assert np.array_equal(once, base + counts) and np.array_equal(twice, base + 2 * counts)
    perm = rng.permutation(n)
    for offset in (0, 1):
        permuted, _ = run_stage_stats(device, None if group is None else group[perm], G or 1, S, stage[perm], prev[perm],
                                      offset, base=base)
        assert permuted.cpu().numpy().tobytes() == once.tobytes(), offset


# ---- 3. bad input ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["label -1", "label G", "nan", "2.5", "-1", "S"])
@pytest.mark.parametrize("case", [1, "lds", "lds+1"])
def test_bad_input_is_skipped_and_reported(device, case, bad):
    n, S = 5000, 8
    G = _groups_of(case, S)
    rng = np.random.default_rng(5 + G)
    group, stage = rng.integers(0, G, n), rng.integers(0, S, n).astype(np.float32)
    prev = previous(rng, stage, S)
    at = 1234
    if bad.startswith("label"):
        group[at] = -1 if bad == "label -1" else G
        bit = N.GJ_STAGE_ERR_LABEL
    else:
        stage[at] = {"nan": np.nan, "2.5": 2.5, "-1": -1.0, "S": float(S)}[bad]
        bit = N.GJ_STAGE_ERR_STAGE
    for offset in (0, 1):
        got, stats = run_stage_stats(device, group, G, S, stage, prev, offset, check=False)
        got = got.cpu().numpy()
        keep = np.arange(n) != at
        assert np.array_equal(got, expected(group[keep], G, S, stage[keep], prev[keep]))      # numpy on the others
        assert got[0].sum() == n - 1
        assert int(stats.err.item()) == bit
        with pytest.raises(StageLabelError, match="label" if bit == N.GJ_STAGE_ERR_LABEL else "stage"):
            stats.check()
        stats.check()                                                                          # raised once, then clear


# ---- 4. the reference's own 90-day run -----------------------------------------------------------------------------------
def test_the_reference_run_row_by_row(device):
    z = L.load_npz("june769_series.npz")
    rows, dead = z["post/current_stage"], int(z["dead_stage"])
    S, T = dead + 1, rows.shape[0]
    area = (z["age"] % 5).astype(np.int32)                       # any labelling: five groups
    national, by_group = StageStats(None, 1, S, device=device), StageStats(torch.from_numpy(area), 5, S, device=device)
    dev_rows = torch.from_numpy(rows).to(device)
    out = torch.zeros(T, 2, 1, S, dtype=torch.int64, device=device)
    out_g = torch.zeros(T, 2, 5, S, dtype=torch.int64, device=device)
    for t in range(T):
        prev = dev_rows[t - 1] if t else None
        national.add(dev_rows[t], prev, out[t])
        by_group.add(dev_rows[t], prev, out_g[t])
    national.check()
    by_group.check()
    out, out_g = out.cpu().numpy(), out_g.cpu().numpy()
    for t in range(T):
        assert np.array_equal(out[t, 0, 0], np.bincount(rows[t].astype(np.int64), minlength=S)), t
        assert out[t, 0, 0, dead] == z["results/deaths_per_timestep"][t + 1], t
        for s in range(S):
            want = (rows[t] == s) & (rows[t - 1] != s) if t else np.zeros(rows.shape[1], bool)
            assert out[t, 1, 0, s] == want.sum(), (t, s)
            assert np.array_equal(out_g[t, 1, :, s], np.bincount(area[want], minlength=5)), (t, s)
    assert np.array_equal(out_g.sum(2), out[:, :, 0])
    assert (out[:, 0, 0].max(0) > 0).all(), "the record occupies all eight stages"
    entries = out[:, 1, 0].sum(0)
    print("entries by stage over the 90 days:", dict(zip(STAGES, entries.tolist())))
    assert all(entries[s] > 0 for s in range(S) if STAGES[s] != "susceptible"), "a column without an entry"


# ---- 5. the adjoint -------------------------------------------------------------------------------------------------------
def _adjoint_reference(group, G, S, stage, prev, w_occ, w_ent):
    """torch autograd (fp64, CPU) of sum_{g,s} w[g,s] * sum_a (group == g) * (stage == s) * stage / s, the entries with
    their constant mask (prev != stage): taken over the terms that are not identically zero - agent a contributes to
    (group[a], stage[a]) alone - and over s >= 1, where the form is defined."""
    g = np.zeros(stage.shape, np.int64) if group is None else group.astype(np.int64)
    with np.errstate(invalid="ignore"):
        ok = (g >= 0) & (g < G) & (stage >= 1) & (stage < S) & (stage == np.trunc(stage))
    idx = torch.from_numpy(np.nonzero(ok)[0])
    x = torch.from_numpy(stage.astype(np.float64)).requires_grad_(True)
    s = torch.from_numpy(stage[ok].astype(np.int64))
    gi = torch.from_numpy(g[ok])
    xs = x[idx]
    term = (xs == s.double()) * xs / s.double()
    entered = torch.from_numpy((prev != stage)[ok])
    loss = (torch.from_numpy(w_occ.astype(np.float64))[gi, s] * term).sum() + \
           (torch.from_numpy(w_ent.astype(np.float64))[gi, s] * term * entered).sum()
    (grad,) = torch.autograd.grad(loss, x)
    return grad.numpy(), ok


@pytest.mark.parametrize("case", ["null", 5, "adj", "adj+1", "lds+1"])
@pytest.mark.parametrize("n", [1, 63, 4099])
def test_adjoint_equals_torch_autograd(device, n, case):
    S = 8
    G = {"adj": N.GJ_STAGE_ADJ_LDS_BINS // S, "adj+1": N.GJ_STAGE_ADJ_LDS_BINS // S + 1}.get(case, _groups_of(case, S))
    rng = np.random.default_rng(n + (0 if G is None else G))
    group = None if G is None else rng.integers(0, G, n)
    stage = rng.integers(0, S, n).astype(np.float32)                # stage 0 included
    prev = previous(rng, stage, S)
    if n > 10:                                                       # bad stages and labels: exactly 0
        stage[[3, 4, 5, 6]] = [np.nan, 2.5, -1.0, float(S)]
        if G is not None:
            group[[7, 8]] = [-1, G]
    w_occ = rng.standard_normal((G or 1, S)).astype(np.float32)
    w_ent = rng.standard_normal((G or 1, S)).astype(np.float32)
    want, ok = _adjoint_reference(group, G or 1, S, stage, prev, w_occ, w_ent)
    atol = 1e-6 * max(np.abs(w_occ).max(), np.abs(w_ent).max())
    for offset in (0, 1):
        stats = StageStats(None if G is None else offset_tensor(group.astype(np.int32), device, offset), G or 1, S,
                           device=device)
        cur, prv = offset_tensor(stage, device, offset), offset_tensor(prev, device, offset)
        both = stats.gather(cur, prv, torch.from_numpy(w_occ).to(device), torch.from_numpy(w_ent).to(device))
        got = both.cpu().numpy()
        assert np.all(got[~ok] == 0.0), "0 for stage 0, a bad label or a bad stage"
        assert np.allclose(got, want, rtol=1e-6, atol=atol), np.abs(got - want).max()
        # a NULL table is zeros; without a previous stage there are no entries
        only_occ = stats.gather(cur, prv, torch.from_numpy(w_occ).to(device), None).cpu().numpy()
        no_prev = stats.gather(cur, None, torch.from_numpy(w_occ).to(device), torch.from_numpy(w_ent).to(device)).cpu().numpy()
        want_occ, _ = _adjoint_reference(group, G or 1, S, stage, prev, w_occ, np.zeros_like(w_ent))
        assert np.allclose(only_occ, want_occ, rtol=1e-6, atol=atol) and np.array_equal(only_occ, no_prev)


# ---- the Runner on the bundled world ---------------------------------------------------------------------------------------
TOTAL_DAYS = 30


def _params(device, days=TOTAL_DAYS, **extra):
    """test_gpu_group_series._params, and - as the record of the reference's 90-day run does (make_golden.py) - the
    later stages made likely: the default severity table kills about one in 10^4 of the infected, so no run of 769
    agents would ever enter `critical` or `dead`."""
    from grad_june_amd.defaults import default_parameters

    p = default_parameters(str(device))
    p["timer"]["total_days"] = days
    p["infection_seed"]["log_fraction_initial_cases"] = -1.3
    for n in p["networks"]:
        p["networks"][n]["log_beta"] += 0.6
    for stage in ("symptomatic", "severe", "critical"):
        p["symptoms"]["stage_transition_probabilities"][stage] = {"0-100": 0.8}
    p.update(extra)
    return p


def _snapshotting(base):
    class Snapshots(base):
        """Keeps, for every row, the previous stage the row was counted against and the stage itself (on the graph in a
        differentiable run)."""

        def _record_stages(self, data, row, diff_rows=None):
            stage = data["agent"].symptoms["current_stage"]
            self.snapshots.append((self._stage_prev.detach().clone(),
                                   stage if diff_rows is not None else stage.detach().clone()))
            super()._record_stages(data, row, diff_rows)

    return Snapshots


def _runner(params, seed=21):
    import grad_june_amd as G
    from grad_june_amd import infection

    torch.manual_seed(seed)
    infection._philox_step = itertools.count(1 << 40)
    runner = _snapshotting(G.Runner).from_parameters(params)
    runner.snapshots = []
    return runner


def _run(params):
    runner = _runner(params)
    with torch.no_grad():
        results, is_infected = runner()
    return runner, results, is_infected


@pytest.fixture(scope="module")
def plain_all(device):
    """The plain run with every stage saved, by area too: shared by the tests below, never modified."""
    return _run(_params(device, stages_to_save="all", groups_to_save=["area"]))


@pytest.fixture(scope="module")
def plain_without(device):
    """The same run without stages_to_save."""
    return _run(_params(device, groups_to_save=["area"]))


def _assert_coverage(results):
    for st in STAGES[2:]:
        assert float(results[f"new_{st}_per_timestep"].detach().sum()) >= 1, f"nobody entered '{st}': lengthen the run"


def test_runner_plain_series(device, plain_all, plain_without, tmp_path):
    runner, res, inf = plain_all
    _, without, inf_without = plain_without
    for key, value in without.items():                           # nothing that existed changes by a bit
        assert value == res[key] if key == "dates" else torch.equal(value, res[key]), key
    assert torch.equal(inf_without, inf)
    new_keys = sorted(set(res) - set(without))
    assert new_keys == sorted(f"{p}{st}_{tail}" for p in ("", "new_") for st in STAGES for tail in ("per_timestep", "by_area"))
    _assert_coverage(res)
    T, A = len(res["dates"]), runner.n_agents
    assert torch.equal(res["dead_per_timestep"], res["deaths_per_timestep"])
    assert torch.equal(res["dead_by_area"], res["deaths_by_area"])
    occupancy = torch.stack([res[f"{st}_per_timestep"] for st in STAGES], 1)
    assert occupancy.shape == (T, 8) and occupancy.dtype == torch.float32
    assert torch.equal(occupancy.sum(1), torch.full((T,), float(A), device=occupancy.device))
    for st in STAGES:
        for p in ("", "new_"):
            by_area = res[f"{p}{st}_by_area"]
            assert by_area.shape == (T, 3) and by_area.dtype == torch.float32
            assert torch.equal(by_area.sum(1), res[f"{p}{st}_per_timestep"]), (p, st)
    # numpy on the stage at every row; row 0 against the restored initial stage
    assert len(runner.snapshots) == T
    initial = runner.data_backup["symptoms"]["current_stage"].to(torch.float32)
    assert torch.equal(runner.snapshots[0][0], initial)
    area = runner.data["agent"].group_labels["area"].cpu().numpy()
    for t, (prev, stage) in enumerate(runner.snapshots):
        prev, stage = prev.cpu().numpy(), stage.cpu().numpy()
        if t:
            assert np.array_equal(prev, runner.snapshots[t - 1][1].cpu().numpy())
        want = expected(area, 3, 8, stage, prev)
        for s, st in enumerate(STAGES):
            assert np.array_equal(res[f"{st}_by_area"][t].cpu().numpy(), want[0, :, s]), (t, st)
            assert np.array_equal(res[f"new_{st}_by_area"][t].cpu().numpy(), want[1, :, s]), (t, st)
    seeded = float(res["new_exposed_per_timestep"][0])
    assert seeded == float(res["cases_per_timestep"][0]) > 0        # row 0: the agents the seed moved
    # save_results: the 1-D keys in results.csv, two columns per saved stage behind the three of results_by_area.csv
    import pandas as pd

    runner.save_path = tmp_path
    runner.save_results(res, inf)
    flat = pd.read_csv(tmp_path / "results.csv")
    assert {"severe_per_timestep", "new_severe_per_timestep"} <= set(flat.columns)
    by_area = pd.read_csv(tmp_path / "results_by_area.csv")
    assert list(by_area.columns) == ["date", "area", "cases", "daily_cases", "deaths"] + \
        [c for st in STAGES for c in (st, "new_" + st)]
    assert np.array_equal(by_area["new_severe"].to_numpy().reshape(T, 3), res["new_severe_by_area"].cpu().numpy())


def test_runner_selected_stages(device, plain_all, plain_without):
    _, res_all, _ = plain_all
    _, without, _ = plain_without
    _, res, _ = _run(_params(device, stages_to_save=["severe", "critical"], groups_to_save=["area"]))
    wanted = {f"{p}{st}_{tail}" for p in ("", "new_") for st in ("severe", "critical") for tail in ("per_timestep", "by_area")}
    assert set(res) - set(without) == wanted
    for key in wanted:
        assert torch.equal(res[key], res_all[key]), key


def _differentiable(runner):
    nets = runner.model.infection_networks.networks
    for n in nets.values():
        n.log_beta = torch.nn.Parameter(n.log_beta.detach().clone())
    results, _ = runner()
    return results, [n.log_beta for n in nets.values()]


def _grads(loss, betas):
    return [0.0 if g is None else float(g) for g in torch.autograd.grad(loss, betas, retain_graph=True, allow_unused=True)]


def test_runner_differentiable_series(device, plain_all, plain_without):
    _, plain, _ = plain_all
    new_keys = set(plain) - set(plain_without[1])
    runner = _runner(_params(device, stages_to_save="all", groups_to_save=["area"]))
    res, betas = _differentiable(runner)
    _assert_coverage(res)
    for key in sorted(new_keys | {"deaths_per_timestep", "deaths_by_area"}):
        assert torch.equal(res[key].detach(), plain[key]), key
    assert res["severe_per_timestep"].requires_grad and res["new_severe_by_area"].requires_grad
    # the deaths, through either node
    a, b = _grads(res["dead_per_timestep"].sum(), betas), _grads(res["deaths_per_timestep"].sum(), betas)
    print("d dead:", a, "\nd deaths:", b)
    assert any(v != 0.0 for v in b)
    for x, y in zip(a, b):
        assert x == pytest.approx(y, rel=1e-6, abs=0.0)
    # a weighted loss on three of the series against the same loss in torch ops on the per-row stage tensors
    T = len(res["dates"])
    gen = torch.Generator().manual_seed(5)
    w1, w2 = torch.rand(T, generator=gen).to(device) + 0.5, torch.rand(T, generator=gen).to(device) + 0.5
    w3 = torch.rand(T, 3, generator=gen).to(device) + 0.5
    loss = (w1 * res["severe_per_timestep"]).sum() + (w2 * res["new_critical_per_timestep"]).sum() + \
           (w3 * res["new_severe_by_area"]).sum()
    area = runner.data["agent"].group_labels["area"].to(device).long()
    onehot = torch.nn.functional.one_hot(area, 3).to(torch.float32)                  # [A, 3]
    dense = 0.0
    for t, (prev, stage) in enumerate(runner.snapshots):
        entered = (prev != stage.detach()).to(torch.float32)
        severe, critical = (stage == 5.0) * stage / 5.0, (stage == 6.0) * stage / 6.0
        dense = dense + w1[t] * severe.sum() + w2[t] * (critical * entered).sum() + \
            (w3[t] * ((severe * entered) @ onehot)).sum()
    assert float(loss.detach()) == pytest.approx(float(dense.detach()), rel=1e-5)           # (fp32 sums of ~100 weighted counts)
    got, want = _grads(loss, betas), _grads(dense, betas)
    print("d loss, node:", got, "\nd loss, torch ops:", want)
    scale = max(abs(v) for v in want)
    assert sum(v != 0.0 for v in got) >= 5
    for x, y in zip(got, want):
        assert abs(x - y) <= 2e-5 * abs(y) + 2e-5 * scale, (x, y)


# ---- two ranks ---------------------------------------------------------------------------------------------------------
def _stage_worker(rank, R, port, out):
    """DistributedRunner with stages_to_save on two ranks (gloo), plain and differentiable, against the single-GPU Runner."""
    import os

    import torch.distributed as dist

    import grad_june_amd as G
    from grad_june_amd import infection
    from grad_june_amd.distributed_api import DistributedRunner

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=R)
    try:
        def run(runner, differentiable):
            nets = runner.model.infection_networks.networks
            if not differentiable:
                with torch.no_grad():
                    return runner()[0], None
            for n in nets.values():
                n.log_beta = torch.nn.Parameter(n.log_beta.detach().clone())
            results, _ = runner()
            w = torch.linspace(0.5, 1.5, 3, device=results["severe_by_area"].device)
            loss = (results["severe_by_area"] * w).sum() + 3.0 * results["new_critical_per_timestep"].sum() + \
                results["dead_per_timestep"].sum() + (results["new_symptomatic_by_area"] * w).sum()
            loss.backward()
            return results, {k: (None if n.log_beta.grad is None else float(n.log_beta.grad)) for k, n in nets.items()}

        params = lambda: _params("cuda:0", stages_to_save="all", groups_to_save=["area"])      # noqa: E731
        for differentiable in (False, True):
            torch.manual_seed(33)
            infection._philox_step = itertools.count(1 << 40)        # the seeding stream of a fresh process
            runner = DistributedRunner.from_parameters(params())
            assert runner.n_agents < 769 and runner.stages_saved == STAGES
            res, grads = run(runner, differentiable)
            gathered = [None] * R
            dist.all_gather_object(gathered, grads)
            assert gathered[0] == gathered[1], "every rank holds the whole gradient"
            if rank == 0:
                torch.manual_seed(33)
                infection._philox_step = itertools.count(1 << 40)
                ref_res, ref = run(G.Runner.from_parameters(params()), differentiable)
                _assert_coverage(ref_res)
                for st in STAGES:
                    for key in (f"{st}_per_timestep", f"new_{st}_per_timestep", f"{st}_by_area", f"new_{st}_by_area"):
                        assert torch.equal(res[key].detach().cpu(), ref_res[key].detach().cpu()), (differentiable, key)
                if differentiable:
                    nonzero = 0
                    for k, g in ref.items():
                        if g is None:
                            assert grads[k] is None, k
                            continue
                        assert grads[k] == pytest.approx(g, rel=2e-5, abs=1e-7), (k, grads[k], g)
                        nonzero += g != 0.0
                    assert nonzero >= 5
                    out[0] = 1
    finally:
        dist.destroy_process_group()


def test_two_ranks_stage_series_match_single_gpu(device):
    import os

    import torch.multiprocessing as mp

    R = 2
    out = mp.get_context("spawn").Array("i", [0])
    mp.spawn(_stage_worker, args=(R, 29600 + os.getpid() % 90, out), nprocs=R, join=True)
    assert out[0] == 1
