"""GPU: the transmission tree through the step and the Runner, on the bundled 769-agent world: what must hold of any
tree a run writes - every infected agent has one entry, an infector was infected in an earlier row, the counts are the
daily new cases - and that the key changes no other result and no gradient by a bit."""
import numpy as np
import pytest
import torch

from grad_june_amd import _native as N
from test_gpu_location_series import PARENT_KEYS, _differentiable, _params, _run

pytestmark = pytest.mark.gpu

NEW_KEYS = {"infections_sampled_by_location", "infections_unresolved_per_timestep", "generation_interval_per_timestep"}
PER_AGENT = ("infector", "infection_location", "infection_venue", "infected_row", "offspring")


@pytest.fixture(scope="module")
def with_key(device):
    return _run(_params(device, infection_tree_to_save=True))


@pytest.fixture(scope="module")
def without_key(device):
    lib = N.load()
    calls, real = [], lib.gj_infection_tree
    try:
        lib.gj_infection_tree = lambda *a: (calls.append(1), real(*a))[1]
        out = _run(_params(device))
    finally:
        lib.gj_infection_tree = real
    return out + (calls,)


def test_the_tree_of_a_run(with_key, tmp_path):
    runner, res, inf = with_key
    assert NEW_KEYS <= set(res)
    T, keys = len(res["dates"]), runner.location_keys
    assert keys == list(runner.model.infection_networks.networks) + ["background", "seed"]
    counts = res["infections_sampled_by_location"]
    assert counts.shape == (T, len(keys)) and counts.dtype == torch.float64 and not counts.requires_grad
    counts = counts.cpu().numpy()
    daily = res["daily_cases_per_timestep"].cpu().numpy().astype(np.int64)
    assert daily.sum() > 100
    assert np.array_equal(counts.sum(1), daily)                                    # exactly the daily new cases
    col = {k: i for i, k in enumerate(keys)}
    assert counts[0, col["seed"]] == daily[0] > 0 and counts[0].sum() == daily[0]   # row 0 lies in `seed`
    assert not counts[1:, col["seed"]].any()
    ag = runner.data["agent"]
    infector, via, venue, row, offspring = (ag[k].cpu().numpy() for k in PER_AGENT)
    assert all(ag[k].dtype == torch.int32 for k in PER_AGENT[:4]) and ag["offspring"].dtype == torch.int64
    ever = inf.cpu().numpy() > 0
    assert np.array_equal(row >= 0, ever)                                          # every agent ever infected, no other
    assert np.array_equal(infector != -1, ever) and np.array_equal(via >= 0, ever)
    assert np.array_equal(np.bincount(row[ever], minlength=T), daily)
    assert np.array_equal(np.stack([np.bincount(via[row == r], minlength=len(keys)) for r in range(T)]), counts)
    assert (infector[row == 0] == -2).all() and (via[row == 0] == col["seed"]).all()
    has = infector >= 0
    assert has.sum() > 50 and (infector[has] < runner.n_agents).all()
    assert (row[infector[has]] >= 0).all() and (row[infector[has]] < row[has]).all()      # infected in an earlier row
    assert (infector[has] != np.nonzero(has)[0]).all()
    assert offspring.sum() == has.sum() and np.array_equal(offspring, np.bincount(infector[has], minlength=len(row)))
    through = has | (infector == -3)                                               # came through a venue of a network
    assert (venue[through] >= 0).all() and (venue[~through] == -1).all()
    assert (via[through] < col["background"]).all() and (via[infector == -2] >= col["background"]).all()
    unresolved = res["infections_unresolved_per_timestep"].cpu().numpy()
    assert unresolved.shape == (T,) and unresolved.sum() == (infector == -3).sum()
    assert np.array_equal(unresolved, np.bincount(row[infector == -3], minlength=T))
    # the generation interval: the mean over a row's infections with an infector of the days back to the infector's row
    days = np.array([(d - res["dates"][0]).total_seconds() / 86400.0 for d in res["dates"]])
    gi = res["generation_interval_per_timestep"].cpu().numpy()
    assert gi.shape == (T,) and gi.dtype == np.float32
    for r in range(T):
        mine = has & (row == r)
        if not mine.any():
            assert np.isnan(gi[r]), r
        else:
            want = (days[r] - days[row[infector[mine]]]).mean()
            assert want > 0 and abs(gi[r] - want) <= 1e-6 * want, (r, gi[r], want)
    assert np.isnan(gi[0]) and np.nanmax(gi) > 1.0
    print("offspring distribution:", np.bincount(offspring[ever]).tolist(), "mean generation interval (days):",
          float(np.nanmean(gi)), "unresolved:", int(unresolved.sum()), "of", int(daily.sum()))
    # the CSV: one line per infected agent
    import pandas as pd

    runner.save_path = tmp_path
    runner.save_results(res, inf)
    lines = pd.read_csv(tmp_path / "results_infection_tree.csv")
    assert list(lines.columns) == ["infected", "infector", "date", "location", "venue"] and len(lines) == ever.sum()
    assert np.array_equal(lines["infected"].to_numpy(), np.nonzero(ever)[0])
    assert np.array_equal(lines["infector"].to_numpy(), infector[ever])
    assert list(lines["location"]) == [keys[c] for c in via[ever]]
    assert list(pd.to_datetime(lines["date"])) == [pd.Timestamp(res["dates"][r]) for r in row[ever]]


def test_the_key_changes_no_other_result(with_key, without_key, device):
    runner, res, inf = with_key
    plain_runner, plain, plain_inf, calls = without_key
    assert calls == []                                                              # off: never launched
    assert plain_runner._tree() is None and plain_runner.model.tree_stats is None
    plan = plain_runner.model._engine(plain_runner.data, torch.device(device)).plan
    assert getattr(plan, "_venue_rows", None) is None                               # ... and nothing built
    assert not any(k in plain_runner.data["agent"] for k in PER_AGENT)
    assert set(plain) == PARENT_KEYS and set(res) - set(plain) == NEW_KEYS
    for key, value in plain.items():
        assert value == res[key] if key == "dates" else torch.equal(value, res[key]), key
    assert torch.equal(plain_inf, inf)


def test_the_same_run_writes_the_same_tree(with_key, device):
    runner, res, _ = with_key
    again, res2, _ = _run(_params(device, infection_tree_to_save=True))
    for k in PER_AGENT:
        assert torch.equal(runner.data["agent"][k], again.data["agent"][k]), k
    for k in NEW_KEYS:
        assert torch.equal(torch.nan_to_num(res[k], nan=-1.0), torch.nan_to_num(res2[k], nan=-1.0)), k


def test_the_infector_series_and_the_tree_write_the_same_rows(device):
    runner, res, _ = _run(_params(device, infection_tree_to_save=True, infectors_to_save=True))
    assert torch.equal(runner._tree().infected_row, runner._infectors().infected_row)
    assert torch.equal(runner.data["agent"]["infected_row"], runner._tree().infected_row)
    # nobody transmitted in the tree exactly where the infector series counts an unattributed infection
    T = len(res["dates"])
    tree = runner._tree()
    nobody = torch.bincount(tree.infected_row[tree.infector == -2].long(), minlength=T)
    assert torch.equal(nobody, runner._infectors().unattributed[:T])
    # an agent that was drawn as an infector has a credit in the infector series
    caused = runner.data["agent"]["infections_caused"]
    assert bool((caused[runner.data["agent"]["offspring"] > 0] > 0).all())


def test_a_renumbered_world_reports_the_tree_in_the_files_numbering(device):
    """``system.locality_order`` renumbers the agents at load time (so they draw anew: another tree); positions and the
    ids held in ``infector`` are reported in the file's order, like is_infected."""
    params = _params(device, infection_tree_to_save=True)
    params["system"]["locality_order"] = "household"
    runner, res, inf = _run(params)
    ag = runner.data["agent"]
    infector, row, offspring = (ag[k].cpu().numpy() for k in ("infector", "infected_row", "offspring"))
    ever = inf.cpu().numpy() > 0
    assert np.array_equal(row >= 0, ever) and ever.sum() > 100
    has = infector >= 0
    assert has.sum() > 50 and (row[infector[has]] >= 0).all() and (row[infector[has]] < row[has]).all()
    assert np.array_equal(offspring, np.bincount(infector[has], minlength=len(row)))
    daily = res["daily_cases_per_timestep"].cpu().numpy().astype(np.int64)
    assert np.array_equal(np.bincount(row[ever], minlength=len(daily)), daily)
    # an infector and the agent it infected share the venue: in the file's edge lists too
    keys, via, venue = runner.location_keys, ag["infection_location"].cpu().numpy(), ag["infection_venue"].cpu().numpy()
    nets = runner.model.infection_networks.networks
    original = ag.original_index.cpu().numpy()                 # original[new id] = the file's id
    for a in np.nonzero(has)[0][:40]:
        edges = runner.data["attends_" + nets[keys[via[a]]].edge_set].edge_index.cpu().numpy()
        at_venue = original[edges[0][edges[1] == venue[a]]]
        assert a in at_venue and infector[a] in at_venue, a


def test_a_differentiable_run_keeps_every_gradient_bit(device):
    days = 8
    runner, res, grads = _differentiable(_params(device, days=days, infection_tree_to_save=True))
    _, plain, plain_grads = _differentiable(_params(device, days=days))
    assert sum(g is not None and float(g) != 0.0 for g in grads) >= 5
    for a, b in zip(grads, plain_grads):
        assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes())
    for key in NEW_KEYS:
        assert key not in plain and not res[key].requires_grad and res[key].grad_fn is None
    for key, value in plain.items():
        assert value == res[key] if key == "dates" else torch.equal(value.detach(), res[key].detach()), key
    # the same tree as the plain (in-place) run of the same configuration
    same_runner, same, _ = _run(_params(device, days=days, infection_tree_to_save=True))
    for k in PER_AGENT:
        assert torch.equal(runner.data["agent"][k], same_runner.data["agent"][k]), k
    for key in NEW_KEYS:
        assert torch.equal(torch.nan_to_num(same[key], nan=-1.0), torch.nan_to_num(res[key], nan=-1.0)), key


def test_a_partitioned_run_refuses_the_key(device):
    from grad_june_amd.distributed_api import DistributedRunner

    with pytest.raises(NotImplementedError, match="partitioned"):
        DistributedRunner.from_parameters(_params(device, infection_tree_to_save=True))
