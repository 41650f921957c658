"""GPU: one Runner with EVERY result series switched on at once, on the 769-agent world for 6 steps, against a recording.

The other series tests each turn on one series (or two); what one series' arming and clearing around the step does to
another's shows only with all of them in one time loop.  tests/golden/runner_all_series.npz holds what the runner gave
when the fixture was recorded - the ordered keys of ``results``, every tensor in it, the returned ``is_infected``, every
per-agent array the run leaves in ``data["agent"]`` and the text of every CSV ``save_results`` writes - once under
``torch.no_grad()`` and once in grad mode with the ``log_beta``s as ``nn.Parameter``s (forward values only).  Everything
is compared exactly: the counts are integers or fixed-point sums, the sampling is Philox keyed by seed, step and agent,
and two recordings on one MI355X gave the same bytes.

The symptom clock is shortened (days, not weeks, to symptoms and to recovery) so that within 6 steps agents turn
symptomatic - the Testing and the ContactQuarantine find somebody - and recover, wane and are infected again.

Record again (on the GPU, from the repository root) with

    python tests/test_gpu_runner_all_series.py --record [path]
"""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runner_all_series.npz")
DAYS, SEED = 6, 21
AGE_BANDS = {"age_band": {"attribute": "age", "bins": [0, 18, 65, 100]}}
PER_AGENT = ("infections_caused", "infected_row", "infector", "infection_location", "infection_venue", "offspring",
             "confirmed_time")
#: series that must not be all zero in the recording: a run in which a policy found nobody would pin nothing of it
LIVE = ("daily_cases_per_timestep", "new_symptomatic_per_timestep", "new_recovered_per_timestep",
        "infections_by_location", "infections_caused_per_timestep", "infection_matrix_by_age_band",
        "infections_sampled_by_location", "vaccine_doses_by_area", "reinfections_by_age_band",
        "quarantined_contacts_by_area", "isolating_by_age_band", "confirmed_cases_by_area")


def _params(device, save_path):
    """tests/test_gpu_testing.py::_params, with every series asked for."""
    from grad_june_amd.defaults import default_parameters

    p = default_parameters(str(device))
    p["timer"]["total_days"] = DAYS
    p["infection_seed"]["log_fraction_initial_cases"] = -1.0
    for n in p["networks"]:
        p["networks"][n]["log_beta"] += 1.0
    p["system"]["locality_order"] = "household"      # the per-agent results come back in the file's order
    p["groups_to_save"] = ["area", AGE_BANDS]
    p["stages_to_save"] = "all"
    p["locations_to_save"] = True
    p["infectors_to_save"] = True
    p["infection_matrices_to_save"] = ["age_band"]
    p["infection_tree_to_save"] = True
    # rows 1 .. 3: the Testing, with isolations that outlast it; rows 4 .. 6: the ContactQuarantine (no shared date)
    p["policies"]["testing"] = {"testing": {
        "start_date": "2022-02-01", "end_date": "2022-02-05", "stage_threshold": 4,
        "probability": {"0-18": 0.5, "18-65": 0.7, "65-100": 0.9}, "delay": {0: 0.5, 1: 0.5},
        "isolation": {"days": 2, "compliance": 0.8}}}
    p["policies"]["quarantine"] = {"contact_quarantine": {
        "start_date": "2022-02-05", "end_date": "2022-03-01", "stage_threshold": 4, "contacts": {"household": 7},
        "compliance": 0.9}}
    p["policies"]["vaccination"] = {"vaccination": {
        "start_date": "2022-01-30", "end_date": "2022-02-06", "coverage": {"18-65": 0.6, "65-100": 0.9},
        "efficacy": {"30-65": 0.8, "65-100": 0.6}}}
    p["immunity"] = {"half_life": {"0-40": 1.0, "40-100": 1.5}, "residual_protection": 0.1}
    times = p["symptoms"]["stage_transition_times"]
    times["exposed"].update(loc=-0.4, scale=0.3)         # about 0.7 days
    times["infectious"].update(loc=-0.5, scale=0.3)
    for stage in ("infectious", "symptomatic"):
        p["symptoms"]["recovery_times"][stage].update(loc=0.3, scale=0.25)      # about 1.3 days
    p["save_path"] = str(save_path)
    return p


def _run(device, save_path, grad):
    """The run's outcome as a flat {name: numpy array}: tensors as they are, text as numpy strings."""
    import grad_june_amd as G
    from grad_june_amd import infection

    torch.manual_seed(SEED)
    infection._philox_step = itertools.count(1 << 40)      # the seeding's Philox stream: the same for every run
    runner = G.Runner.from_parameters(_params(device, save_path))
    if grad:
        for net in runner.model.infection_networks.networks.values():
            net.log_beta = torch.nn.Parameter(net.log_beta.detach().clone())
    torch.manual_seed(SEED)
    infection._philox_step = itertools.count(1 << 40)
    with torch.set_grad_enabled(grad):
        results, is_infected = runner()
    runner.save_results(results, is_infected)
    out = {"keys": np.array(list(results)), "dates": np.array([str(d) for d in results["dates"]]),
           "is_infected": is_infected.detach().cpu().numpy()}
    for key, series in results.items():
        if key != "dates":
            out["results/" + key] = series.detach().cpu().numpy()
    for key in PER_AGENT:
        out["agent/" + key] = runner.data["agent"][key].detach().cpu().numpy()
    for name in sorted(os.listdir(save_path)):
        with open(os.path.join(save_path, name), newline="") as f:
            out["csv/" + name] = np.array(f.read())
    return out


def _same(a, b):
    """Same dtype, shape and bytes (a NaN - the generation interval of a row without a sampled infector - equals itself)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "U":
        return a.tolist() == b.tolist()
    a, b = (torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).view(torch.uint8) for x in (a, b))
    return torch.equal(a, b)


def _record(device, root):
    """{"no_grad/<name>": array} of the run under no_grad, and {"grad/<name>": array} for what the run in grad mode gives
    differently (the confirmed cases - float32 on the graph there - and with them results.csv); the rest of it is the
    no-grad run's entry."""
    out = {"no_grad/" + key: value for key, value in _run(device, os.path.join(root, "no_grad"), False).items()}
    for key, value in _run(device, os.path.join(root, "grad"), True).items():
        if "no_grad/" + key not in out or not _same(value, out["no_grad/" + key]):
            out["grad/" + key] = value
    return out


@pytest.fixture(scope="module")
def golden():
    """{mode: {name: array}} of the two recorded runs."""
    with np.load(GOLDEN, allow_pickle=False) as z:
        flat = {k: z[k] for k in z.files}
    no_grad = {k[len("no_grad/"):]: v for k, v in flat.items() if k.startswith("no_grad/")}
    return {"no_grad": no_grad, "grad": dict(no_grad, **{k[len("grad/"):]: v for k, v in flat.items() if k.startswith("grad/")})}


def test_the_recording_exercises_every_series(golden):
    for mode, want in golden.items():
        for key in LIVE:
            assert want["results/" + key].any(), (mode, key)
        assert len(want["dates"]) == DAYS + 1
        assert (want["agent/confirmed_time"] >= 0).any() and (want["agent/infector"] >= 0).any()


@pytest.mark.parametrize("mode", ["no_grad", "grad"])
def test_every_series_at_once_against_the_recording(device, tmp_path, golden, mode):
    got, want = _run(device, tmp_path, grad=mode == "grad"), golden[mode]
    assert got["keys"].tolist() == want["keys"].tolist()      # the keys of results, in their order
    assert sorted(got) == sorted(want)      # and the same per-agent arrays and CSV files
    for key, value in want.items():      # every tensor bit for bit, every text character for character
        assert _same(got[key], value), (key, got[key], value)


if __name__ == "__main__":
    import tempfile

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(ROOT, "gradabm-june_amd"))
    if "--record" not in sys.argv:
        sys.exit(__doc__)
    rest = sys.argv[sys.argv.index("--record") + 1:]
    path = rest[0] if rest else GOLDEN
    with tempfile.TemporaryDirectory() as tmp:
        recorded = _record(torch.device("cuda:0"), tmp)
    for key in LIVE:
        print(key, float(recorded["no_grad/results/" + key].sum()))
    print("differently in grad mode:", [key for key in recorded if key.startswith("grad/")])
    np.savez_compressed(path, **recorded)
    print("recorded", path, os.path.getsize(path), "bytes")
