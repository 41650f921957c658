"""Generate grads_params.npz by RUNNING THE REFERENCE: gradients w.r.t. the transmission-profile parameters.

Run once, where the reference tree exists (as make_golden.py, whose helpers this imports):

    python tests/golden/make_golden_params.py

The four TransmissionSampler distributions are built on nn.Parameters (loc and scale of each) and the per-agent
profile is drawn with the reference's own ``rsample`` (transmission.py:15-20).  Then the reference runs 4 / 6 timesteps
on its autograd graph with the sampler noise recorded, like grads.npz.  Recorded per case (p1: the 100-agent world,
three networks; p2: the 769-agent world, default parameters + quarantine + distancing), in grads.npz's layout and
keys plus:
    dist/<param>/loc, dist/<param>/scale        the distribution parameters
    grad_<loss>/dist/<param>/{loc,scale}        d loss / d them (reference autograd)
    grad_<loss>/agent/<param>                   d loss / d the drawn per-agent values
    state0/<param>                              the drawn per-agent values (as grads.npz)
for the losses ``last`` (infected count after the last step) and ``series`` (sum over the steps), next to the
log_beta gradients of the same run (``grad_<loss>/<network>``).
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as MG  # noqa: E402  (imports the reference through _pyg_standin)

import torch  # noqa: E402

PROFILE = ("max_infectiousness", "shape", "rate", "shift")


def parameterised_profile(params, n, out, prefix):
    """Draw the profile with rsample from distributions whose loc / scale are leaves; returns (leaves, drawn rows)."""
    leaves, dists = {}, {}
    for k in PROFILE:
        spec = params["transmission"][k]
        loc = torch.nn.Parameter(torch.tensor(float(spec["loc"])))
        scale = torch.nn.Parameter(torch.tensor(float(spec["scale"])))
        leaves[k] = (loc, scale)
        dists[k] = getattr(torch.distributions, spec["dist"])(loc, scale)
        out[f"{prefix}dist/{k}/kind"] = np.array(spec["dist"])
        out[f"{prefix}dist/{k}/loc"] = np.float32(loc.item())
        out[f"{prefix}dist/{k}/scale"] = np.float32(scale.item())
    v = MG.TransmissionSampler(*[dists[k] for k in PROFILE])(n)
    return leaves, {k: v[i] for i, k in enumerate(PROFILE)}


def run_case(model, data, timer, n_steps, out, prefix, leaves, rows):
    """make_golden.run_with_grads on the parameterised profile; the gradients of each of its two backward calls are
    caught by hooks (they fire once per backward with that call's gradient)."""
    caught = {}
    for k in PROFILE:
        for which, t in zip(("loc", "scale"), leaves[k]):
            t.register_hook(lambda g, key=f"dist/{k}/{which}": caught.setdefault(key, []).append(g.detach().clone()))
        rows[k].register_hook(lambda g, key=f"agent/{k}": caught.setdefault(key, []).append(g.detach().clone()))
    data["agent"].infection_parameters = dict(rows)
    MG.run_with_grads(model, data, timer, n_steps, out, prefix, step_first=True)
    for key, gs in caught.items():
        assert len(gs) == 2, key
        for tag, g in zip(("last", "series"), gs):
            out[f"{prefix}grad_{tag}/{key}"] = g.numpy().astype(np.float32)
    print(prefix, {k: float(out[f"{prefix}grad_series/dist/{k}/loc"]) for k in PROFILE})


def make_grads_params():
    out = {}
    params = MG.default_params()
    # p1: the 100-agent fixture, three networks, 4 steps (grads.npz g1's set-up)
    data = MG.conftest_data()
    MG.seed_all(41)
    leaves, rows = parameterised_profile(params, len(data["agent"].id), out, "p1/")
    MG.flat_world(MG.world_of(data), out, prefix="p1/world/")
    nets = MG.InfectionNetworks(household=MG.HouseholdNetwork(log_beta=0.2), company=MG.CompanyNetwork(log_beta=0.4),
                                school=MG.SchoolNetwork(log_beta=0.3))
    model = MG.GradJune(infection_networks=nets, policies=MG.Policies.from_policy_list([]))
    timer = MG.Timer(initial_day="2022-02-01", total_days=10, weekday_step_duration=(24,), weekend_step_duration=(24,),
                     weekday_activities=(("company", "school", "household"),),
                     weekend_activities=(("company", "school", "household"),))
    next(timer); next(timer)
    run_case(model, data, timer, 4, out, "p1/", leaves, rows)
    # p2: the 769-agent world, default parameters + quarantine + distancing (grads.npz g2's set-up), 6 steps
    p2 = MG.default_params()
    p2["policies"]["quarantine"] = {
        "quarantine": {1: {"start_date": "2022-02-03", "end_date": "2022-02-20", "stage_threshold": 4}}}
    p2["policies"]["interaction"]["social_distancing"][1]["start_date"] = "2022-02-04"
    for n in p2["networks"]:
        p2["networks"][n]["log_beta"] += 0.7
    MG.seed_all(78)
    runner = MG.Runner.from_parameters(p2)
    with torch.no_grad():
        runner.timer.reset()
        runner.restore_initial_data()
        runner.set_initial_cases()
    leaves, rows = parameterised_profile(p2, len(runner.data["agent"].id), out, "p2/")
    MG.flat_world(MG.world_of(runner.data), out, prefix="p2/world/")
    for n, t in MG.tables_of(runner.model).items():
        out["p2/table/" + n] = t.numpy()
    run_case(runner.model, runner.data, runner.timer, 6, out, "p2/", leaves, rows)
    MG.save("grads_params.npz", out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    make_grads_params()
