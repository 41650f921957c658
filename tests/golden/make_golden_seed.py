"""Generate grads_seed.npz by RUNNING THE REFERENCE: gradients w.r.t. the initial-case fraction(s).

Run once, where the reference tree exists (as make_golden.py, whose helpers this imports):

    python tests/golden/make_golden_seed.py

The 769-agent world, default parameters with every log_beta raised by 0.7 (as grads.npz's g2 / g3), 4 timesteps after
the seed, the whole run on the reference's autograd graph with every draw recorded (the seed's and the steps' sampler
noise, the symptoms draws of every call as in grads_symptoms.npz).  Two cases:

    s1/  national: the reference's own ``Runner.set_initial_cases`` with ``log_fraction_initial_cases`` an nn.Parameter
    s2/  three groups derived from the agents' areas: ``probs = (10 ** log_fraction)[labels]`` fed to the reference's
         IsInfectedSampler, infect_people and symptoms_updater (the reference has no group seeding of its own)

Recorded per case, in grads.npz's layout and keys (state0 = the state AFTER the seed) plus:
    seed/log_fraction [G], seed/labels [n] (int32), seed/now, seed/exp_noise [2, n], seed/new_infected
    seed/pre/<state>, seed/pre/sym/<key>         the state before the seed
    seed/sym/..., step<i>/sym/...                the symptoms draws and states of every call (grads_symptoms.npz's keys)
    grad_<loss>/log_fraction [G]                 d loss / d log_fraction (reference autograd), next to grad_<loss>/<network>
    torch_seed                                   the seed that was used
for the losses ``last`` and ``series``.  The generator asserts that every fraction gradient is finite and non-zero and
that the seed infects at least one agent of every group; if not, change TORCH_SEED.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as MG  # noqa: E402  (imports the reference through _pyg_standin)

import torch  # noqa: E402
import grad_june.infection as ref_infection  # noqa: E402

TORCH_SEED = {"s1/": 211, "s2/": 212}
N_STEPS = 4
SYM = ("current_stage", "next_stage", "time_to_next_stage")


def area_groups(n_groups=3):
    """Labels 0 .. n_groups-1 from the shipped world's areas: the sorted distinct areas cut into equal runs."""
    with np.load(os.path.join(MG.HERE, "world769.npz"), allow_pickle=False) as z:
        area = z["agent/area"]
    uniq, inverse = np.unique(area, return_inverse=True)
    labels = (inverse.reshape(-1) * n_groups // len(uniq)).astype(np.int32)
    assert np.bincount(labels, minlength=n_groups).min() >= 20
    return labels


def run_case(prefix, log_fraction, labels, out):
    params = MG.default_params()
    for n in params["networks"]:
        params["networks"][n]["log_beta"] += 0.7
    MG.seed_all(TORCH_SEED[prefix])
    runner = MG.Runner.from_parameters(params)
    model, data, timer = runner.model, runner.data, runner.timer
    A = len(data["agent"].id)
    timer.reset()
    runner.restore_initial_data()
    MG.flat_world(MG.world_of(data), out, prefix=prefix + "world/")
    for n, t in MG.tables_of(model).items():
        out[prefix + "table/" + n] = t.numpy()
    out[prefix + "sym_table"] = model.symptoms_updater.symptoms_sampler.stage_transition_probabilities.numpy()
    for k, v in MG.state_of(data).items():
        out[f"{prefix}seed/pre/{k}"] = v.numpy().copy()
    for k in SYM:
        out[f"{prefix}seed/pre/sym/{k}"] = data["agent"].symptoms[k].detach().float().numpy().copy()
    sym_rec = MG._SymptomsRecorder(model.symptoms_updater)
    model.symptoms_updater = sym_rec
    seed_rec = MG._NoiseRecorder(ref_infection.IsInfectedSampler())
    leaf = torch.nn.Parameter(torch.tensor(log_fraction, dtype=torch.float32))
    caught = []
    leaf.register_hook(lambda g: caught.append(g.detach().clone()))
    if labels is None:                      # s1: the reference's Runner, its sampler recorded
        real = ref_infection.IsInfectedSampler
        ref_infection.IsInfectedSampler = lambda: seed_rec
        try:
            runner.log_fraction_initial_cases = leaf
            runner.set_initial_cases()
        finally:
            ref_infection.IsInfectedSampler = real
        out[prefix + "seed/labels"] = np.zeros(A, dtype=np.int32)
    else:                                   # s2: reference functions on probs = fraction[labels]
        probs = (10.0 ** leaf)[torch.from_numpy(labels).long()]
        new_infected = seed_rec(1.0 - probs)
        ref_infection.infect_people(data, timer, new_infected)
        model.symptoms_updater(data=data, timer=timer, new_infected=new_infected)
        out[prefix + "seed/labels"] = labels
    lab = out[prefix + "seed/labels"]
    new = data["agent"].is_infected.detach().numpy().copy()        # everybody starts at 0: the seed's decisions
    assert all(new[lab == g].sum() >= 1 for g in range(int(lab.max()) + 1)), "a group without an initial case"
    out[prefix + "seed/log_fraction"] = np.atleast_1d(leaf.detach().numpy()).astype(np.float32)
    out[prefix + "seed/now"] = np.float64(timer.now)
    out[prefix + "seed/exp_noise"] = seed_rec.noise[0].numpy().copy()
    out[prefix + "seed/new_infected"] = new
    for k in SYM:
        out[f"{prefix}state0/sym/{k}"] = data["agent"].symptoms[k].detach().float().numpy().copy()
    MG.run_with_grads(model, data, timer, N_STEPS, out, prefix, step_first=True)
    assert len(sym_rec.calls) == N_STEPS + 1 and len(caught) == 2
    for i, rec in enumerate(sym_rec.calls):
        for k, v in rec.items():
            out[f"{prefix}{'seed' if i == 0 else f'step{i - 1}'}/sym/{k}"] = v
    for tag, g in zip(("last", "series"), caught):
        g = np.atleast_1d(g.numpy()).astype(np.float32)
        assert np.all(np.isfinite(g)) and np.all(g != 0.0), (prefix, tag, g)
        out[f"{prefix}grad_{tag}/log_fraction"] = g
    out[prefix + "torch_seed"] = np.int64(TORCH_SEED[prefix])
    print(prefix, "initial cases by group", np.bincount(lab, weights=new).tolist(),
          {t: out[f"{prefix}grad_{t}/log_fraction"].tolist() for t in ("last", "series")})


def make_grads_seed():
    out = {}
    run_case("s1/", -1.0, None, out)
    run_case("s2/", [-0.6, -1.0, -1.4], area_groups(), out)
    MG.save("grads_seed.npz", out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    make_grads_seed()
