"""Time one backward step on a synthetic world (default C3, 10 M agents) with and without the transmission-profile
parameters requiring a gradient.

    python tools/param_grad_timing.py [--preset c3] [--agents A] [--steps 4] [--repeats 5] [--out FILE]

Modes (each: T chained ``autograd.HotPathStep`` nodes, loss = cases after the last step, ``loss.backward()``):
  log_beta  every network's log_beta a leaf (the form ``bench.py --backward`` measures);
  profile   + the four per-agent profile tensors as leaves: the profile's adjoint becomes
            gj_adjoint_transmission_params (+16 bytes per agent written per step) and torch accumulates
            4 x [A] gradients across the steps.
Prints one JSON object (per mode: forward / backward ms per step, medians over the repeats)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gradabm-june_amd"))

PROFILE = ("max_infectiousness", "shape", "rate", "shift")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", default="c3")
    ap.add_argument("--agents", type=int, default=None)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    import bench as B
    from types import SimpleNamespace

    from grad_june_amd.autograd import HotPathStep
    from grad_june_amd.benchrun import SingleGpuHotPath
    from grad_june_amd.synthetic import make_world, reorder_agents

    dev = torch.device("cuda", 0)
    t0 = time.time()
    world = reorder_agents(make_world(args.preset, n_agents=args.agents, seed=args.seed), by="household")
    networks, betas, specs = world["networks"], B.betas_of(world), B.network_specs(world)
    r = SingleGpuHotPath(world, specs, betas, dev, seed=args.seed, device_compile=True)
    print(f"[timing] world ready after {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    A = world["n_agents"]
    logb = {n: torch.nn.Parameter(torch.tensor(B.DEFAULT_LOG_BETA[n], device=dev)) for n in networks}
    nets = [SimpleNamespace(name=n, log_beta=logb[n]) for n in networks]
    fixed = {k: r.state[k] for k in PROFILE}
    state0 = [r.state[k].clone() for k in ("susceptibility", "is_infected", "infection_time")]
    T = args.steps

    def once(mode):
        profile = [fixed[k].clone().requires_grad_() for k in PROFILE] if mode == "profile" else []
        for v in logb.values():
            v.grad = None
        s, i, t = state0
        torch.cuda.synchronize()
        t_a = time.perf_counter()
        for k in range(T):
            params = r.engine.params(now=1.0 + k, delta_time=1.0, day_type=0, active=networks, betas=betas,
                                     seed=args.seed, step=k)
            env = {"engine": r.engine, "params": params, "fixed": fixed, "stage": None, "exp_noise": None,
                   "nets": nets, "betas": betas}
            s, i, t, _new = HotPathStep.apply(env, s, i, t, *[n.log_beta for n in nets], *profile)
        loss = i.sum()
        torch.cuda.synchronize()
        t_b = time.perf_counter()
        loss.backward()
        torch.cuda.synchronize()
        t_c = time.perf_counter()
        if profile:
            assert all(p.grad is not None for p in profile)
        return 1e3 * (t_b - t_a) / T, 1e3 * (t_c - t_b) / T

    out = {"preset": args.preset, "n_agents": A, "networks": len(networks), "steps": T, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "modes": {}}
    for mode in ("log_beta", "profile"):
        once(mode)                                            # warm-up
        runs = [once(mode) for _ in range(args.repeats)]
        out["modes"][mode] = {"forward_ms_per_step": float(np.median([x[0] for x in runs])),
                              "backward_ms_per_step": float(np.median([x[1] for x in runs])),
                              "runs": [{"forward_ms": x[0], "backward_ms": x[1]} for x in runs]}
        print(f"[timing] {mode}: {out['modes'][mode]['backward_ms_per_step']:.3f} ms backward per step",
              file=sys.stderr, flush=True)
    m = out["modes"]
    out["profile_minus_log_beta_backward_ms"] = m["profile"]["backward_ms_per_step"] - m["log_beta"]["backward_ms_per_step"]
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
