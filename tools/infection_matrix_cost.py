"""Cost of the who-infects-whom matrix next to the infector series it extends, on one device.

    python tools/infection_matrix_cost.py [--agents 10000000] [--groups 4 16] [--launches 30] [--warmup 5] [--out FILE]

On the C3 world of bench.py (10 M agents, eight networks on six edge sets, household-major order) at the benchmark's
low- and high-prevalence states (1 % and 30 % infected), as tools/infector_cost.py does it: one production step is run
from the state, then - in the same process, every launch bracketed by device events - ``gj_infector_scatter`` and
``gj_infector_gather`` (the national call with ``caused``, and the call by the labelling without), and for G equal-width
age bands (G = 4 and 16) ``gj_infection_matrix_scatter``, ``gj_infection_matrix_gather`` and the two ways of clearing
``UG``: a memset of all of it, and ``gj_infection_matrix_clear``'s walk over the step's new infections.  Per case:
median, min, max over the launches; what a matrix adds to a step with the cheaper clear; the bytes of ``U`` and ``UG``.
Writes one JSON object (default profiles/infection_matrix_c3_10m.json) and prints it."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gradabm-june_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--agents", type=int, default=10_000_000)
    ap.add_argument("--groups", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--high-prevalence", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infection_matrix_c3_10m.json"))
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    import bench as B
    from grad_june_amd import _native as N
    from grad_june_amd.benchrun import SingleGpuHotPath
    from grad_june_amd.groups import InfectorStats
    from grad_june_amd.synthetic import epidemic_state, make_world, reorder_agents
    from infector_cost import timed

    t0 = time.time()

    def progress(msg):
        print(f"[cost {time.time() - t0:6.1f}s] {msg}", file=sys.stderr, flush=True)

    dev = torch.device("cuda", 0)
    lib = N.load()
    world = reorder_agents(make_world("c3", n_agents=args.agents, seed=args.seed, infected_fraction=0.01,
                                      progress=progress), by="household")
    n, networks = world["n_agents"], list(world["networks"])
    progress(f"world: {n} agents, networks {networks}")
    runner = SingleGpuHotPath(world, B.network_specs(world), B.betas_of(world), dev, seed=args.seed, layout="tiled",
                              device_compile=True, progress=progress)
    plan = runner.engine.plan
    edges = {s: (es["agent"], es["venue"]) for s, es in world["edge_sets"].items() if s in plan.host.set_index}
    plan.location_rows(edges)
    units = plan.infector_units()[0]
    units_bytes = int(sum(u.numel() * 8 for u in units))
    age = plan.agent_class[:n].to(torch.int32) % 100
    labellings = {f"age_{G}": ((age * G // 100).to(torch.int32).contiguous(), G) for G in args.groups}
    low = {k: np.array(v, copy=True) for k, v in world["state"].items()}
    out = {"device": torch.cuda.get_device_name(0), "n_agents": n, "networks": networks, "launches": args.launches,
           "warmup": args.warmup, "tile_geometry": "size-based defaults (not tuned)", "units_bytes": units_bytes,
           "units_by_group_bytes": {}, "states": []}
    for what, state in (("low prevalence (1 % infected)", low),
                        (f"high prevalence ({100 * args.high_prevalence:g} % infected)",
                         epidemic_state(n, args.high_prevalence, args.seed + 1))):
        runner.load_state(state)
        st = runner.state
        s0 = st["susceptibility"].clone()
        p = runner.params()
        runner.step()                                  # eager: the plan's cum workspaces hold THIS step's sums
        nu = runner.new_infected.clone()
        tr = st["transmission"].clone()
        torch.cuda.synchronize()
        case = {"state": what, "new_infections": int(nu.sum().item()), "infectious_agents": int((tr[:n] > 0).sum().item()),
                "infected_fraction_at_start": float(np.mean(state["is_infected"])), "groups": {}}
        one = InfectorStats(n, None, device=dev, clear="memset")
        case["gj_infector_scatter"] = timed(lambda: one.scatter(plan, p, nu, s0, None), args.warmup, args.launches,
                                            before=lambda: one.clear(plan))
        case["gj_infector_gather, national with caused"] = timed(lambda: one.gather(plan, p, tr, None), args.warmup,
                                                                 args.launches)
        one.check()
        one.clear(plan)
        one.scatter(plan, p, nu, s0, None)             # U holds the step's units from here on
        total = int(sum(int(u.sum().item()) for u in units))
        med = lambda d: d["median_us"]
        for name, (labels, G) in labellings.items():
            by = {w: InfectorStats(n, {name: (labels, G)}, device=dev, matrices=[name], matrix_clear=w)
                  for w in ("memset", "walk")}
            UG = plan.infection_matrix_units(name, G)[0]
            out["units_by_group_bytes"][str(G)] = int(sum(u.numel() * 8 for u in UG))
            m = by["memset"]
            g = {"n_groups": G}
            g["gj_infection_matrix_scatter"] = timed(lambda: m.matrix_scatter(plan, p, nu, s0, None), args.warmup,
                                                     args.launches, before=lambda: m.matrix_clear(plan))
            assert int(sum(int(u.sum().item()) for u in UG)) == total, "UG does not sum to U"
            assert all(torch.equal(ug.sum(-1), u) for ug, u in zip(UG, units)), "UG does not sum to U in every cell"
            g["gj_infection_matrix_gather"] = timed(lambda: m.matrix_gather(plan, p, tr, None), args.warmup, args.launches)
            only = lambda: N.check(lib.gj_infector_gather(      # the labelling's own gather, without caused
                C.byref(plan.c), C.byref(p), plan.location_rows(), N.ptr(tr), None, plan.infector_units()[1],
                N.ptr(m.labels[name]), G, None, N.ptr(m.out[name][0]), N.ptr(m.err), N.current_stream()),
                "gj_infector_gather")
            g["gj_infector_gather, by the labelling"] = timed(only, args.warmup, args.launches)
            m.check()
            g["matrix_sum_over_gj_infector_gather_sum"] = float(m.matrix[name][0].sum().item()) / max(
                1.0, float(m.out[name][0].sum().item()))
            refill = lambda: m.matrix_scatter(plan, p, nu, s0, None)
            g["clear, memset of UG"] = timed(lambda: by["memset"].matrix_clear(plan, nu), args.warmup, args.launches,
                                             before=refill)
            g["clear, gj_infection_matrix_clear (walk)"] = timed(lambda: by["walk"].matrix_clear(plan, nu), args.warmup,
                                                                 args.launches, before=refill)
            assert not any(bool(u.any()) for u in UG), "the walk left units behind"
            clear = min(med(g["clear, memset of UG"]), med(g["clear, gj_infection_matrix_clear (walk)"]))
            added = med(g["gj_infection_matrix_scatter"]) + med(g["gj_infection_matrix_gather"]) + clear
            g["added_per_step_us (matrix scatter + matrix gather + cheaper clear)"] = added
            g["added_over_infector_scatter_plus_gather"] = added / (
                med(case["gj_infector_scatter"]) + med(case["gj_infector_gather, national with caused"]))
            progress(f"{what}, G = {G}: scatter {med(g['gj_infection_matrix_scatter']):.1f} us (gj_infector_scatter "
                     f"{med(case['gj_infector_scatter']):.1f}), gather {med(g['gj_infection_matrix_gather']):.1f} us "
                     f"(gj_infector_gather {med(g['gj_infector_gather, by the labelling']):.1f}), memset "
                     f"{med(g['clear, memset of UG']):.1f} us, walk {med(g['clear, gj_infection_matrix_clear (walk)']):.1f} us")
            case["groups"][str(G)] = g
            del by, UG, m
            plan._infection_matrix_units.pop(name)      # one labelling's UG at a time
        one.clear(plan)
        out["states"].append(case)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
