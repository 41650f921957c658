"""Cost of the transmission tree next to its sibling kernels and the step it follows, on one device.

    python tools/infection_tree_cost.py [--agents 10000000] [--launches 30] [--warmup 5] [--out FILE]

On the C3 world of bench.py (10 M agents, eight networks on six edge sets, household-major order) at the benchmark's
low- and high-prevalence states (1 % and 30 % infected): one production step is run from the state, then - in the same
process, every launch bracketed by device events - ``gj_infection_tree`` on that step's new infections, ``cum`` workspaces
and transmissions, the same launch without venue rows (the walk over the pairs alone: every infection stays unresolved;
the difference is the venue-row walk), and next to them ``gj_infector_scatter``, ``gj_location_stats`` and the hot-path
step itself.  Per case: median, min, max over the launches.  Also: the time ``DevicePlan.venue_rows`` takes to build the
by-venue rows, their bytes (4 B per edge + 4 B per venue), the longest venue row of every set and the longest row a drawn
pair met in each state.  Writes one JSON object (default profiles/infection_tree_c3_10m.json) and prints it."""
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

from infector_cost import timed  # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--agents", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--high-prevalence", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infection_tree_c3_10m.json"))
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    import bench as B
    from grad_june_amd import _native as N
    from grad_june_amd.benchrun import SingleGpuHotPath
    from grad_june_amd.groups import InfectionTree, InfectorStats, LocationStats
    from grad_june_amd.synthetic import epidemic_state, make_world, reorder_agents

    t0 = time.time()

    def progress(msg):
        print(f"[cost {time.time() - t0:6.1f}s] {msg}", file=sys.stderr, flush=True)

    dev = torch.device("cuda", 0)
    world = reorder_agents(make_world("c3", n_agents=args.agents, seed=args.seed, infected_fraction=0.01,
                                      progress=progress), by="household")
    n, networks = world["n_agents"], list(world["networks"])
    progress(f"world: {n} agents, networks {networks}")
    runner = SingleGpuHotPath(world, B.network_specs(world), B.betas_of(world), dev, seed=args.seed, layout="tiled",
                              device_compile=True, progress=progress)
    plan = runner.engine.plan
    edges = {s: (es["agent"], es["venue"]) for s, es in world["edge_sets"].items() if s in plan.host.set_index}
    plan.location_rows(edges)
    torch.cuda.synchronize()
    t_build = time.time()
    plan.venue_rows(edges)
    torch.cuda.synchronize()
    build_s = time.time() - t_build
    rows_bytes = int(sum(r.numel() * 4 + a.numel() * 4 for r, a in plan._venue_rows_keep))
    progress(f"venue rows: built in {build_s:.2f} s, {rows_bytes / 1e6:.1f} MB, longest rows {plan.venue_rows_max}")
    no_rows = (N.VenueRows * N.GJ_MAX_SETS)()
    lengths = {s.name: torch.diff(plan._venue_rows_keep[i][0]) for i, s in enumerate(plan.host.sets)}
    set_of_column = [plan.networks[name].edge_set for name in networks]

    low = {k: np.array(v, copy=True) for k, v in world["state"].items()}
    out = {"device": torch.cuda.get_device_name(0), "n_agents": n, "networks": networks, "launches": args.launches,
           "warmup": args.warmup, "tile_geometry": "size-based defaults (not tuned)", "venue_rows_build_s": build_s,
           "venue_rows_bytes": rows_bytes, "venue_rows_bytes_rule": "4 B per edge + 4 B per venue (+ 4 B per set)",
           "longest_venue_row_by_set": plan.venue_rows_max, "GJ_TREE_MAX_VENUE_ROW": N.GJ_TREE_MAX_VENUE_ROW,
           "venue_row_walk": "a group of 16 lanes per infection; a row of more than 256 members by the whole wave",
           "states": []}
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
                "infected_fraction_at_start": float(np.mean(state["is_infected"]))}
        tree = InfectionTree(n, networks + ["background"], device=dev)
        full = lambda: tree.record(plan, p, nu, s0, None, tr, active=networks, seed=args.seed, step=1)
        case["gj_infection_tree"] = timed(full, args.warmup, args.launches)
        tree.check()
        launches = args.warmup + args.launches
        case["unresolved"] = int(tree.unresolved[0].item()) // launches
        case["nobody_transmitted"] = int((tree.infector == -2).sum().item())
        case["infectors_drawn"] = int((tree.infector >= 0).sum().item())
        assert int(tree.counts[0].sum().item()) == launches * case["new_infections"], "counts do not sum to the new infections"
        offspring = tree.offspring()
        case["largest_offspring_count"] = int(offspring.max().item())
        # the longest venue row a drawn pair met, by the set of the location it came through
        met = {}
        for c, name in enumerate(networks):
            s = set_of_column[c]
            if s not in lengths:
                continue
            v = tree.venue[(tree.via == c) & (tree.venue >= 0)].long()
            if v.numel():
                met[s] = max(met.get(s, 0), int(lengths[s][v].max().item()))
        case["longest_venue_row_met_by_set"] = met
        # the same launch without venue rows: the pairs are walked and drawn, every infection stays unresolved
        pairs = InfectionTree(n, networks + ["background"], device=dev)
        real = plan._venue_rows
        try:
            plan._venue_rows = no_rows
            case["gj_infection_tree, no venue rows (pairs only)"] = timed(
                lambda: pairs.record(plan, p, nu, s0, None, tr, active=networks, seed=args.seed, step=1), args.warmup,
                args.launches)
        finally:
            plan._venue_rows = real
        one = InfectorStats(n, None, device=dev, clear="memset")
        case["gj_infector_scatter"] = timed(lambda: one.scatter(plan, p, nu, s0, None), args.warmup, args.launches,
                                            before=lambda: one.clear(plan))
        one.clear(plan)
        loc = LocationStats(None, 1, networks + ["background"], device=dev)
        case["gj_location_stats, national"] = timed(lambda: loc.add(plan, p, nu, s0, None, active=networks),
                                                    args.warmup, args.launches)
        case["hot_path_step"] = timed(runner.step, args.warmup, args.launches)
        med = lambda k: case[k]["median_us"]
        case["venue_row_walk_share_of_the_launch"] = 1.0 - med("gj_infection_tree, no venue rows (pairs only)") / med("gj_infection_tree")
        case["tree_over_gj_infector_scatter"] = med("gj_infection_tree") / med("gj_infector_scatter")
        case["tree_over_gj_location_stats"] = med("gj_infection_tree") / med("gj_location_stats, national")
        case["tree_over_hot_path_step"] = med("gj_infection_tree") / med("hot_path_step")
        progress(f"{what}: {case['new_infections']} new infections; tree {med('gj_infection_tree'):.1f} us (pairs only "
                 f"{med('gj_infection_tree, no venue rows (pairs only)'):.1f} us), scatter {med('gj_infector_scatter'):.1f} us, "
                 f"gj_location_stats {med('gj_location_stats, national'):.1f} us; step {med('hot_path_step'):.1f} us; "
                 f"longest row met {met}")
        out["states"].append(case)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
