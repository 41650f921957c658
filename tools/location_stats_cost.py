"""Cost of the infection-location attribution next to the step it follows, on one device.

    python tools/location_stats_cost.py [--agents 10000000] [--launches 30] [--warmup 5] [--out FILE]

On the C3 world of bench.py (10 M agents, eight networks on six edge sets, household-major order) at the benchmark's
low- and high-prevalence states (1 % and 30 % infected): one production step is run from the state, then - in the same
process, every launch bracketed by device events - ``gj_location_stats`` on that step's new infections and ``cum``
workspaces (the national call, and by super areas of 8000 agents), the clone of the pre-step susceptibility the model
takes for it, ``gj_step_stats`` on the same arrays, and the hot-path step itself.  Per case: median, min, max over the
launches and the ratio of the medians to gj_step_stats' and to the step's.  Also the one-time set-up of the by-agent
rows.  Writes one JSON object (default profiles/location_stats_c3_10m.json) and prints it."""
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


def timed(fn, warmup, launches):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = np.array([1e3 * a.elapsed_time(b) for a, b in pairs])
    return {"median_us": float(np.median(us)), "min_us": float(us.min()), "max_us": float(us.max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--agents", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--high-prevalence", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "location_stats_c3_10m.json"))
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    import bench as B
    from grad_june_amd import _native as N
    from grad_june_amd.benchrun import SingleGpuHotPath
    from grad_june_amd.groups import LocationStats
    from grad_june_amd.synthetic import epidemic_state, make_world, reorder_agents

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
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    edges = {s: (es["agent"], es["venue"]) for s, es in world["edge_sets"].items() if s in plan.host.set_index}
    plan.location_rows(edges)
    torch.cuda.synchronize()
    rows_s = time.perf_counter() - t1
    set_edges = int(sum(len(e[0]) for e in edges.values()))
    progress(f"by-agent rows: {set_edges} edges in {rows_s:.2f} s")

    columns = networks + ["background"]
    G8 = -(-n // 8000)
    labels = (torch.arange(n, device=dev) // 8000).to(torch.int32)
    cls = plan.agent_class[:n]
    age_edges = (C.c_int32 * 4)(0, 18, 65, 100)
    national = torch.zeros(5, dtype=torch.float64, device=dev)
    low = {k: np.array(v, copy=True) for k, v in world["state"].items()}
    out = {"device": torch.cuda.get_device_name(0), "n_agents": n, "networks": networks, "set_edges": set_edges,
           "launches": args.launches, "warmup": args.warmup, "tile_geometry": "size-based defaults (not tuned)",
           "rows_setup_s": rows_s, "rows_bytes": 4 * set_edges + 4 * (n + 1) * len(edges), "states": []}
    for what, state in (("low prevalence (1 % infected)", low),
                        (f"high prevalence ({100 * args.high_prevalence:g} % infected)",
                         epidemic_state(n, args.high_prevalence, args.seed + 1))):
        runner.load_state(state)
        st = runner.state
        s0 = st["susceptibility"].clone()
        p = runner.params()
        runner.step()                                  # eager: the plan's cum workspaces hold THIS step's sums
        nu = runner.new_infected.clone()
        torch.cuda.synchronize()
        case = {"state": what, "new_infections": int(nu.sum().item()),
                "infected_fraction_at_start": float(np.mean(state["is_infected"]))}
        for name, lab, G in (("national", None, 1), ("super areas of 8000, world order", labels, G8)):
            stats = LocationStats(lab, G, columns, device=dev)
            case[f"gj_location_stats, {name}"] = dict(
                timed(lambda: stats.add(plan, p, nu, s0, None, active=networks), args.warmup, args.launches),
                n_groups=G, regime="lds" if G * len(columns) <= N.GJ_LOC_LDS_BINS else "global")
            stats.check()
            total = args.warmup + args.launches
            units = stats.out[0].sum(0).cpu().numpy()
            assert int(units.sum()) == total * N.GJ_LOC_UNIT * case["new_infections"], "a row does not sum to the new infections"
            if lab is None:
                case["shares"] = {c: float(u) / total / N.GJ_LOC_UNIT for c, u in zip(columns, units)}
        case["susceptibility_clone"] = timed(lambda: st["susceptibility"].clone(), args.warmup, args.launches)
        case["gj_step_stats"] = timed(lambda: N.check(lib.gj_step_stats(
            n, N.ptr(cls), N.ptr(st["is_infected"]), N.ptr(st["current_stage"]), 3, age_edges, 7, N.ptr(national),
            N.current_stream()), "gj_step_stats"), args.warmup, args.launches)
        case["hot_path_step"] = timed(runner.step, args.warmup, args.launches)
        case["infected_fraction_at_end"] = float(st["is_infected"].clamp(max=1).mean())
        added = case["gj_location_stats, national"]["median_us"] + case["susceptibility_clone"]["median_us"]
        case["added_per_step_us (national launch + clone)"] = added
        case["added_over_gj_step_stats"] = added / case["gj_step_stats"]["median_us"]
        case["added_over_hot_path_step"] = added / case["hot_path_step"]["median_us"]
        progress(f"{what}: {case['new_infections']} new infections; launch "
                 f"{case['gj_location_stats, national']['median_us']:.1f} us + clone "
                 f"{case['susceptibility_clone']['median_us']:.1f} us; gj_step_stats "
                 f"{case['gj_step_stats']['median_us']:.1f} us; step {case['hot_path_step']['median_us']:.1f} us")
        out["states"].append(case)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
