"""Cost of the infector attribution next to the step it follows, on one device.

    python tools/infector_cost.py [--agents 10000000] [--launches 30] [--warmup 5] [--out FILE]

On the C3 world of bench.py (10 M agents, eight networks on six edge sets, household-major order) at the benchmark's
low- and high-prevalence states (1 % and 30 % infected): one production step is run from the state, then - in the same
process, every launch bracketed by device events - ``gj_infector_scatter`` on that step's new infections and ``cum``
workspaces, ``gj_infector_gather`` on its transmissions (with ``caused``, the national call; and by super areas of 8000
agents without), the two ways of clearing ``U`` (a memset of all of it; ``gj_infector_clear``'s walk over the step's new
infections), and next to them ``gj_location_stats``, ``gj_step_stats`` and the hot-path step itself.  Per case: median,
min, max over the launches, and the ratios of scatter + gather + the cheaper clear to gj_location_stats and to the step.
Writes one JSON object (default profiles/infector_c3_10m.json) and prints it."""
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


def timed(fn, warmup, launches, before=None):
    """Median / min / max of ``fn`` in microseconds; ``before`` runs ahead of every launch, outside the bracket."""
    for _ in range(warmup):
        if before is not None:
            before()
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in pairs:
        if before is not None:
            before()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infector_c3_10m.json"))
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    import bench as B
    from grad_june_amd import _native as N
    from grad_june_amd.benchrun import SingleGpuHotPath
    from grad_june_amd.groups import InfectorStats, LocationStats
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
    edges = {s: (es["agent"], es["venue"]) for s, es in world["edge_sets"].items() if s in plan.host.set_index}
    plan.location_rows(edges)
    units = plan.infector_units()[0]
    units_bytes = int(sum(u.numel() * 8 for u in units))
    progress(f"U: {units_bytes / 1e6:.1f} MB over {len(units)} sets")

    G8 = -(-n // 8000)
    labels = (torch.arange(n, device=dev) // 8000).to(torch.int32)
    cls = plan.agent_class[:n]
    age_edges = (C.c_int32 * 4)(0, 18, 65, 100)
    national = torch.zeros(5, dtype=torch.float64, device=dev)
    low = {k: np.array(v, copy=True) for k, v in world["state"].items()}
    out = {"device": torch.cuda.get_device_name(0), "n_agents": n, "networks": networks, "launches": args.launches,
           "warmup": args.warmup, "tile_geometry": "size-based defaults (not tuned)", "units_bytes": units_bytes,
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
        one = InfectorStats(n, None, device=dev, clear="memset")
        by8 = InfectorStats(n, {"super_area": (labels, G8)}, device=dev, clear="walk")
        memset = lambda: one.clear(plan)
        walk = lambda: by8.clear(plan, nu)
        # scatter: U is zero before every launch (cleared outside the bracket)
        case["gj_infector_scatter"] = timed(lambda: one.scatter(plan, p, nu, s0, None), args.warmup, args.launches,
                                            before=memset)
        one.check()
        case["unattributed"] = int(one.unattributed[0].item()) // (args.warmup + args.launches)
        total = int(sum(int(u.sum().item()) for u in units))
        assert total == N.GJ_LOC_UNIT * (case["new_infections"] - case["unattributed"]), "U does not sum to the attributed infections"
        # gather: U holds the step's units
        case["gj_infector_gather, national with caused"] = timed(lambda: one.gather(plan, p, tr, None), args.warmup, args.launches)
        credited = float(one.caused.sum().item()) / (args.warmup + args.launches)
        case["credits_sum"] = credited
        case["conservation_residual"] = abs(credited - (case["new_infections"] - case["unattributed"]))
        only8 = lambda: N.check(lib.gj_infector_gather(
            C.byref(plan.c), C.byref(p), plan.location_rows(), N.ptr(tr), None, plan.infector_units()[1],
            N.ptr(by8.labels["super_area"]), G8, None, N.ptr(by8.out["super_area"][0]), N.ptr(by8.err),
            N.current_stream()), "gj_infector_gather")
        case["gj_infector_gather, super areas of 8000"] = dict(timed(only8, args.warmup, args.launches), n_groups=G8,
                                                               regime="lds" if G8 <= N.GJ_LOC_LDS_BINS else "global")
        by8.check()
        # the two clears, same run: each on a U that holds the step's units (scattered again outside the bracket)
        refill = lambda: one.scatter(plan, p, nu, s0, None)
        case["clear, memset of U"] = timed(memset, args.warmup, args.launches, before=refill)
        case["clear, gj_infector_clear (walk)"] = timed(walk, args.warmup, args.launches, before=refill)
        assert not any(bool(u.any()) for u in units), "the walk left units behind"
        loc = LocationStats(None, 1, networks + ["background"], device=dev)
        case["gj_location_stats, national"] = timed(lambda: loc.add(plan, p, nu, s0, None, active=networks),
                                                    args.warmup, args.launches)
        case["gj_step_stats"] = timed(lambda: N.check(lib.gj_step_stats(
            n, N.ptr(cls), N.ptr(st["is_infected"]), N.ptr(st["current_stage"]), 3, age_edges, 7, N.ptr(national),
            N.current_stream()), "gj_step_stats"), args.warmup, args.launches)
        case["hot_path_step"] = timed(runner.step, args.warmup, args.launches)
        med = lambda k: case[k]["median_us"]
        clear = min(med("clear, memset of U"), med("clear, gj_infector_clear (walk)"))
        added = med("gj_infector_scatter") + med("gj_infector_gather, national with caused") + clear
        case["added_per_step_us (scatter + national gather + cheaper clear)"] = added
        case["added_over_gj_location_stats"] = added / med("gj_location_stats, national")
        case["added_over_hot_path_step"] = added / med("hot_path_step")
        progress(f"{what}: {case['new_infections']} new infections, {case['infectious_agents']} infectious; scatter "
                 f"{med('gj_infector_scatter'):.1f} us, gather {med('gj_infector_gather, national with caused'):.1f} us, "
                 f"memset {med('clear, memset of U'):.1f} us, walk {med('clear, gj_infector_clear (walk)'):.1f} us; "
                 f"gj_location_stats {med('gj_location_stats, national'):.1f} us; step {med('hot_path_step'):.1f} us")
        out["states"].append(case)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
