"""Cost of a ContactQuarantine's two launches and of its series next to the step they precede, on one device.

    python tools/contact_quarantine_cost.py [--agents 10000000] [--launches 30] [--warmup 5] [--out FILE]

On the C3 world of bench.py (10 M agents, household-major order) with ``contacts: {household: 14}``, at the benchmark's
low-prevalence state (1 % infected) and at 30 % infected, each with the symptomatic share the state implies (an infected
agent's stage is uniform on 2 .. 5: half of them are at or above the threshold 4): in one process, every launch bracketed
by device events, ``gj_contact_mark``, ``gj_contact_mask`` (compliance 0.8, four agents per lane - the quad form of the
walk - and, on arrays one element off a 16-byte boundary, one agent per lane - the simple form; and compliance 0, where no
agent walks a row, which shows what the walk costs) and the ``gj_stage_stats`` call of the series (three bins, no labels), next to
``gj_step_stats`` on the same world and the hot-path step itself.  ``until`` is in its steady state when the launches are
timed (the first mark has run).  Per case: median, min, max over the launches, the ratio of the medians to
gj_step_stats' and to the step's, and the bandwidth the byte model implies - mark: 4 B per agent, plus 8 B of row
pointers and 4 B per edge of the index agents; mask: 4 B + 4 B per agent, plus, for a complying agent that is no index
case, 8 B of row pointers, 4 B per traced edge and one ``until`` gather per edge (counted as 4 B; it moves a cache line).
Writes one JSON object (default profiles/contact_quarantine_c3_10m.json) and prints it."""
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

THRESHOLD, DAYS, COMPLIANCE = 4.0, 14.0, 0.8


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
    ap.add_argument("--high-prevalence", type=float, default=0.30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contact_quarantine_c3_10m.json"))
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    import bench as B
    from grad_june_amd import _native as N
    from grad_june_amd.benchrun import SingleGpuHotPath
    from grad_june_amd.groups import StageStats
    from grad_june_amd.policies import QUARANTINE_STREAM
    from grad_june_amd.synthetic import epidemic_state, make_world, reorder_agents

    t0 = time.time()

    def progress(msg):
        print(f"[cost {time.time() - t0:6.1f}s] {msg}", file=sys.stderr, flush=True)

    dev = torch.device("cuda", 0)
    lib = N.load()
    world = reorder_agents(make_world("c3", n_agents=args.agents, seed=args.seed, infected_fraction=0.01,
                                      progress=progress), by="household")
    n = world["n_agents"]
    runner = SingleGpuHotPath(world, B.network_specs(world), B.betas_of(world), dev, seed=args.seed, layout="tiled",
                              device_compile=True, progress=progress)
    plan, st = runner.engine.plan, runner.state
    es = world["edge_sets"]["household"]
    (rowptr, venue, n_venues), = plan.contact_rows(["household"], {"household": (es["agent"], es["venue"])})
    degree = (rowptr[1:] - rowptr[:-1]).long()
    progress(f"world: {n} agents, {n_venues} households, {venue.numel()} household edges")
    until = torch.zeros(max(1, n_venues), dtype=torch.int32, device=dev)
    sets = (N.ContactSet * 1)()
    sets[0].a_rowptr, sets[0].a_venue, sets[0].until, sets[0].n_venues = rowptr.data_ptr(), venue.data_ptr(), until.data_ptr(), n_venues
    qstate = torch.empty(n, dtype=torch.float32, device=dev)
    # the same arrays one element off a 16-byte boundary: the library then takes one agent per lane, the simple walk
    stage_off, qstate_off = (torch.empty(n + 4, dtype=torch.float32, device=dev)[1: n + 1] for _ in range(2))
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, 1, 3, dtype=torch.int64, device=dev)
    stats = StageStats(None, 1, 3, device=dev)
    cls = plan.agent_class[:n]
    age_edges = (C.c_int32 * 4)(0, 18, 65, 100)
    national = torch.zeros(5, dtype=torch.float64, device=dev)
    stream = QUARANTINE_STREAM | 0

    out = {"device": torch.cuda.get_device_name(0), "n_agents": n, "n_households": n_venues,
           "household_edges": int(venue.numel()), "launches": args.launches, "warmup": args.warmup,
           "contacts": {"household": DAYS}, "stage_threshold": THRESHOLD, "compliance": COMPLIANCE,
           "tile_geometry": "size-based defaults (not tuned)",
           "byte_model": "mark: 4 B per agent + (8 B + 4 B per edge) per index agent; mask: 8 B per agent + (8 B + 8 B per "
                         "edge) per complying agent that is no index case (the until gather counted as 4 B per edge)",
           "cases": []}

    def step_stats():
        N.check(lib.gj_step_stats(n, N.ptr(cls), N.ptr(st["is_infected"]), N.ptr(st["current_stage"]), 3, age_edges, 7,
                                  N.ptr(national), N.current_stream()), "gj_step_stats")

    for what, state in (("1 % infected", None), (f"{args.high_prevalence:.0%} infected",
                                                 epidemic_state(n, args.high_prevalence, args.seed + 1))):
        if state is not None:
            runner.load_state(state)
        stage = st["current_stage"]
        now = 1.0
        sets[0].release = now + DAYS
        until.zero_()

        def mark():
            N.check(lib.gj_contact_mark(n, N.ptr(stage), THRESHOLD, sets, 1, N.ptr(err), N.current_stream()),
                    "gj_contact_mark")

        def mask(compliance=COMPLIANCE, stage=stage, qstate=qstate):
            N.check(lib.gj_contact_mask(n, N.ptr(stage), THRESHOLD, sets, 1, now, compliance, args.seed, stream, 0,
                                        N.ptr(qstate), N.ptr(err), N.current_stream()), "gj_contact_mask")

        stage_off.copy_(stage)

        mark()
        mask()
        index = ~(stage < THRESHOLD)
        walkers = int((n - int(index.sum().item())) * COMPLIANCE)      # (expected: the draw is uniform)
        index_edges = int(degree[index].sum().item())
        walker_edges = int(degree[~index].sum().item() * COMPLIANCE)
        case = {"case": what, "infected_fraction": float(st["is_infected"].clamp(max=1).mean()),
                "index_agents": int(index.sum().item()), "contacts": int((qstate == 2.0).sum().item()),
                "marked_households": int((until != 0).sum().item())}
        base = timed(step_stats, args.warmup, args.launches)
        step = timed(runner.step, args.warmup, args.launches)
        case["gj_step_stats"], case["hot_path_step"] = base, step
        n_index = case["index_agents"]
        for key, fn, bytes_moved in (
                ("gj_contact_mark", mark, 4 * n + 8 * n_index + 4 * index_edges),
                ("gj_contact_mask", mask, 8 * n + 8 * walkers + 8 * walker_edges),
                ("gj_contact_mask, one agent per lane", lambda: mask(COMPLIANCE, stage_off, qstate_off),
                 8 * n + 8 * walkers + 8 * walker_edges),
                ("gj_contact_mask, compliance 0", lambda: mask(0.0), 8 * n),
                ("gj_stage_stats on qstate", lambda: stats.add(qstate, None, counts), 4 * n)):
            if key.startswith("gj_stage_stats"):
                mask()                                                # (the counted mask is the policy's, not compliance 0's)
            t = timed(fn, args.warmup, args.launches)
            case[key] = dict(t, ratio_to_gj_step_stats=t["median_us"] / base["median_us"],
                             ratio_to_hot_path_step=t["median_us"] / step["median_us"], model_bytes=bytes_moved,
                             model_GBps=bytes_moved / t["median_us"] * 1e-3)
        case["gj_step_stats_again"] = timed(step_stats, 2, args.launches)
        assert int(err.item()) == 0, "a row outside the household set"
        assert torch.equal(qstate, qstate_off), "the two forms of the mask disagree"
        stats.check("gj_stage_stats on qstate")
        progress(f"{what}: {n_index} index agents, {case['contacts']} contacts; mark "
                 f"{case['gj_contact_mark']['median_us']:.1f} us, mask {case['gj_contact_mask']['median_us']:.1f} us "
                 f"(compliance 0: {case['gj_contact_mask, compliance 0']['median_us']:.1f} us), stage stats "
                 f"{case['gj_stage_stats on qstate']['median_us']:.1f} us; gj_step_stats {base['median_us']:.1f} us; step "
                 f"{step['median_us']:.1f} us")
        out["cases"].append(case)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
