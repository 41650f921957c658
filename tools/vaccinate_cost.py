"""Cost of a vaccination launch and of its adjoint next to the step they precede, on one device.

    python tools/vaccinate_cost.py [--agents 10000000] [--launches 30] [--warmup 5] [--out FILE]

On the C3 world of bench.py (10 M agents, household-major order) at the benchmark's low-prevalence state: in one process,
every launch bracketed by device events, ``gj_vaccinate`` (with ``newly_out`` and ``count_out``, as the Runner calls it
when it records the series by group; without ``newly_out``; and without ``count_out`` either, which shows what the
count's atomics cost) and ``gj_adjoint_vaccinate`` (the per-agent launch plus the two fp64 summing launches, two efficacy
bands) for a slice of the rollout that moves about 1 % of the agents and for one that moves none, next to
``gj_step_stats`` on the same world and the hot-path step itself.  Per case: median, min,
max over the launches, the ratio of the medians to gj_step_stats' and to the step's, and the bandwidth the byte model -
1 B + 4 B read per agent, 4 B written per newly vaccinated agent (the kernel stores the float4 that holds one); with
``newly_out`` 4 B more written per agent - implies.  Writes one JSON object (default profiles/vaccinate_c3_10m.json)
and prints it."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vaccinate_c3_10m.json"))
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    import bench as B
    from grad_june_amd import _native as N
    from grad_june_amd.benchrun import SingleGpuHotPath
    from grad_june_amd.policies import VACCINE_STREAM, Vaccination
    from grad_june_amd.synthetic import make_world, reorder_agents

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
    cls = plan.agent_class[:n]
    policy = Vaccination("2021-01-01", "2021-04-11", coverage=1.0, efficacy={"0-50": 0.5, "50-100": 0.25})
    band, band_plan = policy.bands((cls.long() % 100))
    progress(f"world: {n} agents; bands' plan: {band_plan.n_chunks} chunks")
    susc = st["susceptibility"].clone()
    newly = torch.empty(n, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    g_out = torch.ones(n, dtype=torch.float32, device=dev)
    g_in = torch.empty(n, dtype=torch.float32, device=dev)
    contrib = torch.empty(n, dtype=torch.float64, device=dev)
    partial = torch.empty(max(1, band_plan.n_chunks), dtype=torch.float64, device=dev)
    grad = torch.empty(band_plan.n_groups, dtype=torch.float64, device=dev)
    age_edges = (C.c_int32 * 4)(0, 18, 65, 100)
    national = torch.zeros(5, dtype=torch.float64, device=dev)
    stream = VACCINE_STREAM | 0

    out = {"device": torch.cuda.get_device_name(0), "n_agents": n, "launches": args.launches, "warmup": args.warmup,
           "tile_geometry": "size-based defaults (not tuned)",
           "byte_model": "1 B + 4 B read per agent, 4 B written per newly vaccinated agent; newly_out: + 4 B written per "
                         "agent; adjoint: 1 + 4 + 4 + 4 B read, 8 + 4 B written per agent, then the plan's gathers"}
    out["gj_step_stats"] = timed(lambda: N.check(lib.gj_step_stats(
        n, N.ptr(cls), N.ptr(st["is_infected"]), N.ptr(st["current_stage"]), 3, age_edges, 7, N.ptr(national),
        N.current_stream()), "gj_step_stats"), args.warmup, args.launches)
    out["hot_path_step"] = timed(runner.step, args.warmup, args.launches)
    base, step = out["gj_step_stats"]["median_us"], out["hot_path_step"]["median_us"]
    out["cases"] = []
    for what, lo, hi in (("a step that moves about 1 % of the agents", 0.10, 0.11), ("a step that moves none", 0.11, 0.11)):
        tables = policy.tables(lo, hi)

        def forward(with_newly, with_count=True):
            N.check(lib.gj_vaccinate(n, N.ptr(cls), tables, args.seed, stream, 0, N.ptr(susc),
                                     N.ptr(newly) if with_newly else None, N.ptr(count) if with_count else None,
                                     N.current_stream()), "gj_vaccinate")

        def adjoint():
            N.check(lib.gj_adjoint_vaccinate(n, N.ptr(cls), tables, args.seed, stream, 0, N.ptr(susc), N.ptr(g_out),
                                             N.ptr(band), band_plan.n_groups, C.byref(band_plan.c), N.ptr(contrib),
                                             N.ptr(partial), N.ptr(grad), N.ptr(g_in), N.current_stream()),
                    "gj_adjoint_vaccinate")

        count.zero_()
        forward(True)
        moved = int(count.item())
        assert moved == int(newly.sum().item()), "count_out and newly_out disagree"
        case = {"case": what, "ramp": [lo, hi], "newly_vaccinated": moved, "fraction": moved / n}
        for key, fn, bytes_moved in (
                ("gj_vaccinate", lambda: forward(False), 5 * n + 4 * moved),
                ("gj_vaccinate, newly_out", lambda: forward(True), 9 * n + 4 * moved),
                ("gj_vaccinate, no count_out", lambda: forward(False, False), 5 * n + 4 * moved),
                ("gj_adjoint_vaccinate", adjoint, 25 * n)):
            t = timed(fn, args.warmup, args.launches)
            case[key] = dict(t, ratio_to_gj_step_stats=t["median_us"] / base, ratio_to_hot_path_step=t["median_us"] / step,
                             model_bytes=bytes_moved, model_GBps=bytes_moved / t["median_us"] * 1e-3)
        case["gj_step_stats_again"] = timed(lambda: N.check(lib.gj_step_stats(
            n, N.ptr(cls), N.ptr(st["is_infected"]), N.ptr(st["current_stage"]), 3, age_edges, 7, N.ptr(national),
            N.current_stream()), "gj_step_stats"), 2, args.launches)
        progress(f"{what}: {moved} moved; gj_vaccinate {case['gj_vaccinate']['median_us']:.1f} us, with newly_out "
                 f"{case['gj_vaccinate, newly_out']['median_us']:.1f} us, adjoint "
                 f"{case['gj_adjoint_vaccinate']['median_us']:.1f} us; gj_step_stats {base:.1f} us; step {step:.1f} us")
        out["cases"].append(case)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
