"""Cost of the waning-immunity launch and of its adjoint next to the step they follow, on one device.

    python tools/immunity_cost.py [--agents 10000000] [--launches 30] [--warmup 5] [--earlier-steps 20] [--out FILE]

On the C3 world of bench.py (10 M agents, household-major order), seeded at 1 % and at 30 % infected and then run for
``--earlier-steps`` days of hot path + ``gj_immunity_step`` + symptoms update, so that agents have recovered, wane and
are infected again.  Then one more hot-path step, and on the state it leaves - restored before every launch, outside the
timed bracket - in one process, every launch bracketed by device events: ``gj_immunity_step`` without the optional
outputs, with ``flags_out`` (what the autograd node keeps) and with all four (what the Runner asks for when it records the
series by group), ``gj_adjoint_immunity`` (the per-agent launch plus two pairs of fp64 summing launches, two bands), and
in the same run ``gj_vaccinate``, ``gj_step_stats`` and the hot-path step.  Per case: median, min, max over the launches,
the ratios of the medians, and the bandwidth the byte model implies - the launch reads 4 B stage + 4 B new_infected + 1 B
class per agent; it reads and writes 4 B + 4 B of susceptibility where a lane holds a waning agent (counted per waning
agent; the kernel moves the float4 that holds one); it reads 4 B of is_infected per newly infected agent and writes 4 B
per reinfected one; flags_out: + 1 B, reinfected_out: + 4 B written per agent; susc_sum_out: the susceptibility of every
agent is read (4 B per agent in the place of the waning agents' reads).  Writes one JSON object (default
profiles/immunity_c3_10m.json) and prints it."""
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


def timed(fn, warmup, launches, prepare=None):
    """Device-event times of ``fn``; ``prepare`` runs before every launch, outside the bracket."""
    for _ in range(warmup):
        if prepare is not None:
            prepare()
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in pairs:
        if prepare is not None:
            prepare()
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
    ap.add_argument("--earlier-steps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "immunity_c3_10m.json"))
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    import bench as B
    from grad_june_amd import _native as N
    from grad_june_amd.benchrun import SingleGpuHotPath
    from grad_june_amd.immunity import Immunity
    from grad_june_amd.policies import VACCINE_STREAM, Vaccination
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
    cls = plan.agent_class[:n]
    immunity = Immunity({"0-50": 10.0, "50-100": 20.0}, 0.2)
    tables = immunity.tables(1.0)
    band, band_plan = immunity.bands((cls.long() % 100))
    policy = Vaccination("2021-01-01", "2021-04-11", coverage=1.0, efficacy={"0-50": 0.5, "50-100": 0.25})
    vaccine_tables = policy.tables(0.10, 0.11)
    progress(f"world: {n} agents; bands' plan: {band_plan.n_chunks} chunks")

    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    reinf = torch.empty(n, dtype=torch.float32, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    ones = torch.ones(n, dtype=torch.float32, device=dev)
    g_outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)]
    contrib = torch.empty(2 * n, dtype=torch.float64, device=dev)
    partial = torch.empty(max(1, 2 * band_plan.n_chunks), dtype=torch.float64, device=dev)
    sums = torch.empty(2, band_plan.n_groups, dtype=torch.float64, device=dev)
    age_edges = (C.c_int32 * 4)(0, 18, 65, 100)
    national = torch.zeros(5, dtype=torch.float64, device=dev)

    def immunity_step(susc, inf, with_flags=False, with_all=False):
        N.check(lib.gj_immunity_step(n, N.ptr(cls), tables, N.ptr(st["current_stage"]), 0, N.ptr(runner.new_infected),
                                     N.ptr(susc), N.ptr(inf), N.ptr(flags) if with_flags or with_all else None,
                                     N.ptr(reinf) if with_all else None, N.ptr(counts[0:1]) if with_all else None,
                                     N.ptr(counts[1:2]) if with_all else None, N.current_stream()), "gj_immunity_step")

    out = {"device": torch.cuda.get_device_name(0), "n_agents": n, "launches": args.launches, "warmup": args.warmup,
           "earlier_steps": args.earlier_steps, "tile_geometry": "size-based defaults (not tuned)",
           "immunity": {"half_life": {"0-50": 10.0, "50-100": 20.0}, "residual_protection": 0.2},
           "byte_model": "9 B read per agent, 8 B per waning agent, 4 B per newly infected and 4 B per reinfected agent; "
                         "flags_out: + 1 B, reinfected_out: + 4 B written per agent; susc_sum_out: 4 B read per agent in the "
                         "place of the waning agents' reads; adjoint: 1 + 1 + 4 + 4 + 4 + 4 B read, 16 + 4 + 4 B written per "
                         "agent, then the plan's gathers twice",
           "cases": []}
    for fraction in (0.01, 0.30):
        runner.load_state(epidemic_state(n, fraction, args.seed))
        runner.enable_full_step()
        p = runner._sym_p
        for _ in range(args.earlier_steps):      # a day: hot path, immunity, symptoms
            runner.step()
            immunity_step(st["susceptibility"], st["is_infected"])
            p.time, p.seed, p.step, p.agent_offset = float(runner.t), runner.seed, runner.t, 0
            N.check(lib.gj_symptoms_update(n, N.ptr(cls), N.ptr(runner.new_infected), N.ptr(st["current_stage"]),
                                           N.ptr(st["next_stage"]), N.ptr(st["time_to_next_stage"]), C.byref(p), None,
                                           None, N.current_stream()), "gj_symptoms_update")
        runner.step()                            # the step the launch follows: its new_infected and updated state
        susc0, inf0 = st["susceptibility"].clone(), st["is_infected"].clone()
        susc, inf = susc0.clone(), inf0.clone()

        def restore():
            susc.copy_(susc0)
            inf.copy_(inf0)

        counts.zero_()
        restore()
        immunity_step(susc, inf, with_all=True)
        reinfected = int(counts[0].item())
        waning = int((flags & 1).sum().item())
        new = int((runner.new_infected != 0).sum().item())
        recovered = int((st["current_stage"] == 0).sum().item())
        assert reinfected == int(reinf.sum().item()) == int(((flags & 2) != 0).sum().item()), "the outputs disagree"
        kept_flags = flags.clone()

        def adjoint():
            N.check(lib.gj_adjoint_immunity(n, N.ptr(kept_flags), N.ptr(cls), tables, N.ptr(susc0), N.ptr(ones), N.ptr(ones),
                                            N.ptr(band), band_plan.n_groups, C.byref(band_plan.c), N.ptr(contrib),
                                            N.ptr(partial), N.ptr(sums[0]), N.ptr(sums[1]), N.ptr(g_outs[0]), None,
                                            N.ptr(g_outs[1]), N.current_stream()), "gj_adjoint_immunity")

        vsusc = susc0.clone()

        def vaccinate():
            N.check(lib.gj_vaccinate(n, N.ptr(cls), vaccine_tables, args.seed, VACCINE_STREAM, 0, N.ptr(vsusc), None,
                                     N.ptr(counts[0:1]), N.current_stream()), "gj_vaccinate")

        counts.zero_()
        vaccinate()
        vaccinated = int(counts[0].item())
        stats = timed(lambda: N.check(lib.gj_step_stats(
            n, N.ptr(cls), N.ptr(st["is_infected"]), N.ptr(st["current_stage"]), 3, age_edges, 7, N.ptr(national),
            N.current_stream()), "gj_step_stats"), args.warmup, args.launches)
        step = timed(runner.step, args.warmup, args.launches)      # (last: it moves the state on)
        case = {"seeded_fraction": fraction, "recovered": recovered, "waning": waning, "newly_infected": new,
                "reinfected": reinfected, "newly_vaccinated_per_launch": vaccinated, "hot_path_step": step,
                "gj_step_stats": stats}
        moved = 8 * waning + 4 * new + 4 * reinfected
        for key, fn, prepare, model in (
                ("gj_immunity_step", lambda: immunity_step(susc, inf), restore, 9 * n + moved),
                ("gj_immunity_step, flags_out", lambda: immunity_step(susc, inf, with_flags=True), restore, 10 * n + moved),
                ("gj_immunity_step, all outputs", lambda: immunity_step(susc, inf, with_all=True), restore,
                 18 * n + 4 * waning + 4 * new + 4 * reinfected),
                ("gj_adjoint_immunity", adjoint, None, 42 * n),
                ("gj_vaccinate", vaccinate, None, 5 * n + 4 * vaccinated)):
            t = timed(fn, args.warmup, args.launches, prepare)
            case[key] = dict(t, ratio_to_gj_step_stats=t["median_us"] / stats["median_us"],
                             ratio_to_hot_path_step=t["median_us"] / step["median_us"], model_bytes=model,
                             model_GBps=model / t["median_us"] * 1e-3)
        progress(f"{fraction}: recovered {recovered}, waning {waning}, new {new}, reinfected {reinfected}; immunity "
                 f"{case['gj_immunity_step']['median_us']:.1f} us, all outputs "
                 f"{case['gj_immunity_step, all outputs']['median_us']:.1f} us, adjoint "
                 f"{case['gj_adjoint_immunity']['median_us']:.1f} us; gj_vaccinate {case['gj_vaccinate']['median_us']:.1f} us; "
                 f"gj_step_stats {stats['median_us']:.1f} us; step {step['median_us']:.1f} us")
        out["cases"].append(case)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
