"""Cost of the Testing policy's launch and of its adjoint next to the step they precede, on one device.

    python tools/testing_cost.py [--agents 10000000] [--launches 30] [--warmup 5] [--earlier-steps 20] [--out FILE]

On the C3 world of bench.py (10 M agents, household-major order), seeded at 1 % and at 30 % infected and then run for
``--earlier-steps`` days of ``gj_testing_step`` + hot path + symptoms update, so that agents have reached the threshold,
decisions are pending and results fall due.  Then, on the state the last day left - the policy's five arrays restored
before every launch, outside the timed bracket - in one process, every launch bracketed by device events:
``gj_testing_step`` without optional outputs and without isolation, with ``qstate_out`` and ``newly_confirmed_out``
(what the Runner asks for with isolation and a labelling), with every optional output, ``gj_adjoint_testing`` (the
per-agent launch plus the pair of fp64 summing launches, three bands), and in the same run ``gj_immunity_step``,
``gj_step_stats`` and the hot-path step.  Per case: median, min, max over the launches, the ratios of the medians, and the
bandwidth the byte model implies - the launch reads 4 B stage + 4 B infection_time + 4 B decided + 4 B result_time + 1 B
class per agent; a decision writes 12 B, a report 4 B and reads 4 B, a confirmation writes 4 or 8 B; ``qstate_out``: + 4 B
read (isolate_until) and + 4 B written per agent; ``newly_confirmed_out``: + 4 B, ``flags_out``: + 1 B written per
agent.  Writes one JSON object (default profiles/testing_c3_10m.json) and prints it."""
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

STATE = ("decided", "result_time", "positive", "isolate_until", "confirmed_time")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "testing_c3_10m.json"))
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    import bench as B
    from grad_june_amd import _native as N
    from grad_june_amd import policies as GP
    from grad_june_amd.benchrun import SingleGpuHotPath
    from grad_june_amd.immunity import Immunity
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
    config = {"stage_threshold": 4, "probability": {"0-18": 0.1, "18-65": 0.4, "65-100": 0.7},
              "delay": {1: 0.2, 2: 0.5, 3: 0.3}, "isolation": {"days": 10, "compliance": 0.9}}
    policy = GP.Testing("2020-01-01", "2030-01-01", **config)
    tables = policy.tables()
    band, band_plan = policy.bands(cls.long() % 100)
    immunity_tables = Immunity({"0-50": 10.0, "50-100": 20.0}, 0.2).tables(1.0)
    progress(f"world: {n} agents; bands' plan: {band_plan.n_chunks} chunks")

    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    newly = torch.empty(n, dtype=torch.float32, device=dev)
    qstate = torch.empty(n, dtype=torch.float32, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    ones = torch.ones(n, dtype=torch.float32, device=dev)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    g_outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)]
    contrib = torch.empty(n, dtype=torch.float64, device=dev)
    partial = torch.empty(max(1, band_plan.n_chunks), dtype=torch.float64, device=dev)
    sums = torch.empty(band_plan.n_groups, dtype=torch.float64, device=dev)
    age_edges = (C.c_int32 * 4)(0, 18, 65, 100)
    national = torch.zeros(5, dtype=torch.float64, device=dev)

    def fresh():
        return {"decided": torch.full((n,), -1, dtype=torch.int32, device=dev),
                "result_time": torch.full((n,), float("inf"), dtype=torch.float32, device=dev),
                "positive": torch.zeros(n, dtype=torch.float32, device=dev),
                "isolate_until": torch.zeros(n, dtype=torch.float32, device=dev),
                "confirmed_time": torch.full((n,), -1.0, dtype=torch.float32, device=dev)}

    def testing_step(s, now, isolates=False, with_mask=False, with_all=False):
        mask = isolates or with_mask or with_all
        N.check(lib.gj_testing_step(
            n, N.ptr(cls), tables, N.ptr(st["current_stage"]), N.ptr(st["infection_time"]), policy.stage_threshold, 1,
            now, float("inf"), now + policy.isolation_days, policy.compliance, args.seed, GP.TESTING_STREAM,
            GP.TESTING_COMPLY_STREAM, 0, N.ptr(s["decided"]), N.ptr(s["result_time"]), N.ptr(s["positive"]),
            N.ptr(s["isolate_until"]) if mask else None, N.ptr(s["confirmed_time"]),
            N.ptr(newly) if with_mask or with_all else None, N.ptr(qstate) if mask else None,
            N.ptr(flags) if with_all else None, N.ptr(counts) if with_all else None, N.current_stream()),
            "gj_testing_step")

    out = {"device": torch.cuda.get_device_name(0), "n_agents": n, "launches": args.launches, "warmup": args.warmup,
           "earlier_steps": args.earlier_steps, "tile_geometry": "size-based defaults (not tuned)",
           "testing": {k: (v if not isinstance(v, dict) else {str(a): b for a, b in v.items()}) for k, v in config.items()},
           "byte_model": "17 B read per agent; 12 B written per decision, 4 B read and 4 B written per report, 4 or 8 B "
                         "written per confirmation; qstate_out: + 4 B read and + 4 B written, newly_confirmed_out: + 4 B, "
                         "flags_out: + 1 B written per agent; adjoint: 1 + 4 + 4 + 4 B read, 8 + 4 + 4 B written per "
                         "agent, then the plan's gathers",
           "cases": []}
    for fraction in (0.01, 0.30):
        runner.load_state(epidemic_state(n, fraction, args.seed))
        runner.enable_full_step()
        p = runner._sym_p
        state = fresh()
        for _ in range(args.earlier_steps):      # a day: testing (with its mask), hot path, symptoms
            testing_step(state, 1.0 + runner.t, isolates=True)
            runner.step()
            p.time, p.seed, p.step, p.agent_offset = float(runner.t), runner.seed, runner.t, 0
            N.check(lib.gj_symptoms_update(n, N.ptr(cls), N.ptr(runner.new_infected), N.ptr(st["current_stage"]),
                                           N.ptr(st["next_stage"]), N.ptr(st["time_to_next_stage"]), C.byref(p), None,
                                           None, N.current_stream()), "gj_symptoms_update")
        now = 1.0 + runner.t
        kept = {k: v.clone() for k, v in state.items()}

        def restore():
            for k in STATE:
                state[k].copy_(kept[k])

        counts.zero_()
        testing_step(state, now, with_all=True)
        confirmed, decisions = (int(v) for v in counts.tolist())
        due = int(((flags & N.GJ_TESTING_DUE) != 0).sum().item())
        isolating = int((qstate == 3).sum().item())
        at_threshold = int((~(st["current_stage"] < policy.stage_threshold)).sum().item())
        assert confirmed == int(newly.sum().item()), "the outputs disagree"
        kept_flags = flags.clone()
        restore()

        def adjoint():
            N.check(lib.gj_adjoint_testing(n, N.ptr(kept_flags), N.ptr(st["current_stage"]), N.ptr(ones), N.ptr(one),
                                           N.ptr(band), band_plan.n_groups, C.byref(band_plan.c), N.ptr(contrib),
                                           N.ptr(partial), N.ptr(sums), N.ptr(g_outs[0]), N.ptr(g_outs[1]),
                                           N.current_stream()), "gj_adjoint_testing")

        susc, inf = st["susceptibility"].clone(), st["is_infected"].clone()

        def immunity_step():
            N.check(lib.gj_immunity_step(n, N.ptr(cls), immunity_tables, N.ptr(st["current_stage"]), 0,
                                         N.ptr(runner.new_infected), N.ptr(susc), N.ptr(inf), None, None, None, None,
                                         N.current_stream()), "gj_immunity_step")

        stats = timed(lambda: N.check(lib.gj_step_stats(
            n, N.ptr(cls), N.ptr(st["is_infected"]), N.ptr(st["current_stage"]), 3, age_edges, 7, N.ptr(national),
            N.current_stream()), "gj_step_stats"), args.warmup, args.launches)
        case = {"seeded_fraction": fraction, "at_threshold": at_threshold, "decisions": decisions, "results_due": due,
                "confirmed": confirmed, "isolating": isolating, "gj_step_stats": stats}
        moved = 12 * decisions + 8 * due + 8 * confirmed
        cases = [
            ("gj_testing_step", lambda: testing_step(state, now), restore, 17 * n + moved),
            ("gj_testing_step, qstate_out and newly_confirmed_out", lambda: testing_step(state, now, with_mask=True), restore,
             29 * n + moved),
            ("gj_testing_step, all outputs", lambda: testing_step(state, now, with_all=True), restore, 30 * n + moved),
            ("gj_adjoint_testing", adjoint, None, 29 * n),
            ("gj_immunity_step", immunity_step, None, 9 * n)]
        measured = {key: (timed(fn, args.warmup, args.launches, prepare), model) for key, fn, prepare, model in cases}
        step = timed(runner.step, args.warmup, args.launches)      # (last: it moves the state on)
        case["hot_path_step"] = step
        for key, (t, model) in measured.items():
            case[key] = dict(t, ratio_to_gj_step_stats=t["median_us"] / stats["median_us"],
                             ratio_to_hot_path_step=t["median_us"] / step["median_us"], model_bytes=model,
                             model_GBps=model / t["median_us"] * 1e-3)
        progress(f"{fraction}: at the threshold {at_threshold}, decisions {decisions}, due {due}, confirmed {confirmed}, "
                 f"isolating {isolating}; testing {case['gj_testing_step']['median_us']:.1f} us, with the mask "
                 f"{case['gj_testing_step, qstate_out and newly_confirmed_out']['median_us']:.1f} us, all outputs "
                 f"{case['gj_testing_step, all outputs']['median_us']:.1f} us, adjoint "
                 f"{case['gj_adjoint_testing']['median_us']:.1f} us; gj_immunity_step "
                 f"{case['gj_immunity_step']['median_us']:.1f} us; gj_step_stats {stats['median_us']:.1f} us; step "
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
