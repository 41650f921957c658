"""Cost of the symptom-stage reductions next to the national ones, on one device.

    python tools/stage_stats_cost.py [--agents 10000000] [--launches 50] [--warmup 10] [--out FILE]

Times ``gj_stage_stats`` for the national call (no labels) and for G = agents / 8000 labels (the super areas of
``synthetic.super_area_map``), in world order (consecutive agents share a label) and shuffled, and
``gj_adjoint_stage_stats`` for the same labellings, next to ``gj_step_stats`` on the same current_stage array in the
same process.  The stages are drawn as an epidemic has them: 90 % of the agents in `susceptible`, the others spread
over the eight stages; a third of the agents changed stage since the previous step (far more than in a run: every
entry is counted).  Every launch is bracketed by device events; per case: median, min, max over the launches and the
ratio of the medians to gj_step_stats'.  Then the Runner on the bundled 769-agent world with and without
``stages_to_save: all``: the added host time per step.  Prints one JSON object."""
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


def runner_step_cost(repeats, days):
    """Median wall time per step of Runner.forward() on the bundled world, without and with ``stages_to_save: all``."""
    import grad_june_amd as G
    from grad_june_amd.defaults import default_parameters

    out = {}
    for what, extra in (("without", {}), ("stages_to_save_all", {"stages_to_save": "all"}),
                        ("stages_to_save_all_by_area", {"stages_to_save": "all", "groups_to_save": ["area"]})):
        params = default_parameters("cuda:0")
        params["timer"]["total_days"] = days
        params.update(extra)
        runner = G.Runner.from_parameters(params)
        per_step = []
        for _ in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                results, _ = runner()
            torch.cuda.synchronize()
            per_step.append(1e6 * (time.perf_counter() - t0) / (len(results["dates"]) - 1))
        out[what] = {"median_us_per_step": float(np.median(per_step[1:])), "min_us_per_step": float(min(per_step[1:]))}
    base = out["without"]["median_us_per_step"]
    for what in list(out):
        out[what]["added_us_per_step"] = out[what]["median_us_per_step"] - base
    return {"world": "world769.npz", "n_agents": 769, "days": days, "repeats": repeats, **out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--agents", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--runner-repeats", type=int, default=5)
    ap.add_argument("--runner-days", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    from grad_june_amd import _native as N
    from grad_june_amd.groups import StageStats

    dev = torch.device("cuda", 0)
    lib = N.load()
    n, S, dead = args.agents, 8, 7
    rng = np.random.default_rng(args.seed)
    stage_h = np.where(rng.random(n) < 0.9, 1, rng.integers(0, S, n)).astype(np.float32)
    prev_h = np.where(rng.random(n) < 1.0 / 3.0, (stage_h + 1) % S, stage_h).astype(np.float32)
    stage, prev = torch.from_numpy(stage_h).to(dev), torch.from_numpy(prev_h).to(dev)
    inf = torch.from_numpy((rng.random(n) < 0.05).astype(np.float32)).to(dev)
    cls = torch.from_numpy(rng.integers(0, 200, n).astype(np.uint8)).to(dev)
    edges = (C.c_int32 * 4)(0, 18, 65, 100)
    national = torch.zeros(5, dtype=torch.float64, device=dev)

    def step_stats():
        N.check(lib.gj_step_stats(n, N.ptr(cls), N.ptr(inf), N.ptr(stage), 3, edges, dead, N.ptr(national),
                                  N.current_stream()), "gj_step_stats")

    out = {"device": torch.cuda.get_device_name(0), "n_agents": n, "n_stages": S, "launches": args.launches,
           "warmup": args.warmup,
           "bytes_per_agent": {"gj_step_stats": 9, "gj_stage_stats": 8, "gj_stage_stats_with_labels": 12,
                               "gj_adjoint_stage_stats": 12, "gj_adjoint_stage_stats_with_labels": 16},
           "gj_step_stats": timed(step_stats, args.warmup, args.launches), "cases": []}
    base = out["gj_step_stats"]["median_us"]
    perm = torch.from_numpy(rng.permutation(n)).to(dev)
    ids = torch.arange(n, device=dev)
    G8 = -(-n // 8000)
    want = np.bincount(stage_h.astype(np.int64), minlength=S)
    for what, G, labels in (("national", 1, None), ("super areas of 8000, world order", G8, (ids // 8000).to(torch.int32)),
                            ("super areas of 8000, shuffled", G8, (ids // 8000)[perm].to(torch.int32))):
        stats = StageStats(labels, G, S, device=dev)
        row = torch.zeros(2, G, S, dtype=torch.int64, device=dev)
        g = torch.ones(G, S, dtype=torch.float32, device=dev)
        fwd = timed(lambda: stats.add(stage, prev, row), args.warmup, args.launches)
        stats.check()
        total = args.warmup + args.launches
        assert np.array_equal(row[0].sum(0).cpu().numpy(), total * want), "the counts are not the national ones"
        adj = timed(lambda: stats.gather(stage, prev, g, g), args.warmup, args.launches)
        again = timed(step_stats, 2, args.launches)           # the yardstick again, next to this case
        bytes_ratio = (8 if labels is None else 12) / 9
        out["cases"].append({"labels": what, "n_groups": G, "regime": "one group" if G == 1 else (
                                 "lds" if G * S <= N.GJ_STAGE_LDS_BINS else "global"),
                             "gj_stage_stats": fwd, "ratio_to_gj_step_stats": fwd["median_us"] / base,
                             "byte_ratio_to_gj_step_stats": bytes_ratio, "gj_adjoint_stage_stats": adj,
                             "adjoint_ratio_to_gj_step_stats": adj["median_us"] / base, "gj_step_stats_again": again})
        print(f"[cost] {what}: {fwd['median_us']:.1f} us = {fwd['median_us'] / base:.2f} x gj_step_stats "
              f"({base:.1f} us; bytes {bytes_ratio:.2f} x); adjoint {adj['median_us']:.1f} us", file=sys.stderr, flush=True)
    out["runner"] = runner_step_cost(args.runner_repeats, args.runner_days)
    print(f"[cost] runner: {out['runner']}", file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
