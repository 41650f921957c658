"""Cost of the per-group result reductions next to the national ones, on one device.

    python tools/group_stats_cost.py [--agents 10000000] [--launches 50] [--warmup 10] [--out FILE]

Times ``gj_group_stats`` (both launches of a call) for G = agents / 8000 (the super areas of ``synthetic.super_area_map``),
G = agents / 300 (areas of 300) and G = 1, with the labels in world order (consecutive agents share a label) and
shuffled, and ``gj_adjoint_group_stats`` for the same labellings, next to ``gj_step_stats`` on the same is_infected /
current_stage arrays in the same process.  Every launch is bracketed by device events; per case: median, min, max over
the launches and the ratio of the medians to gj_step_stats'.  Prints one JSON object."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

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
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__ as entry

    entry.build()
    from grad_june_amd import _native as N
    from grad_june_amd.groups import GroupStats

    dev = torch.device("cuda", 0)
    lib = N.load()
    n, dead = args.agents, 7
    rng = np.random.default_rng(args.seed)
    inf = torch.from_numpy((rng.random(n) < 0.05).astype(np.float32)).to(dev)
    stage = torch.from_numpy(rng.integers(1, dead + 1, n).astype(np.float32)).to(dev)
    cls = torch.from_numpy(rng.integers(0, 200, n).astype(np.uint8)).to(dev)
    edges = (C.c_int32 * 4)(0, 18, 65, 100)
    national = torch.zeros(5, dtype=torch.float64, device=dev)

    def step_stats():
        N.check(lib.gj_step_stats(n, N.ptr(cls), N.ptr(inf), N.ptr(stage), 3, edges, dead, N.ptr(national),
                                  N.current_stream()), "gj_step_stats")

    out = {"device": torch.cuda.get_device_name(0), "n_agents": n, "launches": args.launches, "warmup": args.warmup,
           "bytes_per_agent": {"gj_step_stats": 9, "gj_group_stats": 12},
           "gj_step_stats": timed(step_stats, args.warmup, args.launches), "cases": []}
    base = out["gj_step_stats"]["median_us"]
    perm = torch.from_numpy(rng.permutation(n)).to(dev)
    ids = torch.arange(n, device=dev)
    for what, G, labels in (("super areas of 8000", -(-n // 8000), ids // 8000), ("areas of 300", -(-n // 300), ids // 300),
                            ("one group", 1, torch.zeros_like(ids))):
        for order in ("world", "shuffled"):
            if G == 1 and order == "shuffled":
                continue
            stats = GroupStats((labels if order == "world" else labels[perm]).to(torch.int32), G)
            row = torch.zeros(2 * G, dtype=torch.float64, device=dev)
            g = torch.ones(G, dtype=torch.float32, device=dev)
            fwd = timed(lambda: stats.add(inf, stage, dead, row), args.warmup, args.launches)
            stats.check()
            total = args.warmup + args.launches
            assert float(row[:G].sum()) == total * float(inf.sum(dtype=torch.float64)), "the sums are not the national ones"
            adj = timed(lambda: stats.gather(stage, dead, g, g), args.warmup, args.launches)
            again = timed(step_stats, 2, args.launches)           # the yardstick again, next to this case
            out["cases"].append({"labels": what, "n_groups": G, "order": order, "gj_group_stats": fwd,
                                 "ratio_to_gj_step_stats": fwd["median_us"] / base,
                                 "gj_adjoint_group_stats": adj, "gj_step_stats_again": again})
            print(f"[cost] G={G} {order}: {fwd['median_us']:.1f} us = {fwd['median_us'] / base:.2f} x gj_step_stats "
                  f"({base:.1f} us); adjoint {adj['median_us']:.1f} us", file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
