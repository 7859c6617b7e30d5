#!/usr/bin/env python3
"""What the percentageOfNodesToScore window costs on the split grid.

On one GPU, for C2 (5,000 nodes x 10,000 pods, default profile: k_simple, 2 parts x 16 shards) and
C4 (100,000 nodes x 20,000 pods, zone spread: k_spread, 2 parts x 128 shards): the split grid
against the unsplit grid of the same build, at pct 0 (the adaptive window, the simulator's
setting) and at pct 100 (the reference gap).  Every run starts from reset node state and cursor 0;
the split and unsplit runs of one (config, pct) must choose the same nodes.  Wall time of the run
call (launches, kernels, the read-back of the chosen vector), median and best of --steps.

  python tools/split_window_bench.py --out profiles/split_window.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator_amd"))

SHAPES = {"c2": (2, 5000, 10000, 16), "c4": (4, 100000, 20000, 128)}


def timed(run, reset, steps, warmup):
    ts, out = [], None
    for i in range(warmup + steps):
        reset()
        t0 = time.perf_counter()
        out = run()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return ts, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="c2,c4")
    ap.add_argument("--pods", type=int, default=0, help="pods per run (default: the shape's own)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.zeros(1, device="cuda")  # torch's HIP runtime before libkss's
    from kss import abi, native, split
    from kss.synth import SEED_BASE
    rows = []
    for name in args.shapes.split(","):
        cfg, n_nodes, n_pods, wl = SHAPES[name]
        n_pods = args.pods or n_pods
        s = native.Synth(cfg, SEED_BASE + cfg, n_nodes, n_pods)
        for pct in (0, 100):
            prof = abi.default_profile()
            prof.pct_nodes_to_score = pct
            chosen = {}
            for grid in ("unsplit", "split"):
                if grid == "split":
                    sp = split.InProcessSplit(s.cluster, s.pods, 2, wl, profile=prof)
                    ctxs, run, close = sp.ctxs, (lambda: sp.run(n_pods)[0]), sp.close
                else:
                    c = native.Context(prof)
                    c.load(s.cluster)
                    c.stage(s.pods)
                    ctxs, run, close = [c], (lambda: c.run_staged(n_pods)), c.close

                def reset():
                    for x in ctxs:
                        x.reset()
                        x.set_next_start_node_index(0)

                ts, out = timed(run, reset, args.steps, args.warmup)
                chosen[grid] = np.asarray(out).copy()
                med = statistics.median(ts)
                row = {"shape": name, "config": cfg, "nodes": n_nodes, "pods": n_pods, "pct": pct, "grid": grid,
                       "parts": len(ctxs), "kernel": ctxs[0].last_kernel(), "geometry": ctxs[0].last_geometry(),
                       "xcd_local": ctxs[0].last_xcd_local()["used"] if grid == "unsplit" else 0,
                       "next_start": [x.next_start_node_index() for x in ctxs],
                       "pods_per_s_median": n_pods / med, "us_per_pod_median": med / n_pods * 1e6,
                       "pods_per_s_best": n_pods / min(ts), "us_per_pod_best": min(ts) / n_pods * 1e6,
                       "loop_kernel_ms_last": ctxs[0].last_loop_ms(), "seconds": ts}
                rows.append(row)
                print(json.dumps(row), flush=True)
                close()
            assert (chosen["split"] == chosen["unsplit"]).all(), (name, pct, "split and unsplit runs differ")
    gaps = {}
    for name in args.shapes.split(","):
        for pct in (0, 100):
            r = {x["grid"]: x for x in rows if x["shape"] == name and x["pct"] == pct}
            gaps[f"{name}_pct{pct}"] = {
                "unsplit_pods_per_s": r["unsplit"]["pods_per_s_median"], "split_pods_per_s": r["split"]["pods_per_s_median"],
                "split_over_unsplit": r["split"]["pods_per_s_median"] / r["unsplit"]["pods_per_s_median"],
                "extra_us_per_pod": r["split"]["us_per_pod_median"] - r["unsplit"]["us_per_pod_median"]}
    result = {"tool": "tools/split_window_bench.py", "steps": args.steps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "gaps": gaps, "runs": rows}
    print(json.dumps({"gaps": gaps}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
