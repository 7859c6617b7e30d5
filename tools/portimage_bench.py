#!/usr/bin/env python3
"""A NodePorts / ImageLocality batch on k_simple's ports-and-images form (option
simple_ports_images = 1: k_static_pi + k_simple_pi) against the path it took before, k_schedule
(option 0), on the same cluster in one process run.

tests/portimage_fuzz.py's cluster (5,000 nodes, 5,000 bound pods, 10,000 pending pods by default:
every node lists images, half the containers hold host ports), compiled once.  Each mode is checked
against the C oracle (chosen nodes, final UsedPorts) before anything is timed; then the two modes
alternate, `--pairs` times, each run a reset and one kss_schedule_batch (wall clock around the call,
which ends in the read-back of the outcomes, and the library's device time of the launches).  The
same at percentageOfNodesToScore = 0.  Prints one JSON line; --out writes it to a file as well.

  python tools/portimage_bench.py --out profiles/portimage_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import oracle_c  # noqa: E402
import portimage_fuzz  # noqa: E402
from kss import abi, native  # noqa: E402
from kss.compile import compile_cluster  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--bound", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    nodes, bound, pods = portimage_fuzz.make(args.seed, n_nodes=args.nodes, n_bound=args.bound, n_pods=args.pods)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    cl, ps, n, N = cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes
    want = {0: "k_schedule", 1: "k_simple"}
    out = {"metric": "NodePorts / ImageLocality batch: k_simple's ports-and-images form vs k_schedule",
           "seed": args.seed, "nodes": N, "bound": args.bound, "pods": n, "pairs": args.pairs}
    for pct in (100, 0):
        prof = abi.default_profile()
        prof.pct_nodes_to_score = pct
        ch_o, _, st = oracle_c.schedule(prof, cl, ps, n, N, threads=min(16, os.cpu_count() or 1), record=False,
                                        n_classes=len(cc.classes), n_terms=len(cc.terms))
        ctx = native.Context(prof)
        ctx.load(cl)

        def run(on):
            native.set_option("simple_ports_images", on)
            ctx.reset()
            t = time.perf_counter()
            chosen = ctx.schedule_batch(ps, n)
            wall = (time.perf_counter() - t) * 1e3
            assert ctx.last_kernel() == want[on], (on, ctx.last_kernel())
            return chosen, wall, ctx.last_timing()[0]

        for on in (0, 1):  # correctness first (also the warm-up of both paths' kernels)
            chosen, _, _ = run(on)
            assert (chosen == ch_o).all(), "%s differs from the oracle at pct %d" % (want[on], pct)
            assert (ctx.port_state() == st["port_used"][:N]).all(), "UsedPorts differ from the oracle (%s)" % want[on]
        geom = {}
        wall, dev = {0: [], 1: []}, {0: [], 1: []}
        for _ in range(args.pairs):
            for on in (0, 1):
                _, w, d = run(on)
                wall[on].append(w)
                dev[on].append(d)
                geom[want[on]] = ctx.last_geometry()
        ctx.close()

        def stats(x):
            x = np.array(x)
            return {"median": round(float(np.median(x)), 3), "min": round(float(x.min()), 3),
                    "max": round(float(x.max()), 3)}

        ratios = np.array(wall[0]) / np.array(wall[1])
        out["pct%d" % pct] = {
            "unschedulable": int((ch_o < 0).sum()), "geometry": geom,
            "k_schedule_wall_ms": stats(wall[0]), "k_simple_pi_wall_ms": stats(wall[1]),
            "k_schedule_device_ms": stats(dev[0]), "k_simple_pi_device_ms": stats(dev[1]),
            "k_simple_pi_us_per_pod": round(float(np.median(wall[1])) * 1e3 / n, 3),
            "k_schedule_us_per_pod": round(float(np.median(wall[0])) * 1e3 / n, 3),
            "speedup_wall": {"median": round(float(np.median(ratios)), 2), "min": round(float(ratios.min()), 2),
                             "max": round(float(ratios.max()), 2)},
        }
    native.reset_options()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
