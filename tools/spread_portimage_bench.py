#!/usr/bin/env python3
"""A batch WITH PodTopologySpread / InterPodAffinity programs whose pods reference images and hold
host ports, on k_spread's ports-and-images form (option spread_ports_images = 1: k_static_pi +
k_spread<.., PI>) against the path it took before, k_schedule (option 0), on the same cluster in
one process run.

kss/synth.py make_cluster(3, ...) objects (the C3 recipe: 5,000 nodes in 3 zones, two bound pods
per node, 10,000 pending pods by default) with tests/spread_portimage_fuzz.py's graft (every node
lists up to three images, every container names one, three in ten hold host ports), compiled once.
Each mode is checked against the C oracle (chosen nodes, final UsedPorts) before anything is timed;
then the two modes alternate, `--pairs` times, each run a reset and one kss_schedule_batch (wall
clock around the call, which ends in the read-back of the outcomes, and the library's device time
of the launches).  The same at percentageOfNodesToScore = 0.  Prints one JSON line; --out writes it
to a file as well.

  python tools/spread_portimage_bench.py --out profiles/spread_portimage_bench.json
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
import spread_portimage_fuzz  # noqa: E402
from kss import abi, native  # noqa: E402
from kss.compile import compile_cluster  # noqa: E402
from kss.synth import make_cluster  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    nodes, bound, pods = make_cluster(3, args.nodes, args.pods)
    spread_portimage_fuzz.graft(args.seed, nodes, bound, pods)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    cl, ps, n, N = cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes
    want = {0: "k_schedule", 1: "k_spread"}
    out = {"metric": "C3 recipe with images and host ports: k_spread's ports-and-images form vs k_schedule",
           "seed": args.seed, "nodes": N, "bound": len(bound), "pods": n, "pairs": args.pairs,
           "port_dictionary": len(cc.ports),
           "port_pods": int(sum(1 for i in range(n) if cp.pods[i]["port_add"] or cp.pods[i]["port_conflict"]))}
    for pct in (100, 0):
        prof = abi.default_profile()
        prof.pct_nodes_to_score = pct
        ch_o, _, st = oracle_c.schedule(prof, cl, ps, n, N, threads=min(16, os.cpu_count() or 1), record=False,
                                        n_classes=len(cc.classes), n_terms=len(cc.terms))
        ctx = native.Context(prof)
        ctx.load(cl)

        def run(on):
            native.set_option("spread_ports_images", on)
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
            for on in (1, 0):
                _, w, d = run(on)
                wall[on].append(w)
                dev[on].append(d)
                geom[want[on]] = dict(ctx.last_geometry(), xcd_local=ctx.last_xcd_local()["used"],
                                      lds_bytes=ctx.last_spread_lds())
        ctx.close()

        def stats(x):
            x = np.array(x)
            return {"median": round(float(np.median(x)), 3), "min": round(float(x.min()), 3),
                    "max": round(float(x.max()), 3)}

        ratios = np.array(wall[0]) / np.array(wall[1])
        dratios = np.array(dev[0]) / np.array(dev[1])
        out["pct%d" % pct] = {
            "unschedulable": int((ch_o < 0).sum()), "geometry": geom,
            "k_schedule_wall_ms": stats(wall[0]), "k_spread_pi_wall_ms": stats(wall[1]),
            "k_schedule_device_ms": stats(dev[0]), "k_spread_pi_device_ms": stats(dev[1]),
            "k_spread_pi_us_per_pod": {"wall": round(float(np.median(wall[1])) * 1e3 / n, 3),
                                       "device": round(float(np.median(dev[1])) * 1e3 / n, 3)},
            "k_schedule_us_per_pod": {"wall": round(float(np.median(wall[0])) * 1e3 / n, 3),
                                      "device": round(float(np.median(dev[0])) * 1e3 / n, 3)},
            "k_spread_pi_pods_per_s": round(n / (float(np.median(wall[1])) * 1e-3), 1),
            "k_schedule_pods_per_s": round(n / (float(np.median(wall[0])) * 1e-3), 1),
            "speedup_wall": {"median": round(float(np.median(ratios)), 2), "min": round(float(ratios.min()), 2),
                             "max": round(float(ratios.max()), 2)},
            "speedup_device": {"median": round(float(np.median(dratios)), 2), "min": round(float(dratios.min()), 2),
                               "max": round(float(dratios.max()), 2)},
            "faster_in_every_pair": bool((ratios > 1.0).all()),
        }
    native.reset_options()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
