#!/usr/bin/env python3
"""A batch WITH PodTopologySpread / InterPodAffinity programs in which about a third of the pods carry
volumes, on k_spread's volumes form (options spread_ports_images = 1 and spread_volumes = 1:
k_static_pi + k_static_vol + k_spread_vol) against the path it took before, k_schedule
(spread_volumes = 0), on the same cluster in one process run.

tools/spread_portimage_bench.py's cluster -- kss/synth.py make_cluster(3, ...) objects (the C3 recipe:
5,000 nodes in 3 zones, two bound pods per node, 10,000 pending pods by default) with
tests/spread_portimage_fuzz.py's graft of images and host ports -- and tests/spread_volume_fuzz.py's
graft of volumes on top (attach limits, CSINode counts, shared claims, inline disks, private claims),
compiled once.  Each mode is checked against the C oracle (chosen nodes, UsedPorts, vol_count,
vol_attached) before anything is timed; then the two modes alternate, `--pairs` times, each run a
reset and one kss_schedule_batch (wall clock around the call, which ends in the read-back of the
outcomes, and the library's device time of the launches).  The same at percentageOfNodesToScore = 0.
Prints one JSON line; --out writes it to a file as well.

  python tools/spread_volume_bench.py --out profiles/spread_volume_bench.json
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
import spread_volume_fuzz  # noqa: E402
from kss import abi, native  # noqa: E402
from kss.compile import compile_cluster  # noqa: E402
from kss.synth import make_cluster  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--share", type=float, default=0.33)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    nodes, bound, pods = make_cluster(3, args.nodes, args.pods)
    spread_portimage_fuzz.graft(args.seed, nodes, bound, pods)
    storage = spread_volume_fuzz.graft_volumes(args.seed, nodes, bound, pods, share=args.share)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=storage)
    cl, ps, n, N = cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes
    want = {0: "k_schedule", 1: "k_spread"}
    out = {"metric": "C3 recipe with images, host ports and volumes: k_spread's volumes form vs k_schedule",
           "seed": args.seed, "nodes": N, "bound": len(bound), "pods": n, "pairs": args.pairs,
           "volume_rows": int(cl.n_vol_rows), "limit_keys": int(cl.n_vol_keys),
           "volume_pods": int(sum(1 for i in range(n) if cp.pods[i]["vol_len"] > 0))}
    native.set_option("spread_ports_images", 1)
    for pct in (100, 0):
        prof = abi.default_profile()
        prof.pct_nodes_to_score = pct
        ch_o, _, st = oracle_c.schedule(prof, cl, ps, n, N, threads=min(16, os.cpu_count() or 1), record=False,
                                        n_classes=len(cc.classes), n_terms=len(cc.terms))
        ctx = native.Context(prof)
        ctx.load(cl)

        def run(on):
            native.set_option("spread_volumes", on)
            ctx.reset()
            t = time.perf_counter()
            chosen = ctx.schedule_batch(ps, n)
            wall = (time.perf_counter() - t) * 1e3
            assert ctx.last_kernel() == want[on], (on, ctx.last_kernel())
            assert ctx.last_spread_form()[0] == (2 if on else 0), ctx.last_spread_form()
            return chosen, wall, ctx.last_timing()[0]

        for on in (0, 1):  # correctness first (also the warm-up of both paths' kernels)
            chosen, _, _ = run(on)
            assert (chosen == ch_o).all(), "%s differs from the oracle at pct %d" % (want[on], pct)
            assert (ctx.port_state() == st["port_used"][:N]).all(), "UsedPorts differ from the oracle (%s)" % want[on]
            vc, va = ctx.volume_state()
            assert (vc == st["vol_count"]).all() and (va == st["vol_attached"]).all(), \
                "volume state differs from the oracle (%s)" % want[on]
        geom = {}
        wall, dev = {0: [], 1: []}, {0: [], 1: []}
        for _ in range(args.pairs):
            for on in (1, 0):
                _, w, d = run(on)
                wall[on].append(w)
                dev[on].append(d)
                geom[want[on]] = dict(ctx.last_geometry(), xcd_local=ctx.last_xcd_local()["used"],
                                      lds_bytes=ctx.last_spread_form()[1], launches=ctx.last_timing()[1])
        ctx.close()

        def stats(x):
            x = np.array(x)
            return {"median": round(float(np.median(x)), 3), "min": round(float(x.min()), 3),
                    "max": round(float(x.max()), 3)}

        ratios = np.array(wall[0]) / np.array(wall[1])
        dratios = np.array(dev[0]) / np.array(dev[1])
        out["pct%d" % pct] = {
            "unschedulable": int((ch_o < 0).sum()), "geometry": geom,
            "k_schedule_wall_ms": stats(wall[0]), "k_spread_vol_wall_ms": stats(wall[1]),
            "k_schedule_device_ms": stats(dev[0]), "k_spread_vol_device_ms": stats(dev[1]),
            "k_spread_vol_us_per_pod": {"wall": round(float(np.median(wall[1])) * 1e3 / n, 3),
                                        "device": round(float(np.median(dev[1])) * 1e3 / n, 3)},
            "k_schedule_us_per_pod": {"wall": round(float(np.median(wall[0])) * 1e3 / n, 3),
                                      "device": round(float(np.median(dev[0])) * 1e3 / n, 3)},
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
