#!/usr/bin/env python3
"""An image-only batch on the shape-table loop (options simple_ports_images = 1 and
table_images = 1: k_static_pi + k_simple_tab_flat_pi / k_simple_tab_pi) against the two paths it
can take otherwise, k_simple_pi (table_images = 0) and k_schedule (simple_ports_images = 0), on the
same cluster in one process run.

The cluster is tests/portimage_fuzz.py's (5,000 nodes, 5,000 bound pods by default), every node
listing at least one image; the 10,000 pending pods are one container each, naming one of those
images, their requests drawn from a fixed list of 30 resource shapes, no host port.  Compiled once.
Each mode is checked against the C oracle (chosen nodes, every pod's outcome, final node rows, the
untouched UsedPorts column) before anything is timed; then the three modes alternate, `--pairs`
times, each run a reset and one kss_schedule_batch (wall clock around the call, which ends in the
read-back of the outcomes, and the library's device time of the launches).  Prints one JSON line;
--out writes it to a file as well.

  python tools/imagetable_bench.py --out profiles/imagetable_bench.json
"""
import argparse
import json
import os
import random
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

MI = 1024 * 1024
SHAPES = [{"cpu": c, "memory": m} for c in ("50m", "100m", "200m", "250m", "500m", "1")
          for m in ("64Mi", "128Mi", "256Mi", "512Mi", "1Gi")]  # 30 resource shapes
# mode -> (simple_ports_images, table_images, kernel)
MODES = {"k_schedule": (0, 0, "k_schedule"), "k_simple_pi": (1, 0, "k_simple"), "table": (1, 1, "k_simple")}


def manifests(seed, n_nodes, n_bound, n_pods):
    nodes, bound, _ = portimage_fuzz.make(seed, n_nodes=n_nodes, n_bound=n_bound, n_pods=0)
    r = random.Random(seed * 7919 + 3)
    for n in nodes:
        if not n["status"].get("images"):
            n["status"]["images"] = [{"names": [r.choice(portimage_fuzz.IMAGES)],
                                      "sizeBytes": r.choice([30, 400, 800, 1500, 3000]) * MI}]
    pods = [{"metadata": {"name": "p%05d" % j, "namespace": "default", "labels": {"app": "p"}},
             "spec": {"containers": [{"name": "c", "image": r.choice(portimage_fuzz.IMAGES),
                                      "resources": {"requests": dict(r.choice(SHAPES))}}]}} for j in range(n_pods)]
    return nodes, bound, pods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--bound", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    nodes, bound, pods = manifests(args.seed, args.nodes, args.bound, args.pods)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    cl, ps, n, N = cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes
    assert all(int(cp.pods[i]["img_len"]) > 0 for i in range(n)), "a pending pod names no node-cached image"
    assert not any(int(cp.pods[i]["port_conflict"]) | int(cp.pods[i]["port_add"]) for i in range(n))
    prof = abi.default_profile()
    ch_o, res, st = oracle_c.schedule(prof, cl, ps, n, N, threads=min(16, os.cpu_count() or 1), record="meta",
                                      n_classes=len(cc.classes), n_terms=len(cc.terms))
    want_meta = np.array([[m["chosen"], m["n_feasible"], m["scored"], m["status"], m["best_total"] if m["scored"] else 0]
                          for m in (res.meta(j) for j in range(n))], dtype=np.int64)
    native.reset_options()
    native.set_option("simple_ports_images", 1)
    _, n_shapes = native.plan_shapes(ps, len(cc.scalars))
    ctx = native.Context(prof)
    ctx.load(cl)

    def run(mode):
        pi, ti, kernel = MODES[mode]
        native.set_option("simple_ports_images", pi)
        native.set_option("table_images", ti)
        ctx.reset()
        t = time.perf_counter()
        chosen = ctx.schedule_batch(ps, n)
        wall = (time.perf_counter() - t) * 1e3
        assert ctx.last_kernel() == kernel, (mode, ctx.last_kernel())
        assert (ctx.last_shape_table()["shapes"] > 0) == (mode == "table"), (mode, ctx.last_shape_table())
        return chosen, wall, ctx.last_timing()[0]

    for mode in MODES:  # correctness first (also the warm-up of every path's kernels)
        chosen, _, _ = run(mode)
        assert (chosen == ch_o).all(), "%s: chosen nodes differ from the oracle" % mode
        meta = ctx.fetch_meta(n)
        meta[:, 4] *= meta[:, 2]
        assert (meta == want_meta).all(), "%s: pod outcomes differ from the oracle" % mode
        g = ctx.node_state()
        assert (g["requested"][:, :N] == st["requested"][:, :N]).all() and (g["pod_count"][:N] == st["pod_count"][:N]).all(), \
            "%s: node rows differ from the oracle" % mode
        assert (ctx.port_state() == st["port_used"][:N]).all() and (ctx.port_state() == cc.arrays["port_used"][:N]).all(), \
            "%s: UsedPorts changed" % mode
    wall, dev, info = {m: [] for m in MODES}, {m: [] for m in MODES}, {}
    for _ in range(args.pairs):
        for mode in MODES:
            _, w, d = run(mode)
            wall[mode].append(w)
            dev[mode].append(d)
            info[mode] = {"geometry": ctx.last_geometry(), "xcd_local": ctx.last_xcd_local(),
                          "last_shape_table": ctx.last_shape_table(), "last_simple_exchange": ctx.last_simple_exchange()}
    ctx.close()
    native.reset_options()

    def stats(x):
        x = np.array(x)
        return {"median": round(float(np.median(x)), 3), "min": round(float(x.min()), 3), "max": round(float(x.max()), 3)}

    out = {"metric": "image-only batch: shape-table loop (table_images = 1) vs k_simple_pi vs k_schedule",
           "seed": args.seed, "nodes": N, "bound": args.bound, "pods": n, "shapes": n_shapes, "pairs": args.pairs,
           "unschedulable": int((np.asarray(ch_o) < 0).sum())}
    for mode in MODES:
        out[mode] = dict(info[mode], wall_ms=stats(wall[mode]), device_ms=stats(dev[mode]),
                         us_per_pod=round(float(np.median(wall[mode])) * 1e3 / n, 3),
                         us_per_pod_min_max=[round(min(wall[mode]) * 1e3 / n, 3), round(max(wall[mode]) * 1e3 / n, 3)])
    ratios = np.array(wall["k_simple_pi"]) / np.array(wall["table"])
    out["table_vs_k_simple_pi_wall"] = {"median": round(float(np.median(ratios)), 3), "min": round(float(ratios.min()), 3),
                                        "max": round(float(ratios.max()), 3)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
