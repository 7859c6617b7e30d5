#!/usr/bin/env python3
"""A what-if sweep over scenarios whose pods hold volume programs, in the sweep's volumes form (options
sweep_ports_images = 1 and sweep_volumes = 1: k_static_pi + k_static_vol + k_simple_vol_sweep, one
workgroup per scenario) against what such a sweep had to do before: the same scenarios one after
another through kss_schedule_batch.

S scenarios of tools/volume_bench.py's generator (default 64, 700 nodes x 700 pending pods, a different
seed each: at most 64 volume rows and 8 limit keys, a third of the pods with a volume program, every
pod with an image), compiled once; 700 nodes is within the 768 node slots the form's LDS holds.  Every
scenario's chosen nodes are checked against the C oracle on all three routes before anything is
timed.  Then, `--pairs` rounds, interleaved:

  (a) Sweep.run() in the volumes form (wall clock around the call: reset, launches, read-back);
  (b) every scenario in turn on one context: kss_load_cluster (not timed), then kss_schedule_batch with
      simple_ports_images = 1 and simple_volumes = 1 (k_simple_vol; the wall clock of the batch calls, summed);
  (c) the same with simple_volumes = 0 (k_schedule).

Prints one JSON line; --out writes it to a file as well.

  python tools/sweep_volume_bench.py --out profiles/sweep_volume_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import oracle_c  # noqa: E402
import volume_bench  # noqa: E402
from kss import abi, native  # noqa: E402
from kss.compile import compile_cluster  # noqa: E402


def stats(x):
    x = np.array(x)
    return {"median": round(float(np.median(x)), 3), "min": round(float(x.min()), 3), "max": round(float(x.max()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", type=int, default=64)
    ap.add_argument("--seed", type=int, default=2000)
    ap.add_argument("--nodes", type=int, default=700)
    ap.add_argument("--bound", type=int, default=500)
    ap.add_argument("--pods", type=int, default=700)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    S = args.scenarios
    prof = abi.default_profile()
    threads = min(16, os.cpu_count() or 1)
    keep, clusters, podsets, want = [], [], [], []
    vol_pods = rows = 0
    t0 = time.perf_counter()
    for s in range(S):
        nodes, bound, pods, storage = volume_bench.make(args.seed + s, args.nodes, args.bound, args.pods)
        cc, cp, _ = compile_cluster(nodes, bound, pods, storage=storage)
        cl, ps = cc.as_struct(), cp.as_struct()
        assert cl.n_vol_rows <= 64 and cl.n_vol_keys <= 8, (s, cl.n_vol_rows, cl.n_vol_keys)
        ch_o, _, _ = oracle_c.schedule(prof, cl, ps, cp.n, cc.n_nodes, threads=threads, record=False,
                                       n_classes=len(cc.classes), n_terms=len(cc.terms))
        vol_pods += sum(int(cp.pods[i]["vol_len"] > 0) for i in range(cp.n))
        rows = max(rows, cl.n_vol_rows)
        keep.append((cc, cp))
        clusters.append(cl)
        podsets.append(ps)
        want.append(ch_o)
    prep_s = time.perf_counter() - t0
    want_all = np.concatenate(want)
    total = int(len(want_all))

    native.set_option("sweep_ports_images", 1)
    native.set_option("sweep_volumes", 1)
    native.set_option("simple_ports_images", 1)
    sw = native.Sweep(prof, clusters, podsets)
    info = sw.info()
    assert info["kernel"] == "k_simple" and info["volumes"], info
    ctx = native.Context(prof)
    kernel_of = {0: "k_schedule", 1: "k_simple"}

    def run_sweep():
        t = time.perf_counter()
        chosen, dev = sw.run()
        return chosen, (time.perf_counter() - t) * 1e3, dev

    def run_batches(on):
        native.set_option("simple_volumes", on)
        wall = dev = 0.0
        out = []
        for s in range(S):
            ctx.load(clusters[s])
            t = time.perf_counter()
            chosen = ctx.schedule_batch(podsets[s], podsets[s].n_pods)
            wall += (time.perf_counter() - t) * 1e3
            assert ctx.last_kernel() == kernel_of[on], (on, ctx.last_kernel())
            dev += ctx.last_timing()[0]
            out.append(chosen.copy())
        return np.concatenate(out), wall, dev

    # correctness first (also the warm-up of every route's kernels)
    assert (run_sweep()[0] == want_all).all(), "the sweep differs from the oracle"
    for on in (1, 0):
        assert (run_batches(on)[0] == want_all).all(), "%s batches differ from the oracle" % kernel_of[on]
    wall = {"a": [], "b": [], "c": []}
    dev = {"a": [], "b": [], "c": []}
    for _ in range(args.pairs):
        for mode in ("a", "b", "c"):
            _, w, d = run_sweep() if mode == "a" else run_batches(1 if mode == "b" else 0)
            wall[mode].append(w)
            dev[mode].append(d)
    sw.close()
    ctx.close()
    native.reset_options()

    def ratio(x, y):
        r = np.array(wall[x]) / np.array(wall[y])
        return {"median": round(float(np.median(r)), 2), "min": round(float(r.min()), 2), "max": round(float(r.max()), 2)}

    out = {"metric": "what-if sweep with volume programs: one sweep vs one kss_schedule_batch per scenario",
           "scenarios": S, "seed": args.seed, "nodes": args.nodes, "bound": args.bound, "pods": args.pods,
           "pairs": args.pairs, "total_pods": total, "pods_with_volume_programs": vol_pods, "max_volume_rows": rows,
           "unschedulable": int((want_all < 0).sum()),
           "prepare_s": round(prep_s, 1), "sweep_stage_ms": round(info["stage_ms"], 1), "upload_bytes": info["upload_bytes"],
           "a_sweep_wall_ms": stats(wall["a"]), "b_batches_k_simple_vol_wall_ms": stats(wall["b"]),
           "c_batches_k_schedule_wall_ms": stats(wall["c"]),
           "a_sweep_device_ms": stats(dev["a"]), "b_batches_k_simple_vol_device_ms": stats(dev["b"]),
           "c_batches_k_schedule_device_ms": stats(dev["c"]),
           "a_evals_per_s": round(total * args.nodes / (float(np.median(wall["a"])) * 1e-3), 1),
           "a_us_per_pod": round(float(np.median(wall["a"])) * 1e3 / max(total, 1), 3),
           "speedup_a_over_b_wall": ratio("b", "a"), "speedup_a_over_c_wall": ratio("c", "a")}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
