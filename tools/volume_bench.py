#!/usr/bin/env python3
"""A batch with volume programs on k_simple's volumes form (options simple_ports_images = 1 and
simple_volumes = 1: k_static_pi + k_static_vol + k_simple_vol) against the path it took before,
k_schedule (simple_volumes = 0), on the same cluster in one process run.

The cluster (5,000 nodes, 5,000 bound pods, 10,000 pending pods by default) comes from a generator
of its own that keeps the form's limits at that size: shared volumes are drawn from bounded name
pools (inline EBS / GCE PD disks and bound CSI claims, so <= 64 volume rows), private volumes are
CSI claims of one pod each (no row), and there are four limit keys (EBS, GCE PD, two CSI drivers).
Roughly a third of the pods carry a volume program; every pod runs an image some nodes list.  The
bounds are asserted on the CPU.  Each mode is checked against the C oracle (chosen nodes, final
vol_count / vol_attached) before anything is timed; then the two modes alternate, `--pairs` times,
each run a reset and one kss_schedule_batch (wall clock around the call, which ends in the read-back
of the outcomes, and the library's device time of the launches), at percentageOfNodesToScore = 100
by default.  --pct P (below 100; 0 is the adaptive window, the simulator's own setting) runs the
windowed search instead: the form's window kernels (option simple_volumes_window = 1) against
simple_volumes_window = 0, where the batch stays on k_schedule; nextStartNodeIndex is checked against
the oracle as well.  Prints one JSON line; --out writes it to a file as well.

  python tools/volume_bench.py --out profiles/volume_bench.json
  python tools/volume_bench.py --pct 0 --out profiles/volume_bench_pct0.json
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
import volume_fixtures as vf  # noqa: E402
from edge_fixtures import node  # noqa: E402
from kss import abi, native  # noqa: E402
from kss.compile import compile_cluster  # noqa: E402

MI = 1024 * 1024
ZONES = ["zone-a", "zone-b", "zone-c"]
DRIVERS = ["ebs.csi.aws.com", "pd.csi.storage.gke.io"]
IMAGES = ["app:v1", "app:v2", "base:latest", "registry:5000/tool:latest", "big:1"]
N_SHARED_CLAIMS, N_EBS, N_GCE = 16, 8, 6


def make(seed, n_nodes, n_bound, n_pods, share=1 / 3):
    r = random.Random(seed)
    nodes, csinodes = [], []
    for i in range(n_nodes):
        name = "n%05d" % i
        extra = {}
        if r.random() < 0.5:
            extra["attachable-volumes-aws-ebs"] = str(r.randint(1, 6))
        if r.random() < 0.5:
            extra["attachable-volumes-gce-pd"] = str(r.randint(1, 6))
        images = [{"names": [nm], "sizeBytes": r.choice([30, 400, 800, 1500, 3000]) * MI}
                  for nm in r.sample(IMAGES, r.choice([1, 2, 3]))]
        nodes.append(node(name, zone=r.choice(ZONES) if r.random() < 0.8 else None, cpu=r.choice(["16", "32"]),
                          mem=r.choice(["64Gi", "128Gi"]), extra=extra, images=images))
        if r.random() < 0.6:
            csinodes.append({"metadata": {"name": name},
                             "spec": {"drivers": [{"name": d, "allocatable": {"count": r.randint(1, 6)}} for d in DRIVERS]}})
    pvs, pvcs = [], []
    for k in range(N_SHARED_CLAIMS):
        labels = {vf.ZONE: r.choice(ZONES)} if r.random() < 0.3 else {}
        aff = None
        if r.random() < 0.3:
            aff = [{"matchExpressions": [{"key": vf.ZONE, "operator": "In", "values": r.sample(ZONES, 2)}]}]
        pvs.append(vf.pv("pv-s%d" % k, vf.csi(r.choice(DRIVERS), "h-s%d" % k), labels=labels, affinity_terms=aff))
        pvcs.append(vf.pvc("c-s%d" % k, "pv-s%d" % k))

    def volumes(tag, private):
        out = []
        for _ in range(r.choice([1, 1, 2])):
            x = r.random()
            if x < 0.2:
                out.append(vf.ebs("vol-%d" % r.randrange(N_EBS), ro=r.random() < 0.3))
            elif x < 0.35:
                out.append(vf.gce("pd-%d" % r.randrange(N_GCE), ro=r.random() < 0.5))
            elif x < 0.7 or not private:
                out.append(vf.claim("c-s%d" % r.randrange(N_SHARED_CLAIMS)))
            else:  # a claim of this pod alone: no row, a private count under its driver's key
                pvs.append(vf.pv("pv-p-%s-%d" % (tag, len(out)), vf.csi(r.choice(DRIVERS), "h-p-%s-%d" % (tag, len(out)))))
                pvcs.append(vf.pvc("c-p-%s-%d" % (tag, len(out)), "pv-p-%s-%d" % (tag, len(out))))
                out.append(vf.claim("c-p-%s-%d" % (tag, len(out))))
        return out

    def finish(p):
        c = p["spec"]["containers"][0]
        c["image"] = r.choice(IMAGES)
        c["resources"] = {"requests": {"cpu": r.choice(["100m", "250m", "500m"]), "memory": r.choice(["128Mi", "256Mi", "1Gi"])}}
        return p

    bound = [finish(vf.vpod("b%05d" % i, *(volumes("b%d" % i, False) if r.random() < share else []),
                            node_name="n%05d" % r.randrange(n_nodes))) for i in range(n_bound)]
    pods = [finish(vf.vpod("p%05d" % i, *(volumes("p%d" % i, True) if r.random() < share else []))) for i in range(n_pods)]
    return nodes, bound, pods, vf.storage(pvs, pvcs, [], csinodes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--bound", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--pct", type=int, default=100, help="percentageOfNodesToScore (0: adaptive)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    nodes, bound, pods, storage = make(args.seed, args.nodes, args.bound, args.pods)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=storage)
    cl, ps, n, N = cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes
    vol_pods = sum(int(cp.pods[i]["vol_len"] > 0) for i in range(n))
    img_pods = sum(int(cp.pods[i]["img_len"] > 0) for i in range(n))
    assert cl.n_vol_rows <= 64 and cl.n_vol_keys <= 8, (cl.n_vol_rows, cl.n_vol_keys)
    assert img_pods == n and 0.25 * n < vol_pods < 0.42 * n, (img_pods, vol_pods)
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    want = {0: "k_schedule", 1: "k_simple"}
    prof = abi.default_profile()
    prof.pct_nodes_to_score = args.pct
    windowed = args.pct < 100
    # the option that separates the two modes: under the window the form stays on, its window kernels toggle
    toggle = "simple_volumes_window" if windowed else "simple_volumes"
    for on in (0, 1):
        native.set_option(toggle, on)
        plan = native.plan_podset(cl, ps, prof)
        assert plan["kernel"] == want[on], (on, plan)
    ch_o, _, st = oracle_c.schedule(prof, cl, ps, n, N, threads=min(16, os.cpu_count() or 1), record=False,
                                    n_classes=len(cc.classes), n_terms=len(cc.terms))
    out = {"metric": "batch with volume programs: k_simple's volumes form vs k_schedule", "seed": args.seed, "nodes": N,
           "bound": args.bound, "pods": n, "pairs": args.pairs, "volume_rows": cl.n_vol_rows, "limit_keys": cl.n_vol_keys,
           "pods_with_volume_programs": vol_pods, "pods_with_images": img_pods, "unschedulable": int((ch_o < 0).sum()),
           "pct_nodes_to_score": args.pct, "next_start": int(st["next_start"])}
    ctx = native.Context(prof)
    ctx.load(cl)

    def run(on):
        native.set_option(toggle, on)
        ctx.reset()
        t = time.perf_counter()
        chosen = ctx.schedule_batch(ps, n)
        wall = (time.perf_counter() - t) * 1e3
        assert ctx.last_kernel() == want[on] and ctx.last_simple_form()["volumes"] == on, (on, ctx.last_kernel())
        return chosen, wall, ctx.last_timing()[0]

    for on in (0, 1):  # correctness first (also the warm-up of both paths' kernels)
        chosen, _, _ = run(on)
        assert (chosen == ch_o).all(), "%s differs from the oracle" % want[on]
        vc, va = ctx.volume_state()
        assert (vc == st["vol_count"]).all() and (va == st["vol_attached"]).all(), "volume state differs (%s)" % want[on]
        assert ctx.next_start_node_index() == st["next_start"], "nextStartNodeIndex differs (%s)" % want[on]
    geom, lds = {}, 0
    wall, dev = {0: [], 1: []}, {0: [], 1: []}
    for _ in range(args.pairs):
        for on in (0, 1):
            _, w, d = run(on)
            wall[on].append(w)
            dev[on].append(d)
            geom[want[on]] = ctx.last_geometry()
            lds = max(lds, ctx.last_simple_form()["lds_bytes"])
    ctx.close()

    def stats(x):
        x = np.array(x)
        return {"median": round(float(np.median(x)), 3), "min": round(float(x.min()), 3), "max": round(float(x.max()), 3)}

    ratios = np.array(wall[0]) / np.array(wall[1])
    out["pct%d" % args.pct] = {
        "geometry": geom, "k_simple_vol_lds_bytes": lds,
        "k_schedule_wall_ms": stats(wall[0]), "k_simple_vol_wall_ms": stats(wall[1]),
        "k_schedule_device_ms": stats(dev[0]), "k_simple_vol_device_ms": stats(dev[1]),
        "k_simple_vol_us_per_pod": round(float(np.median(wall[1])) * 1e3 / n, 3),
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
