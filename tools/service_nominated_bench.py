#!/usr/bin/env python3
"""Per-pod latency with a non-empty nominator: the service grid (kss_service_eval full / slim /
compact + kss_service_commit) against the launch-per-call path (kss_eval_pod_view + kss_commit),
which was the only path while pods were nominated, on the same state in one process run.

C2 cluster (5,000 nodes by default), 500 pods evaluated in order, 16 further pods of the highest
priority nominated to distinct nodes for the whole run (the nominator a saturated run's
PostFilters leave behind).  Prints one JSON line; --out writes it to a file as well.

  python tools/service_nominated_bench.py --out profiles/service_nominated.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator_amd"))

import numpy as np  # noqa: E402

from kss import abi, native  # noqa: E402
from kss.synth import SEED_BASE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=500)
    ap.add_argument("--nominees", type=int, default=16)
    ap.add_argument("--pct", type=int, default=100)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n_nodes, n_pods, n_nom = args.nodes, args.pods, args.nominees
    s = native.Synth(2, SEED_BASE + 2, n_nodes, n_pods + n_nom)
    top = max(s.pods.pods[j].priority for j in range(n_pods)) + 1000
    for j in range(n_pods, n_pods + n_nom):
        s.pods.pods[j].priority = top
    # distinct nodes spread over the node list (and so over the grid's shards)
    noms = [(n_pods + k, (k * n_nodes) // n_nom + 7 * k % max(n_nodes // n_nom, 1)) for k in range(n_nom)]
    assert len({n for _, n in noms}) == n_nom
    prof = abi.default_profile()
    prof.pct_nodes_to_score = args.pct
    ctx = native.Context(prof)
    ctx.load(s.cluster)
    pods_ref = ctypes.byref(s.pods)
    L = native.lib()

    def fresh():
        ctx.reset()  # empties the nominator too
        ctx.stage(s.pods)
        for j, n in noms:
            ctx.nominate(s.pods, j, n)

    view = abi.PodView()

    def launch_loop():
        t_eval, t_commit, ch = [], [], []
        for j in range(n_pods):
            a = time.perf_counter()
            native.check(L.kss_eval_pod_view(ctx.h, pods_ref, j, abi.KSS_FIELD_ALL, ctypes.byref(view)))
            b = time.perf_counter()
            if view.chosen >= 0:
                native.check(L.kss_commit(ctx.h, pods_ref, j, view.chosen))
            c = time.perf_counter()
            t_eval.append(b - a)
            t_commit.append(c - b)
            ch.append(view.chosen)
        return np.array(t_eval) * 1e6, np.array(t_commit) * 1e6, ch

    sview, cview = abi.PodView(), abi.PodCView()

    def svc_loop(fields, compact=False):
        fn = L.kss_service_eval_compact if compact else L.kss_service_eval
        v = cview if compact else sview
        vp = ctypes.byref(v)
        t_eval, t_commit, ch = [], [], []
        for j in range(n_pods):
            a = time.perf_counter()
            native.check(fn(ctx.h, j, fields, vp))
            b = time.perf_counter()
            if v.chosen >= 0:
                native.check(L.kss_service_commit(ctx.h, j, v.chosen))
            c = time.perf_counter()
            t_eval.append(b - a)
            t_commit.append(c - b)
            ch.append(v.chosen)
        mode = ctx.service_mode()
        ctx.service_stop()
        return np.array(t_eval) * 1e6, np.array(t_commit) * 1e6, ch, mode

    def stats(x):
        return {"median": round(float(np.median(x)), 2), "mean": round(float(x.mean()), 2),
                "p90": round(float(np.percentile(x, 90)), 2)}

    slim = abi.KSS_FIELD_FAIL | abi.KSS_FIELD_DETAIL | abi.KSS_FIELD_TOTAL
    fresh()
    launch_loop()  # warm both paths' kernels
    fresh()
    svc_loop(abi.KSS_FIELD_ALL)
    fresh()
    ev, cm, chosen = launch_loop()
    assert len(ctx.nominations()) == n_nom
    fresh()
    ev_f, cm_f, ch_f, mode = svc_loop(abi.KSS_FIELD_ALL)
    fresh()
    ev_s, _, ch_s, _ = svc_loop(slim)
    fresh()
    ev_c, _, ch_c, _ = svc_loop(abi.KSS_FIELD_ALL, compact=True)
    assert ch_f == chosen and ch_s == chosen and ch_c == chosen, "service choices differ from kss_eval_pod_view's"
    # the nominees' reach: the same run without them (choices that differ)
    ctx.reset()
    _, _, plain = launch_loop()
    out = {
        "metric": "per-pod latency with a non-empty nominator: service grid vs launch-per-call",
        "nodes": n_nodes, "pods": n_pods, "nominees": n_nom, "pct": args.pct, "service_mode": mode,
        "choices_changed_by_nominees": int(sum(1 for a, b in zip(chosen, plain) if a != b)),
        "launch_eval_view_us": stats(ev), "launch_commit_us": stats(cm),
        "service_eval_full_us": stats(ev_f), "service_eval_slim_us": stats(ev_s),
        "service_eval_compact_us": stats(ev_c), "service_commit_us": stats(cm_f),
        "speedup_full": round(float(np.median(ev) / np.median(ev_f)), 2),
        "speedup_slim": round(float(np.median(ev) / np.median(ev_s)), 2),
        "speedup_compact": round(float(np.median(ev) / np.median(ev_c)), 2),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()
    s.close()


if __name__ == "__main__":
    main()
