#!/usr/bin/env python3
"""Per-pod latency of NodePorts / ImageLocality pods on the service grid: the k_simple-shaped
chain's ports-and-images form (option service_ports_images = 1) against the general chain
(option 0, which is where such a staged list ran before), on the same cluster in one process run.

tools/portimage_bench.py's cluster recipe (tests/portimage_fuzz.py: 5,000 nodes, 5,000 bound pods,
every node lists images, half the containers hold host ports), `--staged` pending pods staged and
the first `--pods` evaluated in order, each committed to the node it chose.  Both settings are
checked against the C oracle first (every record's outcome, verdicts, details and totals, the final
UsedPorts); then the two settings alternate, `--pairs` times: each run restages the list under its
setting and measures kss_service_eval full / slim / compact and the queued kss_service_commit,
medians over the pods.  The same at percentageOfNodesToScore = 0.  `--workload c2` runs the same
loops on a default-profile list without such pods (synthetic config 2), where both settings launch
the same kernel: any difference there is the box.  Prints one JSON line; --out writes it as well.

  python tools/service_portimage_bench.py --out profiles/service_portimage.json
"""
import argparse
import ctypes
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
from kss.synth import SEED_BASE  # noqa: E402

OPTION = "service_ports_images"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["portimage", "c2"], default="portimage")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--bound", type=int, default=5000)
    ap.add_argument("--staged", type=int, default=1000)
    ap.add_argument("--pods", type=int, default=300)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--stamps", action="store_true", help="also report shard 0's phase stamps (service_stamps)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n = args.pods
    keep = []
    if args.workload == "portimage":
        nodes, bound, pods = portimage_fuzz.make(args.seed, n_nodes=args.nodes, n_bound=args.bound, n_pods=args.staged)
        cc, cp, _ = compile_cluster(nodes, bound, pods)
        cl, ps, N, n_classes, n_terms = cc.as_struct(), cp.as_struct(), cc.n_nodes, len(cc.classes), len(cc.terms)
        keep = [cc, cp]
    else:
        s = native.Synth(2, SEED_BASE + 2, args.nodes, args.staged)
        cl, ps, N, n_classes, n_terms = s.cluster, s.pods, args.nodes, s.cluster.n_classes, s.cluster.n_terms
        keep = [s]
    L = native.lib()
    slim = abi.KSS_FIELD_FAIL | abi.KSS_FIELD_DETAIL | abi.KSS_FIELD_TOTAL
    out = {"metric": "service grid, NodePorts / ImageLocality pods: ports-and-images form of the k_simple-shaped "
                     "chain (option 1) vs the general chain (option 0)",
           "workload": args.workload, "seed": args.seed, "nodes": N, "bound": args.bound, "staged": args.staged,
           "pods": n, "pairs": args.pairs}
    if args.stamps:
        native.set_option("service_stamps", 1)
    for pct in (100, 0):
        prof = abi.default_profile()
        prof.pct_nodes_to_score = pct
        ch_o, res, st = oracle_c.schedule(prof, cl, ps, n, N, threads=min(16, os.cpu_count() or 1), record=True,
                                          n_classes=n_classes, n_terms=n_terms)
        ctx = native.Context(prof)
        ctx.load(cl)
        sview, cview = abi.PodView(), abi.PodCView()

        def fresh(on):
            native.set_option(OPTION, on)
            ctx.reset()
            ctx.stage(ps)  # the staged records follow the option

        def check(on):
            fresh(on)
            for j in range(n):
                got = ctx.service_eval(j)
                m = res.meta(j)
                assert (got.chosen, got.n_feasible, got.scored, got.status) == \
                       (m["chosen"], m["n_feasible"], m["scored"], m["status"]), (on, pct, j, m)
                assert (got.fail_plugin[:N] == res.fail_plugin[j, :N]).all(), (on, pct, j, "verdicts")
                assert (got.fail_detail[:N] == res.fail_detail[j, :N]).all(), (on, pct, j, "details")
                if m["scored"]:
                    kept = (res.fail_plugin[j, :N] == 0) & (res.fail_detail[j, :N] != abi.KSS_PASS_NOT_KEPT)
                    assert (got.total[:N][kept] == res.total[j, :N][kept]).all(), (on, pct, j, "totals")
                if got.chosen >= 0:
                    ctx.service_commit(j, got.chosen)
            mode, form = ctx.service_mode(), ctx.service_form()
            ctx.service_stop()
            assert (ctx.port_state()[:N] == st["port_used"][:N]).all(), "UsedPorts differ from the oracle (option %d)" % on
            return mode, form

        def loop(fields, compact=False):
            fn = L.kss_service_eval_compact if compact else L.kss_service_eval
            v = cview if compact else sview
            vp = ctypes.byref(v)
            t_eval, t_commit, stamps = [], [], []
            for j in range(n):
                a = time.perf_counter()
                native.check(fn(ctx.h, j, fields, vp))
                b = time.perf_counter()
                if v.chosen >= 0:
                    native.check(L.kss_service_commit(ctx.h, j, v.chosen))
                c = time.perf_counter()
                assert v.chosen == ch_o[j], (j, v.chosen, ch_o[j])
                t_eval.append(b - a)
                t_commit.append(c - b)
                if args.stamps:
                    stamps.append(ctx.service_stamps())
            ctx.service_stop()
            return np.array(t_eval) * 1e6, np.array(t_commit) * 1e6, stamps

        modes = {on: check(on) for on in (0, 1)}  # correctness first (also the warm-up of both chains' kernels)
        if args.workload == "portimage":
            assert modes[0][0] == 0 and modes[0][1][0] == 0 and modes[1][0] in (1, 2) and modes[1][1][0] == 1, modes
        else:
            assert modes[0] == modes[1] and modes[0][0] in (1, 2) and modes[0][1][0] == 0, modes
        med = {on: {"full": [], "slim": [], "compact": [], "commit": []} for on in (0, 1)}
        phases = {on: [] for on in (0, 1)}
        for _ in range(args.pairs):
            for on in (0, 1):
                fresh(on)
                ev, cm, stp = loop(abi.KSS_FIELD_ALL)
                med[on]["full"].append(float(np.median(ev)))
                med[on]["commit"].append(float(np.median(cm)))
                if stp:  # 100 MHz ticks -> us: command taken .. node pass .. statistics exchange .. keys .. visible
                    t = np.array(stp, dtype=np.float64) / 100.0
                    if on == 1 or args.workload == "c2":
                        phases[on].append([float(np.median(t[:, 5] - t[:, 0])), float(np.median(t[:, 6] - t[:, 5])),
                                           float(np.median(t[:, 7] - t[:, 6])), float(np.median(t[:, 3] - t[:, 7]))])
                    else:
                        phases[on].append([float(np.median(t[:, 2] - t[:, 0])), float(np.median(t[:, 3] - t[:, 2]))])
                fresh(on)
                med[on]["slim"].append(float(np.median(loop(slim)[0])))
                fresh(on)
                med[on]["compact"].append(float(np.median(loop(abi.KSS_FIELD_ALL, compact=True)[0])))
        geom = ctx.last_geometry()
        ctx.close()

        def stats(x):
            x = np.array(x)
            return {"median": round(float(np.median(x)), 2), "min": round(float(x.min()), 2), "max": round(float(x.max()), 2)}

        r = {"unschedulable": int((ch_o < 0).sum()), "geometry": geom,
             "service_mode": {str(on): modes[on][0] for on in (0, 1)},
             "lds_bytes": {str(on): modes[on][1][1] for on in (0, 1)}}
        for on in (0, 1):
            for k in ("full", "slim", "compact", "commit"):
                r["option%d_%s_us" % (on, k)] = stats(med[on][k])
            if phases[on]:
                r["option%d_phases_us" % on] = [round(float(x), 2) for x in np.median(np.array(phases[on]), axis=0)]
        for k in ("full", "slim", "compact"):
            ratios = np.array(med[0][k]) / np.array(med[1][k])
            r["speedup_" + k] = {"median": round(float(np.median(ratios)), 2), "min": round(float(ratios.min()), 2),
                                 "max": round(float(ratios.max()), 2)}
        out["pct%d" % pct] = r
    native.reset_options()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    del keep


if __name__ == "__main__":
    main()
