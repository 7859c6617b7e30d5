"""The batch path's routing table: which kernel, geometry and form a batch runs on (or which refusal
it gets), pinned case by case against tests/golden/path_table.json, and every scheduling result
against the C oracle bit for bit.

A batch routed to another kernel still gives the oracle's results, so the other GPU tests do not see
a routing change unless a feature needed the pin.  Here the whole decision is observed after every
call: last_kernel, last_geometry, last_xcd_local, last_shape_table, last_simple_exchange,
last_simple_form, last_spread_lds and last_timing()'s launch count; for a refused call the return
code and kss_last_error.

The golden is recorded, never derived from the library under test: run this file as a script
(`python tests/test_gpu_path_table.py --record`, with KSS_LIB naming the library that decides) on
the device the golden is for.  It stores the device's name and CU count; on another device the
shard counts differ and the whole module skips.

Cases are enumerated below (CASES), nothing is randomised.  Clusters are tiny: 1, 64, 65 and 1,000
nodes; 3,000 and 20,000 only where a branch needs them (noted at the case).  Split grids are left to
test_gpu_split*.py.

The spread geometry branches of the plan step, and the case that reaches each (per-slot LDS of
k_spread is about 150 B, so a shard holds about 1,000 nodes within the 160 KiB budget):
  * 512-lane preference: spread-1000-nps512 -- 2 shards of 500 nodes; the context's preferred 256
    lanes give 2 nodes per lane, SPREAD_PREF_THREADS gives 512 x 1;
  * KSS_MAX_THREADS retry: spread-1000-nps512-threads64 -- option threads skips the preference;
    128 lanes x 4 leave 64 prefetch lanes 8 words each (G_PF is 4), 512 x 1 fits;
  * shard doubling: c4-20000-nps4096 -- 7 shards of 2,858 nodes exceed LDS; 14 (1,429) still do; 28 fit;
  * XCD shrink: spread-1000-xcdshards4 -- 8 shards do not fit a 4-CU XCD-local grid, 4 of 250 nodes do;
  * one workgroup after all (need.xw > XW_MAX): rack130-3000-shards2 -- k_spread admits the 267-value
    exchange (G_XW 512) but a 1,500-node shard exceeds LDS and option shards forbids doubling, so
    k_schedule runs, whose granules hold 256 values: one workgroup.
"""
import copy
import json
import os
import sys

if __name__ == "__main__":
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_ROOT, os.path.join(_ROOT, "kube-scheduler-simulator_amd"), os.path.join(_ROOT, "oracle"),
               os.path.join(_ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import numpy as np
import pytest

import oracle_c
import volume_fuzz
from edge_fixtures import HOST, ZONE, node, pod
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_table.json")
FLAGS = {"single": abi.KSS_SCHED_FORCE_SINGLE_WG, "multi": abi.KSS_SCHED_FORCE_MULTI_WG,
         "general": abi.KSS_SCHED_GENERAL_KERNEL}
RACK, FOO = "example.com/rack", "example.com/foo"
N_PODS = 12


# --------------------------------------------------------------------------------------
# clusters and batches
# --------------------------------------------------------------------------------------
def _nodes(n, racks=0, images=False, foo=False):
    out = []
    for i in range(n):
        img = [{"names": ["img%d:v1" % (i % 3)], "sizeBytes": (200 + 100 * (i % 3)) << 20}] if images else None
        out.append(node("n%05d" % i, zone="z%d" % (i % 3), cpu=str(4 + 2 * (i % 3)), mem="%dGi" % (8 + 4 * (i % 2)),
                        labels={RACK: "r%d" % (i % racks)} if racks else None, images=img,
                        extra={FOO: str(2 + i % 3)} if foo else None))
    return out


def _pods(kind, n_nodes):
    shapes = [{"cpu": "250m", "memory": "256Mi"}, {"cpu": "500m", "memory": "1Gi"}, {"cpu": "1", "memory": "512Mi"}]
    out = []
    for j in range(N_PODS):
        p = pod("p%02d" % j, requests=shapes[j % 3], labels={"app": "a%d" % (j % 2)})
        c = p["spec"]["containers"][0]
        if kind == "names" and j % 4 == 0:  # a PreFilterResult node list
            names = ["n%05d" % (i % n_nodes) for i in range(j, j + 3)]
            p["spec"]["affinity"] = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {
                "nodeSelectorTerms": [{"matchFields": [{"key": "metadata.name", "operator": "In", "values": names}]}]}}}
        if kind in ("ports", "spread-pi") and j % 2 == 0:
            c["ports"] = [{"containerPort": 80, "hostPort": 8000 + j % 4, "protocol": "TCP"}]
        if kind in ("ports", "images", "spread-pi"):
            c["image"] = "img%d:v1" % (j % 3)
        if kind in ("spread", "spread-pi", "nominated-spread"):
            sel = {"matchLabels": {"app": "a%d" % (j % 2)}}
            p["spec"]["topologySpreadConstraints"] = [
                {"maxSkew": 2, "topologyKey": ZONE, "whenUnsatisfiable": "DoNotSchedule", "labelSelector": sel},
                {"maxSkew": 1, "topologyKey": HOST, "whenUnsatisfiable": "ScheduleAnyway", "labelSelector": sel}]
            if j % 3 == 0:
                p["spec"]["affinity"] = {"podAntiAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
                    {"weight": 10, "podAffinityTerm": {"labelSelector": sel, "topologyKey": ZONE}}]}}
        if kind == "rack":  # a hard constraint over a key of many values: a long exchange vector
            p["spec"]["topologySpreadConstraints"] = [
                {"maxSkew": 3, "topologyKey": RACK, "whenUnsatisfiable": "DoNotSchedule",
                 "labelSelector": {"matchLabels": {"app": "a%d" % (j % 2)}}}]
        if kind == "foo":
            c["resources"]["requests"][FOO] = "1"
        if kind == "nominated" or kind == "nominated-spread":
            p["spec"]["priority"] = 1000 if j == N_PODS - 1 else 0
        out.append(p)
    return out


_CLUSTERS = {}


def _cluster(kind, n_nodes, racks=0):
    """(cluster struct, podset struct, n_nodes, n_classes, n_terms, keep-alive) -- built once, never written."""
    key = (kind, n_nodes, racks)
    if key in _CLUSTERS:
        return _CLUSTERS[key]
    if kind in ("c1", "c4"):  # the synthetic recipes, for the 20,000-node cases
        s = native.Synth(1 if kind == "c1" else 4, 7, n_nodes, N_PODS)
        v = (s.cluster, s.pods, n_nodes, s.cluster.n_classes, s.cluster.n_terms, s)
    elif kind in ("vol", "vol-wffc"):
        nodes, bound, pods, st = volume_fuzz.make(5, n_nodes=n_nodes, n_bound=min(n_nodes, 16), n_pods=N_PODS,
                                                  wffc=kind == "vol-wffc")
        cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
        v = (cc.as_struct(), cp.as_struct(), cc.n_nodes, len(cc.classes), len(cc.terms), (cc, cp))
    else:
        nodes = _nodes(n_nodes, racks=racks, images=kind in ("ports", "images", "spread-pi"), foo=kind == "foo")
        cc, cp, _ = compile_cluster(nodes, [], _pods(kind, n_nodes))
        v = (cc.as_struct(), cp.as_struct(), cc.n_nodes, len(cc.classes), len(cc.terms), (cc, cp))
    _CLUSTERS[key] = v
    return v


def _profile(tag, pct):
    p = abi.default_profile()
    if tag == "weights":  # a non-default profile
        p.weight[abi.KSS_S_NODE_RESOURCES_FIT] = 3
        p.weight[abi.KSS_S_BALANCED_ALLOCATION] = 2
    elif tag == "scores-foo":  # NodeResourcesFit scores the extended resource
        p.fit_n = 3
        p.fit_res[2], p.fit_weight[2] = abi.KSS_RES_SCALAR0, 1
    p.pct_nodes_to_score = pct
    return p


# --------------------------------------------------------------------------------------
# the cases: (name, kind, nodes, how it is called, pct, profile, options, flag, extras)
# --------------------------------------------------------------------------------------
def _case(name, kind, n, api="staged", pct=100, prof="default", opts=None, flag=None, racks=0):
    return dict(name=name, kind=kind, n=n, api=api, pct=pct, prof=prof, opts=opts or {}, flag=flag, racks=racks)


PI = dict(simple_ports_images=1)
VOL = dict(simple_ports_images=1, simple_volumes=1)


def _cases():
    c = []
    # plain batches: the cluster-size edges, every call form, the window, the flags
    for n in (1, 64, 65, 1000):
        for pct in (100, 50, 0):
            c.append(_case("plain-%d-pct%d" % (n, pct), "plain", n, pct=pct))
        c.append(_case("plain-%d-record" % n, "plain", n, api="record"))
    c.append(_case("plain-1000-eval", "plain", 1000, api="eval"))
    c.append(_case("plain-1000-eval-pct50", "plain", 1000, api="eval", pct=50))
    for f in FLAGS:
        c.append(_case("plain-1000-%s" % f, "plain", 1000, flag=f))
        c.append(_case("plain-65-%s" % f, "plain", 65, flag=f))
        c.append(_case("spread-1000-%s" % f, "spread", 1000, flag=f))
    # geometry options on k_simple: shards, nodes_per_shard, xcd, xcd_shards, threads, force_threads
    for nm, o in (("shards3", dict(shards=3)), ("shards1", dict(shards=1)), ("nps64", dict(nodes_per_shard=64)),
                  ("xcd0", dict(xcd=0)), ("xcdshards4", dict(xcd_shards=4)), ("threads64", dict(threads=64)),
                  ("force192", dict(shards=3, force_threads=192)), ("force64-1shard", dict(shards=1, force_threads=64))):
        c.append(_case("plain-1000-" + nm, "plain", 1000, opts=o))
        c.append(_case("plain-1000-pct50-" + nm, "plain", 1000, pct=50, opts=o))
    # the shape table and its exchange
    for st in (0, 1, 2):
        for fl in (0, 1):
            o = dict(shape_table=st, flat_exchange=fl)
            c.append(_case("plain-1000-table%d-flat%d" % (st, fl), "plain", 1000, opts=o))
            c.append(_case("plain-64-table%d-flat%d" % (st, fl), "plain", 64, opts=o))
    c.append(_case("plain-1000-table1-pct50", "plain", 1000, pct=50, opts=dict(shape_table=1)))
    c.append(_case("plain-1000-no_simple", "plain", 1000, opts=dict(no_simple=1)))
    c.append(_case("plain-1000-weights", "plain", 1000, prof="weights"))
    c.append(_case("plain-1000-weights-pct50", "plain", 1000, prof="weights", pct=50))
    # 20,000 nodes: k_simple's 64 * SX_CHUNKS cap on the automatic shard count
    c.append(_case("c1-20000", "c1", 20000))
    c.append(_case("c1-20000-pct0", "c1", 20000, pct=0))
    # PreFilterResult name lists: a windowed batch leaves the loop kernels
    for pct in (100, 50):
        c.append(_case("names-1000-pct%d" % pct, "names", 1000, pct=pct))
        c.append(_case("names-64-pct%d" % pct, "names", 64, pct=pct))
    # host ports / images: each form option off and on
    for kind in ("ports", "images"):
        for n in (65, 1000):
            for pct in (100, 50):
                for on in (0, 1):
                    c.append(_case("%s-%d-pct%d-pi%d" % (kind, n, pct, on), kind, n, pct=pct,
                                   opts=dict(simple_ports_images=on)))
        for ti in (0, 1):
            for st in (1, 2):
                c.append(_case("%s-1000-pi1-ti%d-table%d" % (kind, ti, st), kind, 1000,
                               opts=dict(PI, table_images=ti, shape_table=st)))
        c.append(_case("%s-1000-pi1-ti1-flat0" % kind, kind, 1000, opts=dict(PI, table_images=1, flat_exchange=0)))
    # volumes: the form, its window option, a batch the form does not admit
    for kind in ("vol", "vol-wffc"):
        for n in (65, 1000):
            for pct in (100, 50):
                for o_nm, o in (("off", {}), ("pi-only", PI), ("vol", VOL), ("vol-win", dict(VOL, simple_volumes_window=1)),
                                ("vol-nopi", dict(simple_volumes=1))):
                    if kind == "vol-wffc" and o_nm not in ("vol", "vol-win"):
                        continue
                    c.append(_case("%s-%d-pct%d-%s" % (kind, n, pct, o_nm), kind, n, pct=pct, opts=o))
    c.append(_case("vol-1000-vol-shards3", "vol", 1000, opts=dict(VOL, shards=3)))
    c.append(_case("vol-1000-vol-table2", "vol", 1000, opts=dict(VOL, shape_table=2, table_images=1)))
    # spread / inter-pod programs: k_spread, its window, fold, its ports-and-images form
    for n in (1, 64, 65, 1000):
        for pct in (100, 50, 0):
            c.append(_case("spread-%d-pct%d" % (n, pct), "spread", n, pct=pct))
    c.append(_case("spread-1000-record", "spread", 1000, api="record"))
    c.append(_case("spread-1000-eval", "spread", 1000, api="eval"))
    for nm, o in (("fold", dict(fold=1)), ("no_spread", dict(no_spread=1)), ("no_simple", dict(no_simple=1)),
                  ("shards3", dict(shards=3)), ("xcd0", dict(xcd=0)), ("xcdshards4", dict(xcd_shards=4)),
                  ("nps512", dict(nodes_per_shard=512)), ("nps512-threads64", dict(nodes_per_shard=512, threads=64)),
                  ("nps512-force128", dict(nodes_per_shard=512, force_threads=128)), ("spi1", dict(spread_ports_images=1))):
        c.append(_case("spread-1000-" + nm, "spread", 1000, opts=o))
        c.append(_case("spread-1000-pct50-" + nm, "spread", 1000, pct=50, opts=o))
    # programs and host ports / images in one batch: k_spread's ports-and-images form, option off and on,
    # under the window, with the fold (which the form does not take), under a runtime profile
    for n in (65, 1000):
        for pct in (100, 50):
            for on in (0, 1):
                c.append(_case("spread-pi-%d-pct%d-spi%d" % (n, pct, on), "spread-pi", n, pct=pct,
                               opts=dict(spread_ports_images=on)))
    for nm, o in (("fold", dict(fold=1)), ("shards3", dict(shards=3)), ("xcd0", dict(xcd=0)), ("nps512", dict(nodes_per_shard=512)),
                  ("simple-pi", dict(simple_ports_images=1))):
        c.append(_case("spread-pi-1000-spi1-" + nm, "spread-pi", 1000, opts=dict(o, spread_ports_images=1)))
    c.append(_case("spread-pi-1000-pct50-spi1-fold", "spread-pi", 1000, pct=50, opts=dict(fold=1, spread_ports_images=1)))
    c.append(_case("spread-pi-1000-spi1-weights", "spread-pi", 1000, prof="weights", opts=dict(spread_ports_images=1)))
    c.append(_case("spread-1000-weights", "spread", 1000, prof="weights"))
    c.append(_case("spread-1000-weights-pct50", "spread", 1000, prof="weights", pct=50))
    # 20,000 nodes (C4's recipe): more than 64 shards (the two-level exchange area), shard doubling
    c.append(_case("c4-20000", "c4", 20000))
    c.append(_case("c4-20000-pct0", "c4", 20000, pct=0))
    c.append(_case("c4-20000-shards80", "c4", 20000, opts=dict(shards=80)))
    c.append(_case("c4-20000-nps4096", "c4", 20000, opts=dict(nodes_per_shard=4096)))
    # programs past k_spread's tables (300 rack values: 607 exchange values, G_XW is 512) and past
    # k_schedule's granules (XW_MAX 256): one workgroup, or refused where one cannot hold the cluster
    c.append(_case("rack300-1000", "rack", 1000, racks=300))
    c.append(_case("rack300-1000-pct50", "rack", 1000, racks=300, pct=50))
    c.append(_case("rack300-1000-multi", "rack", 1000, racks=300, flag="multi"))
    c.append(_case("rack300-20000-refused", "rack", 20000, racks=300))
    c.append(_case("rack130-3000-shards2", "rack", 3000, racks=130, opts=dict(shards=2)))
    c.append(_case("rack130-3000", "rack", 3000, racks=130))
    # a profile that scores an extended resource; extended resources the profile does not score
    for n in (65, 1000):
        c.append(_case("foo-%d" % n, "foo", n))
        c.append(_case("foo-%d-scored" % n, "foo", n, prof="scores-foo"))
        c.append(_case("foo-%d-scored-pct50" % n, "foo", n, prof="scores-foo", pct=50))
    # a nominated pod (the last of the batch, not run): k_schedule
    for kind in ("nominated", "nominated-spread"):
        for pct in (100, 50):
            c.append(_case("%s-1000-pct%d" % (kind, pct), kind, 1000, pct=pct))
    c.append(_case("nominated-1000-eval", "nominated", 1000, api="eval"))
    names = [x["name"] for x in c]
    assert len(names) == len(set(names))
    return c


CASES = _cases()


# --------------------------------------------------------------------------------------
# one case: the routing tuple, and the results against the oracle
# --------------------------------------------------------------------------------------
def _observe(ctx):
    t = ctx.last_timing()[1]
    return dict(kernel=ctx.last_kernel(), geometry=ctx.last_geometry(), xcd_local=ctx.last_xcd_local(),
                shape_table=ctx.last_shape_table(), simple_exchange=ctx.last_simple_exchange(),
                simple_form=ctx.last_simple_form(), spread_lds=ctx.last_spread_lds(), launches=t)


def _refused(e):
    """A refusal is a routing decision (KSS_E_UNSUPPORTED -95, KSS_E_INVAL -22); a device error is not."""
    if e.rc not in (-95, -22):
        raise e
    return dict(refused=[e.rc, str(e)])


_ORACLE = {}


def _oracle(case, cl, ps, prof, n_run, N, ncl, nt, noms):
    key = (case["kind"], case["n"], case["racks"], case["pct"], case["prof"], n_run)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_c.schedule(prof, cl, ps, n_run, N, record=True, n_classes=ncl, n_terms=nt,
                                         nominations=noms, threads=min(16, os.cpu_count() or 1))
    return _ORACLE[key]


def run_case(case):
    """The case's routing tuple (or refusal) as the loaded library decides it; the results are
    compared with the oracle's on the way."""
    cl, ps, N, ncl, nt, _keep = _cluster(case["kind"], case["n"], case["racks"])
    prof = _profile(case["prof"], case["pct"])
    native.reset_options()
    for k, v in case["opts"].items():
        native.set_option(k, v)
    nominated = case["kind"].startswith("nominated")
    n_run = N_PODS - 1 if nominated else N_PODS
    noms = [(N_PODS - 1, min(3, N - 1))] if nominated else []
    record = case["api"] == "record"
    ctx = native.Context(prof, max_pods_record=N_PODS if record else 0)
    try:
        ctx.load(cl)
        for j, nd in noms:
            ctx.nominate(ps, j, nd)
        flags = FLAGS[case["flag"]] if case["flag"] else 0
        if case["api"] == "eval":
            ch_o, res, _ = _oracle(case, cl, ps, prof, 1, N, ncl, nt, noms)
            try:
                r = ctx.eval_pod(ps, 0)
            except native.KssError as e:
                return _refused(e)
            assert r.chosen == ch_o[0]
            np.testing.assert_array_equal(r.fail_plugin[:N], res.fail_plugin[0, :N])
            m = res.meta(0)
            assert (r.n_feasible, r.scored, r.status) == (m["n_feasible"], m["scored"], m["status"])
            # the oracle filters every node and cuts the list afterwards: the kept nodes are the first
            # n_feasible that pass, from nextStartNodeIndex 0
            kept = np.flatnonzero(res.fail_plugin[0, :N] == 0)[:m["n_feasible"]]
            if r.scored:
                np.testing.assert_array_equal(r.total[:N][kept], res.total[0, :N][kept])
            return _observe(ctx)
        try:
            if case["api"] == "staged":
                ctx.stage(ps)
                chosen = ctx.run_staged(n_run, flags=flags)
            else:
                chosen = ctx.schedule_batch(ps, n_run, record=True, flags=flags)
        except native.KssError as e:
            return _refused(e)
        obs = _observe(ctx)
        ch_o, res, st = _oracle(case, cl, ps, prof, n_run, N, ncl, nt, noms)
        np.testing.assert_array_equal(chosen[:n_run], ch_o)
        meta = ctx.fetch_meta(n_run)
        for j in range(n_run):
            m = res.meta(j)
            got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
            assert got == {k: m[k] for k in got}, (j, got, m)
            if m["scored"]:
                assert meta[j, 4] == m["best_total"], j
        g = ctx.node_state()
        np.testing.assert_array_equal(g["requested"][:, :N], st["requested"][:, :N])
        np.testing.assert_array_equal(g["nonzero"][:, :N], st["nonzero"][:, :N])
        np.testing.assert_array_equal(g["pod_count"][:N], st["pod_count"][:N])
        if ncl:
            np.testing.assert_array_equal(g["class_count"][:ncl, :N], st["class_count"][:ncl, :N])
        np.testing.assert_array_equal(ctx.port_state()[:N], st["port_used"][:N])
        if cl.n_vol_rows:
            vc, va = ctx.volume_state()
            np.testing.assert_array_equal(vc, st["vol_count"])
            np.testing.assert_array_equal(va, st["vol_attached"])
        assert ctx.next_start_node_index() == st["next_start"]
        if record:
            for j in range(n_run):
                r = ctx.fetch_record(j)
                np.testing.assert_array_equal(r.fail_plugin[:N], res.fail_plugin[j, :N])
        return obs
    finally:
        ctx.close()
        native.reset_options()


def _device():
    import torch
    p = torch.cuda.get_device_properties(0)
    return dict(name=p.name, cus=int(p.multi_processor_count))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    dev = _device()
    if g["device"] != dev:
        pytest.skip("the golden was recorded on %s, this is %s" % (g["device"], dev))
    assert sorted(g["cases"]) == sorted(c["name"] for c in CASES), "the golden and CASES list different cases"
    return g["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_path(case, golden):
    got = run_case(case)
    print(case["name"], json.dumps(got, sort_keys=True))
    assert got == golden[case["name"]]


def test_branches_reached(golden):
    """The golden itself shows the branches the cases were chosen for (module docstring)."""
    g = golden
    k = lambda n: (g[n]["kernel"], g[n]["geometry"]["shards"], g[n]["geometry"]["threads"], g[n]["geometry"]["nodes_per_lane"])
    assert k("spread-1000-nps512") == ("k_spread", 2, 512, 1)
    assert k("spread-1000-nps512-threads64") == ("k_spread", 2, 512, 1)
    assert k("c4-20000-nps4096")[:2] == ("k_spread", 28)
    assert k("spread-1000-xcdshards4")[:2] == ("k_spread", 4) and g["spread-1000-xcdshards4"]["xcd_local"]["used"] == 1
    assert k("rack130-3000-shards2")[:2] == ("k_schedule", 1)
    assert k("rack300-1000")[:2] == ("k_schedule", 1)
    assert "topology histograms too large" in g["rack300-20000-refused"]["refused"][1]
    assert k("c1-20000")[:2] == ("k_simple", 128)                      # 64 * SX_CHUNKS
    assert k("c4-20000-shards80")[:2] == ("k_spread", 80)              # W > 64: the two-level exchange area
    assert g["plain-1000-table1-flat1"]["simple_exchange"]["flat"] == 1
    assert g["plain-1000-table1-flat0"]["shape_table"]["shapes"] > 0 and g["plain-1000-table1-flat0"]["simple_exchange"]["flat"] == 0
    assert g["vol-1000-pct100-vol"]["simple_form"]["volumes"] == 1
    assert g["vol-1000-pct50-vol"]["kernel"] == "k_schedule" and g["vol-1000-pct50-vol-win"]["simple_form"]["volumes"] == 1
    assert g["names-1000-pct50"]["kernel"] == "k_schedule" and g["names-1000-pct100"]["kernel"] == "k_simple"
    assert g["nominated-1000-pct100"]["kernel"] == "k_schedule" and g["foo-1000-scored"]["kernel"] == "k_schedule"
    assert g["foo-1000"]["kernel"] == "k_simple"
    # k_spread's ports-and-images form: 8 B more LDS per node slot than the same batch's plain form would take
    on, off = g["spread-pi-1000-pct100-spi1"], g["spread-pi-1000-pct100-spi0"]
    assert on["kernel"] == "k_spread" and on["spread_lds"] > g["spread-1000-pct100"]["spread_lds"] and off["kernel"] == "k_schedule"
    assert g["spread-pi-1000-pct50-spi1"]["kernel"] == "k_spread" and g["spread-pi-1000-spi1-fold"]["kernel"] == "k_schedule"


def record():
    """Write the golden from the loaded library's decisions (KSS_LIB selects it); one line per case."""
    import torch
    torch.zeros(1, device="cuda")  # torch's runtime before libkss.so's (tests/conftest.py)
    out = dict(device=_device(), cases={})
    print("library: KSS_LIB=%s, %s" % (os.environ.get("KSS_LIB", "base"), os.path.basename(native.lib()._name)), flush=True)
    failed = []
    for case in CASES:
        try:
            got = run_case(copy.deepcopy(case))
        except AssertionError:  # a result that differs from the oracle's: reported, nothing is written
            import traceback
            traceback.print_exc()
            failed.append(case["name"])
            continue
        print(case["name"], json.dumps(got, sort_keys=True), flush=True)
        out["cases"][case["name"]] = got
    if failed:
        sys.exit("results differ from the oracle in %s: no golden written" % failed)
    with open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, "w") as f:
        f.write('{"device": %s, "cases": {\n' % json.dumps(out["device"], sort_keys=True))  # one case per line
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in out["cases"].items()))
        f.write("\n}}\n")
    print("recorded %d cases" % len(CASES))


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: test_gpu_path_table.py --record [path]")
    record()
