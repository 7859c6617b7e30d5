"""k_simple's shape table (kss_simple.cuh simple_schedule_tab): a default-profile
batch of few resource shapes keeps the state-dependent filter verdict and scores of every
(shape, node) in LDS, a pod reads them, and per pod only the candidates' rows are re-evaluated.

Every case runs with option shape_table 1 and 0, asserts through last_shape_table() that the
table ran (or did not) as intended, and compares the chosen nodes, the per-pod outcomes
(fetch_meta) and the final node state with the C oracle, computed once per case.  The
geometries (shards / force_threads options) are chosen so that the per-wave split is known:
a shard's `own` nodes over n waves, ceil(own / n) slots per wave.

Reference semantics: NodeResourcesFit fitsRequest and the LeastAllocated / BalancedAllocation
scorers as the oracle states them (oracle/kss_oracle.c)."""
import random

import numpy as np
import pytest

import oracle_c
import progfuzz
from kss import abi, native, split
from kss.compile import compile_cluster
from kss.synth import SEED_BASE

pytestmark = pytest.mark.gpu

BASE_SHAPES = [{"cpu": "100m", "memory": "128Mi"}, {"cpu": "250m", "memory": "512Mi"},
               {"cpu": "500m", "memory": "256Mi", "ephemeral-storage": "256Mi"}, {}]


def _manifests(seed, n_nodes, n_pods, shapes, bound_per_node=(0, 3), extended=False):
    """progfuzz nodes / bound pods / pending pods without programs (static filters and scores kept:
    taints, tolerations, node selectors and affinity, node names), every pending pod's requests
    drawn from `shapes`."""
    nodes, bound, pods = progfuzz.make(seed, n_nodes, n_pods, bound_per_node=bound_per_node, extended=extended,
                                       programs=False)
    r = random.Random(seed * 7919 + 1)
    for p in pods:
        p["spec"].pop("initContainers", None)
        p["spec"]["containers"][0]["resources"]["requests"].clear()
        p["spec"]["containers"][0]["resources"]["requests"].update(shapes[r.randrange(len(shapes))])
    return nodes, bound, pods


def _rounds(threads, shapes):
    nwave = threads // 64
    return -(-nwave * shapes // (64 * (nwave - 1)))


def _check(ctx, chosen, cc, n_pods, want):
    chosen_o, res, st = want
    np.testing.assert_array_equal(chosen, chosen_o)
    meta = ctx.fetch_meta(n_pods)
    for j in range(n_pods):
        m = res.meta(j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], j
    g, n = ctx.node_state(), cc.n_nodes
    np.testing.assert_array_equal(g["requested"][:, :n], st["requested"][:, :n])
    np.testing.assert_array_equal(g["nonzero"][:, :n], st["nonzero"][:, :n])
    np.testing.assert_array_equal(g["pod_count"][:n], st["pod_count"][:n])


def _run(nodes, bound, pods, opts, expect_shapes, prof=None, threads=None, kernel="k_simple", on=1):
    """expect_shapes: the table's shape count with shape_table `on` (0: the batch must not take it).
    on: 1, the default, takes the table on grids of two or more shards; 2 also on one shard.
    Returns the oracle's results."""
    prof = prof or abi.default_profile()
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    want = oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record="meta",
                             n_classes=len(cc.classes), n_terms=len(cc.terms))
    _, n_shapes = native.plan_shapes(cp.as_struct(), len(cc.scalars))
    for table in (on, 0):
        native.reset_options()
        for k, v in opts.items():
            native.set_option(k, v)
        native.set_option("shape_table", table)
        ctx = native.Context(prof)
        ctx.load(cc.as_struct())
        chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
        if kernel:
            assert ctx.last_kernel() == kernel
        for k in ("shards",):
            if k in opts:
                assert ctx.last_geometry()["shards"] == opts[k]
        got = ctx.last_shape_table()
        if table and expect_shapes:
            assert n_shapes == expect_shapes
            t = threads or opts["force_threads"]
            assert ctx.last_geometry()["threads"] == t
            assert got == {"shapes": expect_shapes, "rounds": _rounds(t, expect_shapes)}, got
        else:
            assert got == {"shapes": 0, "rounds": 0}, (table, got)
        _check(ctx, chosen, cc, cp.n, want)
        ctx.close()
    return want


def test_repeated_winner_on_filling_nodes():
    """3 nodes on one shard of two waves (slots 0, 1 on wave 0, slot 2 on wave 1), 300 pods of 4
    shapes: the same node wins pod after pod (its pending row goes into the table and is read by
    the next pod), the nodes fill up (the H1 verdict of the candidate flips) until the last pods
    find no feasible node.  One shard: no exchange hides the refresh, so the default (shape_table 1)
    leaves such a grid on today's kernel (asserted) and shape_table 2 asks for the table."""
    nodes, bound, pods = _manifests(31, 3, 300, BASE_SHAPES, bound_per_node=(0, 1))
    for n in nodes:  # every node schedulable, small, so that the batch fills them
        n["spec"] = {}
        n["status"]["allocatable"].update({"cpu": "8", "memory": "32Gi", "ephemeral-storage": "50Gi", "pods": "110"})
    for p in pods:  # every pod passes the static filters everywhere
        p["spec"] = {"containers": p["spec"]["containers"]}
    _, res, _ = _run(nodes, bound, pods, {"shards": 1, "force_threads": 128}, 4, on=2)
    _run(nodes[:3], bound, pods[:40], {"shards": 1, "force_threads": 128}, 0, on=1)
    chosen = [res.meta(j)["chosen"] for j in range(300)]
    assert any(a == b and a >= 0 for a, b in zip(chosen, chosen[1:])), "no consecutive wins on one node"
    assert res.meta(299)["n_feasible"] == 0 and res.meta(0)["n_feasible"] == 3
    assert any(0 < res.meta(j)["n_feasible"] < 3 for j in range(300))


@pytest.mark.parametrize("nwave", [2, 3, 8])
@pytest.mark.parametrize("own", ["1", "2", "full", "full-1"])
def test_slots_at_the_wave_boundaries(nwave, own):
    """Shards of 1, 2, 63 x waves and 63 x waves - 1 nodes: empty waves, one full wave after the
    other, a candidate in the last (the prefetch) wave; three shards, the last one a node short."""
    per = {"1": 1, "2": 2, "full": 63 * nwave, "full-1": 63 * nwave - 1}[own]
    n_nodes = 3 * per - (1 if per > 1 else 0)
    nodes, bound, pods = _manifests(40 + nwave, n_nodes, 200, BASE_SHAPES)
    _run(nodes, bound, pods, {"shards": 3, "force_threads": 64 * nwave}, 4)


@pytest.mark.parametrize("nwave,n_shapes,rounds", [(2, 40, 2), (3, 64, 2), (2, 65, 0)])
def test_refresh_rounds_and_the_shape_limit(nwave, n_shapes, rounds):
    """40 shapes on two waves are 80 evaluations for the 64 lanes of the one idle wave: two rounds;
    64 shapes on three waves: 192 on 128 lanes; 65 shapes: today's kernel."""
    shapes = [{"cpu": "%dm" % (50 + 10 * i), "memory": "%dMi" % (64 + 8 * (i % 7))} for i in range(n_shapes)]
    nodes, bound, pods = _manifests(50 + n_shapes, 200, 300, shapes)
    if rounds:
        assert _rounds(64 * nwave, n_shapes) == rounds
    _run(nodes, bound, pods, {"shards": 2, "force_threads": 64 * nwave}, n_shapes if rounds else 0)


def test_shape_edge_values():
    """The all-zero-request pod; pods whose PreFilter fails in mid-batch (no commit, no refresh);
    nodes without allocatable cpu or memory; pods that ask for exactly what an empty node has."""
    shapes = [{}, {"cpu": "2", "memory": "8Gi"}, {"cpu": "4", "memory": "16Gi"}, {"cpu": "500m", "memory": "1Gi"},
              {"cpu": "1"}, {"memory": "4Gi"}]
    nodes, bound, pods = _manifests(61, 9, 120, shapes, bound_per_node=(0, 0))
    for i, n in enumerate(nodes):
        n["spec"] = {}
        cores = [2, 4, 2, 4, 8, 2, 4, 2, 16][i]
        n["status"]["allocatable"].update({"cpu": str(cores), "memory": "%dGi" % (4 * cores), "pods": "16"})
    nodes[2]["status"]["allocatable"]["cpu"] = "0"
    nodes[3]["status"]["allocatable"]["memory"] = "0"
    names = [n["metadata"]["name"] for n in nodes]
    conflict = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [{"matchFields": [
        {"key": "metadata.name", "operator": "In", "values": [names[0]]},
        {"key": "metadata.name", "operator": "In", "values": [names[1]]}]}]}}}
    for j, p in enumerate(pods):
        p["spec"] = {"containers": p["spec"]["containers"]}
        if j in (5, 6, 40):
            p["spec"]["affinity"] = conflict
    _, res, _ = _run(nodes, bound, pods, {"shards": 2, "force_threads": 128}, len(shapes))
    assert all(res.meta(j)["status"] == 2 and res.meta(j)["chosen"] < 0 for j in (5, 6, 40))
    assert any(res.meta(j)["chosen"] >= 0 for j in range(120)) and res.meta(119)["n_feasible"] < 9


def test_table_rebuilt_at_every_launch():
    """static_bytes forces ten launches of 40 pods: each rebuilds the table from the node state
    the launch before it wrote back."""
    n_nodes, n_pods = 300, 400
    nodes, bound, pods = _manifests(71, n_nodes, n_pods, BASE_SHAPES)
    _run(nodes, bound, pods, {"shards": 3, "force_threads": 128, "static_bytes": 4 * n_nodes * 40}, 4)


def _synth_check(ctx, chosen, s, n_pods, want):
    chosen_o, res, st = want
    np.testing.assert_array_equal(chosen, chosen_o)
    meta = ctx.fetch_meta(n_pods)
    for j in range(n_pods):
        m = res.meta(j)
        assert (meta[j, 0], meta[j, 1], meta[j, 2], meta[j, 3]) == (m["chosen"], m["n_feasible"], m["scored"],
                                                                    m["status"]), j
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], j


@pytest.mark.parametrize("mode", ["forced_fallback", "xcd_off"])
def test_placement_fallback_and_off(mode):
    """Config 2's recipe, 500 nodes x 300 pods, on an XCD-local launch that reports failed placement
    (the unrestricted rerun schedules the batch) and with XCD-local grids off."""
    prof = abi.default_profile()
    n_nodes, n_pods = 500, 300
    s = native.Synth(2, SEED_BASE + 2, n_nodes, n_pods)
    want = oracle_c.schedule(prof, s.cluster, s.pods, n_pods, n_nodes, record="meta")
    _, n_shapes = native.plan_shapes(s.pods)
    assert 1 < n_shapes <= 64
    for table in (1, 0):
        native.reset_options()
        native.set_option("xcd_force_fallback" if mode == "forced_fallback" else "xcd", 1 if mode == "forced_fallback" else 0)
        native.set_option("shape_table", table)
        ctx = native.Context(prof)
        ctx.load(s.cluster)
        ctx.stage(s.pods)
        chosen = ctx.run_staged(n_pods)
        assert ctx.last_kernel() == "k_simple"
        xl = ctx.last_xcd_local()
        assert xl == ({"used": 1, "fallbacks": 1} if mode == "forced_fallback" else {"used": 0, "fallbacks": 0}), xl
        got = ctx.last_shape_table()
        assert got["shapes"] == (n_shapes if table else 0), got
        _synth_check(ctx, chosen, s, n_pods, want)
        g = ctx.node_state()
        np.testing.assert_array_equal(g["requested"][:, :n_nodes], want[2]["requested"][:, :n_nodes])
        np.testing.assert_array_equal(g["nonzero"][:, :n_nodes], want[2]["nonzero"][:, :n_nodes])
        np.testing.assert_array_equal(g["pod_count"][:n_nodes], want[2]["pod_count"][:n_nodes])
        ctx.close()
    s.close()


def test_split_grid_two_parts():
    """Two in-process parts of one grid (the table is shard-local): config 2's recipe, 600 nodes x
    300 pods, 2 x 4 shards of 75 nodes on two waves."""
    prof = abi.default_profile()
    n_nodes, n_pods = 600, 300
    s = native.Synth(2, SEED_BASE + 2, n_nodes, n_pods)
    want = oracle_c.schedule(prof, s.cluster, s.pods, n_pods, n_nodes, record="meta")
    _, n_shapes = native.plan_shapes(s.pods)
    for table in (1, 0):
        native.reset_options()
        native.set_option("shape_table", table)
        sp = split.InProcessSplit(s.cluster, s.pods, 2, 4)
        outs = sp.run(n_pods)
        for p, (c, ch) in enumerate(zip(sp.ctxs, outs)):
            assert c.last_kernel() == "k_simple"
            assert c.last_geometry()["shards"] == 8
            assert c.last_shape_table()["shapes"] == (n_shapes if table else 0), (p, c.last_shape_table())
            np.testing.assert_array_equal(ch, want[0], err_msg=f"part {p}")
        _synth_check(sp.ctxs[-1], outs[-1], s, n_pods, want)
        g = sp.node_state()
        np.testing.assert_array_equal(g["requested"][:, :n_nodes], want[2]["requested"][:, :n_nodes])
        np.testing.assert_array_equal(g["nonzero"][:, :n_nodes], want[2]["nonzero"][:, :n_nodes])
        np.testing.assert_array_equal(g["pod_count"][:n_nodes], want[2]["pod_count"][:n_nodes])
        sp.close()
    s.close()


def _custom_profile():
    prof = abi.default_profile()
    prof.fit_strategy = abi.KSS_FIT_MOST_ALLOCATED
    prof.fit_weight[0], prof.fit_weight[1] = 3, 2
    prof.weight[abi.KSS_S_BALANCED_ALLOCATION] = 4
    return prof


@pytest.mark.parametrize("why", ["extended_resource", "pct_30", "custom_profile"])
def test_batches_that_do_not_take_the_table(why):
    """A cluster with an extended resource, percentageOfNodesToScore 30 (the window) and a custom
    profile run today's kernels: 0 shapes reported, results equal to the oracle."""
    prof = abi.default_profile()
    if why == "extended_resource":
        nodes, bound, pods = progfuzz.make(81, 300, 200, n_extended=1, programs=False)
    else:
        nodes, bound, pods = _manifests(82, 300, 200, BASE_SHAPES)
    if why == "pct_30":
        prof.pct_nodes_to_score = 30
    if why == "custom_profile":
        prof = _custom_profile()
    _run(nodes, bound, pods, {"shards": 3, "force_threads": 128}, 0, prof=prof, kernel=None)


# The loop variants of kss_simple.cuh at their smallest shapes.  k_simple picks per-wave mode by its
# own rule, per <= 63 x waves (per: the nodes of a full shard); the geometry options pin shards and
# lanes, so the rule places each case.  (nodes, shards, pods, profile, pct, extended resources,
# shape_table option, loop)
VARIANTS = {
    "per_wave_full_waves": (378, 3, 200, "default", 100, 0, 0, "per-wave"),
    "per_wave_short_last_shard": (377, 3, 200, "custom", 100, 1, 0, "per-wave"),
    "per_wave_window": (378, 3, 200, "default", 30, 0, 0, "per-wave"),
    "two_reduction_default": (127, 1, 200, "default", 100, 1, 0, "two-reduction"),
    "two_reduction_custom": (127, 1, 200, "custom", 100, 1, 0, "two-reduction"),
    "two_reduction_window": (127, 1, 200, "default", 30, 0, 0, "two-reduction"),
    "table": (378, 3, 200, "default", 100, 0, 1, "table"),
    "table_one_pod": (378, 3, 1, "default", 100, 0, 1, "table"),
    "table_three_pods": (378, 3, 3, "default", 100, 0, 1, "table"),
}


@pytest.mark.parametrize("case", sorted(VARIANTS))
def test_loop_variants_at_their_smallest_shapes(case):
    """simple_schedule in per-wave mode (two waves of 63 slots each: 126 nodes per shard, the last
    shard full or one node short), its two-reduction form (127 nodes on one shard of 128 lanes, one
    node past per-wave mode's limit), both with the window (pct 30: numFeasibleNodesToFind is 113 of
    378 nodes and the 100-node floor of 127, so the window cuts), with an extended resource and a custom
    profile, and simple_schedule_tab, also on batches of one pod (the prologue and one iteration)
    and of three (the prefetch distance: nothing is prefetched).  Chosen nodes, per-pod outcomes and
    the final node state against the C oracle; the routing through last_kernel, last_geometry,
    last_shape_table and the kernel's rule for per-wave mode."""
    n_nodes, shards, n_pods, profile, pct, n_ext, table, loop = VARIANTS[case]
    if n_ext:
        nodes, bound, pods = progfuzz.make(90 + n_nodes, n_nodes, n_pods, n_extended=n_ext, programs=False)
    else:
        nodes, bound, pods = _manifests(90 + n_nodes, n_nodes, n_pods, BASE_SHAPES)
    prof = _custom_profile() if profile == "custom" else abi.default_profile()
    prof.pct_nodes_to_score = pct
    if pct < 100:  # k_simple runs the window for pods without a PreFilterResult node list (metadata.name terms)
        for p in pods:
            na = p["spec"].get("affinity", {}).get("nodeAffinity", {})
            req = na.get("requiredDuringSchedulingIgnoredDuringExecution", {})
            if any("matchFields" in t for t in req.get("nodeSelectorTerms", [])):
                del na["requiredDuringSchedulingIgnoredDuringExecution"]
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    assert len(cc.scalars) == n_ext
    want = oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record="meta",
                             n_classes=len(cc.classes), n_terms=len(cc.terms))
    if pct < 100:  # the window cuts: pods keep exactly numFeasibleNodesToFind nodes of more, none keeps more
        k_find = max(100, n_nodes * pct // 100)  # 100 (the floor) of 127 nodes, 113 of 378
        kept = [want[1].meta(j)["n_feasible"] for j in range(n_pods)]
        assert k_find < n_nodes and max(kept) == k_find and kept.count(k_find) > 1
    _, n_shapes = native.plan_shapes(cp.as_struct(), n_ext)
    native.reset_options()
    native.set_option("shards", shards)
    native.set_option("force_threads", 128)
    native.set_option("shape_table", table)
    ctx = native.Context(prof)
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
    assert ctx.last_kernel() == "k_simple"
    g = ctx.last_geometry()
    assert (g["shards"], g["threads"]) == (shards, 128), g
    per = -(-n_nodes // shards)
    assert (per <= 63 * (g["threads"] // 64)) == (loop != "two-reduction")
    if loop == "table":
        assert 1 <= n_shapes <= 64
        assert ctx.last_shape_table() == {"shapes": n_shapes, "rounds": _rounds(128, n_shapes)}
    else:
        assert ctx.last_shape_table() == {"shapes": 0, "rounds": 0}
    _check(ctx, chosen, cc, cp.n, want)
    ctx.close()
