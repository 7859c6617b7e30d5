"""Operand staging in k_simple's shape-table loop (kss_simple.cuh simple_schedule_tab):
in pod k's exchange window every lane loads the table words and static words of pods k+1 and k+2
on its own slot, and the record fields the pass reads, into registers; once the winner is known its
lane takes the pending table values instead; the owner wave's commit and column copy follow its
next pass B; the prefetch wave loads one window and stores the next.  The cases are the smallest
shapes at which that can go wrong: a winner that is the next pod's candidate, a commit that flips
the next verdict, skipped pods, batches and launches shorter than the prefetch distance, every
wave layout, normalisation maxima that change from pod to pod, the two-level form on a split grid.

Every case runs with flat_exchange 1 and 0 and compares the chosen nodes, the per-pod outcomes
(fetch_meta) and the final node state with the C oracle, computed once per case; each asserts its
own condition on the oracle's output.  Geometries are pinned with shards / force_threads."""
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
FILL_SHAPES = [{}, {"cpu": "2", "memory": "8Gi"}, {"cpu": "4", "memory": "16Gi"}, {"cpu": "500m", "memory": "1Gi"},
               {"cpu": "1"}, {"memory": "4Gi"}]


def _manifests(seed, n_nodes, n_pods, shapes, bound_per_node=(0, 3), cycle=False):
    """progfuzz nodes / bound pods / pending pods without programs (taints, tolerations, node
    selectors and affinity, node names kept), every pending pod's requests from `shapes`: drawn,
    or pod j takes shape j % len(shapes) (cycle)."""
    nodes, bound, pods = progfuzz.make(seed, n_nodes, n_pods, bound_per_node=bound_per_node, extended=False, programs=False)
    r = random.Random(seed * 7919 + 1)
    for j, p in enumerate(pods):
        p["spec"].pop("initContainers", None)
        p["spec"]["containers"][0]["resources"]["requests"].clear()
        p["spec"]["containers"][0]["resources"]["requests"].update(shapes[j % len(shapes) if cycle else r.randrange(len(shapes))])
    return nodes, bound, pods


def _plain(nodes, pods):
    """No taints, selectors, affinity or node names: every static word passes with raw scores 0."""
    for n in nodes:
        n["spec"] = {}
    for p in pods:
        p["spec"] = {"containers": p["spec"]["containers"]}


def _conflict(nodes):
    """Required node affinity no node can satisfy: the NodeAffinity PreFilter fails (status 2)."""
    names = [n["metadata"]["name"] for n in nodes]
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [{"matchFields": [
        {"key": "metadata.name", "operator": "In", "values": [names[0]]},
        {"key": "metadata.name", "operator": "In", "values": [names[1]]}]}]}}}


def _check_meta(ctx, chosen, n_pods, want):
    chosen_o, res, _ = want
    np.testing.assert_array_equal(chosen, chosen_o)
    meta = ctx.fetch_meta(n_pods)
    for j in range(n_pods):
        m = res.meta(j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], j


def _check_state(g, n, st):
    np.testing.assert_array_equal(g["requested"][:, :n], st["requested"][:, :n])
    np.testing.assert_array_equal(g["nonzero"][:, :n], st["nonzero"][:, :n])
    np.testing.assert_array_equal(g["pod_count"][:n], st["pod_count"][:n])


def _run(nodes, bound, pods, shards, threads, extra=None):
    """Both exchange forms of the table loop on `shards` x `threads` lanes against the oracle,
    whose results are returned."""
    assert len(pods) <= 300 and len(nodes) <= 1010
    prof = abi.default_profile()
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    want = oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record="meta",
                             n_classes=len(cc.classes), n_terms=len(cc.terms))
    _, n_shapes = native.plan_shapes(cp.as_struct(), len(cc.scalars))
    assert 1 <= n_shapes <= 64 and not cc.scalars
    entries = shards * (threads // 64)
    for opt in (1, 0):
        native.reset_options()
        native.set_option("shards", shards)
        native.set_option("force_threads", threads)
        for k, v in (extra or {}).items():
            native.set_option(k, v)
        native.set_option("flat_exchange", opt)
        ctx = native.Context(prof)
        ctx.load(cc.as_struct())
        chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
        assert ctx.last_kernel() == "k_simple"
        g = ctx.last_geometry()
        assert (g["shards"], g["threads"]) == (shards, threads), g
        assert ctx.last_shape_table()["shapes"] == n_shapes, ctx.last_shape_table()
        assert ctx.last_simple_exchange() == ({"flat": 1, "entries": entries} if opt else {"flat": 0, "entries": 0})
        _check_meta(ctx, chosen, cp.n, want)
        _check_state(ctx.node_state(), cc.n_nodes, want[2])
        ctx.close()
    native.reset_options()
    return want


def _repeats(chosen):
    ch = np.asarray(chosen)
    return int(((ch[1:] == ch[:-1]) & (ch[1:] >= 0)).sum())


@pytest.mark.parametrize("n_nodes,n_shapes", [(7, 3), (6, 2), (9, 1)])
def test_winner_is_the_next_candidate(n_nodes, n_shapes):
    """3 shards x 2 waves on a few large, empty nodes: a small pod does not move a node's integer
    scores, so consecutive pods win the same node -- the winner's lane needs the pending values of
    both following shapes (or twice the same one) before its wave has copied them into the table."""
    nodes, bound, pods = _manifests(300 + n_nodes, n_nodes, 200, BASE_SHAPES[:n_shapes], bound_per_node=(0, 0), cycle=True)
    _plain(nodes, pods)
    for n in nodes:
        n["status"]["allocatable"].update({"cpu": "64", "memory": "256Gi", "ephemeral-storage": "500Gi", "pods": "110"})
    chosen, _, _ = _run(nodes, bound, pods, 3, 128)
    assert _repeats(chosen) >= 5, "consecutive pods never won the same node"
    assert len(set(np.asarray(chosen))) > 1 and (np.asarray(chosen) >= 0).all()


@pytest.mark.parametrize("shards,threads", [(2, 128), (3, 192)])
def test_commit_flips_the_next_verdict(shards, threads):
    """Nodes that fill within the batch, by resources and by the pods limit (2 - 4 on some): the
    candidate's verdict for the next pod after the commit differs from the one before it, the
    feasible count and the maxima change from pod to pod, and the last pods find nothing."""
    nodes, bound, pods = _manifests(61, 9, 150, FILL_SHAPES, bound_per_node=(0, 0))
    _plain(nodes, pods)
    for i, n in enumerate(nodes):
        cores = [2, 4, 2, 4, 8, 2, 4, 2, 16][i]
        n["status"]["allocatable"].update({"cpu": str(cores), "memory": "%dGi" % (4 * cores),
                                           "pods": str([2, 16, 3, 16, 4, 16, 2, 16, 16][i])})
    _, res, _ = _run(nodes, bound, pods, shards, threads)
    nfe = [res.meta(j)["n_feasible"] for j in range(150)]
    assert nfe[0] >= 8 and min(nfe) == 0 and any(a > b for a, b in zip(nfe, nfe[1:])), nfe
    assert all(res.meta(j)["status"] == 1 and res.meta(j)["chosen"] < 0 for j in range(146, 150)), "the batch does not end unschedulable"
    assert sum(res.meta(j)["chosen"] >= 0 for j in range(150)) > 30


def test_skipped_pods_do_not_leak():
    """PreFilter failures (status 2: the pod publishes zeros and commits nothing) at positions 0, 1,
    two in a row in mid-batch, and the last: their staged operands must not reach their neighbours."""
    n_pods = 90
    nodes, bound, pods = _manifests(62, 140, n_pods, BASE_SHAPES)
    bad = (0, 1, 40, 41, 57, n_pods - 1)
    for j in bad:
        pods[j]["spec"] = {"containers": pods[j]["spec"]["containers"], "affinity": _conflict(nodes)}
    _, res, _ = _run(nodes, bound, pods, 2, 128)
    assert all(res.meta(j)["status"] == 2 and res.meta(j)["chosen"] < 0 for j in bad)
    assert all(res.meta(j)["chosen"] >= 0 for j in (2, 39, 42, 56, 58, n_pods - 2))


@pytest.mark.parametrize("n_pods", [1, 2, 3])
def test_tiny_batches(n_pods):
    """Batches shorter than the prefetch distance: nothing is prefetched, the one staging is the
    prologue's (and, from two pods on, one window's)."""
    nodes, bound, pods = _manifests(63, 130, n_pods, BASE_SHAPES[:3])
    _plain(nodes, pods)
    chosen, _, _ = _run(nodes, bound, pods, 2, 128)
    assert (np.asarray(chosen) >= 0).all()


@pytest.mark.parametrize("launch_pods,n_pods", [(1, 40), (30, 300)])
def test_launch_boundaries(launch_pods, n_pods):
    """static_bytes cuts the batch into launches of 1 pod and of 30 pods: every launch's first
    iteration stages from its prologue's table, built from the state the launch before wrote back."""
    n_nodes = 300
    nodes, bound, pods = _manifests(71, n_nodes, n_pods, BASE_SHAPES)
    chosen, _, _ = _run(nodes, bound, pods, 3, 128, extra={"static_bytes": 4 * n_nodes * launch_pods})
    assert (np.asarray(chosen) >= 0).sum() > n_pods // 2


@pytest.mark.parametrize("n_nodes,shards,threads", [(378, 3, 128), (377, 2, 192), (1008, 2, 512), (9, 2, 192), (3, 3, 192)])
def test_wave_layouts(n_nodes, shards, threads):
    """2 waves (the prefetch wave is wave 1, which also refreshes), 3 waves, 8 waves (the prefetch
    wave is wave 7), 9 nodes on 2 shards x 3 waves (the last shard holds 4 as 2 + 2 + 0: an empty
    last wave), shards of one node (waves 1.. own nothing)."""
    small = n_nodes < 10
    nodes, bound, pods = _manifests(80 + n_nodes, n_nodes, 120 if small else 200, BASE_SHAPES,
                                    bound_per_node=(0, 1) if small else (0, 3))
    if small:
        _plain(nodes, pods)
    chosen, _, _ = _run(nodes, bound, pods, shards, threads)
    ch = np.asarray(chosen)
    if small:
        assert set(ch[ch >= 0]) == set(range(n_nodes)), "some node never won"
    else:
        per = -(-n_nodes // shards)
        assert (ch >= (shards - 1) * per).any() and ((ch >= 0) & (ch < per)).any()


def test_normalisation_maxima_change():
    """PreferNoSchedule taints / tolerations and preferred node affinity kept: the raw
    TaintToleration and NodeAffinity scores of a pod's feasible nodes, so the maxima the exchange
    hands to the next pod, are non-zero and differ between consecutive pods."""
    nodes, bound, pods = _manifests(45, 400, 200, BASE_SHAPES)
    assert sum(any(t["effect"] == "PreferNoSchedule" for t in n["spec"].get("taints", [])) for n in nodes) >= 10
    pref = [bool(p["spec"].get("affinity", {}).get("nodeAffinity", {}).get("preferredDuringSchedulingIgnoredDuringExecution"))
            for p in pods]
    tol = [any(t.get("effect") == "PreferNoSchedule" for t in p["spec"].get("tolerations", [])) for p in pods]
    assert any(a != b for a, b in zip(pref, pref[1:])) and sum(pref) >= 10, "preferred node affinity never changes"
    assert any(a != b for a, b in zip(tol, tol[1:])), "PreferNoSchedule tolerations never change"
    _, res, _ = _run(nodes, bound, pods, 3, 192)
    tot = [res.meta(j)["best_total"] for j in range(200) if res.meta(j)["scored"]]
    assert len(set(tot)) > 5


def test_split_grid_two_level_form():
    """Two in-process parts x 4 shards: the two-level form of the same loop (simple_sync_pw), whatever
    flat_exchange says."""
    prof = abi.default_profile()
    n_nodes, n_pods = 600, 300
    s = native.Synth(2, SEED_BASE + 2, n_nodes, n_pods)
    want = oracle_c.schedule(prof, s.cluster, s.pods, n_pods, n_nodes, record="meta")
    for opt in (1, 0):
        native.reset_options()
        native.set_option("flat_exchange", opt)
        sp = split.InProcessSplit(s.cluster, s.pods, 2, 4)
        outs = sp.run(n_pods)
        for p, (c, ch) in enumerate(zip(sp.ctxs, outs)):
            assert c.last_kernel() == "k_simple"
            assert c.last_shape_table()["shapes"] > 1
            assert c.last_simple_exchange() == {"flat": 0, "entries": 0}, (p, c.last_simple_exchange())
            np.testing.assert_array_equal(ch, want[0], err_msg=f"part {p}")
        _check_meta(sp.ctxs[-1], outs[-1], n_pods, want)
        _check_state(sp.node_state(), n_nodes, want[2])
        sp.close()
    native.reset_options()
    s.close()


def test_library_geometry_config2():
    """Config 2's recipe at 500 nodes x 300 pods on the geometry the library chooses itself (the
    XCD-local grid)."""
    prof = abi.default_profile()
    n_nodes, n_pods = 500, 300
    s = native.Synth(2, SEED_BASE + 2, n_nodes, n_pods)
    want = oracle_c.schedule(prof, s.cluster, s.pods, n_pods, n_nodes, record="meta")
    for opt in (1, 0):
        native.reset_options()
        native.set_option("flat_exchange", opt)
        ctx = native.Context(prof)
        ctx.load(s.cluster)
        ctx.stage(s.pods)
        chosen = ctx.run_staged(n_pods)
        assert ctx.last_kernel() == "k_simple"
        assert ctx.last_shape_table()["shapes"] > 1
        assert ctx.last_simple_exchange()["flat"] == opt
        _check_meta(ctx, chosen, n_pods, want)
        _check_state(ctx.node_state(), n_nodes, want[2])
        ctx.close()
    native.reset_options()
    s.close()
