"""The flat exchange of k_simple's shape-table loop (kss_simple.cuh simple_sync_flat):
every wave of every shard publishes its own best key and statistics (4 granules per entry,
entry = shard x waves + wave) and wave 0 of each shard reduces all shards x waves entries in one
sweep: "the winner's wave contributes H1, every other wave H0".  The two-level form (a reduction
inside the shard, then one over the shards) stays for one shard, split grids and more than 128
entries, and behind option flat_exchange = 0.

Every case runs with flat_exchange 1 and 0, asserts the routing through last_simple_exchange()
and last_shape_table(), and compares the chosen nodes, the per-pod outcomes (fetch_meta) and the
final node state with the C oracle, computed once per case.  Geometries are pinned with the
shards / force_threads options (a pinned shard count runs on an unrestricted grid; the XCD-local
grid is the library's own choice in test_xcd_local_placement_fallback_and_off): a shard's `own`
nodes over n waves, ceil(own / n) slots per wave, so node -> entry is known in each case."""
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


def _manifests(seed, n_nodes, n_pods, shapes, bound_per_node=(0, 3)):
    """progfuzz nodes / bound pods / pending pods without programs (taints, tolerations, node
    selectors and affinity, node names kept), every pending pod's requests drawn from `shapes`."""
    nodes, bound, pods = progfuzz.make(seed, n_nodes, n_pods, bound_per_node=bound_per_node, extended=False, programs=False)
    r = random.Random(seed * 7919 + 1)
    for p in pods:
        p["spec"].pop("initContainers", None)
        p["spec"]["containers"][0]["resources"]["requests"].clear()
        p["spec"]["containers"][0]["resources"]["requests"].update(shapes[r.randrange(len(shapes))])
    return nodes, bound, pods


def _rounds(threads, shapes):
    nwave = threads // 64
    return -(-nwave * shapes // (64 * (nwave - 1)))


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


def _run(nodes, bound, pods, shards, threads, flat=True, extra=None):
    """Both exchange forms on `shards` x `threads` lanes.  flat: whether flat_exchange 1 must take
    the flat form on this geometry.  Returns the oracle's results."""
    prof = abi.default_profile()
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    want = oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record="meta",
                             n_classes=len(cc.classes), n_terms=len(cc.terms))
    _, n_shapes = native.plan_shapes(cp.as_struct(), len(cc.scalars))
    assert 1 <= n_shapes <= 64 and not cc.scalars
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
        assert ctx.last_shape_table() == {"shapes": n_shapes, "rounds": _rounds(threads, n_shapes)}
        entries = shards * (threads // 64)
        assert ctx.last_simple_exchange() == ({"flat": 1, "entries": entries} if opt and flat else
                                              {"flat": 0, "entries": 0}), (opt, ctx.last_simple_exchange())
        _check_meta(ctx, chosen, cp.n, want)
        _check_state(ctx.node_state(), cc.n_nodes, want[2])
        ctx.close()
    native.reset_options()
    return want


@pytest.mark.parametrize("n_nodes", [378, 377])
def test_three_shards_two_waves(n_nodes):
    """126 nodes per shard on two waves of 63 slots; with 377 nodes the last shard holds 125 as
    63 + 62 (entry 5 = nodes 315 .. 376) and pods win there: the winner's entry is the last one."""
    nodes, bound, pods = _manifests(90 + n_nodes, n_nodes, 200, BASE_SHAPES)
    chosen, _, _ = _run(nodes, bound, pods, 3, 128)
    assert (np.asarray(chosen) >= 315).any(), "no winner in the last wave of the last shard"
    assert ((np.asarray(chosen) >= 0) & (np.asarray(chosen) < 63)).any(), "no winner in the first wave"


def test_fewer_granules_than_lanes():
    """3 shards x 3 waves: 9 entries, 36 granules -- one sweep load, lanes 36 .. 63 past the end."""
    nodes, bound, pods = _manifests(41, 3 * 63 * 3, 200, BASE_SHAPES)
    _run(nodes, bound, pods, 3, 192)


def test_entries_not_a_multiple_of_sixteen():
    """5 shards x 3 waves of 63 nodes: 15 entries, a sweep load covers 16."""
    nodes, bound, pods = _manifests(42, 5 * 63 * 3, 200, BASE_SHAPES)
    chosen, _, _ = _run(nodes, bound, pods, 5, 192)
    assert (np.asarray(chosen) >= 4 * 189 + 126).any(), "no winner in entry 14"


def test_empty_waves_publish_zeros():
    """3 shards of one node on 3 waves: waves 1 and 2 of every shard own no slot and publish zeros."""
    nodes, bound, pods = _manifests(43, 3, 120, BASE_SHAPES, bound_per_node=(0, 1))
    for n in nodes:
        n["spec"] = {}
    for p in pods:
        p["spec"] = {"containers": p["spec"]["containers"]}
    chosen, _, _ = _run(nodes, bound, pods, 3, 192)
    assert set(np.asarray(chosen)[np.asarray(chosen) >= 0]) == {0, 1, 2}


@pytest.mark.parametrize("shards,flat", [(64, True), (65, False)])
def test_at_and_past_the_entry_limit(shards, flat):
    """64 shards x 2 waves = 128 entries, 512 granules, eight sweep loads per lane: the flat form;
    65 shards x 2 waves = 130 entries: the two-level form.  Two nodes per shard, one per wave, on an
    unrestricted grid (more shards than an XCD has CUs)."""
    nodes, bound, pods = _manifests(44 + shards, 2 * shards, 200, BASE_SHAPES)
    chosen, _, _ = _run(nodes, bound, pods, shards, 128, flat=flat, extra={"xcd": 0})
    assert (np.asarray(chosen) >= 2 * shards - 8).any() and (np.asarray(chosen) >= 0).sum() > 100


def test_eight_waves():
    """2 shards x 504 nodes on 8 waves of 63 slots: 16 entries, the prefetch wave is wave 7."""
    nodes, bound, pods = _manifests(45, 1008, 200, BASE_SHAPES)
    _run(nodes, bound, pods, 2, 512)


def test_no_feasible_node_and_prefilter_failures():
    """Nodes fill until pods find nothing feasible (every entry carries key 0: no wave contributes
    H1) and pods whose PreFilter fails in mid-batch publish zeros, on 2 shards x 2 waves."""
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
    _, res, _ = _run(nodes, bound, pods, 2, 128)
    assert all(res.meta(j)["status"] == 2 and res.meta(j)["chosen"] < 0 for j in (5, 6, 40))
    assert any(res.meta(j)["chosen"] >= 0 for j in range(120))
    assert any(res.meta(j)["status"] == 1 and res.meta(j)["n_feasible"] == 0 for j in range(120)), "no pod found nothing"


def test_ten_launches():
    """static_bytes forces ten launches of 30 pods: every launch restarts the epochs on the zeroed
    flat region (2 x 6 entries x 4 granules and the counters behind it)."""
    n_nodes, n_pods = 300, 300
    nodes, bound, pods = _manifests(71, n_nodes, n_pods, BASE_SHAPES)
    _run(nodes, bound, pods, 3, 128, extra={"static_bytes": 4 * n_nodes * 30})


@pytest.mark.parametrize("mode", ["xcd_local", "forced_fallback", "xcd_off"])
def test_xcd_local_placement_fallback_and_off(mode):
    """Config 2's recipe, 500 nodes x 300 pods, the library's own geometry: an XCD-local grid (plain
    stores into that XCD's L2; the claim counters lie behind the flat region), an XCD-local launch
    that reports failed placement (the buffer is zeroed again and the unrestricted rerun schedules
    the batch through agent-scope publishes) and XCD-local grids off."""
    prof = abi.default_profile()
    n_nodes, n_pods = 500, 300
    s = native.Synth(2, SEED_BASE + 2, n_nodes, n_pods)
    want = oracle_c.schedule(prof, s.cluster, s.pods, n_pods, n_nodes, record="meta")
    _, n_shapes = native.plan_shapes(s.pods)
    assert 1 < n_shapes <= 64
    for opt in (1, 0):
        native.reset_options()
        if mode != "xcd_local":
            native.set_option("xcd_force_fallback" if mode == "forced_fallback" else "xcd", 1 if mode == "forced_fallback" else 0)
        native.set_option("flat_exchange", opt)
        ctx = native.Context(prof)
        ctx.load(s.cluster)
        ctx.stage(s.pods)
        chosen = ctx.run_staged(n_pods)
        assert ctx.last_kernel() == "k_simple"
        xl = ctx.last_xcd_local()
        if mode == "xcd_local":  # (a placement that fails by itself falls back: correct either way)
            assert xl["used"] == 1, xl
        else:
            assert xl == ({"used": 1, "fallbacks": 1} if mode == "forced_fallback" else {"used": 0, "fallbacks": 0}), xl
        assert ctx.last_shape_table()["shapes"] == n_shapes
        g = ctx.last_geometry()
        assert g["shards"] > 1
        entries = g["shards"] * (g["threads"] // 64)
        assert entries <= 128
        assert ctx.last_simple_exchange() == ({"flat": 1, "entries": entries} if opt else {"flat": 0, "entries": 0})
        _check_meta(ctx, chosen, n_pods, want)
        _check_state(ctx.node_state(), n_nodes, want[2])
        ctx.close()
    native.reset_options()
    s.close()


def test_split_grid_stays_two_level():
    """Two in-process parts of one grid (2 x 4 shards of 75 nodes on two waves): a part's peers
    exchange per shard, so the table loop keeps the two-level form whatever flat_exchange says."""
    prof = abi.default_profile()
    n_nodes, n_pods = 600, 300
    s = native.Synth(2, SEED_BASE + 2, n_nodes, n_pods)
    want = oracle_c.schedule(prof, s.cluster, s.pods, n_pods, n_nodes, record="meta")
    _, n_shapes = native.plan_shapes(s.pods)
    for opt in (1, 0):
        native.reset_options()
        native.set_option("flat_exchange", opt)
        sp = split.InProcessSplit(s.cluster, s.pods, 2, 4)
        outs = sp.run(n_pods)
        for p, (c, ch) in enumerate(zip(sp.ctxs, outs)):
            assert c.last_kernel() == "k_simple"
            assert c.last_geometry()["shards"] == 8
            assert c.last_shape_table()["shapes"] == n_shapes, (p, c.last_shape_table())
            assert c.last_simple_exchange() == {"flat": 0, "entries": 0}, (p, c.last_simple_exchange())
            np.testing.assert_array_equal(ch, want[0], err_msg=f"part {p}")
        _check_meta(sp.ctxs[-1], outs[-1], n_pods, want)
        _check_state(sp.node_state(), n_nodes, want[2])
        sp.close()
    native.reset_options()
    s.close()
