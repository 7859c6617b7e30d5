"""The shape-table loop for image-only batches (options simple_ports_images + table_images:
k_static_pi's words, k_simple_tab_pi / k_simple_tab_flat_pi) against the C oracle, bit
for bit: chosen nodes, every pod's outcome including best_total, the final node rows, and the
UsedPorts column, which the form neither reads nor writes.

ImageLocality is in the static word and has no NormalizeScore; the loop adds il x weight to the key
and masks the NodeAffinity field to the form's 13 bits.  A loop that ignored either would still
fill nodes plausibly, so every case first asserts on the oracle's own records that ImageLocality
decides choices (the pod's node is not the argmax of total - ImageLocality), that no pod holds a
host port and that the shapes fit the table.  Every case runs with flat_exchange 1 and 0 and asserts
the routing through last_shape_table() and last_simple_exchange().  Batches are
tests/imagetable_fuzz.py's, each computed once; geometries are pinned as in
tests/test_gpu_flat_exchange.py."""
import numpy as np
import pytest

import imagetable_fuzz as itf
import portimage_fuzz
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu
MI = 1024 * 1024


def _rounds(threads, shapes):
    nwave = threads // 64
    return -(-nwave * shapes // (64 * (nwave - 1)))


def _meta_equal(meta, res, n):
    for j in range(n):
        m = res.meta(j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], j


def _check(ctx, chosen, cc, cp, ch_o, res, st):
    N = cc.n_nodes
    np.testing.assert_array_equal(chosen, ch_o)
    _meta_equal(ctx.fetch_meta(cp.n), res, cp.n)
    g = ctx.node_state()
    np.testing.assert_array_equal(g["requested"][:, :N], st["requested"][:, :N])
    np.testing.assert_array_equal(g["nonzero"][:, :N], st["nonzero"][:, :N])
    np.testing.assert_array_equal(g["pod_count"][:N], st["pod_count"][:N])
    # the port column: what was loaded (no pod adds a port; the loop does not touch it)
    np.testing.assert_array_equal(st["port_used"][:N], cc.arrays["port_used"][:N])
    np.testing.assert_array_equal(ctx.port_state(), cc.arrays["port_used"][:N])


def _reach(cc, cp, res, il_min):
    """The oracle's own records: no host-port pod, 1..64 shapes, ImageLocality decides."""
    assert itf.host_port_pods(cp) == 0 and not cc.scalars
    native.set_option("simple_ports_images", 1)
    _, n_shapes = native.plan_shapes(cp.as_struct(), 0)
    assert 1 <= n_shapes <= 64, n_shapes
    il = itf.il_decides(cc, cp, res)
    print("ImageLocality decides", il, "of", cp.n, "shapes", n_shapes)
    assert il >= il_min, il
    return n_shapes


def _run(case, shards, threads, il_min=100, extra=None, flat=True, pin=True):
    """The table form on `shards` x `threads` lanes with both exchange forms.  Returns (launches,
    geometry, XCD-local report) of the last run."""
    cc, cp, ch_o, res, st = case
    native.reset_options()
    n_shapes = _reach(cc, cp, res, il_min)
    out = None
    for opt in (1, 0):
        native.reset_options()
        native.set_option("simple_ports_images", 1)
        native.set_option("table_images", 1)
        if pin:
            native.set_option("shards", shards)
            native.set_option("force_threads", threads)
        for k, v in (extra or {}).items():
            native.set_option(k, v)
        native.set_option("flat_exchange", opt)
        ctx = native.Context(abi.default_profile())
        ctx.load(cc.as_struct())
        chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
        assert ctx.last_kernel() == "k_simple"
        g = ctx.last_geometry()
        if pin:
            assert (g["shards"], g["threads"]) == (shards, threads), g
        assert g["shards"] > 1
        assert ctx.last_shape_table() == {"shapes": n_shapes, "rounds": _rounds(g["threads"], n_shapes)}
        entries = g["shards"] * (g["threads"] // 64)
        assert entries <= 128
        assert ctx.last_simple_exchange() == ({"flat": 1, "entries": entries} if opt and flat else
                                              {"flat": 0, "entries": 0}), (opt, ctx.last_simple_exchange())
        _check(ctx, chosen, cc, cp, ch_o, res, st)
        out = (ctx.last_timing()[1], g, ctx.last_xcd_local())
        ctx.close()
    native.reset_options()
    return out


# --------------------------------------------------------------------------------------
# 1 - 4. geometries (tests/test_gpu_flat_exchange.py's)
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes", [378, 377])
def test_three_shards_two_waves(n_nodes):
    """126 nodes per shard on two waves of 63 slots; with 377 nodes the last shard holds 125 as
    63 + 62.  Pods win in the last wave of the last shard (entry 5) and in the first wave."""
    case = itf.case(90 + n_nodes, n_nodes, 200)
    ch_o = np.asarray(case[2])
    assert (ch_o >= 315).any(), "no winner in the last wave of the last shard"
    assert ((ch_o >= 0) & (ch_o < 63)).any(), "no winner in the first wave"
    _run(case, 3, 128)


def test_fewer_granules_than_lanes():
    """3 shards x 3 waves on 567 nodes: 9 entries, 36 granules, fewer than a wave's lanes."""
    _run(itf.case(41, 567, 200), 3, 192)


def test_eight_waves():
    """2 shards x 504 nodes on 8 waves of 63 slots: the prefetch wave is wave 7."""
    _run(itf.case(45, 1008, 200), 2, 512)


def test_empty_waves_and_pods_without_image_rows():
    """3 shards of one node on 3 waves: waves 1 and 2 of every shard own no slot.  Some pods name an
    image a node lists (image rows, ImageLocality scores) and some name none that any node lists (no
    rows: ImageLocality 0 everywhere) in one batch; the three nodes fill and later pods find nothing."""
    case = itf.case(43, 3, 120, bound_per_node=(0, 1))
    cc, cp, ch_o, res, st = case
    with_rows = sum(int(cp.pods[i]["img_len"] > 0) for i in range(cp.n))
    assert 0 < with_rows < cp.n, with_rows
    assert sum(int(res.meta(j)["chosen"] < 0) for j in range(cp.n)) >= 1
    _run(case, 3, 192, il_min=1)


# --------------------------------------------------------------------------------------
# 5. chunked: the table is rebuilt from PI words on every launch
# --------------------------------------------------------------------------------------
def test_chunked_launches():
    case = itf.case(46, 130, 200)
    launches, _, _ = _run(case, 2, 128, extra={"static_bytes": 4 * case[0].n_nodes * 60})
    assert launches >= 2 * 3, launches  # k_static_pi + the loop kernel per chunk, at least 3 chunks


# --------------------------------------------------------------------------------------
# 6. word edges, hand-derived
# --------------------------------------------------------------------------------------
def _node(name, images=None):
    st = {"allocatable": {"cpu": "4", "memory": "8Gi", "pods": "20", "ephemeral-storage": "20Gi"}}
    if images:
        st["images"] = images
    return {"metadata": {"name": name, "labels": {"kubernetes.io/hostname": name}}, "spec": {}, "status": st}


def _pod(name, image, prefer=None):
    spec = {"containers": [{"name": "c", "image": image, "resources": {"requests": {"cpu": "500m", "memory": "1Gi"}}}]}
    if prefer:
        pref = {"matchExpressions": [{"key": "kubernetes.io/hostname", "operator": "In", "values": [prefer]}]}
        spec["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
            {"weight": 8091, "preference": pref}, {"weight": 100, "preference": pref}]}}
    return {"metadata": {"name": name, "namespace": "default", "labels": {"app": "p"}}, "spec": spec}


def test_word_edges():
    """Four equal nodes (4 cpu, 8 Gi), two shards of two nodes, one-container pods of 500m / 1Gi.
    n1 alone lists big:1, 9000 MiB: scaledImageScore = 9000 MiB x 1/4 = 2250 MiB, above the
    1000 MiB x 1 container ceiling: ImageLocality 100, the field's maximum -- bits 25-31 hold
    1100100b, so bit 31 of n1's word is set.  Pod a prefers n2 with weights 8091 + 100 = 8191, the
    13-bit NodeAffinity field's maximum (all ones below the ImageLocality field in n2's word).
    On an empty node: TaintToleration 100 x 3, PodTopologySpread 100 x 2, Fit: cpu (4000 - 500) x 100 /
    4000 = 87, memory 7 x 100 / 8 = 87, mean 87; BalancedAllocation: both fractions 0.125, 100.
    300 + 200 + 87 + 100 = 687.
      pod a: n0 687, n1 687 + 100 = 787, n2 687 + 100 x 2 (NodeAffinity 8191 / 8191) = 887, n3 687 -> n2.
      pod b (no affinity): n2 now holds pod a: Fit cpu 3000 x 100 / 4000 = 75, memory 75 -> 675;
             n0 687, n1 787, n2 675, n3 687 -> n1."""
    nodes = [_node("n0"), _node("n1", [{"names": ["big:1"], "sizeBytes": 9000 * MI}]), _node("n2"), _node("n3")]
    pods = [_pod("a", "big:1", prefer="n2"), _pod("b", "big:1")]
    cc, cp, _ = compile_cluster(nodes, [], pods)
    assert cp.pods[0]["img_len"] == 1 and cp.pods[0]["n_containers"] == 1
    ch_o, res, st = itf.oracle(cc, cp)
    np.testing.assert_array_equal(res.norm[0][abi.KSS_S_IMAGE_LOCALITY, :4], [0, 100, 0, 0])
    np.testing.assert_array_equal(res.raw[0][abi.KSS_S_NODE_AFFINITY, :4], [0, 0, 8191, 0])
    np.testing.assert_array_equal(res.total[0, :4], [687, 787, 887, 687])
    np.testing.assert_array_equal(res.total[1, :4], [687, 787, 675, 687])
    np.testing.assert_array_equal(ch_o, [2, 1])
    for opt in (1, 0):
        native.reset_options()
        native.set_option("simple_ports_images", 1)
        native.set_option("table_images", 1)
        native.set_option("shards", 2)
        native.set_option("force_threads", 128)
        native.set_option("flat_exchange", opt)
        ctx = native.Context(abi.default_profile())
        ctx.load(cc.as_struct())
        chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
        assert ctx.last_kernel() == "k_simple"
        assert ctx.last_shape_table() == {"shapes": 1, "rounds": 1}
        assert ctx.last_simple_exchange() == ({"flat": 1, "entries": 4} if opt else {"flat": 0, "entries": 0})
        meta = ctx.fetch_meta(2)
        assert [list(m) for m in meta] == [[2, 4, 1, 0, 887], [1, 4, 1, 0, 787]], meta
        _check(ctx, chosen, cc, cp, ch_o, res, st)
        ctx.close()


# --------------------------------------------------------------------------------------
# 7. PreFilter-rejected pods and spec.nodeName pods in the batch
# --------------------------------------------------------------------------------------
def _edit_prefilter(nodes, bound, pods):
    names = [n["metadata"]["name"] for n in nodes]
    for j, i in ((5, 3), (40, 17), (41, 17)):  # (pod 41 follows pod 40 onto the same node)
        pods[j]["spec"]["nodeName"] = names[i]

    def after(cp):
        for j, status in ((9, abi.KSS_PF_NODE_AFFINITY_CONFLICT), (60, abi.KSS_PF_ERROR),
                          (61, abi.KSS_PF_NODE_AFFINITY_CONFLICT)):
            cp.pods[j]["prefilter_status"] = status
    return after


def test_prefilter_status_and_node_name_pods():
    case = itf.case(46, 130, 200, edit=("prefilter", _edit_prefilter))
    cc, cp, ch_o, res, st = case
    assert all(int(cp.pods[j]["node_name"]) >= 0 for j in (5, 40, 41))
    assert [res.meta(j)["status"] for j in (9, 60, 61)] == [2, 3, 2]
    _run(case, 2, 128)


# --------------------------------------------------------------------------------------
# 8. XCD-local placement, forced fallback, XCD-local grids off (the library's own geometry)
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["xcd_local", "forced_fallback", "xcd_off"])
def test_xcd_local_placement_fallback_and_off(mode):
    extra = {"xcd_local": {}, "forced_fallback": {"xcd_force_fallback": 1}, "xcd_off": {"xcd": 0}}[mode]
    _, _, xl = _run(itf.case(467, 377, 200), 0, 0, extra=extra, pin=False)
    if mode == "xcd_local":  # (a placement that fails by itself falls back: correct either way)
        assert xl["used"] == 1, xl
    else:
        assert xl == ({"used": 1, "fallbacks": 1} if mode == "forced_fallback" else {"used": 0, "fallbacks": 0}), xl


# --------------------------------------------------------------------------------------
# 9. routing stays put
# --------------------------------------------------------------------------------------
def _k_simple_pi(cc, cp, ch_o, res, st, prof=None, opts=(), cursor=False, kernel="k_simple"):
    """simple_ports_images on and `opts`: the batch runs on `kernel` without a table, equal to the oracle."""
    native.reset_options()
    native.set_option("simple_ports_images", 1)
    for k, v in opts:
        native.set_option(k, v)
    N = cc.n_nodes
    ctx = native.Context(prof or abi.default_profile())
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
    assert ctx.last_kernel() == kernel
    assert ctx.last_shape_table() == {"shapes": 0, "rounds": 0}
    assert ctx.last_simple_exchange() == {"flat": 0, "entries": 0}
    np.testing.assert_array_equal(chosen, ch_o)
    _meta_equal(ctx.fetch_meta(cp.n), res, cp.n)
    np.testing.assert_array_equal(ctx.port_state(), st["port_used"][:N])
    g = ctx.node_state()
    np.testing.assert_array_equal(g["requested"][:, :N], st["requested"][:, :N])
    np.testing.assert_array_equal(g["pod_count"][:N], st["pod_count"][:N])
    if cursor:
        assert ctx.next_start_node_index() == st["next_start"]
    geom = ctx.last_geometry()
    ctx.close()
    native.reset_options()
    return geom


def test_host_port_batch_stays_on_k_simple_pi():
    nodes, bound, pods = portimage_fuzz.make(31, n_nodes=40, n_bound=30, n_pods=120)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    assert itf.host_port_pods(cp) > 0
    ch_o, res, st = itf.oracle(cc, cp)
    assert (st["port_used"][:cc.n_nodes] != cc.arrays["port_used"][:cc.n_nodes]).any()
    geom = _k_simple_pi(cc, cp, ch_o, res, st, opts=(("table_images", 1), ("shards", 2), ("force_threads", 128)))
    assert (geom["shards"], geom["threads"]) == (2, 128)


def _edit_no_name_lists(nodes, bound, pods):
    """Drop the required node affinity of pods whose terms name nodes (matchFields metadata.name):
    no pod has a NodeAffinity PreFilterResult list, so k_simple runs the window itself."""
    for p in pods:
        na = (p["spec"].get("affinity") or {}).get("nodeAffinity") or {}
        req = na.get("requiredDuringSchedulingIgnoredDuringExecution") or {}
        if any(t.get("matchFields") for t in req.get("nodeSelectorTerms") or []):
            del na["requiredDuringSchedulingIgnoredDuringExecution"]


@pytest.mark.parametrize("kind", ["pct-40", "pct-40-no-name-lists", "il-weight-3", "one-shard", "table-images-0"])
def test_image_only_batch_off_the_table(kind):
    """The image-only batch where the table loop does not apply -- the window, a runtime profile, one
    shard with shape_table = 1 -- and with table_images 0: what ran before.  That is k_simple_pi,
    except for the window on this batch as it is: some of its pods carry a NodeAffinity
    PreFilterResult list, which keeps a windowed batch on k_schedule; without those lists k_simple_pi
    runs the window."""
    prof = abi.default_profile()
    opts = [("table_images", 0 if kind == "table-images-0" else 1), ("shards", 1 if kind == "one-shard" else 2),
            ("force_threads", 128)]
    kernel = "k_simple"
    if kind.startswith("pct-40"):
        prof.pct_nodes_to_score = 40
        lists = kind == "pct-40"
        cc, cp, ch_o, res, st = itf.case(46, 130, 200, pct=40, edit=None if lists else ("no-name-lists", _edit_no_name_lists))
        assert any(int(cp.pods[i]["names_len"]) >= 0 for i in range(cp.n)) == lists
        assert max(res.meta(j)["n_feasible"] for j in range(cp.n)) <= 100 < cc.n_nodes  # windowed
        kernel = "k_schedule" if lists else "k_simple"
    elif kind == "il-weight-3":
        prof.weight[abi.KSS_S_IMAGE_LOCALITY] = 3
        cc, cp = itf.case(46, 130, 200)[:2]
        ch_o, res, st = itf.oracle(cc, cp, prof)
    else:
        cc, cp, ch_o, res, st = itf.case(46, 130, 200)
    assert itf.host_port_pods(cp) == 0 and itf.il_decides(cc, cp, res, prof) >= 100
    geom = _k_simple_pi(cc, cp, ch_o, res, st, prof=prof, opts=opts, cursor=kind.startswith("pct-40"), kernel=kernel)
    if kernel == "k_simple":
        assert geom["shards"] == (1 if kind == "one-shard" else 2) and geom["threads"] == 128
