"""k_simple's ports-and-images form (option simple_ports_images: k_static_pi + k_simple_pi) against the
C oracle, bit for bit: chosen nodes, every pod's outcome, the final UsedPorts and node rows.

NodePorts is state of the loop (one UsedPorts word per node slot in LDS: filter, AssumePod, the H1
re-evaluation with the previous pod's ports), ImageLocality is in the static word.  The clusters
are tests/portimage_fuzz.py's; every fuzz case first asserts on the oracle's own records that the
batch reaches what it is meant to (NodePorts failures, a NodePorts failure caused by the previous
pod's commit on the node it took, choices that ImageLocality decides)."""
import copy

import numpy as np
import pytest

import oracle_c
import portimage_fuzz
import preempt_fixtures as pf
import preempt_port_fixtures as ppf
import progfuzz
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu
MI = 1024 * 1024


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _oracle(cc, cp, prof=None, record=True):
    return oracle_c.schedule(prof or abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes,
                             record=record, n_classes=len(cc.classes), n_terms=len(cc.terms))


_CACHE = {}


def _fuzz(seed, n_nodes=12, n_bound=10, n_pods=30, pct=100):
    """(cc, cp, oracle chosen, records, final state) of one fuzz cluster, computed once and shared
    (nothing writes to them)."""
    key = (seed, n_nodes, n_bound, n_pods, pct)
    if key not in _CACHE:
        nodes, bound, pods = portimage_fuzz.make(seed, n_nodes=n_nodes, n_bound=n_bound, n_pods=n_pods)
        cc, cp, _ = compile_cluster(nodes, bound, pods)
        prof = abi.default_profile()
        prof.pct_nodes_to_score = pct
        _CACHE[key] = (cc, cp) + tuple(_oracle(cc, cp, prof))
    return _CACHE[key]


def _reach(cc, cp, ch_o, res, prof=None):
    """What the oracle's records say the batch exercises: pods with a node failing NodePorts, pairs
    (k, k+1) where pod k+1 fails NodePorts on the node pod k took only because of pod k's own ports
    (the loop's H1 evaluation), pods whose choice is not the argmax of total - ImageLocality."""
    prof = prof or abi.default_profile()
    N = cc.n_nodes
    used = cc.arrays["port_used"][:N].copy()
    w_il = prof.weight[abi.KSS_S_IMAGE_LOCALITY] if (prof.score_enabled >> abi.KSS_S_IMAGE_LOCALITY) & 1 else 0
    port_pods = h1 = il_pods = 0
    for j in range(cp.n):
        fp = res.fail_plugin[j, :N]
        port_pods += int((fp == abi.KSS_F_NODE_PORTS).any())
        if j > 0 and ch_o[j - 1] >= 0:
            x = int(ch_o[j - 1])
            conflict = int(cp.pods[j]["port_conflict"])
            if fp[x] == abi.KSS_F_NODE_PORTS and not (int(before[x]) & conflict) and (int(cp.pods[j - 1]["port_add"]) & conflict):
                h1 += 1
        m = res.meta(j)
        if m["scored"]:
            kept = (fp == 0) & (res.fail_detail[j, :N] != abi.KSS_PASS_NOT_KEPT)
            rest = np.where(kept, res.total[j, :N] - w_il * res.norm[j][abi.KSS_S_IMAGE_LOCALITY, :N], -1)
            il_pods += int(np.argmax(rest) != m["chosen"])
        before = used.copy()
        if ch_o[j] >= 0:
            used[int(ch_o[j])] |= np.uint64(int(cp.pods[j]["port_add"]))
    return port_pods, h1, il_pods


def _meta_equal(meta, res, n):
    for j in range(n):
        m = res.meta(j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], j


def _run(cc, cp, ch_o, res, st, prof=None, flags=0, kernel="k_simple", cursor=False):
    """One batch on a fresh context against the oracle; returns the context's launch count."""
    N = cc.n_nodes
    ctx = native.Context(prof or abi.default_profile())
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n, flags=flags)
    assert ctx.last_kernel() == kernel
    if kernel == "k_simple":
        assert ctx.last_shape_table()["shapes"] == 0
    np.testing.assert_array_equal(chosen, ch_o)
    _meta_equal(ctx.fetch_meta(cp.n), res, cp.n)
    np.testing.assert_array_equal(ctx.port_state(), st["port_used"][:N])
    g = ctx.node_state()
    np.testing.assert_array_equal(g["requested"][:, :N], st["requested"][:, :N])
    np.testing.assert_array_equal(g["nonzero"][:, :N], st["nonzero"][:, :N])
    np.testing.assert_array_equal(g["pod_count"][:N], st["pod_count"][:N])
    if cursor:
        assert ctx.next_start_node_index() == st["next_start"]
    launches = ctx.last_timing()[1]
    geom = dict(ctx.last_geometry(), xcd_local=ctx.last_xcd_local()["used"])
    ctx.close()
    return launches, geom


# --------------------------------------------------------------------------------------
# 1. fuzz over geometries
# --------------------------------------------------------------------------------------
GEOMETRIES = (
    [("small-%d" % s, (s, 12, 10, 30), dict(shards=1), abi.KSS_SCHED_FORCE_SINGLE_WG, 1) for s in range(6)]
    + [("one-wave", (31, 40, 30, 120), dict(shards=2, force_threads=64), 0, 2),
       ("pw-2-waves", (11, 300, 300, 200), dict(shards=3, force_threads=128), 0, 3),
       ("pw-3-waves", (11, 300, 300, 200), dict(shards=3, force_threads=192), 0, 3),
       ("nine-shards", (11, 300, 300, 200), dict(shards=9), 0, 9),
       ("slots-per-lane", (11, 300, 300, 200), dict(shards=1, force_threads=64), 0, 1)])
# the oracle's own counts for these seeds and sizes: (pods with a NodePorts failure, H1 pairs, pods
# whose choice ImageLocality decides)
REACH = {(31, 40, 30, 120): (62, 8, 50), (11, 300, 300, 200): (109, 7, 104)}


# every sharded geometry once on the XCD-local grid (the shard count through nodes_per_shard: a
# forced count keeps the grid unrestricted) and once with xcd = 0; one shard has no exchange
CASES = [g + (x,) for g in GEOMETRIES for x in ((1, 0) if g[4] > 1 else (0,))]


@pytest.mark.parametrize("name,cluster,opts,flags,shards,xcd", CASES,
                         ids=["%s-%s" % (c[0], "xcd" if c[5] else "plain") for c in CASES])
def test_fuzz_geometries(name, cluster, opts, flags, shards, xcd):
    seed, n_nodes, n_bound, n_pods = cluster
    cc, cp, ch_o, res, st = _fuzz(seed, n_nodes, n_bound, n_pods)
    reach = _reach(cc, cp, ch_o, res)
    print(name, "reach", reach)
    if cluster in REACH:
        assert reach == REACH[cluster], reach
    else:  # 12 x 30, seeds 0-5
        assert 12 <= reach[0] <= 18 and 1 <= reach[1] <= 4 and 4 <= reach[2] <= 20, reach
    native.set_option("simple_ports_images", 1)
    native.set_option("xcd", xcd)
    for k, v in opts.items():
        if k == "shards" and xcd:
            native.set_option("nodes_per_shard", (n_nodes + v - 1) // v)
        else:
            native.set_option(k, v)
    _, geom = _run(cc, cp, ch_o, res, st, flags=flags)
    assert geom["shards"] == shards and geom["xcd_local"] == xcd, geom
    if "force_threads" in opts:
        assert geom["threads"] == opts["force_threads"], geom
    if name == "slots-per-lane":
        assert geom["nodes_per_lane"] > 1, geom


# --------------------------------------------------------------------------------------
# 2. port exhaustion, hand-derived
# --------------------------------------------------------------------------------------
def _node(name, images=None):
    st = {"allocatable": {"cpu": "4", "memory": "8Gi", "pods": "20", "ephemeral-storage": "20Gi"}}
    if images:
        st["images"] = images
    return {"metadata": {"name": name, "labels": {"kubernetes.io/hostname": name}}, "spec": {}, "status": st}


def _pod(name, containers):
    return {"metadata": {"name": name, "namespace": "default", "labels": {"app": "p"}}, "spec": {"containers": containers}}


def _ctr(name, image, ports=None):
    c = {"name": name, "image": image, "resources": {"requests": {"cpu": "500m", "memory": "1Gi"}}}
    if ports:
        c["ports"] = ports
    return c


@pytest.mark.parametrize("shards", [1, 2, 3])
def test_port_exhaustion(shards):
    """Six identical nodes, eight identical pods that each hold hostPort 8080.  Equal totals: a pod
    takes the lowest-index node whose port is free, so pods 0-5 land on nodes 0..5 in order (each
    sees its predecessor's port through the H1 evaluation) and pods 6, 7 find no node."""
    nodes = [_node("n%d" % i) for i in range(6)]
    pods = [_pod("p%d" % j, [_ctr("c", "none:1", [{"containerPort": 80, "hostPort": 8080}])]) for j in range(8)]
    cc, cp, _ = compile_cluster(nodes, [], pods)
    assert len(cc.ports) == 1
    ch_o, res, st = _oracle(cc, cp)
    want_chosen = [0, 1, 2, 3, 4, 5, -1, -1]
    want_feasible = [6, 5, 4, 3, 2, 1, 0, 0]
    np.testing.assert_array_equal(ch_o, want_chosen)
    assert [res.meta(j)["n_feasible"] for j in range(8)] == want_feasible
    np.testing.assert_array_equal(st["port_used"][:6], [1] * 6)
    native.set_option("simple_ports_images", 1)
    native.set_option("shards", shards)
    N = 6
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
    assert ctx.last_kernel() == "k_simple" and ctx.last_shape_table()["shapes"] == 0
    assert ctx.last_geometry()["shards"] == shards
    np.testing.assert_array_equal(chosen, want_chosen)
    meta = ctx.fetch_meta(8)
    assert list(meta[:, 1]) == want_feasible
    assert list(meta[:, 3]) == [0] * 6 + [1, 1]  # pods 6, 7: unschedulable
    _meta_equal(meta, res, 8)
    np.testing.assert_array_equal(ctx.port_state(), [1] * N)
    np.testing.assert_array_equal(ctx.node_state()["pod_count"][:N], [1] * N)
    ctx.close()


# --------------------------------------------------------------------------------------
# 3. dictionary edge: 64 entries, the conflicting holder is bit 63
# --------------------------------------------------------------------------------------
def test_port_dictionary_bit_63():
    """preempt_port_fixtures.bit63's cluster (x: the holder of 10.0.0.9 TCP 60000, the dictionary's
    last entry; y: a wildcard holder; z: another group) plus two free nodes w, v.  Pod a wants
    0.0.0.0 TCP 60000: x fails on bit 63 alone, y on the wildcard entry, it takes w.  Pod b wants
    10.0.0.9 TCP 60000: w now fails through pod a's commit, it takes v, whose word gets bit 63."""
    nodes, bound, _, holder = ppf.bit63()
    nodes = nodes + [pf.node("w", "g1"), pf.node("v", "g1")]
    pods = [ppf.with_ports(pf.pod("a", 10, "100m", group="g1"), (60000, "TCP", None)),
            ppf.with_ports(pf.pod("b", 10, "100m", group="g1"), (60000, "TCP", "10.0.0.9"))]
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    assert len(cc.ports) == 64 and cc.port_index[holder] == 63
    top = 1 << 63
    assert int(cp.pods[0]["port_conflict"]) & top and int(cp.pods[1]["port_add"]) == top
    x = cc.node_names.index("x")
    assert int(cc.arrays["port_used"][x]) & int(cp.pods[0]["port_conflict"]) == top  # bit 63 alone fails x
    ch_o, res, st = _oracle(cc, cp)
    w, v = cc.node_names.index("w"), cc.node_names.index("v")
    np.testing.assert_array_equal(ch_o, [w, v])
    assert res.fail_plugin[0, x] == abi.KSS_F_NODE_PORTS and res.fail_plugin[1, w] == abi.KSS_F_NODE_PORTS
    assert int(st["port_used"][v]) == top
    native.set_option("simple_ports_images", 1)
    native.set_option("shards", 2)
    _, geom = _run(cc, cp, ch_o, res, st)
    assert geom["shards"] == 2


# --------------------------------------------------------------------------------------
# 4. image score ends
# --------------------------------------------------------------------------------------
def test_image_score_ends():
    """Three equal nodes, a two-container pod (500m / 1Gi each).  scaledImageScore = size x 1/3 (each
    image on one of three nodes).  n0 lists nothing: 0.  n1 lists small:1, 30 MiB -> 10 MiB, below
    the 23 MiB threshold: 0.  n2 lists big:1, 9000 MiB -> 3000 MiB, above 1000 MiB x 2 containers:
    100.  Elsewhere the nodes tie: TaintToleration 100 x 3, NodeAffinity 0, Fit (75 + 75) / 2,
    PodTopologySpread 100 x 2, BalancedAllocation 100 = 675; n2 wins with 775."""
    nodes = [_node("n0"), _node("n1", [{"names": ["small:1"], "sizeBytes": 30 * MI}]),
             _node("n2", [{"names": ["big:1"], "sizeBytes": 9000 * MI}])]
    pods = [_pod("p", [_ctr("c0", "small:1"), _ctr("c1", "big:1")])]
    cc, cp, _ = compile_cluster(nodes, [], pods)
    assert cp.pods[0]["img_len"] == 2 and cp.pods[0]["n_containers"] == 2
    ch_o, res, st = _oracle(cc, cp)
    np.testing.assert_array_equal(res.norm[0][abi.KSS_S_IMAGE_LOCALITY, :3], [0, 0, 100])
    np.testing.assert_array_equal(res.total[0, :3], [675, 675, 775])
    native.set_option("simple_ports_images", 1)
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), 1)
    assert ctx.last_kernel() == "k_simple" and ctx.last_shape_table()["shapes"] == 0
    np.testing.assert_array_equal(chosen, [2])
    meta = ctx.fetch_meta(1)
    assert list(meta[0]) == [2, 3, 1, 0, 775]
    _meta_equal(meta, res, 1)
    ctx.close()


# --------------------------------------------------------------------------------------
# 5. chunked batch: UsedPorts carried from launch to launch
# --------------------------------------------------------------------------------------
def test_chunked_batch_carries_ports():
    cc, cp, ch_o, res, st = _fuzz(11, 300, 300, 200)
    native.set_option("simple_ports_images", 1)
    native.set_option("shards", 3)
    native.set_option("static_bytes", 4 * cc.n_nodes * 60)  # 60 pods per chunk: 4 chunk launches
    launches, _ = _run(cc, cp, ch_o, res, st)
    assert launches >= 2 * 3, launches  # k_static + the loop kernel per chunk, at least 3 chunks


# --------------------------------------------------------------------------------------
# 6. the window
# --------------------------------------------------------------------------------------
# 1 and 3 shards in per-wave mode; "1x64": one shard of 64 lanes, three node slots per lane (the
# window's per-thread passes and its local cut scan)
@pytest.mark.parametrize("shards", [1, 3, "1x64"])
@pytest.mark.parametrize("pct", [0, 40])
@pytest.mark.parametrize("cluster", [(32, 180, 150, 150), (33, 130, 100, 400)], ids=["180x150", "130x400"])
def test_window(cluster, pct, shards):
    seed, n_nodes, n_bound, n_pods = cluster
    cc, cp, ch_o, res, st = _fuzz(seed, n_nodes, n_bound, n_pods, pct=pct)
    N = cc.n_nodes
    feas = [res.meta(j)["n_feasible"] for j in range(cp.n)]
    assert max(feas) <= 100 < N  # every pod's search is windowed: K = 100 feasible nodes at most
    port_pods = sum(int((res.fail_plugin[j, :N] == abi.KSS_F_NODE_PORTS).any()) for j in range(cp.n))
    print("window", cluster, pct, "pods with a NodePorts failure", port_pods, "cursor", st["next_start"])
    assert port_pods >= 1
    prof = abi.default_profile()
    prof.pct_nodes_to_score = pct
    native.set_option("simple_ports_images", 1)
    if shards == "1x64":
        shards = 1
        native.set_option("force_threads", 64)
    native.set_option("shards", shards)
    _, geom = _run(cc, cp, ch_o, res, st, prof=prof, cursor=True)
    assert geom["shards"] == shards


# --------------------------------------------------------------------------------------
# 7. runtime profile
# --------------------------------------------------------------------------------------
def _profile(kind):
    p = abi.default_profile()
    if kind == "il-weight-3":
        p.weight[abi.KSS_S_IMAGE_LOCALITY] = 3
    elif kind == "il-disabled":
        p.score_enabled &= ~(1 << abi.KSS_S_IMAGE_LOCALITY)
    else:  # the filter off: ports filter nothing, AssumePod still records them
        p.filter_enabled &= ~(1 << abi.KSS_F_NODE_PORTS)
    return p


@pytest.mark.parametrize("kind", ["il-weight-3", "il-disabled", "ports-filter-off"])
def test_runtime_profile(kind):
    nodes, bound, pods = portimage_fuzz.make(31, n_nodes=40, n_bound=30, n_pods=120)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    prof = _profile(kind)
    ch_o, res, st = _oracle(cc, cp, prof)
    port_pods, _, il_pods = _reach(cc, cp, ch_o, res, prof)
    if kind == "ports-filter-off":
        assert port_pods == 0 and (st["port_used"][:cc.n_nodes] != cc.arrays["port_used"][:cc.n_nodes]).any()
    else:
        assert port_pods > 0
    assert (il_pods == 0) == (kind == "il-disabled")
    native.set_option("simple_ports_images", 1)
    native.set_option("shards", 2)
    _run(cc, cp, ch_o, res, st, prof=prof)


# --------------------------------------------------------------------------------------
# 8. option off / a batch not of the form
# --------------------------------------------------------------------------------------
def test_option_off_runs_k_schedule():
    cc, cp, ch_o, res, st = _fuzz(31, 40, 30, 120)
    native.set_option("shards", 2)
    _run(cc, cp, ch_o, res, st, kernel="k_schedule")


def test_option_turned_off_between_stage_and_run():
    """The option is process-wide and read twice: at the stage (records of the form) and again at the
    run.  Turned off in between, the staged batch runs on k_schedule, with the oracle's results."""
    cc, cp, ch_o, res, st = _fuzz(3)
    N = cc.n_nodes
    native.set_option("simple_ports_images", 1)
    assert native.plan_podset(cc.as_struct(), cp.as_struct())["kernel"] == "k_simple"
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    ctx.stage(cp.as_struct())
    native.set_option("simple_ports_images", 0)
    chosen = ctx.run_staged(cp.n)
    assert ctx.last_kernel() == "k_schedule"
    np.testing.assert_array_equal(chosen, ch_o)
    _meta_equal(ctx.fetch_meta(cp.n), res, cp.n)
    np.testing.assert_array_equal(ctx.port_state(), st["port_used"][:N])
    g = ctx.node_state()
    np.testing.assert_array_equal(g["requested"][:, :N], st["requested"][:, :N])
    np.testing.assert_array_equal(g["nonzero"][:, :N], st["nonzero"][:, :N])
    np.testing.assert_array_equal(g["pod_count"][:N], st["pod_count"][:N])
    ctx.close()


def test_batch_without_ports_or_images_is_untouched():
    nodes, bound, pods = progfuzz.make(2, 300, 300, extended=False, programs=False)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    assert not any(cp.pods[i]["port_conflict"] or cp.pods[i]["port_add"] or cp.pods[i]["img_len"] > 0
                   for i in range(cp.n))
    ch_o, res, st = _oracle(cc, cp, record="meta")
    seen = []
    for on in (0, 1):
        native.set_option("simple_ports_images", on)
        ctx = native.Context(abi.default_profile())
        ctx.load(cc.as_struct())
        chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
        np.testing.assert_array_equal(chosen, ch_o)
        _meta_equal(ctx.fetch_meta(cp.n), res, cp.n)
        seen.append((ctx.last_kernel(), ctx.last_shape_table(), ctx.last_simple_exchange(), ctx.last_geometry(),
                     ctx.node_state()["requested"].tobytes(), ctx.port_state().tobytes()))
        ctx.close()
    assert seen[0][0] == "k_simple" and seen[0] == seen[1]


# --------------------------------------------------------------------------------------
# 9. PreFilter-rejected pods and spec.nodeName pods in the batch
# --------------------------------------------------------------------------------------
def test_prefilter_status_and_node_name_pods():
    nodes, bound, pods = portimage_fuzz.make(31, n_nodes=40, n_bound=30, n_pods=120)
    pods = copy.deepcopy(pods)
    for j, nm in ((5, "n03"), (40, "n17"), (41, "n17")):  # (pod 41 follows pod 40 onto the same node)
        pods[j]["spec"]["nodeName"] = nm
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    for j, status in ((9, abi.KSS_PF_NODE_AFFINITY_CONFLICT), (60, abi.KSS_PF_ERROR), (61, abi.KSS_PF_NODE_AFFINITY_CONFLICT)):
        cp.pods[j]["prefilter_status"] = status
    assert sum(int(cp.pods[j]["node_name"] >= 0) for j in range(cp.n)) == 3
    ch_o, res, st = _oracle(cc, cp)
    assert [res.meta(j)["status"] for j in (9, 60, 61)] == [2, 3, 2]
    assert _reach(cc, cp, ch_o, res)[0] > 0
    native.set_option("simple_ports_images", 1)
    native.set_option("shards", 2)
    _run(cc, cp, ch_o, res, st)
