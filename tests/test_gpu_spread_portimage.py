"""k_spread's ports-and-images form (option spread_ports_images: k_static_pi + k_spread<.., PI>)
against the C oracle, bit for bit: chosen nodes, every pod's outcome, the final UsedPorts, node
rows and class / term counts.

The batches are tests/spread_portimage_fuzz.py's: progfuzz's programs (every PodTopologySpread /
InterPodAffinity kind) with node images, container images and host ports grafted on.  Every fuzz
case first asserts on the oracle's own records what the batch reaches -- pods with a NodePorts
failure, pods whose choice ImageLocality decides, pods with a PodTopologySpread / InterPodAffinity
failure -- and only then runs the device."""
import copy

import numpy as np
import pytest

import oracle_c
import spread_portimage_fuzz as spf
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu
MI = 1024 * 1024
MODES = {"auto": 0, "single": abi.KSS_SCHED_FORCE_SINGLE_WG, "multi": abi.KSS_SCHED_FORCE_MULTI_WG}

# the oracle's own counts under the default profile: (scheduled, pods with a NodePorts failure, pods
# whose choice ImageLocality decides, pods with a PodTopologySpread failure, with an InterPodAffinity
# failure), keyed by (seed, nodes, pods, names_lists, pct)
REACH = {
    (1, 60, 200, True, 100): (182, 50, 13, 119, 150),
    (2, 300, 300, True, 100): (235, 74, 28, 172, 291),
    (4, 5, 40, True, 100): (27, 5, 3, 15, 12),
    (20, 211, 150, True, 100): (138, 37, 23, 74, 132),
    (21, 211, 150, True, 100): (110, 42, 8, 91, 137),
    (22, 211, 150, True, 100): (118, 40, 12, 84, 145),
    (2, 300, 300, False, 0): (237, 76, 28, 175, 293),
    (20, 211, 150, False, 0): (138, 38, 28, 77, 138),
    (2, 300, 300, False, 50): (237, 76, 27, 175, 293),
    (20, 211, 150, False, 50): (138, 38, 23, 77, 138),
    (2, 300, 300, True, 0): (235, 74, 28, 172, 291),
    (1, 12, 40, True, 100): (31, 6, 4, 18, 20),
}


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _prof(pct=100):
    p = abi.default_profile()
    p.pct_nodes_to_score = pct
    return p


def _oracle(cc, cp, prof):
    return oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record=True, threads=8,
                             n_classes=len(cc.classes), n_terms=len(cc.terms))


def _reach(cc, cp, ch_o, res, prof):
    """What the oracle's records say the batch exercises (the columns of REACH)."""
    N = cc.n_nodes
    w_il = prof.weight[abi.KSS_S_IMAGE_LOCALITY] if (prof.score_enabled >> abi.KSS_S_IMAGE_LOCALITY) & 1 else 0
    port = il = pts = ipa = 0
    for j in range(cp.n):
        fp = res.fail_plugin[j, :N]
        port += int((fp == abi.KSS_F_NODE_PORTS).any())
        pts += int((fp == abi.KSS_F_POD_TOPOLOGY_SPREAD).any())
        ipa += int((fp == abi.KSS_F_INTER_POD_AFFINITY).any())
        m = res.meta(j)
        if m["scored"]:
            kept = (fp == 0) & (res.fail_detail[j, :N] != abi.KSS_PASS_NOT_KEPT)
            rest = np.where(kept, res.total[j, :N] - w_il * res.norm[j][abi.KSS_S_IMAGE_LOCALITY, :N], -1)
            il += int(np.argmax(rest) != m["chosen"])
    return int((np.asarray(ch_o) >= 0).sum()), port, il, pts, ipa


_CACHE = {}


def _fuzz(seed, n_nodes, n_pods, names_lists=True, pct=100):
    """(cc, cp, oracle chosen, records, final state) of one grafted batch under the default profile,
    computed once and shared (nothing writes to them); its reach is asserted here, before any
    device run."""
    key = (seed, n_nodes, n_pods, names_lists, pct)
    if key not in _CACHE:
        cc, cp, _ = compile_cluster(*spf.make(seed, n_nodes, n_pods, names_lists=names_lists))
        prof = _prof(pct)
        ch_o, res, st = _oracle(cc, cp, prof)
        reach = _reach(cc, cp, ch_o, res, prof)
        print("reach", key, reach, "ports", len(cc.ports))
        assert reach == REACH[key], (key, reach)
        assert reach[1] > 0 and reach[2] > 0
        assert len(cc.ports) <= 24
        _CACHE[key] = (cc, cp, ch_o, res, st)
    return _CACHE[key]


def _check(ctx, cc, cp, ch_o, res, st, chosen, cursor=False):
    N, ncl, nt = cc.n_nodes, len(cc.classes), len(cc.terms)
    np.testing.assert_array_equal(chosen, ch_o)
    meta = ctx.fetch_meta(cp.n)
    for j in range(cp.n):
        m = res.meta(j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], (j, meta[j, 4], m["best_total"])
    np.testing.assert_array_equal(ctx.port_state(), st["port_used"][:N])
    g = ctx.node_state()
    np.testing.assert_array_equal(g["requested"][:, :N], st["requested"][:, :N])
    np.testing.assert_array_equal(g["nonzero"][:, :N], st["nonzero"][:, :N])
    np.testing.assert_array_equal(g["pod_count"][:N], st["pod_count"][:N])
    if ncl:
        np.testing.assert_array_equal(g["class_count"][:ncl], st["class_count"][:ncl])
    if nt:
        np.testing.assert_array_equal(g["term_count"][:nt], st["term_count"][:nt])
    if cursor:
        assert ctx.next_start_node_index() == st["next_start"]


def _run(cc, cp, ch_o, res, st, prof=None, flags=0, kernel="k_spread", cursor=False, on=1):
    """One batch on a fresh context against the oracle; returns what the launch reports."""
    native.set_option("spread_ports_images", on)
    ctx = native.Context(prof or abi.default_profile())
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n, flags=flags)
    assert ctx.last_kernel() == kernel, ctx.last_kernel()
    _check(ctx, cc, cp, ch_o, res, st, chosen, cursor=cursor)
    info = dict(ctx.last_geometry(), xcd=ctx.last_xcd_local(), launches=ctx.last_timing()[1], lds=ctx.last_spread_lds(),
                retries=ctx.last_handoff_retries(), handoff=ctx.last_handoff_status())
    ctx.close()
    print("launch", info)
    return info


# --------------------------------------------------------------------------------------
# 1. modes
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster,mode", [((4, 5, 40), "auto"), ((4, 5, 40), "single"), ((4, 5, 40), "multi"),
                                          ((1, 60, 200), "auto"), ((1, 60, 200), "single"), ((1, 60, 200), "multi"),
                                          ((2, 300, 300), "auto"), ((2, 300, 300), "multi")],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d" % v[1:])
def test_modes(cluster, mode):
    cc, cp, ch_o, res, st = _fuzz(*cluster)
    info = _run(cc, cp, ch_o, res, st, flags=MODES[mode])
    if mode == "single":
        assert info["shards"] == 1, info
    if mode == "multi":
        assert info["shards"] > 1, info
    assert info["lds"] > 0


# --------------------------------------------------------------------------------------
# 2. nine shards, ragged last shard (211 = 8 x 24 + 19)
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [20, 21, 22])
def test_nine_shards(seed):
    cc, cp, ch_o, res, st = _fuzz(seed, 211, 150)
    native.set_option("shards", 9)
    info = _run(cc, cp, ch_o, res, st)
    assert info["shards"] == 9 and info["xcd"]["used"] == 0, info


# a shard count through nodes_per_shard leaves the placement to the library (a forced count keeps the
# grid unrestricted): the XCD-local grid, the same with xcd = 0, and the placement reported failed
# (xcd_force_fallback: every launch runs again unrestricted, err = 3 retry)
@pytest.mark.parametrize("seed,kind", [(20, "xcd-off"), (21, "xcd-local"), (22, "xcd-fallback")])
def test_nine_shards_placement(seed, kind):
    cc, cp, ch_o, res, st = _fuzz(seed, 211, 150)
    native.set_option("nodes_per_shard", 24)
    if kind == "xcd-off":
        native.set_option("xcd", 0)
    if kind == "xcd-fallback":
        native.set_option("xcd_force_fallback", 1)
    info = _run(cc, cp, ch_o, res, st)
    assert info["shards"] == 9, info
    assert info["xcd"]["used"] == (0 if kind == "xcd-off" else 1), info
    assert (info["xcd"]["fallbacks"] >= 1) == (kind == "xcd-fallback"), info


# --------------------------------------------------------------------------------------
# 3. workgroup sizes: the kernels built for <= 256 lanes and for KSS_MAX_THREADS
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster,opts,lb256", [((20, 211, 150), dict(shards=3, force_threads=128), True),
                                                ((2, 300, 300), dict(shards=2, force_threads=320), False)],
                         ids=["lb256", "320-lanes"])
def test_workgroup_sizes(cluster, opts, lb256):
    cc, cp, ch_o, res, st = _fuzz(*cluster)
    for k, v in opts.items():
        native.set_option(k, v)
    info = _run(cc, cp, ch_o, res, st)
    assert info["shards"] == opts["shards"] and info["threads"] == opts["force_threads"], info
    assert (info["threads"] <= 256) == lb256


# --------------------------------------------------------------------------------------
# 4. the window
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pct", [0, 50])
@pytest.mark.parametrize("cluster", [(2, 300, 300), (20, 211, 150)], ids=["300x300", "211x150"])
def test_window(cluster, pct):
    """numFeasibleNodesToFind is 144 of 300 and 103 of 211 at pct 0 (adaptive: 50 - N / 125 = 48 % and
    49 %), 150 and 105 at pct 50: below N, so every pod's search is windowed."""
    cc, cp, ch_o, res, st = _fuzz(*cluster, names_lists=False, pct=pct)
    N = cc.n_nodes
    k_find = {(300, 0): 144, (211, 0): 103, (300, 50): 150, (211, 50): 105}[(N, pct)]
    feas = [res.meta(j)["n_feasible"] for j in range(cp.n)]
    assert max(feas) <= k_find < N and max(feas) > k_find // 2, (max(feas), k_find)
    native.set_option("shards", 9 if N == 211 else 0)
    _run(cc, cp, ch_o, res, st, prof=_prof(pct), cursor=True)


def test_window_with_name_lists_stays_on_k_schedule():
    cc, cp, ch_o, res, st = _fuzz(2, 300, 300, names_lists=True, pct=0)
    assert any(cp.pods[i]["names_len"] >= 0 for i in range(cp.n))
    _run(cc, cp, ch_o, res, st, prof=_prof(0), kernel="k_schedule", cursor=True)


# --------------------------------------------------------------------------------------
# 5. chunks: UsedPorts carried from launch to launch through the checked hand-off
# --------------------------------------------------------------------------------------
def test_chunked_batch_carries_ports():
    cc, cp, ch_o, res, st = _fuzz(20, 211, 150)
    assert (st["port_used"][:211] != cc.arrays["port_used"][:211]).any()
    native.set_option("shards", 9)
    native.set_option("static_bytes", 4 * 211 * 23)  # 23 pods per chunk
    info = _run(cc, cp, ch_o, res, st)
    assert info["launches"] == 2 * ((150 + 22) // 23), info  # k_static_pi + k_spread per chunk
    print("hand-off retries", info["retries"], info["handoff"])  # reported, not asserted to be zero


# --------------------------------------------------------------------------------------
# 6. runtime profile: the DEF = false kernels
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["il-weight-5-ports-filter-off", "il-disabled"])
def test_custom_profile(kind):
    prof = abi.default_profile()
    if kind == "il-disabled":
        prof.score_enabled &= ~(1 << abi.KSS_S_IMAGE_LOCALITY)
    else:  # the filter off: ports filter nothing, AssumePod still records them
        prof.weight[abi.KSS_S_IMAGE_LOCALITY] = 5
        prof.filter_enabled &= ~(1 << abi.KSS_F_NODE_PORTS)
    cc, cp, _ = compile_cluster(*spf.make(21, 211, 150))
    ch_o, res, st = _oracle(cc, cp, prof)
    reach = _reach(cc, cp, ch_o, res, prof)
    print("reach", kind, reach)
    N = cc.n_nodes
    if kind == "il-disabled":
        assert reach[1] > 0 and reach[2] == 0, reach
    else:
        assert reach[1] == 0 and reach[2] > 0, reach
        assert (st["port_used"][:N] != cc.arrays["port_used"][:N]).any()
    assert reach[3] > 0 and reach[4] > 0, reach
    native.set_option("shards", 9)
    info = _run(cc, cp, ch_o, res, st, prof=prof)
    assert info["shards"] == 9


# --------------------------------------------------------------------------------------
# 7. word edges, hand-derived
# --------------------------------------------------------------------------------------
def _edge_cluster():
    def node(name, zone, pref, images=None):
        status = {"allocatable": {"cpu": "4", "memory": "8Gi", "pods": "20", "ephemeral-storage": "20Gi"}}
        if images:
            status["images"] = images
        labels = {"kubernetes.io/hostname": name, "topology.kubernetes.io/zone": zone}
        if pref:
            labels["pref"] = "yes"
        return {"metadata": {"name": name, "labels": labels}, "spec": {}, "status": status}

    def ctr(image, port=None):
        c = {"name": "c", "image": image, "resources": {"requests": {"cpu": "500m", "memory": "1Gi"}}}
        if port:
            c["ports"] = [{"containerPort": 80, "hostPort": port}]
        return c

    big = [{"names": ["big:1"], "sizeBytes": 9000 * MI}]
    nodes = [node("a", "z1", True, big), node("b", "z3", True, big), node("c", "z2", False)]
    bound = []
    for nm, apps, port in (("a", "xyy", None), ("b", "yyy", 8080), ("c", "xxx", None)):
        for i, app in enumerate(apps):
            bound.append({"metadata": {"name": "%s%d" % (nm, i), "namespace": "default", "labels": {"app": app}},
                          "spec": {"nodeName": nm, "containers": [ctr("none:1", port if i == 0 else None)]}})
    pref = {"matchExpressions": [{"key": "pref", "operator": "In", "values": ["yes"]}]}
    spec = {"containers": [ctr("big:1", 8080)],
            "affinity": {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
                {"weight": 8091, "preference": pref}, {"weight": 100, "preference": pref}]}},
            "topologySpreadConstraints": [{"maxSkew": 1, "topologyKey": "topology.kubernetes.io/zone",
                                           "whenUnsatisfiable": "ScheduleAnyway",
                                           "labelSelector": {"matchLabels": {"app": "x"}}}]}
    pods = [{"metadata": {"name": "p%d" % j, "namespace": "default", "labels": {"app": "p"}}, "spec": copy.deepcopy(spec)}
            for j in range(2)]
    return nodes, bound, pods


@pytest.mark.parametrize("shards", [1, 3])
def test_word_edges(shards):
    """Three equal nodes (4 cpu, 8 Gi), three bound pods of 500m / 1 Gi on each; two identical pending
    pods (500m / 1 Gi, image big:1, hostPort 8080, preferred NodeAffinity 8091 + 100 = 8191 on
    pref=yes, ScheduleAnyway zone spread over app=x).

      a  zone z1, pref=yes, lists big:1, one app=x pod
      b  zone z3, pref=yes, lists big:1, no app=x pod, a bound pod holds hostPort 8080
      c  zone z2, no label, no image, three app=x pods

    ImageLocality: big:1 is 9000 MiB on 2 of 3 nodes, 6000 MiB scaled, above the 1000 MiB ceiling of
    one container: 100 on a and b (bit 31 of the static word), 0 on c.  b is best on every score --
    NodeAffinity 8191, ImageLocality 100, an empty zone -- and fails NodePorts.

    Pod 0, feasible {a, c}.  TaintToleration 100 x 3.  NodeAffinity raw 8191 / 0 -> 100 / 0, x 2.
    Fit: (4000 - 2000) / 4000 and (8 - 4) / 8 -> 50.  BalancedAllocation 100.  InterPodAffinity 0.
    PodTopologySpread: two zones among the feasible nodes, weight log(4) = 1.386; raw round(1 x 1.386)
    = 1 on a, round(3 x 1.386) = 4 on c; normalised 100 x (4 + 1 - raw) / 4 = 100 / 25, x 2.
      a: 300 + 200 + 50 + 200 + 100 + 100 = 950        c: 300 + 0 + 50 + 50 + 100 + 0 = 500
    Pod 0 takes a.  A kernel that counted b in the ScheduleAnyway statistics would see three zones
    and a minimum count of 0: weight log(5) = 1.609, raw 2 / 5, normalised 100 x (5 + 0 - raw) / 5 =
    60 / 0, and a total of 870 on a.

    Pod 1: a now holds 8080 through pod 0's AssumePod, b still does: c alone is feasible and is
    taken without scoring.  Every node ends with the port's bit set."""
    cc, cp, _ = compile_cluster(*_edge_cluster())
    assert len(cc.ports) == 1 and cc.node_names == ["a", "b", "c"]
    assert all(cp.pods[j]["n_soft"] == 1 and cp.pods[j]["port_add"] == 1 for j in range(2))
    prof = abi.default_profile()
    ch_o, res, st = _oracle(cc, cp, prof)
    np.testing.assert_array_equal(ch_o, [0, 2])
    np.testing.assert_array_equal(res.fail_plugin[0, :3], [0, abi.KSS_F_NODE_PORTS, 0])
    np.testing.assert_array_equal(res.fail_plugin[1, :3], [abi.KSS_F_NODE_PORTS, abi.KSS_F_NODE_PORTS, 0])
    np.testing.assert_array_equal(res.total[0, [0, 2]], [950, 500])
    assert res.norm[0][abi.KSS_S_IMAGE_LOCALITY, 0] == 100 and res.raw[0][abi.KSS_S_NODE_AFFINITY, 0] == 8191
    np.testing.assert_array_equal(res.norm[0][abi.KSS_S_POD_TOPOLOGY_SPREAD, [0, 2]], [100, 25])
    assert [res.meta(j)[k] for j in range(2) for k in ("n_feasible", "scored", "best_total")] == [2, 1, 950, 1, 0, 0]
    np.testing.assert_array_equal(st["port_used"][:3], [1, 1, 1])
    native.set_option("shards", shards)
    native.set_option("spread_ports_images", 1)
    ctx = native.Context(prof)
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
    assert ctx.last_kernel() == "k_spread" and ctx.last_geometry()["shards"] == shards
    np.testing.assert_array_equal(chosen, [0, 2])
    meta = ctx.fetch_meta(2)
    assert list(meta[0]) == [0, 2, 1, 0, 950], list(meta[0])
    assert list(meta[1][:4]) == [2, 1, 0, 0], list(meta[1])
    np.testing.assert_array_equal(ctx.port_state(), [1, 1, 1])
    _check(ctx, cc, cp, ch_o, res, st, chosen)
    ctx.close()


# --------------------------------------------------------------------------------------
# 8. routing that stays put
# --------------------------------------------------------------------------------------
def test_option_off_runs_k_schedule():
    cc, cp, ch_o, res, st = _fuzz(4, 5, 40)
    _run(cc, cp, ch_o, res, st, kernel="k_schedule", on=0)


def test_option_turned_off_between_stage_and_run():
    """The option is process-wide and read twice: at the stage (records of the form) and again at the
    run.  Turned off in between, the staged batch runs on k_schedule, with the oracle's results."""
    cc, cp, ch_o, res, st = _fuzz(1, 12, 40)
    native.set_option("spread_ports_images", 1)
    assert native.plan_podset(cc.as_struct(), cp.as_struct())["kernel"] == "k_spread"
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    ctx.stage(cp.as_struct())
    native.set_option("spread_ports_images", 0)
    chosen = ctx.run_staged(cp.n)
    assert ctx.last_kernel() == "k_schedule" and ctx.last_spread_form() == (0, 0), (ctx.last_kernel(), ctx.last_spread_form())
    _check(ctx, cc, cp, ch_o, res, st, chosen)
    ctx.close()


def test_ungrafted_batch_is_untouched():
    """A batch without host ports and images launches the same kernel, geometry and LDS bytes with
    the option on and off, and leaves the same state."""
    cc, cp, _ = compile_cluster(*spf.make(20, 211, 150, grafted=False))
    assert not any(cp.pods[i]["port_conflict"] or cp.pods[i]["port_add"] or cp.pods[i]["img_len"] > 0
                   for i in range(cp.n))
    prof = abi.default_profile()
    ch_o, res, st = oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record="meta", threads=8,
                                      n_classes=len(cc.classes), n_terms=len(cc.terms))
    seen = []
    for on in (0, 1):
        native.set_option("spread_ports_images", on)
        ctx = native.Context(prof)
        ctx.load(cc.as_struct())
        chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
        _check(ctx, cc, cp, ch_o, res, st, chosen)
        seen.append((ctx.last_kernel(), ctx.last_geometry(), ctx.last_xcd_local(), ctx.last_spread_lds(),
                     ctx.last_timing()[1]))
        ctx.close()
    assert seen[0][0] == "k_spread" and seen[0][3] > 0 and seen[0] == seen[1], seen
