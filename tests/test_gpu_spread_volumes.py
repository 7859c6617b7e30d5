"""k_spread's volumes form (options spread_ports_images + spread_volumes: k_static_pi + k_static_vol +
k_spread_vol) against the C oracle, bit for bit: chosen nodes, every pod's outcome, the node rows,
class / term counts, UsedPorts, vol_count / vol_attached and, under the window, nextStartNodeIndex.

The batches are tests/spread_volume_fuzz.py's: progfuzz's programs with images, host ports and
volumes grafted on.  Every fuzz case first asserts on the oracle's own records what the batch reaches
-- pods with a VolumeRestrictions, limit-plugin, static (VolumeBinding / VolumeZone),
PodTopologySpread, InterPodAffinity and NodePorts failure, scored pods with a soft constraint or an
InterPodAffinity entry for which some node fails a volume filter, a changed vol_count -- and only
then runs the device.  Every case asserts last_kernel() == "k_spread" and last_spread_form()[0] == 2."""
import copy

import numpy as np
import pytest

import oracle_c
import spread_volume_fuzz as svf
import volume_fixtures as vf
import volume_form_fixtures as vff
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu
MODES = {"auto": 0, "single": abi.KSS_SCHED_FORCE_SINGLE_WG, "multi": abi.KSS_SCHED_FORCE_MULTI_WG}

# the oracle's own counts under the default profile: (scheduled, VR, limits, static, PTS, IPA, ports,
# soft-and-volume), keyed by (seed, nodes, pods, names_lists, pct)
REACH = {
    (1, 60, 200, True, 100): (166, 28, 67, 21, 110, 132, 49, 54),
    (2, 300, 300, True, 100): (219, 48, 101, 17, 165, 276, 73, 80),
    (20, 211, 150, True, 100): (129, 14, 47, 15, 68, 127, 36, 42),
    (21, 211, 150, True, 100): (106, 26, 53, 12, 87, 134, 40, 35),
    (20, 211, 150, False, 0): (130, 14, 47, 15, 71, 133, 37, 42),
    (2, 300, 300, False, 0): (221, 49, 105, 17, 168, 279, 74, 83),
}
# recorded from the oracle with the generator as committed (the issue lists only the soft-and-volume 39 of seed 22)
REACH_MORE = {
    (22, 211, 150, True, 100): (109, 29, 57, 9, 78, 135, 37, 39),
    (2, 300, 300, False, 50): (221, 49, 105, 17, 168, 279, 74, 83),
    (20, 211, 150, False, 50): (130, 14, 47, 15, 71, 133, 37, 42),
    (2, 300, 300, True, 0): (219, 48, 101, 17, 165, 276, 73, 80),
    (4, 12, 40, True, 100): (36, 2, 11, 3, 16, 13, 7, 9),
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


def _oracle(cc, cp, prof, n=None):
    return oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), cp.n if n is None else n, cc.n_nodes, record=True,
                             threads=8, n_classes=len(cc.classes), n_terms=len(cc.terms))


def _reach(cc, cp, ch_o, res):
    """What the oracle's records say the batch exercises (the columns of REACH)."""
    N = cc.n_nodes
    vr = lm = stc = pts = ipa = port = softvol = 0
    for j in range(cp.n):
        fp = res.fail_plugin[j, :N]
        dyn = np.isin(fp, vff.DYNAMIC).any()
        stat = np.isin(fp, vff.STATIC).any()
        vr += int((fp == abi.KSS_F_VOLUME_RESTRICTIONS).any())
        lm += int(np.isin(fp, vff.LIMITS).any())
        stc += int(stat)
        pts += int((fp == abi.KSS_F_POD_TOPOLOGY_SPREAD).any())
        ipa += int((fp == abi.KSS_F_INTER_POD_AFFINITY).any())
        port += int((fp == abi.KSS_F_NODE_PORTS).any())
        p = cp.pods[j]
        if res.meta(j)["scored"] and (int(p["n_soft"]) > 0 or int(p["ipa_len"]) > 0) and (dyn or stat):
            softvol += 1
    return int((np.asarray(ch_o) >= 0).sum()), vr, lm, stc, pts, ipa, port, softvol


_CACHE = {}


def _fuzz(seed, n_nodes, n_pods, names_lists=True, pct=100):
    """(cc, cp, oracle chosen, records, final state) of one grafted batch under the default profile,
    computed once and shared (nothing writes to them); its reach is asserted here, before any
    device run."""
    key = (seed, n_nodes, n_pods, names_lists, pct)
    if key not in _CACHE:
        nodes, bound, pods, stg = svf.make(seed, n_nodes, n_pods, names_lists=names_lists)
        cc, cp, _ = compile_cluster(nodes, bound, pods, storage=stg)
        prof = _prof(pct)
        ch_o, res, st = _oracle(cc, cp, prof)
        reach = _reach(cc, cp, ch_o, res)
        cs = cc.as_struct()
        print("reach", key, reach, "rows", cs.n_vol_rows, "keys", cs.n_vol_keys)
        assert reach == (REACH.get(key) or REACH_MORE[key]), (key, reach)
        assert all(v > 0 for v in reach[1:6]) and reach[7] > 0, reach
        assert (st["vol_count"] != cc.arrays["vol_count"][:st["vol_count"].shape[0], :st["vol_count"].shape[1]]).any()
        assert cs.n_vol_rows <= 64 and cs.n_vol_keys <= 8
        _CACHE[key] = (cc, cp, ch_o, res, st)
    return _CACHE[key]


def _state_equal(ctx, cc, st):
    N, ncl, nt = cc.n_nodes, len(cc.classes), len(cc.terms)
    np.testing.assert_array_equal(ctx.port_state(), st["port_used"][:N])
    g = ctx.node_state()
    np.testing.assert_array_equal(g["requested"][:, :N], st["requested"][:, :N])
    np.testing.assert_array_equal(g["nonzero"][:, :N], st["nonzero"][:, :N])
    np.testing.assert_array_equal(g["pod_count"][:N], st["pod_count"][:N])
    if ncl:
        np.testing.assert_array_equal(g["class_count"][:ncl], st["class_count"][:ncl])
    if nt:
        np.testing.assert_array_equal(g["term_count"][:nt], st["term_count"][:nt])
    vc, va = ctx.volume_state()
    np.testing.assert_array_equal(vc, st["vol_count"])
    np.testing.assert_array_equal(va, st["vol_attached"])


def _check(ctx, cc, cp, ch_o, res, st, chosen, cursor=False, n=None):
    n = cp.n if n is None else n
    np.testing.assert_array_equal(chosen, ch_o[:n])
    meta = ctx.fetch_meta(n)
    for j in range(n):
        m = res.meta(j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], (j, meta[j, 4], m["best_total"])
    _state_equal(ctx, cc, st)
    if cursor:
        assert ctx.next_start_node_index() == st["next_start"]


def _run(cc, cp, ch_o, res, st, prof=None, flags=0, form=True, cursor=False, on=1):
    """One batch on a fresh context against the oracle; form: the volumes form must have run (else
    k_schedule must have).  Returns what the launch reports."""
    native.set_option("spread_ports_images", 1)
    native.set_option("spread_volumes", on)
    ctx = native.Context(prof or abi.default_profile())
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n, flags=flags)
    f = ctx.last_spread_form()
    if form:
        assert ctx.last_kernel() == "k_spread" and f[0] == 2 and f[1] > 0, (ctx.last_kernel(), f)
        assert f[1] == ctx.last_spread_lds()
    else:
        assert ctx.last_kernel() == "k_schedule" and f == (0, 0), (ctx.last_kernel(), f)
    _check(ctx, cc, cp, ch_o, res, st, chosen, cursor=cursor)
    info = dict(ctx.last_geometry(), xcd=ctx.last_xcd_local(), launches=ctx.last_timing()[1], lds=f[1],
                retries=ctx.last_handoff_retries(), handoff=ctx.last_handoff_status())
    ctx.close()
    print("launch", info)
    return info


# --------------------------------------------------------------------------------------
# 1. modes
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster,mode", [((1, 60, 200), "auto"), ((1, 60, 200), "single"), ((1, 60, 200), "multi"),
                                          ((2, 300, 300), "auto"), ((2, 300, 300), "multi")],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d" % v[1:])
def test_modes(cluster, mode):
    cc, cp, ch_o, res, st = _fuzz(*cluster)
    info = _run(cc, cp, ch_o, res, st, flags=MODES[mode])
    if mode == "single":
        assert info["shards"] == 1, info
    if mode == "multi":
        assert info["shards"] > 1, info


# --------------------------------------------------------------------------------------
# 2. nine shards, ragged last shard (211 = 8 x 24 + 19)
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [20, 21, 22])
def test_nine_shards(seed):
    cc, cp, ch_o, res, st = _fuzz(seed, 211, 150)
    native.set_option("shards", 9)
    info = _run(cc, cp, ch_o, res, st)
    assert info["shards"] == 9 and info["xcd"]["used"] == 0, info


# a shard count through nodes_per_shard leaves the placement to the library: the XCD-local grid, the
# same with xcd = 0, and the placement reported failed (xcd_force_fallback: every launch runs again
# unrestricted, the err = 3 retry, on packed columns the refused launch has not touched)
@pytest.mark.parametrize("seed,kind", [(20, "xcd-local"), (21, "xcd-off"), (22, "xcd-fallback")])
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
# 3. workgroup bounds: the kernels built for <= 256 lanes and for KSS_MAX_THREADS
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster,opts,lb256", [((20, 211, 150), dict(shards=3, force_threads=128), True),
                                                ((2, 300, 300), dict(shards=2, force_threads=320), False)],
                         ids=["lb256", "320-lanes"])
def test_workgroup_bounds(cluster, opts, lb256):
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
    """numFeasibleNodesToFind is 144 of 300 and 103 of 211 at pct 0, 150 and 105 at pct 50: below N, and
    the largest n_feasible reaches it, so the window cuts."""
    cc, cp, ch_o, res, st = _fuzz(*cluster, names_lists=False, pct=pct)
    N = cc.n_nodes
    k_find = {(300, 0): 144, (211, 0): 103, (300, 50): 150, (211, 50): 105}[(N, pct)]
    feas = [res.meta(j)["n_feasible"] for j in range(cp.n)]
    assert max(feas) == k_find < N, (max(feas), k_find)
    native.set_option("shards", 9 if N == 211 else 0)
    _run(cc, cp, ch_o, res, st, prof=_prof(pct), cursor=True)


def test_window_with_name_lists_stays_on_k_schedule():
    cc, cp, ch_o, res, st = _fuzz(2, 300, 300, names_lists=True, pct=0)
    assert any(cp.pods[i]["names_len"] >= 0 for i in range(cp.n))
    _run(cc, cp, ch_o, res, st, prof=_prof(0), form=False, cursor=True)


# --------------------------------------------------------------------------------------
# 5. chunks: the volume columns carried from launch to launch through the checked hand-off
# --------------------------------------------------------------------------------------
def test_chunked_batch_carries_volume_columns():
    cc, cp, ch_o, res, st = _fuzz(20, 211, 150)
    native.set_option("shards", 9)
    native.set_option("static_bytes", 4 * 211 * 23)  # 23 pods per chunk
    info = _run(cc, cp, ch_o, res, st)
    chunks = (150 + 22) // 23
    # k_static_pi + k_static_vol + k_spread_vol per chunk, then k_vol_unpack + k_vol_counts: 3 x 7 + 2 = 23
    assert info["launches"] == 3 * chunks + 2 == 23, info
    print("hand-off retries", info["retries"], info["handoff"])  # reported, not asserted to be zero


# --------------------------------------------------------------------------------------
# 6. runtime profile: the DEF = false kernels
# --------------------------------------------------------------------------------------
def test_runtime_profile():
    """VolumeRestrictions and the EBS limit plugin disabled (their AssumePod still recorded), ImageLocality
    weight 5: the other limit plugins still decide."""
    prof = abi.default_profile()
    prof.weight[abi.KSS_S_IMAGE_LOCALITY] = 5
    prof.filter_enabled &= ~((1 << abi.KSS_F_VOLUME_RESTRICTIONS) | (1 << abi.KSS_F_EBS_LIMITS))
    nodes, bound, pods, stg = svf.make(21, 211, 150)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=stg)
    ch_o, res, st = _oracle(cc, cp, prof)
    reach = _reach(cc, cp, ch_o, res)
    print("reach runtime profile", reach)
    N = cc.n_nodes
    assert reach[1] == 0 and reach[2] > 0 and reach[3] > 0 and reach[4] > 0 and reach[5] > 0, reach
    assert not (res.fail_plugin[:, :N] == abi.KSS_F_EBS_LIMITS).any()
    assert (st["vol_count"] != cc.arrays["vol_count"][:st["vol_count"].shape[0], :st["vol_count"].shape[1]]).any()
    native.set_option("shards", 9)
    info = _run(cc, cp, ch_o, res, st, prof=prof)
    assert info["shards"] == 9


# --------------------------------------------------------------------------------------
# 7. row 63: the used-rows word's top bit
# --------------------------------------------------------------------------------------
def test_row_63():
    """Wider pools of shared claims and inline disks (28 claims, 18 EBS, 9 GCE PD disks on seed 20's
    211 x 150) give exactly 64 volume rows; row 63 is in a pending pod's own mask and held on a node at
    load."""
    nodes, bound, pods, stg = svf.make(20, 211, 150, n_claims=28, n_ebs=18, n_gce=9)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=stg)
    assert cc.as_struct().n_vol_rows == 64
    top = 1 << 63
    masks = [vff.pod_masks(cc, cp, j) for j in range(cp.n)]
    assert any(m[2] & top for m in masks) and any(m[1] & top for m in masks)
    assert (cc.arrays["vol_count"][63][:cc.n_nodes] > 0).any()  # some node's initial used word holds bit 63
    prof = abi.default_profile()
    ch_o, res, st = _oracle(cc, cp, prof)
    reach = _reach(cc, cp, ch_o, res)
    print("reach row 63", reach)
    assert reach == (126, 14, 48, 17, 70, 124, 37, 43), reach
    assert (st["vol_count"][63] != cc.arrays["vol_count"][63][:cc.n_nodes]).any()  # ... and a commit sets it
    native.set_option("shards", 9)
    _run(cc, cp, ch_o, res, st)


# --------------------------------------------------------------------------------------
# 8. state hand-over: what a batch in the form leaves is what k_schedule would have left
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", [1, 0], ids=["then-k_spread", "then-k_schedule"])
def test_state_hand_over(second):
    """Pods [0, 100) on the form; then pods 100 .. 119 one by one (kss_eval_pod + commit) and pods
    [120, 150) as a second batch (the form again, or k_schedule with the option off), continuing the
    oracle; volume_state() equal after each step."""
    import ctypes as C
    cc, cp, ch_all, res_all, st_all = _fuzz(20, 211, 150)
    prof = abi.default_profile()
    N = cc.n_nodes
    n1, n2 = 100, 120
    steps = {n: _oracle(cc, cp, prof, n=n)[2] for n in (n1, n2)}
    native.set_option("spread_ports_images", 1)
    native.set_option("spread_volumes", 1)
    native.set_option("shards", 9)
    ctx = native.Context(prof)
    ctx.load(cc.as_struct())
    ctx.stage(cp.as_struct())
    chosen = ctx.run_staged(n1)
    assert ctx.last_kernel() == "k_spread" and ctx.last_spread_form()[0] == 2
    np.testing.assert_array_equal(chosen, ch_all[:n1])
    _state_equal(ctx, cc, steps[n1])
    seen = 0
    for j in range(n1, n2):
        r = ctx.eval_pod(cp.as_struct(), j)
        np.testing.assert_array_equal(r.fail_plugin[:N], res_all.fail_plugin[j, :N])
        m = res_all.meta(j)
        assert r.chosen == m["chosen"], (j, r.chosen, m)
        seen += int(np.isin(res_all.fail_plugin[j, :N], vff.DYNAMIC).any())
        if m["chosen"] >= 0:
            ctx.commit(cp.as_struct(), j, int(m["chosen"]))
    assert seen > 0
    vc, va = ctx.volume_state()
    np.testing.assert_array_equal(vc, steps[n2]["vol_count"])
    np.testing.assert_array_equal(va, steps[n2]["vol_attached"])
    # the second batch: pods [120, 150) of the same pools (the records index them, so they are shared)
    ps = cp.as_struct()
    tail = abi.PodSet.from_buffer_copy(ps)
    tail.pods = C.cast(C.addressof(ps.pods.contents) + n2 * C.sizeof(abi.Pod), C.POINTER(abi.Pod))
    tail.n_pods = cp.n - n2
    assert any(cp.pods[j]["vol_len"] > 0 for j in range(n2, cp.n))
    native.set_option("spread_volumes", second)
    chosen2 = ctx.schedule_batch(tail, cp.n - n2)
    if second:
        assert ctx.last_kernel() == "k_spread" and ctx.last_spread_form()[0] == 2
    else:
        assert ctx.last_kernel() == "k_schedule" and ctx.last_spread_form() == (0, 0)
    np.testing.assert_array_equal(chosen2, ch_all[n2:])
    _state_equal(ctx, cc, st_all)
    ctx.close()


# --------------------------------------------------------------------------------------
# 9. the word-and-statistics edge, hand-derived
# --------------------------------------------------------------------------------------
MI = 1024 * 1024


def _edge_cluster():
    def node(name, zone, pref, images=None, ebs=None):
        alloc = {"cpu": "4", "memory": "8Gi", "pods": "20", "ephemeral-storage": "20Gi"}
        if ebs is not None:
            alloc["attachable-volumes-aws-ebs"] = str(ebs)
        status = {"allocatable": alloc}
        if images:
            status["images"] = images
        labels = {"kubernetes.io/hostname": name, "topology.kubernetes.io/zone": zone}
        if pref:
            labels["pref"] = "yes"
        return {"metadata": {"name": name, "labels": labels}, "spec": {}, "status": status}

    def ctr(image):
        return {"name": "c", "image": image, "resources": {"requests": {"cpu": "500m", "memory": "1Gi"}}}

    big = [{"names": ["big:1"], "sizeBytes": 9000 * MI}]
    nodes = [node("a", "z1", True, big, ebs=2), node("b", "z3", True, big, ebs=1), node("c", "z2", False, ebs=2)]
    bound = []
    for nm, apps in (("a", "xyy"), ("b", "yyy"), ("c", "xxx")):
        for i, app in enumerate(apps):
            spec = {"nodeName": nm, "containers": [ctr("none:1")]}
            if nm == "b" and i == 0:
                spec["volumes"] = [dict(vf.ebs("vol-held"), name="v0")]
            bound.append({"metadata": {"name": "%s%d" % (nm, i), "namespace": "default", "labels": {"app": app}}, "spec": spec})
    pref = {"matchExpressions": [{"key": "pref", "operator": "In", "values": ["yes"]}]}
    spec = {"containers": [ctr("big:1")],
            "volumes": [dict(vf.ebs("vol-p"), name="v0")],
            "affinity": {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
                {"weight": 8091, "preference": pref}, {"weight": 100, "preference": pref}]}},
            "topologySpreadConstraints": [{"maxSkew": 1, "topologyKey": "topology.kubernetes.io/zone",
                                           "whenUnsatisfiable": "ScheduleAnyway",
                                           "labelSelector": {"matchLabels": {"app": "x"}}}]}
    pods = [{"metadata": {"name": "p%d" % j, "namespace": "default", "labels": {"app": "p"}}, "spec": copy.deepcopy(spec)}
            for j in range(2)]
    return nodes, bound, pods, vf.storage([], [], [], [])


@pytest.mark.parametrize("shards", [1, 3])
def test_word_edges(shards):
    """tests/test_gpu_spread_portimage.py::test_word_edges' cluster with the host port replaced by volumes:
    three equal nodes (4 cpu, 8 Gi), three bound pods of 500m / 1 Gi on each; two identical pending pods
    (500m / 1 Gi, image big:1, inline EBS vol-p, preferred NodeAffinity 8091 + 100 = 8191 on pref=yes,
    ScheduleAnyway zone spread over app=x).

      a  zone z1, pref=yes, lists big:1, EBS limit 2, one app=x pod
      b  zone z3, pref=yes, lists big:1, EBS limit 1, no app=x pod, a bound pod holds inline EBS vol-held
      c  zone z2, no label, no image, EBS limit 2, three app=x pods

    b is best on every score -- NodeAffinity 8191, ImageLocality 100, an empty zone -- and fails
    EBSLimits: one volume attached, one new, limit 1.

    Pod 0, feasible {a, c}.  TaintToleration 100 x 3.  NodeAffinity raw 8191 / 0 -> 100 / 0, x 2.  Fit 50.
    BalancedAllocation 100.  InterPodAffinity 0.  ImageLocality 100 / 0.  PodTopologySpread: two zones among
    the feasible nodes, weight log(4) = 1.386; raw round(1 x 1.386) = 1 on a, round(3 x 1.386) = 4 on c;
    normalised 100 x (4 + 1 - raw) / 4 = 100 / 25, x 2.
      a: 300 + 200 + 50 + 200 + 100 + 100 = 950        c: 300 + 0 + 50 + 50 + 100 + 0 = 500
    Pod 0 takes a.  A kernel that counted b among the ScheduleAnyway filteredNodes would see three zones and a
    minimum count of 0: weight log(5) = 1.609, raw 2 / 5, normalised 100 x (5 + 0 - raw) / 5 = 60 / 0, and a
    total of 870 on a.

    Pod 1: a now holds vol-p read-write through pod 0's AssumePod (VolumeRestrictions), b still exceeds its
    limit: c alone is feasible and is taken without scoring.  Every node ends with one EBS volume attached."""
    nodes, bound, pods, stg = _edge_cluster()
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=stg)
    assert cc.node_names == ["a", "b", "c"]
    assert all(cp.pods[j]["n_soft"] == 1 and cp.pods[j]["vol_len"] > 0 for j in range(2))
    prof = abi.default_profile()
    ch_o, res, st = _oracle(cc, cp, prof)
    np.testing.assert_array_equal(ch_o, [0, 2])
    np.testing.assert_array_equal(res.fail_plugin[0, :3], [0, abi.KSS_F_EBS_LIMITS, 0])
    np.testing.assert_array_equal(res.fail_plugin[1, :3], [abi.KSS_F_VOLUME_RESTRICTIONS, abi.KSS_F_EBS_LIMITS, 0])
    np.testing.assert_array_equal(res.total[0, [0, 2]], [950, 500])
    np.testing.assert_array_equal(res.norm[0][abi.KSS_S_POD_TOPOLOGY_SPREAD, [0, 2]], [100, 25])
    assert [res.meta(j)[k] for j in range(2) for k in ("n_feasible", "scored", "best_total")] == [2, 1, 950, 1, 0, 0]
    ebs = [k for k in range(cc.as_struct().n_vol_keys) if int(cc.arrays["vol_key_plugin"][k]) == abi.KSS_F_EBS_LIMITS]
    assert len(ebs) == 1
    np.testing.assert_array_equal(st["vol_attached"][ebs[0], :3], [1, 1, 1])
    native.set_option("shards", shards)
    native.set_option("spread_ports_images", 1)
    native.set_option("spread_volumes", 1)
    ctx = native.Context(prof)
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
    assert ctx.last_kernel() == "k_spread" and ctx.last_spread_form()[0] == 2
    assert ctx.last_geometry()["shards"] == shards
    np.testing.assert_array_equal(chosen, [0, 2])
    meta = ctx.fetch_meta(2)
    assert list(meta[0]) == [0, 2, 1, 0, 950], list(meta[0])
    assert list(meta[1][:4]) == [2, 1, 0, 0], list(meta[1])
    np.testing.assert_array_equal(ctx.volume_state()[1][ebs[0], :3], [1, 1, 1])
    _check(ctx, cc, cp, ch_o, res, st, chosen)
    ctx.close()


# --------------------------------------------------------------------------------------
# 10. routing that stays put
# --------------------------------------------------------------------------------------
def test_option_off_runs_k_schedule():
    cc, cp, ch_o, res, st = _fuzz(1, 60, 200)
    _run(cc, cp, ch_o, res, st, form=False, on=0)


def test_option_turned_off_between_stage_and_run():
    """spread_volumes is process-wide and read twice: at the stage (records of the volumes form) and
    again at the run.  Turned off in between, the staged batch runs on k_schedule, with the oracle's
    results."""
    cc, cp, ch_o, res, st = _fuzz(4, 12, 40)
    native.set_option("spread_ports_images", 1)
    native.set_option("spread_volumes", 1)
    assert native.plan_podset(cc.as_struct(), cp.as_struct())["kernel"] == "k_spread"
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    ctx.stage(cp.as_struct())
    native.set_option("spread_volumes", 0)
    chosen = ctx.run_staged(cp.n)
    f = ctx.last_spread_form()
    assert ctx.last_kernel() == "k_schedule" and f == (0, 0), (ctx.last_kernel(), f)
    _check(ctx, cc, cp, ch_o, res, st, chosen)
    ctx.close()


def test_batch_without_volume_pods_is_untouched():
    """A batch with programs, host ports and images but no volume pod launches the same kernel, geometry,
    LDS bytes and launch count with the option on and off, and leaves the same state."""
    import spread_portimage_fuzz as spf
    cc, cp, _ = compile_cluster(*spf.make(20, 211, 150))
    assert not any(cp.pods[i]["vol_len"] > 0 for i in range(cp.n))
    prof = abi.default_profile()
    ch_o, res, st = oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record="meta", threads=8,
                                      n_classes=len(cc.classes), n_terms=len(cc.terms))
    native.set_option("spread_ports_images", 1)
    seen = []
    for on in (0, 1):
        native.set_option("spread_volumes", on)
        ctx = native.Context(prof)
        ctx.load(cc.as_struct())
        chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
        _check(ctx, cc, cp, ch_o, res, st, chosen)
        seen.append((ctx.last_kernel(), ctx.last_geometry(), ctx.last_xcd_local(), ctx.last_spread_form(),
                     ctx.last_timing()[1]))
        ctx.close()
    assert seen[0][0] == "k_spread" and seen[0][3][0] == 1 and seen[0][3][1] > 0 and seen[0] == seen[1], seen
