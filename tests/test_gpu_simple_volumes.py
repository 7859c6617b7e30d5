"""k_simple's volumes form (options simple_ports_images + simple_volumes: k_static_pi + k_static_vol +
k_simple_vol) against the C oracle, bit for bit: chosen nodes, every pod's outcome, the node rows,
vol_count / vol_attached and UsedPorts.  Every case also runs with simple_volumes 0 (k_schedule)
for the same results.

The dynamic volume filters are state of the loop (per node slot one used-rows word and packed
attached counters in LDS: filter, AssumePod, the H1 re-evaluation on the state after the previous
pod's commit); VolumeBinding's bound-claim checks and VolumeZone are in the static word.  Every fuzz
case first asserts, from the oracle's own records and a replay of its choices
(volume_form_fixtures.reach), that the batch reaches VolumeRestrictions failures, limit-plugin
failures, static VolumeBinding / VolumeZone failures and H1 pairs."""
import numpy as np
import pytest

import oracle_c
import volume_form_fixtures as vff
import volume_fuzz
import volume_portimage_fuzz
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _oracle(cc, cp, prof=None):
    return oracle_c.schedule(prof or abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes,
                             record=True, n_classes=len(cc.classes), n_terms=len(cc.terms))


_CACHE = {}


def _case(key, made, prof=None):
    """(cc, cp, oracle chosen, records, final state, reach) of one cluster, computed once and shared
    (nothing writes to them)."""
    if key not in _CACHE:
        nodes, bound, pods, st = made()
        cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
        ch_o, res, fin = _oracle(cc, cp, prof)
        _CACHE[key] = (cc, cp, ch_o, res, fin, vff.reach(cc, cp, ch_o, res, prof))
    return _CACHE[key]


def _fuzz(seed, n_nodes=12, n_bound=16, n_pods=40):
    return _case(("fuzz", seed, n_nodes, n_bound, n_pods),
                 lambda: volume_fuzz.make(seed, n_nodes=n_nodes, n_bound=n_bound, n_pods=n_pods))


def _assert_reach(r):
    got = {k: r[k] for k in ("restrictions", "limits", "static", "h1")}
    print("reach", got)
    assert all(v > 0 for v in got.values()), got


def _meta_equal(meta, res, n):
    for j in range(n):
        m = res.meta(j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], j


def _state_equal(ctx, cc, fin):
    N = cc.n_nodes
    g = ctx.node_state()
    np.testing.assert_array_equal(g["requested"][:, :N], fin["requested"][:, :N])
    np.testing.assert_array_equal(g["nonzero"][:, :N], fin["nonzero"][:, :N])
    np.testing.assert_array_equal(g["pod_count"][:N], fin["pod_count"][:N])
    vc, va = ctx.volume_state()
    np.testing.assert_array_equal(vc, fin["vol_count"])
    np.testing.assert_array_equal(va, fin["vol_attached"])
    np.testing.assert_array_equal(ctx.port_state(), fin["port_used"][:N])


def _run(cc, cp, ch_o, res, fin, prof=None, flags=0, form=True, keep=False):
    """One batch on a fresh context against the oracle.  form: the volumes form must have run (else
    k_schedule must have).  Returns (launch count, geometry[, the context])."""
    ctx = native.Context(prof or abi.default_profile())
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n, flags=flags)
    f = ctx.last_simple_form()
    if form:
        assert ctx.last_kernel() == "k_simple" and f["volumes"] == 1 and f["lds_bytes"] > 0, (ctx.last_kernel(), f)
        assert ctx.last_shape_table()["shapes"] == 0
    else:
        assert ctx.last_kernel() == "k_schedule" and f == {"volumes": 0, "lds_bytes": 0}, (ctx.last_kernel(), f)
    np.testing.assert_array_equal(chosen, ch_o)
    _meta_equal(ctx.fetch_meta(cp.n), res, cp.n)
    _state_equal(ctx, cc, fin)
    launches = ctx.last_timing()[1]
    geom = dict(ctx.last_geometry(), xcd_local=ctx.last_xcd_local()["used"], fallbacks=ctx.last_xcd_local()["fallbacks"])
    if keep:
        return launches, geom, ctx
    ctx.close()
    return launches, geom


def _both(cc, cp, ch_o, res, fin, prof=None, flags=0):
    """The form, then the same batch with simple_volumes 0 on k_schedule."""
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    out = _run(cc, cp, ch_o, res, fin, prof=prof, flags=flags)
    native.set_option("simple_volumes", 0)
    _run(cc, cp, ch_o, res, fin, prof=prof, flags=flags, form=False)
    return out


# --------------------------------------------------------------------------------------
# 1. fuzz over geometries (those of test_gpu_simple_portimage.py)
# --------------------------------------------------------------------------------------
GEOMETRIES = (
    [("small-%d" % s, (s, 12, 16, 40), dict(shards=1), abi.KSS_SCHED_FORCE_SINGLE_WG, 1) for s in (2, 4, 6)]
    + [("one-wave", (31, 40, 30, 120), dict(shards=2, force_threads=64), 0, 2),
       ("pw-2-waves", (11, 300, 300, 200), dict(shards=3, force_threads=128), 0, 3),
       ("pw-3-waves", (11, 300, 300, 200), dict(shards=3, force_threads=192), 0, 3),
       ("nine-shards", (11, 300, 300, 200), dict(shards=9), 0, 9),
       ("slots-per-lane", (11, 300, 300, 200), dict(shards=1, force_threads=64), 0, 1)])
# H1 pairs of these clusters, counted by hand from the oracle when the cases were chosen
H1 = {(2, 12, 16, 40): 3, (4, 12, 16, 40): 1, (6, 12, 16, 40): 1, (31, 40, 30, 120): 3, (11, 300, 300, 200): 3}
CASES = [g + (x,) for g in GEOMETRIES for x in ((1, 0) if g[4] > 1 else (0,))]


def _bit63(cc, cp, r):
    """Row 63 is live: in a pending pod's LIMIT and OWN masks and held on some node at load."""
    assert cc.as_struct().n_vol_rows == 64
    top = 1 << 63
    masks = [vff.pod_masks(cc, cp, j) for j in range(cp.n)]
    assert any(m[1] & top for m in masks) and any(m[2] & top for m in masks)
    assert (cc.arrays["vol_count"][63][:cc.n_nodes] > 0).any()


@pytest.mark.parametrize("name,cluster,opts,flags,shards,xcd", CASES,
                         ids=["%s-%s" % (c[0], "xcd" if c[5] else "plain") for c in CASES])
def test_fuzz_geometries(name, cluster, opts, flags, shards, xcd):
    cc, cp, ch_o, res, fin, r = _fuzz(*cluster)
    _assert_reach(r)
    assert r["h1"] == H1[cluster], r["h1"]
    if cluster[1] == 300:
        _bit63(cc, cp, r)
    native.set_option("xcd", xcd)
    for k, v in opts.items():
        if k == "shards" and xcd:
            native.set_option("nodes_per_shard", (cluster[1] + v - 1) // v)
        else:
            native.set_option(k, v)
    _, geom = _both(cc, cp, ch_o, res, fin, flags=flags)
    assert geom["shards"] == shards and geom["xcd_local"] == xcd, geom
    if "force_threads" in opts:
        assert geom["threads"] == opts["force_threads"], geom
    if name == "slots-per-lane":
        assert geom["nodes_per_lane"] > 1, geom


# --------------------------------------------------------------------------------------
# 2. chunked launches: the packed columns carried from launch to launch
# --------------------------------------------------------------------------------------
def test_chunked_batch_carries_volume_state():
    cc, cp, ch_o, res, fin, r = _fuzz(11, 300, 300, 200)
    _assert_reach(r)
    _bit63(cc, cp, r)
    native.set_option("shards", 3)
    native.set_option("static_bytes", 4 * cc.n_nodes * 60)  # 60 pods per chunk: 4 chunk launches
    launches, _ = _both(cc, cp, ch_o, res, fin)
    assert launches >= 2 * 3, launches  # k_static + the loop kernel per chunk, at least 3 chunks


# --------------------------------------------------------------------------------------
# 3. the XCD-local placement reported failed: the unrestricted rerun finds the state untouched
# --------------------------------------------------------------------------------------
def test_xcd_fallback_leaves_state_untouched():
    cc, cp, ch_o, res, fin, r = _fuzz(11, 300, 300, 200)
    _assert_reach(r)
    native.set_option("xcd", 1)
    native.set_option("nodes_per_shard", 100)
    native.set_option("xcd_force_fallback", 1)
    _, geom = _both(cc, cp, ch_o, res, fin)
    assert geom["shards"] == 3 and geom["xcd_local"] == 1 and geom["fallbacks"] >= 1, geom


# --------------------------------------------------------------------------------------
# 4. private volumes, hand-built
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 2])
def test_private_volumes(shards):
    """Six nodes that attach two EBS volumes each, sixteen identical pods with an EBS volume of
    their own: twelve find a slot, four do not, and a pod that takes a node's last slot is followed by
    one that must see it (H1).  Pod 0 is pinned to n0 and names only a CSI volume that a bound pod
    holds there, where the driver's limit (0) is exceeded: NodeVolumeLimits skips a key without a
    new volume, so it is scheduled."""
    cc, cp, ch_o, res, fin, r = _case("private", vff.private_ebs)
    kinds = [{int(cp.vols[int(cp.pods[j]["vol_off"]) + e]["kind"]): int(cp.vols[int(cp.pods[j]["vol_off"]) + e]["row"])
              for e in range(int(cp.pods[j]["vol_len"]))} for j in range(cp.n)]
    for j in range(1, cp.n):
        assert kinds[j].get(abi.KSS_VOL_LIMIT, 0) < 0 and abi.KSS_VOL_OWN_PRIVATE in kinds[j], (j, kinds[j])
    assert sum(int(c >= 0) for c in ch_o[1:]) == 12 and sum(int(c < 0) for c in ch_o[1:]) == 4, list(ch_o)
    assert r["limits"] > 0 and r["h1"] > 0, r
    # pod 0: a shared CSI row, attached on n0 beyond the limit, and still feasible there
    K = cc.as_struct().n_vol_keys
    csi = [k for k in range(K) if cc.arrays["vol_key_plugin"][k] == abi.KSS_F_NODE_VOLUME_LIMITS]
    assert len(csi) == 1 and cc.arrays["vol_attached"][csi[0]][0] == 1 and cc.arrays["vol_limit"][csi[0]][0] == 0
    m0 = vff.pod_masks(cc, cp, 0)
    assert m0[1] and (m0[3] >> csi[0]) & 1 and m0[4][csi[0]] == 0 and ch_o[0] == 0
    native.set_option("shards", shards)
    _, geom = _both(cc, cp, ch_o, res, fin)
    assert geom["shards"] == shards


# --------------------------------------------------------------------------------------
# 5. a runtime profile (the DEF = false kernels); the window stays on k_schedule
# --------------------------------------------------------------------------------------
def _profile():
    p = abi.default_profile()
    p.filter_enabled &= ~(1 << abi.KSS_F_VOLUME_RESTRICTIONS)
    p.filter_enabled &= ~(1 << abi.KSS_F_NODE_VOLUME_LIMITS)
    p.weight[abi.KSS_S_TAINT_TOLERATION] = 1
    p.weight[abi.KSS_S_NODE_RESOURCES_FIT] = 3
    p.weight[abi.KSS_S_BALANCED_ALLOCATION] = 2
    return p


def test_runtime_profile():
    prof = _profile()
    cc, cp, ch_o, res, fin, r = _case("profile", lambda: volume_fuzz.make(31, n_nodes=40, n_bound=30, n_pods=120), prof)
    N = cc.n_nodes
    fails = set(int(x) for x in np.unique(res.fail_plugin[:, :N]))
    assert abi.KSS_F_VOLUME_RESTRICTIONS not in fails and abi.KSS_F_NODE_VOLUME_LIMITS not in fails
    assert r["limits"] > 0 and r["static"] > 0 and r["h1"] > 0, r  # the enabled limit plugins still decide
    d = _fuzz(31, 40, 30, 120)
    assert not np.array_equal(ch_o, d[2])  # ... and the profile changes the choices
    native.set_option("shards", 2)
    _both(cc, cp, ch_o, res, fin, prof=prof)


@pytest.mark.parametrize("pct", [0, 30])
def test_window_runs_on_k_schedule(pct):
    """No window instantiation of the form: a batch whose search is windowed stays on k_schedule."""
    prof = abi.default_profile()
    prof.pct_nodes_to_score = pct
    cc, cp, ch_o, res, fin, _ = _case(("window", pct), lambda: volume_fuzz.make(11, n_nodes=300, n_bound=300, n_pods=200), prof)
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    native.set_option("shards", 3)
    plan = native.plan_podset(cc.as_struct(), cp.as_struct(), prof)
    assert plan["kernel"] == "k_schedule" and "percentageOfNodesToScore" in plan["reason"], plan
    _, _, ctx = _run(cc, cp, ch_o, res, fin, prof=prof, form=False, keep=True)
    assert ctx.next_start_node_index() == fin["next_start"]
    ctx.close()


# --------------------------------------------------------------------------------------
# 6. volumes, host ports and images in one batch
# --------------------------------------------------------------------------------------
def _reach_ports_images(cc, cp, ch_o, res):
    """Pods with a NodePorts failure; pods whose choice is not the argmax of total - ImageLocality."""
    N = cc.n_nodes
    prof = abi.default_profile()
    w_il = prof.weight[abi.KSS_S_IMAGE_LOCALITY]
    port_pods = il_pods = 0
    for j in range(cp.n):
        fp = res.fail_plugin[j, :N]
        port_pods += int((fp == abi.KSS_F_NODE_PORTS).any())
        m = res.meta(j)
        if m["scored"]:
            kept = (fp == 0) & (res.fail_detail[j, :N] != abi.KSS_PASS_NOT_KEPT)
            rest = np.where(kept, res.total[j, :N] - w_il * res.norm[j][abi.KSS_S_IMAGE_LOCALITY, :N], -1)
            il_pods += int(np.argmax(rest) != m["chosen"])
    return port_pods, il_pods


def test_volumes_ports_and_images_together():
    cc, cp, ch_o, res, fin, r = _case("all-three", lambda: volume_portimage_fuzz.make(31, n_nodes=40, n_bound=30, n_pods=120))
    _assert_reach(r)
    port_pods, il_pods = _reach_ports_images(cc, cp, ch_o, res)
    print("ports / images reach", port_pods, il_pods)
    assert port_pods > 0 and il_pods > 0
    assert (fin["port_used"][:cc.n_nodes] != cc.arrays["port_used"][:cc.n_nodes]).any()
    native.set_option("shards", 3)
    _, geom = _both(cc, cp, ch_o, res, fin)
    assert geom["shards"] == 3


# --------------------------------------------------------------------------------------
# 7. state hand-over: what a batch in the form leaves is what k_schedule would have left
# --------------------------------------------------------------------------------------
def test_state_hand_over():
    """After a batch in the form: the per-pod evaluation of further volume pods equals the oracle
    continued from the same state, and after reset() the staged batch reproduces the first run."""
    nodes, bound, pods, st = volume_fuzz.make(31, n_nodes=40, n_bound=30, n_pods=120)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    n1 = 100  # the batch: pods [0, 100) of the staged list; then pods 100 .. 119 one by one
    prof = abi.default_profile()
    ch_all, res_all, _ = _oracle(cc, cp)
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    native.set_option("shards", 2)
    ctx = native.Context(prof)
    ctx.load(cc.as_struct())
    ctx.stage(cp.as_struct())
    chosen = ctx.run_staged(n1)
    assert ctx.last_kernel() == "k_simple" and ctx.last_simple_form()["volumes"] == 1
    np.testing.assert_array_equal(chosen, ch_all[:n1])
    vc1, va1 = (a.copy() for a in ctx.volume_state())
    N = cc.n_nodes
    seen = 0
    for j in range(n1, cp.n):  # evaluate + commit, as the oracle continues
        r = ctx.eval_pod(cp.as_struct(), j)
        np.testing.assert_array_equal(r.fail_plugin[:N], res_all.fail_plugin[j, :N])
        m = res_all.meta(j)
        assert r.chosen == m["chosen"], (j, r.chosen, m)
        seen += int(np.isin(res_all.fail_plugin[j, :N], vff.DYNAMIC).any())
        if m["chosen"] >= 0:
            ctx.commit(cp.as_struct(), j, int(m["chosen"]))
    assert seen > 0
    ctx.reset()
    again = ctx.run_staged(n1)
    assert ctx.last_simple_form()["volumes"] == 1
    np.testing.assert_array_equal(again, chosen)
    vc2, va2 = ctx.volume_state()
    np.testing.assert_array_equal(vc2, vc1)
    np.testing.assert_array_equal(va2, va1)
    ctx.close()


# --------------------------------------------------------------------------------------
# 8. the option turned off between the stage and the run
# --------------------------------------------------------------------------------------
def test_option_turned_off_between_stage_and_run():
    """simple_volumes is process-wide and read twice: at the stage (records of the volumes form) and
    again at the run.  Turned off in between, the staged batch runs on k_schedule, with the oracle's
    results."""
    cc, cp, ch_o, res, fin, r = _fuzz(2)
    _assert_reach(r)
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    assert native.plan_podset(cc.as_struct(), cp.as_struct())["kernel"] == "k_simple"
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    ctx.stage(cp.as_struct())
    native.set_option("simple_volumes", 0)
    chosen = ctx.run_staged(cp.n)
    f = ctx.last_simple_form()
    assert ctx.last_kernel() == "k_schedule" and f == {"volumes": 0, "lds_bytes": 0}, (ctx.last_kernel(), f)
    np.testing.assert_array_equal(chosen, ch_o)
    _meta_equal(ctx.fetch_meta(cp.n), res, cp.n)
    _state_equal(ctx, cc, fin)
    ctx.close()
