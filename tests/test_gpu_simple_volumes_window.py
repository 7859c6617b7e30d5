"""k_simple's volumes form under the percentageOfNodesToScore window (options simple_ports_images +
simple_volumes + simple_volumes_window: k_static_pi + k_static_vol + k_simple_vol<.., WIN = true>)
against the C oracle, bit for bit: chosen nodes, every pod's outcome, the node rows, vol_count /
vol_attached, UsedPorts and nextStartNodeIndex.  Every case also runs with simple_volumes_window 0
(k_schedule, as before the option) for the same results.

The window passes carry the dynamic volume verdict where they carry the NodePorts verdict: ahead of
the feasible counts that place the cut.  So every case first asserts, from the oracle's own records,
that pods whose search stopped at numFeasibleNodesToFind saw a dynamic volume failure on a visited
node (a wrong verdict there moves the cut, the kept set and the next pod's start), next to what
test_gpu_simple_volumes.py asserts (volume_form_fixtures.reach).  The counts in CLUSTERS were
recorded from the oracle when the cases were chosen."""
import ctypes as C

import numpy as np
import pytest

import oracle_c
import volume_form_fixtures as vff
import volume_fuzz
import volume_portimage_fuzz
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu

BIG, MID = (11, 300, 300, 200), (7, 130, 100, 150)
# (generator, cluster, pct) -> numFeasibleNodesToFind, pods that reached it, those of them with a dynamic
# volume failure on a visited node, those with a NodePorts failure, H1 pairs
CLUSTERS = {
    ("vol", BIG, 0): (144, 92, 51, 0, 3),
    ("vol", BIG, 30): (100, 108, 65, 0, 2),
    ("vol", MID, 0): (100, 66, 33, 0, 6),
    ("vol", MID, 30): (100, 66, 33, 0, 6),
    ("all", BIG, 0): (144, 92, 52, 26, 2),
    ("all", BIG, 30): (100, 107, 63, 34, 1),
    ("all", MID, 0): (100, 66, 33, 19, 4),
    ("all", MID, 30): (100, 66, 33, 19, 4),
}
MAKERS = {"vol": volume_fuzz.make, "all": volume_portimage_fuzz.make}


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _prof(pct, base=None):
    p = base or abi.default_profile()
    p.pct_nodes_to_score = pct
    return p


def _oracle(cc, cp, prof, n=None):
    return oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), cp.n if n is None else n, cc.n_nodes,
                             record=True, n_classes=len(cc.classes), n_terms=len(cc.terms))


def windowed(cc, cp, res, k_find):
    """(pods whose search stopped at k_find, those with a dynamic volume failure on a visited node,
    those with a NodePorts failure on one)."""
    N = cc.n_nodes
    hit = dyn = ports = 0
    for j in range(cp.n):
        if res.meta(j)["n_feasible"] != k_find:
            continue
        fp = res.fail_plugin[j, :N]
        hit += 1
        dyn += int(np.isin(fp, vff.DYNAMIC).any())
        ports += int((fp == abi.KSS_F_NODE_PORTS).any())
    return hit, dyn, ports


_CACHE = {}


def _case(gen, cluster, pct, prof=None, tag=None):
    """(cc, cp, prof, oracle chosen, records, final state, reach, windowed counts) of one cluster,
    percentage and profile (tag names a profile other than the default one), computed once and shared
    (nothing writes to them)."""
    assert (prof is None) == (tag is None)
    key = (gen, cluster, pct, tag)
    if key not in _CACHE:
        if (gen, cluster) not in _CACHE:
            nodes, bound, pods, st = MAKERS[gen](cluster[0], n_nodes=cluster[1], n_bound=cluster[2], n_pods=cluster[3])
            _CACHE[(gen, cluster)] = compile_cluster(nodes, bound, pods, storage=st)[:2]
        cc, cp = _CACHE[(gen, cluster)]
        prof = _prof(pct, prof)
        ch_o, res, fin = _oracle(cc, cp, prof)
        k_find = CLUSTERS[(gen, cluster, pct)][0]
        _CACHE[key] = (cc, cp, prof, ch_o, res, fin, vff.reach(cc, cp, ch_o, res, prof), windowed(cc, cp, res, k_find))
    return _CACHE[key]


def _assert_recorded(gen, cluster, pct, r, w):
    k_find, hit, dyn, ports, h1 = CLUSTERS[(gen, cluster, pct)]
    got = {k: r[k] for k in ("restrictions", "limits", "static", "h1")}
    print("reach", got, "windowed", w)
    assert all(v > 0 for v in got.values()), got
    assert k_find < cluster[1]
    assert w == (hit, dyn, ports) and dyn > 0 and r["h1"] == h1, (w, r["h1"])


def _meta_equal(meta, res, n, first=0):
    for j in range(n):
        m = res.meta(first + j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (first + j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], first + j


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
    assert ctx.next_start_node_index() == fin["next_start"]


def _ran(ctx, form):
    f = ctx.last_simple_form()
    if form:
        assert ctx.last_kernel() == "k_simple" and f["volumes"] == 1 and f["lds_bytes"] > 0, (ctx.last_kernel(), f)
        assert ctx.last_shape_table()["shapes"] == 0
    else:
        assert ctx.last_kernel() == "k_schedule" and f == {"volumes": 0, "lds_bytes": 0}, (ctx.last_kernel(), f)


def _run(cc, cp, prof, ch_o, res, fin, form=True):
    ctx = native.Context(prof)
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
    _ran(ctx, form)
    np.testing.assert_array_equal(chosen, ch_o)
    _meta_equal(ctx.fetch_meta(cp.n), res, cp.n)
    _state_equal(ctx, cc, fin)
    launches = ctx.last_timing()[1]
    geom = dict(ctx.last_geometry(), xcd_local=ctx.last_xcd_local()["used"], fallbacks=ctx.last_xcd_local()["fallbacks"])
    ctx.close()
    return launches, geom


def _both(cc, cp, prof, ch_o, res, fin):
    """The window form, then the same batch with simple_volumes_window 0 on k_schedule."""
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    native.set_option("simple_volumes_window", 1)
    plan = native.plan_podset(cc.as_struct(), cp.as_struct(), prof)
    assert plan["kernel"] == "k_simple", plan
    out = _run(cc, cp, prof, ch_o, res, fin)
    native.set_option("simple_volumes_window", 0)
    plan = native.plan_podset(cc.as_struct(), cp.as_struct(), prof)
    assert plan["kernel"] == "k_schedule" and "percentageOfNodesToScore" in plan["reason"], plan
    _run(cc, cp, prof, ch_o, res, fin, form=False)
    return out


# --------------------------------------------------------------------------------------
# 1. geometries: slots per lane (whole workgroup), per wave with 2 and 3 waves, nine shards; the
#    XCD-local grid and the plain one
# --------------------------------------------------------------------------------------
GEOMETRIES = [("slots-per-lane", BIG, dict(shards=1, force_threads=64), 1),
              ("pw-2-waves", BIG, dict(shards=3, force_threads=128), 3),
              ("pw-3-waves", BIG, dict(shards=3, force_threads=192), 3),
              ("nine-shards", BIG, dict(shards=9), 9),
              ("mid-one-shard", MID, dict(shards=1), 1),
              ("mid-pw-2-shards", MID, dict(shards=2, force_threads=128), 2)]
CASES = [g + (pct, x) for g in GEOMETRIES for pct in (0, 30) for x in ((1, 0) if g[3] > 1 else (0,))
         if not (g[1] == MID and pct == 30 and g[3] == 1)]  # (MID: k_find 100 at both percentages; 30 once)


@pytest.mark.parametrize("name,cluster,opts,shards,pct,xcd", CASES,
                         ids=["%s-pct%d-%s" % (c[0], c[4], "xcd" if c[5] else "plain") for c in CASES])
def test_fuzz_geometries(name, cluster, opts, shards, pct, xcd):
    cc, cp, prof, ch_o, res, fin, r, w = _case("vol", cluster, pct)
    _assert_recorded("vol", cluster, pct, r, w)
    native.set_option("xcd", xcd)
    for k, v in opts.items():
        if k == "shards" and xcd:
            native.set_option("nodes_per_shard", (cluster[1] + v - 1) // v)
        else:
            native.set_option(k, v)
    _, geom = _both(cc, cp, prof, ch_o, res, fin)
    assert geom["shards"] == shards and geom["xcd_local"] == xcd, geom
    if "force_threads" in opts:
        assert geom["threads"] == opts["force_threads"], geom
    if name == "slots-per-lane":
        assert geom["nodes_per_lane"] > 1, geom


# --------------------------------------------------------------------------------------
# 2. chunked launches: the packed columns and the cursor carried from launch to launch
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pct", [0, 30])
def test_chunked_batch_carries_volume_state_and_cursor(pct):
    cc, cp, prof, ch_o, res, fin, r, w = _case("vol", BIG, pct)
    _assert_recorded("vol", BIG, pct, r, w)
    native.set_option("shards", 3)
    native.set_option("static_bytes", 4 * cc.n_nodes * 60)  # 60 pods per chunk: 4 chunk launches
    launches, _ = _both(cc, cp, prof, ch_o, res, fin)
    assert launches >= 2 * 3, launches  # k_static + the loop kernel per chunk, at least 3 chunks


# --------------------------------------------------------------------------------------
# 3. the XCD-local placement reported failed: the unrestricted rerun finds state and cursor untouched
# --------------------------------------------------------------------------------------
def test_xcd_fallback_leaves_state_untouched():
    cc, cp, prof, ch_o, res, fin, r, w = _case("vol", BIG, 0)
    _assert_recorded("vol", BIG, 0, r, w)
    native.set_option("xcd", 1)
    native.set_option("nodes_per_shard", 100)
    native.set_option("xcd_force_fallback", 1)
    _, geom = _both(cc, cp, prof, ch_o, res, fin)
    assert geom["shards"] == 3 and geom["xcd_local"] == 1 and geom["fallbacks"] >= 1, geom


# --------------------------------------------------------------------------------------
# 4. a runtime profile (the DEF = false window kernel)
# --------------------------------------------------------------------------------------
def _profile():
    p = abi.default_profile()
    p.filter_enabled &= ~(1 << abi.KSS_F_VOLUME_RESTRICTIONS)
    p.filter_enabled &= ~(1 << abi.KSS_F_NODE_VOLUME_LIMITS)
    p.weight[abi.KSS_S_TAINT_TOLERATION] = 1
    p.weight[abi.KSS_S_NODE_RESOURCES_FIT] = 3
    p.weight[abi.KSS_S_BALANCED_ALLOCATION] = 2
    return p


# under _profile() at pct 0, recorded from the oracle when the case was chosen: pods with a limit-plugin
# failure, with a static failure, H1 pairs; the windowed counts as in CLUSTERS
PROFILE_REACH, PROFILE_WINDOWED = dict(limits=105, static=93, h1=4), (94, 44, 0)


@pytest.mark.parametrize("shards,threads", [(3, 128), (1, 64)])
def test_runtime_profile(shards, threads):
    cc, cp, prof, ch_o, res, fin, r, w = _case("vol", BIG, 0, prof=_profile(), tag="profile")
    N = cc.n_nodes
    fails = set(int(x) for x in np.unique(res.fail_plugin[:, :N]))
    assert abi.KSS_F_VOLUME_RESTRICTIONS not in fails and abi.KSS_F_NODE_VOLUME_LIMITS not in fails
    print("reach", {k: r[k] for k in ("limits", "static", "h1")}, "windowed", w)
    assert {k: r[k] for k in PROFILE_REACH} == PROFILE_REACH, r  # the enabled limit plugins still decide
    assert w == PROFILE_WINDOWED and w[1] > 0, w
    assert not np.array_equal(ch_o, _case("vol", BIG, 0)[3])  # ... and the profile changes the choices
    native.set_option("shards", shards)
    native.set_option("force_threads", threads)
    _, geom = _both(cc, cp, prof, ch_o, res, fin)
    assert geom["shards"] == shards and geom["threads"] == threads, geom


# --------------------------------------------------------------------------------------
# 5. volumes, host ports and images in one windowed batch
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster,pct,shards", [(BIG, 0, 3), (BIG, 30, 1), (MID, 0, 2), (MID, 30, 1)])
def test_volumes_ports_and_images_together(cluster, pct, shards):
    cc, cp, prof, ch_o, res, fin, r, w = _case("all", cluster, pct)
    _assert_recorded("all", cluster, pct, r, w)
    assert w[2] > 0
    assert (fin["port_used"][:cc.n_nodes] != cc.arrays["port_used"][:cc.n_nodes]).any()
    native.set_option("shards", shards)
    _, geom = _both(cc, cp, prof, ch_o, res, fin)
    assert geom["shards"] == shards


# --------------------------------------------------------------------------------------
# 6. state hand-over: a second batch on the same context continues from nextStartNodeIndex and the
#    written-back volume state, on either kernel
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", ["k_simple", "k_schedule"])
def test_second_batch_continues(second):
    cc, cp, prof, ch_o, res, fin, r, w = _case("vol", BIG, 0)
    n1 = 120
    _, _, mid = _oracle(cc, cp, prof, n=n1)
    N = cc.n_nodes
    later = [j for j in range(n1, cp.n) if np.isin(res.fail_plugin[j, :N], vff.DYNAMIC).any()]
    assert later and mid["next_start"] not in (0, fin["next_start"])
    assert (mid["vol_attached"] != fin["vol_attached"]).any() and (mid["vol_count"] != fin["vol_count"]).any()
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    native.set_option("simple_volumes_window", 1)
    native.set_option("shards", 3)
    ctx = native.Context(prof)
    ctx.load(cc.as_struct())
    ps = cp.as_struct()
    a = ctx.schedule_batch(ps, n1)
    _ran(ctx, True)
    np.testing.assert_array_equal(a, ch_o[:n1])
    _state_equal(ctx, cc, mid)
    tail = abi.PodSet.from_buffer_copy(ps)  # the same podset with its first n1 pods removed (a new staging)
    tail.n_pods = cp.n - n1
    tail.pods = C.cast(C.addressof(ps.pods.contents) + n1 * C.sizeof(abi.Pod), C.POINTER(abi.Pod))
    native.set_option("simple_volumes_window", 1 if second == "k_simple" else 0)
    b = ctx.schedule_batch(tail, cp.n - n1)
    _ran(ctx, second == "k_simple")
    np.testing.assert_array_equal(b, ch_o[n1:])
    _meta_equal(ctx.fetch_meta(cp.n - n1), res, cp.n - n1, first=n1)
    _state_equal(ctx, cc, fin)
    ctx.close()


# --------------------------------------------------------------------------------------
# 7. the option turned off between the stage and the run
# --------------------------------------------------------------------------------------
def test_option_turned_off_between_stage_and_run():
    """simple_volumes_window is process-wide and read at the run (the stage builds the volumes form's
    records whatever it says).  Turned off between the stage and the run, the staged batch runs the
    window on k_schedule, with the oracle's results and nextStartNodeIndex."""
    cc, cp, prof, ch_o, res, fin, r, w = _case("vol", MID, 30)
    _assert_recorded("vol", MID, 30, r, w)
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    native.set_option("simple_volumes_window", 1)
    assert native.plan_podset(cc.as_struct(), cp.as_struct(), prof)["kernel"] == "k_simple"
    ctx = native.Context(prof)
    ctx.load(cc.as_struct())
    ctx.stage(cp.as_struct())
    native.set_option("simple_volumes_window", 0)
    chosen = ctx.run_staged(cp.n)
    _ran(ctx, False)
    np.testing.assert_array_equal(chosen, ch_o)
    _meta_equal(ctx.fetch_meta(cp.n), res, cp.n)
    _state_equal(ctx, cc, fin)
    ctx.close()
