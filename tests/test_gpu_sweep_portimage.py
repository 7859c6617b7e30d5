"""Scenario sweeps whose pods hold host ports (NodePorts) or node-cached images (ImageLocality), option
sweep_ports_images: k_static_pi + k_simple_pi_sweep, or k_schedule over the same packed columns,
against the C oracle scenario by scenario.

The UsedPorts column is mutable state of every scenario (a pristine and a live copy in the arena,
restored by every run, carried through HBM between chunked launches); the image-score rows are
read-only inputs; nothing is shared between scenarios.  The clusters are tests/portimage_fuzz.py's;
before a case touches the device it asserts on the oracle's own records that its inputs reach what
the case is for."""
import copy

import numpy as np
import pytest

import oracle_c
import portimage_fuzz
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu
ZONE = "topology.kubernetes.io/zone"

# (seed, nodes, bound pods, pods): per-wave and whole-workgroup mode in one 512-lane sweep, odd and
# even node counts, more than one node slot per lane
SCENARIOS = [(0, 12, 10, 30), (3, 3, 2, 20), (17, 37, 30, 151), (23, 64, 40, 151), (5, 513, 300, 150),
             (19, 700, 500, 151), (7, 1000, 600, 150), (13, 1001, 800, 151)]
LONG = [s for s in SCENARIOS if s[3] >= 150]
CHUNK = 37


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _custom_profile():
    """MostAllocated over cpu:3 / memory:2, BalancedAllocation over three resources, non-default plugin
    weights (the shape of test_gpu_scale.py's runtime profile), ImageLocality's weight raised to 3."""
    prof = abi.default_profile()
    prof.fit_strategy = abi.KSS_FIT_MOST_ALLOCATED
    prof.fit_weight[0], prof.fit_weight[1] = 3, 2
    prof.ba_n = 3
    prof.ba_res[2] = abi.KSS_RES_EPHEMERAL
    prof.weight[abi.KSS_S_NODE_AFFINITY] = 5
    prof.weight[abi.KSS_S_TAINT_TOLERATION] = 1
    prof.weight[abi.KSS_S_BALANCED_ALLOCATION] = 4
    prof.weight[abi.KSS_S_IMAGE_LOCALITY] = 3
    return prof


def _profile(kind):
    if kind == "custom":
        return _custom_profile()
    prof = abi.default_profile()
    if kind == "pct0":
        prof.pct_nodes_to_score = 0
    return prof


_CACHE = {}


def _scen(key, kind="default", edit=None):
    """(cc, cp, oracle chosen, records) of one fuzz cluster under one profile, computed once and shared
    (nothing writes to them).  edit: (name, function over the pod list)."""
    ck = (key, kind, edit[0] if edit else None)
    if ck not in _CACHE:
        seed, n_nodes, n_bound, n_pods = key
        nodes, bound, pods = portimage_fuzz.make(seed, n_nodes=n_nodes, n_bound=n_bound, n_pods=n_pods)
        if edit:
            pods = copy.deepcopy(pods)
            edit[1](pods)
        cc, cp, _ = compile_cluster(nodes, bound, pods)
        ch_o, res, _ = oracle_c.schedule(_profile(kind), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record=True,
                                         n_classes=len(cc.classes), n_terms=len(cc.terms))
        _CACHE[ck] = (cc, cp, ch_o, res)
    return _CACHE[ck]


def _reach(cc, cp, ch_o, res, prof=None):
    """What the oracle's records say the scenario exercises: (port_pods, h1_pairs, il_decided) -- pods
    with a node failing NodePorts; pods that fail NodePorts on the node the previous pod took only
    because of that pod's ports; pods whose choice is not the argmax of total - ImageLocality."""
    prof = prof or abi.default_profile()
    N = cc.n_nodes
    used = cc.arrays["port_used"][:N].copy()
    before = used.copy()
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


def _cross(cc, cp, ch_o, res, chunk):
    """Pods that, with `chunk` pods per launch, fail NodePorts on some node only because of ports
    committed in an earlier chunk: neither the snapshot's ports nor this chunk's commits conflict there."""
    N = cc.n_nodes
    used0 = cc.arrays["port_used"][:N].astype(np.uint64)
    earlier = np.zeros(N, np.uint64)  # committed in chunks before the current one
    here = np.zeros(N, np.uint64)     # committed in the current chunk so far
    n = 0
    for j in range(cp.n):
        if j % chunk == 0:
            earlier |= here
            here[:] = 0
        c = np.uint64(int(cp.pods[j]["port_conflict"]))
        fails = res.fail_plugin[j, :N] == abi.KSS_F_NODE_PORTS
        n += int((fails & ((used0 & c) == 0) & ((here & c) == 0) & ((earlier & c) != 0)).any())
        if ch_o[j] >= 0:
            here[int(ch_o[j])] |= np.uint64(int(cp.pods[j]["port_add"]))
    return n


def _assert_reach(keys, kind="default"):
    prof = _profile(kind)
    for key in keys:
        cc, cp, ch_o, res = _scen(key, kind)
        reach = _reach(cc, cp, ch_o, res, prof)
        print("reach", key, kind, reach, "unschedulable", int((ch_o < 0).sum()))
        assert min(reach) >= 1, (key, reach)


def _sweep(scen, prof=None):
    return native.Sweep(prof or abi.default_profile(), [s[0].as_struct() for s in scen], [s[1].as_struct() for s in scen])


def _check_runs(sw, want, runs=2):
    for rep in range(runs):
        chosen, _ = sw.run()
        o = 0
        for s, w in enumerate(want):  # scenario by scenario
            np.testing.assert_array_equal(chosen[o:o + len(w)], w, err_msg=f"run {rep}, scenario {s}")
            o += len(w)
        assert o == len(chosen)


# --------------------------------------------------------------------------------------
# 1. ragged sweep, two runs
# --------------------------------------------------------------------------------------
def test_ragged_sweep_two_runs():
    """The second run is the check that UsedPorts lies in the mutable region and is restored by the
    reset: dozens of pods per scenario fail NodePorts only because of this run's own commits, so a
    stale column changes the choices."""
    _assert_reach(SCENARIOS)
    scen = [_scen(k) for k in SCENARIOS]
    assert int((scen[1][2] < 0).sum()) >= 1  # 3 nodes x 20 pods: some pod finds no node
    native.set_option("sweep_ports_images", 1)
    sw = _sweep(scen)
    info = sw.info()
    assert info["kernel"] == "k_simple" and info["ports_images"], info
    _check_runs(sw, [s[2] for s in scen])
    sw.close()


# --------------------------------------------------------------------------------------
# 2. forced chunks: the port column travels between launches through HBM
# --------------------------------------------------------------------------------------
def test_forced_chunks_carry_ports():
    _assert_reach(LONG)
    scen = [_scen(k) for k in LONG]
    for k, (cc, cp, ch_o, res) in zip(LONG, scen):
        cross = _cross(cc, cp, ch_o, res, CHUNK)
        print("cross37", k, cross)
        assert cross >= 1, (k, cross)
    assert len({s[1].n for s in scen}) > 1  # differing pod counts: scenarios end in different chunks
    native.set_option("sweep_ports_images", 1)
    native.set_option("static_bytes", str(4 * sum(s[0].n_nodes for s in scen) * CHUNK))
    sw = _sweep(scen)
    info = sw.info()
    assert info["kernel"] == "k_simple" and info["ports_images"], info
    _check_runs(sw, [s[2] for s in scen])
    sw.close()


# --------------------------------------------------------------------------------------
# 3. mixed forms: scenarios without ports, images or a port column among the others
# --------------------------------------------------------------------------------------
def _synth_pair():
    syn = [native.Synth(2, 4242 + 7919 * k, n, 60) for k, n in enumerate((97, 600))]
    for x in syn:
        assert not x.cluster.port_used and x.cluster.n_images == 0
        assert not any(x.pods.pods[i].port_conflict or x.pods.pods[i].port_add or x.pods.pods[i].img_len > 0
                       for i in range(x.n_pods))
    prof = abi.default_profile()
    want = [oracle_c.schedule(prof, x.cluster, x.pods, x.n_pods, x.n_nodes, record=False,
                              n_classes=x.cluster.n_classes, n_terms=x.cluster.n_terms)[0] for x in syn]
    return syn, want


def test_mixed_forms():
    keys = [SCENARIOS[0], SCENARIOS[2], SCENARIOS[4]]
    _assert_reach(keys)
    pi = [_scen(k) for k in keys]
    syn, syn_want = _synth_pair()
    prof = abi.default_profile()
    native.set_option("sweep_ports_images", 1)
    clusters = [pi[0][0].as_struct(), syn[0].cluster, pi[1][0].as_struct(), syn[1].cluster, pi[2][0].as_struct()]
    podsets = [pi[0][1].as_struct(), syn[0].pods, pi[1][1].as_struct(), syn[1].pods, pi[2][1].as_struct()]
    want = [pi[0][2], syn_want[0], pi[1][2], syn_want[1], pi[2][2]]
    sw = native.Sweep(prof, clusters, podsets)
    info = sw.info()
    assert info["kernel"] == "k_simple" and info["ports_images"], info
    _check_runs(sw, want)
    sw.close()
    # the Synth-only pair: not of the form, and the same arena with the option on and off
    seen = []
    for on in (1, 0):
        native.set_option("sweep_ports_images", on)
        sw = native.Sweep(prof, [x.cluster for x in syn], [x.pods for x in syn])
        info = sw.info()
        assert info["kernel"] == "k_simple" and not info["ports_images"], info
        _check_runs(sw, syn_want, runs=1)
        seen.append(info["upload_bytes"])
        sw.close()
    assert seen[0] == seen[1], seen


# --------------------------------------------------------------------------------------
# 4. the routes that put the whole sweep on k_schedule
# --------------------------------------------------------------------------------------
def _weights(pods):
    """Pod 3: two preferred NodeAffinity terms whose weights sum to 8192 (one past the form's 13 bits)."""
    pref = {"matchExpressions": [{"key": "kubernetes.io/hostname", "operator": "Exists"}]}
    pods[3]["spec"]["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
        {"weight": 8092, "preference": pref}, {"weight": 100, "preference": pref}]}}


def _zone_spread(pods):
    pods[4]["spec"]["topologySpreadConstraints"] = [
        {"maxSkew": 1, "topologyKey": ZONE, "whenUnsatisfiable": "ScheduleAnyway",
         "labelSelector": {"matchLabels": {"app": "p"}}}]


@pytest.mark.parametrize("route", ["pct0", "zone-spread", "weights-8192"])
def test_k_schedule_routes(route):
    keys = [SCENARIOS[0], SCENARIOS[2], SCENARIOS[4]]
    kind = "pct0" if route == "pct0" else "default"
    _assert_reach(keys, kind)
    scen = [_scen(k, kind) for k in keys]
    if route == "zone-spread":
        scen[1] = _scen(keys[1], edit=("zone-spread", _zone_spread))
        assert scen[1][1].pods[4]["n_soft"] == 1
    elif route == "weights-8192":
        scen[1] = _scen(keys[1], edit=("weights-8192", _weights))
    native.set_option("sweep_ports_images", 1)
    prof = _profile(kind)
    plan = native.plan_sweep(prof, [s[0].as_struct() for s in scen], [s[1].as_struct() for s in scen])
    assert plan["kernel"] == "k_schedule" and plan["form"], plan
    sw = _sweep(scen, prof)
    info = sw.info()
    assert info["kernel"] == "k_schedule" and info["ports_images"], info
    _check_runs(sw, [s[2] for s in scen])
    sw.close()


# --------------------------------------------------------------------------------------
# 5. runtime profile: k_simple_pi_sweep<false>
# --------------------------------------------------------------------------------------
def test_runtime_profile():
    keys = [SCENARIOS[0], SCENARIOS[3], SCENARIOS[5]]
    _assert_reach(keys, "custom")  # il_decided >= 1 under that profile
    scen = [_scen(k, "custom") for k in keys]
    native.set_option("sweep_ports_images", 1)
    sw = _sweep(scen, _custom_profile())
    info = sw.info()
    assert info["kernel"] == "k_simple" and info["ports_images"], info
    _check_runs(sw, [s[2] for s in scen])
    sw.close()


# --------------------------------------------------------------------------------------
# 6. the one-shot entry
# --------------------------------------------------------------------------------------
def test_schedule_scenarios_one_shot():
    keys = [SCENARIOS[1], SCENARIOS[2], SCENARIOS[4]]
    _assert_reach(keys)
    scen = [_scen(k) for k in keys]
    native.set_option("sweep_ports_images", 1)
    chosen, _ = native.schedule_scenarios(abi.default_profile(), [s[0].as_struct() for s in scen],
                                          [s[1].as_struct() for s in scen])
    np.testing.assert_array_equal(chosen, np.concatenate([s[2] for s in scen]))


# --------------------------------------------------------------------------------------
# 7. option off: refused, as before
# --------------------------------------------------------------------------------------
def test_option_off_refuses():
    scen = [_scen(SCENARIOS[0])]
    with pytest.raises(native.KssError):
        _sweep(scen)
    with pytest.raises(native.KssError):
        native.schedule_scenarios(abi.default_profile(), [scen[0][0].as_struct()], [scen[0][1].as_struct()])
