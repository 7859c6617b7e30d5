"""Scenario sweeps whose pods hold volume programs (options sweep_ports_images + sweep_volumes):
k_static_pi + k_static_vol + k_simple_vol_sweep, or k_schedule over the packed volume columns, against
the C oracle scenario by scenario.

The used-rows / attached columns are mutable state of every scenario (packed on the host, a pristine
and a live copy in the arena, restored by every run, carried through HBM between chunked launches); the
limit columns, the row masks and the pods' SVol records are read-only inputs; nothing is shared between
scenarios.  The clusters are tests/volume_fuzz.py's; before a case touches the device it asserts on
the oracle's own records (volume_form_fixtures.reach) that its inputs reach what the case is for."""
import numpy as np
import pytest

import oracle_c
import portimage_fuzz
import volume_form_fixtures as vff
import volume_fuzz
import volume_portimage_fuzz
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu

# (seed, nodes, bound pods, pods).  RAGGED: per-wave and whole-workgroup mode in one 384 x 2 sweep
# (12 / 59 / 56 / 60 / 60 volume rows); SMALL: the clusters of test_gpu_simple_volumes.py
RAGGED = [(4, 3, 2, 20), (1, 37, 30, 151), (1, 64, 40, 151), (3, 513, 150, 150), (2, 700, 150, 151)]
ROWS = [12, 59, 56, 60, 60]
SMALL = [(2, 12, 16, 40), (31, 40, 30, 120), (7, 130, 100, 150), (11, 300, 300, 200)]
THOUSAND = (4, 1000, 150, 150)
LONG = [k for k in RAGGED if k[3] >= 150]
CHUNK = 37
MAKERS = {"vol": volume_fuzz.make, "all": volume_portimage_fuzz.make}


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _custom_profile():
    """The runtime profile of test_gpu_sweep_portimage.py: MostAllocated over cpu:3 / memory:2,
    BalancedAllocation over three resources, non-default plugin weights."""
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


def _scen(key, kind="default", gen="vol"):
    """(cc, cp, oracle chosen, records, reach) of one fuzz cluster under one profile, computed once and
    shared (nothing writes to them)."""
    ck = (gen, key, kind)
    if ck not in _CACHE:
        if (gen, key) not in _CACHE:
            nodes, bound, pods, st = MAKERS[gen](key[0], n_nodes=key[1], n_bound=key[2], n_pods=key[3])
            _CACHE[(gen, key)] = compile_cluster(nodes, bound, pods, storage=st)[:2]
        cc, cp = _CACHE[(gen, key)]
        prof = _profile(kind)
        ch_o, res, _ = oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record=True,
                                         n_classes=len(cc.classes), n_terms=len(cc.terms))
        _CACHE[ck] = (cc, cp, ch_o, res, vff.reach(cc, cp, ch_o, res, None if kind == "default" else prof))
    return _CACHE[ck]


def _pi_scen(seed=5):
    """A tests/portimage_fuzz.py scenario: host ports and images, no volume, no volume rows."""
    if ("pi", seed) not in _CACHE:
        nodes, bound, pods = portimage_fuzz.make(seed)
        cc, cp, _ = compile_cluster(nodes, bound, pods)
        ch_o, res, _ = oracle_c.schedule(abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes,
                                         record=True, n_classes=len(cc.classes), n_terms=len(cc.terms))
        _CACHE[("pi", seed)] = (cc, cp, ch_o, res, None)
    return _CACHE[("pi", seed)]


def _assert_reach(scen, what=("restrictions", "limits", "static", "h1")):
    for cc, cp, ch_o, res, r in scen:
        got = {k: r[k] for k in what}
        print("reach", cc.n_nodes, cp.n, got, "unschedulable", int((ch_o < 0).sum()))
        assert all(v > 0 for v in got.values()), got


def _cross(cc, cp, ch_o, res, chunk):
    """Pods that, with `chunk` pods per launch, fail a dynamic volume filter on some node only through
    commits of an earlier chunk: on that node neither the snapshot's state nor the snapshot plus this
    chunk's commits fails the pod (default profile; the replay of volume_form_fixtures.reach)."""
    cs = cc.as_struct()
    N, R, K = cc.n_nodes, cs.n_vol_rows, cs.n_vol_keys
    A = cc.arrays
    plug = [int(x) for x in A["vol_key_plugin"][:K]]
    keyrows = [sum(1 << r for r in range(R) if int(A["vol_row_key"][r]) == k) for k in range(K)]
    used0 = [sum(1 << r for r in range(R) if A["vol_count"][r][n] > 0) for n in range(N)]
    att0 = [[int(A["vol_attached"][k][n]) for k in range(K)] for n in range(N)]
    lim = [[int(A["vol_limit"][k][n]) for k in range(K)] for n in range(N)]

    def fails(masks, u, a, n):
        conflict, shared, own, keys, pnew, padd = masks
        if u & conflict:
            return True
        for k in range(K):
            if not (keys >> k) & 1 or lim[n][k] < 0:
                continue
            new = bin(shared & keyrows[k] & ~u).count("1") + pnew[k]
            if plug[k] == abi.KSS_F_NODE_VOLUME_LIMITS and new == 0:
                continue
            if a[k] + new > lim[n][k]:
                return True
        return False

    def commit(masks, u, a, x):
        own, padd = masks[2], masks[5]
        fresh = own & ~u[x]
        for k in range(K):
            a[x][k] += bin(fresh & keyrows[k]).count("1") + padd[k]
        u[x] |= own

    used, att = list(used0), [list(a) for a in att0]    # every commit so far
    hu, ha = list(used0), [list(a) for a in att0]       # the snapshot plus this chunk's commits
    n_cross = 0
    for j in range(cp.n):
        if j % chunk == 0:
            hu, ha = list(used0), [list(a) for a in att0]
        masks = vff.pod_masks(cc, cp, j)
        fp = res.fail_plugin[j, :N]
        hit = False
        for n in np.nonzero(np.isin(fp, vff.DYNAMIC))[0]:
            n = int(n)
            assert fails(masks, used[n], att[n], n), (j, n)
            hit |= not fails(masks, used0[n], att0[n], n) and not fails(masks, hu[n], ha[n], n)
        n_cross += int(hit)
        x = int(ch_o[j])
        if x >= 0:
            commit(masks, used, att, x)
            commit(masks, hu, ha, x)
    return n_cross


def _sweep(scen, prof=None):
    return native.Sweep(prof or abi.default_profile(), [s[0].as_struct() for s in scen], [s[1].as_struct() for s in scen])


def _on():
    native.set_option("sweep_ports_images", 1)
    native.set_option("sweep_volumes", 1)


def _check_runs(sw, want, runs=2):
    first = None
    for rep in range(runs):
        chosen, _ = sw.run()
        o = 0
        for s, w in enumerate(want):  # scenario by scenario
            np.testing.assert_array_equal(chosen[o:o + len(w)], w, err_msg=f"run {rep}, scenario {s}")
            o += len(w)
        assert o == len(chosen)
        if first is None:
            first = chosen.copy()
        np.testing.assert_array_equal(chosen, first)  # the restore: every run the same


def _info(sw, kernel):
    info = sw.info()
    assert info["kernel"] == kernel and info["volumes"] and info["ports_images"], info
    return info


# --------------------------------------------------------------------------------------
# 1. the ragged and the small set, two runs each (the second run checks the restore)
# --------------------------------------------------------------------------------------
def test_ragged_sweep_two_runs():
    scen = [_scen(k) for k in RAGGED]
    assert [s[0].as_struct().n_vol_rows for s in scen] == ROWS
    _assert_reach(scen)
    _on()
    plan = native.plan_sweep(abi.default_profile(), [s[0].as_struct() for s in scen], [s[1].as_struct() for s in scen],
                             detail=True)
    assert plan["kernel"] == "k_simple" and plan["volumes"], plan
    sw = _sweep(scen)
    _info(sw, "k_simple")
    _check_runs(sw, [s[2] for s in scen])
    sw.close()


def test_small_sweep_two_runs():
    scen = [_scen(k) for k in SMALL]
    _assert_reach(scen)
    assert scen[3][0].as_struct().n_vol_rows == 64  # row 63 is live
    _on()
    sw = _sweep(scen)
    _info(sw, "k_simple")
    _check_runs(sw, [s[2] for s in scen])
    sw.close()


# --------------------------------------------------------------------------------------
# 2. forced chunks: the packed columns travel between launches through HBM
# --------------------------------------------------------------------------------------
def test_forced_chunks_carry_volume_state():
    scen = [_scen(k) for k in LONG]
    _assert_reach(scen)
    for k, (cc, cp, ch_o, res, _) in zip(LONG, scen):
        cross = _cross(cc, cp, ch_o, res, CHUNK)
        print("cross37", k, cross)
        assert cross >= 1, (k, cross)
    assert len({s[1].n for s in scen}) > 1  # differing pod counts: scenarios end in different chunks
    _on()
    native.set_option("static_bytes", str(4 * sum(s[0].n_nodes for s in scen) * CHUNK))
    sw = _sweep(scen)
    _info(sw, "k_simple")
    _check_runs(sw, [s[2] for s in scen])
    sw.close()


# --------------------------------------------------------------------------------------
# 3. a mixed sweep: a scenario without volumes (zero columns) among the others; host ports and
#    images beside the volumes
# --------------------------------------------------------------------------------------
def test_mixed_sweep():
    scen = [_scen(SMALL[0]), _pi_scen(), _scen(SMALL[2]), _scen((31, 40, 30, 120), gen="all")]
    _assert_reach([scen[0], scen[2], scen[3]])
    assert scen[1][0].as_struct().n_vol_rows == 0 and not any(scen[1][1].pods[i]["vol_len"] > 0 for i in range(scen[1][1].n))
    N = scen[3][0].n_nodes
    assert any((scen[3][3].fail_plugin[j, :N] == abi.KSS_F_NODE_PORTS).any() for j in range(scen[3][1].n))
    _on()
    sw = _sweep(scen)
    _info(sw, "k_simple")
    _check_runs(sw, [s[2] for s in scen])
    sw.close()


# --------------------------------------------------------------------------------------
# 4. runtime profile: k_simple_vol_sweep<false>
# --------------------------------------------------------------------------------------
def test_runtime_profile():
    keys = [SMALL[2], RAGGED[2], RAGGED[4]]  # (each keeps H1 pairs under this profile; (31, 40, ..) and (11, 300, ..) do not)
    scen = [_scen(k, "custom") for k in keys]
    _assert_reach(scen)
    assert any(not np.array_equal(_scen(k)[2], s[2]) for k, s in zip(keys, scen))  # the profile changes choices
    _on()
    sw = _sweep(scen, _custom_profile())
    _info(sw, "k_simple")
    _check_runs(sw, [s[2] for s in scen])
    sw.close()


# --------------------------------------------------------------------------------------
# 5. the routes that put the whole sweep on k_schedule, over the packed volume columns
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["pct0", "thousand-nodes", "seventy-rows"])
def test_k_schedule_routes(route):
    kind = "pct0" if route == "pct0" else "default"
    keys = SMALL[:3] + ([THOUSAND] if route == "thousand-nodes" else [(5, 100, 120, 300)] if route == "seventy-rows" else [SMALL[3]])
    scen = [_scen(k, kind) for k in keys]
    _assert_reach(scen, ("restrictions", "limits", "static"))
    if route == "pct0":  # the window decides somewhere: a pod's search stops at numFeasibleNodesToFind
        N = scen[3][0].n_nodes
        assert any((scen[3][3].fail_detail[j, :N] == abi.KSS_PASS_NOT_KEPT).any() for j in range(scen[3][1].n))
    _on()
    prof = _profile(kind)
    plan = native.plan_sweep(prof, [s[0].as_struct() for s in scen], [s[1].as_struct() for s in scen], detail=True)
    assert plan["kernel"] == "k_schedule" and plan["volumes"], plan
    sw = _sweep(scen, prof)
    _info(sw, "k_schedule")
    _check_runs(sw, [s[2] for s in scen])
    sw.close()


# --------------------------------------------------------------------------------------
# 6. the one-shot entry
# --------------------------------------------------------------------------------------
def test_schedule_scenarios_one_shot():
    scen = [_scen(k) for k in (RAGGED[0], RAGGED[1], SMALL[2])]
    _assert_reach(scen)
    _on()
    chosen, _ = native.schedule_scenarios(abi.default_profile(), [s[0].as_struct() for s in scen],
                                          [s[1].as_struct() for s in scen])
    np.testing.assert_array_equal(chosen, np.concatenate([s[2] for s in scen]))


# --------------------------------------------------------------------------------------
# 7. either option off: refused, as before; a sweep without volume pods keeps its arena
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi,vol", [(1, 0), (0, 1)])
def test_either_option_off_refuses(pi, vol):
    native.set_option("sweep_ports_images", pi)
    native.set_option("sweep_volumes", vol)
    with pytest.raises(native.KssError):
        _sweep([_scen(SMALL[0])])


def test_sweep_without_volume_pods_keeps_its_upload():
    scen = [_pi_scen(5), _pi_scen(6)]
    seen = []
    for on in (0, 1):
        native.set_option("sweep_ports_images", 1)
        native.set_option("sweep_volumes", on)
        sw = _sweep(scen)
        info = sw.info()
        assert info["kernel"] == "k_simple" and info["ports_images"] and not info["volumes"], info
        _check_runs(sw, [s[2] for s in scen], runs=1)
        seen.append(info["upload_bytes"])
        sw.close()
    assert seen[0] == seen[1], seen
