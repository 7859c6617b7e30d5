"""The service grid's k_simple-shaped chain in its ports-and-images form (option
service_ports_images: k_static_pi's words, UsedPorts held in LDS as grid state, NodePorts decided
in the chain ahead of NodeResourcesFit, ImageLocality in the record) against the C oracle, record
for record: outcome, every node's verdict and detail, raw / normalised / total scores over the kept
feasible nodes, the cursor, the final node rows and the final UsedPorts.

The clusters are tests/portimage_fuzz.py's.  Every fuzz case first asserts on the oracle's own
records that the sequence reaches what it is meant to (REACH): NodePorts failures, failures that a
service commit caused, choices ImageLocality decides, rolled-back port holders, and nodes that pass
NodePorts only because a rollback cleared the port."""
import copy
import functools
import time
import types

import numpy as np
import pytest

import oracle_c
import portimage_fuzz
import preempt_fixtures as pf
import preempt_port_fixtures as ppf
import progfuzz
from kss import abi, native
from kss.compile import compile_cluster
from kss.synth import SEED_BASE

pytestmark = pytest.mark.gpu
MI = 1024 * 1024
RB = 7  # the commit of every RB-th pod (0, 7, 14, ...) is rolled back


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _prof(pct=100):
    p = abi.default_profile()
    p.pct_nodes_to_score = pct
    return p


def _skip(n, noms=()):
    skip = np.zeros(n, np.uint8)
    skip[::RB] = 1
    for j, _ in noms:  # (a nominated pod's commit is kept: commit + rollback would drop the nomination)
        if j < n:
            skip[j] = 0
    return skip


@functools.lru_cache(maxsize=None)
def _compiled(cluster):
    seed, n_nodes, n_bound, n_pods = cluster
    nodes, bound, pods = portimage_fuzz.make(seed, n_nodes=n_nodes, n_bound=n_bound, n_pods=n_pods)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    return cc, cp


def _oracle(cc, cp, prof, n=None, noms=(), skip=None):
    n = cp.n if n is None else n
    return oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), n, cc.n_nodes, threads=8, record=True,
                             n_classes=len(cc.classes), n_terms=len(cc.terms), nominations=noms,
                             skip_commit=_skip(n, noms) if skip is None else skip)


@functools.lru_cache(maxsize=None)
def _fuzz(cluster, pct):
    """(cc, cp, oracle chosen, records, final state) of one fuzz sequence with the rollback pattern,
    computed once and shared (nothing writes to them)."""
    cc, cp = _compiled(cluster)
    return (cc, cp) + tuple(_oracle(cc, cp, _prof(pct)))


def _reach(cc, cp, ch_o, res, st, skip):
    """What the oracle's records say the sequence exercises:
    (pods with a NodePorts failure,
     pods with a NodePorts failure on a node whose snapshot UsedPorts do not conflict: a service commit caused it,
     pods whose choice is not the argmax of total - ImageLocality,
     rolled-back pods that held ports,
     pods for which some node reaches NodePorts and passes it although the ports of the pods rolled
     back there would conflict: only the rollback cleared them).
    Also checks the oracle's final UsedPorts against the replayed sets ("evaluated, not assumed" and
    "committed, then rolled back" agree on ports: HostPortInfo is a set)."""
    N = cc.n_nodes
    snap = cc.arrays["port_used"][:N].astype(np.uint64)
    used = snap.copy()      # the replayed sets: a rollback clears the pod's entries
    ghost = snap.copy()     # ... and as they would stand had no rollback cleared anything
    port_pods = commit_pods = il_pods = rb_ports = rb_pass = 0
    for j in range(len(ch_o)):
        fp = res.fail_plugin[j, :N]
        conflict = np.uint64(int(cp.pods[j]["port_conflict"]))
        ports = fp == abi.KSS_F_NODE_PORTS
        port_pods += int(ports.any())
        commit_pods += int((ports & ((snap & conflict) == 0)).any())
        reached = (fp == abi.KSS_F_PASS) | ((fp > abi.KSS_F_NODE_PORTS) & (fp != abi.KSS_F_NOT_EVALUATED))
        rb_pass += int((reached & ((used & conflict) == 0) & ((ghost & conflict) != 0)).any())
        m = res.meta(j)
        if m["scored"]:
            kept = (fp == 0) & (res.fail_detail[j, :N] != abi.KSS_PASS_NOT_KEPT)
            rest = np.where(kept, res.total[j, :N] - res.norm[j][abi.KSS_S_IMAGE_LOCALITY, :N], -1)
            il_pods += int(np.argmax(rest) != m["chosen"])
        if ch_o[j] >= 0:
            add = np.uint64(int(cp.pods[j]["port_add"]))
            ghost[int(ch_o[j])] |= add
            if skip[j]:
                rb_ports += int(add != 0)
                used[int(ch_o[j])] &= ~add
            else:
                used[int(ch_o[j])] |= add
    np.testing.assert_array_equal(st["port_used"][:N], used)
    return port_pods, commit_pods, il_pods, rb_ports, rb_pass


def _copy(v):
    out = types.SimpleNamespace()
    for k in ("fail_plugin", "fail_detail", "raw", "norm", "total"):
        setattr(out, k, None if getattr(v, k) is None else np.array(getattr(v, k)))
    for k in ("chosen", "n_feasible", "scored", "status", "best_total"):
        setattr(out, k, getattr(v, k))
    return out


def _ctx(cc, prof):
    ctx = native.Context(prof)
    ctx.load(cc.as_struct())
    return ctx


def _check_record(got, res, j, N):
    """test_service_records_match_c_oracle's comparison of one record."""
    m = res.meta(j)
    assert (got.chosen, got.n_feasible, got.scored, got.status) == \
           (m["chosen"], m["n_feasible"], m["scored"], m["status"]), (j, m)
    np.testing.assert_array_equal(got.fail_plugin[:N], res.fail_plugin[j, :N], err_msg=f"pod {j} verdicts")
    np.testing.assert_array_equal(got.fail_detail[:N], res.fail_detail[j, :N], err_msg=f"pod {j} details")
    if m["scored"]:
        assert got.best_total == m["best_total"], j
        kept = (res.fail_plugin[j, :N] == 0) & (res.fail_detail[j, :N] != abi.KSS_PASS_NOT_KEPT)
        np.testing.assert_array_equal(got.raw[:, :N][:, kept], res.raw[j][:, :N][:, kept], err_msg=f"pod {j} raw")
        np.testing.assert_array_equal(got.norm[:, :N][:, kept], res.norm[j][:, :N][:, kept], err_msg=f"pod {j} norm")
        np.testing.assert_array_equal(got.total[:N][kept], res.total[j, :N][kept], err_msg=f"pod {j} total")


def _check_state(svc, st, N, cursor=True):
    """After service_stop: the cursor, the node rows and UsedPorts against the oracle's final state."""
    if cursor:
        assert svc.next_start_node_index() == st["next_start"]
    g = svc.node_state()
    for k in ("requested", "nonzero", "pod_count"):
        np.testing.assert_array_equal(g[k][..., :N], st[k][..., :N], err_msg=k)
    np.testing.assert_array_equal(svc.port_state()[:N], st["port_used"][:N], err_msg="port_used")


def _service(cc, cp, prof, res, st, n=None, noms=(), skip=None, mode_pi=True, first=0, svc=None, stop=True,
             sleep_at=-1, keep=None):
    """The service sequence [first, n) against the oracle's records (res), committing the oracle's
    pattern; returns the context (stopped and checked against st when `stop`)."""
    n = cp.n if n is None else n
    skip = _skip(n, noms) if skip is None else skip
    ps = cp.as_struct()
    if svc is None:
        svc = _ctx(cc, prof)
        svc.stage(ps)
        for j, node in noms:
            svc.nominate(ps, j, node)
    N = svc.n_nodes
    for j in range(first, n):
        if j == sleep_at:
            time.sleep(2.5)  # the grid leaves after ~1 s idle; the next call relaunches it
        got = svc.service_eval(j)
        _check_record(got, res, j, N)
        if keep is not None:
            keep.append(_copy(got))
        if j == first:
            mode, form = svc.service_mode(), svc.service_form()
            if mode_pi:
                assert mode in (1, 2) and form[0] == 1, (mode, form)
            else:
                assert mode == 0 and form[0] == 0, (mode, form)
        if got.chosen >= 0:
            svc.service_commit(j, got.chosen)
            if skip[j]:
                svc.service_rollback(j, got.chosen)
    if stop:
        svc.service_stop()
        _check_state(svc, st, N)
    return svc


# --------------------------------------------------------------------------------------
# 1. records against the oracle, over geometries
# --------------------------------------------------------------------------------------
SMALL, BIG = (31, 40, 30, 120), (11, 300, 300, 200)
SEQUENCES = [(SMALL, 100), (BIG, 100), (BIG, 0), (BIG, 30)]
# the oracle's own counts for these sequences (_reach): with 40 nodes the window is inactive
REACH = {(SMALL, 100): (62, 57, 51, 7, 24), (BIG, 100): (109, 99, 107, 19, 67),
         (BIG, 0): (109, 94, 104, 19, 55), (BIG, 30): (109, 90, 102, 19, 40)}
GEOMETRIES = {"auto": {}, "one-shard": dict(shards=1), "3x128": dict(shards=3, force_threads=128),
              "nine-shards": dict(shards=9), "1x64": dict(shards=1, force_threads=64)}


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
@pytest.mark.parametrize("cluster,pct", SEQUENCES, ids=["%dx%d-pct%d" % (c[1], c[3], p) for c, p in SEQUENCES])
def test_records_match_c_oracle(cluster, pct, geometry):
    cc, cp, ch_o, res, st = _fuzz(cluster, pct)
    reach = _reach(cc, cp, ch_o, res, st, _skip(cp.n))
    print(cluster, pct, "reach", reach)
    assert all(x > 0 for x in reach), reach
    assert reach == REACH[(cluster, pct)], reach
    assert all(c >= 0 for c in ch_o)  # no pod is left unscheduled
    native.set_option("service_ports_images", 1)
    for k, v in GEOMETRIES[geometry].items():
        native.set_option(k, v)
    svc = _service(cc, cp, _prof(pct), res, st)
    geom = svc.last_geometry()
    if "shards" in GEOMETRIES[geometry]:
        assert geom["shards"] == GEOMETRIES[geometry]["shards"], geom
    if "force_threads" in GEOMETRIES[geometry]:
        assert geom["threads"] == GEOMETRIES[geometry]["force_threads"], geom
    if geometry == "1x64" and cluster == BIG:
        assert geom["nodes_per_lane"] > 1, geom
    svc.close()


# --------------------------------------------------------------------------------------
# 2. the two chains against each other
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster,pct", [(SMALL, 100), (BIG, 100), (BIG, 30)], ids=["40", "300", "300-pct30"])
def test_general_chain_and_simple_chain_agree(cluster, pct):
    """The same sequence with the option 0 (the general chain, mode 0) and 1, entry for entry: the
    whole record of every pod, all nodes and rows.  Both also equal the oracle's records."""
    cc, cp, ch_o, res, st = _fuzz(cluster, pct)
    recs = []
    for on in (0, 1):
        native.set_option("service_ports_images", on)
        keep = []
        _service(cc, cp, _prof(pct), res, st, mode_pi=bool(on), keep=keep).close()
        recs.append(keep)
    N = cc.n_nodes
    for j, (a, b) in enumerate(zip(*recs)):
        assert (a.chosen, a.n_feasible, a.scored, a.status, a.best_total) == \
               (b.chosen, b.n_feasible, b.scored, b.status, b.best_total), j
        for k in ("fail_plugin", "fail_detail", "raw", "norm", "total"):
            np.testing.assert_array_equal(getattr(a, k)[..., :N], getattr(b, k)[..., :N], err_msg=f"pod {j} {k}")


# --------------------------------------------------------------------------------------
# 3. compact equals full
# --------------------------------------------------------------------------------------
def test_compact_record_equals_full():
    cc, cp, ch_o, res, st = _fuzz(BIG, 100)
    native.set_option("service_ports_images", 1)
    svc = _ctx(cc, _prof())
    svc.stage(cp.as_struct())
    N = svc.n_nodes
    skip = _skip(cp.n)
    sub = abi.KSS_FIELD_FAIL | abi.KSS_FIELD_TOTAL
    for j in range(cp.n):
        fields = sub if j % 5 == 4 else abi.KSS_FIELD_ALL
        if j % 2:
            c = _copy(svc.service_eval_compact(j, fields))
            f = _copy(svc.service_eval(j, fields))
        else:
            f = _copy(svc.service_eval(j, fields))
            c = _copy(svc.service_eval_compact(j, fields))
        assert (c.chosen, c.n_feasible, c.scored, c.status, c.best_total) == \
               (f.chosen, f.n_feasible, f.scored, f.status, f.best_total), j
        assert f.chosen == ch_o[j], j
        for k in ("fail_plugin", "fail_detail", "raw", "norm", "total"):
            a, b = getattr(c, k), getattr(f, k)
            assert (a is None) == (b is None), (j, k)
            if a is not None:
                assert a.dtype == {"fail_plugin": np.uint8, "fail_detail": np.uint16, "raw": np.int32,
                                   "norm": np.uint8, "total": np.int32}[k], (j, k, a.dtype)
                np.testing.assert_array_equal(a[..., :N].astype(np.int64), b[..., :N].astype(np.int64),
                                              err_msg=f"pod {j} {k}")
        if f.chosen >= 0:
            svc.service_commit(j, f.chosen)
            if skip[j]:
                svc.service_rollback(j, f.chosen)
    assert svc.service_form()[0] == 1
    svc.service_stop()
    _check_state(svc, st, N)
    svc.close()


# --------------------------------------------------------------------------------------
# 4. edges
# --------------------------------------------------------------------------------------
def _node(name, images=None, cpu="4", pods="20"):
    st = {"allocatable": {"cpu": cpu, "memory": "8Gi", "pods": pods, "ephemeral-storage": "20Gi"}}
    if images:
        st["images"] = images
    return {"metadata": {"name": name, "labels": {"kubernetes.io/hostname": name}}, "spec": {}, "status": st}


def _pod(name, containers, node=None):
    spec = {"containers": containers}
    if node:
        spec["nodeName"] = node
    return {"metadata": {"name": name, "namespace": "default", "labels": {"app": "p"}}, "spec": spec}


def _ctr(name, image, ports=None, cpu="500m"):
    c = {"name": name, "image": image, "resources": {"requests": {"cpu": cpu, "memory": "1Gi"}}}
    if ports:
        c["ports"] = ports
    return c


P8080 = [{"containerPort": 80, "hostPort": 8080}]


def _hand(nodes, bound, pods, skip=None, shards=None):
    """A hand-made case on the service against the oracle (no rollback unless `skip`); returns
    (cc, cp, chosen, records)."""
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    skip = np.zeros(cp.n, np.uint8) if skip is None else np.asarray(skip, np.uint8)
    ch_o, res, st = _oracle(cc, cp, _prof(), skip=skip)
    return cc, cp, ch_o, res, st, skip


def test_port_dictionary_bit_63():
    """test_gpu_simple_portimage's case: the 64-entry dictionary whose conflicting holder is bit 63."""
    nodes, bound, _, holder = ppf.bit63()
    nodes = nodes + [pf.node("w", "g1"), pf.node("v", "g1")]
    pods = [ppf.with_ports(pf.pod("a", 10, "100m", group="g1"), (60000, "TCP", None)),
            ppf.with_ports(pf.pod("b", 10, "100m", group="g1"), (60000, "TCP", "10.0.0.9"))]
    cc, cp, ch_o, res, st, skip = _hand(nodes, bound, pods)
    assert len(cc.ports) == 64 and cc.port_index[holder] == 63
    top = 1 << 63
    x, w, v = (cc.node_names.index(k) for k in "xwv")
    assert int(cc.arrays["port_used"][x]) & int(cp.pods[0]["port_conflict"]) == top  # bit 63 alone fails x
    np.testing.assert_array_equal(ch_o, [w, v])
    assert res.fail_plugin[0, x] == abi.KSS_F_NODE_PORTS and res.fail_plugin[1, w] == abi.KSS_F_NODE_PORTS
    assert int(st["port_used"][v]) == top
    native.set_option("service_ports_images", 1)
    native.set_option("shards", 2)
    _service(cc, cp, _prof(), res, st, skip=skip).close()


def test_image_score_ends_with_node_affinity_8191():
    """test_image_score_ends' nodes (ImageLocality 0, 0 and 100) under a pod whose preferred terms
    give every node raw NodeAffinity 8191, the 13-bit field's maximum: the word's two top fields full
    together (score 100 sets bit 31)."""
    nodes = [_node("n0"), _node("n1", [{"names": ["small:1"], "sizeBytes": 30 * MI}]),
             _node("n2", [{"names": ["big:1"], "sizeBytes": 9000 * MI}])]
    pref = {"matchExpressions": [{"key": "kubernetes.io/hostname", "operator": "Exists"}]}
    p = _pod("p", [_ctr("c0", "small:1"), _ctr("c1", "big:1")])
    p["spec"]["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
        {"weight": 8091, "preference": pref}, {"weight": 100, "preference": pref}]}}
    q = copy.deepcopy(p)
    q["metadata"]["name"] = "q"  # the second pod meets n2 with one pod more
    cc, cp, ch_o, res, st, skip = _hand(nodes, [], [p, q])
    np.testing.assert_array_equal(res.raw[0][abi.KSS_S_NODE_AFFINITY, :3], [8191] * 3)
    np.testing.assert_array_equal(res.raw[0][abi.KSS_S_IMAGE_LOCALITY, :3], [0, 0, 100])
    np.testing.assert_array_equal(res.norm[0][abi.KSS_S_IMAGE_LOCALITY, :3], [0, 0, 100])
    assert ch_o[0] == 2 and res.total[0, 2] - res.total[0, 0] == 100
    native.set_option("service_ports_images", 1)
    _service(cc, cp, _prof(), res, st, skip=skip).close()


def test_node_failing_ports_and_fit_records_node_ports():
    """Three nodes; n1 holds hostPort 8080 and has 300m of CPU left.  Pod a (8080, 500m) fails both
    NodePorts and NodeResourcesFit there: the record says NodePorts, detail 0 (NodePorts comes first
    in the filter order); pod b (no port, 500m) shows that the node does fail NodeResourcesFit."""
    nodes = [_node("n0"), _node("n1"), _node("n2")]
    bound = [_pod("h", [_ctr("c", "none:1", P8080, cpu="3700m")], node="n1")]
    pods = [_pod("a", [_ctr("c", "none:1", P8080)]), _pod("b", [_ctr("c", "none:1")])]
    cc, cp, ch_o, res, st, skip = _hand(nodes, bound, pods)
    assert res.fail_plugin[0, 1] == abi.KSS_F_NODE_PORTS and res.fail_detail[0, 1] == 0
    assert res.fail_plugin[1, 1] == abi.KSS_F_NODE_RESOURCES_FIT and res.fail_detail[1, 1] == abi.KSS_FIT_CPU
    assert res.meta(0)["n_feasible"] == 2
    native.set_option("service_ports_images", 1)
    _service(cc, cp, _prof(), res, st, skip=skip).close()


def test_rollback_frees_a_port_on_a_node_over_its_pod_limit():
    """n1 allows one pod and holds one.  Pod a (hostPort 8080) is assumed there and forgotten again
    (Reserve / Unreserve on a node the caller picked); pod b (8080) then fails n1 by NodeResourcesFit
    with the too-many-pods bit: the port the rollback freed must not come back as a NodePorts verdict
    from a stale copy of UsedPorts."""
    nodes = [_node("n0"), _node("n1", pods="1"), _node("n2")]
    bound = [_pod("h", [_ctr("c", "none:1")], node="n1")]
    pods = [_pod("a", [_ctr("c", "none:1", P8080)]), _pod("b", [_ctr("c", "none:1", P8080)])]
    cc, cp, ch_o, res, st, skip = _hand(nodes, bound, pods, skip=[1, 0])
    assert res.fail_plugin[1, 1] == abi.KSS_F_NODE_RESOURCES_FIT and res.fail_detail[1, 1] == abi.KSS_FIT_TOO_MANY_PODS
    native.set_option("service_ports_images", 1)
    svc = _ctx(cc, _prof())
    svc.stage(cp.as_struct())
    _check_record(svc.service_eval(0), res, 0, 3)
    assert svc.service_mode() in (1, 2) and svc.service_form()[0] == 1
    svc.service_commit(0, 1)
    mid = _copy(svc.service_eval(1))  # while a sits on n1: its port is the first failing filter there
    assert mid.fail_plugin[1] == abi.KSS_F_NODE_PORTS and mid.fail_detail[1] == 0
    svc.service_rollback(0, 1)
    _check_record(svc.service_eval(1), res, 1, 3)
    svc.service_commit(1, int(ch_o[1]))
    svc.service_stop()
    _check_state(svc, st, 3)
    svc.close()


# --------------------------------------------------------------------------------------
# 5. runtime profiles
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
    cc, cp = _compiled(SMALL)
    prof = _profile(kind)
    ch_o, res, st = _oracle(cc, cp, prof)
    N = cc.n_nodes
    port_pods = sum(int((res.fail_plugin[j, :N] == abi.KSS_F_NODE_PORTS).any()) for j in range(cp.n))
    if kind == "ports-filter-off":
        assert port_pods == 0 and (st["port_used"][:N] != cc.arrays["port_used"][:N]).any()
    else:
        assert port_pods > 0
    il_rows = sum(int(res.norm[j][abi.KSS_S_IMAGE_LOCALITY, :N].any()) for j in range(cp.n))
    assert il_rows > 0  # the score is recorded whether or not it is enabled; only the total follows the profile
    native.set_option("service_ports_images", 1)
    native.set_option("shards", 2)
    _service(cc, cp, prof, res, st).close()


# --------------------------------------------------------------------------------------
# 6. nominees that hold ports
# --------------------------------------------------------------------------------------
N_RUN = 100


@functools.lru_cache(maxsize=None)
def _nominated_input():
    """SMALL with five of the pods behind the run (priority 1000, each holding a host port)
    nominated to distinct nodes, and one pod of the run nominated to a node whose snapshot ports
    conflict with its own (PreferNominatedNode fails by NodePorts)."""
    seed, n_nodes, n_bound, n_pods = SMALL
    nodes, bound, pods = portimage_fuzz.make(seed, n_nodes=n_nodes, n_bound=n_bound, n_pods=n_pods)
    cc0, cp0, _ = compile_cluster(nodes, bound, pods)
    holders = [j for j in range(N_RUN, n_pods) if int(cp0.pods[j]["port_add"])][:5]
    assert len(holders) == 5
    pods = copy.deepcopy(pods)
    for j in holders:
        pods[j]["spec"]["priority"] = 1000
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    snap = cc.arrays["port_used"][:cc.n_nodes]
    noms = [(j, 3 + 7 * i) for i, j in enumerate(holders)]  # nodes 3, 10, 17, 24, 31
    own = next((j, n) for j in range(20, N_RUN) for n in range(cc.n_nodes)
               if int(snap[n]) & int(cp.pods[j]["port_conflict"]) and n not in [x for _, x in noms])
    noms.append(own)
    return cc, cp, tuple(noms), own


def test_nominees_that_hold_ports():
    cc, cp, noms, own = _nominated_input()
    prof = _prof()
    N = cc.n_nodes
    ch_o, res, st = _oracle(cc, cp, prof, n=N_RUN, noms=noms)
    skip = _skip(N_RUN, noms)
    # some node's verdict is NodePorts only because of a nominee's ports: neither the snapshot nor
    # any pod the sequence left there conflicts
    used = cc.arrays["port_used"][:N].astype(np.uint64)
    nominee_only = 0
    for j in range(N_RUN):
        conflict = np.uint64(int(cp.pods[j]["port_conflict"]))
        ports = res.fail_plugin[j, :N] == abi.KSS_F_NODE_PORTS
        nominee_only += int((ports & ((used & conflict) == 0)).sum())
        if ch_o[j] >= 0 and not skip[j]:
            used[int(ch_o[j])] |= np.uint64(int(cp.pods[j]["port_add"]))
    assert nominee_only > 0
    j_own, n_own = own  # PreferNominatedNode: the nominated node fails NodePorts, the full search runs
    assert res.fail_plugin[j_own, n_own] == abi.KSS_F_NODE_PORTS and ch_o[j_own] not in (-1, n_own)
    recs = []
    for on in (1, 0):
        native.set_option("service_ports_images", on)
        keep = []
        # (one idle exit in the middle of the ports-and-images run: the relaunch reloads the column
        # with the commits made so far)
        svc = _service(cc, cp, prof, res, st, n=N_RUN, noms=noms, mode_pi=bool(on), keep=keep,
                       sleep_at=N_RUN // 2 if on else -1)
        assert svc.nominations() == st["nominations"]
        svc.close()
        recs.append(keep)
    for j, (a, b) in enumerate(zip(*recs)):
        for k in ("fail_plugin", "fail_detail", "raw", "norm", "total"):
            np.testing.assert_array_equal(getattr(a, k)[..., :N], getattr(b, k)[..., :N], err_msg=f"pod {j} {k}")


# --------------------------------------------------------------------------------------
# 7. hand-over of the column
# --------------------------------------------------------------------------------------
def test_port_delta_between_two_service_runs():
    """kss_apply_port_delta between two runs of the grid: the second run loads the overwritten word.
    Node 5 gets every dictionary bit, so every later pod that wants a port fails NodePorts there
    unless a static filter fails it first; the general chain, given the same delta, agrees entry
    for entry."""
    cc, cp = _compiled(SMALL)
    N, half, node = cc.n_nodes, 40, 5
    full = (1 << len(cc.ports)) - 1
    recs = []
    for on in (1, 0):
        native.set_option("service_ports_images", on)
        svc = _ctx(cc, _prof())
        svc.stage(cp.as_struct())
        keep = []
        for j in range(cp.n):
            if j == half:
                svc.apply_port_delta([node], [full])  # (stops the grid first)
                assert int(svc.port_state()[node]) == full
            got = _copy(svc.service_eval(j))
            keep.append(got)
            if j in (0, half):
                assert (svc.service_form()[0], svc.service_mode() in (1, 2)) == (on, bool(on))
            if j >= half and int(cp.pods[j]["port_conflict"]) and got.status == 0:
                assert got.fail_plugin[node] in (abi.KSS_F_NODE_PORTS, abi.KSS_F_NODE_UNSCHEDULABLE, abi.KSS_F_NODE_NAME,
                                                 abi.KSS_F_TAINT_TOLERATION, abi.KSS_F_NODE_AFFINITY), j
            if got.chosen >= 0:
                svc.service_commit(j, got.chosen)
        svc.service_stop()
        keep.append(svc.port_state()[:N].copy())
        svc.close()
        recs.append(keep)
    assert any(r.fail_plugin[node] == abi.KSS_F_NODE_PORTS for r in recs[0][half:-1])
    np.testing.assert_array_equal(recs[0][-1], recs[1][-1])
    for j, (a, b) in enumerate(zip(recs[0][:-1], recs[1][:-1])):
        assert a.chosen == b.chosen, j
        for k in ("fail_plugin", "fail_detail", "raw", "norm", "total"):
            np.testing.assert_array_equal(getattr(a, k)[..., :N], getattr(b, k)[..., :N], err_msg=f"pod {j} {k}")


def test_batch_after_the_service_sees_its_ports():
    """The first 60 pods on the service, then the same 60 pod specs once more as a batch on
    k_schedule: the oracle schedules the 120 in one sequence (the second 60 are copies under other
    names, so their records equal the first 60's and the batch of pods [0, 60) computes them)."""
    seed, n_nodes, n_bound, _ = SMALL
    nodes, bound, pods = portimage_fuzz.make(seed, n_nodes=n_nodes, n_bound=n_bound, n_pods=60)
    again = copy.deepcopy(pods)
    for p in again:
        p["metadata"]["name"] = "r" + p["metadata"]["name"]
    cc, cp, _ = compile_cluster(nodes, bound, pods + again)
    N, h = cc.n_nodes, 60
    skip = np.zeros(cp.n, np.uint8)
    ch_o, res, st = _oracle(cc, cp, _prof(), skip=skip)
    port_pods = sum(int((res.fail_plugin[j, :N] == abi.KSS_F_NODE_PORTS).any()) for j in range(h, 2 * h))
    assert port_pods > 0
    native.set_option("service_ports_images", 1)
    svc = _service(cc, cp, _prof(), res, None, n=h, skip=skip, stop=False)
    chosen = svc.schedule_batch(cp.as_struct(), h)  # (stops the grid first: the column goes back to HBM)
    assert svc.last_kernel() == "k_schedule"
    np.testing.assert_array_equal(chosen, ch_o[h:])
    _check_state(svc, st, N, cursor=False)
    svc.close()


# --------------------------------------------------------------------------------------
# 8. routing that stays put
# --------------------------------------------------------------------------------------
def test_list_without_ports_or_images_runs_what_it_ran():
    s = native.Synth(1, SEED_BASE + 1, 100, 40)
    seen = []
    for on in (0, 1):
        native.set_option("service_ports_images", on)
        svc = native.Context(abi.default_profile())
        svc.load(s.cluster)
        svc.stage(s.pods)
        r = _copy(svc.service_eval(0))
        seen.append((svc.service_mode(), svc.service_form(), svc.last_geometry(), r.chosen, r.total.tobytes()))
        svc.service_stop()
        svc.close()
    assert seen[0][0] in (1, 2) and seen[0][1][0] == 0 and seen[0][1][1] > 0 and seen[0] == seen[1], seen
    s.close()


def test_option_turned_off_between_stage_and_start():
    """The option is process-wide and read twice: at the stage (records of the form) and again when
    the service starts.  Turned off in between, the service runs its general chain (mode 0), with the
    oracle's records and final state."""
    cc, cp, ch_o, res, st = _fuzz((3, 12, 10, 30), 100)
    prof = _prof()
    native.set_option("service_ports_images", 1)
    assert native.plan_service(cc.as_struct(), cp.as_struct(), prof)["chain"] == 1
    svc = _ctx(cc, prof)
    svc.stage(cp.as_struct())
    native.set_option("service_ports_images", 0)
    svc.service_start()
    _service(cc, cp, prof, res, st, mode_pi=False, svc=svc).close()


@pytest.mark.parametrize("how", ["service_general", "svc_no_static", "volume-pod"])
def test_lists_that_keep_the_general_chain(how):
    """With the option on: service_general forces mode 0, a list without the static-word table keeps
    the general chain (no inline ports-and-images word), and so does a list with a volume pod --
    records equal to the oracle's in each case."""
    native.set_option("service_ports_images", 1)
    if how == "volume-pod":
        seed, n_nodes, n_bound, n_pods = SMALL
        nodes, bound, pods = portimage_fuzz.make(seed, n_nodes=n_nodes, n_bound=n_bound, n_pods=n_pods)
        pods[7]["spec"]["volumes"] = [{"name": "v0", "gcePersistentDisk": {"pdName": "disk-1"}}]
        cc, cp, _ = compile_cluster(nodes, bound, pods)
        assert cp.pods[7]["vol_len"] > 0
        ch_o, res, st = _oracle(cc, cp, _prof())
    else:
        native.set_option(how, 1)
        cc, cp, ch_o, res, st = _fuzz(SMALL, 100)
    _service(cc, cp, _prof(), res, st, mode_pi=False).close()
