"""k_preempt (kss_postfilter_pod) on the branch fixtures of tests/preempt_branch_fixtures.py,
compared as the full tuple of tests/preempt_compare.py: the hand-derived cases, the constructed
clusters for the per-workgroup and cross-workgroup reductions, the rich seeded recipe (dry runs
and the committing sequence), pinned probes (a clone pinned to one node shows that node's own
dry run, winner or not), the victims_cap boundary of the C ABI, and one context reused across
pods of different bin plans and a grown bound table.

Expected values: the hand-derived tuples where the fixture states them, oracle_c.postfilter
elsewhere (tests/test_preemption_branches.py pins it to the object-level restatement)."""
import ctypes as C

import numpy as np
import pytest

import k8s_oracle as ko
import k8s_preemption as kp
import preempt_branch_fixtures as bf
import preempt_compare as pc
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu


def _ctx(cc, record=1):
    ctx = native.Context(abi.default_profile(), max_pods_record=record)
    ctx.load(cc.as_struct(), names=native.make_names(cc.node_names, cc.taints, cc.scalars))
    ctx.load_bound(cc.as_boundset())
    return ctx


def _device_dry_runs(compiled, noms=(), only=None, ctx=None):
    """kss_postfilter_pod of every pod (or the indices in `only`) on the unchanged snapshot, one context."""
    cc, cp, _ = compiled
    ps = cp.as_struct()
    own = ctx is None
    if own:
        ctx = _ctx(cc)
        for j, n in pc.index_noms(cc, cp, noms):
            ctx.nominate(ps, j, n)
    out = [pc.from_native(ctx.postfilter_pod(ps, j), cc, cp) for j in (range(cp.n) if only is None else only)]
    if own:
        ctx.close()
    return out


def _check(nodes, bound, pods, expect=None, noms=()):
    """Device == oracle_c on every pod, and == the hand-derived tuple where one is stated."""
    compiled = compile_cluster(nodes, bound, pods)
    got = _device_dry_runs(compiled, noms)
    want = pc.c_dry_runs(compiled, 4, noms)
    by = {ko._name(b): b for b in bound}
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, (ko._name(pods[j]), g, w)
        if expect is not None and expect[j] is not None:
            assert g == pc.expected(*expect[j], by), ko._name(pods[j])
    return got


def test_branch_fixture_on_device():
    _check(*bf.branch_fixture())


def test_min_rise_on_device():
    nodes, bound, pods, noms, expect = bf.min_rise_fixture()
    _check(nodes, bound, pods, expect, noms)


def test_after_remove_on_device():
    nodes, bound, pods, gone, before, after = bf.after_remove_fixture()
    cc, cp, _ = compiled = compile_cluster(nodes, bound, pods)
    by = {ko._name(b): b for b in bound}
    ctx = _ctx(cc)
    assert _device_dry_runs(compiled, ctx=ctx) == [pc.expected(*before, by)]
    ctx.remove_bound([[nm[1] for nm in cc.bound_names].index(gone)])
    assert _device_dry_runs(compiled, ctx=ctx) == [pc.expected(*after, by)]
    ctx.close()


@pytest.mark.parametrize("n_nodes", [65, 130, 200])
def test_ladder_on_device(n_nodes):
    nodes, bound, pods, expect, _ = bf.ladder(n_nodes)
    _check(nodes, bound, pods, expect)


def test_wide_start_on_device():
    _check(*bf.wide_start())


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65])
def test_plain_edge_sizes_on_device(n_nodes):
    _check(*bf.plain(n_nodes))


def test_twelve_victims_on_device():
    _check(*bf.twelve())


@pytest.mark.parametrize("key", [bf.HOST, bf.RACK], ids=["hostname", "rack"])
@pytest.mark.parametrize("n_nodes", [257, 520])
def test_two_smallest_on_device(n_nodes, key):
    for name in bf.two_smallest_placements(n_nodes):
        nodes, bound, pods, noms, info = bf.two_smallest(n_nodes, name, key)
        _check(nodes, bound, pods, info["expect"], noms)


@pytest.mark.parametrize("seed,n_nodes,n_pods", bf.RICH_SHAPES)
def test_saturated_rich_dry_runs(seed, n_nodes, n_pods):
    nodes, bound, pods = bf.saturated_rich(seed, n_nodes, n_pods)
    compiled = compile_cluster(nodes, bound, pods)
    got = _device_dry_runs(compiled)
    want = pc.c_dry_runs(compiled, 8)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, (j, g, w)
    assert sum(w[0] == "nominated" for w in want) >= 5


@pytest.mark.parametrize("seed,n_nodes,n_pods", bf.RICH_SHAPES)
def test_saturated_rich_sequence(seed, n_nodes, n_pods):
    """The committing sequence: placed pods become bound pods (and victims) of the later dry runs."""
    nodes, bound, pods = bf.saturated_rich(seed, n_nodes, n_pods)
    o, out = kp.schedule_with_preemption(nodes, bound, pods)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    ps = cp.as_struct()
    ctx = _ctx(cc)
    placed = 0
    for j, (r, pre, _) in enumerate(out):
        e = ctx.eval_pod(ps, j)
        if r["selected"] is not None:
            assert e.chosen >= 0 and cc.node_names[e.chosen] == ko._name(o.nodes[r["selected"]]), j
            ctx.commit(ps, j, e.chosen)
            placed += 1
        else:
            assert e.chosen < 0, j
            assert pc.from_native(ctx.postfilter_pod(ps, j), cc, cp) == pc.from_python(o, pre), j
    ctx.close()
    assert placed >= 1


def _probes_on_device(nodes, bound, pods):
    probes = pc.pinned_probes(nodes, bound, pods)
    clones = [q for q, _ in probes]
    got = _device_dry_runs(compile_cluster(nodes, bound, clones))
    for (q, want), g in zip(probes, got):
        assert pc.probe_view(g) == want, ko._name(q)
    return probes


def test_pinned_probes_hand_fixtures_on_device():
    nodes, bound, pods, _ = bf.branch_fixture()
    assert len(_probes_on_device(nodes, bound, pods)) > 20


def test_pinned_probes_saturated_rich_on_device():
    """Every potential node's own dry run, not only the winner's: a wrong spread minimum or
    affinity count on a node that does not win shows here and nowhere else."""
    probes = _probes_on_device(*bf.saturated_rich(1, 60, 40))
    assert sum(w[0] == "nominated" for _, w in probes) > 100


def test_victims_cap():
    """kss_postfilter_pod's victims buffer: n_victims is the full count whatever the cap, the
    written prefix is the full list's, the words past the cap are untouched, and nothing else
    in the result depends on the cap."""
    nodes, bound, pods, expect = bf.twelve()
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    ps = cp.as_struct()
    ctx = _ctx(cc)
    full = ctx.postfilter_pod(ps, 0)
    n = full["n_victims"]
    assert n == 12 and len(full["victims"]) == n
    assert pc.from_native(full, cc, cp) == pc.expected(*expect[0], {ko._name(b): b for b in bound})
    SENT = -0x5A5A5A5A5A5A5A5B
    fields = ("status", "nominated", "n_potential", "n_candidates", "n_victims", "highest_priority",
              "sum_priority", "earliest_start")
    for cap in (0, 1, n - 1, n, n + 3):
        buf = np.full(n + 8, SENT, np.int64)
        r = abi.PreemptResult()
        r.victims_cap = cap
        r.victims = buf.ctypes.data_as(C.POINTER(C.c_int64))
        native.check(native.lib().kss_postfilter_pod(ctx.h, C.byref(ps), 0, C.byref(r)))
        assert [getattr(r, f) for f in fields] == [full[f] for f in fields], cap
        k = min(cap, n)
        assert [int(v) for v in buf[:k]] == full["victims"][:k], cap
        assert (buf[k:] == SENT).all(), cap
    ctx.close()


def test_context_reuse():
    """One context across pods whose bin plans differ (a zone histogram, none, node-valued
    counts, affinity bins), twice round, with a batch commit in between that grows the bound
    table (the victims scratch is sized by it): every result equals a fresh context's on the
    same state.  The batch (priority -100, 100m each) takes exactly the 300m every kind=mem node
    has free, so afterwards the 100m preemptor "on-cpu" -- placeable before -- must evict one of
    the batch's pods: a victim that exists only in the grown table."""
    nodes, bound, _ = bf.saturated_rich(1, 60, 40)
    a0 = {"app": "a0"}
    n_mem = sum(n["metadata"]["labels"]["kind"] == "mem" for n in nodes)
    batch = [bf.bpod("batch-%d" % k, -100, "100m", nodeSelector={"kind": "mem"}) for k in range(3 * n_mem)]
    probes = [bf.bpod("zone-spread", 1000, "2000m", labels=a0, topologySpreadConstraints=[bf._spread(a0, bf.ZONE, 4)]),
              bf.bpod("plain", 100, "1000m"),
              bf.bpod("host-spread", 1000, "2000m", labels=a0, topologySpreadConstraints=[bf._spread(a0, bf.HOST, 2)]),
              bf.bpod("affinity", 100, "1000m", labels=a0, affinity=bf._aff(a0)),
              bf.bpod("on-mem", 5000, {"cpu": "100m", "memory": "1536Mi"}, nodeSelector={"kind": "mem"}),
              bf.bpod("on-cpu", 50, "100m", nodeSelector={"kind": "mem"})]
    pods = batch + probes
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    ps = cp.as_struct()
    idx = list(range(len(batch), len(pods)))

    def fresh(j, committed):
        c = _ctx(cc, record=len(batch))
        if committed:
            chosen = c.schedule_batch(ps, len(batch), record=True)
            assert (chosen >= 0).all()
        r = pc.from_native(c.postfilter_pod(ps, j), cc, cp)
        c.close()
        return r

    ctx = _ctx(cc, record=len(batch))
    first = [pc.from_native(ctx.postfilter_pod(ps, j), cc, cp) for j in idx]
    chosen = ctx.schedule_batch(ps, len(batch), record=True)
    assert (chosen >= 0).all()
    second = [pc.from_native(ctx.postfilter_pod(ps, j), cc, cp) for j in idx]
    third = [pc.from_native(ctx.postfilter_pod(ps, j), cc, cp) for j in reversed(idx)][::-1]
    ctx.close()
    assert first == [fresh(j, False) for j in idx]
    want = [fresh(j, True) for j in idx]
    assert second == want and third == want
    assert sum(t[0] == "nominated" for t in first) >= 3
    assert first[-1][0] == "schedulable"
    assert second[-1][0] == "nominated" and second[-1][2][0].startswith("batch-") and second[-1][4] == n_mem
