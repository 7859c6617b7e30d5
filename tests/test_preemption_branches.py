"""DefaultPreemption branch fixtures on the CPU: the object-level restatement
(oracle/k8s_preemption.py) equals every hand-derived expectation of
tests/preempt_branch_fixtures.py, the C restatement (oracle/kss_oracle.c) equals it as the full
tuple of tests/preempt_compare.py, the seeded `saturated_rich` recipe reaches the branches it
was written for, the constructed clusters sit where the device's workgroups need them, and a
clone pinned to one node exposes that node's own dry run (what the GPU tests rely on)."""
import collections
import functools

import pytest

import k8s_oracle as ko
import k8s_preemption as kp
import preempt_branch_fixtures as bf
import preempt_compare as pc
from kss.compile import compile_cluster


def _check(nodes, bound, pods, expect, noms=(), threads=(1, 4)):
    """Python == hand-derived, C == Python at every thread count; returns the Python tuples."""
    by = {ko._name(b): b for b in bound}
    o, got, _ = pc.py_dry_runs(nodes, bound, pods, noms)
    for j, e in enumerate(expect):
        if e is not None:
            assert got[j] == pc.expected(*e, by), ko._name(pods[j])
    comp = compile_cluster(nodes, bound, pods)
    for t in threads:
        for j, (g, w) in enumerate(zip(pc.c_dry_runs(comp, t, noms), got)):
            assert pc.same(g, w), (t, ko._name(pods[j]), g, w)
    return comp, got


def test_branch_fixture():
    nodes, bound, pods, expect = bf.branch_fixture()
    assert all(e is not None for e in expect)
    _check(nodes, bound, pods, expect)


def test_min_rise_fixture():
    nodes, bound, pods, noms, expect = bf.min_rise_fixture()
    _check(nodes, bound, pods, expect, noms)
    # without the nominee the same pod evicts the same filler: the nominee is what exposes the
    # second criticalPaths entry, not what makes the node a candidate
    _check(nodes, bound, pods, expect)


def test_after_remove_fixture():
    """NodeInfo.RemovePod swaps the last pod into the freed slot; the C restatement reads the
    bound table in NodeInfo order, so it gets the table as it stands after the removal."""
    nodes, bound, pods, gone, before, after = bf.after_remove_fixture()
    by = {ko._name(b): b for b in bound}
    _check(nodes, bound, pods, [before])
    o = ko.Oracle(nodes, bound)
    o.infos[0].remove_pod(by[gone])
    r = o.schedule_one(pods[0], commit=False)
    assert pc.from_python(o, kp.preempt(o, pods[0], r)) == pc.expected(*after, by)
    swapped = [by[v] for v in after[2]]  # NodeInfo order after the removal
    _check(nodes, swapped, pods, [after])


@pytest.mark.parametrize("n_nodes", [65, 130, 200])
def test_ladder(n_nodes):
    nodes, bound, pods, expect, layout = bf.ladder(n_nodes)
    comp, _ = _check(nodes, bound, pods, expect)
    cc = comp[0]
    assert list(cc.node_names) == [ko._name(n) for n in nodes]  # device index == list index
    W = (n_nodes + bf.WG - 1) // bf.WG
    seen = collections.defaultdict(set)
    winners = set()
    for crit, kind, cand, winner in layout:
        wgs = {i // bf.WG for i in cand}
        assert (len(wgs) == 1) == (kind == "same"), (crit, kind, cand)
        seen[crit].add(kind)
        winners.add(winner // bf.WG)
    for crit in ("hp", "sum", "cnt", "start", "index", "nostart"):
        assert seen[crit] == {"same", "cross"}, crit
    assert {"lex-hp", "lex-sum"} <= set(seen)
    assert 0 in winners and W - 1 in winners
    if W > 2:
        assert winners & set(range(1, W - 1))


def test_wide_start():
    """More than 64 node workgroups: one lane of the last reduction folds two tuples."""
    nodes, bound, pods, expect = bf.wide_start()
    comp, _ = _check(nodes, bound, pods, expect, threads=(4,))
    assert list(comp[0].node_names) == [ko._name(n) for n in nodes]
    nb = (len(nodes) + bf.WG - 1) // bf.WG
    assert nb > bf.PICK_LANES
    idx = {ko._name(n): i for i, n in enumerate(nodes)}
    a, b = idx[expect[0][1]], bf.WG * bf.PICK_LANES + 10
    assert (a // bf.WG) % bf.PICK_LANES == (b // bf.WG) % bf.PICK_LANES and a // bf.WG != b // bf.WG


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65])
def test_plain_edge_sizes(n_nodes):
    _check(*bf.plain(n_nodes))


def test_twelve_victims():
    nodes, bound, pods, expect = bf.twelve()
    assert len(expect[0][2]) == 12
    _check(nodes, bound, pods, expect)


@pytest.mark.parametrize("key", [bf.HOST, bf.RACK], ids=["hostname", "rack"])
@pytest.mark.parametrize("n_nodes", [257, 520])
def test_two_smallest(n_nodes, key):
    nb, per = bf.stats_ranges(n_nodes)
    assert nb == {257: 2, 520: 3}[n_nodes]
    placements = bf.two_smallest_placements(n_nodes)
    rng = {k: (v[0] // per, v[1] // per) for k, v in placements.items()}
    assert rng["one-range"] == (0, 0) and rng["adjacent-up"] == (0, 1) and rng["adjacent-down"] == (1, 0)
    assert rng["tied"] == (0, 1) and rng["last-range"] == (nb - 1, 0)
    for name in placements:
        nodes, bound, pods, noms, info = bf.two_smallest(n_nodes, name, key)
        comp, got = _check(nodes, bound, pods, info["expect"], noms, threads=(4,))
        assert list(comp[0].node_names) == [ko._name(n) for n in nodes]
        assert got[0][1] == "n%04d" % info["x"] and got[1][1] == "n%04d" % info["a"]  # another node / the minimum node


# --------------------------------------------------------------------------------------
def reach(nodes, bound, pods):
    """What the committing sequence of the object-level restatement reaches, counted by an
    observer around Oracle.filter_with_nominated (the oracle itself is unchanged)."""
    c = collections.Counter()
    o = ko.Oracle(nodes, bound)
    inner = o.filter_with_nominated
    seen = []

    def watch(pod, i, ni, pts_st, ipa_st, vb_claims=None):
        failed, rec = inner(pod, i, ni, pts_st, ipa_st, vb_claims)
        seen.append((failed, rec.get(failed) if failed else None))
        return failed, rec

    for p in pods:
        r = o.schedule_one(p)
        if r["selected"] is not None:
            continue
        o.filter_with_nominated = watch
        del seen[:]
        pre = kp.preempt(o, p, r)
        o.filter_with_nominated = inner
        c[pre["status"]] += 1
        if any(f == "InterPodAffinity" and m == ko.MSG["IPA_AFF"] for f, m in seen):
            c["affinity_decides"] += 1
        if pre["status"] != "nominated":
            continue
        rec = r["filter"][ko._name(o.nodes[pre["nominated"]])]
        plugin = next(reversed(rec))
        c["status:" + plugin] += 1
        if plugin == "NodeResourcesFit":
            c["fit:" + rec[plugin]] += 1
        if len(pre["victims"]) >= 5:
            c["victims>=5"] += 1
        c["max_victims"] = max(c["max_victims"], len(pre["victims"]))
    return c


def test_saturated_rich_reaches_its_branches():
    """Conditions on the inputs (not measurements): over the three shapes the committing
    sequence nominates on nodes whose cycle status was PodTopologySpread / InterPodAffinity, lets a
    required-affinity term decide dry-run filter calls, and has memory, the extended resource and
    the pod limit each force evictions alone.  Achieved (seeds 1-3 at 60/40, 130/50, 300/50):
    96 nominations -- cycle status PodTopologySpread 4, InterPodAffinity 12, NodeResourcesFit 80
    (memory alone 14, example.com/gpu alone 17, the pod limit alone 13, CPU alone 17, two
    reasons 19); 17 dry runs in which "didn't match pod affinity rules" decided a filter call;
    5 nominations with 5 or more victims (9 at most); 14 no_candidate, 10 not_eligible."""
    tot = collections.Counter()
    for seed, n, m in bf.RICH_SHAPES:
        nodes, bound, pods = bf.saturated_rich(seed, n, m)
        per_node = collections.Counter()
        prio = {ko._name(b): ko.pod_priority(b) for b in bound}
        top = max(ko.pod_priority(p) for p in pods)
        for b in bound:
            if prio[ko._name(b)] < top:
                per_node[b["spec"]["nodeName"]] += 1
        assert max(per_node.values()) <= 12
        c = reach(nodes, bound, pods)
        mv = max(tot["max_victims"], c["max_victims"])
        tot.update(c)
        tot["max_victims"] = mv
    print(dict(tot))
    assert tot["status:PodTopologySpread"] >= 3 and tot["status:InterPodAffinity"] >= 3
    assert tot["affinity_decides"] >= 3
    assert tot["fit:Insufficient memory"] >= 3
    assert tot["fit:Insufficient " + bf.GPU] >= 3
    assert tot["fit:Too many pods"] >= 3
    assert tot["victims>=5"] >= 1
    assert tot["no_candidate"] >= 1 and tot["not_eligible"] >= 1


@functools.lru_cache(maxsize=None)
def _rich(seed, n_nodes, n_pods):
    """The Python dry runs of a rich shape (computed once for both thread counts) and its compilation."""
    nodes, bound, pods = bf.saturated_rich(seed, n_nodes, n_pods)
    return pc.py_dry_runs(nodes, bound, pods)[1], compile_cluster(nodes, bound, pods)


@pytest.mark.parametrize("seed,n_nodes,n_pods,threads", [(s, n, m, t) for s, n, m in bf.RICH_SHAPES for t in (1, 4)])
def test_saturated_rich_c_matches_python(seed, n_nodes, n_pods, threads):
    want, compiled = _rich(seed, n_nodes, n_pods)
    got = pc.c_dry_runs(compiled, threads)
    for j, (g, w) in enumerate(zip(got, want)):
        assert pc.same(g, w), (j, g, w)
    assert sum(w[0] == "nominated" for w in want) >= 5


# --------------------------------------------------------------------------------------
def _probe_case(nodes, bound, pods, noms=()):
    probes = pc.pinned_probes(nodes, bound, pods, noms)
    assert probes
    clones = [q for q, _ in probes]
    _, got, _ = pc.py_dry_runs(nodes, bound, clones + [p for p in pods if any(ko._name(p) == pn for pn, _ in noms)], noms)
    for (q, want), g in zip(probes, got):
        assert pc.probe_view(g) == want, ko._name(q)
        assert g[4] == (1 if want[0] == "nominated" else 0)
    return probes


def test_pinned_probes_hand_fixtures():
    probes = _probe_case(*bf.branch_fixture()[:3])
    assert sum(w[0] == "nominated" for _, w in probes) >= 10 and any(w[0] == "no_candidate" for _, w in probes)


def test_pinned_probes_saturated_rich():
    probes = _probe_case(*bf.saturated_rich(1, 60, 40))
    losers = [w for _, w in probes if w[0] == "nominated"]
    assert len(losers) > 100  # most of them are candidates that did not win: invisible without the pin
