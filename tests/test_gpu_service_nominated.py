"""The per-pod service grid with a non-empty nominator (kss_nominate + kss_service_*):
RunFilterPluginsWithNominatedPods' first pass, PreferNominatedNode and DeleteNominatedPodIfExists on
the k_simple-shaped evaluation (svc_simple_eval's nominee code) and on the general chain
(schedule_pod with the service's NomView), against the C oracle, against each other, against the
hand-derived fixtures and against the preemption oracle's saturated sequences; the nominator
across the grid's idle exits; and the refusals that stay."""
import functools
import time
import types

import numpy as np
import pytest

import k8s_oracle as ko
import nominated_fixtures as nf
import oracle_c
import preempt_compare as pc
import preempt_fixtures as pf
import test_gpu_nominated as tgn
import volume_fuzz
from kss import abi, native, synth
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu

NRF = tgn.FILTER_CODE["NodeResourcesFit"]
RB = 7  # every RB-th scheduled pod is rolled back, unless it is nominated


@functools.lru_cache(maxsize=None)
def _simple_input():
    """Case 1's input: config 2, 150 nodes, 700 pods, priorities and nominations as
    test_gpu_nominated builds them (8 nominated pods among the 600 run, 40 behind them)."""
    nodes, bound, pods = synth.make_cluster(2, 150, 700)
    pods = tgn._with_priorities(pods, 17)
    noms = tgn._noms(pods, 150, 600, 17, inside=8, outside=40)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    return cc, cp, noms, 600


@functools.lru_cache(maxsize=None)
def _program_input():
    """test_gpu_nominated's spread_ipa recipe."""
    nodes, bound, pods = synth.make_cluster(3, 120, 200)
    pods = tgn._with_priorities(pods, 17)
    noms = tgn._noms(pods, 120, 150, 17, inside=6, outside=12)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    return cc, cp, noms, 150


def _skip(n_run, noms):
    """The rollback set: every RB-th pod except the nominated ones (the oracle's skip_commit leaves
    a nomination in place, commit + rollback drops it)."""
    skip = np.zeros(n_run, np.uint8)
    skip[::RB] = 1
    for j, _ in noms:
        if j < n_run:
            skip[j] = 0
    return skip


@functools.lru_cache(maxsize=None)
def _oracle(which, pct, nominated=True):
    cc, cp, noms, n_run = _simple_input() if which == "simple" else _program_input()
    prof = abi.default_profile()
    prof.pct_nodes_to_score = pct
    return oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), n_run, cc.n_nodes, threads=8, record=True,
                             n_classes=len(cc.classes), n_terms=len(cc.terms),
                             nominations=noms if nominated else (), skip_commit=_skip(n_run, noms))


def _copy(v):
    out = types.SimpleNamespace()
    for k in ("fail_plugin", "fail_detail", "raw", "norm", "total"):
        setattr(out, k, None if getattr(v, k) is None else np.array(getattr(v, k)))
    for k in ("chosen", "n_feasible", "scored", "status", "best_total"):
        setattr(out, k, getattr(v, k))
    return out


def _ctx(cc, prof=None):
    ctx = native.Context(prof or abi.default_profile())
    ctx.load(cc.as_struct(), names=native.make_names(cc.node_names, cc.taints, cc.scalars))
    return ctx


def _run_service(which, pct):
    """The service sequence against the C oracle, as test_service_records_match_c_oracle compares:
    outcome, every verdict and detail, raw / normalised / total scores over the kept nodes, the
    cursor, the final node state and the nominations left.  Returns (mode, the records)."""
    cc, cp, noms, n_run = _simple_input() if which == "simple" else _program_input()
    ch_o, res, st = _oracle(which, pct)
    skip = _skip(n_run, noms)
    prof = abi.default_profile()
    prof.pct_nodes_to_score = pct
    ps = cp.as_struct()
    svc = _ctx(cc, prof)
    svc.stage(ps)
    for j, n in noms:
        svc.nominate(ps, j, n)
    N = svc.n_nodes
    recs, mode = [], -1
    for j in range(n_run):
        got = svc.service_eval(j)
        recs.append(_copy(got))
        m = res.meta(j)
        assert (got.chosen, got.n_feasible, got.scored, got.status) == \
               (m["chosen"], m["n_feasible"], m["scored"], m["status"]), (j, m)
        np.testing.assert_array_equal(got.fail_plugin[:N], res.fail_plugin[j, :N], err_msg=f"pod {j} verdicts")
        np.testing.assert_array_equal(got.fail_detail[:N], res.fail_detail[j, :N], err_msg=f"pod {j} details")
        if j == 0:
            mode = svc.service_mode()
        if m["scored"]:
            assert got.best_total == m["best_total"], j
            kept = (res.fail_plugin[j, :N] == 0) & (res.fail_detail[j, :N] != abi.KSS_PASS_NOT_KEPT)
            np.testing.assert_array_equal(got.raw[:, :N][:, kept], res.raw[j][:, :N][:, kept], err_msg=f"pod {j} raw")
            np.testing.assert_array_equal(got.norm[:, :N][:, kept], res.norm[j][:, :N][:, kept], err_msg=f"pod {j} norm")
            np.testing.assert_array_equal(got.total[:N][kept], res.total[j, :N][kept], err_msg=f"pod {j} total")
        if got.chosen >= 0:
            svc.service_commit(j, got.chosen)
            if skip[j]:
                svc.service_rollback(j, got.chosen)
    svc.service_stop()
    assert svc.nominations() == st["nominations"]
    assert svc.next_start_node_index() == st["next_start"]
    g = svc.node_state()
    for k in ("requested", "nonzero", "pod_count"):
        np.testing.assert_array_equal(g[k][..., :N], st[k][..., :N], err_msg=k)
    if len(cc.classes):
        np.testing.assert_array_equal(g["class_count"][:len(cc.classes), :N], st["class_count"][:len(cc.classes), :N])
    svc.close()
    return mode, recs


def _plain_fit(cc, cp, j, req, pods):
    """Per node: NodeResourcesFit's fitsRequest of pod j on the plain node state (no nominee)."""
    a = cc.arrays
    N = cc.n_nodes
    ok = pods[:N].astype(np.int64) + 1 <= a["allowed_pods"][:N]
    fr = cp.pods["fit_request"][j]
    nr = 3 + len(cc.scalars)
    if any(int(fr[r]) != 0 for r in range(nr)):
        for r in range(nr):
            if r >= 3 and int(fr[r]) == 0:
                continue
            ok &= int(fr[r]) <= a["alloc"][r, :N] - req[r, :N]
    return ok


def _sensitive_pods(pct):
    """Non-nominated pods with a NodeResourcesFit verdict on a node whose plain state would pass:
    only the nominees' requests or pod count can have failed it.  The node state before each pod
    is replayed from the oracle's choices (rolled-back pods not assumed)."""
    cc, cp, noms, n_run = _simple_input()
    ch_o, res, _ = _oracle("simple", pct)
    skip = _skip(n_run, noms)
    nominated = {j for j, _ in noms}
    N = cc.n_nodes
    req = np.array(cc.arrays["requested"], np.int64)
    pods = np.array(cc.arrays["pod_count"], np.int64)
    out = []
    for j in range(n_run):
        if j not in nominated:
            hit = (res.fail_plugin[j, :N] == NRF) & _plain_fit(cc, cp, j, req, pods)
            if hit.any():
                out.append(j)
        if ch_o[j] >= 0 and not skip[j]:
            req[:, ch_o[j]] += cp.pods["commit_req"][j]
            pods[ch_o[j]] += 1
    return out


@pytest.mark.parametrize("shards", [0, 5])
@pytest.mark.parametrize("pct", [100, 0])
def test_simple_chain_records_match_c_oracle(pct, shards):
    """Case 1.  Shards automatic, and forced to 5 so that nominees and the nominated node of a
    PreferNominatedNode pod fall into different shards.  The input must exercise the nominee code:
    at least 20 non-nominated pods carry a verdict only a nominee explains, some nominated pod takes
    its node by PreferNominatedNode and some fails it, and nominations are left at the end."""
    cc, cp, noms, n_run = _simple_input()
    ch_o, res, st = _oracle("simple", pct)
    sens = _sensitive_pods(pct)
    assert len(sens) >= 20, sens
    # ... and those rows differ from a run of the same sequence without nominations wherever the two
    # runs still share their state (up to the first differing choice)
    ch_p, res_p, _ = _oracle("simple", pct, nominated=False)
    first = next((j for j in range(n_run) if ch_o[j] != ch_p[j]), n_run)
    for j in sens:
        if j <= first:
            assert (res.fail_plugin[j] != res_p.fail_plugin[j]).any(), j
    where = dict(noms)
    N = cc.n_nodes
    pnn = [j for j in where if j < n_run and ch_o[j] == where[j] and res.meta(j)["scored"] == 0 and
           (res.fail_plugin[j, :N] != abi.KSS_F_NOT_EVALUATED).sum() == 1]
    failed = [j for j in where if j < n_run and res.fail_plugin[j, where[j]] not in (0, abi.KSS_F_NOT_EVALUATED) and
              (res.fail_plugin[j, :N] != abi.KSS_F_NOT_EVALUATED).sum() > 1]
    assert pnn and failed and st["nominations"], (pnn, failed, st["nominations"])
    if shards:
        native.set_option("shards", shards)
    mode, _ = _run_service("simple", pct)
    assert mode in (1, 2), mode


@pytest.mark.parametrize("pct", [100, 0])
def test_general_chain_equals_simple_chain(pct):
    """Case 2.  service_general = 1 keeps the same pods on the general chain (mode 0); its records
    equal the k_simple-shaped chain's entry for entry (both are canonical: every entry written)."""
    mode_s, simple = _run_service("simple", pct)
    assert mode_s in (1, 2), mode_s
    native.set_option("service_general", 1)
    mode_g, general = _run_service("simple", pct)
    assert mode_g == 0, mode_g
    for j, (a, b) in enumerate(zip(simple, general)):
        assert (a.chosen, a.n_feasible, a.scored, a.status, a.best_total) == \
               (b.chosen, b.n_feasible, b.scored, b.status, b.best_total), j
        for k in ("fail_plugin", "fail_detail", "raw", "norm", "total"):
            np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"pod {j} {k}")


@pytest.mark.parametrize("pct", [100, 30])
def test_general_chain_with_programs_matches_c_oracle(pct):
    """Case 3.  Spread and inter-pod programs with nominees (classes, term rows) on the general chain."""
    mode, _ = _run_service("programs", pct)
    assert mode == 0, mode


def test_compact_record_equals_full_under_nominations():
    """Case 4.  kss_service_eval_compact against kss_service_eval on case 1's input at pct 0, pod
    after pod in both orders, the cursor put back between the two evaluations of a pod (the window
    moves it), for the first 120 pods -- and, since this input nominates no pod below 178, for
    the nominated pods of the 600 as well (the pods in between are evaluated once and committed),
    so that PreferNominatedNode pods are among them."""
    cc, cp, noms, n_run = _simple_input()
    prof = abi.default_profile()
    prof.pct_nodes_to_score = 0
    ps = cp.as_struct()
    svc = _ctx(cc, prof)
    svc.stage(ps)
    for j, n in noms:
        svc.nominate(ps, j, n)
    N = svc.n_nodes
    where = dict(noms)
    pnn = 0
    for j in range(n_run):
        if j >= 120 and j not in where:
            r = svc.service_eval(j, abi.KSS_FIELD_FAIL)
            if r.chosen >= 0:
                svc.service_commit(j, r.chosen)
            continue
        c0 = svc.next_start_node_index()
        first = _copy(svc.service_eval_compact(j) if j % 2 else svc.service_eval(j))
        c1 = svc.next_start_node_index()
        svc.set_next_start_node_index(c0)
        second = _copy(svc.service_eval(j) if j % 2 else svc.service_eval_compact(j))
        assert svc.next_start_node_index() == c1, j
        c, f = (first, second) if j % 2 else (second, first)
        assert (c.chosen, c.n_feasible, c.scored, c.status, c.best_total) == \
               (f.chosen, f.n_feasible, f.scored, f.status, f.best_total), j
        for k in ("fail_plugin", "fail_detail", "raw", "norm", "total"):
            a, b = getattr(c, k), getattr(f, k)
            assert a.dtype == {"fail_plugin": np.uint8, "fail_detail": np.uint16, "raw": np.int32,
                               "norm": np.uint8, "total": np.int32}[k], (j, k, a.dtype)
            np.testing.assert_array_equal(a[..., :N].astype(np.int64), b[..., :N].astype(np.int64), err_msg=f"pod {j} {k}")
        if j in where and f.chosen == where[j] and (f.fail_plugin[:N] != abi.KSS_F_NOT_EVALUATED).sum() == 1:
            pnn += 1
            assert (f.n_feasible, f.scored) == (1, 0) and c1 == 0, j
        if f.chosen >= 0:
            svc.service_commit(j, f.chosen)
    assert svc.service_mode() in (1, 2)
    assert pnn >= 1
    svc.close()


def test_fixture_through_the_service():
    """Case 5.  nominated_fixtures.fixture(): stage, nominate, service_eval + service_commit."""
    nodes, bound, pods, noms, expect = nf.fixture()
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    ps = cp.as_struct()
    idx = {n: i for i, n in enumerate(cc.node_names)}
    ctx = _ctx(cc)
    ctx.stage(ps)
    for j, n in noms:
        ctx.nominate(ps, j, idx[n])
    assert ctx.nominations() == [(j, idx[n]) for j, n in noms]
    for j, want in expect:
        r = ctx.service_eval(j)
        got = cc.node_names[r.chosen] if r.chosen >= 0 else None
        assert got == want["selected"], (j, got, want)
        for node, plugin in want.get("fail", {}).items():
            assert int(r.fail_plugin[idx[node]]) == (0 if plugin is None else tgn.FILTER_CODE[plugin]), (j, node)
        if "evaluated" in want:
            ev = sorted(cc.node_names[i] for i in range(cc.n_nodes) if r.fail_plugin[i] != abi.KSS_F_NOT_EVALUATED)
            assert ev == want["evaluated"], j
        if r.chosen >= 0:
            ctx.service_commit(j, r.chosen)
        if "nominated_left" in want:
            assert sorted(cp.names[q][1] for q, _ in ctx.nominations()) == want["nominated_left"], j
    ctx.close()


def test_fixture_without_programs_on_the_simple_chain():
    """The same fixture without its inter-pod pod: every pod is default-shaped, so the expectations
    are checked on the k_simple-shaped chain too."""
    nodes, bound, pods, noms, expect = nf.fixture()
    keep = [i for i in range(len(pods)) if i != 1]
    cc, cp, _ = compile_cluster(nodes, bound, [pods[i] for i in keep])
    ps = cp.as_struct()
    idx = {n: i for i, n in enumerate(cc.node_names)}
    ctx = _ctx(cc)
    ctx.stage(ps)
    for j, n in noms:
        ctx.nominate(ps, keep.index(j), idx[n])
    for j, want in expect:
        if j == 1:
            continue
        k = keep.index(j)
        r = ctx.service_eval(k)
        got = cc.node_names[r.chosen] if r.chosen >= 0 else None
        assert got == want["selected"], (j, got, want)
        for node, plugin in want.get("fail", {}).items():
            assert int(r.fail_plugin[idx[node]]) == (0 if plugin is None else tgn.FILTER_CODE[plugin]), (j, node)
        if "evaluated" in want:
            ev = sorted(cc.node_names[i] for i in range(cc.n_nodes) if r.fail_plugin[i] != abi.KSS_F_NOT_EVALUATED)
            assert ev == want["evaluated"], j
        if r.chosen >= 0:
            ctx.service_commit(k, r.chosen)
        if "nominated_left" in want:
            assert sorted(cp.names[q][1] for q, _ in ctx.nominations()) == want["nominated_left"], j
    assert ctx.service_mode() in (1, 2)
    ctx.close()


def test_window_fixture_cursor_through_the_service():
    """Case 5.  nominated_fixtures.window_fixture(): nextStartNodeIndex counts the nominated node's
    status once more when the search does not reach that node again (101, then 1).  The
    name-listed pod keeps the whole staged list on the general chain under the window; pod 0
    staged alone runs the k_simple-shaped chain to the same cursor."""
    nodes, bound, pods, noms, pct, cursors = nf.window_fixture()
    prof = abi.default_profile()
    prof.pct_nodes_to_score = pct
    for n_staged, want_mode in ((2, (0,)), (1, (1, 2))):
        cc, cp, _ = compile_cluster(nodes, bound, pods[:n_staged])
        idx = {n: i for i, n in enumerate(cc.node_names)}
        ps = cp.as_struct()
        nn = [(j, idx[n]) for j, n in noms if j < n_staged]
        for n_run in range(1, n_staged + 1):
            ch_o, res, st = oracle_c.schedule(prof, cc.as_struct(), ps, n_run, cc.n_nodes, n_classes=len(cc.classes),
                                              n_terms=len(cc.terms), nominations=nn)
            assert st["next_start"] == cursors[n_run - 1]
            ctx = _ctx(cc, prof)
            ctx.stage(ps)
            for j, n in nn:
                ctx.nominate(ps, j, n)
            for j in range(n_run):
                r = ctx.service_eval(j)
                assert r.chosen == ch_o[j], j
                np.testing.assert_array_equal(r.fail_plugin[:cc.n_nodes], res.fail_plugin[j, :cc.n_nodes], err_msg=str(j))
                np.testing.assert_array_equal(r.fail_detail[:cc.n_nodes], res.fail_detail[j, :cc.n_nodes], err_msg=str(j))
                if r.chosen >= 0:
                    ctx.service_commit(j, r.chosen)
            assert ctx.service_mode() in want_mode
            assert ctx.next_start_node_index() == cursors[n_run - 1]
            ctx.close()


def _service_seq(nodes, bound, pods):
    """test_gpu_nominated._device_seq with the evaluation and the commit on the service grid; the
    PostFilter and the nominator calls in between stop the grid, the next service call restarts it."""
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    ps = cp.as_struct()
    ctx = _ctx(cc)
    ctx.load_bound(cc.as_boundset())
    ctx.stage(ps)
    prio = [ko.pod_priority(p) for p in pods]

    queue, tries, out = list(range(cp.n)), [0] * cp.n, []
    while queue:
        j = queue.pop(0)
        r = ctx.service_eval(j, abi.KSS_FIELD_FAIL)
        if r.chosen >= 0:
            ctx.service_commit(j, r.chosen)
            out.append((j, "scheduled", cc.node_names[r.chosen], []))
            continue
        pre = ctx.postfilter_pod(ps, j)
        st = tgn.STATUS[pre["status"]]
        out.append((j,) + pc.from_native(pre, cc, cp))  # the full tuple, as test_gpu_nominated._device_seq
        if st == "nominated":
            node = pre["nominated"]
            ctx.remove_bound(pre["victims"])
            for q, n in ctx.nominations():
                if n == node and prio[q] < prio[j]:
                    ctx.clear_nomination(ps, q)
            ctx.nominate(ps, j, node)
            if tries[j] < 1:
                tries[j] += 1
                queue.append(j)
        elif st == "no_candidate":
            ctx.clear_nomination(ps, j)
    ctx.close()
    return out


@pytest.mark.parametrize("seed,n_nodes,n_pods", [(1, 60, 40), (3, 200, 60)])
def test_saturated_sequence_on_the_service(seed, n_nodes, n_pods):
    """Case 6.  Statuses, nominated nodes, victims and chosen nodes equal
    oracle/k8s_preemption.schedule_with_nominations."""
    nodes, bound, pods = pf.saturated(seed, n_nodes, n_pods)
    want = tgn._oracle_seq(nodes, bound, pods)
    got = _service_seq(nodes, bound, pods)
    assert got == want
    assert any(w[1] == "nominated" for w in want)


def test_nominator_across_idle_exits():
    """Case 7.  Three 4-CPU nodes, n1 holding 1 CPU; "big" (3 CPUs, priority 100) nominated to n2;
    "low" (2 CPUs, priority 0) fails n2 by the nominee alone.  The grid leaves idle, the nominated
    pod is committed (to n1: n2 stays empty) on the relaunched grid, the grid leaves again, and
    low is evaluated on a grid launched with the emptied table: n2 passes, n1 is full."""
    nodes = [nf._node("n1"), nf._node("n2"), nf._node("n3")]
    bound = [nf._pod("b1", "1", 0, node="n1"), nf._pod("b3", "3", 0, node="n3")]
    pods = [nf._pod("low", "2", 0, {"app": "low"}), nf._pod("big", "3", 100, {"app": "big"})]
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    ps = cp.as_struct()
    idx = {n: i for i, n in enumerate(cc.node_names)}
    ctx = _ctx(cc)
    ctx.stage(ps)
    ctx.nominate(ps, 1, idx["n2"])
    r = ctx.service_eval(0)
    assert ctx.service_mode() in (1, 2)
    assert [int(r.fail_plugin[idx[n]]) for n in ("n1", "n2", "n3")] == [0, NRF, NRF]
    time.sleep(2.5)  # the grid leaves after ~1 s idle
    ctx.service_commit(1, idx["n1"])
    assert ctx.nominations() == []
    r = ctx.service_eval(0)  # the grid that took the commit: the entry's bit is cleared
    assert [int(r.fail_plugin[idx[n]]) for n in ("n1", "n2", "n3")] == [NRF, 0, NRF]
    time.sleep(2.5)
    r = ctx.service_eval(0)  # relaunched with the table as it stands: empty
    assert [int(r.fail_plugin[idx[n]]) for n in ("n1", "n2", "n3")] == [NRF, 0, NRF]
    assert r.chosen == idx["n2"]
    assert ctx.nominations() == []
    ctx.close()


def test_refusals_that_stay():
    """Case 8.  With a non-empty nominator a split-configured context still refuses, and a
    nominated pod with volumes is still refused."""
    cc, cp, noms, _ = _simple_input()
    ps = cp.as_struct()
    ctx = _ctx(cc)
    ctx.stage(ps)
    ctx.nominate(ps, noms[0][0], noms[0][1])
    ctx.split_config(2, 0, 4)
    ctx.split_peers([ctx.split_inbox()[0]] * 2)
    with pytest.raises(native.KssError, match="one device"):
        ctx.service_eval(0)
    with pytest.raises(native.KssError, match="nominator"):
        ctx.run_staged(4)
    with pytest.raises(native.KssError, match="nominator"):
        ctx.nominate(ps, noms[1][0], noms[1][1])
    ctx.close()
    vnodes, vbound, vpods, st = volume_fuzz.make(1, n_nodes=30, n_bound=30, n_pods=20)
    vc, vp, _ = compile_cluster(vnodes, vbound, vpods, storage=st)
    with_vols = [j for j in range(vp.n) if vp.pods["vol_len"][j] > 0]
    without = [j for j in range(vp.n) if vp.pods["vol_len"][j] == 0]
    assert with_vols and without
    ctx = native.Context(abi.default_profile())
    ctx.load(vc.as_struct())
    vs = vp.as_struct()
    ctx.stage(vs)
    ctx.nominate(vs, without[0], 0)
    ctx.service_eval(0)  # the service takes the volume-free nominee
    with pytest.raises(native.KssError, match="volumes"):
        ctx.nominate(vs, with_vols[0], 0)
    assert ctx.nominations() == [(without[0], 0)]
    ctx.service_eval(1)  # and runs on with the nominator as it was
    ctx.close()


def _name_list(names):
    # one term per name (a field selector's In takes exactly one value); the terms' union is the list
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
        {"matchFields": [{"key": "metadata.name", "operator": "In", "values": [n]}]} for n in names]}}}


@functools.lru_cache(maxsize=None)
def _name_list_input():
    """NodeAffinity PreFilterResult lists next to nominees, at pct 100 (where a staged list with
    name-listed pods stays on the k_simple-shaped chain).  Twelve 4-CPU nodes m00..m11; m11 is full.
    "out" (3 CPUs, priority 100) is nominated to m08, "big" (3 CPUs, priority 100) to m02.

      0 lst    (2 CPUs, list m00..m03)  m02 fails NodeResourcesFit by big alone; m08 holds a nominee
               but lies outside the list: never filtered, whatever the first pass would say.
      1 lstnom (1 CPU, list m00..m03, nominated to m11)  evaluateNominatedNode filters m11 although
               it is outside the list: NodeAffinity; that status stands in the record of the full
               search, and its map entry is one more than the 4 listed nodes: cursor 5 % 4 = 1.
      2 plain  (1 CPU)  the whole node list: the cursor stays 1.
      3 lst3   (1 CPU, list m00..m02)  cursor 1 % 3 = 1.
      4 lstnom2 (1 CPU, list m00..m03, nominated to m08, where out is nominated too)  NodeAffinity again.
      5 lst1   (1 CPU, list m01)  cursor 1 % 1 = 0.
      6 out, 7 big  PreferNominatedNode."""
    nodes = [nf._node("m%02d" % i) for i in range(12)]
    bound = [nf._pod("fill", "4", 0, node="m11")]
    l4, l3, l1 = ["m%02d" % i for i in range(4)], ["m%02d" % i for i in range(3)], ["m01"]
    pods = [nf._pod("lst", "2", 0, {"app": "lst"}, affinity=_name_list(l4)),
            nf._pod("lstnom", "1", 0, {"app": "lstnom"}, affinity=_name_list(l4)),
            nf._pod("plain", "1", 0, {"app": "plain"}),
            nf._pod("lst3", "1", 0, {"app": "lst3"}, affinity=_name_list(l3)),
            nf._pod("lstnom2", "1", 0, {"app": "lstnom2"}, affinity=_name_list(l4)),
            nf._pod("lst1", "1", 0, {"app": "lst1"}, affinity=_name_list(l1)),
            nf._pod("out", "3", 100, {"app": "out"}),
            nf._pod("big", "3", 100, {"app": "big"})]
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    idx = {n: i for i, n in enumerate(cc.node_names)}
    noms = [(6, idx["m08"]), (7, idx["m02"]), (1, idx["m11"]), (4, idx["m08"])]
    return cc, cp, noms, idx


@pytest.mark.parametrize("general", [0, 1])
def test_name_lists_with_nominees_at_pct_100(general):
    """A node outside a pod's PreFilterResult list stays KSS_F_NOT_EVALUATED although it holds a
    nominee, and a pod nominated outside its own list gets that node's real status and the cursor
    the extra map entry leaves -- on the k_simple-shaped chain and on the general chain, against
    the C oracle after every prefix of the sequence (the oracle reports the final cursor)."""
    cc, cp, noms, idx = _name_list_input()
    ps = cp.as_struct()
    N = cc.n_nodes
    prof = abi.default_profile()
    NA, NE = tgn.FILTER_CODE["NodeAffinity"], abi.KSS_F_NOT_EVALUATED
    runs = [oracle_c.schedule(prof, cc.as_struct(), ps, n_run, N, record=True, n_classes=len(cc.classes),
                              n_terms=len(cc.terms), nominations=noms) for n_run in range(1, cp.n + 1)]
    ch_o, res, st = runs[-1]
    # the hand-derived facts above, on the oracle's own records
    listed = [idx["m%02d" % i] for i in range(4)]
    outside = [i for i in range(N) if i not in listed]
    assert int(res.fail_plugin[0, idx["m02"]]) == NRF and (res.fail_plugin[0, outside] == NE).all()
    for j, node in ((1, idx["m11"]), (4, idx["m08"])):
        assert int(res.fail_plugin[j, node]) == NA
        assert (res.fail_plugin[j, [i for i in outside if i != node]] == NE).all() and ch_o[j] in listed
    assert [r[2]["next_start"] for r in runs[:6]] == [0, 1, 1, 1, 1, 0]
    assert (ch_o[6], ch_o[7]) == (idx["m08"], idx["m02"]) and st["nominations"] == []
    if general:
        native.set_option("service_general", 1)
    ctx = _ctx(cc, prof)
    ctx.stage(ps)
    for j, n in noms:
        ctx.nominate(ps, j, n)
    for j in range(cp.n):
        got = ctx.service_eval(j)
        if j == 0:
            assert ctx.service_mode() == 0 if general else ctx.service_mode() in (1, 2)
        m = res.meta(j)
        assert (got.chosen, got.n_feasible, got.scored, got.status) == \
               (m["chosen"], m["n_feasible"], m["scored"], m["status"]), (j, m)
        np.testing.assert_array_equal(got.fail_plugin[:N], res.fail_plugin[j, :N], err_msg=f"pod {j} verdicts")
        np.testing.assert_array_equal(got.fail_detail[:N], res.fail_detail[j, :N], err_msg=f"pod {j} details")
        if m["scored"]:
            kept = res.fail_plugin[j, :N] == 0
            np.testing.assert_array_equal(got.raw[:, :N][:, kept], res.raw[j][:, :N][:, kept], err_msg=f"pod {j} raw")
            np.testing.assert_array_equal(got.norm[:, :N][:, kept], res.norm[j][:, :N][:, kept], err_msg=f"pod {j} norm")
            np.testing.assert_array_equal(got.total[:N][kept], res.total[j, :N][kept], err_msg=f"pod {j} total")
        # a second cycle of the same pod, as a compact record: the same verdicts, and (below) the same cursor
        c = ctx.service_eval_compact(j)
        assert c.chosen == got.chosen, j
        np.testing.assert_array_equal(c.fail_plugin[:N], res.fail_plugin[j, :N], err_msg=f"pod {j} compact verdicts")
        if got.chosen >= 0:
            ctx.service_commit(j, got.chosen)
        assert ctx.next_start_node_index() == runs[j][2]["next_start"], j
    assert ctx.nominations() == st["nominations"]
    ctx.close()
