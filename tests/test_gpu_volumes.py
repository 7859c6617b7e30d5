"""The volume plugins on the device (k_schedule; k_simple / k_spread refuse volume programs):
the hand-derived fixtures of tests/volume_fixtures.py as recorded batches, unrecorded
batches and through the per-pod eval / commit API, byte for byte against the object-level
oracle's annotations; the random volume clusters of tests/volume_fuzz.py bit-exactly against
the C oracle (every verdict, detail, score, choice, and the final vol_count / vol_attached
state); rollback and the volume delta sync; the refusals (node axis, sweeps, PostFilter)."""
import numpy as np
import pytest

import edge_fixtures as ef
import k8s_oracle
import k8s_volumes
import oracle_c
import volume_fixtures as vf
import volume_fuzz
import volume_rollback as vr
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu


def _want(nodes, bound, pods, st):
    o = k8s_oracle.Oracle(nodes, bound, storage=k8s_volumes.Storage(st["pvs"], st["pvcs"], st["storage_classes"],
                                                                      st["csinodes"]))
    return [o.annotations(o.schedule_one(p)) for p in pods]


def _ctx(cc, cp, n_record):
    ctx = native.Context(abi.default_profile(), max_pods_record=n_record)
    ctx.load(cc.as_struct(), names=native.make_names(cc.node_names, cc.taints, cc.scalars, cp.messages))
    return ctx


@pytest.mark.parametrize("name", sorted(vf.FIXTURES))
def test_recorded_batch_matches_hand_derived(name):
    nodes, bound, pods, expect, st = vf.FIXTURES[name]()
    want = _want(nodes, bound, pods, st)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    ps = cp.as_struct()
    ctx = _ctx(cc, cp, cp.n)
    chosen = ctx.schedule_batch(ps, cp.n, record=True)
    assert ctx.last_kernel() == "k_schedule"
    for j, exp in enumerate(expect):
        ann = ctx.format_annotations(ctx.fetch_record(j), ps, j)
        assert ann == want[j], (name, j)
        ef.check_expect(ann, exp, where=(name, j))
        sel = want[j]["scheduler-simulator/selected-node"]
        assert (cc.node_names[chosen[j]] if chosen[j] >= 0 else "") == sel, (name, j)
    ctx.close()


@pytest.mark.parametrize("name", sorted(vf.FIXTURES))
def test_unrecorded_and_per_pod_paths(name):
    nodes, bound, pods, expect, st = vf.FIXTURES[name]()
    want = _want(nodes, bound, pods, st)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    ps = cp.as_struct()
    ctx = _ctx(cc, cp, 1)
    chosen = ctx.schedule_batch(ps, cp.n)
    assert [cc.node_names[c] if c >= 0 else "" for c in chosen] == [a["scheduler-simulator/selected-node"]
                                                                    for a in want]
    ctx.reset()
    for j, exp in enumerate(expect):  # PreFilter -> kss_eval_pod, Reserve -> kss_commit
        r = ctx.eval_pod(ps, j)
        assert ctx.format_annotations(r, ps, j) == want[j], (name, j)
        if r.chosen >= 0:
            ctx.commit(ps, j, r.chosen)
    ctx.close()


def _oracle(cc, cp, record=True):
    return oracle_c.schedule(abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record=record,
                             n_classes=len(cc.classes), n_terms=len(cc.terms))


@pytest.mark.parametrize("seed", range(8))
def test_random_volume_clusters_match_oracle(seed):
    nodes, bound, pods, st = volume_fuzz.make(seed)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    ch_o, res, fin = _oracle(cc, cp)
    ctx = native.Context(abi.default_profile(), max_pods_record=cp.n)
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n, record=True)
    np.testing.assert_array_equal(chosen, ch_o)
    N = cc.n_nodes
    for j in range(cp.n):
        r = ctx.fetch_record(j)
        np.testing.assert_array_equal(r.fail_plugin[:N], res.fail_plugin[j], err_msg=f"pod {j}")
        np.testing.assert_array_equal(r.fail_detail[:N], res.fail_detail[j], err_msg=f"pod {j}")
        if r.scored:
            feas = res.fail_plugin[j] == 0
            np.testing.assert_array_equal(r.total[feas], res.total[j][feas], err_msg=f"pod {j}")
    vc, va = ctx.volume_state()
    np.testing.assert_array_equal(vc, fin["vol_count"])
    np.testing.assert_array_equal(va, fin["vol_attached"])
    ctx.close()


@pytest.mark.parametrize("seed,n_nodes,n_pods,flags", [(21, 400, 300, 0), (22, 3000, 200, 0),
                                                       (23, 200, 150, abi.KSS_SCHED_FORCE_SINGLE_WG)])
def test_larger_unrecorded_batches(seed, n_nodes, n_pods, flags):
    nodes, bound, pods, st = volume_fuzz.make(seed, n_nodes=n_nodes, n_bound=n_nodes, n_pods=n_pods)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    ch_o, _, fin = _oracle(cc, cp, record="meta")
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    np.testing.assert_array_equal(ctx.schedule_batch(cp.as_struct(), cp.n, flags=flags), ch_o)
    vc, va = ctx.volume_state()
    np.testing.assert_array_equal(vc, fin["vol_count"])
    np.testing.assert_array_equal(va, fin["vol_attached"])
    ctx.close()


def test_rollback_and_volume_delta():
    """kss_rollback undoes a commit's volume rows and attach counts (ForgetPod); the delta sync
    overwrites cells and a reset restores the snapshot."""
    nodes, bound, pods, st = volume_fuzz.make(3)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    ps = cp.as_struct()
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    vc0, va0 = ctx.volume_state()
    done = []
    for j in range(cp.n):
        r = ctx.eval_pod(ps, j)
        if r.chosen >= 0:
            ctx.commit(ps, j, r.chosen)
            done.append((j, r.chosen))
    vc1, va1 = ctx.volume_state()
    assert (vc1 != vc0).any() and (va1 != va0).any()
    for j, n in reversed(done):
        ctx.rollback(ps, j, n)
    vc2, va2 = ctx.volume_state()
    np.testing.assert_array_equal(vc2, vc0)
    np.testing.assert_array_equal(va2, va0)
    R = len(cc.vol_rows)
    ctx.apply_volume_delta([0, 1], [0, R], [7, 9], overwrite=True)
    vc3, va3 = ctx.volume_state()
    assert vc3[0, 0] == 7 and va3[0, 1] == 9
    ctx.reset()
    vc4, va4 = ctx.volume_state()
    np.testing.assert_array_equal(vc4, vc0)
    np.testing.assert_array_equal(va4, va0)
    ctx.close()


def test_refusals():
    nodes, bound, pods, st = volume_fuzz.make(4)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    ps = cp.as_struct()
    with pytest.raises(native.KssError, match="volumes"):
        native.Sweep(abi.default_profile(), [cc.as_struct()], [ps])
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    j = next(i for i in range(cp.n) if cp.pods[i]["vol_len"] > 0)
    with pytest.raises(native.KssError, match="volumes"):
        ctx.postfilter_pod(ps, j)
    ctx.close()


def _binding_equal(ctx, fin):
    po, cn = ctx.binding_state()
    np.testing.assert_array_equal(po, fin["pv_owner"])
    np.testing.assert_array_equal(cn, fin["claim_node"])


@pytest.mark.parametrize("seed,n_nodes,flags", [(100, 12, 0), (103, 12, 0), (105, 12, abi.KSS_SCHED_FORCE_MULTI_WG),
                                                (108, 12, 0), (111, 12, 0), (114, 300, 0)])
def test_random_wffc_clusters_match_oracle(seed, n_nodes, flags):
    """Unbound WaitForFirstConsumer claims (binder.go FindPodVolumes / AssumePodVolumes) on random
    clusters against the C oracle: every verdict and detail (bind conflicts, the joined node + bind
    reason), choice and total, the vol_count / vol_attached state and the assume cache the batch
    leaves (pv_owner, claim_node) -- on one shard and on several (every shard applies the assume)."""
    nodes, bound, pods, st = volume_fuzz.make(seed, n_nodes=n_nodes, n_bound=max(16, n_nodes), wffc=True)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    assert cc.wclaims
    ch_o, res, fin = _oracle(cc, cp)
    ctx = native.Context(abi.default_profile(), max_pods_record=cp.n)
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n, record=True, flags=flags)
    if flags:
        assert ctx.last_geometry()["shards"] > 1
    np.testing.assert_array_equal(chosen, ch_o)
    N = cc.n_nodes
    for j in range(cp.n):
        r = ctx.fetch_record(j)
        np.testing.assert_array_equal(r.fail_plugin[:N], res.fail_plugin[j], err_msg=f"pod {j}")
        np.testing.assert_array_equal(r.fail_detail[:N], res.fail_detail[j], err_msg=f"pod {j}")
        if r.scored:
            feas = res.fail_plugin[j] == 0
            np.testing.assert_array_equal(r.total[feas], res.total[j][feas], err_msg=f"pod {j}")
    vc, va = ctx.volume_state()
    np.testing.assert_array_equal(vc, fin["vol_count"])
    np.testing.assert_array_equal(va, fin["vol_attached"])
    _binding_equal(ctx, fin)
    ctx.reset()  # the snapshot's assume cache back
    po, cn = ctx.binding_state()
    np.testing.assert_array_equal(po, cc.arrays["pv_owner"][:len(cc.pvs)])
    np.testing.assert_array_equal(cn, cc.arrays["claim_node"][:len(cc.wclaims)])
    ctx.close()


def _state_equal(ctx, fs, k, where):
    """binding_state() and volume_state() against the C oracle's trace after step k."""
    po, cn = ctx.binding_state()
    vc, va = ctx.volume_state()
    tr = fs["trace"]
    np.testing.assert_array_equal(po, tr["pv_owner"][k], err_msg=f"{where} step {k} pv_owner")
    np.testing.assert_array_equal(cn, tr["claim_node"][k], err_msg=f"{where} step {k} claim_node")
    np.testing.assert_array_equal(vc, tr["vol_count"][k], err_msg=f"{where} step {k} vol_count")
    np.testing.assert_array_equal(va, tr["vol_attached"][k], err_msg=f"{where} step {k} vol_attached")


def _record_equal(r, res, k, N, where):
    np.testing.assert_array_equal(r.fail_plugin[:N], res.fail_plugin[k, :N], err_msg=f"{where} step {k} verdicts")
    np.testing.assert_array_equal(r.fail_detail[:N], res.fail_detail[k, :N], err_msg=f"{where} step {k} details")
    m = res.meta(k)
    assert (r.chosen, r.n_feasible, r.scored) == (m["chosen"], m["n_feasible"], m["scored"]), (where, k, m)
    if m["scored"]:
        feas = res.fail_plugin[k, :N] == 0
        np.testing.assert_array_equal(r.total[:N][feas], res.total[k, :N][feas], err_msg=f"{where} step {k} totals")


def _run_program(ctx, ps, ops, res, fs, chosen, N, path, where, state_every_step=True):
    """A rollback program (tests/volume_rollback.py) on the per-pod API (eval_pod / commit /
    rollback) or the resident service grid (service_eval / service_commit / service_rollback):
    every evaluation's record and choice and, after every step, the volume columns and the assume
    cache against the C oracle's.  Reading state stops the service grid (the next command starts
    it again); state_every_step=False reads it only at the end, the grid resident throughout."""
    on = {}
    for k, op in enumerate(ops):
        j = op if op >= 0 else -1 - op
        if op >= 0:
            r = ctx.eval_pod(ps, j) if path == "per_pod" else ctx.service_eval(j)
            _record_equal(r, res, k, N, where)
            if r.chosen >= 0:
                on[j] = r.chosen
                ctx.commit(ps, j, r.chosen) if path == "per_pod" else ctx.service_commit(j, r.chosen)
        elif j in on:
            n = on.pop(j)
            assert n == chosen[k], (where, k)
            ctx.rollback(ps, j, n) if path == "per_pod" else ctx.service_rollback(j, n)
        if state_every_step or k == len(ops) - 1:
            _state_equal(ctx, fs, k, where)


def test_wffc_per_pod_commit_rollback_and_service():
    """The drop-in's per-pod shape with WaitForFirstConsumer claims: kss_eval_pod + kss_commit
    (Reserve's AssumePodVolumes through k_wffc_commit) pod after pod equals the batch oracle and
    its assume cache; kss_rollback in reverse (RevertAssumedPodVolumes), compared with the C
    oracle's rollback() after each one, ends at the snapshot's; the resident service grid (eval +
    queued commits, every shard applying the assume) does the same."""
    nodes, bound, pods, st = volume_fuzz.make(100, wffc=True)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    ps = cp.as_struct()
    ch_o, _, fin = _oracle(cc, cp, record="meta")
    ops = list(range(cp.n)) + [-1 - j for j in reversed(range(cp.n)) if ch_o[j] >= 0]
    _, _, fs = vr.run_c_oracle(cc, cp, ops, record="meta")
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    done = []
    for j in range(cp.n):
        r = ctx.eval_pod(ps, j)
        assert r.chosen == ch_o[j], j
        if r.chosen >= 0:
            ctx.commit(ps, j, r.chosen)
            done.append((j, r.chosen))
    _binding_equal(ctx, fin)
    for k, (j, n) in enumerate(reversed(done)):
        ctx.rollback(ps, j, n)
        _state_equal(ctx, fs, cp.n + k, "reverse")
    po, cn = ctx.binding_state()
    np.testing.assert_array_equal(po, cc.arrays["pv_owner"][:len(cc.pvs)])
    np.testing.assert_array_equal(cn, cc.arrays["claim_node"][:len(cc.wclaims)])
    ctx.reset()
    ctx.stage(ps)
    for j in range(cp.n):
        v = ctx.service_eval(j)
        assert v.chosen == ch_o[j], j
        if v.chosen >= 0:
            ctx.service_commit(j, v.chosen)
    ctx.service_stop()
    _binding_equal(ctx, fin)
    ctx.close()


@pytest.mark.parametrize("path", ["per_pod", "service", "batch_prefix"])
@pytest.mark.parametrize("case", ["provisioned_elsewhere", "rebound_same_pv"])
def test_shared_claim_rollback_fixture(case, path):
    """fx_wffc_shared_claim_rollback on the device: a rollback restores the rolled-back pod's own
    picks only (provisioned_elsewhere: pv-x stays pod-b's when pod-a, which provisioned the shared
    claim in the other zone, is rolled back) and all of them (rebound_same_pv: pv-x, which pod-a
    bound again, goes back to the snapshot).  Per-pod API and service grid: every step's record and
    state against the C oracle, the state after every step against the literals, the annotations
    against the object oracle; schedule_batch: the two commits before the rollback."""
    nodes, bound, pods, steps, expect, st = vf.fx_wffc_shared_claim_rollback()[case]
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    ps = cp.as_struct()
    N = cc.n_nodes
    chosen, res, fs = vr.run_c_oracle(cc, cp, steps)
    ctx = _ctx(cc, cp, cp.n)
    if path == "batch_prefix":
        got = ctx.schedule_batch(ps, 2, record=True)
        np.testing.assert_array_equal(got, chosen[:2])
        for k in range(2):
            _record_equal(ctx.fetch_record(k), res, k, N, case)
        _state_equal(ctx, fs, 1, case)
        b, s = vr.decode(cc, *ctx.binding_state())
        assert ({c: pv for pv, c in b.items()}, s) == (expect[1]["bound"], expect[1]["selected_nodes"])
        ctx.close()
        return
    want = vr.run_object_oracle(nodes, bound, pods, st, steps)
    if path == "service":
        ctx.stage(ps)
    on = {}
    for k, (op, exp) in enumerate(zip(steps, expect)):
        j = op if op >= 0 else -1 - op
        if op >= 0:
            r = ctx.eval_pod(ps, j) if path == "per_pod" else ctx.service_eval(j)
            _record_equal(r, res, k, N, case)
            if path == "per_pod":
                ann = ctx.format_annotations(r, ps, j)
                assert ann == want[k]["ann"], (case, k)
                ef.check_expect(ann, exp, where=(case, k))
            assert (cc.node_names[r.chosen] if r.chosen >= 0 else "") == exp["selected"], (case, k)
            on[j] = r.chosen
            ctx.commit(ps, j, r.chosen) if path == "per_pod" else ctx.service_commit(j, r.chosen)
        else:
            n = on.pop(j)
            ctx.rollback(ps, j, n) if path == "per_pod" else ctx.service_rollback(j, n)
        _state_equal(ctx, fs, k, case)
        b, s = vr.decode(cc, *ctx.binding_state())
        assert ({c: pv for pv, c in b.items()}, s) == (exp["bound"], exp["selected_nodes"]), (case, k)
    if path == "service":
        ctx.service_stop()
    ctx.close()


ROLLBACK_ORDERS = {"immediate": lambda n: vr.ops_immediate(n, 3), "lifo": lambda n: vr.ops_lifo(n, 3, 5)}


@pytest.mark.parametrize("path", ["per_pod", "service"])
@pytest.mark.parametrize("order", sorted(ROLLBACK_ORDERS))
@pytest.mark.parametrize("seed,n_nodes,shards", [(101, 4, 0), (116, 12, 0), (118, 300, 5)])
def test_rollback_programs_match_oracle(seed, n_nodes, shards, order, path):
    """The rollback fuzz on the device: random WaitForFirstConsumer clusters whose pods share w-*
    claims, 40 pods, under the immediate pattern (every third pod: commit, rollback, go on) and
    the LIFO pattern (after every five pods the last three rolled back, newest first) -- on the
    per-pod API and on the service grid, at 4 and 12 nodes and at 300 with the service grid forced
    to 5 shards (every shard applies the rollback to the global columns).  Every evaluation's
    verdicts, details, totals and choice, and the volume columns and the assume cache after every
    step, equal the C oracle's (commit() / rollback() of the recorded picks)."""
    nodes, bound, pods, st = volume_fuzz.make(seed, n_nodes=n_nodes, n_bound=max(16, n_nodes), wffc=True)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    assert cc.wclaims
    ps = cp.as_struct()
    ops = ROLLBACK_ORDERS[order](cp.n)
    chosen, res, fs = vr.run_c_oracle(cc, cp, ops)
    if shards:
        native.set_option("shards", shards)
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    if path == "service":
        ctx.stage(ps)
    _run_program(ctx, ps, ops, res, fs, chosen, cc.n_nodes, path, (seed, order, path))
    if path == "service":
        if shards:
            assert ctx.last_geometry()["shards"] > 1
        ctx.service_stop()
    ctx.close()


def test_rollback_program_on_a_resident_service_grid():
    """The LIFO program on the service grid without reading state in between: the grid stays
    resident from the first evaluation to the last rollback (commits and rollbacks queued behind
    the evaluations), the records are compared pod by pod and the state at the end."""
    nodes, bound, pods, st = volume_fuzz.make(116, wffc=True)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    ps = cp.as_struct()
    ops = ROLLBACK_ORDERS["lifo"](cp.n)
    chosen, res, fs = vr.run_c_oracle(cc, cp, ops)
    ctx = native.Context(abi.default_profile())
    ctx.load(cc.as_struct())
    ctx.stage(ps)
    _run_program(ctx, ps, ops, res, fs, chosen, cc.n_nodes, "service", "resident", state_every_step=False)
    ctx.service_stop()
    ctx.close()


def test_empty_topology_terms_match_c_oracle():
    """fx_allowed_topologies_empty_terms on the device against the C oracle (the object oracle and
    the literals: the FIXTURES tests above, recorded batch and per-pod API): every verdict and
    detail of the recorded batch, the hand-derived bind-conflict detail per node, and the assume
    cache it leaves; then the same pods through the service grid, record by record."""
    nodes, bound, pods, expect, st = vf.fx_allowed_topologies_empty_terms()
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    chosen, res, fs = vr.run_c_oracle(cc, cp, list(range(cp.n)))
    ctx = _ctx(cc, cp, cp.n)
    got = ctx.schedule_batch(cp.as_struct(), cp.n, record=True)
    np.testing.assert_array_equal(got, chosen)
    for j, exp in enumerate(expect):
        r = ctx.fetch_record(j)
        _record_equal(r, res, j, cc.n_nodes, "empty terms")
        for i, n in enumerate(cc.node_names):
            want = (abi.KSS_F_VOLUME_BINDING, abi.KSS_VB_BIND_CONFLICT) if exp["vb"][n] == "bind" else (0, 0)
            assert (int(r.fail_plugin[i]), int(r.fail_detail[i]) if want[0] else 0) == want, (j, n)
    _state_equal(ctx, fs, cp.n - 1, "empty terms")
    assert vr.decode(cc, *ctx.binding_state()) == ({}, vf.EMPTY_TERMS_FINAL_SELECTED)
    ctx.reset()  # the same pods through the service grid
    ps = cp.as_struct()
    ctx.stage(ps)
    _run_program(ctx, ps, list(range(cp.n)), res, fs, chosen, cc.n_nodes, "service", "empty terms, service")
    ctx.service_stop()
    assert vr.decode(cc, *ctx.binding_state()) == ({}, vf.EMPTY_TERMS_FINAL_SELECTED)
    ctx.close()
