"""The volume plugins on CPU: both oracles (object-level oracle/k8s_volumes.py and the SoA-level
C oracle over kss/volumes.py's compiled programs) and the lazy annotation formatter against
the hand-derived fixtures of tests/volume_fixtures.py (disk conflicts, the in-tree and CSI
attach limits, VolumeBinding PreFilter / Filter, VolumeZone), and against each other on
random clusters with volumes (tests/volume_fuzz.py)."""
import json

import numpy as np
import pytest

import edge_fixtures as ef
import k8s_oracle
import k8s_volumes
import volume_fixtures as vf
from crosscheck import run_both
from kss import abi
from kss.compile import Unsupported, compile_cluster
from test_format import _format_from_oracle


def _oracle(nodes, bound, st):
    return k8s_oracle.Oracle(nodes, bound, storage=k8s_volumes.Storage(
        st["pvs"], st["pvcs"], st["storage_classes"], st["csinodes"]))


@pytest.mark.parametrize("name", sorted(vf.FIXTURES))
def test_object_oracle_matches_hand_derived(name):
    nodes, bound, pods, expect, st = vf.FIXTURES[name]()
    o = _oracle(nodes, bound, st)
    for j, (p, exp) in enumerate(zip(pods, expect)):
        ef.check_expect(o.annotations(o.schedule_one(p)), exp, where=(name, j))


@pytest.mark.parametrize("name", sorted(vf.FIXTURES))
def test_c_oracle_and_formatter_match_hand_derived(name):
    nodes, bound, pods, expect, st = vf.FIXTURES[name]()
    cc, cp, chosen, res = run_both(nodes, bound, pods, storage=st)  # the two oracles agree first
    prof = abi.default_profile()
    o = _oracle(nodes, bound, st)
    for j, exp in enumerate(expect):
        ann = _format_from_oracle(cc, cp, res, j, prof, pod_aware=True)
        assert ann == o.annotations(o.schedule_one(pods[j])), (name, j)  # all 13 values, byte for byte
        ef.check_expect(ann, exp, where=(name, j))


def test_every_volume_reason_is_covered():
    seen, pre = set(), set()
    for fx in vf.FIXTURES.values():
        for exp in fx()[3]:
            seen.update(f[1] for f in exp["filter"].values() if f is not None)
            st = (exp.get("extra") or {}).get("scheduler-simulator/prefilter-result-status")
            if st:
                pre.add(st["VolumeBinding"])
    for msg in (vf.M_DISK, vf.M_MAXVOL, vf.M_VB_CONFLICT, vf.M_VB_NOPV, vf.M_ZONE, vf.M_VB_BIND,
                vf.M_VB_CONFLICT + ", " + vf.M_VB_BIND):
        assert msg in seen, msg
    assert vf.M_UNBOUND in pre
    plugins = {f[0] for fx in vf.FIXTURES.values() for exp in fx()[3] for f in exp["filter"].values() if f}
    assert {"VolumeRestrictions", "EBSLimits", "GCEPDLimits", "NodeVolumeLimits", "AzureDiskLimits",
            "VolumeBinding", "VolumeZone"} <= plugins


def test_volume_rows_and_keys():
    """Shared volumes get vol_count rows, private ones count on the chosen node only; the
    attach-limit keys follow the plugin order."""
    nodes, bound, pods, _, st = vf.fx_csi_limits()
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    assert cc.vol_keys == ["attachable-volumes-csi-ebs.csi.aws.com"]
    shared = sorted(u for kind, (k, u) in cc.vol_rows if kind == "vol")
    assert shared == ["ebs.csi.aws.com/h-1", "ebs.csi.aws.com/h-2", "ebs.csi.aws.com/h-3"]
    a = cc.arrays
    assert list(a["vol_attached"][0]) == [1, 1, 0]  # x's h-1 on a, y's unbound u-1 on b
    assert list(a["vol_limit"][0]) == [1, 3, -1]


def test_intree_rbd_provisioner_is_not_a_csi_driver():
    """csi-translation-lib (v1.26) lists the in-tree RBD plugin: with migration off, an unbound
    claim whose StorageClass provisioner is kubernetes.io/rbd has no CSI driver
    (getCSIDriverInfoFromSC returns ""), so it counts toward no attach-limit key, while a CSI
    provisioner's claim does; an inline rbd volume on a node whose CSINode lists the plugin as
    migrated is refused like the other migratable sources (parity unpinned: the translation
    lib is not vendored under the reference)."""
    nodes = [ef.node("a"), ef.node("b")]
    st = vf.storage(pvs=[vf.pv("pv-1", vf.csi("ebs.csi.aws.com", "h-1"))],
                    pvcs=[vf.pvc("u-rbd", bound=False, sc="rbd-sc"), vf.pvc("u-csi", bound=False, sc="csi-sc"),
                          vf.pvc("c-1", "pv-1")],
                    scs=[{"metadata": {"name": "rbd-sc"}, "provisioner": "kubernetes.io/rbd",
                          "volumeBindingMode": "Immediate"},
                         {"metadata": {"name": "csi-sc"}, "provisioner": "ebs.csi.aws.com",
                          "volumeBindingMode": "Immediate"}],
                    csinodes=[{"metadata": {"name": n}, "spec": {"drivers": [
                        {"name": "ebs.csi.aws.com", "allocatable": {"count": 5}},
                        {"name": "kubernetes.io/rbd", "allocatable": {"count": 5}}]}} for n in "ab"])
    bound = [vf.vpod("x", vf.claim("u-rbd"), node_name="a"), vf.vpod("y", vf.claim("u-csi"), node_name="b")]
    cc, cp, _ = compile_cluster(nodes, bound, [vf.vpod("p", vf.claim("c-1"))], storage=st)
    assert cc.vol_keys == ["attachable-volumes-csi-ebs.csi.aws.com"]
    assert list(cc.arrays["vol_attached"][0]) == [0, 1]
    mig = [{"metadata": {"name": "a", "annotations": {"storage.alpha.kubernetes.io/migrated-plugins":
                                                      "kubernetes.io/rbd"}}, "spec": {"drivers": []}}]
    with pytest.raises(Unsupported, match="migrated"):
        compile_cluster([ef.node("a")], [], [vf.vpod("p", vf.rbd(["m1"], "p", "img"))],
                        storage=vf.storage(csinodes=mig))


def test_refusals():
    nodes = [ef.node("a")]
    wffc = {"metadata": {"name": "late"}, "provisioner": "x", "volumeBindingMode": "WaitForFirstConsumer"}
    claims = [vf.pvc(f"u{i}", bound=False, sc="late") for i in range(abi.KSS_MAX_WFFC + 1)]
    st = vf.storage(pvcs=claims, scs=[wffc])
    compile_cluster(nodes, [], [vf.vpod("p", *[vf.claim(f"u{i}") for i in range(abi.KSS_MAX_WFFC)])], storage=st)
    with pytest.raises(Unsupported, match="WaitForFirstConsumer"):  # one delayed claim too many
        compile_cluster(nodes, [], [vf.vpod("p", *[vf.claim(f"u{i}") for i in range(abi.KSS_MAX_WFFC + 1)])],
                        storage=st)
    twice = vf.storage(pvs=[vf.wpv("x", 1, "late", claim_ref="u0"), vf.wpv("y", 1, "late", claim_ref="u0")],
                       pvcs=claims, scs=[wffc])
    with pytest.raises(Unsupported, match="pre-bound"):
        compile_cluster(nodes, [], [vf.vpod("p", vf.claim("u0"))], storage=twice)
    mig = [{"metadata": {"name": "a", "annotations": {"storage.alpha.kubernetes.io/migrated-plugins":
                                                      "kubernetes.io/aws-ebs"}}, "spec": {"drivers": []}}]
    with pytest.raises(Unsupported, match="migrated"):
        compile_cluster(nodes, [], [vf.vpod("p", vf.ebs("v"))], storage=vf.storage(csinodes=mig))


def test_long_csi_driver_key():
    """GetCSIAttachLimitKey: names reaching 63 characters keep 23 characters and 16 hex of sha1."""
    from kss.volumes import csi_attach_limit_key
    d = "a-very-long-csi-driver-name.storage.example.com"
    k = csi_attach_limit_key(d)
    assert k == k8s_volumes.csi_attach_limit_key(d)
    assert k.startswith("attachable-volumes-csi-a-very-long-csi-driver") and len(k) == 23 + 23 + 16
    assert csi_attach_limit_key("ebs.csi.aws.com") == "attachable-volumes-csi-ebs.csi.aws.com"


@pytest.mark.parametrize("seed", range(12))
def test_oracles_agree_on_random_volume_clusters(seed):
    """The object-level restatement (objects, NodeInfo.Pods re-read per filter call) and the
    C oracle over the compiled volume rows agree on every per-node verdict, score and
    choice, pod after pod (each AssumePod visible to the next pod)."""
    import volume_fuzz
    nodes, bound, pods, st = volume_fuzz.make(seed)
    cc, cp, chosen, res = run_both(nodes, bound, pods, storage=st)
    fails = {int(f) for f in res.fail_plugin.ravel()}
    assert cp.n_vols > 0 and len(cc.vol_rows) > 0
    if seed == 0:  # the generator reaches the volume plugins' failures
        assert fails & {abi.KSS_F_VOLUME_RESTRICTIONS, abi.KSS_F_VOLUME_BINDING, abi.KSS_F_VOLUME_ZONE}


def test_snapshot_round_trip_with_volumes():
    """ResourcesForSnap (snapshot.go:32-41) carries pvs / pvcs / storageClasses: written, read
    back and compiled, it schedules like the objects it came from."""
    from kss import snapshot
    import volume_fuzz
    nodes, bound, pods, st = volume_fuzz.make(5)
    snap = snapshot.Snapshot(nodes=nodes, bound=bound, pending=pods, namespaces={"default": {}},
                             pvs=st["pvs"], pvcs=st["pvcs"], storage_classes=st["storage_classes"])
    back = snapshot.read_snapshot(json.dumps(snapshot.write_snapshot(snap)))
    st2 = back.storage()
    assert st2["pvs"] == st["pvs"] and st2["pvcs"] == st["pvcs"]
    run_both(back.nodes, back.bound, back.pending, storage=st2)


def test_plan_names_volumes():
    """kss_plan_podset (host only): volume programs keep a batch on k_schedule, and say so."""
    from kss import native
    nodes, bound, pods, _, st = vf.fx_volume_zone()
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    plan = native.plan_podset(cc.as_struct(), cp.as_struct())
    assert plan["kernel"] == "k_schedule" and "volumes" in plan["reason"], plan


def test_wffc_assume_cache_final_state():
    """Both oracles end the WaitForFirstConsumer fixture with the hand-derived assume cache: each
    claim's static binding (pv_owner) and the provisioned claim's selected node (claim_node)."""
    import oracle_c
    nodes, bound, pods, _, st = vf.fx_wait_for_first_consumer()
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    _, _, fs = oracle_c.schedule(abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes,
                                 record=False, n_classes=len(cc.classes), n_terms=len(cc.terms))
    claim_of = {i + 1: name for i, (_, name) in enumerate(cc.wclaims)}
    got = {claim_of[o]: cc.pvs[v] for v, o in enumerate(fs["pv_owner"]) if o}
    assert got == vf.WFFC_FINAL_BINDINGS
    sel = {cc.wclaims[c][1]: cc.node_names[n] for c, n in enumerate(fs["claim_node"]) if n >= 0}
    assert sel == vf.WFFC_FINAL_SELECTED
    o = _oracle(nodes, bound, st)
    for p in pods:
        o.schedule_one(p)
    assert {ref[1]: pv for pv, ref in o.storage.pv_ref.items()} == vf.WFFC_FINAL_BINDINGS
    assert o.storage.selected == {("default", k): v for k, v in vf.WFFC_FINAL_SELECTED.items()}


@pytest.mark.parametrize("seed", range(16))
def test_oracles_agree_on_random_wffc_clusters(seed):
    """WaitForFirstConsumer claims on random clusters (tests/volume_fuzz.py wffc=True): the object
    oracle's FindPodVolumes / AssumePodVolumes and the C oracle over the compiled candidate lists
    agree pod after pod, and on the assume cache they leave."""
    import oracle_c
    import volume_fuzz
    nodes, bound, pods, st = volume_fuzz.make(100 + seed, wffc=True)
    cc, cp, chosen, res = run_both(nodes, bound, pods, storage=st)
    assert cc.wclaims and cp.n_vols > 0
    _, _, fs = oracle_c.schedule(abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes,
                                 record=False, n_classes=len(cc.classes), n_terms=len(cc.terms))
    o = _oracle(nodes, bound, st)
    for p in pods:
        o.schedule_one(p)
    claim_of = {i + 1: name for i, (_, name) in enumerate(cc.wclaims)}
    got = {cc.pvs[v]: claim_of[int(x)] for v, x in enumerate(fs["pv_owner"]) if x}
    want = {pv: ref[1] for pv, ref in o.storage.pv_ref.items() if pv in set(cc.pvs)}
    assert got == want
    sel = {cc.wclaims[c][1]: int(n) for c, n in enumerate(fs["claim_node"]) if n != -1}
    want_sel = {k[1]: (cc.node_names.index(v) if v in cc.node_names else -2) for k, v in o.storage.selected.items()
                if k in set(cc.wclaims)}
    assert sel == want_sel


def test_random_wffc_clusters_reach_every_branch():
    """Across the seeds the WaitForFirstConsumer fuzz reaches bind conflicts, the combined node +
    bind conflict reason, static bindings and provisioning (both assume-cache columns move)."""
    import oracle_c
    import volume_fuzz
    details, moved_pv, moved_claim = set(), False, False
    for seed in range(16):
        nodes, bound, pods, st = volume_fuzz.make(100 + seed, wffc=True)
        cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
        ch, res, fs = oracle_c.schedule(abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes,
                                        record=True, n_classes=len(cc.classes), n_terms=len(cc.terms))
        vb = res.fail_plugin == abi.KSS_F_VOLUME_BINDING
        details |= {int(d) for d in res.fail_detail[vb]}
        moved_pv |= bool((fs["pv_owner"] != cc.arrays["pv_owner"][:len(cc.pvs)]).any())
        moved_claim |= bool((fs["claim_node"] != cc.arrays["claim_node"][:len(cc.wclaims)]).any())
    assert {abi.KSS_VB_BIND_CONFLICT} <= details, details
    assert moved_pv and moved_claim


# ---------------------------------------------------------------------------------------------
# Unreserve's RevertAssumedPodVolumes: the assume cache after a rollback that more scheduling follows
import volume_rollback as vr

ROLLBACK_SEEDS = (100, 109, 111, 113, 116, 121)
ROLLBACK_ORDERS = {"immediate": lambda n: vr.ops_immediate(n, 3), "lifo": lambda n: vr.ops_lifo(n, 3, 5)}


def _c_steps_equal_expect(cc, res, fs, chosen, steps, expect, where):
    from crosscheck import FILTER_CODE
    for k, (op, exp) in enumerate(zip(steps, expect)):
        if op >= 0:
            assert (cc.node_names[chosen[k]] if chosen[k] >= 0 else "") == exp["selected"], (where, k)
            want = [0 if exp["filter"][n] is None else FILTER_CODE[exp["filter"][n][0]] for n in cc.node_names]
            assert [int(f) for f in res.fail_plugin[k, :cc.n_nodes]] == want, (where, k)
        b, s = vr.decode(cc, fs["trace"]["pv_owner"][k], fs["trace"]["claim_node"][k])
        assert {c: pv for pv, c in b.items()} == exp["bound"], (where, k)
        assert s == exp["selected_nodes"], (where, k)


@pytest.mark.parametrize("case", ["provisioned_elsewhere", "rebound_same_pv"])
def test_shared_claim_rollback_matches_hand_derived(case):
    """fx_wffc_shared_claim_rollback on both oracles, step by step: verdicts, selected nodes and
    the assume cache after every step equal the literals -- the object oracle's recorded
    podVolumes, the C oracle's rollback() of the recorded picks, and the C oracle's skip_commit
    (a commit rolled back at once), which must leave the cache as commit then rollback do."""
    nodes, bound, pods, steps, expect, st = vf.fx_wffc_shared_claim_rollback()[case]
    got = vr.run_object_oracle(nodes, bound, pods, st, steps)
    for k, (g, exp) in enumerate(zip(got, expect)):
        if g["res"] is not None:
            ef.check_expect(g["ann"], exp, where=(case, k))
        assert {c: pv for pv, c in g["bound"].items()} == exp["bound"], (case, k)
        assert g["selected"] == exp["selected_nodes"], (case, k)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    chosen, res, fs = vr.run_c_oracle(cc, cp, steps)
    assert [int(c) for c in chosen] == [g["chosen"] for g in got]
    _c_steps_equal_expect(cc, res, fs, chosen, steps, expect, case)
    # the same sequence as a skipped commit: steps 1 and 2 become one evaluation, not assumed
    skip = np.zeros(cp.n, np.uint8)
    skip[1] = 1
    chosen, res, fs = vr.run_c_oracle(cc, cp, [0, 1, 2], skip_commit=skip)
    _c_steps_equal_expect(cc, res, fs, chosen, [0, 1, 2], [expect[0], dict(expect[1], **{
        "bound": expect[2]["bound"], "selected_nodes": expect[2]["selected_nodes"]}), expect[3]], case + " skip")


def test_empty_topology_terms_detail_and_cache():
    """fx_allowed_topologies_empty_terms: the C oracle's VolumeBinding detail per node (the bind
    conflict wherever no usable term admits the node) and both oracles' final assume cache."""
    nodes, bound, pods, expect, st = vf.fx_allowed_topologies_empty_terms()
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    chosen, res, fs = vr.run_c_oracle(cc, cp, list(range(cp.n)))
    for j, exp in enumerate(expect):
        for i, n in enumerate(cc.node_names):
            if exp["vb"][n] == "bind":
                assert (int(res.fail_plugin[j, i]), int(res.fail_detail[j, i])) == \
                       (abi.KSS_F_VOLUME_BINDING, abi.KSS_VB_BIND_CONFLICT), (j, n)
            else:
                assert int(res.fail_plugin[j, i]) == 0, (j, n)
    assert vr.decode(cc, fs["pv_owner"], fs["claim_node"]) == ({}, vf.EMPTY_TERMS_FINAL_SELECTED)
    got = vr.run_object_oracle(nodes, bound, pods, st, list(range(len(pods))))
    assert (got[-1]["bound"], got[-1]["selected"]) == ({}, vf.EMPTY_TERMS_FINAL_SELECTED)


def _rollback_case(seed, order):
    import volume_fuzz
    nodes, bound, pods, st = volume_fuzz.make(seed, wffc=True)
    return nodes, bound, pods, st, ROLLBACK_ORDERS[order](len(pods))


@pytest.mark.parametrize("order", sorted(ROLLBACK_ORDERS))
@pytest.mark.parametrize("seed", ROLLBACK_SEEDS)
def test_oracles_agree_on_rollback_programs(seed, order):
    """The rollback fuzz: random WaitForFirstConsumer clusters (pods sharing w-* claims) under a
    rollback pattern -- immediate (every third pod's commit undone at once) and LIFO (after every
    five pods the last three undone, newest first).  The object oracle (assume, forget, go on)
    and the C oracle (commit(), rollback() of the recorded picks) agree on every chosen node,
    every per-node verdict and on the assume cache after every step."""
    from crosscheck import FILTER_CODE
    nodes, bound, pods, st, ops = _rollback_case(seed, order)
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    got = vr.run_object_oracle(nodes, bound, pods, st, ops)
    chosen, res, fs = vr.run_c_oracle(cc, cp, ops)
    for k, (op, g) in enumerate(zip(ops, got)):
        assert int(chosen[k]) == g["chosen"], (k, op)
        if op >= 0:
            for i in range(cc.n_nodes):
                want = g["res"]["fail"].get(i, "not evaluated")  # (a PreFilter rejection: no node is)
                code = 0 if want is None else FILTER_CODE.get(want, abi.KSS_F_NOT_EVALUATED)
                assert int(res.fail_plugin[k, i]) == code, (k, op, i)
        assert vr.decode(cc, fs["trace"]["pv_owner"][k], fs["trace"]["claim_node"][k]) == \
               vr.restrict(cc, g["bound"], g["selected"]), (k, op)
    if order == "immediate":  # the same program as skipped commits (kss_oracle_schedule_wm's skip_commit)
        n = len(pods)
        ch2, _, fs2 = vr.run_c_oracle(cc, cp, list(range(n)), record="meta", skip_commit=[j % 3 == 2 for j in range(n)])
        at = [k for k, op in enumerate(ops) if op >= 0]
        for j in range(n):
            k = at[j] + (1 if j % 3 == 2 else 0)  # the step that leaves pod j's state: its rollback, if any
            assert int(ch2[j]) == int(chosen[at[j]]), j
            for col in ("pv_owner", "claim_node", "vol_count", "vol_attached"):
                np.testing.assert_array_equal(fs2["trace"][col][j], fs["trace"][col][k], err_msg=f"pod {j} {col}")


def test_rollback_programs_reach_the_shared_claim_cases():
    """Counted on the object oracle alone, across the seeds and both orders: rollbacks of a pod
    that provisioned a claim another live pod had statically bound (the claim-keyed revert frees
    that PV), of a pod that re-bound a PV another live pod had assumed (a skipped commit keeps
    it), and of a pod holding two delayed claims."""
    counts = dict(provisioned_others_binding=0, rebound_others_pv=0, two_claims=0, rollbacks=0)

    def on_rollback(o, pod):
        mine = o.storage.pod_volumes.get(o._key(pod))
        if mine is None:
            return
        counts["rollbacks"] += 1
        others = [v for k, v in o.storage.pod_volumes.items() if k != o._key(pod)]
        theirs = [b for v in others for b in v[0]]
        counts["provisioned_others_binding"] += any(c == key for key in mine[1] for c, _ in theirs)
        counts["rebound_others_pv"] += any(b in theirs for b in mine[0])
        counts["two_claims"] += len(mine[0]) + len(mine[1]) >= 2
    for seed in ROLLBACK_SEEDS:
        for order in sorted(ROLLBACK_ORDERS):
            nodes, bound, pods, st, ops = _rollback_case(seed, order)
            vr.run_object_oracle(nodes, bound, pods, st, ops, on_rollback=on_rollback)
    print(counts)
    assert counts["provisioned_others_binding"] >= 1, counts
    assert counts["rebound_others_pv"] >= 1, counts
    assert counts["two_claims"] >= 1, counts


def test_out_of_order_rollback_pins_the_recorded_form():
    """The ordering limit of the device's rollback, pinned on the reference.  kss_rollback finds the
    pod's picks by evaluating FindPodVolumes again, which is exact when the commit being undone is
    the newest live one (immediate and LIFO rollbacks); upstream keeps podVolumes from Reserve, so
    a binding cycle may fail after later pods were assumed.  rebound_same_pv with one more step:
    pod-b assumed pv-x for c-c (step 0), pod-a's Unreserve freed it (2), pod-d assumed it for c-e
    (3); now pod-b's Unreserve (out of order: pod-d is newer and live) restores pv-x -- in its
    recorded StaticBindings -- to the snapshot and wipes pod-d's assumption.  Evaluating again
    would find no PV for c-c (pv-x is c-e's), take c-c for provisioned and leave {c-e: pv-x}."""
    nodes, bound, pods, steps, _, st = vf.fx_wffc_shared_claim_rollback()["rebound_same_pv"]
    steps = steps + [-1]
    got = vr.run_object_oracle(nodes, bound, pods, st, steps)
    assert got[3]["bound"] == {"pv-x": "c-e"}
    assert (got[4]["chosen"], got[4]["bound"], got[4]["selected"]) == (0, {}, {})
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    _, _, fs = vr.run_c_oracle(cc, cp, steps, record=False)
    assert vr.decode(cc, fs["pv_owner"], fs["claim_node"]) == ({}, {})
