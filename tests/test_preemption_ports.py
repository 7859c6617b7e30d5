"""DefaultPreemption with host ports on the CPU: the hand-derived cases of
tests/preempt_port_fixtures.py against the object-level restatement (oracle/k8s_preemption.py),
and the conditions that keep a device parity test over the seeded clusters from passing
vacuously, checked on the oracle alone for every (seed, shape) the fixture names."""
import pytest

import k8s_oracle as ko
import k8s_preemption as kp
import preempt_port_fixtures as ppf
from kss import abi
from kss.compile import compile_cluster, host_ports, ports_conflict


def _dry_run(o, pods, case):
    by_name = {p["metadata"]["name"]: p for p in pods}
    index = {ko._name(n): i for i, n in enumerate(o.nodes)}
    for q, n in case["noms"]:
        o.nominate(by_name[q], index[n])
    p = by_name[case["pod"]]
    r = o.schedule_one(p, commit=False)
    pre = kp.preempt(o, p, r)
    for q, _ in case["noms"]:
        o.clear_nomination(by_name[q])
    return pre


def test_oracle_matches_hand_derived():
    nodes, bound, pods, cases = ppf.fixture()
    assert len(nodes) == 14
    o = ko.Oracle(nodes, bound)
    for case in cases:
        pre = _dry_run(o, pods, case)
        node = ko._name(o.nodes[pre["nominated"]]) if pre["nominated"] is not None else None
        assert (pre["status"], node, [v[1] for v in pre["victims"]]) == case["expect"], case["name"]
        for k in ("n_potential", "n_candidates"):
            if case[k] is not None:
                assert pre[k] == case[k], (case["name"], k)


def test_bit63_fixture_shape():
    """The dictionary has exactly 64 entries, the holder's is the last, and the preemptor
    conflicts with that entry and its own only; the oracle evicts the holder."""
    nodes, bound, pods, holder = ppf.bit63()
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    assert len(cc.ports) == 64 == abi.KSS_MAX_PORTS
    assert cc.ports[63] == holder
    own = cc.port_index[("0.0.0.0", "TCP", 60000)]
    assert int(cp.pods[0]["port_conflict"]) == (1 << 63) | (1 << own)
    row = [i for i, (_, name) in enumerate(cc.bound_names) if name == "x-hold"][0]
    assert int(cc.bound["ports"][row]) == 1 << 63
    assert int(cc.arrays["port_used"][cc.node_names.index("x")]) == (1 << 64) - 1 - (1 << own)
    o = ko.Oracle(nodes, bound)
    pre = kp.preempt(o, pods[0], o.schedule_one(pods[0], commit=False))
    assert (pre["status"], ko._name(o.nodes[pre["nominated"]]), [v[1] for v in pre["victims"]]) == \
        ("nominated", "x", ["x-hold"])


def port_nominations(bound, pods, results):
    """Of (pod, PostFilter result or None) pairs: the nominated host-port preemptors with a victim
    on the nominated node that holds an entry conflicting with one they want."""
    by_name = {b["metadata"]["name"]: b for b in bound}
    n = 0
    for p, pre in results:
        if pre is None or pre["status"] != "nominated":
            continue
        held = [e for _, v in pre["victims"] if v in by_name for e in host_ports(by_name[v])]
        if any(ports_conflict(w, e) for w in host_ports(p) for e in held):
            n += 1
    return n


@pytest.mark.parametrize("seed,n_nodes,n_pods", ppf.SEEDED)
def test_seeded_clusters_reach_port_evictions(seed, n_nodes, n_pods):
    assert n_nodes <= 130 and n_pods <= 60
    nodes, bound, pods = ppf.saturated_ports(seed, n_nodes, n_pods)
    cc, _, _ = compile_cluster(nodes, bound, pods)
    assert 0 < len(cc.ports) <= abi.KSS_MAX_PORTS
    _, out = kp.schedule_with_preemption(nodes, bound, pods)
    res = [(p, pre) for p, (_, pre, _) in zip(pods, out)]
    assert port_nominations(bound, pods, res) >= 3
    assert any(pre is not None and pre["status"] in ("no_candidate", "not_eligible") for _, pre in res)


def test_sequence_and_batch_clusters_reach_port_evictions():
    """The same conditions for the cluster of the nomination loop (on its own sequence) and of the
    batch test."""
    seed, n_nodes, n_pods = ppf.SEQUENCE
    nodes, bound, pods = ppf.saturated_ports(seed, n_nodes, n_pods)
    _, out = kp.schedule_with_nominations(nodes, bound, pods)
    assert port_nominations(bound, pods, [(pods[j], pre) for j, _, pre in out]) >= 3
    seed, n_nodes, n_pods, first = ppf.BATCH
    nodes, bound, pods = ppf.saturated_ports(seed, n_nodes, n_pods)
    _, out = kp.schedule_with_preemption(nodes, bound, pods)
    assert port_nominations(bound, pods, [(p, pre) for p, (_, pre, _) in list(zip(pods, out))[first:]]) >= 1


def test_snapshot_is_conflict_free_and_stripped_copy_has_no_ports():
    nodes, bound, pods = ppf.saturated_ports(3, 40, 30)
    held = {}
    for b in bound:
        mine = held.setdefault(b["spec"]["nodeName"], [])
        es = ppf.entries(b)
        assert not any(ppf.conflict(e, x) for e in es for x in mine)
        mine.extend(es)
    assert sum(1 for b in bound if ppf.entries(b)) > len(bound) // 3
    assert sum(1 for p in pods if ppf.entries(p)) > len(pods) // 3
    assert not any(ppf.entries(p) for p in ppf.strip_ports(bound + pods))
    assert any(ppf.entries(p) for p in pods)  # the originals are untouched
