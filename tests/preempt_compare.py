"""One comparison form for a DefaultPreemption PostFilter dry run (test infrastructure).

A dry run from the object-level restatement (oracle/k8s_preemption.preempt), from the C
restatement (oracle_c.postfilter) or from the device (native.Context.postfilter_pod) becomes

  (status, node, victims in eviction order, n_potential, n_candidates,
   n_victims, highest_priority, sum_priority, earliest_start)

with names for the node and the victims.  The last four fields describe the nominated node
(pickOneNodeForPreemption's criteria), so they are None unless the status is "nominated"; the
two counts are None for "schedulable" (PostFilter never runs for such a pod: the restatements
report 0 and the device what its filter pass saw).  For the object-level restatement the
criteria come from candidates[nominated], the victims in reprieve order:
  highest_priority  priority of the first victim (the most important one),
  sum_priority      sum(priority + 2^31)                    (pickOneNodeForPreemption, step 3),
  earliest_start    util.GetEarliestPodStartTime: the earliest start among the
                    highest-priority victims, KSS_START_UNSET when none of them has one.
"""
import copy

import k8s_oracle as ko
import k8s_preemption as kp
from kss import abi

STATUS = {abi.KSS_PREEMPT_NOMINATED: "nominated", abi.KSS_PREEMPT_NO_CANDIDATE: "no_candidate",
          abi.KSS_PREEMPT_NOT_ELIGIBLE: "not_eligible", abi.KSS_PREEMPT_SCHEDULABLE: "schedulable"}


def _shape(status, node, victims, n_pot, n_cand, n_victims, hp, sp, st):
    if status == "schedulable":
        n_pot = n_cand = None
    if status != "nominated":
        return (status, None, [], n_pot, n_cand, None, None, None, None)
    return (status, node, list(victims), n_pot, n_cand, n_victims, hp, sp, st)


def criteria(victim_infos):
    """(highest_priority, sum_priority, earliest_start) of a candidate's victims (PodInfos in
    reprieve order), as pickOneNodeForPreemption reads them."""
    prios = [ko.pod_priority(v.pod) for v in victim_infos]
    top = max(prios)
    starts = [kp.pod_start_ns(v.pod) for v, p in zip(victim_infos, prios) if p == top]
    starts = [s for s in starts if s is not None]
    return prios[0], sum(p + 2**31 for p in prios), (min(starts) if starts else abi.KSS_START_UNSET)


def from_python(o, pre):
    """The full tuple of kp.preempt's result on Oracle o."""
    if pre["status"] != "nominated":
        return _shape(pre["status"], None, [], pre["n_potential"], pre["n_candidates"], None, None, None, None)
    vs = pre["candidates"][pre["nominated"]]
    hp, sp, st = criteria(vs)
    assert hp == max(ko.pod_priority(v.pod) for v in vs)  # reprieve order starts at the most important
    return _shape("nominated", ko._name(o.nodes[pre["nominated"]]), [v[1] for v in pre["victims"]],
                  pre["n_potential"], pre["n_candidates"], len(vs), hp, sp, st)


def victim_namer(cc, cp=None):
    """Bound-table ids to pod names: the loaded rows by index, pods committed from podset cp as -1 - index."""
    def name(v):
        return cc.bound_names[v][1] if v >= 0 else cp.names[-1 - v][1]
    return name


def from_native(r, cc, cp=None):
    """The full tuple of an oracle_c.postfilter / Context.postfilter_pod dict; the victims list must
    be complete (victims_cap at least n_victims)."""
    status = STATUS[r["status"]]
    if status == "nominated":
        assert r["n_victims"] == len(r["victims"]), (r["n_victims"], len(r["victims"]))
    name = victim_namer(cc, cp)
    node = cc.node_names[r["nominated"]] if r["nominated"] >= 0 else None
    return _shape(status, node, [name(v) for v in r["victims"]], r["n_potential"], r["n_candidates"],
                  r["n_victims"], r["highest_priority"], r["sum_priority"], r["earliest_start"])


def expected(status, node, victims, n_pot, n_cand, bound_by_name):
    """The full tuple of a hand-derived expectation (status, node, victims, n_potential,
    n_candidates): the criteria follow from the named victims' priorities and start times."""
    if status != "nominated":
        return _shape(status, None, [], n_pot, n_cand, None, None, None, None)

    class _V:  # what criteria() reads of a PodInfo
        def __init__(self, pod):
            self.pod = pod
    hp, sp, st = criteria([_V(bound_by_name[v]) for v in victims])
    return _shape(status, node, victims, n_pot, n_cand, len(victims), hp, sp, st)


def same(got, want):
    """got == want, except that PostFilter never runs for a pod the cycle can place: the C
    restatement and the device refuse a preemptionPolicy Never pod before they look."""
    if want[0] == "schedulable":
        return got[0] in ("schedulable", "not_eligible")
    return got == want


def py_dry_runs(nodes, bound, pods, noms=()):
    """The object-level restatement's dry run of every pod on the unchanged snapshot, with
    noms = [(pod name, node name)] in the nominator: (oracle, [full tuple], [(cycle result, preempt result)])."""
    o = ko.Oracle(nodes, bound)
    by_name = {ko._name(p): p for p in pods}
    for pn, nn in noms:
        o.nominate(by_name[pn], o.by_name[nn])
    out, raw = [], []
    for p in pods:
        r = o.schedule_one(p, commit=False)
        pre = kp.preempt(o, p, r)
        out.append(from_python(o, pre))
        raw.append((r, pre))
    return o, out, raw


def index_noms(cc, cp, noms):
    """[(pod name, node name)] as [(podset index, device node index)]."""
    pod_idx = {nm[1]: j for j, nm in enumerate(cp.names)}
    node_idx = {n: i for i, n in enumerate(cc.node_names)}
    return [(pod_idx[pn], node_idx[nn]) for pn, nn in noms]


def c_dry_runs(compiled, threads=1, noms=(), only=None):
    """The C restatement's dry run of every pod (or the indices in `only`) of a compiled cluster
    (compile_cluster's triple) on the unchanged snapshot: [full tuple]."""
    import oracle_c
    cc, cp, _ = compiled
    cl, ps, bs = cc.as_struct(), cp.as_struct(), cc.as_boundset()
    nn = index_noms(cc, cp, noms)
    return [from_native(oracle_c.postfilter(abi.default_profile(), cl, ps, j, bs, threads=threads, nominations=nn), cc, cp)
            for j in (range(cp.n) if only is None else only)]


def potential_nodes(o, res):
    """nodesWherePreemptionMightHelp: the indices preempt() dry-runs."""
    out = []
    for i, ni in enumerate(o.infos):
        rec = res["filter"].get(ko._name(ni.node))
        if rec is not None:
            plugin = next(reversed(rec))
            if kp._unresolvable(plugin, rec[plugin]):
                continue
        out.append(i)
    return out


def pinned(pod, node_name, tag):
    """A clone of `pod` that only node_name admits (kubernetes.io/hostname nodeSelector)."""
    q = copy.deepcopy(pod)
    q["metadata"]["name"] = "%s@%s" % (ko._name(pod), tag)
    q["spec"].setdefault("nodeSelector", {})["kubernetes.io/hostname"] = node_name
    return q


def pinned_probes(nodes, bound, pods, noms=()):
    """[(clone, expected (status, node, victims, n_victims, highest, sum, start))] for every
    preemptor without a spread constraint and every node its PostFilter dry-runs: the node's
    entry in the unpinned run's candidates, or no_candidate when it has none.  (A spread
    preemptor is left out: its nodeSelector decides which nodes its constraints count.)"""
    o, full, raw = py_dry_runs(nodes, bound, pods, noms)
    out = []
    for p, t, (r, pre) in zip(pods, full, raw):
        if t[0] not in ("nominated", "no_candidate") or r["status"] == "prefilter":
            continue
        if p["spec"].get("topologySpreadConstraints"):
            continue
        for i in potential_nodes(o, r):
            name = ko._name(o.nodes[i])
            vs = pre["candidates"].get(i)
            if vs:
                want = ("nominated", name, [ko._name(v.pod) for v in vs], len(vs)) + criteria(vs)
            else:
                want = ("no_candidate", None, [], None, None, None, None)
            out.append((pinned(p, name, "%d" % i), want))
    return out


def probe_view(t):
    """The fields of a full tuple a pinned probe compares (the counts describe the pinned run)."""
    return t[:3] + t[5:]
