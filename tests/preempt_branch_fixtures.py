"""DefaultPreemption branch fixtures (test infrastructure): hand-derived cases for the branches
of SelectVictimsOnNode / pickOneNodeForPreemption the seeded `saturated` clusters never reach,
constructed clusters for the device's reductions, and a richer seeded recipe.

Every expectation is (status, node, victims in eviction order, n_potential, n_candidates) and
follows by hand from k8s.io/kubernetes v1.26.2:
  preemption.go           nodesWherePreemptionMightHelp, DryRunPreemption, pickOneNodeForPreemption
  default_preemption.go   SelectVictimsOnNode (remove every lower-priority pod, filter, reprieve
                          in MoreImportantPod order: priority descending, start ascending)
  noderesources/fit.go    fitsRequest
  podtopologyspread/filtering.go   calPreFilterState, updateWithPod, Filter
  interpodaffinity/filtering.go    updateWithPod, satisfyPodAffinity, satisfyExistingPodsAntiAffinity

branch_fixture() -- one cluster; each pending pod selects one node group (nodeSelector group=G),
so the other groups' nodes fail NodeAffinity (UnschedulableAndUnresolvable: never potential).
Nodes have 2 CPU, 8Gi, 110 pods unless stated.  Pending pods have priority 10, "low" pods 1,
"high" pods 100, unless stated.  T0 < T10 are start times.

 Required pod affinity (hostname unless stated), the node's cycle status is NodeResourcesFit
 (Fit runs before InterPodAffinity, so a full node's first failure is Fit: Unschedulable).
 Affinity labels are unique per case: affinityCounts are cluster-wide.
  aff-a  aa1: low filler 1900m + low app=afa 100m; aa2: high app=afa 2000m.  pa (1000m, term
         app=afa, no such label itself).  aa1: both removed, Fit passes; affinityCounts still
         holds (hostname, aa2), aa1's own pair is 0 -> podsExist false, len(affinityCounts) != 0
         -> fails: no candidate.  aa2: nothing of lower priority.  potential 2 (both Fit).
  aff-b  ab1: low filler 1500m (T0), low app=afb 500m (T10).  pb (1000m, labelled app=afb, term
         app=afb).  Both removed: affinityCounts empty and the pod matches its own terms -> the
         "first pod of its group" exception passes.  Reprieve filler: 2500m > 2000m -> victim.
         Reprieve the matching pod: 1500m fits and its pair is 1 -> reprieved.  [ab1-fill].
  aff-c  ac1: low app=afc 2000m.  pc as pb (app=afc).  Removed -> exception passes; reprieving
         it fails Fit -> the matching pod itself is the victim.
  aff-d  ad1 as ab1 (app=afd); pd has the term but not the label: after the removals
         affinityCounts is empty but podMatchesAllAffinityTerms is false -> no candidate.
  aff-e  ae1 (no "rack" label): low 2000m.  pe (labelled app=afe, term app=afe on key "rack").
         Cycle status Fit -> potential.  Dry run: Fit passes, satisfyPodAffinity returns false at
         once for a node without the term's topology key -> never a candidate.  1 / 0.
  aff-f  af1, af2 in zone zf.  af1: low 2000m; af2: high app=aff 2000m.  pf (1000m, term app=aff
         on the zone key).  af1: removal -> Fit passes, the pair (zone, zf) is 1 through af2 and
         no removal touches it -> passes; reprieving the filler fails Fit -> [af1-fill].
         af2 is potential (Fit) with nothing to evict: 2 / 1.

 Resources (cycle status Fit with one reason each)
  mem    m1: low 100m/6Gi (T0), low 100m/1Gi (T10).  pm 100m/4Gi: "Insufficient memory" only.
         Reprieve big: 10Gi > 8Gi -> victim; small: 5Gi fits -> reprieved.  [m1-big].
  ext    x1 (example.com/gpu: 2): low gpu 1 (T0), low gpu 1 (T10), 100m each.  px 100m + gpu 1:
         "Insufficient example.com/gpu" only.  Reprieve the first: 2 <= 2; the second: 3 > 2 ->
         [x1-g2].
  ext0   x2 (example.com/gpu: 1, over-committed): high gpu 2 / 500m, low 1500m.  px0 1000m, no
         gpu request: fitsRequest skips a scalar the pod does not request, so the column at
         2 > 1 is ignored; CPU decides: [x2-c].
  lim    l1 (pods: 2): two low pods without requests (T0, T10).  pl has no requests at all:
         "Too many pods" only (fitsRequest returns before the resources for an all-zero
         request).  Reprieve the first: 1 + 1 <= 2; the second: 2 + 1 > 2 -> [l1-b].

 Spread (DoNotSchedule; the preemptor matches its own selectors: selfMatch 1)
  two    zone maxSkew 3 and hostname maxSkew 1, selector app=sp1.  s1a (zone zs1): low app=sp1
         x2 (T0, T10); s1c (zs1): high app=sp1 2000m; s1b (zs2): high 2000m, no label.
         Pairs: zone zs1 3, zs2 0; host s1a 2, s1c 1, s1b 0.  Cycle: s1a zone 3+1-0 = 4 > 3 ->
         PodTopologySpread; s1b, s1c Fit.  Dry run s1a: removal -> zone 1+1-0 <= 3, host
         0+1-0 <= 1.  Reprieve y1: zone 2+1-0 = 3 <= 3 passes, host 1+1-0 = 2 > 1 -> victim
         (the hostname constraint decides); y2 the same.  [s1a-y1, s1a-y2], 3 / 1.
  same   two hostname constraints, maxSkew 1, selectors app=sk and tier=t.  s2a: low v
         (app=sk, tier=t), high w (tier=t); s2b: high 2000m.  calPreFilterState keeps, per node,
         the count of the last constraint on the key: (host, s2a) = 2.  Cycle: 2+1-0 > 1.
         updateWithPod moves the shared pair once per matching constraint: removing v gives
         2 - 2 = 0 -> 0+1-0 <= 1 passes (moving it by 1 would leave 1+1-0 = 2 > 1: no candidate).
         Reprieve v: back to 2 -> victim.  [s2a-v], 2 / 1.
  atmin  hostname, app=s3, maxSkew 1.  s3a: low app=s3 x2 (100m, T0 / T10) + low filler 1800m
         (T10, listed last); s3b: 3 high app=s3, full; s3c: 5 high app=s3, full.  s3a is the
         global minimum (2).  Cycle: 2+1-2 <= 1 passes spread, Fit fails (ps3 1000m).  Dry run:
         removal -> pair 0, minimum min(0, 3) = 0.  Reprieve y1: 1+1-1, y2: 2+1-2 -> both stay;
         filler: 3000m -> victim.  [s3a-fill].  (Without nominees the node's own pair never
         exceeds its original count, so the minimum over the OTHER pairs -- the second
         criticalPaths entry -- cannot show here; min_rise_fixture() adds the nominee that
         makes it show.)
  above  hostname, app=s4, maxSkew 1.  s4a: low app=s4 x3 (T0, T10, T20); s4b: one high app=s4,
         full.  Minimum 1 (s4b).  Cycle: s4a 3+1-1 > 1.  Removal: 0+1-0.  Reprieve y1:
         1+1-1 = 1 stays; y2: 2+1-1 = 2 -> victim; y3 likewise.  [s4a-y2, s4a-y3], 2 / 1.

 Existing pods' anti-affinity (hostname)
  anti2  e1: low guard with two terms (app=web2; tier=front).  pe1 carries both labels:
         existingAntiAffinityCounts (hostname, e1) = 2.  Removing the guard moves it by 2 to 0
         (by 1 would leave 1 > 0: no candidate); reprieving it fails -> [e1-guard].
  antih  e2: HIGH guard (term app=web3) + low 100m.  pe2 (app=web3): removing the low pod does
         not clear the count -> the filter after removal fails: no candidate, 1 / 0.

 Ordering
  neg    o1: prio -5 1000m, prio -1 1000m (T0); o2: prio -2 2000m.  po1 (prio 10, 1500m): o1
         evicts both (-1 first), highest victim priority -1; o2 evicts [o2-n2], highest -2;
         -2 < -1 -> o2.  po2 (prio -3, 1000m): on o1 only the prio -5 pod is lower -> removed,
         fits, its reprieve overflows -> [o1-n5]; o2's pod (-2) is not lower: no victims there.
  ties   o3: NodeInfo order u1 (no startTime), s (T10), u2 (no startTime), prio 1, 600m each.
         po3 2000m evicts all.  MoreImportantPod: the started pod first; the two without a
         start time tie and keep NodeInfo order: [o3-s, o3-u1, o3-u2].

 Node lists and PreFilter
  names  n1: low 2000m; n2: prio-5 2000m; n3: low 2000m.  pn (group gn, 1000m) requires
         metadata.name In [n1] or In [n2] (two terms).  NodeAffinity's PreFilterResult is
         {n1, n2}: the cycle filters only those (both Fit), so NodeToStatusMap has no entry for
         any other node of the CLUSTER.
         nodesWherePreemptionMightHelp keeps every node whose status is not
         UnschedulableAndUnresolvable -- a missing entry is not -- so all len(nodes) nodes are
         potential; the dry run's NodeAffinity filter then rejects those outside the list.
         Candidates n1 [n1-l] (highest 1) and n2 [n2-l] (highest 5): n1.  len(nodes) / 2.
  names2 pn2 writes the list as ONE requirement In [n1, n2].  PreFilter still returns {n1, n2}
         (it reads any In values), but the Filter's field selector accepts exactly one value
         (nodeSelectorRequirementsAsFieldSelector), so the term matches no node: n1 and n2 fail
         NodeAffinity (unresolvable) and the rest have no entry: len(nodes) - 2 / 0.
  conflict  metadata.name In [a] and In [b] in one term: NodeAffinity's PreFilter returns
         UnschedulableAndUnresolvable; Preempt finds no potential node: 0 / 0.
"""
import random

import preempt_fixtures as pf
from preempt_fixtures import HOST, ZONE, T0, T10

G = pf.G
T20 = "2024-01-01T00:00:20Z"
GPU = "example.com/gpu"
MIN_PRIO = -2**31


def bnode(name, group=None, cpu="2", mem="8Gi", pods="110", labels=None, alloc=None, host=True):
    lb = dict(labels or {})
    if host:
        lb[HOST] = name
    if group:
        lb[G] = group
    al = {"cpu": cpu, "memory": mem, "pods": pods}
    al.update(alloc or {})
    return {"metadata": {"name": name, "labels": lb}, "spec": {}, "status": {"allocatable": al}}


def bpod(name, prio, req=None, node=None, start=None, group=None, labels=None, **spec):
    """req: a CPU string or a full requests dict."""
    if isinstance(req, str):
        req = {"cpu": req}
    s = {"containers": [{"name": "c", "resources": {"requests": dict(req or {})}}], "priority": prio}
    if node:
        s["nodeName"] = node
    if group:
        s["nodeSelector"] = {G: group}
    s.update(spec)
    out = {"metadata": {"name": name, "namespace": "default", "labels": dict(labels or {})}, "spec": s}
    if start:
        out["status"] = {"startTime": start}
    return out


def _aff(labels, key=HOST):
    return {"podAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"labelSelector": {"matchLabels": dict(labels)}, "topologyKey": key}]}}


def _anti_terms(*label_sets, key=HOST):
    return {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"labelSelector": {"matchLabels": dict(ls)}, "topologyKey": key} for ls in label_sets]}}


def _spread(labels, key, skew=1):
    return {"maxSkew": skew, "topologyKey": key, "whenUnsatisfiable": "DoNotSchedule",
            "labelSelector": {"matchLabels": dict(labels)}}


def _names_affinity(*lists):
    """One term whose matchFields are ANDed."""
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
        {"matchFields": [{"key": "metadata.name", "operator": "In", "values": list(v)} for v in lists]}]}}}


def _names_terms(*names):
    """One term per name (terms are ORed)."""
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
        {"matchFields": [{"key": "metadata.name", "operator": "In", "values": [v]}]} for v in names]}}}


def branch_fixture():
    """(nodes, bound, pods, expect); expect[j] = (status, node, victims, n_potential, n_candidates)."""
    N, B, P, E = [], [], [], []

    def case(nodes, bound, pod, expect):
        N.extend(nodes)
        B.extend(bound)
        P.append(pod)
        E.append(expect)

    # ---- required pod affinity
    case([bnode("aa1", "ga"), bnode("aa2", "ga")],
         [bpod("aa1-fill", 1, "1900m", "aa1", T0), bpod("aa1-m", 1, "100m", "aa1", T10, labels={"app": "afa"}),
          bpod("aa2-m", 100, "2000m", "aa2", T0, labels={"app": "afa"})],
         bpod("pa", 10, "1000m", group="ga", affinity=_aff({"app": "afa"})),
         ("no_candidate", None, [], 2, 0))
    case([bnode("ab1", "gb")],
         [bpod("ab1-fill", 1, "1500m", "ab1", T0), bpod("ab1-m", 1, "500m", "ab1", T10, labels={"app": "afb"})],
         bpod("pb", 10, "1000m", group="gb", labels={"app": "afb"}, affinity=_aff({"app": "afb"})),
         ("nominated", "ab1", ["ab1-fill"], 1, 1))
    case([bnode("ac1", "gc")],
         [bpod("ac1-m", 1, "2000m", "ac1", T0, labels={"app": "afc"})],
         bpod("pc", 10, "1000m", group="gc", labels={"app": "afc"}, affinity=_aff({"app": "afc"})),
         ("nominated", "ac1", ["ac1-m"], 1, 1))
    case([bnode("ad1", "gd")],
         [bpod("ad1-fill", 1, "1500m", "ad1", T0), bpod("ad1-m", 1, "500m", "ad1", T10, labels={"app": "afd"})],
         bpod("pd", 10, "1000m", group="gd", affinity=_aff({"app": "afd"})),
         ("no_candidate", None, [], 1, 0))
    case([bnode("ae1", "ge")],
         [bpod("ae1-fill", 1, "2000m", "ae1", T0)],
         bpod("pe", 10, "1000m", group="ge", labels={"app": "afe"}, affinity=_aff({"app": "afe"}, key="rack")),
         ("no_candidate", None, [], 1, 0))
    case([bnode("af1", "gf", labels={ZONE: "zf"}), bnode("af2", "gf", labels={ZONE: "zf"})],
         [bpod("af1-fill", 1, "2000m", "af1", T0), bpod("af2-m", 100, "2000m", "af2", T0, labels={"app": "aff"})],
         bpod("pf", 10, "1000m", group="gf", affinity=_aff({"app": "aff"}, key=ZONE)),
         ("nominated", "af1", ["af1-fill"], 2, 1))
    # ---- resources
    case([bnode("m1", "gm")],
         [bpod("m1-big", 1, {"cpu": "100m", "memory": "6Gi"}, "m1", T0),
          bpod("m1-small", 1, {"cpu": "100m", "memory": "1Gi"}, "m1", T10)],
         bpod("pm", 10, {"cpu": "100m", "memory": "4Gi"}, group="gm"),
         ("nominated", "m1", ["m1-big"], 1, 1))
    case([bnode("x1", "gx", alloc={GPU: "2"})],
         [bpod("x1-g1", 1, {"cpu": "100m", GPU: "1"}, "x1", T0), bpod("x1-g2", 1, {"cpu": "100m", GPU: "1"}, "x1", T10)],
         bpod("px", 10, {"cpu": "100m", GPU: "1"}, group="gx"),
         ("nominated", "x1", ["x1-g2"], 1, 1))
    case([bnode("x2", "gx0", alloc={GPU: "1"})],
         [bpod("x2-g", 100, {"cpu": "500m", GPU: "2"}, "x2", T0), bpod("x2-c", 1, "1500m", "x2", T0)],
         bpod("px0", 10, "1000m", group="gx0"),
         ("nominated", "x2", ["x2-c"], 1, 1))
    case([bnode("l1", "gl", pods="2")],
         [bpod("l1-a", 1, None, "l1", T0), bpod("l1-b", 1, None, "l1", T10)],
         bpod("pl", 10, None, group="gl"),
         ("nominated", "l1", ["l1-b"], 1, 1))
    # ---- spread
    case([bnode("s1a", "gs1", labels={ZONE: "zs1"}), bnode("s1b", "gs1", labels={ZONE: "zs2"}),
          bnode("s1c", "gs1", labels={ZONE: "zs1"})],
         [bpod("s1a-y1", 1, "100m", "s1a", T0, labels={"app": "sp1"}),
          bpod("s1a-y2", 1, "100m", "s1a", T10, labels={"app": "sp1"}),
          bpod("s1b-h", 100, "2000m", "s1b", T0), bpod("s1c-h", 100, "2000m", "s1c", T0, labels={"app": "sp1"})],
         bpod("ps1", 10, "100m", group="gs1", labels={"app": "sp1"},
              topologySpreadConstraints=[_spread({"app": "sp1"}, ZONE, 3), _spread({"app": "sp1"}, HOST, 1)]),
         ("nominated", "s1a", ["s1a-y1", "s1a-y2"], 3, 1))
    case([bnode("s2a", "gs2"), bnode("s2b", "gs2")],
         [bpod("s2a-v", 1, "100m", "s2a", T0, labels={"app": "sk", "tier": "t"}),
          bpod("s2a-w", 100, "100m", "s2a", T0, labels={"tier": "t"}), bpod("s2b-h", 100, "2000m", "s2b", T0)],
         bpod("ps2", 10, "100m", group="gs2", labels={"app": "sk", "tier": "t"},
              topologySpreadConstraints=[_spread({"app": "sk"}, HOST), _spread({"tier": "t"}, HOST)]),
         ("nominated", "s2a", ["s2a-v"], 2, 1))
    s3 = {"app": "s3"}
    case([bnode("s3a", "gs3"), bnode("s3b", "gs3"), bnode("s3c", "gs3")],
         [bpod("s3a-y1", 1, "100m", "s3a", T0, labels=s3), bpod("s3a-y2", 1, "100m", "s3a", T10, labels=s3),
          bpod("s3a-fill", 1, "1800m", "s3a", T10)]
         + [bpod("s3b-h%d" % k, 100, "500m", "s3b", T0, labels=s3) for k in range(3)] + [bpod("s3b-f", 100, "500m", "s3b", T0)]
         + [bpod("s3c-h%d" % k, 100, "400m", "s3c", T0, labels=s3) for k in range(5)],
         bpod("ps3", 10, "1000m", group="gs3", labels=s3, topologySpreadConstraints=[_spread(s3, HOST)]),
         ("nominated", "s3a", ["s3a-fill"], 3, 1))
    s4 = {"app": "s4"}
    case([bnode("s4a", "gs4"), bnode("s4b", "gs4")],
         [bpod("s4a-y1", 1, "100m", "s4a", T0, labels=s4), bpod("s4a-y2", 1, "100m", "s4a", T10, labels=s4),
          bpod("s4a-y3", 1, "100m", "s4a", T20, labels=s4), bpod("s4b-h", 100, "2000m", "s4b", T0, labels=s4)],
         bpod("ps4", 10, "100m", group="gs4", labels=s4, topologySpreadConstraints=[_spread(s4, HOST)]),
         ("nominated", "s4a", ["s4a-y2", "s4a-y3"], 2, 1))
    # ---- existing pods' anti-affinity
    case([bnode("e1", "ge1")],
         [bpod("e1-guard", 1, "100m", "e1", T0, affinity=_anti_terms({"app": "web2"}, {"tier": "front"}))],
         bpod("pe1", 10, "100m", group="ge1", labels={"app": "web2", "tier": "front"}),
         ("nominated", "e1", ["e1-guard"], 1, 1))
    case([bnode("e2", "ge2")],
         [bpod("e2-guard", 100, "100m", "e2", T0, affinity=_anti_terms({"app": "web3"})), bpod("e2-low", 1, "100m", "e2", T0)],
         bpod("pe2", 10, "100m", group="ge2", labels={"app": "web3"}),
         ("no_candidate", None, [], 1, 0))
    # ---- ordering
    case([bnode("o1", "go1"), bnode("o2", "go1")],
         [bpod("o1-n5", -5, "1000m", "o1", T0), bpod("o1-n1", -1, "1000m", "o1", T0), bpod("o2-n2", -2, "2000m", "o2", T0)],
         bpod("po1", 10, "1500m", group="go1"),
         ("nominated", "o2", ["o2-n2"], 2, 2))
    case([], [], bpod("po2", -3, "1000m", group="go1"), ("nominated", "o1", ["o1-n5"], 2, 1))
    case([bnode("o3", "go3")],
         [bpod("o3-u1", 1, "600m", "o3"), bpod("o3-s", 1, "600m", "o3", T10), bpod("o3-u2", 1, "600m", "o3")],
         bpod("po3", 10, "2000m", group="go3"),
         ("nominated", "o3", ["o3-s", "o3-u1", "o3-u2"], 1, 1))
    # ---- node lists and PreFilter
    case([bnode("n1", "gn"), bnode("n2", "gn"), bnode("n3", "gn")],
         [bpod("n1-l", 1, "2000m", "n1", T0), bpod("n2-l", 5, "2000m", "n2", T0), bpod("n3-l", 1, "2000m", "n3", T0)],
         bpod("pn", 10, "1000m", group="gn", affinity=_names_terms("n1", "n2")),
         None)  # filled in below: n_potential is the cluster's node count
    case([], [], bpod("pn2", 10, "1000m", group="gn", affinity=_names_affinity(["n1", "n2"])), None)
    case([], [], bpod("conflict", 10, "100m", affinity=_names_affinity(["a"], ["b"])),
         ("no_candidate", None, [], 0, 0))
    names = [p["metadata"]["name"] for p in P]
    E[names.index("pn")] = ("nominated", "n1", ["n1-l"], len(N), 2)
    E[names.index("pn2")] = ("no_candidate", None, [], len(N) - 2, 0)
    return N, B, P, E


def min_rise_fixture():
    """The second criticalPaths entry (the minimum over the OTHER pairs), which only a nominee
    can expose: (nodes, bound, pods, nominations [(pod name, node name)], expect).

    hostname spread, app=mr, maxSkew 1.  r1: low app=mr y1 (100m, T0), low filler 1900m (T10);
    r2: two high app=mr, full; r3: four high app=mr, full.  Pairs r1 1 (the minimum), r2 2, r3 4.
    q (priority 50, app=mr, 100m) is nominated to r1; pr has priority 10, 1000m, app=mr.
    RunFilterPluginsWithNominatedPods adds q in a first pass (priority 50 >= 10).
    Cycle on r1: first pass Fit 2000m + 100m + 1000m > 2000m -> Fit, potential.
    Dry run: remove y1 and the filler.  First pass: CPU 1100m; pair 0 + 1 (q) = 1, minimum
    min(1, 2) = 1 -> 1+1-1 passes; second pass 0+1-0 passes.
    Reprieve y1: first pass pair 1 + 1 = 2, the other pairs' minimum is 2 (r2) -> 2+1-2 = 1
    passes (taking r1's own ORIGINAL count 1 as "the others" gives 2+1-1 = 2 > 1 and evicts y1);
    second pass 1+1-1 passes -> y1 stays.  Reprieve the filler: 3100m -> victim.
    [r1-fill]; r2, r3 are potential (Fit) without lower-priority pods: 3 / 1."""
    mr = {"app": "mr"}
    nodes = [bnode("r1"), bnode("r2"), bnode("r3")]
    bound = [bpod("r1-y1", 1, "100m", "r1", T0, labels=mr), bpod("r1-fill", 1, "1900m", "r1", T10)]
    bound += [bpod("r2-h%d" % k, 100, "1000m", "r2", T0, labels=mr) for k in range(2)]
    bound += [bpod("r3-h%d" % k, 100, "500m", "r3", T0, labels=mr) for k in range(4)]
    pods = [bpod("pr", 10, "1000m", labels=mr, topologySpreadConstraints=[_spread(mr, HOST)]),
            bpod("q", 50, "100m", labels=mr)]
    return nodes, bound, pods, [("q", "r1")], [("nominated", "r1", ["r1-fill"], 3, 1), None]


def after_remove_fixture():
    """NodeInfo order after RemovePod: (nodes, bound, pods, removed pod name, expect before, expect after).

    v1: r0, r1, r2, r3 in NodeInfo order, priority 1, no startTime, 500m each.  pv 2000m evicts
    every one of them; equal priority and no start time -> NodeInfo order [r0, r1, r2, r3].
    NodeInfo.RemovePod(r0) moves the last pod into the freed slot (removeFromSlice): the list
    is [r3, r1, r2], and so is the eviction order afterwards."""
    nodes = [bnode("v1")]
    bound = [bpod("v1-r%d" % k, 1, "500m", "v1") for k in range(4)]
    pods = [bpod("pv", 10, "2000m")]
    return (nodes, bound, pods, "v1-r0",
            ("nominated", "v1", ["v1-r0", "v1-r1", "v1-r2", "v1-r3"], 1, 1),
            ("nominated", "v1", ["v1-r3", "v1-r1", "v1-r2"], 1, 1))


# --------------------------------------------------------------------------------------
# Constructed clusters for the device's reductions.  No zone labels: the nodeTree order is the
# input order, so node i of the list is device index i (the CPU test asserts it).
WG = 64        # k_preempt_nodes: one lane per node, 64-node workgroups
T5, T1, T9 = "2024-01-01T00:00:05Z", "2024-01-01T00:00:01Z", "2024-01-01T00:00:09Z"
STD = [(5, T5)]  # the standard candidate: one victim of priority 5 started at T5


def _ident_nodes(n):
    return [bnode("n%04d" % i, labels={"id": str(i)}) for i in range(n)]


def _only(allowed, all_special):
    """Node affinity that keeps every node except the special ones of other rungs."""
    out = sorted(all_special - set(allowed))
    if not out:
        return None
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
        {"matchExpressions": [{"key": "id", "operator": "NotIn", "values": [str(i) for i in out]}]}]}}}


def _fill_cluster(n, victims_of):
    """n nodes of 2 CPU; node i holds victims_of[i] = [(priority, start)] as 100m pods in that
    NodeInfo order, every other node one priority-1000 pod of 2000m."""
    nodes = _ident_nodes(n)
    bound = []
    for i in range(n):
        name = "n%04d" % i
        if i in victims_of:
            for k, (prio, start) in enumerate(victims_of[i]):
                bound.append(bpod("%s-v%d" % (name, k), prio, "100m", name, start))
        else:
            bound.append(bpod("%s-full" % name, 1000, "2000m", name, T0))
    return nodes, bound


# rung: (criterion, A's victims, winner).  B is the standard candidate [(5, T5)]; the preemptor
# (priority 10, 2000m) needs the whole node, so every listed pod is evicted, in the listed order
# (priority descending, start ascending, NodeInfo order on ties).
#   hp      A's highest victim priority 4 < 5                                  -> A
#   sum     A evicts (5, 3): sums 8 + 2*2^31 > 5 + 2^31, equal highest         -> B
#   cnt     A evicts (5, -2^31): sums equal (5 + 2^31 + 0), 2 > 1 victims      -> B
#           (Sum(priority + 2^31) ties between different counts only through priority -2^31)
#   start   equal through the count; A's victim started later (T9 > T5)        -> A
#   index   identical victims: the lower node index (the tie upstream leaves to map order)
#   nostart A's victim has no startTime: it sorts after every start time       -> A
# and two rungs without the standard candidate, for the lexicographic order:
#   lex-hp  X evicts (6): sum 6 + 2^31 is the smaller, highest 6 the larger;
#           Y evicts (5, 5)                                                    -> Y
#   lex-sum X evicts (5, -2^31, -2^31): sum 5 + 2^31 the smaller, 3 victims;
#           Y evicts (5, 4): 2 victims                                         -> X
RUNGS = [("hp", [(4, T5)], "A"), ("sum", [(5, T5), (3, T5)], "B"), ("cnt", [(5, T5), (MIN_PRIO, T5)], "B"),
         ("start", [(5, T9)], "A"), ("index", [(5, T5)], "low"), ("nostart", [(5, None)], "A")]
LEX = [("lex-hp", [(6, T5)], [(5, T5), (5, T5)], "Y"),
       ("lex-sum", [(5, T5), (MIN_PRIO, T5), (MIN_PRIO, T5)], [(5, T5), (4, T5)], "X")]
CROSS = {2: [(0, 1)] * 8,
         3: [(0, 2), (0, 1), (1, 2), (0, 1), (1, 2), (0, 2), (0, 1), (0, 1)],
         4: [(0, 3), (1, 2), (2, 3), (0, 1), (1, 3), (0, 2), (1, 3), (2, 3)]}
SAME = {2: [0] * 8, 3: [1, 0, 1, 0, 1, 0, 1, 0], 4: [1, 2, 0, 3, 1, 2, 3, 0]}


def ladder(n_nodes):
    """(nodes, bound, pods, expect, layout): one pending pod per rung; layout[j] = (criterion,
    "same" | "cross", [candidate node indices], winner index).  Each criterion of RUNGS and LEX
    decides once between two candidates of one 64-node workgroup and once between candidates of
    different workgroups (a lex rung across workgroups is left out where the upper workgroup
    has a single node: n_nodes = 65)."""
    W = (n_nodes + WG - 1) // WG
    nxt = {w: w * WG for w in range(W)}

    def take(w):
        i = nxt[w]
        assert i < min(n_nodes, (w + 1) * WG), "workgroup %d is out of nodes" % w
        nxt[w] = i + 1
        return i

    std = {}

    def std_of(w):
        if w not in std:
            std[w] = take(w)
        return std[w]

    victims_of, layout = {}, []
    # the upper workgroup's standard candidates first: they may be its only node
    for a, b in CROSS[W][:len(RUNGS)]:
        std_of(b)
    for k, (crit, spec, win) in enumerate(RUNGS):
        for kind in ("same", "cross"):
            if kind == "same":
                w = SAME[W][k]
                b_node, a_node = std_of(w), take(w)
            else:
                wa, wb = CROSS[W][k]
                a_node, b_node = take(wa), std_of(wb)
            victims_of[a_node], victims_of[b_node] = spec, STD
            winner = {"A": a_node, "B": b_node, "low": min(a_node, b_node)}[win]
            layout.append((crit, kind, [a_node, b_node], winner))
    for k, (crit, xs, ys, win) in enumerate(LEX):
        for kind in ("same", "cross"):
            if kind == "same":
                wx = wy = SAME[W][len(RUNGS) + k]
            else:
                wx, wy = CROSS[W][len(RUNGS) + k]
                if min(n_nodes, (wy + 1) * WG) - nxt[wy] < 1:
                    continue
            x, y = take(wx), take(wy)
            victims_of[x], victims_of[y] = xs, ys
            layout.append((crit, kind, [x, y], x if win == "X" else y))
    nodes, bound = _fill_cluster(n_nodes, victims_of)
    special = set(victims_of)
    pods, expect = [], []
    for j, (crit, kind, cand, winner) in enumerate(layout):
        pods.append(bpod("rung-%02d-%s-%s" % (j, crit, kind), 10, "2000m", affinity=_only(cand, special)))
        name = "n%04d" % winner
        expect.append(("nominated", name, ["%s-v%d" % (name, k) for k in range(len(victims_of[winner]))],
                       n_nodes - (len(special) - len(cand)), len(cand)))
    return nodes, bound, pods, expect, layout


PICK_LANES = 64  # pickOneNodeForPreemption's last workgroup folds tuples b, b + 64, ... on one lane


def wide_start(n_nodes=4200):
    """More than 64 k_preempt_nodes workgroups, so one lane of the final reduction folds two
    workgroups' tuples itself: candidates at nodes 10 (workgroup 0) and 64 * 64 + 10 (workgroup
    64), equal through the count; the first started later (T9 > T5) -> node 10.  A second pod
    sees them with the later start on the other side.  (nodes, bound, pods, expect)."""
    a, a2, b, c = 10, 30, WG * PICK_LANES + 10, WG * PICK_LANES + 40
    victims_of = {a: [(5, T9)], a2: [(5, T5)], b: [(5, T5)], c: [(5, T9)]}
    nodes, bound = _fill_cluster(n_nodes, victims_of)
    special = set(victims_of)
    pods = [bpod("wide-first", 10, "2000m", affinity=_only([a, b], special)),
            bpod("wide-second", 10, "2000m", affinity=_only([a2, c], special))]
    # the second pod: node 30 (workgroup 0) started T5, node c (workgroup 64, the same lane) T9 -> c;
    # the third sees a2 and b (workgroups 0 and 64), a full tie -> the lower index
    pods.append(bpod("wide-third", 10, "2000m", affinity=_only([a2, b], special)))
    expect = [("nominated", "n%04d" % a, ["n%04d-v0" % a], n_nodes - 2, 2),
              ("nominated", "n%04d" % c, ["n%04d-v0" % c], n_nodes - 2, 2),
              ("nominated", "n%04d" % a2, ["n%04d-v0" % a2], n_nodes - 2, 2)]
    return nodes, bound, pods, expect


def plain(n_nodes):
    """Edge sizes of the node grid: every node full of priority-1000 pods except the last one,
    which holds two low pods (priority 3 at T5, priority 2 at T1; 1000m each); a preemptor of
    2000m evicts both, the more important first.  n_nodes / 1."""
    last = n_nodes - 1
    nodes, bound = _fill_cluster(n_nodes, {last: [(3, T5), (2, T1)]})
    for b in bound:
        if b["spec"]["nodeName"] == "n%04d" % last:
            b["spec"]["containers"][0]["resources"]["requests"]["cpu"] = "1000m"
    name = "n%04d" % last
    return nodes, bound, [bpod("edge", 10, "2000m")], [("nominated", name, [name + "-v0", name + "-v1"], n_nodes, 1)]


def twelve():
    """One node with 12 potential victims, all evicted: priorities 3, 2, 1 cycling over the
    NodeInfo order, start times T9, T5, T1, none cycling with another period, so the sort has
    ties in both keys.  The expected order is written out: priority descending, start
    ascending (none last), NodeInfo order on ties -- an insertion sort (Go's sort.Slice below
    13 elements) is stable, so the ties keep NodeInfo order."""
    starts = [T9, T5, T1, None]
    spec = [(3 - k % 3, starts[(k * 3 + k // 3) % 4]) for k in range(12)]
    nodes, bound = _fill_cluster(3, {1: spec})
    key = {T1: 1, T5: 5, T9: 9, None: 99}
    order = sorted(range(12), key=lambda k: (-spec[k][0], key[spec[k][1]], k))
    return nodes, bound, [bpod("dozen", 10, "2000m")], [("nominated", "n0001", ["n0001-v%d" % k for k in order], 3, 1)]


# --------------------------------------------------------------------------------------
RACK = "example.com/rack"
STATS_NODES = 256  # k_preempt_stats: one workgroup per 256 nodes, ranges ceil(N / workgroups) wide


def stats_ranges(n_nodes):
    nb = max((n_nodes + STATS_NODES - 1) // STATS_NODES, 1)
    per = (n_nodes + nb - 1) // nb
    return nb, per


def two_smallest_placements(n_nodes):
    """{name: (a, b, count a, count b)}: the node (or rack) of the smallest count, of the second
    smallest, and the counts.  Indices are chosen with a % 3, b % 3 and X % 3 distinct (X = 2 + 3k),
    so the same placements serve the rack key (rack = index % 3)."""
    nb, per = stats_ranges(n_nodes)
    lo1 = per + (-per) % 3  # the first multiple of 3 inside the second range
    assert per <= lo1 < 2 * per
    return {"one-range": (3, 13, 1, 2),           # both in range 0
            "adjacent-up": (3, lo1 + 1, 1, 2),    # smallest in range 0, second in range 1
            "adjacent-down": (lo1, 4, 1, 2),      # smallest in range 1, second in range 0
            "tied": (3, lo1 + 1, 2, 2),           # the same count in both ranges: the lower pair is "the" minimum
            "last-range": ((n_nodes - 1) // 3 * 3, 4, 1, 2)}  # smallest in the last (shorter) range


def two_smallest(n_nodes, placement, key=HOST):
    """The spread PreFilter's two smallest pair counts across k_preempt_stats workgroups.

    hostname key (node-valued: each workgroup's two smallest, merged by the last one): every
    node holds 4 priority-1000 app=ts pods of 500m (pair count 4, full), except
      a   `ca` app=ts pods of priority 5 (100m, distinct start times), two priority-4 pods
          without the label (junk1 = 1200m - ca * 100m, junk2 = 800m): full, pair count ca;
      b   `cb` priority-1000 app=ts pods + a priority-1000 filler: full, pair count cb;
      X   six priority-2 app=ts pods of 300m (T0 + k seconds): pair count 6.
    rack key (3 values, index % 3: a histogram whose bins every workgroup adds to by atomics):
    the other nodes hold one priority-1000 pod of 2000m without the label, so the rack counts
    are ca (a's rack), cb (b's rack) and 6 (X's rack).

    px (priority 3, 200m, app=ts, DoNotSchedule maxSkew 1 on the key) can evict only X's pods.
    Every other node fails Fit with nothing below priority 3; X passes Fit (2000m) and fails the
    spread: 6 + 1 - m0 > 1.  Dry run on X: pair 0 after the removals; a reprieve passes while
    pair + 1 - min(pair, m0) <= 1, i.e. pair <= m0: m0 pods stay and 6 - m0 are evicted, the
    latest started -> X-v[m0..5].  n_nodes / 1: the victims count the global minimum m0.

    pa (priority 50, the same constraint, 200m and 7Gi) never fits X, which also holds a
    priority-1000 pod of 2Gi (8Gi allocatable): X is potential but no candidate.  It runs with
    q (priority 500, app=ts, no requests) nominated to a.  Cycle on a: Fit (2000m + 200m).  Dry
    run on a: pair 0.
    Reprieving the app=ts pods (priority 5, first in order): the first pass adds q, so the
    t-th reprieve passes while t + 1 + 1 - min(t + 1, m1) <= 1, i.e. t + 1 <= m1 (m1: the
    minimum over the OTHER pairs, a being the minimum itself).  With m1 >= ca + 1 all ca stay;
    when b ties (m1 = ca) the last one is evicted.  Then junk1 stays (CPU <= 1400m) and junk2
    overflows: victims [junk2], or [a's last app=ts pod, junk2] on the tie.
    n_nodes / 1: the victims tell m1 == ca from m1 > ca on the minimum node itself.

    (nodes, bound, pods, nominations, info)."""
    a, b, ca, cb = two_smallest_placements(n_nodes)[placement]
    x = 2 + 3 * ((n_nodes // 2) // 3)
    assert len({a % 3, b % 3, x % 3}) == 3 and max(a, b, x) < n_nodes
    ts = {"app": "ts"}
    nodes = [bnode("n%04d" % i, labels={"id": str(i), RACK: "r%d" % (i % 3)}) for i in range(n_nodes)]
    bound = []
    for i in range(n_nodes):
        name = "n%04d" % i
        if i == a:
            for k in range(ca):
                bound.append(bpod("%s-m%d" % (name, k), 5, "100m", name, "2024-01-01T00:00:%02dZ" % k, labels=ts))
            bound.append(bpod(name + "-junk1", 4, "%dm" % (1200 - 100 * ca), name, T0))
            bound.append(bpod(name + "-junk2", 4, "800m", name, T10))
        elif i == b:
            for k in range(cb):
                bound.append(bpod("%s-m%d" % (name, k), 1000, "100m", name, T0, labels=ts))
            bound.append(bpod(name + "-fill", 1000, "%dm" % (2000 - 100 * cb), name, T0))
        elif i == x:
            for k in range(6):
                bound.append(bpod("%s-v%d" % (name, k), 2, "300m", name, "2024-01-01T00:00:%02dZ" % k, labels=ts))
            bound.append(bpod(name + "-pin", 1000, {"memory": "2Gi"}, name, T0))
        elif key == HOST:
            for k in range(4):
                bound.append(bpod("%s-h%d" % (name, k), 1000, "500m", name, T0, labels=ts))
        else:
            bound.append(bpod(name + "-full", 1000, "2000m", name, T0))
    con = [_spread(ts, key)]
    pods = [bpod("px", 3, "200m", labels=ts, topologySpreadConstraints=con),
            bpod("pa", 50, {"cpu": "200m", "memory": "7Gi"}, labels=ts, topologySpreadConstraints=con),
            bpod("q", 500, None, labels=ts)]
    m0, m1 = min(ca, cb), max(ca, cb)
    xn, an = "n%04d" % x, "n%04d" % a
    expect = [("nominated", xn, ["%s-v%d" % (xn, k) for k in range(m0, 6)], n_nodes, 1),
              ("nominated", an, ([] if m1 > ca else ["%s-m%d" % (an, ca - 1)]) + [an + "-junk2"], n_nodes, 1),
              None]
    return nodes, bound, pods, [("q", an)], dict(a=a, b=b, x=x, expect=expect)




# --------------------------------------------------------------------------------------
# saturated_rich: preempt_fixtures.saturated plus what it lacks.  Every node is of one kind
# (label kind=...), full in that kind's resource:
#   cpu  CPU requested == allocatable; the 4-core ones hold 5 to 12 pods
#   mem  2Gi of memory, less than 256Mi free; 300m of CPU free
#   gpu  every example.com/gpu taken; 300m of CPU free
#   lim  as many pods as the pod limit (4 or 6) allows; 300m of CPU free
# and pending pods select a kind whose one resource they lack (mem: 1 to 1.5Gi; gpu: 1 or 2
# devices; lim: no requests at all -> "Too many pods" alone), or take CPU anywhere.  On top:
# required pod affinity on hostname and zone (half of them matching their own term), pod
# anti-affinity, single, two-key and same-key spreads, bound pods with one or two anti-affinity
# terms, negative priorities, three distinct start times (ties are common), at most 12 pods
# per node.
KINDS = ["cpu", "cpu", "mem", "gpu", "lim"]


def _split(r, total, k, step):
    """k positive multiples of `step` that sum to total (total >= k * step)."""
    units = total // step
    cuts = sorted(r.sample(range(1, units), k - 1)) if k > 1 else []
    parts = [b - a for a, b in zip([0] + cuts, cuts + [units])]
    return [p * step for p in parts]


def saturated_rich(seed: int, n_nodes: int, n_pods: int):
    r = random.Random(1000 + seed)
    zones = ["z%d" % i for i in range(4)]
    starts = [T0, T10, T20]
    apps = ["a%d" % i for i in range(3)]
    tiers = ["t0", "t1"]
    nodes, bound, pods = [], [], []
    for i in range(n_nodes):
        name = "n%04d" % i
        kind = r.choice(KINDS)
        cores = r.choice([2, 4])
        k = r.randint(5, 12) if (kind == "cpu" and cores == 4) else r.randint(3, 8)
        al = {"cpu": str(cores), "memory": "2Gi" if kind == "mem" else "%dGi" % (4 * cores), "pods": "110"}
        gpus = 0
        if kind == "gpu":
            gpus = r.choice([2, 4])
            k = max(k, gpus)
            al[GPU] = str(gpus)
        if kind == "lim":
            k = r.choice([4, 6])
            al["pods"] = str(k)
        nodes.append({"metadata": {"name": name, "labels": {HOST: name, ZONE: r.choice(zones), "kind": kind}},
                      "spec": {}, "status": {"allocatable": al}})
        cpus = _split(r, cores * 1000 - (0 if kind == "cpu" else 300), k, 50)
        mems = _split(r, 2048 - 64 * r.randint(1, 3), k, 64) if kind == "mem" else [r.choice([128, 256])] * k
        for j in range(k):
            req = {"cpu": "%dm" % cpus[j], "memory": "%dMi" % mems[j]}
            if j < gpus:
                req[GPU] = "1"
            spec = {"nodeName": name, "priority": r.choice([-10, -1, 0, 10, 10, 100, 1000]),
                    "containers": [{"name": "c", "resources": {"requests": req}}]}
            u = r.random()
            if u < 0.03:
                spec["affinity"] = _anti_terms({"app": r.choice(apps)}, {"tier": r.choice(tiers)})
            elif u < 0.06:
                spec["affinity"] = _anti_terms({"app": r.choice(apps)})
            pod_ = {"metadata": {"name": "%s-b%d" % (name, j), "namespace": "default",
                                 "labels": {"app": r.choice(apps), "tier": r.choice(tiers)}}, "spec": spec}
            if r.random() < 0.85:
                pod_["status"] = {"startTime": r.choice(starts)}
            bound.append(pod_)
    for j in range(n_pods):
        shape = r.choice(["cpu", "cpu", "big", "mem", "gpu", "lim", "small", "small"])
        sel = None
        if shape == "cpu":
            req = {"cpu": "%dm" % r.choice([500, 1000, 2000]), "memory": "256Mi"}
        elif shape == "big":
            req = {"cpu": "4000m"}
        elif shape == "mem":
            req, sel = {"cpu": "100m", "memory": "%dMi" % r.choice([1024, 1536])}, "mem"
        elif shape == "gpu":
            req, sel = {"cpu": "100m", "memory": "64Mi", GPU: str(r.choice([1, 2]))}, "gpu"
        elif shape == "lim":
            req, sel = {}, "lim"
        else:
            req, sel = {"cpu": "100m"}, r.choice(["mem", "gpu"])
        spec = {"priority": r.choice([-5, 0, 10, 100, 100, 1000, 5000]),
                "containers": [{"name": "c", "resources": {"requests": req}}]}
        if sel:
            spec["nodeSelector"] = {"kind": sel}
        labels = {"app": r.choice(apps), "tier": r.choice(tiers)}
        u = r.random()
        if shape == "small":
            # these fit by their requests: each gets a constraint that most nodes of the kind fail,
            # so that a node whose cycle status is PodTopologySpread / InterPodAffinity gets nominated
            u = 2.0
            if r.random() < 0.5:
                t = r.choice(tiers)
                spec["affinity"] = _anti_terms({"tier": t})
            else:
                a = r.choice(apps)
                labels["app"] = a
                spec["topologySpreadConstraints"] = [_spread({"app": a}, ZONE, r.choice([1, 2])), _spread({"app": a}, HOST, 1)]
        if u < 0.12:
            spec["topologySpreadConstraints"] = [_spread({"app": r.choice(apps)}, r.choice([HOST, ZONE]))]
        elif u < 0.20:
            a = r.choice(apps)
            spec["topologySpreadConstraints"] = [_spread({"app": a}, ZONE, r.choice([2, 4, 8])), _spread({"app": a}, HOST, 1)]
        elif u < 0.28:
            key = r.choice([HOST, ZONE])
            spec["topologySpreadConstraints"] = [_spread({"app": r.choice(apps)}, key, r.choice([1, 2])),
                                                 _spread({"tier": r.choice(tiers)}, key, r.choice([1, 3]))]
        elif u < 0.48:
            spec["affinity"] = pf._anti(r.choice(apps), r.choice([HOST, HOST, ZONE]))
        elif u < 0.70:
            a = r.choice(apps)
            if r.random() < 0.5:
                labels["app"] = a  # matches its own term
            spec["affinity"] = _aff({"app": a}, r.choice([HOST, HOST, ZONE]))
        if r.random() < 0.06:
            spec["preemptionPolicy"] = "Never"
        pods.append({"metadata": {"name": "p%04d" % j, "namespace": "default", "labels": labels}, "spec": spec})
    return nodes, bound, pods


RICH_SHAPES = [(1, 60, 40), (2, 130, 50), (3, 300, 50)]
