"""Tiny clusters whose class_count / term_count cells sit on k_spread's integer edges (test
infrastructure).

k_spread keeps resident counts as 16-bit cells in LDS and counts, histograms and scores in 32 bits.
The host admits a batch only inside (spread_bounds_ok / build_gpods in csrc/kss_lib.hip), stated
here once in Python integers (spread_bounds):
  cell    the largest single count + n_pods * max_mult <= 65535 (max_mult: how often one pod's commit
          adds to one count row -- 2 for a pod with two identical affinity terms)
  sum32   MAXK * ref_weight * total < 2^31 - 1, where total = max(sum of all class counts, sum of all
          term counts) + n_pods * (1 + the most own term rows of a pod) and ref_weight the largest
          sum of |coefficient| over the count rows one constraint / inter-pod entry reads
  soft2   with more than one ScheduleAnyway constraint on a pod:
          max_soft * (ref_weight * total * log(N + 2) + max maxSkew + 1) < 2^31 - 1 (in doubles)
Each fixture comes as a pair, one value apart: inside its bound by the stated margin (0) and one
unit across, and asserts that from Python integers.  The counts are written into the compiled
arrays (65,535 bound-pod objects per cell is not a fixture): nothing ties them to pod_count, and the
C oracle reads the same arrays.  The object-level oracle is left out for the same reason.

Where the arithmetic is integer only -- DoNotSchedule skew verdicts, InterPodAffinity raw sums and
their normalisation at the maximum -- the fixture also states n_feasible, the chosen node and
best_total per pod (`expect`).  All nodes are huge and the pods best-effort, so NodeResourcesFit is
99 and BalancedAllocation 100 everywhere; every node but one carries a PreferNoSchedule taint, so the
untainted node wins ties by 100 * the TaintToleration weight.  PodTopologySpread soft scores go
through Go's log: there the C oracle is the reference and `expect` is None.

Classes:
  cell   6 nodes in 3 zones, 8 pods that all land on n00: the preferred-affinity term row (two
         identical terms per pod, max_mult 2) holds 65535 - 16 on n00 and reaches exactly 65535; the
         class row read by the DoNotSchedule constraint and the inter-pod score sits beside it, and the
         other zones are filled so that the skew of zones 1 / 2 is maxSkew + 1 for pod n - 4 and
         exactly maxSkew for pod n - 3 at counts near 65535.  soft=True adds a ScheduleAnyway
         constraint reading the same class row.
  sum32  24 nodes, 4 topology keys (MAXK), preferred terms of weight 100 over two class rows on every
         key and the hard-affinity weight on one term row: ref_weight 201.  A reference's true sum is
         at most max |coefficient| * total, so with two rows of 100 the largest true intermediate
         (stated as `largest`) is about half the bound; one row cannot reach the bound within 24 nodes
         of 65535 (24 * 65535 * 4 * 101 < 2^31).
  soft2  2 and 4 ScheduleAnyway constraints; the zone constraint's maxSkew moves the bound by one.
fold16 (ref_weight * max_mult of 32767 against 32768 with option fold) is not built.  build_gpods does
not refuse such a record; the class is dropped because nothing observable sits on that edge: across it
the host only clears GPod::fold, the batch stays on k_spread on both sides (last_kernel cannot tell),
and the delta that really travels as an int16 is one pod's commit -- at most its class row and 7 own
term rows, each under a coefficient of at most 7 * 100 -- so no admissible pod brings a true delta
within a factor of five of 32767.  It would also need 328 class rows, i.e. 328 pod objects.  The fold
path itself runs on the cell and sum32 fixtures (tests/test_gpu_count_envelope.py, option fold 1)."""
import math

import numpy as np

MAXK = 4
LIM32 = (1 << 31) - 1
CELL_MAX = 65535
ZONE = "topology.kubernetes.io/zone"
HOST = "kubernetes.io/hostname"
W = dict(tt=3, pts=2, ipa=2, fit=1, ba=1)  # the default profile's weights
CONST = 100 * W["tt"] + 100 * W["pts"] + 99 * W["fit"] + 100 * W["ba"]  # every score but InterPodAffinity, untainted node


def spread_bounds(needs, total, cell, N):
    """spread_bounds_ok: needs = dict(ref_weight, max_soft, max_skew); total and cell as the host
    forms them (after the batch).  Returns (inside, figures)."""
    ref = needs["ref_weight"] * total
    fig = dict(cell=cell, sum32=MAXK * ref)
    ok = cell <= CELL_MAX and MAXK * ref < LIM32
    if needs.get("max_soft", 0) > 1:
        fig["soft2"] = float(needs["max_soft"]) * (float(ref) * math.log(float(N) + 2.0) + float(needs["max_skew"]) + 1.0)
        ok = ok and fig["soft2"] < float(LIM32)
    return ok, fig


def f64_sum(max_req, max_nz, n_pods, max_creq, max_cnz):
    """f64_exact's two sums (both must stay below 2^52)."""
    return max_req + n_pods * max_creq, max_nz + n_pods * max_cnz


def _node(name, labels, tainted):
    n = {"metadata": {"name": name, "labels": dict(labels, **{HOST: name})}, "spec": {},
         "status": {"allocatable": {"cpu": "%dm" % (1 << 40), "memory": "%d" % (1 << 45), "pods": "1000"}}}
    if tainted:
        n["spec"]["taints"] = [{"key": "edge", "value": "t", "effect": "PreferNoSchedule"}]
    return n


def _pod(name, labels, spec):
    return {"metadata": {"name": name, "namespace": "default", "labels": labels},
            "spec": dict(spec, containers=[{"name": "c"}])}


def _pref(key, labels, weight=100):
    return {"weight": weight, "podAffinityTerm": {"topologyKey": key, "labelSelector": {"matchLabels": labels}}}


def class_row(cc, labels):
    return cc.classes.index(("default", tuple(sorted(labels.items()))))


def term_row(cc, kind, key):
    rows = [i for i, (k, _w, t) in enumerate(cc.terms) if k == kind and t.topology_key == key]
    assert len(rows) == 1, rows
    return rows[0]


def totals(cc, cp):
    """(total, cell) as the host forms them for the whole podset, from the compiled arrays."""
    N = cc.n_nodes
    # (without rows the compiled column is a one-element placeholder)
    c = cc.arrays["class_count"][:, :N].astype(int) if cc.classes else np.zeros((0, N), int)
    t = cc.arrays["term_count"][:, :N].astype(int) if cc.terms else np.zeros((0, N), int)
    own = [int(p["own_terms_len"]) for p in cp.pods]
    mult = 1
    for p in cp.pods:
        ids = [int(x) for x in cp.ints[int(p["own_terms_off"]):int(p["own_terms_off"]) + int(p["own_terms_len"])]]
        mult = max([mult] + [ids.count(i) for i in ids])
    total = max(int(c.sum()), int(t.sum())) + cp.n * (1 + max(own))
    cell = max(int(c.max()) if c.size else 0, int(t.max()) if t.size else 0) + cp.n * mult
    return total, cell


# --------------------------------------------------------------------------------------
# cell
# --------------------------------------------------------------------------------------
CELL_PODS, CELL_SKEW = 8, 2
CELL_REF = 2 * 100 + 100  # the inter-pod score entry: the class row under two identical terms, the term row
CELL_NODES = ["n00", "n01", "n10", "n11", "n20", "n21"]


def cell_objects(soft=False, port=False, wide=0):
    """port: pod 3 also holds a host port (the ports-and-images form).  wide: that many more empty,
    tainted nodes in zone 2 (a cluster large enough for the percentageOfNodesToScore window)."""
    nodes = [_node(n, {ZONE: "z" + n[1]}, tainted=n != "n00") for n in CELL_NODES]
    nodes += [_node("x%03d" % i, {ZONE: "z2"}, tainted=True) for i in range(wide)]
    cons = [{"maxSkew": CELL_SKEW, "topologyKey": ZONE, "whenUnsatisfiable": "DoNotSchedule", "nodeAffinityPolicy": "Ignore",
             "labelSelector": {"matchLabels": {"app": "w"}}}]
    if soft:
        cons.append({"maxSkew": 1, "topologyKey": ZONE, "whenUnsatisfiable": "ScheduleAnyway", "nodeAffinityPolicy": "Ignore",
                     "labelSelector": {"matchLabels": {"app": "w"}}})
    aff = {"podAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [_pref(ZONE, {"app": "w"})] * 2}}
    pods = [_pod("w%02d" % i, {"app": "w"}, {"topologySpreadConstraints": cons, "affinity": aff}) for i in range(CELL_PODS)]
    if port:
        pods[3]["spec"]["containers"] = [{"name": "c", "ports": [{"containerPort": 8080, "hostPort": 8080, "protocol": "TCP"}]}]
    return nodes, [], pods


def cell_fill(cc, across, batches=1):
    """Write the counts; returns dict(term, cls: the rows, c0, t0: the cells of n00).  batches: the
    term cell leaves room for that many batches (tests/test_gpu_bounds_lifetime.py)."""
    n = CELL_PODS
    a = cc.arrays
    cls, term = class_row(cc, {"app": "w"}), term_row(cc, "PA", ZONE)
    c0 = CELL_MAX - 2 * n * batches
    t0 = CELL_MAX - 2 * n * batches + (1 if across else 0)
    idx = {name: cc.node_names.index(name) for name in CELL_NODES}
    a["term_count"][term, idx["n00"]] = t0
    a["class_count"][cls, idx["n00"]] = c0
    for z in "12":  # zones 1 and 2 hold c0 + n - 2 each, in two cells below c0
        a["class_count"][cls, idx["n%s0" % z]] = c0 - 5
        a["class_count"][cls, idx["n%s1" % z]] = n + 3
    return dict(cls=cls, term=term, c0=c0, t0=t0)


def cell_expect(fill):
    """Per pod (chosen node name, n_feasible, best_total) and the counts reached, in integers."""
    n, S = CELL_PODS, CELL_SKEW
    zone = [fill["c0"], fill["c0"] + n - 2, fill["c0"] + n - 2]
    t_z0 = fill["t0"]
    out = []
    for i in range(n):
        ok = [zone[z] + 1 - min(zone) <= S for z in range(3)]
        assert ok[0]
        skew12 = zone[1] + 1 - min(zone)
        nf = 2 * sum(ok)
        raw = [200 * zone[z] + (100 * t_z0 if z == 0 else 0) for z in range(3)]  # two identical preferred terms: class coefficient 200
        feas = [raw[z] for z in range(3) if ok[z]]
        assert max(feas) == raw[0] and max(raw) < (1 << 31)
        ipa = 100 if max(feas) > min(feas) else 0
        out.append(dict(chosen="n00", n_feasible=nf, best_total=CONST + W["ipa"] * ipa, skew12=skew12))
        zone[0] += 1
        t_z0 += 2
    assert [e["skew12"] for e in out[n - 4:n - 2]] == [S + 1, S]  # one across, then exactly maxSkew
    return out, dict(term_n00=t_z0, class_n00=zone[0])


# --------------------------------------------------------------------------------------
# sum32
# --------------------------------------------------------------------------------------
SUM_NODES, SUM_PODS = 24, 2
SUM_KEYS = [ZONE, "edge/ka", "edge/kb", "edge/kc"]
SUM_REF = 2 * 100 + 1  # two class rows at weight 100 and the hard-affinity weight on one term row


def sum32_objects():
    nodes = []
    for i in range(SUM_NODES):
        d = "d1" if i == SUM_NODES - 1 else "d0"
        nodes.append(_node("s%02d" % i, {k: d for k in SUM_KEYS}, tainted=i != 0))
    # the anchors: two classes the preferred terms select, one of them with a required affinity term
    # that matches the incoming pods (scored with the hard-affinity weight)
    ra = {"podAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"topologyKey": ZONE, "labelSelector": {"matchLabels": {"app": "p"}}}]}}
    bound = [_pod("anchor-a", {"app": "w", "tier": "a"}, {"nodeName": "s01", "affinity": ra}),
             _pod("anchor-b", {"app": "w", "tier": "b"}, {"nodeName": "s02"})]
    aff = {"podAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [_pref(k, {"app": "w"}) for k in SUM_KEYS]}}
    pods = [_pod("p%02d" % i, {"app": "p"}, {"affinity": aff}) for i in range(SUM_PODS)]
    return nodes, bound, pods


def sum32_total(across):
    """The host's `total` on the edge: the largest with MAXK * SUM_REF * total < 2^31 - 1, or one more."""
    t = (LIM32 - 1) // (MAXK * SUM_REF)
    assert MAXK * SUM_REF * t < LIM32 <= MAXK * SUM_REF * (t + 1)
    return t + (1 if across else 0)


def sum32_fill(cc, across):
    a = cc.arrays
    rows = [class_row(cc, {"app": "w", "tier": "a"}), class_row(cc, {"app": "w", "tier": "b"})]
    term = term_row(cc, "RA", ZONE)
    want = sum32_total(across) - SUM_PODS * (1 + len(SUM_KEYS))  # sum of all class counts
    have = int(a["class_count"][:, :SUM_NODES].sum())                # the anchors' own two
    d0 = [cc.node_names.index("s%02d" % i) for i in range(SUM_NODES - 1)]
    cells = [(r, i) for i in d0 for r in rows]                       # domain d0 only
    each, rest = divmod(want - have, len(cells))
    for k, (r, i) in enumerate(cells):
        a["class_count"][r, i] += each + (1 if k < rest else 0)
    assert int(a["class_count"][:, :SUM_NODES].sum()) == want
    a["term_count"][term, d0[3]] += 60000  # the hard-affinity term row, also in d0
    return dict(rows=rows, term=term, classes=want, terms=int(a["term_count"][:, :SUM_NODES].sum()))


def sum32_expect(fill):
    """Both pods: 24 feasible nodes, the untainted s00 (domain d0) chosen with the largest raw
    InterPodAffinity sum (the one node of d1 has 0), normalised to 100.  `largest`: the largest true
    32-bit intermediate (the raw sum of a d0 node for the last pod)."""
    out = []
    raw = 0
    for i in range(SUM_PODS):
        # the pods' own class (app=p) is selected by no term; their own term rows match no incoming pod
        raw = len(SUM_KEYS) * 100 * fill["classes"] + 1 * fill["terms"]
        out.append(dict(chosen="s00", n_feasible=SUM_NODES, best_total=CONST + W["ipa"] * 100))
    return out, raw


# --------------------------------------------------------------------------------------
# soft2
# --------------------------------------------------------------------------------------
SOFT_NODES, SOFT_PODS = 6, 6


def soft2_skew(n_soft, total, across):
    """The zone constraint's maxSkew on the edge: the largest with the bound inside, or one more."""
    def inside(k):
        return spread_bounds(dict(ref_weight=1, max_soft=n_soft, max_skew=k), total, 0, SOFT_NODES)[0]
    k = LIM32 // n_soft
    while not inside(k):
        k -= 1
    assert inside(k) and not inside(k + 1)
    return k + (1 if across else 0)


def soft2_total():
    return 40 + SOFT_PODS  # forty bound pods of the selected class, one own commit per pod (no own term rows)


def soft2_objects(n_soft, across):
    nodes = [_node(n, {ZONE: "z" + n[1], "edge/rack": "r" + n[1:]}, tainted=False) for n in CELL_NODES]
    sel = {"matchLabels": {"app": "w"}}
    keys = [ZONE, HOST, "edge/rack", ZONE][:n_soft]
    skews = [soft2_skew(n_soft, soft2_total(), across), 1, 2, 3][:n_soft]
    cons = [{"maxSkew": s, "topologyKey": k, "whenUnsatisfiable": "ScheduleAnyway", "labelSelector": sel}
            for k, s in zip(keys, skews)]
    pods = [_pod("w%02d" % i, {"app": "w"}, {"topologySpreadConstraints": cons}) for i in range(SOFT_PODS)]
    return nodes, [], pods


def soft2_fill(cc):
    a = cc.arrays
    cls = class_row(cc, {"app": "w"})
    for name, v in zip(CELL_NODES, [13, 0, 9, 7, 1, 10]):
        a["class_count"][cls, cc.node_names.index(name)] = v
    assert int(a["class_count"][:, :SOFT_NODES].sum()) == 40
    return dict(cls=cls)
