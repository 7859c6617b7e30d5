"""Clusters at the edges of the fast kernels' exact-arithmetic envelope (test infrastructure).

k_simple (all its forms), k_spread and the service's k_simple-shaped chain replace the reference's
Go int64 and IEEE float64 divisions by integers held in doubles, one reciprocal per node and a +-1
correction (csrc/kss_fastmath.cuh; least_bf, dyn_eval_def, dyn_eval of csrc/kss_simple.cuh).  That is
exact only while every allocatable is below 2^46, every Fit weight below 2^20, every pod request
below 2^52 and max Requested + n_pods * max commit below 2^52.  This module builds clusters whose
operands sit on those edges, and states what the reference computes there with Python integers
(`//`) and correctly rounded `int / int` divisions only -- no oracle, no numpy.

The twin cluster: operand case j is a pair of identical nodes a<j>, b<j>; b<j> carries a
PreferNoSchedule taint; pod j names both through NodeAffinity matchFields (one metadata.name In [x]
requirement per term).  Two feasible nodes make the pod scored, a<j> wins by 100 * the
TaintToleration weight, and best_total minus the constant part is a<j>'s weighted Fit and
BalancedAllocation scores -- observable from the compact kernels, which keep no per-node record.

Operand classes (classify / pair_classes), per (capacity, requested-with-the-pod) of one resource:
  cap_special  the capacity is one of SPECIAL_CAPS (2^46-1, 2^46-2, 2^45+1, 3*2^44-1, all-ones
               mantissas, small primes)
  on / below / above   x = (capacity - requested) * 100 is k * capacity, within 100 below it, within
               100 above it (1 <= k <= 99)
  full         requested == capacity (score 0, fraction 1)
  over         requested > capacity (overcommitted node: score 0, fraction clipped to 1)
  cap0         capacity 0 (the resource drops out of both scores)
  est_low      the first estimate (int)(x * RN(1 / capacity)) is floor(x / capacity) - 1: the +1
               correction of quot_small_d / least_bf must run (x = k * capacity exactly, where
               RN(1 / capacity) fell below the reciprocal)
  est_high     the first estimate is floor(x / capacity) + 1: the -1 correction must run (x one below
               k * capacity at a capacity near 2^46, where RN(1 / capacity) lies above the reciprocal;
               7 in 10^6 random operands of this shape, so they are searched for)
  near_bound   Requested within a few units of 2^52 - n_pods * max commit, the f64_exact bound
and per (cpu, memory) pair of fractions:
  ba_equal     equal fractions (deviation 0)
  ba_exact     different fractions whose (1 - sd) * 100 is an exact integer (halves and quarters)
"""
import math
from fractions import Fraction

CPU, MEM, EPH = 0, 1, 2
DEFAULT_NZ = (100, 200 * 1024 * 1024)  # schedutil.DefaultMilliCPURequest / DefaultMemoryRequest
ALLOWED_PODS = 110

E46, E52, E53 = 1 << 46, 1 << 52, 1 << 53
ALL_ONES = [(1 << k) - 1 for k in (13, 24, 31, 40, 45)]
SMALL_PRIMES = [3, 7, 97, 101, 257, 1009]
SPECIAL_CAPS = [E46 - 1, E46 - 2, (1 << 45) + 1, 3 * (1 << 44) - 1] + ALL_ONES + SMALL_PRIMES
# divisible by 100 (2^46 = 64 mod 100) and by 4: every k * capacity / 100 and every quarter is an integer
ROUND_CAPS = [E46 - 64, E46 - 164, 3 * (1 << 44) - 48, (1 << 45) + 68, 4 * 25 * 1009, 100 * 257]
assert all(c % 100 == 0 for c in ROUND_CAPS)
CLASSES = ("cap_special", "on", "below", "above", "full", "over", "cap0", "est_low", "est_high", "near_bound")
PAIR_CLASSES = ("ba_equal", "ba_exact")


# --------------------------------------------------------------------------------------
# exact arithmetic
# --------------------------------------------------------------------------------------
def first_estimate(x, cap):
    """(int)(x * RN(1 / cap)) as the kernels form it (doubles; Python's float operations are IEEE)."""
    return int(float(x) * (1.0 / float(cap)))


def classify(cap, requested):
    """The classes of one operand: the capacity and Requested (NonZeroRequested for cpu / memory)
    with the pod's own request added, as the Fit score reads them."""
    out = set()
    if cap == 0:
        return {"cap0"}
    if cap in SPECIAL_CAPS:
        out.add("cap_special")
    if requested > cap:
        out.add("over")
        return out
    if requested == cap:
        out.add("full")
        return out
    x = (cap - requested) * 100
    k, rem = divmod(x, cap)
    if 1 <= k <= 99 and rem == 0:
        out.add("on")
    if 1 <= k <= 99 and 0 < rem <= 100:
        out.add("above")
    if 0 <= k <= 98 and 0 < cap - rem <= 100:
        out.add("below")
    if first_estimate(x, cap) == k - 1:
        out.add("est_low")
    if first_estimate(x, cap) == k + 1:
        out.add("est_high")
    assert first_estimate(x, cap) in (k - 1, k, k + 1)
    return out


def pair_classes(cap0, r0, cap1, r1):
    if cap0 == 0 or cap1 == 0:
        return set()
    f0, f1 = min(Fraction(r0, cap0), 1), min(Fraction(r1, cap1), 1)
    if f0 == f1:
        return {"ba_equal"}
    if ((1 - abs(f0 - f1) / 2) * 100).denominator == 1:
        return {"ba_exact"}
    return set()


def least_or_most(strategy, requested, cap):
    """leastRequestedScore / mostRequestedScore (noderesources/least_allocated.go, most_allocated.go)."""
    if cap == 0:
        return 0
    if strategy == "most":
        return min(requested, cap) * 100 // cap
    return 0 if requested > cap else (cap - requested) * 100 // cap


def exact_scores(prof, cap, req, nz, sreq, snz):
    """(NodeResourcesFit score, BalancedAllocation score) of one node for one pod under profile
    description `prof` (PROFILES): cap / req [3] the node's Allocatable and Requested, nz [2] its
    NonZeroRequested, sreq / snz [3] the pod's requests without and with the non-zero defaults.
    Fit by //, the fractions by int / int, the deviation and the truncation in the order of
    balancedResourceScorer (balanced_allocation.go)."""
    score = wsum = 0
    for r, w in prof["fit"]:
        if cap[r] == 0:
            continue
        base = nz[r] if r < 2 else req[r]
        score += least_or_most(prof["strategy"], base + snz[r], cap[r]) * w
        wsum += w
    fit = score // wsum if wsum else 0
    fr = []
    total = 0.0
    for r in prof["ba"]:
        if cap[r] == 0:
            continue
        # float64(requested) / float64(capacity): below 2^53 both convert exactly and this is int / int,
        # the correctly rounded quotient; above (k_schedule's range) the reference rounds the operands first
        f = float(req[r] + sreq[r]) / float(cap[r])
        f = 1.0 if f > 1 else f
        total += f
        fr.append(f)
    sd = 0.0
    if len(fr) == 2:
        sd = abs((fr[0] - fr[1]) / 2)
    elif len(fr) > 2:
        mean = total / float(len(fr))
        s = 0.0
        for f in fr:
            s = s + (f - mean) * (f - mean)
        sd = math.sqrt(s / float(len(fr)))
    return fit, int((1 - sd) * 100.0)


# --------------------------------------------------------------------------------------
# profiles (descriptions; make_profile builds the ABI struct)
# --------------------------------------------------------------------------------------
def _prof(strategy="least", fit=((CPU, 1), (MEM, 1)), ba=(CPU, MEM), w_fit=1, w_ba=1):
    return dict(strategy=strategy, fit=tuple(fit), ba=tuple(ba), w_tt=3, w_pts=2, w_fit=w_fit, w_ba=w_ba)


FIT_WEIGHT_LIMIT = 1 << 20
PROFILES = {
    "default": _prof(),
    "least124": _prof(fit=((CPU, 1), (MEM, 2), (EPH, 4))),                  # weight sum 7: small_div
    "most124": _prof(strategy="most", fit=((CPU, 1), (MEM, 2), (EPH, 4))),
    "ba3": _prof(ba=(CPU, MEM, EPH)),                                        # the sqrt branch
    "least124_ba3": _prof(fit=((CPU, 1), (MEM, 2), (EPH, 4)), ba=(CPU, MEM, EPH), w_fit=2, w_ba=3),
    "w_inside": _prof(fit=((CPU, FIT_WEIGHT_LIMIT - 1), (MEM, FIT_WEIGHT_LIMIT - 3), (EPH, 5))),
    "w_outside": _prof(fit=((CPU, FIT_WEIGHT_LIMIT), (MEM, FIT_WEIGHT_LIMIT - 3), (EPH, 5))),
}


def is_default(prof):
    return prof == PROFILES["default"]


def make_profile(prof):
    """The kss_profile of a description (the default profile with the Fit / BalancedAllocation
    arguments and the two plugin weights replaced)."""
    from kss import abi
    p = abi.default_profile()
    if is_default(prof):
        return p
    p.fit_strategy = abi.KSS_FIT_MOST_ALLOCATED if prof["strategy"] == "most" else abi.KSS_FIT_LEAST_ALLOCATED
    p.fit_n = len(prof["fit"])
    for i in range(4):
        p.fit_res[i], p.fit_weight[i] = (prof["fit"][i] if i < p.fit_n else (0, 0))
    p.ba_n = len(prof["ba"])
    for i in range(4):
        p.ba_res[i] = prof["ba"][i] if i < p.ba_n else 0
    p.weight[abi.KSS_S_NODE_RESOURCES_FIT] = prof["w_fit"]
    p.weight[abi.KSS_S_BALANCED_ALLOCATION] = prof["w_ba"]
    return p


# --------------------------------------------------------------------------------------
# operand search
# --------------------------------------------------------------------------------------
def _search_caps():
    caps = list(SPECIAL_CAPS[:4]) + ALL_ONES[2:]
    for base in (E46, 3 * (1 << 44), 1 << 45, (1 << 46) - (1 << 40)):
        caps += [base - 1 - 2 * i for i in range(1, 20)]
    return caps


def _round_search_caps():
    # multiples of 100 with full mantissas (a Weyl sequence below 2^46).  The estimate is one too low
    # only at x = k * cap exactly, where RN(1 / cap) fell below 1 / cap and the product rounds down:
    # a remainder of 100 already lifts x * inv above k by 2^-40, far more than the reciprocal's error.
    return [E46 - 64 - 100 * ((i * 0x9E3779B97F4A7C15) % (1 << 38)) for i in range(1, 40)]


def x_operands():
    """{class: [(cap, requested)]} for on / below / above / est_low, by search over capacities at
    the top of the envelope and k = 1 .. 99: requested = cap - x / 100 with x the multiple of 100
    at, just below and just above k * cap."""
    out = {"on": [], "below": [], "above": [], "est_low": [], "est_high": []}
    for cap in ROUND_CAPS:
        for k in (1, 33, 50, 67, 99):
            out["on"].append((cap, cap - k * cap // 100))
    for cap in ROUND_CAPS + _round_search_caps():
        for k in range(1, 100):
            if first_estimate(k * cap, cap) == k - 1:
                out["est_low"].append((cap, cap - k * cap // 100))
    for i in range(1, 4000):  # odd capacities just below 2^46; the k with k * cap = 1 (mod 100), if any
        cap = E46 - 1 - 2 * ((i * 0x9E3779B97F4A7C15) % (1 << 40))
        for k in range(1, 100):
            if k * cap % 100 == 1 and first_estimate(k * cap - 1, cap) == k:
                out["est_high"].append((cap, cap - (k * cap - 1) // 100))
    for cap in _search_caps():
        for k in range(1, 100):
            t = k * cap
            lo, hi = t // 100 * 100, -(-t // 100) * 100
            if lo == t:
                lo, hi = t - 100, t + 100
            if len(out["below"]) < 400 and k % 7 == 3:
                out["below"].append((cap, cap - lo // 100))
            if k % 7 == 5:
                out["above"].append((cap, cap - hi // 100))
    for k, v in out.items():
        for cap, r in v:
            assert k in classify(cap, r), (k, cap, r)
    return out


def small_div_operands(n_div=3000):
    """(x, d) for small_div: x in {k d - 1, k d, k d + 1} for k <= 100, over n_div divisors up to
    3 * 2^20 (the normalisation maxima and Fit weight sums the envelope admits), x < 2^31."""
    ds = list(range(1, 130)) + [(1 << k) + e for k in range(7, 22) for e in (-1, 0, 1)] + [3 << 20, (3 << 20) - 1]
    step = ((3 << 20) - 200) // max(n_div - len(ds), 1)
    d = 131
    while len(ds) < n_div:
        ds.append(d)
        d += step | 1
    out = []
    for d in ds:
        for k in range(0, 101):
            for e in (-1, 0, 1):
                x = k * d + e
                if 0 <= x < (1 << 31) and x <= 100 * d + 1:
                    out.append((x, d))
    return out


# --------------------------------------------------------------------------------------
# cases and clusters
# --------------------------------------------------------------------------------------
POD_SIZES = [(1, 1, 1), (7, 1000, 3), (250, 1 << 30, 1 << 20), ((1 << 43) - 1, (1 << 43) - 1, (1 << 43) - 1),
             (1009, (1 << 31) + 1, 0)]
SAME_SHAPE = (250, 1 << 30, 1 << 20)


def _case(name, ops, pod, second=True):
    """ops: three (cap, requested-with-the-pod); pod: the pod's three requests.  The node's own
    Requested is the difference."""
    cap = [c for c, _ in ops]
    req = [r - p for (_, r), p in zip(ops, pod)]
    assert all(v >= 0 for v in req), (name, ops, pod)
    return dict(name=name, cap=cap, req=req, pod=list(pod), second=second)


def make_cases(n_pairs=64, same_shape=False, n_pods_bound=None):
    """n_pairs (>= 64) operand cases covering every class at least 8 times.  same_shape: every pod
    with requests carries SAME_SHAPE (the adversity is in the nodes' allocatables and bound pods);
    the best-effort pods of the overcommitted nodes and the two kinds of pods of the cap0 nodes are
    the other three shapes.  n_pods_bound: the pod count the near_bound operands are computed for
    (default: two pods per pair)."""
    assert n_pairs >= 64
    xo = x_operands()
    cases = []
    zero = (0, 0, 0)

    def add(name, ops, i):
        p = SAME_SHAPE if same_shape else POD_SIZES[i % len(POD_SIZES)]
        if not same_shape:
            p = tuple(min(q, r) for (_, r), q in zip(ops, p))
        cases.append(_case(name, ops, p))

    def pick(lst, i):
        ok = [o for o in lst if all(o[1] >= s for s in SAME_SHAPE)]
        return ok[(i * 37) % len(ok)]

    # x on / below / above a multiple of the capacity, and the estimate one off: on every resource
    for cls in ("on", "below", "above", "est_low", "est_high"):
        for i in range(4):
            add("%s-%d" % (cls, i), [pick(xo[cls], 3 * i), pick(xo[cls], 3 * i + 1), pick(xo[cls], 3 * i + 2)], i)
    # special capacities at assorted fills
    sp = SPECIAL_CAPS if not same_shape else SPECIAL_CAPS[:4] + ALL_ONES[3:]
    for i in range(8):
        c = [sp[i % len(sp)], sp[(i + 1) % len(sp)], sp[(i + 2) % len(sp)]]
        add("special-%d" % i, [(c[r], max(c[r] * (i + 1) // 11, SAME_SHAPE[r] if same_shape else 0)) for r in range(3)], i)
    # requested == capacity: one resource in turn, then all three
    for i in range(5):
        c = [SPECIAL_CAPS[i % 4], ROUND_CAPS[i % 2], ALL_ONES[3 + i % 2]]
        add("full-%d" % i, [(c[r], c[r] if r == i or i >= 3 else c[r] // 2) for r in range(3)], i)
    # overcommitted nodes: only a best-effort pod passes NodeResourcesFit there (fitsRequest of v1.26
    # compares every resource once the pod requests anything)
    for i in range(5):
        c = [SPECIAL_CAPS[i % 4], SPECIAL_CAPS[(i + 1) % 4], ALL_ONES[3]]
        over = [c[r] + 1 + (i << (4 * r)) if (r == i or i >= 3) else c[r] // 3 for r in range(3)]
        cases.append(_case("over-%d" % i, list(zip(c, over)), zero))
    # capacity 0: cpu and ephemeral-storage (the pod requests neither), then one of them
    for i in range(5):
        big = ROUND_CAPS[i % 2]
        no_cpu, no_eph = i != 4, i != 3
        p = (0 if no_cpu else SAME_SHAPE[0], SAME_SHAPE[1] if same_shape else 1 + i, 0 if no_eph else SAME_SHAPE[2])
        if same_shape and not (no_cpu and no_eph):
            continue  # (each would be a fifth and sixth pod shape)
        ops = [(0, 0) if no_cpu else (SPECIAL_CAPS[2], SPECIAL_CAPS[2] // 5), (big, big // 4 + p[1]),
               (0, 0) if no_eph else (E46 - 1, (E46 - 1) // 2)]
        cases.append(_case("cap0-%d" % i, ops, p))
    if same_shape:
        for i in range(5, 7):
            big = ROUND_CAPS[i % 2]
            cases.append(_case("cap0-%d" % i, [(0, 0), (big, big // 5 + SAME_SHAPE[1]), (0, 0)], (0, SAME_SHAPE[1], 0)))
    # BalancedAllocation: equal fractions; halves and quarters
    for i in range(8):
        c0, c1 = ROUND_CAPS[i % 4], ROUND_CAPS[(i + 1) % 4] if i % 3 else ROUND_CAPS[i % 4]
        num = (1, 2, 3, 4)[i % 4]
        add("ba-equal-%d" % i, [(c0, c0 * num // 4), (c1, c1 * num // 4), (c0, c0 * num // 4)], i)
    for i, (a, b) in enumerate([(4, 2), (3, 1), (2, 4), (1, 3), (4, 2), (3, 1), (2, 4), (1, 3)]):
        c0, c1 = ROUND_CAPS[i % 4], ROUND_CAPS[(i + 1) % 4]
        add("ba-exact-%d" % i, [(c0, c0 * a // 4), (c1, c1 * b // 4), (c1, c1 // 4)], i)
    # fill up with more operands whose first estimate is one too low
    i = 0
    while len(cases) < n_pairs - 4:
        add("est-low-more-%d" % i, [pick(xo["est_low"], 40 + 3 * i), pick(xo["est_low"], 41 + 3 * i), pick(xo["above"], 5 * i)], i)
        i += 1
    assert len(cases) == n_pairs - 4
    # Requested near the f64_exact bound 2^52 - n_pods * max commit: overcommitted, best-effort pods
    n_pods = n_pods_bound if n_pods_bound is not None else 2 * n_pairs
    commit = max(max(max(c["pod"]) for c in cases), DEFAULT_NZ[1])
    for i in range(4):
        top = E52 - 1 - n_pods * commit - 3 * i
        ops = [(SPECIAL_CAPS[i % 4], top if i % 3 == 0 else 5), (SPECIAL_CAPS[(i + 1) % 4], top if i % 3 else 9), (E46 - 1, top - 1)]
        cases.append(_case("near-bound-%d" % i, ops, zero))
    return cases


def operands_of(cases, n_pods):
    """([class set] of every single-resource operand, [class set] of every (cpu, memory) pair), as
    the first pod of each case meets them in a batch of n_pods pods."""
    single, pairs = [], []
    commit = max(max(max(c["pod"]) for c in cases), DEFAULT_NZ[1])
    for c in cases:
        has = any(c["req"])
        rq = [c["req"][r] + c["pod"][r] for r in range(3)]
        nzq = [_nz(c["req"], r, has) + (c["pod"][r] or DEFAULT_NZ[r]) for r in range(2)] + [rq[2]]
        for r in range(3):
            k = classify(c["cap"][r], nzq[r])
            if c["req"][r] + n_pods * commit >= E52 - 64:
                k.add("near_bound")
            single.append(k)
        pairs.append(pair_classes(c["cap"][0], rq[0], c["cap"][1], rq[1]))
    return single, pairs


def _nz(req, r, has_pod):
    return 0 if not has_pod else (req[r] or DEFAULT_NZ[r])


def _q(r, v):
    return "%dm" % v if r == CPU else "%d" % v


def _requests(v):
    return {k: _q(r, v[r]) for r, k in enumerate(("cpu", "memory", "ephemeral-storage")) if v[r]}


def twin_cluster(cases, second=False, spread=False, ports=(), images=(), volumes=()):
    """(nodes, bound, pods) of the twin cluster.  second: a second, identical pod per pair right
    after the first, evaluated on the state its predecessor's commit left.  spread: every pod also
    carries one soft PodTopologySpread constraint over the per-pair label (both twins in one domain).
    ports / images / volumes: indices of cases whose pods also hold a host port / name a node-cached
    image / mount an inline EBS volume of their own."""
    nodes, bound, pods = [], [], []
    for j, c in enumerate(cases):
        for t in "ab":
            name = "%s%03d" % (t, j)
            n = {"metadata": {"name": name, "labels": {"kubernetes.io/hostname": name, "pair": "p%03d" % j}},
                 "spec": {}, "status": {"allocatable": {"cpu": _q(CPU, c["cap"][0]), "memory": _q(MEM, c["cap"][1]),
                                                        "ephemeral-storage": _q(EPH, c["cap"][2]), "pods": str(ALLOWED_PODS)}}}
            if t == "b":
                n["spec"]["taints"] = [{"key": "twin", "value": "b", "effect": "PreferNoSchedule"}]
            if j in images:
                n["status"]["images"] = [{"names": ["registry.example/app:v1"], "sizeBytes": 500 * 1024 * 1024}]
            nodes.append(n)
            if any(c["req"]):
                bound.append({"metadata": {"name": "bound-" + name, "namespace": "default", "labels": {"app": "bound"}},
                              "spec": {"nodeName": name,
                                       "containers": [{"name": "c", "resources": {"requests": _requests(c["req"])}}]}})
        for k in range(2 if second and c["second"] else 1):
            ctr = {"name": "c", "resources": {"requests": _requests(c["pod"])}}
            if j in ports:
                ctr["ports"] = [{"containerPort": 8080, "hostPort": 8000 + j % 7, "protocol": "TCP"}]
            if j in images:
                ctr["image"] = "registry.example/app:v1"
            terms = [{"matchFields": [{"key": "metadata.name", "operator": "In", "values": ["%s%03d" % (t, j)]}]} for t in "ab"]
            spec = {"containers": [ctr],
                    "affinity": {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": terms}}}}
            if j in volumes:
                spec["volumes"] = [{"name": "v0", "awsElasticBlockStore": {"volumeID": "vol-%03d-%d" % (j, k)}}]
            if spread:
                spec["topologySpreadConstraints"] = [{"maxSkew": 1, "topologyKey": "pair", "whenUnsatisfiable": "ScheduleAnyway",
                                                      "labelSelector": {"matchLabels": {"app": "twin"}}}]
            pods.append({"metadata": {"name": "pod-%03d-%d" % (j, k), "namespace": "default", "labels": {"app": "twin"}},
                         "spec": spec})
    return nodes, bound, pods


def pod_cases(cases, second=False):
    """The case index of every pod of twin_cluster(cases, second), in pod order."""
    return [j for j, c in enumerate(cases) for _ in range(2 if second and c["second"] else 1)]


def expect_twins(cases, prof, second=False):
    """What the reference decides for every pod of twin_cluster(cases, second) under `prof`, from
    exact arithmetic alone: per pod a dict(case, chosen ("a" / "b" / None), n_feasible, scored,
    best_total, a=(fit, ba), b=(fit, ba)) -- the scores of both twins on the state the pod meets."""
    out = []
    for j, c in enumerate(cases):
        has = any(c["req"])
        st = {t: dict(req=list(c["req"]), nz=[_nz(c["req"], 0, has), _nz(c["req"], 1, has)], pods=int(has)) for t in "ab"}
        sreq = c["pod"]
        snz = [c["pod"][0] or DEFAULT_NZ[0], c["pod"][1] or DEFAULT_NZ[1], c["pod"][2]]
        for _ in range(2 if second and c["second"] else 1):
            feas, sc = {}, {}
            for t in "ab":
                s = st[t]
                ok = s["pods"] + 1 <= ALLOWED_PODS
                if any(sreq):
                    ok = ok and all(sreq[r] <= c["cap"][r] - s["req"][r] for r in range(3))
                feas[t] = ok
                sc[t] = exact_scores(prof, c["cap"], s["req"], s["nz"], sreq, snz)
            nf = int(feas["a"]) + int(feas["b"])
            chosen = "a" if feas["a"] else ("b" if feas["b"] else None)
            total = None
            if nf == 2:
                total = 100 * prof["w_tt"] + 100 * prof["w_pts"] + prof["w_fit"] * sc["a"][0] + prof["w_ba"] * sc["a"][1]
                assert total > prof["w_fit"] * sc["b"][0] + prof["w_ba"] * sc["b"][1] + 100 * prof["w_pts"]
            out.append(dict(case=j, chosen=chosen, n_feasible=nf, scored=int(nf > 1), best_total=total, a=sc["a"], b=sc["b"]))
            if chosen:
                s = st[chosen]
                for r in range(3):
                    s["req"][r] += sreq[r]
                s["nz"][0] += snz[0]
                s["nz"][1] += snz[1]
                s["pods"] += 1
    return out


# --------------------------------------------------------------------------------------
# the bounds, one value moved across each
# --------------------------------------------------------------------------------------
def bound_cases(n_pairs=64, second=False):
    """{name: (cases, profile name)} -- for three of the four bounds a fixture just inside and one
    just across (one unit more), everything else equal:
      alloc      a cpu allocatable of 2^46 - 1 / 2^46
      weight     a Fit weight of 2^20 - 1 / 2^20
      sum        max Requested + n_pods * max commit = 2^52 - 1 / 2^52
    (request_bound_cases: the fourth.)"""
    n_pods = (2 if second else 1) * n_pairs
    base = make_cases(n_pairs, n_pods_bound=n_pods)
    j = next(i for i, c in enumerate(base) if c["name"] == "special-0")
    k = next(i for i, c in enumerate(base) if c["name"] == "near-bound-0")
    assert base[j]["cap"][0] == E46 - 1
    assert f64_sum(base, n_pods) == (E52 - 1, E52 - 1)
    out = {}
    for tag in ("in", "out"):
        c = dict(base[j])
        c["cap"] = [E46 - 1 if tag == "in" else E46] + c["cap"][1:]
        out["alloc-" + tag] = (base[:j] + [c] + base[j + 1:], "default")
        out["weight-" + tag] = (base, "w_inside" if tag == "in" else "w_outside")
        c = dict(base[k])  # near-bound-0 holds the largest Requested (cpu)
        c["req"] = [c["req"][0] + (tag == "out")] + c["req"][1:]
        out["sum-" + tag] = (base[:k] + [c] + base[k + 1:], "default")
    return out


def f64_sum(cases, n_pods):
    """(max Requested + n_pods * max commit, the same for NonZeroRequested), the two sums the host
    keeps below 2^52 (f64_exact in kss_lib.hip)."""
    mreq = max(max(c["req"]) for c in cases)
    mnz = max(max(_nz(c["req"], r, any(c["req"])) for r in range(2)) for c in cases)
    creq = max(max(c["pod"]) for c in cases)
    cnz = max(max(c["pod"][r] or DEFAULT_NZ[r] for r in range(2)) for c in cases)
    return mreq + n_pods * creq, mnz + n_pods * cnz


def lifetime_cases(n_pairs=64, batches=1):
    """make_cases whose near-bound operands are computed for `batches` batches of one pod per pair on
    one context: max Requested + batches * n_pairs * max commit = 2^52 - 1 (and the same for
    NonZeroRequested).  batches=1 is bound_cases' sum-in.  The best-effort pods of the near-bound
    pairs do land there and raise NonZeroRequested by the defaults, so after one batch the true
    maximum plus n_pairs * max commit is across 2^52 for batches=1 and inside it for batches=2."""
    cases = make_cases(n_pairs, n_pods_bound=batches * n_pairs)
    assert f64_sum(cases, batches * n_pairs) == (E52 - 1, E52 - 1)
    return cases


def renamed(pods, suffix):
    """Copies of pods under other names (a second batch of the same shapes)."""
    out = []
    for p in pods:
        q = dict(p)
        q["metadata"] = dict(p["metadata"], name=p["metadata"]["name"] + suffix)
        out.append(q)
    return out


# The wrong-value witness: one pair whose cpu Requested is odd and near 2^51 on nodes far too small for
# it, and one pod whose cpu request is odd and near 2^51.  Under a profile without the
# NodeResourcesFit filter the pod lands on a<0> every time; Requested + commit is 2^52 - 2 for the
# first pod (inside the sum bound) and passes 2^53 on an odd value with the fourth.
WITNESS_REQ, WITNESS_POD = (1 << 51) - 3, (1 << 51) + 1


def witness_cases():
    ops = [(E46 - 1, WITNESS_REQ + WITNESS_POD), (E46 - 1, 1000 + 7), (E46 - 1, 3 + 3)]
    cases = [_case("witness", ops, (WITNESS_POD, 7, 3))]
    assert f64_sum(cases, 1) == (E52 - 2, E52 - 2)
    return cases


def witness_requested(runs):
    """cpu Requested of a<0> after `runs` one-pod batches, in Python integers."""
    return WITNESS_REQ + runs * WITNESS_POD


assert witness_requested(4) > E53 and witness_requested(4) % 2 == 1


def request_bound_cases(inside):
    """One empty pair and one pod whose memory request is 2^52 - 1 (inside) or 2^52 (across).  Only a
    batch of one pod on nodes without bound pods keeps the sum bound beside such a request; the pod
    fits nowhere (0 feasible nodes) either way."""
    return [_case("request", [(4000, 100), (1 << 33, E52 - 1 if inside else E52), (1 << 34, 0)],
                  (100, E52 - 1 if inside else E52, 0))]


def above_cases():
    """Pairs above the envelope (k_schedule only): allocatables from 2^46 to 2^56 - 1 (beyond that
    requested * 100 leaves int64), at fills that put (capacity - requested) * 100 on both sides of
    2^53 -- where div_i64 (kss_eval.cuh) changes from the f64 division to the integer division -- and
    at assorted hundredths."""
    caps = [E46, (1 << 47) + 1, (1 << 50) - 1, E53 // 100 + 5, E53 - 1, E53, E53 + 1, (1 << 55) + 3, (1 << 56) - 1]
    cases = []
    for i, cap in enumerate(caps):
        c2 = caps[(i + 3) % len(caps)]
        for n, d in enumerate((E53 // 100 - 1, E53 // 100, E53 // 100 + 1, E53 // 100 + 2)):
            if d > cap or d > c2:
                continue
            ops = [(cap, cap - d), (c2, c2 - (d + 1 - n)), (E46 - 1, E46 // 3)]
            cases.append(_case("step-%d-%d" % (i, n), ops, [min(q, r) for (_, r), q in zip(ops, POD_SIZES[(i + n) % 3])]))
        for k in (0, 1, 37, 99):
            ops = [(cap, cap - k * cap // 100), (c2, c2 * (k + 1) // 101), (1 << 48, 1 << 40)]
            cases.append(_case("fill-%d-%d" % (i, k), ops, [min(q, r) for (_, r), q in zip(ops, POD_SIZES[(i + k) % 3])]))
    return cases


# --------------------------------------------------------------------------------------
# contests: the choice itself depends on the correction (for paths that report only chosen nodes)
# --------------------------------------------------------------------------------------
CONTEST_POD = (3, 1000, 7)


def contest_cluster(n=12):
    """(nodes, bound, pods, expect): 2 n untainted node pairs x<j>, y<j> of equal allocatables and one
    pod per pair naming both.  In the first n pairs the lower-indexed node meets an est_low operand
    on every resource (x = k * capacity exactly) and the other the same with Requested one less: the
    exact scores tie and selectHost keeps the lower index; a quotient left one too low loses the tie.
    In the last n the HIGHER-indexed node meets an est_high operand (x = k * capacity - 1) and the
    lower-indexed one Requested one more: again a tie in exact arithmetic, which an estimate left
    one too high wins.  expect: per pod the winner's name and both nodes' exact (fit, ba) under the
    default profile."""
    xo = x_operands()
    nodes, bound, pods, expect = [], [], [], []
    for j in range(2 * n):
        low = j < n
        ops = [xo["est_low" if low else "est_high"][(5 * j + 11 * r) % 100] for r in range(3)]
        cap = [c for c, _ in ops]
        R = [r for _, r in ops]
        # (node name, Requested with the pod) in index order; the first is the exact winner of a tie
        pair = [("x%03d" % j, R), ("y%03d" % j, [v - 1 for v in R])] if low else \
               [("x%03d" % j, [v + 1 for v in R]), ("y%03d" % j, R)]
        sc = []
        for name, rq in pair:
            req = [v - p for v, p in zip(rq, CONTEST_POD)]
            nodes.append({"metadata": {"name": name, "labels": {"kubernetes.io/hostname": name}}, "spec": {},
                          "status": {"allocatable": {"cpu": _q(CPU, cap[0]), "memory": _q(MEM, cap[1]),
                                                     "ephemeral-storage": _q(EPH, cap[2]), "pods": str(ALLOWED_PODS)}}})
            bound.append({"metadata": {"name": "bound-" + name, "namespace": "default", "labels": {"app": "bound"}},
                          "spec": {"nodeName": name, "containers": [{"name": "c", "resources": {"requests": _requests(req)}}]}})
            sc.append({p: exact_scores(PROFILES[p], cap, req, req[:2], list(CONTEST_POD), list(CONTEST_POD)) for p in PROFILES})
        terms = [{"matchFields": [{"key": "metadata.name", "operator": "In", "values": [name]}]} for name, _ in pair]
        pods.append({"metadata": {"name": "contest-%03d" % j, "namespace": "default", "labels": {"app": "contest"}},
                     "spec": {"containers": [{"name": "c", "resources": {"requests": _requests(CONTEST_POD)}}],
                              "affinity": {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": terms}}}}})
        expect.append(dict(names=[name for name, _ in pair], scores=sc, kind="est_low" if low else "est_high"))
    return nodes, bound, pods, expect


def contest_winner(e, pname):
    """The reference's choice of one contest under a profile: the higher weighted total, the lower
    index on a tie; and whether it is a tie."""
    prof = PROFILES[pname]
    t = [prof["w_fit"] * s[pname][0] + prof["w_ba"] * s[pname][1] for s in e["scores"]]
    return e["names"][1 if t[1] > t[0] else 0], t[0] == t[1]
