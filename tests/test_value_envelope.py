"""The references and the host planning at the edges of the fast kernels' exact-arithmetic envelope
(tests/value_edge_fixtures.py); no GPU.

  * both oracles agree on every fixture, and the C oracle's per-node raw NodeResourcesFit and
    BalancedAllocation scores equal exact arithmetic (Python // and int / int) under every profile;
  * every twin pod is scored, chooses a<j>, and its best_total decodes to a<j>'s exact scores --
    what makes the compact kernels' arithmetic observable in tests/test_gpu_value_envelope.py;
  * the fixtures hold what they claim: at least 8 operands of every class, among them 8 whose first
    f64 estimate is one too low and 8 where it is one too high, and a small_div operand set that needs either correction under
    some reciprocal within 1 ulp of the correctly rounded one;
  * kss_plan_sweep demotes with the values reason, and the scenario's index, exactly across each of
    the four bounds, while kss_plan_podset / kss_plan_service keep answering "eligible" there: their
    documented contract leaves values to the launch.

The first f64 estimate is one too low at about one operand in a thousand of the shape x = 100 m
near k * A, and one too HIGH at 7 in 10^6 (x = k * A - 1 with A near 2^46): both are reachable,
the fixtures search for them, and both are among the asserted classes (est_low, est_high)."""
import collections

import numpy as np
import pytest

import crosscheck
import oracle_c
import value_edge_fixtures as vx
from kss import abi, native
from kss.compile import compile_cluster

VALUES_REASON = "a scenario's values or the profile's weights leave the exact f64 envelope: the whole sweep runs on k_schedule"
N_PAIRS = 64
FIXTURES = {
    "twin": dict(),
    "second": dict(second=True),
    "same-shape": dict(same_shape=True, second=True),
    "spread": dict(spread=True),
}
_CACHE = {}


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def fixture(name):
    """(cases, nodes, bound, pods, cc, cp) of one fixture, built once (nothing writes to them)."""
    if name not in _CACHE:
        kw = dict(FIXTURES[name])
        cases = vx.make_cases(N_PAIRS, same_shape=kw.pop("same_shape", False))
        nodes, bound, pods = vx.twin_cluster(cases, **kw)
        cc, cp, _ = compile_cluster(nodes, bound, pods)
        _CACHE[name] = (cases, nodes, bound, pods, cc, cp)
    return _CACHE[name]


def oracle(cc, cp, prof):
    return oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record=True,
                             n_classes=len(cc.classes), n_terms=len(cc.terms))


def check_against_exact(cases, cc, cp, desc, second, ch, res):
    """Every pod of a twin fixture against expect_twins: outcome, choice, best_total and both twins'
    raw Fit / BalancedAllocation scores.  Returns the number of scored pods."""
    exp = vx.expect_twins(cases, desc, second)
    assert len(exp) == cp.n
    FIT, BA = abi.KSS_S_NODE_RESOURCES_FIT, abi.KSS_S_BALANCED_ALLOCATION
    scored = 0
    for j, e in enumerate(exp):
        m = res.meta(j)
        idx = {t: cc.node_names.index("%s%03d" % (t, e["case"])) for t in "ab"}
        name = cases[e["case"]]["name"]
        assert ch[j] == (idx[e["chosen"]] if e["chosen"] else -1), (j, name)
        assert (m["n_feasible"], m["scored"]) == (e["n_feasible"], e["scored"]), (j, name, m, e)
        if e["scored"]:
            scored += 1
            for t in "ab":
                got = (int(res.raw[j, FIT, idx[t]]), int(res.raw[j, BA, idx[t]]))
                assert got == e[t], (j, name, t, got, e[t])
            assert m["best_total"] == e["best_total"], (j, name, m, e)
    return scored


@pytest.mark.parametrize("name", list(FIXTURES))
def test_both_oracles_agree(name):
    _, nodes, bound, pods, _, _ = fixture(name)
    crosscheck.run_both(nodes, bound, pods)


@pytest.mark.parametrize("pname", [p for p in vx.PROFILES])
@pytest.mark.parametrize("name", list(FIXTURES))
def test_c_oracle_equals_exact_arithmetic(name, pname):
    cases, _, _, _, cc, cp = fixture(name)
    desc = vx.PROFILES[pname]
    ch, res, _ = oracle(cc, cp, vx.make_profile(desc))
    second = bool(FIXTURES[name].get("second"))
    scored = check_against_exact(cases, cc, cp, desc, second, ch, res)
    first = [j for j, c in enumerate(vx.pod_cases(cases, second)) if j == 0 or vx.pod_cases(cases, second)[j - 1] != c]
    # 100 % of the first pods decode: scored, on a<j>, best_total the exact scores (checked above)
    assert all(res.meta(j)["scored"] == 1 for j in first)
    assert all(cc.node_names[ch[j]].startswith("a") for j in first)
    assert scored >= len(first)
    if second:
        assert scored > len(first) + N_PAIRS // 2  # most second pods are scored on the committed state


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixture_holds_every_operand_class(name):
    cases = fixture(name)[0]
    second = bool(FIXTURES[name].get("second"))
    single, pairs = vx.operands_of(cases, len(vx.pod_cases(cases, True)))
    cnt = collections.Counter(k for s in single for k in s)
    cnt.update(k for s in pairs for k in s)
    print(name, dict(cnt))
    for k in vx.CLASSES + vx.PAIR_CLASSES:
        assert cnt[k] >= 8, (k, cnt[k])
    # near_bound is computed for two pods per pair; with one it is inside by more
    a, b = vx.f64_sum(cases, len(vx.pod_cases(cases, second)))
    assert a < vx.E52 and b < vx.E52
    if FIXTURES[name].get("same_shape"):
        _, _, _, _, _, cp = fixture(name)
        ids, n = native.plan_shapes(cp.as_struct())
        assert 1 < n <= 4, n
        big = [j for j, c in enumerate(vx.pod_cases(cases, second)) if cases[c]["pod"] == list(vx.SAME_SHAPE)]
        assert len(big) > cp.n // 2 and len(set(int(ids[j]) for j in big)) == 1


def _f32_floor_estimates(x, d):
    """floor((float)x * r) for r the correctly rounded float reciprocal of d and its two
    neighbours: the estimates small_div can start from when v_rcp_f32 is within 1 ulp."""
    r0 = np.float32(1.0) / d.astype(np.float32)
    out = []
    for r in (r0, np.nextafter(r0, np.float32(0)), np.nextafter(r0, np.float32(2))):
        out.append((x.astype(np.float32) * r).astype(np.int64))
    return out


def test_small_div_operands_need_both_corrections():
    ops = np.array(vx.small_div_operands(), dtype=np.int64)
    x, d = ops[:, 0], ops[:, 1]
    assert len(ops) >= 1 << 16 and d.max() == 3 << 20 and len(np.unique(d)) >= 2000
    want = x // d
    low = high = np.zeros(len(x), bool)
    for est in _f32_floor_estimates(x, d):
        assert (np.abs(est - want) <= 1).all()  # the +-1 corrections suffice on the host model
        low = low | (est == want - 1)
        high = high | (est == want + 1)
    print("small_div operands", len(x), "need +1:", int(low.sum()), "need -1:", int(high.sum()))
    assert low.sum() >= 8 and high.sum() >= 8


# --------------------------------------------------------------------------------------
# host planning at the bounds
# --------------------------------------------------------------------------------------
def _compiled(cases, second=False):
    nodes, bound, pods = vx.twin_cluster(cases, second=second)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    return cc, cp


def _plans(cc, cp, prof, scen=1):
    """plan_sweep with the fixture as scenario `scen` behind the plain twin fixture; plan_podset
    and plan_service on the fixture alone."""
    _, _, _, _, cc0, cp0 = fixture("twin")
    cl = [cc0.as_struct()] * scen + [cc.as_struct()]
    ps = [cp0.as_struct()] * scen + [cp.as_struct()]
    return (native.plan_sweep(prof, cl, ps), native.plan_podset(cc.as_struct(), cp.as_struct(), prof),
            native.plan_service(cc.as_struct(), cp.as_struct(), prof))


def _assert_plans(plans, inside, scen):
    sweep, podset, service = plans
    if inside:
        assert sweep["kernel"] == "k_simple" and sweep["reason"] == "eligible", sweep
    else:
        assert sweep["kernel"] == "k_schedule" and sweep["reason"] == VALUES_REASON and sweep["scenario"] == scen, sweep
    assert podset["kernel"] == "k_simple" and podset["reason"] == "eligible", podset
    assert service["chain"] == 1 and service["reason"] == "eligible", service


@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("bound", ["alloc", "weight", "sum"])
def test_plan_sweep_at_each_bound(bound, second):
    bc = vx.bound_cases(N_PAIRS, second=second)
    for tag in ("in", "out"):
        cases, pname = bc[bound + "-" + tag]
        cc, cp = _compiled(cases, second)
        a = vx.f64_sum(cases, cp.n)
        if bound == "alloc":
            assert int(cc.arrays["alloc"][:3, :cc.n_nodes].max()) == (vx.E46 - 1 if tag == "in" else vx.E46)
        elif bound == "weight":
            assert max(w for _, w in vx.PROFILES[pname]["fit"]) == (1 << 20) - (tag == "in")
        else:
            assert max(a) == (vx.E52 - 1 if tag == "in" else vx.E52)
            assert int(cc.arrays["requested"][:3, :cc.n_nodes].max()) + cp.n * int(cp.pods["commit_req"].max()) == max(a)
        if bound != "sum":
            assert max(a) == vx.E52 - 1  # the other bounds are crossed with the sum at its own edge
        # a weight is the profile's: no scenario is named (-1); the others name scenario 1
        _assert_plans(_plans(cc, cp, vx.make_profile(vx.PROFILES[pname])), tag == "in", -1 if bound == "weight" else 1)


def test_plan_sweep_at_the_request_bound():
    for inside in (True, False):
        cases = vx.request_bound_cases(inside)
        cc, cp = _compiled(cases)
        assert int(cp.pods["fit_request"].max()) == (vx.E52 - 1 if inside else vx.E52)
        assert max(vx.f64_sum(cases, 1)) == (vx.E52 - 1 if inside else vx.E52)
        _assert_plans(_plans(cc, cp, abi.default_profile(), scen=2), inside, 2)
        # neither value is schedulable, and both oracles say so
        ch, res, _ = oracle(cc, cp, abi.default_profile())
        assert list(ch) == [-1] and res.meta(0)["n_feasible"] == 0


# --------------------------------------------------------------------------------------
# above the envelope: k_schedule's range
# --------------------------------------------------------------------------------------
def above():
    if "above" not in _CACHE:
        cases = vx.above_cases()
        nodes, bound, pods = vx.twin_cluster(cases, second=True)
        cc, cp, _ = compile_cluster(nodes, bound, pods)
        _CACHE["above"] = (cases, nodes, bound, pods, cc, cp)
    return _CACHE["above"]


def test_above_the_envelope_fixture():
    """Allocatables in [2^46, 2^56): (capacity - requested) * 100 sits on both sides of 2^53 at least
    8 times each, both oracles agree, the C oracle equals exact arithmetic under the default and two
    runtime profiles, and kss_plan_sweep names the values."""
    cases, nodes, bound, pods, cc, cp = above()
    x = [(c["cap"][r] - c["req"][r] - c["pod"][r]) * 100 for c in cases for r in range(2)]
    assert sum(vx.E53 - 300 <= v < vx.E53 for v in x) >= 8 and sum(vx.E53 <= v < vx.E53 + 300 for v in x) >= 8
    assert min(min(c["cap"][:2]) for c in cases) == vx.E46 and max(max(c["cap"]) for c in cases) == (1 << 56) - 1
    crosscheck.run_both(nodes, bound, pods)
    for pname in ("default", "most124", "least124_ba3"):
        ch, res, _ = oracle(cc, cp, vx.make_profile(vx.PROFILES[pname]))
        assert check_against_exact(cases, cc, cp, vx.PROFILES[pname], True, ch, res) >= len(cases)
    _assert_plans(_plans(cc, cp, abi.default_profile()), False, 1)


# --------------------------------------------------------------------------------------
# contests: choices that hang on the correction
# --------------------------------------------------------------------------------------
LEAST_PROFILES = ("default", "least124", "ba3", "least124_ba3")


def test_contests_tie_in_exact_arithmetic():
    """Every contest pod meets an est_low (est_high) operand on all three resources of one node, the
    exact totals tie under every LeastAllocated profile, and both oracles pick the lower index."""
    nodes, bound, pods, expect = vx.contest_cluster()
    cc, cp = crosscheck.run_both(nodes, bound, pods)[:2]
    for e in expect:
        hot = 0 if e["kind"] == "est_low" else 1
        name = e["names"][hot]
        n = next(x for x in nodes if x["metadata"]["name"] == name)
        b = next(x for x in bound if x["spec"]["nodeName"] == name)
        from kss import quantity
        for r, key in enumerate(("cpu", "memory", "ephemeral-storage")):
            f = quantity.milli_value if r == 0 else quantity.value
            cap = f(n["status"]["allocatable"][key])
            rq = f(b["spec"]["containers"][0]["resources"]["requests"][key]) + vx.CONTEST_POD[r]
            assert e["kind"] in vx.classify(cap, rq), (name, key)
    for pname in LEAST_PROFILES:
        ch, res, _ = oracle(cc, cp, vx.make_profile(vx.PROFILES[pname]))
        ties = collections.Counter()
        for j, e in enumerate(expect):
            want, tie = vx.contest_winner(e, pname)
            ties[e["kind"]] += tie
            assert cc.node_names[ch[j]] == want and res.meta(j)["scored"] == 1, (pname, j, e)
            assert want == e["names"][0] or not tie
        assert ties["est_low"] >= 8 and ties["est_high"] >= 8, (pname, ties)


# --------------------------------------------------------------------------------------
# the fixtures of tests/test_gpu_bounds_lifetime.py hold what they claim
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("batches", [1, 2])
def test_lifetime_cases_cross_the_sum_bound_after_one_batch(batches):
    """lifetime_cases(batches=1): after one batch the largest NonZeroRequested plus n * max commit is
    across 2^52 (the best-effort pods landed on the near-bound nodes); with batches=2 even the load-time
    maximum plus two batches' n * max commit stays inside."""
    cases = vx.lifetime_cases(N_PAIRS, batches)
    cc, cp, _ = compile_cluster(*vx.twin_cluster(cases))
    n, creq, cnz = cp.n, int(cp.pods["commit_req"][:, :3].max()), int(cp.pods["commit_nz"].max())
    N = cc.n_nodes
    load = (int(cc.arrays["requested"][:3, :N].max()), int(cc.arrays["nonzero"][:, :N].max()))
    assert (load[0] + batches * n * creq, load[1] + batches * n * cnz) == vx.f64_sum(cases, batches * n) == (vx.E52 - 1, vx.E52 - 1)
    _, _, fin = oracle(cc, cp, abi.default_profile())
    after = (int(fin["requested"][:3, :N].max()), int(fin["nonzero"][:, :N].max()))
    assert after[1] > load[1] and after[0] == load[0]
    assert (after[1] + n * cnz >= vx.E52) == (batches == 1)


def test_witness_passes_2_53_on_an_odd_value():
    """Five copies of the witness pod, without the NodeResourcesFit filter: all land on a000, and the
    oracle's int64 Requested equals the Python-integer sum after each (odd and above 2^53 after four)."""
    nodes, bound, pods = vx.twin_cluster(vx.witness_cases())
    five = pods + [p for k in range(1, 5) for p in vx.renamed(pods, "-%d" % k)]
    cc, cp, _ = compile_cluster(nodes, bound, five)
    prof = abi.default_profile()
    prof.filter_enabled &= ~(1 << abi.KSS_F_NODE_RESOURCES_FIT)
    a = cc.node_names.index("a000")
    for runs in range(1, 6):
        ch, _, fin = oracle_c.schedule(prof, cc.as_struct(), cp.as_struct(), runs, cc.n_nodes, record="meta")
        assert list(ch) == [a] * runs
        assert int(fin["requested"][0, a]) == vx.witness_requested(runs)
    assert vx.witness_requested(1) + vx.WITNESS_POD >= vx.E52 > vx.witness_requested(1)
    assert float(vx.witness_requested(4)) != vx.witness_requested(4)  # no double holds it
    # with the filter on, the pod fits nowhere: the bound is all that keeps the fast kernels off these sums
    assert list(oracle(cc, cp, abi.default_profile())[0]) == [-1] * 5
