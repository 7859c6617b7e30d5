"""The fast kernels at the edges of their exact-arithmetic envelope, and k_schedule beyond it, against
the C oracle bit for bit (fixtures: tests/value_edge_fixtures.py; tests/test_value_envelope.py shows
on the CPU that the oracle equals exact integer / correctly rounded arithmetic on every one of them,
and that every twin pod's best_total exposes its node's Fit and BalancedAllocation scores).

Inside the envelope (allocatables up to 2^46 - 1, Requested + n * commit = 2^52 - 1, operands whose
first reciprocal estimate is one off in either direction): k_simple in its DEF and runtime-profile
instantiations, the shape-table loop, the ports-and-images and volumes forms, k_spread, the sweep and
the service's k_simple-shaped chain.  Across each of the four host bounds, one unit further: the
batch runs on k_schedule, the service on its general chain, the sweep on k_schedule -- and the
results still equal the oracle's, while the twin one unit inside runs on the fast kernel.  Above the
envelope (allocatables 2^46 .. 2^56, (capacity - requested) * 100 on both sides of 2^53): k_schedule's
records and eval_pod, raw and normalised scores per node.

Every case compares the chosen nodes, fetch_meta (n_feasible, scored, status, best_total) and the
final node state, and asserts which kernel ran."""
import numpy as np
import pytest

import oracle_c
import value_edge_fixtures as vx
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu

N_PAIRS = 64
VALUES_REASON = "a scenario's values or the profile's weights leave the exact f64 envelope: the whole sweep runs on k_schedule"
_CACHE = {}


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _compiled(key, make):
    """(cc, cp) of one cluster, compiled once."""
    if key not in _CACHE:
        nodes, bound, pods = make()
        cc, cp, _ = compile_cluster(nodes, bound, pods)
        _CACHE[key] = (cc, cp)
    return _CACHE[key]


def _fx(name):
    mk = {
        "twin": lambda: vx.twin_cluster(vx.make_cases(N_PAIRS)),
        "second": lambda: vx.twin_cluster(vx.make_cases(N_PAIRS), second=True),
        "same-shape": lambda: vx.twin_cluster(vx.make_cases(N_PAIRS, same_shape=True), second=True),
        "spread": lambda: vx.twin_cluster(vx.make_cases(N_PAIRS), spread=True),
        "ports-images": lambda: vx.twin_cluster(vx.make_cases(N_PAIRS), second=True, ports=range(0, N_PAIRS, 5),
                                                images=range(0, N_PAIRS, 7)),
        "volumes": lambda: vx.twin_cluster(vx.make_cases(N_PAIRS), second=True, volumes=range(0, N_PAIRS, 6)),
        "above": lambda: vx.twin_cluster(vx.above_cases(), second=True),
        "contest": lambda: vx.contest_cluster()[:3],
    }[name]
    return _compiled(name, mk)


def _want(key, cc, cp, pname="default"):
    """The oracle's (chosen, records, final state) of a compiled cluster under a profile, computed
    once and shared (nothing writes to them)."""
    k = ("want", key, pname)
    if k not in _CACHE:
        _CACHE[k] = oracle_c.schedule(vx.make_profile(vx.PROFILES[pname]), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes,
                                      record=True, n_classes=len(cc.classes), n_terms=len(cc.terms))
    return _CACHE[k]


def _meta_equal(meta, res, n):
    for j in range(n):
        m = res.meta(j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], (j, int(meta[j, 4]), m)


def _state_equal(ctx, cc, fin):
    N = cc.n_nodes
    g = ctx.node_state()
    np.testing.assert_array_equal(g["requested"][:, :N], fin["requested"][:, :N])
    np.testing.assert_array_equal(g["nonzero"][:, :N], fin["nonzero"][:, :N])
    np.testing.assert_array_equal(g["pod_count"][:N], fin["pod_count"][:N])
    np.testing.assert_array_equal(ctx.port_state(), fin["port_used"][:N])


def _batch(cc, cp, want, pname="default", kernel="k_simple", flags=0, opts=None, check=None):
    """One unrecorded batch on a fresh context against the oracle; returns the geometry."""
    ch_o, res, fin = want
    for k, v in (opts or {}).items():
        native.set_option(k, v)
    ctx = native.Context(vx.make_profile(vx.PROFILES[pname]))
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n, flags=flags)
    assert ctx.last_kernel() == kernel, ctx.last_kernel()
    np.testing.assert_array_equal(chosen, ch_o)
    _meta_equal(ctx.fetch_meta(cp.n), res, cp.n)
    _state_equal(ctx, cc, fin)
    geom = dict(ctx.last_geometry(), table=ctx.last_shape_table()["shapes"], form=ctx.last_simple_form())
    if check:
        check(ctx)
    ctx.close()
    return geom


# --------------------------------------------------------------------------------------
# inside the envelope
# --------------------------------------------------------------------------------------
GEOMETRIES = [("one-workgroup", dict(shards=1), abi.KSS_SCHED_FORCE_SINGLE_WG),
              ("three-shards", dict(shards=3, force_threads=128), 0),
              ("nodes-per-lane", dict(shards=1, force_threads=64), 0)]


@pytest.mark.parametrize("fixture", ["twin", "second"])
@pytest.mark.parametrize("name,opts,flags", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_k_simple_default_profile(name, opts, flags, fixture):
    """The DEF kernels (dyn_eval_def, least_bf, div_rn_d); `second`: every pair's second pod is
    evaluated on the sums its predecessor's commit left (the H1 re-evaluation)."""
    cc, cp = _fx(fixture)
    geom = _batch(cc, cp, _want(fixture, cc, cp), flags=flags, opts=dict(opts, shape_table=0))
    assert geom["shards"] == opts["shards"] and geom["table"] == 0, geom
    if "force_threads" in opts:
        assert geom["threads"] == opts["force_threads"], geom
    if name == "nodes-per-lane":
        assert geom["nodes_per_lane"] > 1, geom


@pytest.mark.parametrize("pname,fixture", [("least124", "twin"), ("most124", "twin"), ("ba3", "twin"), ("least124_ba3", "twin"),
                                           ("w_inside", "twin"), ("most124", "second"), ("least124_ba3", "second")])
def test_k_simple_runtime_profiles(pname, fixture):
    """dyn_eval: alloc_score_d in both strategies, the weight average by small_div (weight sums 7
    and 2^21 - 1), BalancedAllocation over three resources (sqrt)."""
    cc, cp = _fx(fixture)
    geom = _batch(cc, cp, _want(fixture, cc, cp, pname), pname=pname, opts=dict(shards=2, shape_table=0))
    assert geom["shards"] == 2 and geom["table"] == 0, geom


@pytest.mark.parametrize("shards", [2, 3])
def test_shape_table_loop(shards):
    cc, cp = _fx("same-shape")
    geom = _batch(cc, cp, _want("same-shape", cc, cp), opts=dict(shards=shards, force_threads=128, shape_table=1))
    assert geom["shards"] == shards and geom["table"] > 0, geom


def test_k_spread():
    cc, cp = _fx("spread")
    _batch(cc, cp, _want("spread", cc, cp), kernel="k_spread", opts=dict(shards=2))


def test_ports_and_images_form():
    cc, cp = _fx("ports-images")
    want = _want("ports-images", cc, cp)
    assert (want[1].fail_plugin == abi.KSS_F_NODE_PORTS).any()
    geom = _batch(cc, cp, want, opts=dict(simple_ports_images=1, shards=2))
    assert geom["form"]["volumes"] == 0, geom


def test_volumes_form():
    cc, cp = _fx("volumes")

    def check(ctx):
        vc, va = ctx.volume_state()
        np.testing.assert_array_equal(va, want[2]["vol_attached"])
        np.testing.assert_array_equal(vc, want[2]["vol_count"])
    want = _want("volumes", cc, cp)
    geom = _batch(cc, cp, want, opts=dict(simple_ports_images=1, simple_volumes=1, shards=2), check=check)
    assert geom["form"]["volumes"] == 1, geom


def _sweep_equal(scen, prof, wants, kernel):
    cl, ps = [cc.as_struct() for cc, _ in scen], [cp.as_struct() for _, cp in scen]
    sw = native.Sweep(prof, cl, ps)
    assert sw.info()["kernel"] == kernel, sw.info()
    for _ in range(2):  # the second run: the reset restored the state
        chosen, _ms = sw.run()
        np.testing.assert_array_equal(chosen, np.concatenate([w[0] for w in wants]))
    sw.close()
    chosen, _ms = native.schedule_scenarios(prof, cl, ps)
    np.testing.assert_array_equal(chosen, np.concatenate([w[0] for w in wants]))


@pytest.mark.parametrize("pname", ["default", "least124_ba3"])
def test_sweep(pname):
    """A sweep reports chosen nodes only: the third scenario's choices are ties in exact arithmetic
    that a quotient left one off decides the other way (contest_cluster)."""
    scen = [_fx("twin"), _fx("second"), _fx("contest")]
    wants = [_want("twin", *scen[0], pname), _want("second", *scen[1], pname), _want("contest", *scen[2], pname)]
    _sweep_equal(scen, vx.make_profile(vx.PROFILES[pname]), wants, "k_simple")


@pytest.mark.parametrize("pname", ["default", "least124", "ba3", "least124_ba3"])
def test_contests_are_decided_as_exact_arithmetic_decides(pname):
    cc, cp = _fx("contest")
    want = _want("contest", cc, cp, pname)
    expect = vx.contest_cluster()[3]
    for j, e in enumerate(expect):
        assert cc.node_names[want[0][j]] == vx.contest_winner(e, pname)[0]
    _batch(cc, cp, want, pname=pname, opts=dict(shards=2, shape_table=0))


def _service(cc, cp, want, pname, mode):
    """Every pod through service_eval + service_commit: outcome, best_total, and the per-node raw Fit
    and BalancedAllocation scores of the feasible nodes against the oracle's records."""
    ch_o, res, fin = want
    svc = native.Context(vx.make_profile(vx.PROFILES[pname]))
    svc.load(cc.as_struct())
    svc.stage(cp.as_struct())
    N = cc.n_nodes
    rows = [abi.KSS_S_NODE_RESOURCES_FIT, abi.KSS_S_BALANCED_ALLOCATION]
    for j in range(cp.n):
        got = svc.service_eval(j)
        if j == 0:
            assert svc.service_mode() == mode, svc.service_mode()
        m = res.meta(j)
        assert (got.chosen, got.n_feasible, got.scored, got.status) == (m["chosen"], m["n_feasible"], m["scored"], m["status"]), (j, m)
        np.testing.assert_array_equal(got.fail_plugin[:N], res.fail_plugin[j, :N], err_msg=f"pod {j}")
        if m["scored"]:
            assert got.best_total == m["best_total"], j
            feas = res.fail_plugin[j, :N] == 0
            np.testing.assert_array_equal(got.raw[rows][:, :N][:, feas], res.raw[j][rows][:, :N][:, feas], err_msg=f"pod {j} raw")
            np.testing.assert_array_equal(got.total[:N][feas], res.total[j, :N][feas], err_msg=f"pod {j} total")
        if got.chosen >= 0:
            svc.service_commit(j, got.chosen)
    svc.service_stop()
    _state_equal(svc, cc, fin)
    svc.close()


@pytest.mark.parametrize("pname", ["default", "least124_ba3"])
def test_service_chain(pname):
    cc, cp = _fx("second")
    _service(cc, cp, _want("second", cc, cp, pname), pname, 1)


# --------------------------------------------------------------------------------------
# across each bound: one unit further the batch falls back, and is still right
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", ["alloc", "weight", "sum"])
def test_across_each_bound(bound):
    bc = vx.bound_cases(N_PAIRS)
    for tag in ("in", "out"):
        cases, pname = bc[bound + "-" + tag]
        key = ("bound", bound, tag)
        cc, cp = _compiled(key, lambda: vx.twin_cluster(cases))
        want = _want(key, cc, cp, pname)
        inside = tag == "in"
        prof = vx.make_profile(vx.PROFILES[pname])
        plan = native.plan_sweep(prof, [cc.as_struct()], [cp.as_struct()])
        assert (plan["reason"] == "eligible") if inside else (plan["reason"] == VALUES_REASON and plan["kernel"] == "k_schedule"), plan
        _batch(cc, cp, want, pname=pname, kernel="k_simple" if inside else "k_schedule", opts=dict(shards=2))
        _service(cc, cp, want, pname, 1 if inside else 0)
        _sweep_equal([(cc, cp)], prof, [want], "k_simple" if inside else "k_schedule")


def test_across_the_request_bound():
    """A pod request of 2^52 - 1 / 2^52: schedulable nowhere, on k_simple / k_schedule."""
    for inside in (True, False):
        key = ("bound", "request", inside)
        cc, cp = _compiled(key, lambda: vx.twin_cluster(vx.request_bound_cases(inside)))
        want = _want(key, cc, cp)
        assert list(want[0]) == [-1]
        plan = native.plan_sweep(abi.default_profile(), [cc.as_struct()], [cp.as_struct()])
        assert (plan["reason"] == "eligible") if inside else (plan["reason"] == VALUES_REASON), plan
        _batch(cc, cp, want, kernel="k_simple" if inside else "k_schedule")
        _service(cc, cp, want, "default", 1 if inside else 0)
        _sweep_equal([(cc, cp)], abi.default_profile(), [want], "k_simple" if inside else "k_schedule")


# --------------------------------------------------------------------------------------
# above the envelope: k_schedule's own arithmetic (div_i64 on both sides of 2^53)
# --------------------------------------------------------------------------------------
def _records_equal(got, res, j, N):
    np.testing.assert_array_equal(got.fail_plugin[:N], res.fail_plugin[j, :N], err_msg=f"pod {j} verdicts")
    m = res.meta(j)
    assert (got.chosen, got.n_feasible, got.scored, got.status) == (m["chosen"], m["n_feasible"], m["scored"], m["status"]), (j, m)
    if m["scored"]:
        feas = res.fail_plugin[j, :N] == 0
        np.testing.assert_array_equal(got.raw[:, :N][:, feas], res.raw[j][:, :N][:, feas], err_msg=f"pod {j} raw")
        np.testing.assert_array_equal(got.norm[:, :N][:, feas], res.norm[j][:, :N][:, feas], err_msg=f"pod {j} norm")
        np.testing.assert_array_equal(got.total[:N][feas], res.total[j, :N][feas], err_msg=f"pod {j} total")


@pytest.mark.parametrize("pname", ["default", "most124", "least124_ba3"])
def test_k_schedule_above_the_envelope(pname):
    cc, cp = _fx("above")
    ch_o, res, fin = _want("above", cc, cp, pname)
    N = cc.n_nodes
    assert sum(res.meta(j)["scored"] for j in range(cp.n)) >= len(vx.above_cases())
    prof = vx.make_profile(vx.PROFILES[pname])
    ctx = native.Context(prof, max_pods_record=cp.n)
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n, record=True)
    assert ctx.last_kernel() == "k_schedule"
    np.testing.assert_array_equal(chosen, ch_o)
    for j in range(cp.n):
        _records_equal(ctx.fetch_record(j), res, j, N)
    _state_equal(ctx, cc, fin)
    ctx.close()
    # unrecorded: the host sends the batch to k_schedule by its values
    _batch(cc, cp, (ch_o, res, fin), pname=pname, kernel="k_schedule")
    # pod by pod: eval_pod + commit
    ctx = native.Context(prof)
    ctx.load(cc.as_struct())
    for j in range(cp.n):
        r = ctx.eval_pod(cp.as_struct(), j)
        _records_equal(r, res, j, N)
        if r.chosen >= 0:
            ctx.commit(cp.as_struct(), j, int(r.chosen))
    _state_equal(ctx, cc, fin)
    ctx.close()
