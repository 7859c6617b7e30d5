"""The volumes forms' packed fields and upper-word keys on the CPU (tests/volume_edge_fixtures.py):
the hand-derived expectations of eight_keys against the C oracle and the object-level oracle, the
restated pack's coverage of all 16 field positions, volume_form_fixtures.reach's replay on every
field_tops variant, and the host's routing (kss_plan_podset, kss_plan_sweep): every inside variant is
planned on the form, every across variant on k_schedule with the crossing key named."""
import numpy as np
import pytest

import oracle_c
import volume_edge_fixtures as vef
import volume_form_fixtures as vff
import volume_fuzz
from crosscheck import run_both
from kss import abi, native
from kss.compile import compile_cluster

UPPER = (4, 5, 6, 7)
INSIDE = [v for v in vef.VARIANTS if vef.field_tops(*v)["across"] is None]
ACROSS = [v for v in vef.VARIANTS if v not in INSIDE]


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _oracle(cc, cp, threads=1):
    return oracle_c.schedule(abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record=True,
                             threads=threads, n_classes=len(cc.classes), n_terms=len(cc.terms))


def assert_hand_derived(cc, cp, ch_o, res, fin, expect, final):
    """The oracle's choices, its verdict on every pod's pinned node and its final vol_attached equal
    the fixture's literals."""
    assert cp.n == len(expect)
    for j, (name, at, chosen, fail) in enumerate(expect):
        assert int(ch_o[j]) == chosen, (name, int(ch_o[j]), chosen)
        assert int(res.fail_plugin[j, at]) == fail, (name, int(res.fail_plugin[j, at]), fail)
    np.testing.assert_array_equal(fin["vol_attached"][:8, :cc.n_nodes], vef.final_attached(cc, final))


def assert_upper_keys_decide(r):
    """Keys 4, 5, 6 and 7 each decide at least one limit failure and at least one H1 pair."""
    fail_keys = {k for _, _, k in r["limit_failures"]}
    h1_keys = {k for _, _, k in r["h1_events"]}
    assert set(UPPER) <= fail_keys and set(UPPER) <= h1_keys, (sorted(fail_keys), sorted(h1_keys))


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("soft", [False, True], ids=["plain", "soft"])
def test_eight_keys_c_oracle_matches_hand_derived(threads, soft):
    fx = vef.eight_keys(soft=soft)
    assert len(fx["nodes"]) <= 24 and len(fx["pods"]) <= 40
    cc, cp = vef.compiled(fx)
    assert vef.adds(cc, cp) == vef.A
    if soft:
        assert [int(cp.pods[j]["n_soft"]) for j in range(cp.n)] == [1 - j % 2 for j in range(cp.n)]
    ch_o, res, fin = _oracle(cc, cp, threads)
    assert_hand_derived(cc, cp, ch_o, res, fin, fx["expect"], fx["final"])
    r = vff.reach(cc, cp, ch_o, res)
    assert_upper_keys_decide(r)
    assert {k for _, _, k in r["limit_failures"]} == set(range(8)) and len(r["h1_events"]) == 8
    # (d): under keys 0 and 5 (7) at once, decided by the upper-word key
    for name, key in (("d5", 5), ("d7", 7)):
        j = [e[0] for e in fx["expect"]].index(name)
        m = vff.pod_masks(cc, cp, j)
        assert m[3] == (1 | 1 << key) and (j, fx["expect"][j][1], key) in r["limit_failures"]


@pytest.mark.parametrize("soft", [False, True], ids=["plain", "soft"])
def test_eight_keys_object_oracle_matches_c_oracle(soft):
    fx = vef.eight_keys(soft=soft)
    run_both(fx["nodes"], fx["bound"], fx["pods"], storage=fx["storage"])


@pytest.mark.parametrize("pct", [30, 0])
def test_wide_unpinned_object_oracle_matches_c_oracle(pct):
    """eight_keys(pin=False, wide=True), the window's cluster: 150 nodes, numFeasibleNodesToFind 100."""
    fx = vef.eight_keys(pin=False, wide=True)
    assert len(fx["nodes"]) == 150
    run_both(fx["nodes"], fx["bound"], fx["pods"], storage=fx["storage"], pct=pct)


def test_pack_covers_every_field_position():
    """Over the fixtures, every one of the 8 attached and 8 limit positions holds a non-zero value on
    some node, both limit words hold 0xFFFF somewhere, and the restated pack clamps nothing inside."""
    att_seen, lim_seen, unchecked = set(), set(), set()
    tops = set()
    for v in [None] + INSIDE:
        cc = vef.compiled(vef.eight_keys())[0] if v is None else vef.field_tops(*v)["cc"]
        for n, (used, a0, a1, l0, l1) in enumerate(vef.pack(cc)):
            for k in range(8):
                a, l = vef.field((a0, a1)[k >> 2], k & 3), vef.field((l0, l1)[k >> 2], k & 3)
                assert a == max(int(cc.arrays["vol_attached"][k][n]), 0)
                lv = int(cc.arrays["vol_limit"][k][n])
                assert l == (vef.UNCHECKED if lv < 0 else lv)
                att_seen |= {k} if a else set()
                lim_seen |= {k} if l else set()
                unchecked |= {k >> 2} if l == vef.UNCHECKED else set()
                tops |= {k} if a >= 32768 else set()
    assert att_seen == lim_seen == set(range(8)) and unchecked == {0, 1} and tops == set(range(8))


@pytest.mark.parametrize("v", vef.VARIANTS, ids=vef.variant_id)
def test_field_tops_replay_and_margins(v):
    """The C oracle on the written arrays: the replay in Python integers decides every recorded verdict,
    the hand-derived choices carry over, and the margin is exactly 0 inside / 1 across."""
    t = vef.field_tops(*v)
    cc, cp = t["cc"], t["cp"]
    m = vef.margins(cc, cp)
    if t["across"] is None:
        assert max(max(x) for x in m) == vef.FIELD_MAX, m  # inside by margin 0
        if v[0] == "limit_top":
            assert [x[0] for x in m] == [vef.FIELD_MAX] * 8, m  # att_max + A_k == 65534 for every key
    ch_o, res, fin = _oracle(cc, cp)
    r = vff.reach(cc, cp, ch_o, res)
    np.testing.assert_array_equal(np.array(r["att"]).T, fin["vol_attached"][:8, :cc.n_nodes])
    if t["expect"] is not None:
        assert_hand_derived(cc, cp, ch_o, res, fin, t["expect"], t["final"])
        assert_upper_keys_decide(r)
    if v[0] == "sum_top":
        assert int(fin["vol_attached"][6][vef.G[6]]) == vef.FIELD_MAX  # the counter really ends on the top
        assert int(fin["vol_attached"][6][vef.H[6]]) == vef.FIELD_MAX - 3
        j3 = [i for i in range(cp.n) if int(res.fail_plugin[i, vef.G[6]]) == abi.KSS_F_NODE_VOLUME_LIMITS]
        assert len(j3) == (1 if t["across"] is not None else 0)
    if v[0] == "carry":
        edge = v[1][0]
        for k in range(8):  # crossed during the batch
            assert int(cc.arrays["vol_attached"][k][vef.G[k]]) < edge + 1 == int(fin["vol_attached"][k][vef.G[k]])


# --------------------------------------------------------------------------------------
# routing (host only)
# --------------------------------------------------------------------------------------
FORMS = {"simple": ("simple_ports_images", "simple_volumes", "k_simple", "k_simple's"),
         "spread": ("spread_ports_images", "spread_volumes", "k_spread", "k_spread's")}


def assert_refused(plan, key, whose):
    assert plan["kernel"] == "k_schedule", plan
    assert "key %d" % key in plan["reason"] and "65534" in plan["reason"] and whose in plan["reason"], plan
    for other in range(8):
        assert other == key or "key %d" % other not in plan["reason"], plan


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("v", vef.VARIANTS, ids=vef.variant_id)
def test_plan_podset(v, form):
    pi, vol, kernel, whose = FORMS[form]
    t = vef.field_tops(*v, soft=form == "spread")
    native.set_option(pi, 1)
    native.set_option(vol, 1)
    plan = native.plan_podset(t["cc"].as_struct(), t["cp"].as_struct())
    if t["across"] is None:
        assert plan == {"kernel": kernel, "pod": -1, "reason": "eligible"}, plan
    else:
        assert_refused(plan, t["across"], whose)


def test_plan_podset_names_every_key():
    """The reason tables' other entries: limit_top crossed under each of the 8 keys, both forms."""
    for form in sorted(FORMS):
        pi, vol, kernel, whose = FORMS[form]
        native.reset_options()
        native.set_option(pi, 1)
        native.set_option(vol, 1)
        for k in range(8):
            t = vef.field_tops("limit_top", k, soft=form == "spread")
            assert_refused(native.plan_podset(t["cc"].as_struct(), t["cp"].as_struct()), k, whose)


@pytest.mark.parametrize("v", vef.VARIANTS, ids=vef.variant_id)
def test_plan_sweep(v):
    """The edge scenario second of three."""
    nodes, bound, pods, st = volume_fuzz.make(2, n_nodes=12, n_bound=16, n_pods=40)
    plain = compile_cluster(nodes, bound, pods, storage=st)[:2]
    t = vef.field_tops(*v)
    scen = [plain, (t["cc"], t["cp"]), (vef.field_tops("carry", (255, False))["cc"], vef.field_tops("carry", (255, False))["cp"])]
    native.set_option("sweep_ports_images", 1)
    native.set_option("sweep_volumes", 1)
    plan = native.plan_sweep(abi.default_profile(), [cc.as_struct() for cc, _ in scen], [cp.as_struct() for _, cp in scen],
                             detail=True)
    if t["across"] is None:
        assert plan == {"kernel": "k_simple", "form": True, "volumes": True, "scenario": -1, "pod": -1, "reason": "eligible"}, plan
    else:
        assert plan["volumes"] and plan["scenario"] == 1, plan
        assert_refused(plan, t["across"], "")
