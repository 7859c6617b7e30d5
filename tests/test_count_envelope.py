"""The count-edge fixtures (tests/count_edge_fixtures.py) hold what they claim; no GPU.

  * every fixture is inside, or one unit across, its bound by exactly the stated margin -- from Python
    integers (spread_bounds), not from the library -- and each in / out pair differs in exactly one
    value (one count cell, or one pod-side maxSkew);
  * the C oracle equals the hand-derived expectations (n_feasible, chosen node, best_total) on every
    integer-only fixture, at 1 and 4 threads, and the raw InterPodAffinity sum it records is the
    stated largest 32-bit intermediate;
  * the counts each fixture asserts are reached (the term cell of n00 ends on exactly 65535);
  * kss_plan_podset keeps answering "eligible" on both sides: values are left to the launch.
The object-level oracle (oracle/k8s_oracle.py) is left out: it reads pod objects, and the counts
here exist only in the compiled arrays (65,535 objects per cell is not a fixture)."""
import numpy as np
import pytest

import count_edge_fixtures as cx
import oracle_c
from kss import abi, native
from kss.compile import compile_cluster


def _oracle(cc, cp, threads):
    return oracle_c.schedule(abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record=True,
                             threads=threads, n_classes=len(cc.classes), n_terms=len(cc.terms))


def _equal_expect(cc, cp, exp, threads):
    ch, res, fin = _oracle(cc, cp, threads)
    for j, e in enumerate(exp):
        m = res.meta(j)
        got = dict(chosen=cc.node_names[ch[j]], n_feasible=m["n_feasible"], best_total=m["best_total"])
        assert got == {k: e[k] for k in got}, (j, got, e)
        assert m["scored"] == 1 and m["status"] == 0
    return ch, res, fin


def _count_cells(cc):
    N = cc.n_nodes  # (a column without rows is a one-element placeholder)
    return np.concatenate([cc.arrays[k][:, :N].ravel() for k, rows in (("class_count", cc.classes), ("term_count", cc.terms)) if rows])


def _pods_equal(a, b):
    return a.pods.tobytes() == b.pods.tobytes() and a.spreads.tobytes() == b.spreads.tobytes() and \
        a.ipa.tobytes() == b.ipa.tobytes() and a.ints.tobytes() == b.ints.tobytes()


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "hard+soft"])
def test_cell(soft, threads):
    pair = {}
    for across in (False, True):
        cc, cp, _ = compile_cluster(*cx.cell_objects(soft))
        fill = cx.cell_fill(cc, across)
        total, cell = cx.totals(cc, cp)
        inside, fig = cx.spread_bounds(dict(ref_weight=cx.CELL_REF), total, cell, cc.n_nodes)
        assert fig["cell"] == cx.CELL_MAX + (1 if across else 0) and inside == (not across)
        assert fig["sum32"] < cx.LIM32 // 8                      # nowhere near the other bound
        assert cell == fill["t0"] + cx.CELL_PODS * 2              # max_mult 2: two identical own terms
        exp, reach = cx.cell_expect(fill)
        assert reach["term_n00"] == cx.CELL_MAX + (1 if across else 0)
        assert native.plan_podset(cc.as_struct(), cp.as_struct(), abi.default_profile())["kernel"] == "k_spread"
        if soft:  # the soft score goes through log: the oracle is the reference; the counts are still reached
            ch, res, fin = _oracle(cc, cp, threads)
            assert all(res.meta(j)["n_feasible"] == e["n_feasible"] for j, e in enumerate(exp))
        else:
            ch, res, fin = _equal_expect(cc, cp, exp, threads)
        n00 = cc.node_names.index("n00")
        assert [cc.node_names[c] for c in ch] == ["n00"] * cx.CELL_PODS
        assert int(fin["term_count"][fill["term"], n00]) == reach["term_n00"]
        assert int(fin["class_count"][fill["cls"], n00]) == reach["class_n00"]
        pair[across] = (cc, cp)
    diff = _count_cells(pair[True][0]) - _count_cells(pair[False][0])
    assert sorted(diff.tolist())[-2:] == [0, 1] and diff.sum() == 1
    assert _pods_equal(pair[True][1], pair[False][1])


@pytest.mark.parametrize("threads", [1, 4])
def test_sum32(threads):
    pair = {}
    for across in (False, True):
        cc, cp, _ = compile_cluster(*cx.sum32_objects())
        fill = cx.sum32_fill(cc, across)
        total, cell = cx.totals(cc, cp)
        inside, fig = cx.spread_bounds(dict(ref_weight=cx.SUM_REF), total, cell, cc.n_nodes)
        assert total == cx.sum32_total(across) and inside == (not across) and cell <= cx.CELL_MAX
        if across:
            assert fig["sum32"] >= cx.LIM32 > fig["sum32"] - cx.MAXK * cx.SUM_REF
        else:
            assert fig["sum32"] < cx.LIM32 <= fig["sum32"] + cx.MAXK * cx.SUM_REF
        exp, largest = cx.sum32_expect(fill)
        assert largest < (1 << 31)  # on both sides: the contract over-counts a reference of two rows
        ch, res, fin = _equal_expect(cc, cp, exp, threads)
        s00 = cc.node_names.index("s00")
        assert int(res.raw[cp.n - 1, abi.KSS_S_INTER_POD_AFFINITY, s00]) == largest
        assert int(res.raw[cp.n - 1, abi.KSS_S_INTER_POD_AFFINITY, cc.node_names.index("s23")]) == 0
        assert native.plan_podset(cc.as_struct(), cp.as_struct(), abi.default_profile())["kernel"] == "k_spread"
        pair[across] = (cc, cp)
    diff = _count_cells(pair[True][0]) - _count_cells(pair[False][0])
    assert sorted(diff.tolist())[-2:] == [0, 1] and diff.sum() == 1
    assert _pods_equal(pair[True][1], pair[False][1])


@pytest.mark.parametrize("n_soft", [2, 4])
def test_soft2(n_soft):
    pair = {}
    for across in (False, True):
        cc, cp, _ = compile_cluster(*cx.soft2_objects(n_soft, across))
        cx.soft2_fill(cc)
        total, cell = cx.totals(cc, cp)
        assert total == cx.soft2_total()
        skew = int(cp.spreads["max_skew"].max())
        assert skew == cx.soft2_skew(n_soft, total, across)
        inside, fig = cx.spread_bounds(dict(ref_weight=1, max_soft=n_soft, max_skew=skew), total, cell, cc.n_nodes)
        assert inside == (not across)
        # one unit of maxSkew moves the figure by max_soft: the pair straddles 2^31 - 1
        assert (fig["soft2"] >= cx.LIM32 > fig["soft2"] - n_soft) if across else (fig["soft2"] < cx.LIM32 <= fig["soft2"] + n_soft)
        ch, res, fin = _oracle(cc, cp, 1)
        ch4, res4, _ = _oracle(cc, cp, 4)
        np.testing.assert_array_equal(ch, ch4)
        assert all(res.meta(j) == res4.meta(j) and res.meta(j)["scored"] == 1 for j in range(cp.n))
        assert int(res.raw[:, abi.KSS_S_POD_TOPOLOGY_SPREAD, :cc.n_nodes].max()) < (1 << 31)
        pair[across] = (cc, cp)
    np.testing.assert_array_equal(_count_cells(pair[True][0]), _count_cells(pair[False][0]))
    a, b = pair[False][1].spreads["max_skew"], pair[True][1].spreads["max_skew"]
    assert sorted(set((b.astype(int) - a.astype(int)).tolist())) == [0, 1]  # the zone constraint of every pod, by one
    assert int((b != a).sum()) == cx.SOFT_PODS
