"""k_spread at the edges of its integer envelope (fixtures: tests/count_edge_fixtures.py;
tests/test_count_envelope.py shows on the CPU that every fixture is on its edge and that the C oracle
equals the hand-derived expectations of the integer-only ones).

Inside each bound -- the largest 16-bit resident cell ending on exactly 65535, MAXK * ref_weight *
total the largest value below 2^31 - 1, max_soft * (... + maxSkew + 1) the same -- the batch runs on
k_spread and equals the oracle bit for bit: chosen nodes, fetch_meta (n_feasible, scored, status,
best_total) and the final requested / nonzero / pod_count / class_count / term_count.  Variants: one
shard and three, three chunk launches (the 16-bit cells near 65535 go through the HBM hand-off and its
checksum), option fold 0 / 1, the percentageOfNodesToScore window on the fixture widened to 150
nodes, the ports-and-images form with a host-port pod.  One unit across, the same batch reports
k_schedule and still equals the oracle.  For cell and sum32 the per-pod path (kss_eval_pod +
kss_commit pod by pod) and a recorded k_schedule batch are compared per node -- verdicts, raw and
normalised scores -- because k_spread keeps no per-node record.

spread_two_level is left out: no cluster of at most 24 nodes reaches the two-level exchanges."""
import numpy as np
import pytest

import count_edge_fixtures as cx
import oracle_c
from kss import abi, native
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu
_CACHE = {}


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _fx(name, across, **kw):
    """(cc, cp, expect or None) of one fixture, compiled and filled once (nothing writes to them)."""
    key = (name, across, tuple(sorted(kw.items())))
    if key not in _CACHE:
        if name == "cell":
            cc, cp, _ = compile_cluster(*cx.cell_objects(**kw))
            exp = cx.cell_expect(cx.cell_fill(cc, across))[0]
            if kw.get("soft") or kw.get("wide"):
                exp = None
        elif name == "sum32":
            cc, cp, _ = compile_cluster(*cx.sum32_objects())
            exp = cx.sum32_expect(cx.sum32_fill(cc, across))[0]
        else:
            cc, cp, _ = compile_cluster(*cx.soft2_objects(kw["n_soft"], across))
            cx.soft2_fill(cc)
            exp = None
        _CACHE[key] = (cc, cp, exp)
    return _CACHE[key]


def _want(name, across, prof=None, **kw):
    key = ("want", name, across, tuple(sorted(kw.items())), prof.pct_nodes_to_score if prof else 100)
    if key not in _CACHE:
        cc, cp, _ = _fx(name, across, **kw)
        _CACHE[key] = oracle_c.schedule(prof or abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes,
                                        record=True, n_classes=len(cc.classes), n_terms=len(cc.terms))
    return _CACHE[key]


def _meta_equal(meta, res, n, exp, cc):
    for j in range(n):
        m = res.meta(j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], (j, int(meta[j, 4]), m)
        if exp is not None:  # ... and the hand-derived figures
            assert (cc.node_names[meta[j, 0]], meta[j, 1], meta[j, 4]) == (exp[j]["chosen"], exp[j]["n_feasible"], exp[j]["best_total"]), j


def _state_equal(ctx, cc, fin):
    N = cc.n_nodes
    g = ctx.node_state()
    for k in ("requested", "nonzero", "pod_count"):
        np.testing.assert_array_equal(g[k][..., :N], fin[k][..., :N], err_msg=k)
    for k, n in (("class_count", len(cc.classes)), ("term_count", len(cc.terms))):
        np.testing.assert_array_equal(g[k][:n, :N], fin[k][:n, :N], err_msg=k)
    np.testing.assert_array_equal(ctx.port_state(), fin["port_used"][:N])


def _batch(fx, want, kernel, opts=None, prof=None, launches=None):
    cc, cp, exp = fx
    ch_o, res, fin = want
    for k, v in (opts or {}).items():
        native.set_option(k, v)
    ctx = native.Context(prof or abi.default_profile())
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n)
    assert ctx.last_kernel() == kernel, ctx.last_kernel()
    np.testing.assert_array_equal(chosen, ch_o)
    _meta_equal(ctx.fetch_meta(cp.n), res, cp.n, exp, cc)
    _state_equal(ctx, cc, fin)
    geom = ctx.last_geometry()
    if launches is not None:
        assert ctx.last_timing()[1] == launches, ctx.last_timing()
    ctx.close()
    return geom


CASES = [("cell", {}), ("cell", dict(soft=True)), ("sum32", {}), ("soft2", dict(n_soft=2)), ("soft2", dict(n_soft=4))]
IDS = ["cell", "cell-soft", "sum32", "soft2-2", "soft2-4"]


@pytest.mark.parametrize("shards,threads", [(1, 0), (3, 64)], ids=["one-shard", "three-shards"])
@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_inside_on_k_spread(name, kw, shards, threads):
    opts = dict(shards=shards)
    if threads:
        opts["force_threads"] = threads
    geom = _batch(_fx(name, False, **kw), _want(name, False, **kw), "k_spread", opts)
    assert geom["shards"] == shards, geom


@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_one_unit_across_on_k_schedule(name, kw):
    _batch(_fx(name, True, **kw), _want(name, True, **kw), "k_schedule", dict(shards=1))


@pytest.mark.parametrize("name,kw,per_chunk", [("cell", {}, 3), ("cell", dict(soft=True), 3), ("sum32", {}, 1), ("soft2", dict(n_soft=2), 2)],
                         ids=["cell", "cell-soft", "sum32", "soft2-2"])
def test_chunk_launches_hand_the_cells_over(name, kw, per_chunk):
    """Three launches (two for sum32's two pods): the resident cells, 65519 .. 65535, leave through the
    write-back and come back through the checked hand-off between launches."""
    fx = _fx(name, False, **kw)
    n_chunks = -(-fx[1].n // per_chunk)
    _batch(fx, _want(name, False, **kw), "k_spread", dict(shards=2, static_bytes=4 * fx[0].n_nodes * per_chunk), launches=2 * n_chunks)


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("name,kw", CASES[:3], ids=IDS[:3])
def test_fold_option(name, kw, fold):
    _batch(_fx(name, False, **kw), _want(name, False, **kw), "k_spread", dict(shards=3, force_threads=64, fold=fold))


def test_window_on_the_widened_fixture():
    """percentageOfNodesToScore 0 (adaptive) on 150 nodes: 100 feasible nodes end the search."""
    prof = abi.default_profile()
    prof.pct_nodes_to_score = 0
    for across, kernel in ((False, "k_spread"), (True, "k_schedule")):
        fx = _fx("cell", across, wide=144)
        want = _want("cell", across, prof=prof, wide=144)
        assert max(want[1].meta(j)["n_feasible"] for j in range(fx[1].n)) == 100
        _batch(fx, want, kernel, dict(shards=3), prof=prof)


def test_ports_and_images_form():
    for across, kernel in ((False, "k_spread"), (True, "k_schedule")):
        fx = _fx("cell", across, port=True)
        want = _want("cell", across, port=True)
        assert want[2]["port_used"].any()
        _batch(fx, want, kernel, dict(shards=2, spread_ports_images=1))


def _records_equal(got, res, j, N):
    np.testing.assert_array_equal(got.fail_plugin[:N], res.fail_plugin[j, :N], err_msg=f"pod {j} verdicts")
    m = res.meta(j)
    assert (got.chosen, got.n_feasible, got.scored, got.status) == (m["chosen"], m["n_feasible"], m["scored"], m["status"]), (j, m)
    if m["scored"]:
        feas = res.fail_plugin[j, :N] == 0
        np.testing.assert_array_equal(got.raw[:, :N][:, feas], res.raw[j][:, :N][:, feas], err_msg=f"pod {j} raw")
        np.testing.assert_array_equal(got.norm[:, :N][:, feas], res.norm[j][:, :N][:, feas], err_msg=f"pod {j} norm")
        np.testing.assert_array_equal(got.total[:N][feas], res.total[j, :N][feas], err_msg=f"pod {j} total")


@pytest.mark.parametrize("across", [False, True], ids=["inside", "across"])
@pytest.mark.parametrize("name", ["cell", "sum32"])
def test_per_pod_path_and_recorded_batch(name, across):
    cc, cp, exp = _fx(name, across)
    ch_o, res, fin = _want(name, across)
    N = cc.n_nodes
    prof = abi.default_profile()
    ctx = native.Context(prof, max_pods_record=cp.n)
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n, record=True)
    assert ctx.last_kernel() == "k_schedule"
    np.testing.assert_array_equal(chosen, ch_o)
    for j in range(cp.n):
        _records_equal(ctx.fetch_record(j), res, j, N)
    _state_equal(ctx, cc, fin)
    ctx.reset()
    for j in range(cp.n):
        r = ctx.eval_pod(cp.as_struct(), j)
        _records_equal(r, res, j, N)
        if r.chosen >= 0:
            ctx.commit(cp.as_struct(), j, int(r.chosen))
    _state_equal(ctx, cc, fin)
    ctx.close()
