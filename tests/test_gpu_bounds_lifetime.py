"""The fast kernels' value bounds across a context's life: a sequence of calls on ONE context, every
step against the C oracle continued from the previous step's state (fixtures:
tests/value_edge_fixtures.py lifetime_cases / witness_cases, tests/count_edge_fixtures.py).

test_gpu_value_envelope.py and test_gpu_count_envelope.py pin each bound for the first batch after
kss_load_cluster.  Here the state has moved since the load -- by a batch, kss_commit, the service's
commit, the node axis, kss_apply_node_delta / kss_apply_count_delta -- and the host must still keep
k_simple / k_spread / the service's k_simple-shaped chain off values they cannot hold.

The contract asserted is two-sided and fixes no particular way of tracking:
  never fast when outside      if the true device state (read back before the step) plus the step's
                               n * max commit is at or across a bound, the step does not report
                               k_simple / k_spread / service mode 1
  stay fast when surely inside if even the conservative figure -- the load-time maximum, plus every
                               committed step's n * max commit, plus every delta since -- is inside,
                               the step stays on the fast kernel
Steps in between are compared with the oracle only.  (n * max commit of a batch is over its whole
podset; of kss_commit / service_commit / a node-axis pod, that pod's own largest commit.)

The f64 sum bound (max Requested + n * max commit < 2^52, the same for NonZeroRequested): sequences
1 two batches, 2 kss_commit then a batch, 3 service_commit then a batch, 4 a batch then the service,
5 node deltas, 6 reset and reload, 7 the node axis (world 1) then a batch, 8 the wrong-value witness
(five one-pod batches take an odd Requested past 2^53 under a profile without the NodeResourcesFit
filter).  k_spread's count bounds (a cell <= 65535, MAXK * ref_weight * total < 2^31 - 1): batch
then batch, kss_commit / service_commit of pods with own term rows, kss_apply_count_delta in both
modes, reset."""
import copy

import numpy as np
import pytest

import count_edge_fixtures as cx
import oracle_c
import value_edge_fixtures as vx
from kss import abi, native, nodeaxis
from kss.compile import compile_cluster

pytestmark = pytest.mark.gpu

N_PAIRS = 64
E52 = 1 << 52
FAST = ("k_simple", "k_spread")
STATE = ("requested", "nonzero", "pod_count", "class_count", "term_count", "port_used")
_CACHE = {}


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _compiled(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _twin(batches):
    """(cc, [cp of batch 0, cp of batch 1 (the same pods under other names), ...], cp of one large pod)
    of lifetime_cases(N_PAIRS, batches)."""
    def make():
        nodes, bound, pods = vx.twin_cluster(vx.lifetime_cases(N_PAIRS, batches))
        cc, cp0, _ = compile_cluster(nodes, bound, pods)
        cps = [cp0] + [compile_cluster(nodes, bound, vx.renamed(pods, "-%d" % k))[1] for k in (1, 2)]
        big = {"metadata": {"name": "big", "namespace": "default", "labels": {"app": "big"}},
               "spec": {"containers": [{"name": "c", "resources": {"requests": vx._requests(vx.POD_SIZES[3])}}]}}
        return cc, cps, compile_cluster(nodes, bound, [big])[1]
    return _compiled(("twin", batches), make)


# --------------------------------------------------------------------------------------
# the oracle, continued; the two-sided contract
# --------------------------------------------------------------------------------------
def _state0(cc):
    N = cc.n_nodes
    a = cc.arrays
    st = {k: np.array(a[k][..., :N], copy=True) for k in STATE}
    if st["port_used"].shape[0] < N:  # no host ports anywhere: the compiled column is a placeholder
        st["port_used"] = np.zeros(N, np.uint64)
    for k in ("class_count", "term_count"):  # ... no class / term rows
        if st[k].ndim == 1:
            st[k] = np.zeros((1, N), np.int32)
    return st


def _with_state(cc, st):
    """cc with its mutable columns replaced by st (a copy; cc itself is shared and never written)."""
    c2 = copy.copy(cc)
    c2.arrays = dict(cc.arrays)
    N = cc.n_nodes
    for k in STATE:
        v = np.array(cc.arrays[k], copy=True)
        s = st[k]
        if v.ndim == 2:
            r = min(v.shape[0], s.shape[0])
            v[:r, :N] = s[:r, :N]
        elif v.shape[0] >= N:
            v[:N] = s[:N]
        c2.arrays[k] = v
    return c2


def _oracle_step(prof, cc, st, cp, threads=1):
    """(chosen, results, state after) of one batch on state st."""
    c2 = _with_state(cc, st)
    ch, res, fin = oracle_c.schedule(prof, c2.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record=True, threads=threads,
                                     n_classes=len(cc.classes), n_terms=len(cc.terms))
    return ch, res, {k: fin[k] for k in STATE}


def _commit_state(cc, st, cp, j, node):
    """AssumePod of pod j on `node`, in integers: the state after kss_commit / service_commit."""
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    p = cp.pods[j]
    for r in range(abi.KSS_NRES):
        out["requested"][r, node] += int(p["commit_req"][r])
    for r in range(2):
        out["nonzero"][r, node] += int(p["commit_nz"][r])
    out["pod_count"][node] += 1
    if int(p["cls"]) >= 0:
        out["class_count"][int(p["cls"]), node] += 1
    for t in cp.ints[int(p["own_terms_off"]):int(p["own_terms_off"]) + int(p["own_terms_len"])]:
        out["term_count"][int(t), node] += 1
    return out


def _max_commit(cp, j=None):
    """(largest Requested delta, largest NonZeroRequested delta) of a podset, or of its pod j."""
    p = cp.pods if j is None else cp.pods[j:j + 1]
    return int(p["commit_req"][:, :3].max()), int(p["commit_nz"].max())


def _own_mult(cp, j=None):
    """(most own term rows of a pod, most commits one pod adds to one count row) of a podset / its pod j."""
    own, mult = 0, 1
    for p in (cp.pods if j is None else cp.pods[j:j + 1]):
        ids = [int(x) for x in cp.ints[int(p["own_terms_off"]):int(p["own_terms_off"]) + int(p["own_terms_len"])]]
        own, mult = max(own, len(ids)), max([mult] + [ids.count(i) for i in ids])
    return own, mult


def _count_figures(st):
    """(max(sum of class counts, sum of term counts), the largest cell) of a state."""
    c, t = np.abs(st["class_count"].astype(np.int64)), np.abs(st["term_count"].astype(np.int64))
    return max(int(c.sum()), int(t.sum())), max(int(c.max()), int(t.max()))


class Life:
    """One context and both sides of the contract: the f64 sum bound, and with `needs`
    (count_edge_fixtures.spread_bounds) k_spread's count bounds."""

    def __init__(self, cc, prof=None, ctx=None, needs=None):
        self.cc, self.prof, self.needs = cc, prof or abi.default_profile(), needs
        self.ctx = ctx or native.Context(self.prof)
        if ctx is None:
            self.ctx.load(cc.as_struct())
        self.late = []
        self.loaded()

    def loaded(self):
        self.st = _state0(self.cc)
        self.cons = [int(self.st["requested"][:3].max()), int(self.st["nonzero"].max())]  # the conservative figures
        self.cons_count = list(_count_figures(self.st))                                    # (total, cell)

    def region(self, cp, j=None):
        """'outside' / 'inside' / None for a batch of cp, or the commit of its pod j."""
        n, commit, (own, mult) = (cp.n if j is None else 1), _max_commit(cp, j), _own_mult(cp, j)
        g = self.ctx.node_state()
        N = self.cc.n_nodes
        true = [int(g["requested"][:3, :N].max()), int(g["nonzero"][:, :N].max())]
        outside = any(t + n * c >= E52 for t, c in zip(true, commit))
        inside = all(t + n * c < E52 for t, c in zip(self.cons, commit))
        if self.needs is not None:
            g = {k: g[k][:len(rows), :N] for k, rows in (("class_count", self.cc.classes), ("term_count", self.cc.terms))}
            total, cell = _count_figures(g)
            outside |= not cx.spread_bounds(self.needs, total + n * (1 + own), cell + n * mult, N)[0]
            inside &= cx.spread_bounds(self.needs, self.cons_count[0] + n * (1 + own), self.cons_count[1] + n * mult, N)[0]
        return "outside" if outside else ("inside" if inside else None)

    def committed(self, cp, j=None):
        n, commit, (own, mult) = (cp.n if j is None else 1), _max_commit(cp, j), _own_mult(cp, j)
        self.cons = [t + n * c for t, c in zip(self.cons, commit)]
        # (one committed pod adds its class and its own term rows: at most 1 + own to the sums and to a cell)
        self.cons_count = [self.cons_count[0] + n * (1 + own), self.cons_count[1] + (n * mult if j is None else 1 + own)]

    def check_state(self):
        N = self.cc.n_nodes
        g = self.ctx.node_state()
        for k in ("requested", "nonzero", "pod_count"):
            np.testing.assert_array_equal(g[k][..., :N], self.st[k][..., :N], err_msg=k)
        for k, n in (("class_count", len(self.cc.classes)), ("term_count", len(self.cc.terms))):
            np.testing.assert_array_equal(g[k][:n, :N], self.st[k][:n, :N], err_msg=k)
        np.testing.assert_array_equal(self.ctx.port_state(), self.st["port_used"][:N])

    def batch(self, cp, fast="k_simple", want_region=None, strict=True):
        """One batch: the kernel by the region, everything else against the oracle continued.  strict
        False: a kernel outside the contract is noted in self.late and the sequence goes on (the
        witness: what the values then do is the point)."""
        region = self.region(cp)
        if want_region is not None:
            assert region == want_region[0], (region, want_region)
        ch_o, res, fin = _oracle_step(self.prof, self.cc, self.st, cp)
        chosen = self.ctx.schedule_batch(cp.as_struct(), cp.n)
        kernel = self.ctx.last_kernel()
        np.testing.assert_array_equal(chosen, ch_o)
        _meta_equal(self.ctx.fetch_meta(cp.n), res, cp.n)
        self.st = fin
        self.committed(cp)
        self.check_state()
        # (the values first: a wrong value is the graver finding, and the kernel's name explains it)
        bad = None
        if region == "outside" and kernel in FAST:
            bad = (kernel, "the true state plus n * max commit is across the bound")
        if region == "inside" and kernel != fast:
            bad = (kernel, "even the conservative figure is inside the bound")
        if bad and not strict:
            self.late.append(bad)
        else:
            assert not bad, bad
        return kernel

    def commit(self, cp, j, node, service=False):
        if service:
            self.ctx.stage(cp.as_struct())
            self.ctx.service_commit(j, node)
            self.ctx.service_stop()
        else:
            self.ctx.commit(cp.as_struct(), j, node)
        self.st = _commit_state(self.cc, self.st, cp, j, node)
        self.committed(cp, j)
        self.check_state()

    def service(self, cp):
        """Every pod of cp through service_eval + service_commit; the chain by the region."""
        region = self.region(cp)
        ch_o, res, fin = _oracle_step(self.prof, self.cc, self.st, cp)
        svc, N = self.ctx, self.cc.n_nodes
        svc.stage(cp.as_struct())
        svc.service_start()
        mode = svc.service_mode()
        if region == "outside":
            assert mode == 0, (mode, "the true state plus n * max commit is across the bound")
        if region == "inside":
            assert mode == 1, (mode, "even the conservative figure is inside the bound")
        for j in range(cp.n):
            got = svc.service_eval(j)
            m = res.meta(j)
            assert (got.chosen, got.n_feasible, got.scored, got.status) == (m["chosen"], m["n_feasible"], m["scored"], m["status"]), (j, m)
            np.testing.assert_array_equal(got.fail_plugin[:N], res.fail_plugin[j, :N], err_msg=f"pod {j}")
            if m["scored"]:
                assert got.best_total == m["best_total"], j
                feas = res.fail_plugin[j, :N] == 0
                np.testing.assert_array_equal(got.total[:N][feas], res.total[j, :N][feas], err_msg=f"pod {j} total")
            if got.chosen >= 0:
                svc.service_commit(j, got.chosen)
        svc.service_stop()
        self.st = fin
        self.committed(cp)
        self.check_state()
        return mode

    def delta(self, rows, requested, nonzero):
        """kss_apply_node_delta of whole rows (pod counts kept)."""
        rows = list(rows)
        req = np.zeros((len(rows), abi.KSS_NRES), np.int64)
        nz = np.zeros((len(rows), 2), np.int64)
        for i, (r, q, z) in enumerate(zip(rows, requested, nonzero)):
            req[i, :3], nz[i] = q, z
            self.st["requested"][:, r] = req[i]
            self.st["nonzero"][:, r] = nz[i]
            self.cons = [max(self.cons[0], max(q)), max(self.cons[1], max(z))]
        self.ctx.apply_node_delta(rows, req, nz, self.st["pod_count"][rows])
        self.check_state()

    def count_delta(self, node, row, value, overwrite=False):
        """kss_apply_count_delta on one cell (row: a class row, or n_classes + a term row)."""
        nc = len(self.cc.classes)
        col = self.st["class_count"] if row < nc else self.st["term_count"]
        r = row if row < nc else row - nc
        col[r, node] = value if overwrite else col[r, node] + value
        self.cons_count[0] += max(value, 0)
        self.cons_count[1] = max(self.cons_count[1], value) if overwrite else self.cons_count[1] + max(value, 0)
        self.ctx.apply_count_delta([node], [row], [value], overwrite=overwrite)
        self.check_state()

    def close(self):
        self.ctx.close()


def _meta_equal(meta, res, n):
    for j in range(n):
        m = res.meta(j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], (j, int(meta[j, 4]), m)


def _top_node(cc):
    """The node holding the snapshot's largest cpu Requested (near-bound-0's first twin)."""
    return int(np.argmax(cc.arrays["requested"][0, :cc.n_nodes]))


# --------------------------------------------------------------------------------------
# the f64 sum bound
# --------------------------------------------------------------------------------------
def test_1_two_batches():
    """sum-in twice: the first batch's best-effort pods land on the near-bound nodes and raise their
    NonZeroRequested, so the second batch meets a true maximum across the bound.  With the slack of two
    batches both stay on k_simple; a third is between the regions (the oracle alone judges it)."""
    cc, cps, _ = _twin(1)
    life = Life(cc)
    assert life.batch(cps[0], want_region=("inside",)) == "k_simple"
    assert life.batch(cps[1], want_region=("outside",)) == "k_schedule"
    life.close()
    cc, cps, _ = _twin(2)
    life = Life(cc)
    life.batch(cps[0], want_region=("inside",))
    life.batch(cps[1], want_region=("inside",))
    life.batch(cps[2], want_region=(None,))
    life.close()


@pytest.mark.parametrize("service", [False, True], ids=["kss_commit", "service_commit"])
def test_2_3_commit_then_a_batch(service):
    """One large pod committed (kss_commit; the service's commit and service_stop) onto the node with
    the largest Requested, then sum-in: across.  With one batch of slack: k_simple."""
    cc, cps, big = _twin(1)
    life = Life(cc)
    life.commit(big, 0, _top_node(cc), service=service)
    assert life.batch(cps[0], want_region=("outside",)) == "k_schedule"
    life.close()
    cc, cps, big = _twin(2)
    life = Life(cc)
    life.commit(big, 0, _top_node(cc), service=service)
    assert life.batch(cps[0], want_region=("inside",)) == "k_simple"
    life.close()


def test_4_batch_then_the_service():
    cc, cps, _ = _twin(1)
    life = Life(cc)
    life.batch(cps[0], want_region=("inside",))
    assert life.region(cps[1]) == "outside"
    assert life.service(cps[1]) == 0
    life.close()
    cc, cps, _ = _twin(2)
    life = Life(cc)
    life.batch(cps[0], want_region=("inside",))
    assert life.region(cps[1]) == "inside"
    assert life.service(cps[1]) == 1
    life.close()


def test_5_node_deltas():
    """A delta raises one row to 2^52 - n * max commit (one unit across), then lowers it again: the
    first batch leaves k_simple; the second may stay off it (only the oracle judges it)."""
    cc, cps, _ = _twin(2)
    life = Life(cc)
    n, (creq, cnz) = cps[0].n, _max_commit(cps[0])
    row = cc.node_names.index("a000")
    was = ([int(v) for v in life.st["requested"][:3, row]], [int(v) for v in life.st["nonzero"][:, row]])
    life.delta([row], [[E52 - n * creq, was[0][1], was[0][2]]], [was[1]])
    assert life.batch(cps[0], want_region=("outside",)) == "k_schedule"
    now = ([int(v) for v in life.st["requested"][:3, row]], [int(v) for v in life.st["nonzero"][:, row]])
    life.delta([row], [[was[0][0], now[0][1], now[0][2]]], [now[1]])
    life.batch(cps[1], want_region=(None,))
    life.close()


def test_6_reset_and_reload():
    """reset(): the snapshot's bounds hold again, sum-in runs on k_simple as on a fresh context; the
    same after load() of a second, smaller cluster."""
    cc, cps, big = _twin(1)
    life = Life(cc)
    life.batch(cps[0], want_region=("inside",))
    life.batch(cps[1], want_region=("outside",))
    life.ctx.reset()
    life.loaded()
    life.check_state()
    assert life.batch(cps[0], want_region=("inside",)) == "k_simple"
    life.ctx.reset()
    life.loaded()
    life.commit(big, 0, _top_node(cc))
    life.ctx.reset()
    life.loaded()
    assert life.batch(cps[2], want_region=("inside",)) == "k_simple"
    # a second, smaller cluster on the same context
    cc2, cp2 = _compiled("small", lambda: compile_cluster(*vx.twin_cluster(vx.make_cases(N_PAIRS)[:8]))[:2])
    life.ctx.load(cc2.as_struct())
    small = Life(cc2, ctx=life.ctx)
    assert small.batch(cp2, want_region=("inside",)) == "k_simple"
    life.close()


def test_7_node_axis_then_a_batch():
    """The node axis (world 1) commits pod by pod through kss_axis_commit; then a batch."""
    for batches, region, kernel in ((1, "outside", "k_schedule"), (2, "inside", "k_simple")):
        cc, cps, _ = _twin(batches)
        prof = abi.default_profile()
        ch_o, res, fin = _oracle_step(prof, cc, _state0(cc), cps[0])
        sch = nodeaxis.NodeAxisScheduler(cc.as_struct(), cps[0].as_struct(), prof, device=0)
        chosen = sch.schedule().cpu().numpy()
        np.testing.assert_array_equal(chosen, ch_o)
        life = Life(cc, prof, ctx=sch.ctx)
        life.st = fin
        for j in range(cps[0].n):
            life.committed(cps[0], j)
        life.check_state()
        assert life.batch(cps[1], want_region=(region,)) == kernel
        sch.close()


def test_8_wrong_value_witness():
    """Without the NodeResourcesFit filter one pod with an odd request near 2^51 lands five times on a
    node whose Requested is odd and near 2^51: Requested passes 2^53 on an odd value, which a double
    cannot hold.  After every run it equals the Python-integer sum (and the oracle's int64)."""
    def make():
        nodes, bound, pods = vx.twin_cluster(vx.witness_cases())
        cc, cp, _ = compile_cluster(nodes, bound, pods)
        return cc, cp
    cc, cp = _compiled("witness", make)
    prof = abi.default_profile()
    prof.filter_enabled &= ~(1 << abi.KSS_F_NODE_RESOURCES_FIT)
    life = Life(cc, prof)
    a = cc.node_names.index("a000")
    for run in range(1, 6):
        life.batch(cp, want_region=("inside" if run == 1 else "outside",), strict=False)
        got = int(life.ctx.node_state()["requested"][0, a])
        assert got == vx.witness_requested(run), (run, got - vx.witness_requested(run))
    assert not life.late, life.late
    life.close()


# --------------------------------------------------------------------------------------
# k_spread's count bounds (the cell fixture: its largest cell is the term row of n00)
# --------------------------------------------------------------------------------------
CELL_NEEDS = dict(ref_weight=cx.CELL_REF)


def _cell(batches):
    """(cc, [cp, the same pods under two other names], the term cell's (node, row)) of the cell fixture
    with room for `batches` batches: the term cell of n00 holds 65535 - batches * 16."""
    def make():
        nodes, bound, pods = cx.cell_objects()
        cc, cp0, _ = compile_cluster(nodes, bound, pods)
        fill = cx.cell_fill(cc, False, batches)
        cps = [cp0] + [compile_cluster(nodes, bound, vx.renamed(pods, "-%d" % k))[1] for k in (1, 2)]
        return cc, cps, (cc.node_names.index("n00"), len(cc.classes) + fill["term"])
    return _compiled(("cell", batches), make)


def test_count_batch_then_batch():
    """The first batch takes the term cell of n00 to exactly 65535 on k_spread; the second would take a
    16-bit cell past it and must leave k_spread.  With room for two, both stay."""
    cc, cps, _ = _cell(1)
    life = Life(cc, needs=CELL_NEEDS)
    assert life.batch(cps[0], fast="k_spread", want_region=("inside",)) == "k_spread"
    assert int(life.st["term_count"].max()) == cx.CELL_MAX
    assert life.batch(cps[1], fast="k_spread", want_region=("outside",)) == "k_schedule"
    life.close()
    cc, cps, _ = _cell(2)
    life = Life(cc, needs=CELL_NEEDS)
    life.batch(cps[0], fast="k_spread", want_region=("inside",))
    life.batch(cps[1], fast="k_spread", want_region=("inside",))
    life.batch(cps[2], fast="k_spread")  # (whichever region the second batch's landings leave it in)
    life.close()


@pytest.mark.parametrize("service", [False, True], ids=["kss_commit", "service_commit"])
def test_count_commit_then_a_batch(service):
    """A pod with two identical own term rows committed onto n00 (+2 on the full cell), then the batch."""
    for batches, region, kernel in ((1, "outside", "k_schedule"), (2, "inside", "k_spread")):
        cc, cps, (n00, _row) = _cell(batches)
        life = Life(cc, needs=CELL_NEEDS)
        life.commit(cps[1], 0, n00, service=service)
        assert life.batch(cps[0], fast="k_spread", want_region=(region,)) == kernel
        life.close()


def test_count_deltas_and_reset():
    """kss_apply_count_delta on the term cell of n00 (65503 at the load, a batch adds at most 16):
    mode 0 +16 (the batch ends on exactly 65535: k_spread), reset, +17 (65536: not k_spread), -17 (the
    oracle alone judges: the host may stay conservative); mode 1 to 65519 (k_spread), to 65535 and to
    65536 (neither fits with a batch's commits, and 65536 no 16-bit cell at all); reset(): the snapshot's bounds hold again."""
    cc, cps, (n00, row) = _cell(2)
    life = Life(cc, needs=CELL_NEEDS)
    t0 = cx.CELL_MAX - 32
    assert int(life.st["term_count"].max()) == t0

    def again():
        life.ctx.reset()
        life.loaded()
        life.check_state()
    life.count_delta(n00, row, 16)
    assert life.batch(cps[0], fast="k_spread", want_region=("inside",)) == "k_spread"
    assert int(life.st["term_count"].max()) == cx.CELL_MAX
    again()
    life.count_delta(n00, row, 17)
    assert life.batch(cps[0], fast="k_spread", want_region=("outside",)) == "k_schedule"
    again()
    life.count_delta(n00, row, 17)
    life.count_delta(n00, row, -17)
    life.batch(cps[0], fast="k_spread", want_region=(None,))
    for value, region, kernel in ((cx.CELL_MAX - 16, "inside", "k_spread"), (cx.CELL_MAX, "outside", "k_schedule"),
                                  (cx.CELL_MAX + 1, "outside", "k_schedule")):
        again()
        life.count_delta(n00, row, value, overwrite=True)
        assert life.batch(cps[1], fast="k_spread", want_region=(region,)) == kernel
    again()
    assert life.batch(cps[2], fast="k_spread", want_region=("inside",)) == "k_spread"
    life.close()
