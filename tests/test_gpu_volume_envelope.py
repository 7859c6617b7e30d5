"""The volumes forms on limit keys 4-7 and on 16-bit fields at their edges (tests/volume_edge_fixtures.py),
against the C oracle, bit for bit: chosen nodes, every pod's outcome, the node rows, vol_count /
vol_attached and UsedPorts.  k_simple's form (simple_volumes), its window (simple_volumes_window),
k_spread's form (spread_volumes, the same fixtures with a ScheduleAnyway zone constraint on every other
pod), the sweep form (sweep_volumes) and a context's life (vol_pack_state on the current columns).
Every case in a form also runs with the form's option off, on k_schedule, for the same results; every
across variant must leave the form and still equal the oracle.

Before a case touches the device it asserts on the oracle's own records (volume_form_fixtures.reach)
that keys 4, 5, 6 and 7 each decide a limit failure and an H1 pair, and where the literals apply that
the oracle equals the hand-derived expectations."""
import copy
import ctypes as C

import numpy as np
import pytest

import oracle_c
import volume_edge_fixtures as vef
import volume_form_fixtures as vff
import volume_fuzz
from kss import abi, native
from kss.compile import compile_cluster
from test_volume_envelope import ACROSS, INSIDE, assert_hand_derived, assert_upper_keys_decide

pytestmark = pytest.mark.gpu
MODES = {"single": abi.KSS_SCHED_FORCE_SINGLE_WG, "multi": abi.KSS_SCHED_FORCE_MULTI_WG}
ALL_INSIDE = [None] + INSIDE  # None: eight_keys itself
SOME = [None, ("limit_top", None), ("carry", (32767, False)), ("carry", (255, True))]


def _id(v):
    return "eight_keys" if v is None else vef.variant_id(v)


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _oracle(cc, cp, prof=None, n=None):
    return oracle_c.schedule(prof or abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n if n is None else n,
                             cc.n_nodes, record=True, n_classes=len(cc.classes), n_terms=len(cc.terms))


_CACHE = {}


def _case(v, soft=False, wide=False):
    """(cc, cp, oracle chosen, records, final state, across) of eight_keys (v None) or a field_tops
    variant, computed once and shared (nothing writes to them); its reach is asserted here."""
    key = (v, soft, wide)
    if key not in _CACHE:
        if v is None:
            fx = vef.eight_keys(soft=soft, wide=wide)
            cc, cp = vef.compiled(fx)
            t = dict(across=None, expect=fx["expect"], final=fx["final"])
        else:
            t = vef.field_tops(*v, soft=soft, wide=wide)
            cc, cp = t["cc"], t["cp"]
        ch_o, res, fin = _oracle(cc, cp)
        r = vff.reach(cc, cp, ch_o, res)
        if t["expect"] is not None:
            assert_hand_derived(cc, cp, ch_o, res, fin, t["expect"], t["final"])
            assert_upper_keys_decide(r)
        _CACHE[key] = (cc, cp, ch_o, res, fin, t["across"])
    return _CACHE[key]


def _meta_equal(meta, res, n, first=0):
    for j in range(n):
        m = res.meta(first + j)
        got = dict(chosen=meta[j, 0], n_feasible=meta[j, 1], scored=meta[j, 2], status=meta[j, 3])
        assert got == {k: m[k] for k in got}, (first + j, got, m)
        if m["scored"]:
            assert meta[j, 4] == m["best_total"], first + j


def _state_equal(ctx, cc, fin, cursor=False):
    N = cc.n_nodes
    g = ctx.node_state()
    np.testing.assert_array_equal(g["requested"][:, :N], fin["requested"][:, :N])
    np.testing.assert_array_equal(g["nonzero"][:, :N], fin["nonzero"][:, :N])
    np.testing.assert_array_equal(g["pod_count"][:N], fin["pod_count"][:N])
    for k, n in (("class_count", len(cc.classes)), ("term_count", len(cc.terms))):
        if n:
            np.testing.assert_array_equal(g[k][:n], fin[k][:n])
    vc, va = ctx.volume_state()
    np.testing.assert_array_equal(vc, fin["vol_count"])
    np.testing.assert_array_equal(va, fin["vol_attached"])
    np.testing.assert_array_equal(ctx.port_state(), fin["port_used"][:N])
    if cursor:
        assert ctx.next_start_node_index() == fin["next_start"]


def _ran(ctx, family, form):
    """The kernel and form the last batch reports: family "simple" / "spread" in its volumes form, or
    k_schedule with both forms' reports zero."""
    fs, fg = ctx.last_simple_form(), ctx.last_spread_form()
    if not form:
        assert ctx.last_kernel() == "k_schedule" and fs == {"volumes": 0, "lds_bytes": 0} and fg == (0, 0), (ctx.last_kernel(), fs, fg)
    elif family == "simple":
        assert ctx.last_kernel() == "k_simple" and fs["volumes"] == 1 and fs["lds_bytes"] > 0, (ctx.last_kernel(), fs)
    else:
        assert ctx.last_kernel() == "k_spread" and fg[0] == 2 and fg[1] > 0, (ctx.last_kernel(), fg)


def _run(case, family, form, prof=None, flags=0, cursor=False):
    cc, cp, ch_o, res, fin = case[:5]
    ctx = native.Context(prof or abi.default_profile())
    ctx.load(cc.as_struct())
    chosen = ctx.schedule_batch(cp.as_struct(), cp.n, flags=flags)
    _ran(ctx, family, form)
    np.testing.assert_array_equal(chosen, ch_o)
    _meta_equal(ctx.fetch_meta(cp.n), res, cp.n)
    _state_equal(ctx, cc, fin, cursor=cursor)
    info = dict(ctx.last_geometry(), xcd_local=ctx.last_xcd_local()["used"], launches=ctx.last_timing()[1])
    ctx.close()
    return info


OPTS = {"simple": ("simple_ports_images", "simple_volumes"), "spread": ("spread_ports_images", "spread_volumes")}


def _both(case, family, prof=None, flags=0, cursor=False, inside=True):
    """The form (an across case: k_schedule although the options are on), then the option off."""
    pi, vol = OPTS[family]
    native.set_option(pi, 1)
    native.set_option(vol, 1)
    info = _run(case, family, inside, prof=prof, flags=flags, cursor=cursor)
    native.set_option(vol, 0)
    _run(case, family, False, prof=prof, flags=flags, cursor=cursor)
    return info


# --------------------------------------------------------------------------------------
# 1. k_simple's form: every inside variant on 1 (forced single workgroup), 2 and 3 shards
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards,xcd", [(1, 0), (2, 1), (2, 0), (3, 1), (3, 0)], ids=["wg1", "2-xcd", "2-plain", "3-xcd", "3-plain"])
@pytest.mark.parametrize("v", ALL_INSIDE, ids=_id)
def test_simple_shards(v, shards, xcd):
    case = _case(v)
    native.set_option("xcd", xcd)
    if shards > 1 and xcd:
        native.set_option("nodes_per_shard", vef.N_NODES // shards)
    else:
        native.set_option("shards", shards)
    info = _both(case, "simple", flags=abi.KSS_SCHED_FORCE_SINGLE_WG if shards == 1 else 0)
    assert info["shards"] == shards and info["xcd_local"] == xcd, info


@pytest.mark.parametrize("v", SOME, ids=_id)
def test_simple_slots_per_lane(v):
    """The widened copy (150 nodes) on one 64-lane workgroup: three slots per lane."""
    case = _case(v, wide=True)
    native.set_option("shards", 1)
    native.set_option("force_threads", 64)
    info = _both(case, "simple")
    assert info["shards"] == 1 and info["threads"] == 64 and info["nodes_per_lane"] > 1, info


@pytest.mark.parametrize("v", SOME, ids=_id)
def test_simple_chunks(v):
    """Twelve pods per chunk: the packed words near the top pass from launch to launch."""
    case = _case(v)
    native.set_option("shards", 3)
    native.set_option("static_bytes", 4 * case[0].n_nodes * 12)
    info = _both(case, "simple")
    assert info["launches"] >= 2 * 3, info


def _profile(off):
    p = abi.default_profile()
    for f in off:
        p.filter_enabled &= ~(1 << f)
    return p


@pytest.mark.parametrize("name,off,keys", [("no-csi", (abi.KSS_F_NODE_VOLUME_LIMITS,), (2, 3, 4, 5, 6)),
                                           ("no-azure", (abi.KSS_F_AZURE_DISK_LIMITS,), (7,))])
@pytest.mark.parametrize("v", [None, ("limit_top", None)], ids=_id)
def test_simple_runtime_profile(v, name, off, keys):
    """A limit plugin disabled (key_on clears upper-word bits): its verdict disappears, its keys' pods
    are all bound and their counters still advance -- past the limit -- while the other upper-word
    plugin still decides."""
    cc, cp = _case(v)[:2]
    prof = _profile(off)
    ch_o, res, fin = _oracle(cc, cp, prof)
    r = vff.reach(cc, cp, ch_o, res, prof)
    N = cc.n_nodes
    fails = set(int(x) for x in np.unique(res.fail_plugin[:, :N]))
    assert not fails & set(off), fails
    assert fails & {abi.KSS_F_NODE_VOLUME_LIMITS, abi.KSS_F_AZURE_DISK_LIMITS} and r["h1"] > 0, (fails, r["h1"])
    for k in keys:  # p3 is bound now (and d5 / d7): past the limit
        assert int(fin["vol_attached"][k][vef.G[k]]) == int(cc.arrays["vol_limit"][k][vef.G[k]]) + (2 if k in (5, 7) else 1)
    native.set_option("shards", 2)
    _both((cc, cp, ch_o, res, fin), "simple", prof=prof)


@pytest.mark.parametrize("v", ACROSS, ids=vef.variant_id)
def test_simple_across_runs_k_schedule(v):
    case = _case(v)
    assert case[5] is not None
    native.set_option("shards", 2)
    _both(case, "simple", inside=False)


# --------------------------------------------------------------------------------------
# 2. the window: eight_keys unpinned and widened to 150 nodes
# --------------------------------------------------------------------------------------
def _window_case(pct, soft=False):
    key = ("window", pct, soft)
    if key not in _CACHE:
        fx = vef.eight_keys(pin=False, wide=True, soft=soft)
        cc, cp = vef.compiled(fx)
        prof = abi.default_profile()
        prof.pct_nodes_to_score = pct
        ch_o, res, fin = _oracle(cc, cp, prof)
        r = vff.reach(cc, cp, ch_o, res)
        N = cc.n_nodes
        assert N == 150 and all(res.meta(j)["n_feasible"] == 100 for j in range(cp.n))  # every search stops early
        upper = {k for j, n, k in r["limit_failures"] if k >= 4}
        assert upper == {4, 5, 6, 7}, upper  # upper-word limit failures on visited nodes
        assert fin["next_start"] not in (0, N)
        _CACHE[key] = (cc, cp, ch_o, res, fin, None, prof)
    return _CACHE[key]


@pytest.mark.parametrize("geom", ["whole-workgroup", "per-wave"])
@pytest.mark.parametrize("pct", [30, 0])
def test_simple_window(pct, geom):
    case = _window_case(pct)
    prof = case[6]
    if geom == "whole-workgroup":
        native.set_option("shards", 1)
        native.set_option("force_threads", 64)
    else:
        native.set_option("shards", 3)
        native.set_option("force_threads", 128)
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    native.set_option("simple_volumes_window", 1)
    info = _run(case, "simple", True, prof=prof, cursor=True)
    assert info["threads"] == (64 if geom == "whole-workgroup" else 128), info
    native.set_option("simple_volumes_window", 0)
    _run(case, "simple", False, prof=prof, cursor=True)


# --------------------------------------------------------------------------------------
# 3. k_spread's form
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,shards", [("single", 1), ("multi", 0), ("auto", 3)])
@pytest.mark.parametrize("v", ALL_INSIDE, ids=_id)
def test_spread_modes(v, mode, shards):
    case = _case(v, soft=True)
    plain = _case(v)
    np.testing.assert_array_equal(case[2], plain[2])  # the pins decide: the choices are the plain fixture's
    np.testing.assert_array_equal(case[4]["vol_attached"], plain[4]["vol_attached"])
    native.set_option("shards", shards)
    info = _both(case, "spread", flags=MODES.get(mode, 0))
    assert (info["shards"] == shards) if shards else (info["shards"] > 1), info


@pytest.mark.parametrize("v", SOME, ids=_id)
def test_spread_chunks_fold_off(v):
    """Twelve pods per chunk, the statistics fold off (the form's condition, set here explicitly): the
    packed columns go through the checked hand-off."""
    case = _case(v, soft=True)
    native.set_option("shards", 3)
    native.set_option("fold", 0)
    native.set_option("static_bytes", 4 * case[0].n_nodes * 12)
    info = _both(case, "spread")
    chunks = (case[1].n + 11) // 12
    assert chunks >= 3 and info["launches"] >= 3 * chunks, info  # k_static_pi + k_static_vol + k_spread_vol per chunk


@pytest.mark.parametrize("pct", [30, 0])
def test_spread_window(pct):
    case = _window_case(pct, soft=True)
    native.set_option("shards", 3)
    _both(case, "spread", prof=case[6], cursor=True)


@pytest.mark.parametrize("v", ACROSS, ids=vef.variant_id)
def test_spread_across_runs_k_schedule(v):
    case = _case(v, soft=True)
    assert case[5] is not None
    native.set_option("shards", 3)
    _both(case, "spread", inside=False)


# --------------------------------------------------------------------------------------
# 4. the sweep form
# --------------------------------------------------------------------------------------
def _plain_scenario():
    if "plain" not in _CACHE:
        nodes, bound, pods, st = volume_fuzz.make(2, n_nodes=12, n_bound=16, n_pods=40)
        cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
        _CACHE["plain"] = (cc, cp) + tuple(_oracle(cc, cp)) + (None,)
    return _CACHE["plain"]


@pytest.mark.parametrize("middle", [("limit_top", None)] + [("limit_top", k) for k in (4, 7)], ids=vef.variant_id)
def test_sweep(middle):
    """A plain fuzz scenario, limit_top (inside, or across under an upper-word key) and carry; two runs
    (the second shows the columns restored), every scenario against the oracle."""
    scen = [_plain_scenario(), _case(middle), _case(("carry", (32767, False)))]
    native.set_option("sweep_ports_images", 1)
    native.set_option("sweep_volumes", 1)
    clusters, podsets = [s[0].as_struct() for s in scen], [s[1].as_struct() for s in scen]
    plan = native.plan_sweep(abi.default_profile(), clusters, podsets, detail=True)
    sw = native.Sweep(abi.default_profile(), clusters, podsets)
    info = sw.info()
    inside = scen[1][5] is None
    assert plan["kernel"] == info["kernel"] == ("k_simple" if inside else "k_schedule") and info["volumes"], (plan, info)
    if inside:
        assert plan["form"] is True and plan["reason"] == "eligible", plan
    else:
        assert plan["scenario"] == 1 and "key %d" % scen[1][5] in plan["reason"], plan
    first = None
    for rep in range(2):
        chosen, _ = sw.run()
        o = 0
        for s, c in enumerate(scen):
            np.testing.assert_array_equal(chosen[o:o + c[1].n], c[2], err_msg=f"run {rep}, scenario {s}")
            o += c[1].n
        assert o == len(chosen)
        first = chosen.copy() if first is None else first
        np.testing.assert_array_equal(chosen, first)
    sw.close()


# --------------------------------------------------------------------------------------
# 5. a context's life: the form is admitted on the current columns
# --------------------------------------------------------------------------------------
STATE = ("requested", "nonzero", "pod_count", "class_count", "term_count", "vol_count", "vol_attached", "port_used")


def _with_state(cc, st):
    """cc with its mutable columns replaced by a previous step's final state (a copy)."""
    c2 = copy.copy(cc)
    c2.arrays = dict(cc.arrays)
    N = cc.n_nodes
    for k in STATE:
        v = np.array(cc.arrays[k], copy=True)
        s = np.asarray(st[k])
        if v.ndim == 2:
            r = min(v.shape[0], s.shape[0])
            v[:r, :N] = s[:r, :N]
        elif v.shape[0] >= N:
            v[:N] = s[:N]
        c2.arrays[k] = v
    return c2


def _slice(ps, first, n):
    tail = abi.PodSet.from_buffer_copy(ps)
    tail.pods = C.cast(C.addressof(ps.pods.contents) + first * C.sizeof(abi.Pod), C.POINTER(abi.Pod))
    tail.n_pods = n
    return tail


class _Life:
    def __init__(self, fx):
        self.cc, self.cp, self.slices = fx["cc"], fx["cp"], fx["slices"]
        self.ps = self.cp.as_struct()
        self.prof = abi.default_profile()
        self.ctx = native.Context(self.prof)
        self.ctx.load(self.cc.as_struct())
        self.loaded()

    def loaded(self):
        N = self.cc.n_nodes
        self.st = {k: np.array(self.cc.arrays[k], copy=True) for k in STATE}
        if self.st["port_used"].shape[0] < N:  # no host ports anywhere: the compiled column is a placeholder
            self.st["port_used"] = np.zeros(N, np.uint64)
        assert self.cc.classes and not self.cc.terms

    def key6(self):
        return int(self.ctx.volume_state()[1][vef.LIFE_KEY][vef.LIFE_NODE])

    def batch(self, name, form, ends):
        first, n = self.slices[name]
        c2 = _with_state(self.cc, self.st)
        tail = _slice(self.ps, first, n)
        ch_o, res, fin = oracle_c.schedule(self.prof, c2.as_struct(), tail, n, self.cc.n_nodes, record=True,
                                           n_classes=len(self.cc.classes), n_terms=len(self.cc.terms))
        chosen = self.ctx.schedule_batch(tail, n)
        _ran(self.ctx, "simple", form)
        np.testing.assert_array_equal(chosen, ch_o)
        _meta_equal(self.ctx.fetch_meta(n), res, n)
        self.st = {k: fin[k] for k in STATE}
        self.check(ends)

    def check(self, ends):
        _state_equal(self.ctx, self.cc, self.st)
        assert self.key6() == ends == int(self.st["vol_attached"][vef.LIFE_KEY][vef.LIFE_NODE])

    def commit_pod(self, name, ends):
        """kss_commit of the slice's one pod on n23 (AssumePod: its private volume is attached)."""
        first, n = self.slices[name]
        assert n == 1
        self.ctx.commit(self.ps, first, vef.LIFE_NODE)
        self.st = {k: np.array(v, copy=True) for k, v in self.st.items()}
        self.st["vol_attached"][vef.LIFE_KEY][vef.LIFE_NODE] += 1
        self.st["pod_count"][vef.LIFE_NODE] += 1
        p = self.cp.pods[first]
        self.st["class_count"][int(p["cls"]), vef.LIFE_NODE] += 1
        for r in range(abi.KSS_NRES):
            self.st["requested"][r, vef.LIFE_NODE] += int(p["commit_req"][r])
        for r in range(2):
            self.st["nonzero"][r, vef.LIFE_NODE] += int(p["commit_nz"][r])
        self.check(ends)


@pytest.mark.parametrize("across_by", ["batch", "kss_commit"])
def test_lifetime(across_by):
    """One context.  A ends one below the top on key 6, B ends on it in the form, C (a batch, or
    kss_commit of its pod) takes the count across; D touches keys 0-3 only and must still be refused the
    form -- a form run would pack the clamped 65534 and write it back; a delta takes the count back and
    the form is admitted again; reset() restores the load-time figures, and A runs in the form again."""
    top = vef.FIELD_MAX
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    native.set_option("shards", 3)
    life = _Life(vef.lifetime())
    assert life.key6() == vef.LIFE_LOAD == top - 4
    life.batch("A", True, top - 1)
    life.batch("B", True, top)
    if across_by == "batch":
        life.batch("C", False, top + 1)
    else:
        life.commit_pod("C", top + 1)
    life.batch("D", False, top + 1)
    R = life.cc.as_struct().n_vol_rows
    life.ctx.apply_volume_delta([vef.LIFE_NODE], [R + vef.LIFE_KEY], [top - 1], overwrite=True)
    life.st["vol_attached"] = np.array(life.st["vol_attached"], copy=True)
    life.st["vol_attached"][vef.LIFE_KEY][vef.LIFE_NODE] = top - 1
    life.check(top - 1)
    life.batch("E", True, top)
    life.ctx.reset()
    life.loaded()
    life.check(vef.LIFE_LOAD)
    life.batch("A", True, top - 1)
    life.ctx.close()
