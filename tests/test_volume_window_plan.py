"""Host-only routing of windowed batches with volume programs (kss_plan_podset_ex, no GPU needed):
with simple_ports_images, simple_volumes and simple_volumes_window all on, a batch of k_simple's
volumes form whose search is windowed (percentageOfNodesToScore below 100 on a node list long enough
to stop early) is planned on k_simple; with simple_volumes_window 0 it stays on k_schedule with the
reason it had.  A list too short for a window is unaffected either way, and every refusal of the form
still names its own reason under the window."""
import pytest

import volume_fixtures as vf
import volume_form_fixtures as vff
import volume_fuzz
from kss import abi, native
from kss.compile import compile_cluster

ELIGIBLE = {"kernel": "k_simple", "pod": -1, "reason": "eligible"}


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


_CACHE = {}


def _compile(key, made=None):
    if key not in _CACHE:
        nodes, bound, pods, st = made() if made else volume_fuzz.make(*key)
        _CACHE[key] = compile_cluster(nodes, bound, pods, storage=st)[:2]
    return _CACHE[key]


def _prof(pct):
    p = abi.default_profile()
    p.pct_nodes_to_score = pct
    return p


def _on(window):
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    native.set_option("simple_volumes_window", window)


def _plan(cc, cp, pct):
    return native.plan_podset(cc.as_struct(), cp.as_struct(), _prof(pct))


def test_option_defaults_to_off():
    assert native.get_option("simple_volumes_window") == 0


@pytest.mark.parametrize("pct", [0, 30, 100])
def test_window_routing_follows_the_option(pct):
    cc, cp = _compile((11, 300, 300, 200))
    first = min(i for i in range(cp.n) if cp.pods[i]["vol_len"] > 0)
    _on(1)
    assert _plan(cc, cp, pct) == ELIGIBLE
    _on(0)
    plan = _plan(cc, cp, pct)
    if pct == 100:
        assert plan == ELIGIBLE
    else:
        assert plan["kernel"] == "k_schedule" and plan["pod"] == first, plan
        assert "percentageOfNodesToScore" in plan["reason"] and "volume" in plan["reason"], plan


@pytest.mark.parametrize("pi,vol", [(0, 0), (1, 0), (0, 1)])
def test_window_option_alone_changes_nothing(pi, vol):
    """simple_volumes_window is effective only with the two options of the form."""
    cc, cp = _compile((11, 300, 300, 200))
    native.set_option("simple_ports_images", pi)
    native.set_option("simple_volumes", vol)
    off = _plan(cc, cp, 0)
    native.set_option("simple_volumes_window", 1)
    assert off["kernel"] == "k_schedule" and _plan(cc, cp, 0) == off, off


@pytest.mark.parametrize("pct", [0, 30])
@pytest.mark.parametrize("window", [0, 1])
def test_short_list_is_unaffected(pct, window):
    """40 nodes: numFeasibleNodesToFind is the whole list, there is no window to run."""
    cc, cp = _compile((31, 40, 30, 120))
    _on(window)
    assert _plan(cc, cp, pct) == ELIGIBLE


# every refusal of the form, on clusters above 100 nodes at pct 0 and 30 (k_find 100 < N)
def _many_keys():
    nodes, bound, pods, st = vff.private_ebs(n_nodes=130)
    names = ["d%d.csi.example" % i for i in range(9)]
    st["csinodes"].append({"metadata": {"name": "n1"},
                           "spec": {"drivers": [{"name": d, "allocatable": {"count": 4}} for d in names]}})
    st["pvs"] += [vf.pv("pv-d%d" % i, vf.csi(d, "h%d" % i)) for i, d in enumerate(names)]
    st["pvcs"] += [vf.pvc("c-d%d" % i, "pv-d%d" % i) for i in range(9)]
    return nodes, bound, pods + [vf.vpod("many", *[vf.claim("c-d%d" % i) for i in range(9)])], st


@pytest.mark.parametrize("pct", [0, 30])
def test_refusals_keep_their_reasons_under_the_window(pct):
    _on(1)
    # WaitForFirstConsumer
    cc, cp = _compile(("wffc", 130), lambda: volume_fuzz.make(2, n_nodes=130, n_bound=100, n_pods=60, wffc=True))
    wffc = [i for i in range(cp.n) for e in range(int(cp.pods[i]["vol_len"]))
            if int(cp.vols[int(cp.pods[i]["vol_off"]) + e]["kind"]) == abi.KSS_VOL_BIND_WFFC]
    assert wffc
    plan = _plan(cc, cp, pct)
    assert plan["kernel"] == "k_schedule" and "WaitForFirstConsumer" in plan["reason"] and plan["pod"] == wffc[0], plan
    # 70 rows
    cc, cp = _compile((5, 100, 120, 300))
    assert cc.as_struct().n_vol_rows == 70
    cc, cp = _compile((5, 130, 120, 300))
    assert cc.as_struct().n_vol_rows > 64
    plan = _plan(cc, cp, pct)
    first = min(i for i in range(cp.n) if cp.pods[i]["vol_len"] > 0)
    assert plan["kernel"] == "k_schedule" and "64" in plan["reason"] and plan["pod"] == first, plan
    # more than 8 limit keys
    cc, cp = _compile("many-keys", _many_keys)
    assert cc.as_struct().n_vol_keys > 8 and cc.n_nodes == 130
    plan = _plan(cc, cp, pct)
    assert plan["kernel"] == "k_schedule" and "8 attach-limit keys" in plan["reason"], plan


@pytest.mark.parametrize("pct", [0, 30])
def test_counter_overflow_keeps_its_reason_under_the_window(pct):
    cc, cp = _compile(("private", 130), lambda: vff.private_ebs(n_nodes=130))
    K = cc.as_struct().n_vol_keys
    (k,) = [k for k in range(K) if cc.arrays["vol_key_plugin"][k] == abi.KSS_F_EBS_LIMITS]
    adds = sum(vff.pod_masks(cc, cp, j)[5][k] for j in range(cp.n))
    _on(1)
    old = int(cc.arrays["vol_attached"][k][3])
    try:
        cc.arrays["vol_attached"][k][3] = 65534 - adds
        assert _plan(cc, cp, pct) == ELIGIBLE
        cc.arrays["vol_attached"][k][3] = 65534 - adds + 1
        plan = _plan(cc, cp, pct)
        assert plan["kernel"] == "k_schedule" and "key %d" % k in plan["reason"] and "65534" in plan["reason"], plan
    finally:
        cc.arrays["vol_attached"][k][3] = old
