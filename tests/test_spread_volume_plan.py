"""Host-only routing of batches WITH programs whose pods hold volume programs (kss_plan_podset, no GPU
needed): with the options spread_ports_images and spread_volumes both on, such a batch is planned on
k_spread (its volumes form) when the form can restate it -- no WaitForFirstConsumer claim, at most 64
volume rows and 8 limit keys, packed 16-bit counters that cannot overflow, no statistics fold,
preferred NodeAffinity weights within 13 bits; else, and with either option off, it stays on
k_schedule with a reason that names the limit and the first offending pod; a batch without volume
pods is planned exactly as before."""
import copy

import pytest

import spread_portimage_fuzz as spf
import spread_volume_fuzz as svf
import volume_fixtures as vf
import volume_form_fixtures as vff
import volume_fuzz
from kss import abi, native
from kss.compile import compile_cluster

OLD_REASON = "host ports (NodePorts), node-cached images (ImageLocality) or volumes: k_schedule only"
ELIGIBLE = {"kernel": "k_spread", "pod": -1, "reason": "eligible"}


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _compile(made):
    nodes, bound, pods, st = made
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    return cc, cp


def _plan(cc, cp, profile=None):
    return native.plan_podset(cc.as_struct(), cp.as_struct(), profile)


def _on():
    native.set_option("spread_ports_images", 1)
    native.set_option("spread_volumes", 1)


def _first_vol(cp):
    return min(i for i in range(cp.n) if cp.pods[i]["vol_len"] > 0)


def _weights(pods, j, total):
    """Pod j prefers every node twice over: two terms whose weights sum to `total`."""
    pods = copy.deepcopy(pods)
    pref = {"matchExpressions": [{"key": "kubernetes.io/hostname", "operator": "Exists"}]}
    na = pods[j]["spec"].setdefault("affinity", {}).setdefault("nodeAffinity", {})
    na["preferredDuringSchedulingIgnoredDuringExecution"] = [
        {"weight": total - 100, "preference": pref}, {"weight": 100, "preference": pref}]
    return pods


def test_option_exists_and_defaults_off():
    assert native.get_option("spread_volumes") == 0
    native.set_option("spread_volumes", 1)
    assert native.get_option("spread_volumes") == 1
    native.reset_options()
    assert native.get_option("spread_volumes") == 0


def test_ports_images_option_alone_keeps_todays_reason():
    cc, cp = _compile(svf.make(1, 60, 200))
    native.set_option("spread_ports_images", 1)
    plan = _plan(cc, cp)
    assert plan == {"kernel": "k_schedule", "pod": _first_vol(cp), "reason": OLD_REASON}, plan


def test_both_options_on_takes_k_spread():
    cc, cp = _compile(svf.make(1, 60, 200))
    assert any(cp.pods[i]["vol_len"] > 0 for i in range(cp.n))
    assert any(cp.pods[i]["n_hard"] or cp.pods[i]["n_soft"] or cp.pods[i]["ipa_len"] for i in range(cp.n))
    _on()
    assert _plan(cc, cp) == ELIGIBLE


def test_spread_volumes_alone_is_not_effective():
    cc, cp = _compile(svf.make(1, 60, 200))
    native.set_option("spread_volumes", 1)
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and plan["reason"] == OLD_REASON, plan


def test_simple_volumes_does_not_enable_it():
    cc, cp = _compile(svf.make(1, 60, 200))
    native.set_option("spread_ports_images", 1)
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and "k_spread" not in plan["reason"], plan
    native.set_option("spread_volumes", 1)  # ... and the two do not depend on each other
    native.set_option("simple_volumes", 0)
    assert _plan(cc, cp) == ELIGIBLE


def test_wait_for_first_consumer_refused():
    """volume_fuzz's WaitForFirstConsumer storage grafted on a program batch: pod 5 claims w-0."""
    nodes, bound, pods = spf.make(1, 60, 200)
    st = volume_fuzz.make(2, wffc=True)[3]
    pods[5]["spec"]["volumes"] = [dict(vf.claim("w-0"), name="v0")]
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    kinds = [int(cp.vols[int(cp.pods[5]["vol_off"]) + e]["kind"]) for e in range(int(cp.pods[5]["vol_len"]))]
    assert abi.KSS_VOL_BIND_WFFC in kinds
    _on()
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and plan["pod"] == 5, plan
    assert "WaitForFirstConsumer" in plan["reason"] and "k_spread" in plan["reason"], plan


def test_row_limit():
    """Wider pools of shared claims and inline disks: 64 rows are admitted, more are refused."""
    cc, cp = _compile(svf.make(*ROWS_64[0], **ROWS_64[1]))
    assert cc.as_struct().n_vol_rows == 64
    _on()
    assert _plan(cc, cp) == ELIGIBLE
    cc, cp = _compile(svf.make(*ROWS_65[0], **ROWS_65[1]))
    assert cc.as_struct().n_vol_rows == 65
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and plan["pod"] == _first_vol(cp), plan
    assert "64 volume rows" in plan["reason"] and "k_spread" in plan["reason"], plan


# (seed, nodes, pods), pools: found by a search over the pools' sizes
ROWS_64 = ((20, 211, 150), dict(n_claims=28, n_ebs=18, n_gce=9))
ROWS_65 = ((20, 211, 150), dict(n_claims=28, n_ebs=18, n_gce=8))


def test_more_than_eight_keys_refused():
    """One more pod with claims on volumes of nine CSI drivers, which a node limits."""
    nodes, bound, pods, st = svf.make(1, 60, 200)
    names = ["d%d.csi.example" % i for i in range(9)]
    limited = {c["metadata"]["name"] for c in st["csinodes"]}
    free = next(nd["metadata"]["name"] for nd in nodes if nd["metadata"]["name"] not in limited)
    st["csinodes"].append({"metadata": {"name": free},
                           "spec": {"drivers": [{"name": d, "allocatable": {"count": 4}} for d in names]}})
    st["pvs"] += [vf.pv("pv-d%d" % i, vf.csi(d, "h%d" % i)) for i, d in enumerate(names)]
    st["pvcs"] += [vf.pvc("c-d%d" % i, "pv-d%d" % i) for i in range(9)]
    pods = pods + [vf.vpod("many", *[vf.claim("c-d%d" % i) for i in range(9)])]
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    assert cc.as_struct().n_vol_keys > 8, cc.as_struct().n_vol_keys
    _on()
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and plan["pod"] == _first_vol(cp), plan
    assert "8 attach-limit keys" in plan["reason"] and "k_spread" in plan["reason"], plan


def test_packed_counter_overflow():
    """Per key, the loaded attached count plus everything the batch can add must stay below 65535 (which
    means "not limited"), and so must every limit."""
    cc, cp = _compile(svf.make(1, 60, 200))
    K = cc.as_struct().n_vol_keys
    k = [k for k in range(K) if cc.arrays["vol_key_plugin"][k] == abi.KSS_F_EBS_LIMITS][0]
    rowkey = cc.arrays["vol_row_key"]
    adds = 0  # what vol_form_admit counts: per pod, its own rows of the key (once each) and its private counts
    for j in range(cp.n):
        own, padd = vff.pod_masks(cc, cp, j)[2], vff.pod_masks(cc, cp, j)[5]
        adds += sum(1 for r in range(cc.as_struct().n_vol_rows) if (own >> r) & 1 and int(rowkey[r]) == k) + padd[k]
    assert adds > 0
    _on()
    cc.arrays["vol_attached"][k][3] = 65534 - adds
    assert _plan(cc, cp) == ELIGIBLE
    cc.arrays["vol_attached"][k][3] = 65534 - adds + 1
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and plan["pod"] == _first_vol(cp), plan
    assert "key %d" % k in plan["reason"] and "65534" in plan["reason"] and "k_spread" in plan["reason"], plan
    cc.arrays["vol_attached"][k][3] = 0
    cc.arrays["vol_limit"][k][2] = 65535
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and "key %d" % k in plan["reason"], plan


def test_fold_keeps_the_batch_off_k_spread():
    """No statistics fold in the form: with fold = 1 the batch is refused as with the options off."""
    cc, cp = _compile(svf.make(1, 60, 200))
    _on()
    native.set_option("fold", 1)
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and plan["reason"] == OLD_REASON, plan


def test_node_affinity_weight_limit():
    nodes, bound, pods, st = svf.make(1, 60, 200)
    _on()
    cc, cp, _ = compile_cluster(nodes, bound, _weights(pods, 3, 8192), storage=st)
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and plan["pod"] == 3, plan
    assert "8191" in plan["reason"] and "k_spread" in plan["reason"], plan
    cc, cp, _ = compile_cluster(nodes, bound, _weights(pods, 3, 8191), storage=st)
    assert _plan(cc, cp) == ELIGIBLE


def test_window():
    """The form runs the window under the same option, by k_spread's own window rules: default profile,
    no PreFilterResult node list."""
    prof = abi.default_profile()
    prof.pct_nodes_to_score = 0
    _on()
    cc, cp = _compile(svf.make(2, 300, 300, names_lists=False))
    assert not any(cp.pods[i]["names_len"] >= 0 for i in range(cp.n))
    assert _plan(cc, cp, prof) == ELIGIBLE
    cc, cp = _compile(svf.make(2, 300, 300, names_lists=True))
    names = [i for i in range(cp.n) if cp.pods[i]["names_len"] >= 0]
    plan = _plan(cc, cp, prof)
    assert plan["kernel"] == "k_schedule" and plan["pod"] == names[0] and "percentageOfNodesToScore" in plan["reason"], plan


def test_batch_without_volume_pods_is_planned_as_before():
    for grafted in (True, False):
        cc, cp, _ = compile_cluster(*spf.make(1, 60, 200, grafted=grafted))
        assert not any(cp.pods[i]["vol_len"] > 0 for i in range(cp.n))
        native.set_option("spread_ports_images", 1)
        native.set_option("spread_volumes", 0)
        off = _plan(cc, cp)
        native.set_option("spread_volumes", 1)
        assert off["kernel"] == "k_spread" and _plan(cc, cp) == off
