"""Host-only routing of batches with volume programs (kss_plan_podset, no GPU needed): with the
options simple_ports_images and simple_volumes both on, a batch whose pods hold volume programs is
planned on k_simple (its volumes form) when the form can restate it -- no WaitForFirstConsumer
claim, at most 64 volume rows and 8 limit keys, packed 16-bit counters that cannot overflow; else,
and with either option off, it stays on k_schedule with a reason; a batch without volume programs
is planned exactly as before."""
import pytest

import progfuzz
import volume_fixtures as vf
import volume_form_fixtures as vff
import volume_fuzz
from kss import abi, native
from kss.compile import compile_cluster

OLD_REASON = "host ports (NodePorts), node-cached images (ImageLocality) or volumes: k_schedule only"


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
    native.set_option("simple_ports_images", 1)
    native.set_option("simple_volumes", 1)


def test_both_options_on_takes_k_simple():
    cc, cp = _compile(volume_fuzz.make(31, 40, 30, 120))
    assert any(cp.pods[i]["vol_len"] > 0 for i in range(cp.n))
    _on()
    assert _plan(cc, cp) == {"kernel": "k_simple", "pod": -1, "reason": "eligible"}


@pytest.mark.parametrize("pi,vol", [(0, 0), (1, 0), (0, 1)])
def test_either_option_off_keeps_k_schedule(pi, vol):
    cc, cp = _compile(volume_fuzz.make(31, 40, 30, 120))
    native.set_option("simple_ports_images", pi)
    native.set_option("simple_volumes", vol)
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and plan["reason"] == OLD_REASON, plan


def test_seventy_rows_refused():
    cc, cp = _compile(volume_fuzz.make(5, 100, 120, 300))
    assert cc.as_struct().n_vol_rows == 70
    _on()
    plan = _plan(cc, cp)
    first = min(i for i in range(cp.n) if cp.pods[i]["vol_len"] > 0)
    assert plan["kernel"] == "k_schedule" and "64" in plan["reason"] and plan["pod"] == first, plan


def test_sixty_four_rows_admitted():
    cc, cp = _compile(volume_fuzz.make(11, 300, 300, 200))
    assert cc.as_struct().n_vol_rows == 64
    _on()
    assert _plan(cc, cp)["kernel"] == "k_simple"


def test_wait_for_first_consumer_refused():
    cc, cp = _compile(volume_fuzz.make(2, wffc=True))
    wffc = [i for i in range(cp.n) for e in range(int(cp.pods[i]["vol_len"]))
            if int(cp.vols[int(cp.pods[i]["vol_off"]) + e]["kind"]) == abi.KSS_VOL_BIND_WFFC]
    assert len(wffc) == 20
    _on()
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and "WaitForFirstConsumer" in plan["reason"] and plan["pod"] == wffc[0], plan


def test_more_than_eight_keys_refused():
    """One pod with claims on volumes of nine CSI drivers, which a node limits: with EBS, ten limit keys."""
    nodes, bound, pods, st = vff.private_ebs()
    names = ["d%d.csi.example" % i for i in range(9)]
    st["csinodes"].append({"metadata": {"name": "n1"},
                           "spec": {"drivers": [{"name": d, "allocatable": {"count": 4}} for d in names]}})
    st["pvs"] += [vf.pv("pv-d%d" % i, vf.csi(d, "h%d" % i)) for i, d in enumerate(names)]
    st["pvcs"] += [vf.pvc("c-d%d" % i, "pv-d%d" % i) for i in range(9)]
    pods = pods + [vf.vpod("many", *[vf.claim("c-d%d" % i) for i in range(9)])]
    cc, cp, _ = compile_cluster(nodes, bound, pods, storage=st)
    assert cc.as_struct().n_vol_keys > 8, cc.as_struct().n_vol_keys
    _on()
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and "8 attach-limit keys" in plan["reason"], plan


def test_packed_counter_overflow():
    """The private-volume cluster: 16 pods can each add one volume under the EBS key, so a loaded
    attached count of 65534 - 16 still fits the 16-bit field (65535 means "not limited") and one more
    does not; a limit above 65534 does not fit either."""
    cc, cp = _compile(vff.private_ebs())
    K = cc.as_struct().n_vol_keys
    ebs = [k for k in range(K) if cc.arrays["vol_key_plugin"][k] == abi.KSS_F_EBS_LIMITS]
    assert len(ebs) == 1
    k = ebs[0]
    adds = sum(vff.pod_masks(cc, cp, j)[5][k] for j in range(cp.n))
    assert adds == 16
    _on()
    cc.arrays["vol_attached"][k][3] = 65534 - adds
    assert _plan(cc, cp)["kernel"] == "k_simple"
    cc.arrays["vol_attached"][k][3] = 65534 - adds + 1
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and "key %d" % k in plan["reason"] and "65534" in plan["reason"], plan
    cc.arrays["vol_attached"][k][3] = 0
    cc.arrays["vol_limit"][k][2] = 65534
    assert _plan(cc, cp)["kernel"] == "k_simple"
    cc.arrays["vol_limit"][k][2] = 65535
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and "key %d" % k in plan["reason"], plan


def test_shared_entry_under_another_key_refused():
    """kss/volumes.py always lists a shared volume under its row's key; an entry that does not is
    refused with a reason of its own."""
    cc, cp = _compile(volume_fuzz.make(31, 40, 30, 120))
    rowkey = cc.arrays["vol_row_key"]
    K = cc.as_struct().n_vol_keys
    hit = None
    for e in range(len(cp.vols)):
        v = cp.vols[e]
        if int(v["kind"]) == abi.KSS_VOL_LIMIT and int(v["row"]) >= 0:
            hit = e
            break
    assert hit is not None and K >= 2
    _on()
    assert _plan(cc, cp)["kernel"] == "k_simple"
    cp.vols[hit]["key"] = (int(rowkey[int(cp.vols[hit]["row"])]) + 1) % K
    plan = _plan(cc, cp)
    assert plan["kernel"] == "k_schedule" and "another limit key" in plan["reason"], plan


def test_window_keeps_k_schedule():
    """No window instantiation of the form: under percentageOfNodesToScore < 100, on a node list long
    enough to stop early, the batch stays on k_schedule."""
    cc, cp = _compile(volume_fuzz.make(11, 300, 300, 200))
    _on()
    prof = abi.default_profile()
    assert _plan(cc, cp, prof)["kernel"] == "k_simple"
    prof.pct_nodes_to_score = 30
    plan = _plan(cc, cp, prof)
    assert plan["kernel"] == "k_schedule" and "percentageOfNodesToScore" in plan["reason"] and "volume" in plan["reason"], plan


def test_batch_without_volume_programs_is_planned_as_before():
    nodes, bound, pods = progfuzz.make(2, 60, 200, programs=False)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    assert not any(cp.pods[i]["vol_len"] > 0 for i in range(cp.n))
    native.set_option("simple_ports_images", 1)
    off = native.plan_podset(cc.as_struct(), cp.as_struct())
    ids_off, n_off = native.plan_shapes(cp.as_struct(), len(cc.scalars))
    native.set_option("simple_volumes", 1)
    on = native.plan_podset(cc.as_struct(), cp.as_struct())
    ids_on, n_on = native.plan_shapes(cp.as_struct(), len(cc.scalars))
    assert off["kernel"] == "k_simple" and on == off
    assert n_on == n_off and list(ids_on) == list(ids_off)
