"""Host-only routing of scenario sweeps whose pods hold volume programs (kss_plan_sweep, no GPU
needed): with the options sweep_ports_images and sweep_volumes both on such a sweep is planned on the
k_simple family in the volumes form (form 2: k_static_pi + k_static_vol + k_simple_vol_sweep), or on
k_schedule over the packed volume columns when a scenario leaves the form (more than 64 rows, ...) or
the sweep leaves k_simple's conditions (the window, a scenario too large for the form's LDS); a
WaitForFirstConsumer claim refuses the sweep; with either option off a volume program refuses it as
before; a sweep without volume pods plans the same with the option on and off."""
import pytest

import portimage_fuzz
import volume_form_fixtures as vff
import volume_fuzz
from kss import abi, native
from kss.compile import compile_cluster

SMALL = [(2, 12, 16, 40), (31, 40, 30, 120), (7, 130, 100, 150), (11, 300, 300, 200)]
RAGGED = [(4, 3, 2, 20), (1, 37, 30, 151), (1, 64, 40, 151), (3, 513, 150, 150), (2, 700, 150, 151)]


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


_CACHE = {}


def _vol(key, **kw):
    ck = (key, tuple(sorted(kw.items())))
    if ck not in _CACHE:
        nodes, bound, pods, st = volume_fuzz.make(key[0], n_nodes=key[1], n_bound=key[2], n_pods=key[3], **kw)
        _CACHE[ck] = compile_cluster(nodes, bound, pods, storage=st)[:2]
    return _CACHE[ck]


def _pi(seed):
    if ("pi", seed) not in _CACHE:
        nodes, bound, pods = portimage_fuzz.make(seed)
        _CACHE[("pi", seed)] = compile_cluster(nodes, bound, pods)[:2]
    return _CACHE[("pi", seed)]


def _plan(scen, prof=None, detail=True):
    return native.plan_sweep(prof or abi.default_profile(), [cc.as_struct() for cc, _ in scen],
                             [cp.as_struct() for _, cp in scen], detail=detail)


def _on(pi=1, vol=1):
    native.set_option("sweep_ports_images", pi)
    native.set_option("sweep_volumes", vol)


def _first_vol_pod(cp):
    return min(i for i in range(cp.n) if cp.pods[i]["vol_len"] > 0)


def test_option_defaults_to_off_and_round_trips():
    assert native.get_option("sweep_volumes") == 0
    native.set_option("sweep_volumes", 1)
    assert native.get_option("sweep_volumes") == 1 and native.get_option("sweep_ports_images") == 0
    native.reset_options()
    assert native.get_option("sweep_volumes") == 0


@pytest.mark.parametrize("pi,vol", [(0, 0), (1, 0), (0, 1)])
def test_either_option_off_refuses(pi, vol):
    _on(pi, vol)
    with pytest.raises(native.KssError) as e:
        _plan([_vol(k) for k in SMALL])
    assert e.value.rc == -95 and "volume" in str(e.value), str(e.value)


@pytest.mark.parametrize("keys", [SMALL, RAGGED], ids=["small", "ragged"])
def test_both_on_takes_the_volumes_form(keys):
    scen = [_vol(k) for k in keys]
    assert all(any(cp.pods[i]["vol_len"] > 0 for i in range(cp.n)) for _, cp in scen)
    assert max(cc.as_struct().n_vol_rows for cc, _ in scen) <= 64
    _on()
    assert _plan(scen) == {"kernel": "k_simple", "form": True, "volumes": True, "scenario": -1, "pod": -1,
                           "reason": "eligible"}
    # without detail the dict is what it was
    assert _plan(scen, detail=False) == {"kernel": "k_simple", "form": True, "scenario": -1, "pod": -1, "reason": "eligible"}


def test_mixed_sweep_with_a_scenario_without_volumes():
    scen = [_vol(SMALL[0]), _pi(5), _vol(SMALL[1])]
    assert not any(scen[1][1].pods[i]["vol_len"] > 0 for i in range(scen[1][1].n))
    _on()
    plan = _plan(scen)
    assert plan["kernel"] == "k_simple" and plan["volumes"] and plan["reason"] == "eligible", plan


def test_wait_for_first_consumer_refuses():
    cc, cp = _vol((2, 12, 16, 40), wffc=True)
    assert any(int(cp.vols[int(cp.pods[i]["vol_off"]) + e]["kind"]) == abi.KSS_VOL_BIND_WFFC
               for i in range(cp.n) for e in range(int(cp.pods[i]["vol_len"])))
    _on()
    with pytest.raises(native.KssError) as e:
        _plan([_vol(SMALL[1]), (cc, cp)])
    assert e.value.rc == -95 and "WaitForFirstConsumer" in str(e.value), str(e.value)


def test_seventy_rows_demote_with_reason_scenario_and_pod():
    big = _vol((5, 100, 120, 300))
    assert big[0].as_struct().n_vol_rows == 70
    _on()
    plan = _plan([_vol(SMALL[0]), big, _vol(SMALL[1])])
    assert plan["kernel"] == "k_schedule" and plan["volumes"] and "64" in plan["reason"], plan
    assert (plan["scenario"], plan["pod"]) == (1, _first_vol_pod(big[1])), plan


def test_counter_overflow_demotes_from_the_scenarios_own_columns():
    """Condition 4 is evaluated on the host from the scenario's vol_attached / vol_limit."""
    nodes, bound, pods, st = vff.private_ebs()
    cc, cp = compile_cluster(nodes, bound, pods, storage=st)[:2]
    K = cc.as_struct().n_vol_keys
    (k,) = [k for k in range(K) if cc.arrays["vol_key_plugin"][k] == abi.KSS_F_EBS_LIMITS]
    adds = sum(vff.pod_masks(cc, cp, j)[5][k] for j in range(cp.n))
    _on()
    cc.arrays["vol_attached"][k][3] = 65534 - adds
    assert _plan([_vol(SMALL[0]), (cc, cp)])["kernel"] == "k_simple"
    cc.arrays["vol_attached"][k][3] = 65534 - adds + 1
    plan = _plan([_vol(SMALL[0]), (cc, cp)])
    assert plan["kernel"] == "k_schedule" and plan["scenario"] == 1 and "key %d" % k in plan["reason"], plan


def test_window_demotes():
    prof = abi.default_profile()
    prof.pct_nodes_to_score = 0
    _on()
    plan = _plan([_vol(k) for k in SMALL], prof)
    assert plan["kernel"] == "k_schedule" and plan["volumes"] and "percentageOfNodesToScore" in plan["reason"], plan


def test_thousand_nodes_demote_on_geometry():
    """180 B of LDS per node slot: 768 slots fit the form, a 1,000-node scenario does not."""
    big = _vol((4, 1000, 150, 150))
    assert big[0].as_struct().n_vol_rows == 62
    _on()
    plan = _plan([_vol(SMALL[0]), big])
    assert plan["kernel"] == "k_schedule" and plan["volumes"] and (plan["scenario"], plan["pod"]) == (-1, -1), plan
    assert "does not fit one workgroup's LDS" in plan["reason"], plan
    assert _plan([_vol(k) for k in RAGGED])["kernel"] == "k_simple"  # 700 nodes: 384 lanes x 2 slots


def test_sweep_without_volume_pods_plans_as_with_the_option_off():
    scen = [_pi(5), _pi(6)]
    native.set_option("sweep_ports_images", 1)
    off = _plan(scen)
    native.set_option("sweep_volumes", 1)
    assert _plan(scen) == off and off["kernel"] == "k_simple" and not off["volumes"], off
    syn = [native.Synth(2, 11 + k, n, 20) for k, n in enumerate((40, 64))]
    plans = []
    for on in (0, 1):
        native.set_option("sweep_volumes", on)
        plans.append(native.plan_sweep(abi.default_profile(), [x.cluster for x in syn], [x.pods for x in syn], detail=True))
    assert plans[0] == plans[1] and not plans[0]["form"], plans
