"""Host-only routing of scenario sweeps whose pods hold host ports (NodePorts) or node-cached images
(ImageLocality): kss_plan_sweep, no GPU needed.  The kernel and the form are one decision for the
whole sweep, because one launch serves every scenario.  With the option sweep_ports_images 0 such a
sweep is refused; with 1 it is planned on the k_simple family in the ports-and-images form, or on
k_schedule when one scenario leaves k_simple's conditions (a pod over the form's 13 bits of raw
NodeAffinity, a spread program, the percentageOfNodesToScore window); a volume program refuses the
sweep with either value; a sweep without such pods plans the same with the option on and off."""
import copy

import pytest

import portimage_fuzz
import volume_fixtures as vf
from kss import abi, native
from kss.compile import compile_cluster

ZONE = "topology.kubernetes.io/zone"


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _compiled(seed, edit=None, **kw):
    nodes, bound, pods = portimage_fuzz.make(seed, **kw)
    if edit:
        pods = copy.deepcopy(pods)
        edit(pods)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    return cc, cp


def _plan(scen, prof=None):
    return native.plan_sweep(prof or abi.default_profile(), [cc.as_struct() for cc, _ in scen],
                             [cp.as_struct() for _, cp in scen])


def _weights(pods, j, total):
    """Pod j prefers every node twice over: two terms whose weights sum to `total`."""
    pref = {"matchExpressions": [{"key": "kubernetes.io/hostname", "operator": "Exists"}]}
    pods[j]["spec"]["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
        {"weight": total - 100, "preference": pref}, {"weight": 100, "preference": pref}]}}


def _spread(pods, j):
    pods[j]["spec"]["topologySpreadConstraints"] = [
        {"maxSkew": 1, "topologyKey": ZONE, "whenUnsatisfiable": "ScheduleAnyway",
         "labelSelector": {"matchLabels": {"app": "p"}}}]


def _is_pi(p):
    return bool(p["port_conflict"] or p["port_add"] or p["img_len"] > 0)


def test_option_round_trip():
    assert native.get_option("sweep_ports_images") == 0
    native.set_option("sweep_ports_images", 1)
    assert native.get_option("sweep_ports_images") == 1
    for other in ("simple_ports_images", "table_images", "spread_ports_images", "service_ports_images"):
        assert native.get_option(other) == 0
    native.reset_options()
    assert native.get_option("sweep_ports_images") == 0


def test_option_off_refuses_and_names_ports_or_images():
    scen = [_compiled(5), _compiled(6)]
    with pytest.raises(native.KssError) as e:
        _plan(scen)
    assert e.value.rc == -95
    assert "host ports" in str(e.value) or "images" in str(e.value), str(e.value)


def test_the_other_options_do_not_move_the_sweep():
    for other in ("simple_ports_images", "table_images", "spread_ports_images", "service_ports_images"):
        native.set_option(other, 1)
    with pytest.raises(native.KssError):
        _plan([_compiled(5)])


def test_option_on_takes_the_simple_family_in_the_form():
    native.set_option("sweep_ports_images", 1)
    scen = [_compiled(5), _compiled(6), _compiled(7, n_nodes=37, n_bound=30, n_pods=40)]
    assert all(any(_is_pi(cp.pods[i]) for i in range(cp.n)) for _, cp in scen)
    plan = _plan(scen)
    assert plan == {"kernel": "k_simple", "form": True, "scenario": -1, "pod": -1, "reason": "eligible"}, plan


def test_synth_only_sweep_is_not_of_the_form_with_either_value():
    syn = [native.Synth(2, 11 + k, n, 20) for k, n in enumerate((40, 64))]
    for x in syn:
        for i in range(x.n_pods):
            p = x.pods.pods[i]
            assert not (p.port_conflict or p.port_add or p.img_len > 0)
    plans = []
    for on in (0, 1):
        native.set_option("sweep_ports_images", on)
        plans.append(native.plan_sweep(abi.default_profile(), [x.cluster for x in syn], [x.pods for x in syn]))
    assert plans[0] == {"kernel": "k_simple", "form": False, "scenario": -1, "pod": -1, "reason": "eligible"}, plans
    assert plans[1] == plans[0]


def test_node_affinity_weight_limit_names_scenario_and_pod():
    """The form keeps 13 bits of raw NodeAffinity: Σ preferred weights 8192 in one pod of one scenario
    puts the whole sweep on k_schedule; 8191 fits."""
    native.set_option("sweep_ports_images", 1)
    scen = [_compiled(5), _compiled(6, edit=lambda pods: _weights(pods, 3, 8192)), _compiled(7)]
    plan = _plan(scen)
    assert plan["kernel"] == "k_schedule" and plan["form"] and (plan["scenario"], plan["pod"]) == (1, 3), plan
    assert "8191" in plan["reason"], plan
    scen[1] = _compiled(6, edit=lambda pods: _weights(pods, 3, 8191))
    plan = _plan(scen)
    assert plan["kernel"] == "k_simple" and plan["form"] and plan["reason"] == "eligible", plan


def test_zone_spread_constraint_runs_on_k_schedule():
    native.set_option("sweep_ports_images", 1)
    scen = [_compiled(5), _compiled(6, edit=lambda pods: _spread(pods, 4))]
    assert scen[1][1].pods[4]["n_soft"] == 1
    plan = _plan(scen)
    assert plan["kernel"] == "k_schedule" and plan["form"] and (plan["scenario"], plan["pod"]) == (1, 4), plan
    assert "spread" in plan["reason"], plan


def test_window_runs_on_k_schedule():
    native.set_option("sweep_ports_images", 1)
    prof = abi.default_profile()
    prof.pct_nodes_to_score = 0
    plan = _plan([_compiled(5), _compiled(6)], prof)
    assert plan["kernel"] == "k_schedule" and plan["form"] and "percentageOfNodesToScore" in plan["reason"], plan


@pytest.mark.parametrize("on", [0, 1])
def test_volume_program_refuses_with_either_value(on):
    def edit(pods):
        pods[7]["spec"]["volumes"] = [dict(vf.gce("disk-1"), name="v0")]

    native.set_option("sweep_ports_images", on)
    scen = [_compiled(6), _compiled(5, edit=edit)]
    assert scen[1][1].pods[7]["vol_len"] > 0
    with pytest.raises(native.KssError) as e:
        _plan(scen[1:])
    assert e.value.rc == -95 and "volume" in str(e.value), str(e.value)
    if on:  # (with 0 the first scenario's ports and images already refuse)
        with pytest.raises(native.KssError) as e:
            _plan(scen)
        assert e.value.rc == -95 and "volume" in str(e.value), str(e.value)
