"""Host-only routing of NodePorts / ImageLocality pods on the service grid (kss_plan_service, no GPU
needed): with the option service_ports_images on, a staged list that holds a pod with host ports or
node-cached images is planned on the k_simple-shaped chain (its ports-and-images form); a volume
program, preferred NodeAffinity weights above the form's 13 bits, or the window over a
PreFilterResult list keep it on the general chain; the option is independent of simple_ports_images
in both directions, and a list without such pods plans the same with it on and off."""
import copy

import pytest

import portimage_fuzz
import progfuzz
from kss import abi, native
from kss.compile import compile_cluster


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _plan(nodes, bound, pods, prof=None):
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    return native.plan_service(cc.as_struct(), cp.as_struct(), prof), cc, cp


def _weights(pods, j, total):
    """Pod j prefers every node twice over: two terms whose weights sum to `total`."""
    pods = copy.deepcopy(pods)
    pref = {"matchExpressions": [{"key": "kubernetes.io/hostname", "operator": "Exists"}]}
    pods[j]["spec"]["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
        {"weight": total - 100, "preference": pref}, {"weight": 100, "preference": pref}]}}
    return pods


def test_option_off_keeps_the_general_chain():
    plan, _, cp = _plan(*portimage_fuzz.make(5))
    assert plan["chain"] == 0 and plan["pod"] >= 0, plan
    assert "host ports" in plan["reason"] and "images" in plan["reason"], plan
    p = cp.pods[plan["pod"]]  # the first pod of the list that holds a port or names an image
    assert p["port_conflict"] or p["port_add"] or p["img_len"] > 0


def test_option_on_takes_the_simple_chain():
    native.set_option("service_ports_images", 1)
    plan, _, cp = _plan(*portimage_fuzz.make(5))
    assert any(cp.pods[i]["port_conflict"] or cp.pods[i]["port_add"] for i in range(cp.n))
    assert any(cp.pods[i]["img_len"] > 0 for i in range(cp.n))
    assert plan == {"chain": 1, "pod": -1, "reason": "eligible"}, plan


def test_simple_ports_images_alone_does_not_move_the_service():
    native.set_option("simple_ports_images", 1)
    plan, _, _ = _plan(*portimage_fuzz.make(5))
    assert plan["chain"] == 0 and "host ports" in plan["reason"], plan


def test_service_option_alone_does_not_move_the_batch_plan():
    native.set_option("service_ports_images", 1)
    nodes, bound, pods = portimage_fuzz.make(5)
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    plan = native.plan_podset(cc.as_struct(), cp.as_struct())
    assert plan["kernel"] == "k_schedule" and "host ports" in plan["reason"], plan


def test_volume_program_keeps_the_general_chain():
    native.set_option("service_ports_images", 1)
    nodes, bound, pods = portimage_fuzz.make(5)
    pods[7]["spec"]["volumes"] = [{"name": "v0", "gcePersistentDisk": {"pdName": "disk-1"}}]
    plan, _, cp = _plan(nodes, bound, pods)
    assert cp.pods[7]["vol_len"] > 0
    assert plan["chain"] == 0 and plan["pod"] == 7 and "volume" in plan["reason"] and "service" in plan["reason"], plan


def test_node_affinity_weight_limit():
    """The form keeps 13 bits of raw NodeAffinity: Σ preferred weights 8191 fits, 8192 does not."""
    native.set_option("service_ports_images", 1)
    nodes, bound, pods = portimage_fuzz.make(5)
    plan, _, _ = _plan(nodes, bound, _weights(pods, 3, 8192))
    assert plan["chain"] == 0 and plan["pod"] == 3 and "8191" in plan["reason"] and "service" in plan["reason"], plan
    plan, _, _ = _plan(nodes, bound, _weights(pods, 3, 8191))
    assert plan == {"chain": 1, "pod": -1, "reason": "eligible"}, plan


def test_window_over_a_prefilter_result_list_keeps_the_general_chain():
    native.set_option("service_ports_images", 1)
    nodes, bound, pods = portimage_fuzz.make(5, n_nodes=120, n_bound=60, n_pods=30)
    pods = copy.deepcopy(pods)
    # a required matchFields term on metadata.name: NodeAffinity's PreFilterResult names the nodes
    pods[4]["spec"]["affinity"] = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {
        "nodeSelectorTerms": [{"matchFields": [{"key": "metadata.name", "operator": "In", "values": ["n03", "n17"]}]}]}}}
    prof = abi.default_profile()
    prof.pct_nodes_to_score = 0
    plan, cc, cp = _plan(nodes, bound, pods, prof)
    assert cc.n_nodes >= 100 and cp.pods[4]["names_len"] >= 0
    assert plan["chain"] == 0 and plan["pod"] == 4 and "percentageOfNodesToScore" in plan["reason"], plan
    prof.pct_nodes_to_score = 100  # the same list without the window: the chain takes it
    assert native.plan_service(cc.as_struct(), cp.as_struct(), prof)["chain"] == 1


def test_list_without_ports_or_images_is_planned_as_before():
    nodes, bound, pods = progfuzz.make(2, 60, 200, extended=False, programs=False)
    pods = _weights(pods, 3, 8192)  # no limit of the form applies to it
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    assert not any(cp.pods[i]["port_conflict"] or cp.pods[i]["port_add"] or cp.pods[i]["img_len"] > 0
                   for i in range(cp.n))
    off = native.plan_service(cc.as_struct(), cp.as_struct())
    native.set_option("service_ports_images", 1)
    on = native.plan_service(cc.as_struct(), cp.as_struct())
    assert off == {"chain": 1, "pod": -1, "reason": "eligible"} and on == off
