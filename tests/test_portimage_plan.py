"""Host-only routing of NodePorts / ImageLocality batches (kss_plan_podset, no GPU needed): with the
option simple_ports_images on, a batch that holds a pod with host ports or node-cached images is
planned on k_simple (its ports-and-images form); a volume program or preferred NodeAffinity weights
above the form's 13 bits keep it on k_schedule; with the option off, and for a batch without such
pods, the plan is what it was."""
import copy

import pytest

import portimage_fuzz
import progfuzz
from kss import native
from kss.compile import compile_cluster


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


def _plan(nodes, bound, pods):
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    return native.plan_podset(cc.as_struct(), cp.as_struct()), cp


def _weights(pods, j, total):
    """Pod j prefers every node twice over: two terms whose weights sum to `total`."""
    pods = copy.deepcopy(pods)
    pref = {"matchExpressions": [{"key": "kubernetes.io/hostname", "operator": "Exists"}]}
    pods[j]["spec"]["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
        {"weight": total - 100, "preference": pref}, {"weight": 100, "preference": pref}]}}
    return pods


def test_option_off_keeps_k_schedule():
    plan, _ = _plan(*portimage_fuzz.make(5))
    assert plan["kernel"] == "k_schedule" and "host ports" in plan["reason"], plan


def test_option_on_takes_k_simple():
    native.set_option("simple_ports_images", 1)
    plan, cp = _plan(*portimage_fuzz.make(5))
    assert any(cp.pods[i]["port_conflict"] or cp.pods[i]["port_add"] for i in range(cp.n))
    assert any(cp.pods[i]["img_len"] > 0 for i in range(cp.n))
    assert plan == {"kernel": "k_simple", "pod": -1, "reason": "eligible"}, plan


def test_volume_program_stays_on_k_schedule():
    native.set_option("simple_ports_images", 1)
    nodes, bound, pods = portimage_fuzz.make(5)
    pods[7]["spec"]["volumes"] = [{"name": "v0", "gcePersistentDisk": {"pdName": "disk-1"}}]
    plan, cp = _plan(nodes, bound, pods)
    assert cp.pods[7]["vol_len"] > 0
    assert plan["kernel"] == "k_schedule" and "volumes" in plan["reason"], plan


def test_node_affinity_weight_limit():
    """The form keeps 13 bits of raw NodeAffinity: Σ preferred weights 8191 fits, 8192 does not."""
    native.set_option("simple_ports_images", 1)
    nodes, bound, pods = portimage_fuzz.make(5)
    plan, _ = _plan(nodes, bound, _weights(pods, 3, 8192))
    assert plan["kernel"] == "k_schedule" and plan["pod"] == 3 and "8191" in plan["reason"], plan
    plan, _ = _plan(nodes, bound, _weights(pods, 3, 8191))
    assert plan["kernel"] == "k_simple", plan
    # the limit belongs to the form: without it the 20-bit field holds these weights
    native.set_option("simple_ports_images", 0)
    plan, _ = _plan(nodes, bound, _weights(pods, 3, 8192))
    assert plan["kernel"] == "k_schedule" and "host ports" in plan["reason"], plan


def test_batch_without_ports_or_images_is_planned_as_before():
    nodes, bound, pods = progfuzz.make(2, 60, 200, programs=False)
    pods = _weights(pods, 3, 8192)  # no limit of the form applies to it
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    assert not any(cp.pods[i]["port_conflict"] or cp.pods[i]["port_add"] or cp.pods[i]["img_len"] > 0
                   for i in range(cp.n))
    off = native.plan_podset(cc.as_struct(), cp.as_struct())
    ids_off, n_off = native.plan_shapes(cp.as_struct(), len(cc.scalars))
    native.set_option("simple_ports_images", 1)
    on = native.plan_podset(cc.as_struct(), cp.as_struct())
    ids_on, n_on = native.plan_shapes(cp.as_struct(), len(cc.scalars))
    assert off["kernel"] == "k_simple" and on == off
    assert n_on == n_off and list(ids_on) == list(ids_off)
