"""Host-only routing of batches WITH programs whose pods hold host ports or node-cached images
(kss_plan_podset, no GPU needed): with the option spread_ports_images on, such a batch is planned on
k_spread (its ports-and-images form); the option simple_ports_images alone, a volume program,
preferred NodeAffinity weights above the form's 13 bits or the statistics fold keep it on
k_schedule; with the option off, and for a batch without such pods, the plan is what it was."""
import copy

import pytest

import spread_portimage_fuzz as spf
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
    na = pods[j]["spec"].setdefault("affinity", {}).setdefault("nodeAffinity", {})
    na["preferredDuringSchedulingIgnoredDuringExecution"] = [
        {"weight": total - 100, "preference": pref}, {"weight": 100, "preference": pref}]
    return pods


def test_option_exists_and_defaults_off():
    assert native.get_option("spread_ports_images") == 0
    native.set_option("spread_ports_images", 1)
    assert native.get_option("spread_ports_images") == 1
    native.reset_options()
    assert native.get_option("spread_ports_images") == 0


def test_option_off_keeps_k_schedule():
    plan, _ = _plan(*spf.make(1, 60, 200))
    assert plan["kernel"] == "k_schedule" and "host ports" in plan["reason"], plan


def test_option_on_takes_k_spread():
    native.set_option("spread_ports_images", 1)
    plan, cp = _plan(*spf.make(1, 60, 200))
    assert any(cp.pods[i]["port_conflict"] or cp.pods[i]["port_add"] for i in range(cp.n))
    assert all(cp.pods[i]["img_len"] > 0 for i in range(cp.n))
    assert any(cp.pods[i]["n_hard"] or cp.pods[i]["n_soft"] or cp.pods[i]["ipa_len"] for i in range(cp.n))
    assert plan == {"kernel": "k_spread", "pod": -1, "reason": "eligible"}, plan


def test_simple_option_alone_keeps_k_schedule():
    native.set_option("simple_ports_images", 1)
    plan, _ = _plan(*spf.make(1, 60, 200))
    assert plan["kernel"] == "k_schedule" and "host ports" in plan["reason"], plan
    native.set_option("spread_ports_images", 1)  # the two options do not depend on each other
    plan, _ = _plan(*spf.make(1, 60, 200))
    assert plan["kernel"] == "k_spread", plan


def test_volume_program_stays_on_k_schedule():
    native.set_option("spread_ports_images", 1)
    nodes, bound, pods = spf.make(1, 60, 200)
    pods[7]["spec"]["volumes"] = [{"name": "v0", "gcePersistentDisk": {"pdName": "disk-1"}}]
    plan, cp = _plan(nodes, bound, pods)
    assert cp.pods[7]["vol_len"] > 0
    assert plan["kernel"] == "k_schedule" and plan["pod"] == 7 and "volumes" in plan["reason"], plan


def test_node_affinity_weight_limit():
    """The form keeps 13 bits of raw NodeAffinity: Σ preferred weights 8191 fits, 8192 does not, and
    the refusal has a reason of its own that names the limit, the kernel and the pod."""
    native.set_option("spread_ports_images", 1)
    nodes, bound, pods = spf.make(1, 60, 200)
    plan, _ = _plan(nodes, bound, _weights(pods, 3, 8192))
    assert plan["kernel"] == "k_schedule" and plan["pod"] == 3, plan
    assert "8191" in plan["reason"] and "k_spread" in plan["reason"], plan
    plan, _ = _plan(nodes, bound, _weights(pods, 3, 8191))
    assert plan == {"kernel": "k_spread", "pod": -1, "reason": "eligible"}, plan
    # the limit belongs to the form: without it the batch is refused for its ports and images
    native.set_option("spread_ports_images", 0)
    plan, _ = _plan(nodes, bound, _weights(pods, 3, 8192))
    assert plan["kernel"] == "k_schedule" and "host ports" in plan["reason"], plan


def test_ungrafted_batch_is_planned_as_before():
    nodes, bound, pods = spf.make(1, 60, 200, grafted=False)
    pods = _weights(pods, 3, 8192)  # no limit of the form applies to it: the 20-bit field holds these
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    assert not any(cp.pods[i]["port_conflict"] or cp.pods[i]["port_add"] or cp.pods[i]["img_len"] > 0
                   for i in range(cp.n))
    off = native.plan_podset(cc.as_struct(), cp.as_struct())
    native.set_option("spread_ports_images", 1)
    on = native.plan_podset(cc.as_struct(), cp.as_struct())
    assert off["kernel"] == "k_spread" and on == off, (on, off)


def test_fold_keeps_the_grafted_batch_off_k_spread():
    """No statistics fold in the form: with fold = 1 the batch is refused as with the option off."""
    native.set_option("spread_ports_images", 1)
    native.set_option("fold", 1)
    plan, _ = _plan(*spf.make(1, 60, 200))
    assert plan["kernel"] == "k_schedule" and "host ports" in plan["reason"], plan
    plan, _ = _plan(*spf.make(1, 60, 200, grafted=False))  # (the fold itself still takes k_spread)
    assert plan["kernel"] == "k_spread", plan
