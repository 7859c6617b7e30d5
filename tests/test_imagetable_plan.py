"""Host-only planning of image-only batches for the shape-table loop (no GPU needed): with the option
simple_ports_images on, kss_plan_shapes answers for a batch of the ports-and-images form -- its
resource shapes do not depend on the images its containers name -- and with the option off it
refuses the batch as before.  The option table_images exists, defaults to 0 and is reset with the
others.  kss_plan_podset answers what it answered."""
import copy

import pytest

import imagetable_fuzz
from kss import native
from kss.compile import compile_cluster

CASE = (46, 130, 200)


@pytest.fixture(autouse=True)
def _options():
    native.reset_options()
    yield
    native.reset_options()


@pytest.fixture(scope="module")
def batch():
    nodes, bound, pods = imagetable_fuzz.manifests(*CASE)
    plain = copy.deepcopy(pods)
    for p in plain:
        for c in p["spec"]["containers"]:
            c["image"] = "nobody-lists-this:1"
    cc, cp, _ = compile_cluster(nodes, bound, pods)
    cc0, cp0, _ = compile_cluster(nodes, bound, plain)
    assert imagetable_fuzz.host_port_pods(cp) == 0 and not cc.scalars
    assert any(cp.pods[i]["img_len"] > 0 for i in range(cp.n))
    assert not any(cp0.pods[i]["img_len"] > 0 for i in range(cp0.n))
    return cc, cp, cc0, cp0


def test_plan_shapes_with_the_form(batch):
    cc, cp, cc0, cp0 = batch
    native.set_option("simple_ports_images", 1)
    ids, n = native.plan_shapes(cp.as_struct(), len(cc.scalars))
    assert n == 4 and sorted(set(ids)) == [0, 1, 2, 3]
    ids0, n0 = native.plan_shapes(cp0.as_struct(), len(cc0.scalars))
    assert n0 == 4 and list(ids) == list(ids0)
    # whatever table_images says: the shapes are the batch's
    native.set_option("table_images", 1)
    ids1, n1 = native.plan_shapes(cp.as_struct(), len(cc.scalars))
    assert n1 == 4 and list(ids1) == list(ids)


def test_plan_shapes_option_off_refuses_as_before(batch):
    cc, cp, cc0, cp0 = batch
    with pytest.raises(native.KssError) as e:
        native.plan_shapes(cp.as_struct(), len(cc.scalars))
    assert e.value.rc == -95 and "no compact records" in str(e.value), e.value
    native.set_option("table_images", 1)  # no effect without simple_ports_images
    with pytest.raises(native.KssError):
        native.plan_shapes(cp.as_struct(), len(cc.scalars))
    ids0, n0 = native.plan_shapes(cp0.as_struct(), len(cc0.scalars))
    assert n0 == 4 and len(ids0) == cp0.n


def test_table_images_option():
    assert native.get_option("table_images") == 0
    native.set_option("table_images", 1)
    assert native.get_option("table_images") == 1
    native.reset_options()
    assert native.get_option("table_images") == 0


def test_plan_podset_unchanged(batch):
    cc, cp, cc0, cp0 = batch
    eligible = {"kernel": "k_simple", "pod": -1, "reason": "eligible"}
    for ti in (0, 1):
        native.reset_options()
        native.set_option("table_images", ti)
        off = native.plan_podset(cc.as_struct(), cp.as_struct())
        assert off["kernel"] == "k_schedule" and "host ports" in off["reason"], off
        assert native.plan_podset(cc0.as_struct(), cp0.as_struct()) == eligible
        native.set_option("simple_ports_images", 1)
        assert native.plan_podset(cc.as_struct(), cp.as_struct()) == eligible
        assert native.plan_podset(cc0.as_struct(), cp0.as_struct()) == eligible
