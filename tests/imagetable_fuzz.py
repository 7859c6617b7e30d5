"""Image-only batches for the shape-table loop's ports-and-images form (test infrastructure):
progfuzz clusters without programs whose pending pods draw their requests from a short list of
resource shapes (tests/test_gpu_flat_exchange.py's recipe), every node listing up to three of
portimage_fuzz's images and every container naming one, no host port on any pending pod.
tests/test_imagetable_plan.py (host only) and tests/test_gpu_image_table.py use them."""
import random

import numpy as np

import oracle_c
import portimage_fuzz
import progfuzz
from kss import abi
from kss.compile import compile_cluster

MI = 1024 * 1024
# the list of tests/test_gpu_flat_exchange.py
BASE_SHAPES = [{"cpu": "100m", "memory": "128Mi"}, {"cpu": "250m", "memory": "512Mi"},
               {"cpu": "500m", "memory": "256Mi", "ephemeral-storage": "256Mi"}, {}]


def manifests(seed, n_nodes, n_pods, shapes=BASE_SHAPES, bound_per_node=(0, 3)):
    nodes, bound, pods = progfuzz.make(seed, n_nodes, n_pods, bound_per_node=bound_per_node,
                                       extended=False, programs=False)
    r = random.Random(seed * 7919 + 1)  # as tests/test_gpu_flat_exchange.py _manifests
    for p in pods:
        p["spec"].pop("initContainers", None)
        req = p["spec"]["containers"][0]["resources"]["requests"]
        req.clear()
        req.update(shapes[r.randrange(len(shapes))])
    q = random.Random(seed * 104729 + 5)
    for n in nodes:
        imgs = [{"names": [nm], "sizeBytes": q.choice([30, 400, 800, 1500, 3000]) * MI}
                for nm in q.sample(portimage_fuzz.IMAGES, q.choice([0, 1, 2, 3]))]
        if imgs:
            n.setdefault("status", {})["images"] = imgs
    for p in pods:
        for c in p["spec"]["containers"]:
            c["image"] = q.choice(portimage_fuzz.IMAGES)
            c.pop("ports", None)
    return nodes, bound, pods


def oracle(cc, cp, prof=None, record=True):
    return oracle_c.schedule(prof or abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes,
                             record=record, n_classes=len(cc.classes), n_terms=len(cc.terms))


def host_port_pods(cp):
    return sum(int(bool(cp.pods[i]["port_conflict"] or cp.pods[i]["port_add"])) for i in range(cp.n))


def il_decides(cc, cp, res, prof=None):
    """Pods whose choice is not the argmax of total - ImageLocality, from the oracle's records: a
    loop that ignored ImageLocality would choose another node for each of them."""
    prof = prof or abi.default_profile()
    N = cc.n_nodes
    w_il = prof.weight[abi.KSS_S_IMAGE_LOCALITY] if (prof.score_enabled >> abi.KSS_S_IMAGE_LOCALITY) & 1 else 0
    n = 0
    for j in range(cp.n):
        m = res.meta(j)
        if m["scored"]:
            fp = res.fail_plugin[j, :N]
            kept = (fp == 0) & (res.fail_detail[j, :N] != abi.KSS_PASS_NOT_KEPT)
            rest = np.where(kept, res.total[j, :N] - w_il * res.norm[j][abi.KSS_S_IMAGE_LOCALITY, :N], -1)
            n += int(np.argmax(rest) != m["chosen"])
    return n


_CACHE = {}


def case(seed, n_nodes, n_pods, bound_per_node=(0, 3), edit=None, pct=100):
    """(cc, cp, oracle chosen, records, final state) of one batch under the default profile (pct:
    its percentageOfNodesToScore), computed once and shared: nothing writes to them.  edit
    (optional, hashable): (name, f) with f(nodes, bound, pods) editing the manifests and returning
    g(cp) or None, which edits the compiled pods."""
    key = (seed, n_nodes, n_pods, bound_per_node, edit[0] if edit else None, pct)
    if key not in _CACHE:
        nodes, bound, pods = manifests(seed, n_nodes, n_pods, bound_per_node=bound_per_node)
        after = edit[1](nodes, bound, pods) if edit else None
        cc, cp, _ = compile_cluster(nodes, bound, pods)
        if after:
            after(cp)
        prof = abi.default_profile()
        prof.pct_nodes_to_score = pct
        _CACHE[key] = (cc, cp) + tuple(oracle(cc, cp, prof))
    return _CACHE[key]
