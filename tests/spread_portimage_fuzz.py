"""Program fuzz with NodePorts and ImageLocality grafted on (test infrastructure).

progfuzz.make's clusters (every PodTopologySpread / InterPodAffinity kind, no extended resources)
with node images, container images and host ports drawn by a second generator, so progfuzz's own
draw is undisturbed and the sizes of tests/test_gpu_spread.py stay k_spread batches apart from
the graft.  tests/test_spread_portimage_plan.py plans them and
tests/test_gpu_spread_portimage.py runs them on k_spread's ports-and-images form.
"""
import random

import portimage_fuzz
import progfuzz

MI = 1024 * 1024


def graft(seed, nodes, bound, pods):
    """Images on the nodes, an image on every container, host ports on three containers in ten."""
    r = random.Random(seed * 7919 + 1)
    for nd in nodes:
        imgs = [{"names": [nm], "sizeBytes": r.choice([30, 400, 800, 1500, 3000]) * MI}
                for nm in r.sample(portimage_fuzz.IMAGES, r.choice([0, 1, 2, 3]))]
        if imgs:
            nd["status"]["images"] = imgs
    for p in bound + pods:
        for c in p["spec"]["containers"]:
            c["image"] = r.choice(portimage_fuzz.IMAGES)
            if r.random() < 0.3:
                c["ports"] = [portimage_fuzz._port(r) for _ in range(r.choice([1, 1, 2]))]


def strip_name_lists(pods):
    """Every matchFields leaves the pending pods' required node-affinity terms (no PreFilterResult
    node list: the window refuses those); a term list that becomes empty is replaced by one term,
    hostname Exists."""
    for p in pods:
        req = p["spec"].get("affinity", {}).get("nodeAffinity", {}).get("requiredDuringSchedulingIgnoredDuringExecution")
        if not req:
            continue
        terms = []
        for t in req.get("nodeSelectorTerms", []):
            t.pop("matchFields", None)
            if t.get("matchExpressions"):
                terms.append(t)
        if not terms:
            terms = [{"matchExpressions": [{"key": progfuzz.K_HOST, "operator": "Exists"}]}]
        req["nodeSelectorTerms"] = terms


def make(seed, n_nodes, n_pods, names_lists=True, grafted=True):
    """(nodes, bound pods, pending pods); grafted=False: progfuzz's batch alone."""
    nodes, bound, pods = progfuzz.make(seed, n_nodes, n_pods, extended=False)
    if grafted:
        graft(seed, nodes, bound, pods)
    if not names_lists:
        strip_name_lists(pods)
    return nodes, bound, pods
