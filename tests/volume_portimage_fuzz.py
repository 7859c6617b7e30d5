"""volume_fuzz's clusters with NodePorts and ImageLocality on top (test infrastructure): the same
nodes, storage objects and pods, to which a seeded generator of its own adds Status.Images on the
nodes and, on a share of the bound and pending pods, container images that some nodes list and
host ports (few distinct ones, so pods collide).  One batch then reaches the volume filters, a
NodePorts failure and choices that ImageLocality decides."""
import random

import volume_fuzz

MI = 1024 * 1024
IMAGES = ["app:v1", "app:v2", "base:latest", "registry:5000/tool:latest", "big:1"]
PORTS = [80, 8080, 9090]


def _decorate(r, pod, p_image, p_port):
    c = pod["spec"]["containers"][0]
    if r.random() < p_image:
        c["image"] = r.choice(IMAGES)
    if r.random() < p_port:
        c["ports"] = [{"containerPort": 80, "hostPort": r.choice(PORTS), "protocol": r.choice(["TCP", "UDP"]),
                       "hostIP": r.choice(["", "10.0.0.1"])}]


def make(seed, n_nodes=12, n_bound=16, n_pods=40, p_image=0.7, p_port=0.3):
    nodes, bound, pods, st = volume_fuzz.make(seed, n_nodes=n_nodes, n_bound=n_bound, n_pods=n_pods)
    r = random.Random(1000003 * seed + 17)
    for nd in nodes:
        imgs = [{"names": [nm], "sizeBytes": r.choice([30, 400, 800, 1500, 3000]) * MI}
                for nm in r.sample(IMAGES, r.choice([0, 1, 2, 3]))]
        if imgs:
            nd["status"]["images"] = imgs
    for p in bound:
        _decorate(r, p, p_image, p_port)
    for p in pods:
        _decorate(r, p, p_image, p_port)
    return nodes, bound, pods, st
