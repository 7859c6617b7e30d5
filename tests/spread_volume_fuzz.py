"""Program fuzz with NodePorts, ImageLocality and volumes grafted on (test infrastructure).

spread_portimage_fuzz.make's batches (progfuzz's programs with images and host ports) with attach
limits, CSINode counts, zone-labelled / node-affine PVs, shared claims, inline EBS / GCE PD disks and
private claims drawn by a further seeded generator, so the earlier draws are undisturbed.
tests/test_spread_volume_plan.py plans them and tests/test_gpu_spread_volumes.py runs them on
k_spread's volumes form.  Compile with compile_cluster(nodes, bound, pods, storage=st).

The pools (n_claims shared claims, n_ebs / n_gce inline disks) are parameters: at their defaults the
clusters have 33-45 volume rows and 4 limit keys; wider pools reach the form's 64-row edge.
"""
import random

import spread_portimage_fuzz as spf
import volume_fixtures as vf

ZONES = ["z0", "z1", "z2", "z3"]
DRIVERS = ["ebs.csi.aws.com", "pd.csi.storage.gke.io"]
N_CLAIMS, N_EBS, N_GCE = 12, 6, 5


def graft_volumes(seed, nodes, bound, pods, share=0.4, lim=(1, 3), n_claims=N_CLAIMS, n_ebs=N_EBS, n_gce=N_GCE):
    r = random.Random(seed * 104729 + 3)
    csinodes = []
    for nd in nodes:
        al = nd["status"]["allocatable"]
        if r.random() < 0.5:
            al["attachable-volumes-aws-ebs"] = str(r.randint(*lim))
        if r.random() < 0.5:
            al["attachable-volumes-gce-pd"] = str(r.randint(*lim))
        if r.random() < 0.6:
            csinodes.append({"metadata": {"name": nd["metadata"]["name"]}, "spec": {"drivers": [
                {"name": d, "allocatable": {"count": r.randint(*lim)}} for d in DRIVERS]}})
    pvs, pvcs = [], []
    for k in range(n_claims):
        labels = {vf.ZONE: r.choice(ZONES)} if r.random() < 0.3 else {}
        aff = None
        if r.random() < 0.3:
            aff = [{"matchExpressions": [{"key": vf.ZONE, "operator": "In", "values": r.sample(ZONES, 2)}]}]
        pvs.append(vf.pv("pv-s%d" % k, vf.csi(r.choice(DRIVERS), "h-s%d" % k), labels=labels, affinity_terms=aff))
        pvcs.append(vf.pvc("c-s%d" % k, "pv-s%d" % k))

    def volumes(tag, private):
        out = []
        for _ in range(r.choice([1, 1, 2])):
            x = r.random()
            if x < 0.2:
                out.append(vf.ebs("vol-%d" % r.randrange(n_ebs), ro=r.random() < 0.3))
            elif x < 0.35:
                out.append(vf.gce("pd-%d" % r.randrange(n_gce), ro=r.random() < 0.5))
            elif x < 0.7 or not private:
                out.append(vf.claim("c-s%d" % r.randrange(n_claims)))
            else:
                nm = "%s-%d" % (tag, len(out))
                pvs.append(vf.pv("pv-p-" + nm, vf.csi(r.choice(DRIVERS), "h-p-" + nm)))
                pvcs.append(vf.pvc("c-p-" + nm, "pv-p-" + nm))
                out.append(vf.claim("c-p-" + nm))
        return [dict(v, name="v%d" % i) for i, v in enumerate(out)]

    for i, p in enumerate(bound):
        if r.random() < share:
            p["spec"]["volumes"] = volumes("b%d" % i, False)
    for i, p in enumerate(pods):
        if r.random() < share:
            p["spec"]["volumes"] = volumes("p%d" % i, True)
    return vf.storage(pvs, pvcs, [], csinodes)


def make(seed, n_nodes, n_pods, names_lists=True, **pools):
    """(nodes, bound pods, pending pods, storage); pools: graft_volumes' keyword parameters."""
    nodes, bound, pods = spf.make(seed, n_nodes, n_pods, names_lists=names_lists)
    return nodes, bound, pods, graft_volumes(seed, nodes, bound, pods, **pools)
