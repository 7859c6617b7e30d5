"""Shared by the tests of k_simple's volumes form (test infrastructure): the restatement of the form
on the CPU -- a node's used-rows mask and per-key attached counts replayed over the oracle's choices
-- that counts what a batch reaches, and the hand-built private-volume cluster."""
import numpy as np

import volume_fixtures as vf
from edge_fixtures import HOST, node
from kss import abi

DYNAMIC = (abi.KSS_F_VOLUME_RESTRICTIONS, abi.KSS_F_EBS_LIMITS, abi.KSS_F_GCEPD_LIMITS, abi.KSS_F_NODE_VOLUME_LIMITS,
           abi.KSS_F_AZURE_DISK_LIMITS)
LIMITS = DYNAMIC[1:]
STATIC = (abi.KSS_F_VOLUME_BINDING, abi.KSS_F_VOLUME_ZONE)


def pod_masks(cc, cp, j):
    """Pod j's volume program as the form holds it: (conflict, shared, own, keys, private new counts,
    private commit counts) over the cluster's rows and keys."""
    K = cc.as_struct().n_vol_keys
    rowkey = cc.arrays["vol_row_key"]
    p = cp.pods[j]
    conflict = shared = own = keys = 0
    pnew, padd = [0] * K, [0] * K
    for e in range(int(p["vol_len"])):
        v = cp.vols[int(p["vol_off"]) + e]
        kind, key, row, cnt = int(v["kind"]), int(v["key"]), int(v["row"]), int(v["count"])
        if kind == abi.KSS_VOL_CONFLICT:
            conflict |= 1 << row
        elif kind == abi.KSS_VOL_LIMIT:
            keys |= 1 << key
            if row >= 0:
                assert int(rowkey[row]) == key
                shared |= 1 << row
            else:
                pnew[key] += cnt
        elif kind == abi.KSS_VOL_OWN:
            own |= 1 << row
        elif kind == abi.KSS_VOL_OWN_PRIVATE:
            padd[key] += cnt
    return conflict, shared, own, keys, pnew, padd


def reach(cc, cp, ch_o, res, prof=None):
    """From the oracle's records and a replay of its choices on the masks: pods with a node failing
    VolumeRestrictions, pods with a node failing a limit plugin, pods with a node failing VolumeBinding /
    VolumeZone, and H1 pairs -- pod k+1 fails a dynamic volume filter on the node pod k took, and would
    not on that node's state before pod k's commit.  Asserts on the way that the replayed state decides
    every recorded dynamic verdict (default profile only) and ends in the oracle's final columns.
    Also returned, with the limit key that decides them (the first failing key in filter order):
    h1_events [(pod k+1, node, key)] and limit_failures [(pod, node, key)]."""
    cs = cc.as_struct()
    N, R, K = cc.n_nodes, cs.n_vol_rows, cs.n_vol_keys
    A = cc.arrays
    plug = [int(x) for x in A["vol_key_plugin"][:K]]
    rowkey = [int(x) for x in A["vol_row_key"][:R]]
    keyrows = [sum(1 << r for r in range(R) if rowkey[r] == k) for k in range(K)]
    used = [sum(1 << r for r in range(R) if A["vol_count"][r][n] > 0) for n in range(N)]
    att = [[int(A["vol_attached"][k][n]) for k in range(K)] for n in range(N)]
    lim = [[int(A["vol_limit"][k][n]) for k in range(K)] for n in range(N)]
    cnt = np.array(A["vol_count"][:R, :N]).copy()
    enabled = (prof or abi.default_profile()).filter_enabled
    exact = prof is None
    vr = lm = stc = h1 = 0
    h1_events, limit_failures = [], []
    prev = None
    for j in range(cp.n):
        conflict, shared, own, keys, pnew, padd = pod_masks(cc, cp, j)

        def dyn_key(u, a, n):
            """The deciding limit key on node n's state (u, a), -1 for VolumeRestrictions, None: passes."""
            if (enabled >> abi.KSS_F_VOLUME_RESTRICTIONS) & 1 and u & conflict:
                return -1
            for k in range(K):
                if not (keys >> k) & 1 or lim[n][k] < 0 or not (enabled >> plug[k]) & 1:
                    continue
                new = bin(shared & keyrows[k] & ~u).count("1") + pnew[k]
                if plug[k] == abi.KSS_F_NODE_VOLUME_LIMITS and new == 0:
                    continue
                if a[k] + new > lim[n][k]:
                    return k
            return None

        def dyn_fail(u, a, n):
            return dyn_key(u, a, n) is not None

        if int(cp.pods[j]["prefilter_status"]) == 0:
            fp = res.fail_plugin[j][:N]
            vr += int((fp == abi.KSS_F_VOLUME_RESTRICTIONS).any())
            lm += int(np.isin(fp, LIMITS).any())
            stc += int(np.isin(fp, STATIC).any())
            if exact:
                for n in range(N):
                    f = int(fp[n])
                    if f == abi.KSS_F_NOT_EVALUATED or 0 < f < abi.KSS_F_VOLUME_RESTRICTIONS:
                        continue  # an earlier filter decided the node
                    assert dyn_fail(used[n], att[n], n) == (f in DYNAMIC), (j, n, f)
                    if f in LIMITS:
                        k = dyn_key(used[n], att[n], n)
                        assert k >= 0 and plug[k] == f, (j, n, f, k)
                        limit_failures.append((j, n, k))
            if prev is not None:
                x, u0, a0 = prev
                if int(fp[x]) in DYNAMIC and not dyn_fail(u0, a0, x):
                    h1 += 1
                    h1_events.append((j, x, dyn_key(used[x], att[x], x)))
        prev = None
        x = int(ch_o[j])
        if x >= 0:
            prev = (x, used[x], list(att[x]))
            fresh = own & ~used[x]
            for k in range(K):
                att[x][k] += bin(fresh & keyrows[k]).count("1") + padd[k]
            used[x] |= own
            for r in range(R):
                cnt[r][x] += (own >> r) & 1
    return dict(restrictions=vr, limits=lm, static=stc, h1=h1, used=used, att=att, cnt=cnt, h1_events=h1_events,
                limit_failures=limit_failures)


def private_ebs(n_nodes=6, n_pods=16, limit=2):
    """n_nodes nodes that attach `limit` EBS volumes each, and n_pods identical pods, each with an EBS
    volume no other pod names (KSS_VOL_LIMIT with row < 0, KSS_VOL_OWN_PRIVATE).  In front of them one
    pod pinned to n0 whose only volume is a CSI claim a bound pod already holds on n0, where the
    driver's limit (0) is exceeded: NodeVolumeLimits does not check a key without a new volume."""
    drv = "ebs.csi.aws.com"
    nodes = [node("n%d" % i, extra={"attachable-volumes-aws-ebs": str(limit)}) for i in range(n_nodes)]
    csinodes = [{"metadata": {"name": "n0"}, "spec": {"drivers": [{"name": drv, "allocatable": {"count": 0}}]}}]
    st = vf.storage(pvs=[vf.pv("pv-s", vf.csi(drv, "h-s"))], pvcs=[vf.pvc("c-s", "pv-s")], csinodes=csinodes)
    bound = [vf.vpod("holder", vf.claim("c-s"), node_name="n0")]
    shared = vf.vpod("shared", vf.claim("c-s"))
    shared["spec"]["nodeSelector"] = {HOST: "n0"}
    pods = [shared] + [vf.vpod("p%02d" % j, vf.ebs("vol-only-%d" % j)) for j in range(n_pods)]
    return nodes, bound, pods, st
