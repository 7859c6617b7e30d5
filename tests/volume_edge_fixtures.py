"""Clusters that put the volumes forms' packed node state on its edges (test infrastructure): limit
keys 4-7, which live in the second 64-bit word, and 16-bit fields near 255 / 256, 32767 / 32768 and
the top (65534; 65535 = 0xFFFF is "the node does not limit this key").

The layout (k_vol_pack, vol_pack_host, vol_infeasible / vol_assume / vol_commit, k_vol_unpack): per
node one used-rows word and four words of 16-bit fields -- attached counts a0 / a1, limits l0 / l1 --
key k at bit 16 * (k & 3) of word k >> 2.  `pack` restates it in Python integers.

Key order.  kss/volumes.py numbers the keys in filter order: EBS, GCE PD, the CSI drivers by key name,
Azure Disk.  EBS and GCE PD are therefore always keys 0 and 1 when present, CSI drivers fill the
middle, and Azure Disk is the only in-tree plugin that can reach the upper word (as key 4-7, with at
least one and at most five CSI drivers and both other in-tree plugins in front of it).  eight_keys has
EBS, GCE PD, five CSI drivers and Azure Disk: exactly 8 keys, CSI at 2-6, Azure at 7.

eight_keys(pin=True), 24 nodes n00 .. n23, every pending pod pinned by a hostname nodeSelector (the
other 23 nodes fail NodeAffinity), nothing requests resources.  Per key k two nodes:

  G[k]  limit 3, a bound holder with the shared volume k-a (attached 1)
  H[k]  limit 1, a bound holder with the shared volume k-c and a volume of its own (attached 2 > 1)

and four pending pods, in this order:

  P1  on G[k]: k-a and k-b (shared with nobody yet): one new, 1 + 1 <= 3, passes; attached 2
  P2  on G[k]: a private volume: 2 + 1 == 3 == limit, passes (decided by one unit); attached 3
  P3  on G[k]: a private volume: 3 + 1 == limit + 1, fails its key's plugin.  On the state before
      P2's commit it would pass (2 + 1): the H1 pair (P2, P3) -- P2 takes the last slot, the next pod
      with the same pin must see it.  Unschedulable.
  Pc  on H[k]: names only k-c, attached there, where the count (2) exceeds the limit (1):
        CSI keys 2-6: CSILimits.Filter (v1.26 csi.go) collects newVolumes, deletes those in
        attachedVolumes, and checks a driver's limit only inside
        `for volumeLimitKey, count := range newVolumeCount` -- a key with no new volume is never
        looked at.  Pc passes and is bound to H[k]; nothing is added (k-c is attached).
        In-tree keys 0, 1, 7: nonCSILimits.Filter (non_csi.go) returns early only when the pod has no
        volume of the plugin at all (`if len(newVolumes) == 0 { return nil }`, before the attached
        ones are taken out); then `numExistingVolumes+numNewVolumes > maxAttachLimit` is checked with
        numNewVolumes == 0: 2 + 0 > 1, Pc fails its plugin.  Unschedulable.

Then three more pods:

  D5  on G[5]: a private EBS volume (key 0, lower word: 0 + 1 <= 39 passes) and a private volume of
      CSI key 5 (upper word: 3 + 1 > 3): fails NodeVolumeLimits, not EBSLimits
  D7  on G[7]: a private EBS volume and a private Azure disk (key 7: 3 + 1 > 3): fails AzureDiskLimits
  U   on G[5]: a private volume of CSI key 4, which G[5] does not limit (no CSINode entry: -1): passes,
      attached[4][G[5]] 0 -> 1 -- the same shape as P3 of key 5, which fails on the same node

So every key decides two limit failures or more and one H1 pair; final vol_attached is 3 on G[k], 2 on
H[k], 1 for key 4 on G[5] and 0 elsewhere.  G and H are spread so that with 2 shards (12 nodes each) and
3 shards (8 each) the nodes of keys 4-7 fall into different shards and none is a shard's first node.

A_k, the host's per-key bound on what the batch can add (vol_form_admit's vol_add: own rows and
private counts of every pod, scheduled or not): 5 per group, + 2 for key 0 (D5, D7), + 1 for keys 4
(U), 5 (D5) and 7 (D7).

field_tops(variant, ...) writes counters into the compiled arrays of eight_keys (65,530 volume objects
per field are not a fixture; the C oracle reads the same arrays, the object-level oracle is left
out).  Verdicts depend on attached + new against the limit only, so shifting both by one constant on
a node leaves every verdict and choice as hand-derived; the variants say what vol_attached ends on.
"""
import numpy as np

import volume_fixtures as vf
import volume_form_fixtures as vff
from edge_fixtures import HOST, ZONE, node
from kss import abi
from kss.compile import compile_cluster

FIELD_MAX, UNCHECKED = 65534, 0xFFFF
N_NODES = 24
DRIVERS = ["d%d.csi.example" % i for i in range(5)]  # keys 2 .. 6 (sorted by key name)
PLUGIN = [abi.KSS_F_EBS_LIMITS, abi.KSS_F_GCEPD_LIMITS] + [abi.KSS_F_NODE_VOLUME_LIMITS] * 5 + [abi.KSS_F_AZURE_DISK_LIMITS]
IN_TREE_KEY = {0: "attachable-volumes-aws-ebs", 1: "attachable-volumes-gce-pd", 7: "attachable-volumes-azure-disk"}
G = [1, 13, 5, 17, 10, 22, 3, 19]  # the deciding node of key k
H = [2, 14, 6, 18, 9, 21, 4, 20]   # the over-limit node of key k
LIMIT_G, LIMIT_H = 3, 1
A = [7, 5, 5, 5, 6, 6, 5, 6]       # the per-key add bound, hand-counted above
N_FILL = 126                        # wide: filler nodes x000 .. x125, 150 nodes in all


def _name(i):
    return "n%02d" % i


def _source(k, vid):
    if k == 0:
        return vf.ebs(vid)
    if k == 1:
        return vf.gce(vid)
    if k == 7:
        return vf.azure(vid)
    return vf.csi(DRIVERS[k - 2], vid)


def _limits(k, count):
    """(allocatable entry, CSINode driver entry) that limit key k to count."""
    if k in IN_TREE_KEY:
        return {IN_TREE_KEY[k]: str(count)}, None
    return {}, {"name": DRIVERS[k - 2], "allocatable": {"count": count}}


def eight_keys(pin=True, soft=False, wide=False, drop=()):
    """dict(nodes, bound, pods, storage, expect, final).  expect: per pending pod (name, pinned node
    index, chosen node index or -1, fail_plugin on the pinned node); final: {(key, node index):
    vol_attached}, 0 elsewhere.  Both hold for pin=True only.
    soft: a ScheduleAnyway zone constraint on every other pod and zone labels on the nodes (the batch
    has programs: k_spread's form); the pins leave one feasible node, so nothing else changes.
    wide: 126 filler nodes behind n23; every fifth limits every key to 0, the others limit none of
    the CSI keys and keep the in-tree defaults.  drop: names of pending pods left out."""
    alloc = [dict() for _ in range(N_NODES)]
    drivers = [[] for _ in range(N_NODES)]
    for k in range(8):
        for n, c in ((G[k], LIMIT_G), (H[k], LIMIT_H)):
            a, d = _limits(k, c)
            alloc[n].update(a)
            if d:
                drivers[n].append(d)
    nodes = [node(_name(i), extra=alloc[i], labels={ZONE: "z%d" % (i % 3)} if soft else None) for i in range(N_NODES)]
    csinodes = [{"metadata": {"name": _name(i)}, "spec": {"drivers": drivers[i]}} for i in range(N_NODES) if drivers[i]]
    if wide:
        for i in range(N_FILL):
            a, ds = {}, []
            if i % 5 == 0:
                for k in range(8):
                    ak, d = _limits(k, 0)
                    a.update(ak)
                    if d:
                        ds.append(d)
                csinodes.append({"metadata": {"name": "x%03d" % i}, "spec": {"drivers": ds}})
            nodes.append(node("x%03d" % i, extra=a, labels={ZONE: "z%d" % (i % 3)} if soft else None))
    pvs, pvcs, bound, pods, expect, final = [], [], [], [], [], {}

    def claim(k, tag):
        """A PVC-backed volume of key k (VolumeRestrictions looks at inline volumes only)."""
        nm = "k%d-%s" % (k, tag)
        if not any(p["metadata"]["name"] == "pv-" + nm for p in pvs):
            pvs.append(vf.pv("pv-" + nm, _source(k, "id-" + nm)))
            pvcs.append(vf.pvc("c-" + nm, "pv-" + nm))
        return vf.claim("c-" + nm)

    def private(k, tag):
        """A volume no other pod names: inline for the in-tree plugins, a claim for CSI."""
        return _source(k, "only-%d-%s" % (k, tag)) if k in IN_TREE_KEY else claim(k, "only-" + tag)

    def pending(name, at, vols, ok, fail=0):
        if name in drop:
            return
        p = vf.vpod(name, *vols)
        p["metadata"]["labels"] = {"app": "w"}
        if pin:
            p["spec"]["nodeSelector"] = {HOST: _name(at)}
        if soft and len(pods) % 2 == 0:
            p["spec"]["topologySpreadConstraints"] = [{"maxSkew": 1, "topologyKey": ZONE, "whenUnsatisfiable": "ScheduleAnyway",
                                                       "labelSelector": {"matchLabels": {"app": "w"}}}]
        pods.append(p)
        expect.append((name, at, at if ok else -1, fail))

    for k in range(8):
        bound.append(vf.vpod("hold-g%d" % k, claim(k, "a"), node_name=_name(G[k])))
        bound.append(vf.vpod("hold-h%d" % k, claim(k, "c"), claim(k, "held"), node_name=_name(H[k])))
    for k in range(8):
        pending("p1-k%d" % k, G[k], [claim(k, "a"), claim(k, "b")], True)
        pending("p2-k%d" % k, G[k], [private(k, "p2")], True)
        pending("p3-k%d" % k, G[k], [private(k, "p3")], False, PLUGIN[k])
        csi = PLUGIN[k] == abi.KSS_F_NODE_VOLUME_LIMITS
        pending("pc-k%d" % k, H[k], [claim(k, "c")], csi, 0 if csi else PLUGIN[k])
        final[(k, G[k])] = 3
        final[(k, H[k])] = 2
    pending("d5", G[5], [private(0, "d5"), private(5, "d5")], False, abi.KSS_F_NODE_VOLUME_LIMITS)
    pending("d7", G[7], [private(0, "d7"), private(7, "d7")], False, abi.KSS_F_AZURE_DISK_LIMITS)
    pending("u", G[5], [private(4, "u")], True)
    final[(4, G[5])] = 1
    return dict(nodes=nodes, bound=bound, pods=pods, storage=vf.storage(pvs, pvcs, [], csinodes), expect=expect, final=final)


def compiled(fx):
    """compile_cluster of a fixture, with the layout the module states asserted: 8 keys in the order
    [EBS, GCE PD, CSI x 5, Azure Disk], the hand-counted A_k, at most 64 rows."""
    cc, cp, _ = compile_cluster(fx["nodes"], fx["bound"], fx["pods"], storage=fx["storage"])
    cs = cc.as_struct()
    assert cs.n_vol_keys == 8 and cs.n_vol_rows <= 64, (cs.n_vol_keys, cs.n_vol_rows)
    assert [int(x) for x in cc.arrays["vol_key_plugin"][:8]] == PLUGIN
    assert cc.vol_keys[2:7] == ["attachable-volumes-csi-" + d for d in DRIVERS]
    assert cc.node_names[:N_NODES] == [_name(i) for i in range(N_NODES)]
    return cc, cp


def adds(cc, cp):
    """A_k from the pods' programs (vol_form_admit's vol_add): every pod's own rows and private counts."""
    R = cc.as_struct().n_vol_rows
    rowkey = [int(x) for x in cc.arrays["vol_row_key"][:R]]
    out = [0] * 8
    for j in range(cp.n):
        _, _, own, _, _, padd = vff.pod_masks(cc, cp, j)
        for k in range(8):
            out[k] += sum(1 for r in range(R) if (own >> r) & 1 and rowkey[r] == k) + padd[k]
    return out


def margins(cc, cp):
    """Per key (att_max + A_k, lim_max): vol_fields_fit admits iff both are <= 65534 for every key."""
    a = adds(cc, cp)
    N = cc.n_nodes
    return [(max(int(cc.arrays["vol_attached"][k][:N].max()), 0) + a[k], int(cc.arrays["vol_limit"][k][:N].max()))
            for k in range(8)]


def inside(cc, cp):
    return all(m <= FIELD_MAX and l <= FIELD_MAX for m, l in margins(cc, cp))


def pack(cc):
    """Per node (used, a0, a1, l0, l1) in Python integers, as k_vol_pack / vol_pack_host pack them
    (values that do not fit are clamped to 65534 there and the batch is refused; asserted absent here
    only by the callers that need it)."""
    cs = cc.as_struct()
    N, R, K = cc.n_nodes, cs.n_vol_rows, cs.n_vol_keys
    arr = cc.arrays
    out = []
    for n in range(N):
        used = sum(1 << r for r in range(min(R, 64)) if int(arr["vol_count"][r][n]) > 0)
        a, l = [0, 0], [0, 0]
        for k in range(min(K, 8)):
            av, lv = int(arr["vol_attached"][k][n]), int(arr["vol_limit"][k][n])
            a[k >> 2] |= min(max(av, 0), FIELD_MAX) << (16 * (k & 3))
            l[k >> 2] |= (UNCHECKED if lv < 0 else min(lv, FIELD_MAX)) << (16 * (k & 3))
        out.append((used, a[0], a[1], l[0], l[1]))
    return out


def field(word, pos):
    return (word >> (16 * pos)) & 0xFFFF


# --------------------------------------------------------------------------------------
# field_tops
# --------------------------------------------------------------------------------------
CROSS_KEYS = (0, 3, 4, 7)
CARRY_EDGES = (255, 32767)
VARIANTS = ([("limit_top", None)] + [("limit_top", k) for k in CROSS_KEYS]
            + [("sum_top", False), ("sum_top", True)]
            + [("limit_max", (k, x)) for k in (3, 6) for x in (False, True)]
            + [("carry", (e, m)) for e in CARRY_EDGES for m in (False, True)]
            + [("unchecked_beside_max", None)])


def variant_id(v):
    name, arg = v
    if arg is None:
        return name
    if name == "carry":
        return "carry-%d-%s" % (arg[0], "mirrored" if arg[1] else "plain")
    if isinstance(arg, tuple):
        return "%s-key%d-%s" % (name, arg[0], "across" if arg[1] else "inside")
    if isinstance(arg, bool):
        return "%s-%s" % (name, "across" if arg else "inside")
    return "%s-across-key%d" % (name, arg)


def field_tops(variant, arg=None, soft=False, wide=False):
    """dict(cc, cp, across: None or the crossing key, expect, final; the last two None where the
    hand-derived figures do not apply).  soft, wide: eight_keys' parameters.

    limit_top   per key: on G[k] limit 65535 - A_k, attached two below it (both shifted by one
                constant); on H[k] limit 65533 - A_k, attached 65534 - A_k (one above it, as in
                eight_keys) -- the key's largest loaded count, so att_max + A_k == 65534 exactly.
                arg = k: H[k]'s loaded count one higher (across under key k).
    sum_top     key 6 without p3-k6 and pc-k6, and k6-a not yet on G[6] (its vol_count cell zeroed), so
                both pods that can add under key 6 do, by all they can (A_6 = 3): G[6] loads 65531
                against a limit of 65534 and ends on 65534; H[6] does not limit the key and loads 65531
                beside it.  arg = True: p3-k6 stays (A_6 = 4, across; it fails at 65534 + 1).
    limit_max   arg = (k, across): node n23's limit for key k is 65534 (inside) or 65535 (across);
                small counts.
    carry       arg = (edge, mirrored): on every G[k] the key's field moves edge - 1 -> edge -> edge + 1
                (limit edge + 1; edge 255 and 32767), the key below it holds 65534 - A on the same node
                and the key above it 0 (mirrored: above 65534 - A, below 0).  A carry out of the moving
                field or a borrow into it changes a neighbour's final count.
    unchecked_beside_max
                on G[5] keys 4 (limit -1) and 5 (limit h + 2) both load h = 65534 - 6: u passes under
                key 4 (h -> h + 1), p3-k5 and d5 fail under key 5."""
    drop = ()
    if variant == "sum_top":
        drop = ("pc-k6",) if arg else ("pc-k6", "p3-k6")
    fx = eight_keys(pin=True, soft=soft, wide=wide, drop=drop)
    cc, cp = compiled(fx)
    a = adds(cc, cp)
    att, lim = cc.arrays["vol_attached"], cc.arrays["vol_limit"]
    final = dict(fx["final"])
    across = None
    hand = True

    def shift(k, n, c):
        att[k][n] += c
        lim[k][n] += c
        final[(k, n)] = final.get((k, n), 0) + c

    def hold(k, n, v):
        att[k][n] = v
        final[(k, n)] = final.get((k, n), 0) + v

    if variant == "limit_top":
        assert a == A, a
        for k in range(8):
            shift(k, G[k], 65535 - A[k] - LIMIT_G)
            shift(k, H[k], 65533 - A[k] - LIMIT_H)
            assert int(lim[k][G[k]]) == 65535 - A[k] and int(att[k][H[k]]) == FIELD_MAX - A[k]
        if arg is not None:
            across = arg
            att[arg][H[arg]] += 1
            final[(arg, H[arg])] += 1
    elif variant == "sum_top":
        hand = False  # another pod list; the C oracle alone is the reference
        assert a[6] == (4 if arg else 3), a
        row = [r for r, (kind, ku) in enumerate(cc.vol_rows) if kind == "vol" and ku[0] == 6 and ku[1].endswith("id-k6-a")]
        assert len(row) == 1 and int(cc.arrays["vol_count"][row[0]][G[6]]) == 1
        cc.arrays["vol_count"][row[0]][G[6]] = 0
        att[6][G[6]], lim[6][G[6]] = FIELD_MAX - 3, FIELD_MAX
        att[6][H[6]], lim[6][H[6]] = FIELD_MAX - 3, -1
        final = None
        across = 6 if arg else None
    elif variant == "limit_max":
        k, x = arg
        assert int(att[k][N_NODES - 1]) == 0
        lim[k][N_NODES - 1] = FIELD_MAX + (1 if x else 0)
        across = k if x else None
    elif variant == "carry":
        edge, mirrored = arg
        assert a == A, a
        for k in range(8):
            shift(k, G[k], edge + 1 - LIMIT_G)
            assert int(att[k][G[k]]) == edge - 1 and int(lim[k][G[k]]) == edge + 1
            hi, lo = (k + 1, k - 1) if mirrored else (k - 1, k + 1)
            if 0 <= hi < 8:
                assert int(att[hi][G[k]]) == 0
                hold(hi, G[k], FIELD_MAX - A[hi])
            if 0 <= lo < 8:
                assert int(att[lo][G[k]]) == 0
    elif variant == "unchecked_beside_max":
        assert a == A and A[4] == A[5], a
        h = FIELD_MAX - A[5]
        assert int(lim[4][G[5]]) == -1 and int(att[4][G[5]]) == 0
        hold(4, G[5], h)
        shift(5, G[5], h - 1)
        assert int(att[5][G[5]]) == h and int(lim[5][G[5]]) == h + 2
    else:
        raise ValueError(variant)
    assert inside(cc, cp) == (across is None), (variant, arg, margins(cc, cp))
    if across is not None:
        m = margins(cc, cp)
        assert [k for k in range(8) if m[k][0] > FIELD_MAX or m[k][1] > FIELD_MAX] == [across], m
        assert max(m[across]) == FIELD_MAX + 1  # one unit across
    return dict(cc=cc, cp=cp, across=across, expect=fx["expect"] if hand else None, final=final if hand else None)


def final_attached(cc, final):
    """The hand-derived final vol_attached as an array."""
    out = np.zeros((8, cc.n_nodes), np.int32)
    for (k, n), v in final.items():
        out[k][n] = v
    return out


# --------------------------------------------------------------------------------------
# a context's life: the form is admitted on the device's current columns (vol_pack_state)
# --------------------------------------------------------------------------------------
LIFE_NODE, LIFE_KEY = N_NODES - 1, 6
LIFE_LOAD = FIELD_MAX - 4


def lifetime(soft=False):
    """dict(cc, cp, slices).  eight_keys without key 6's group, then pods pinned to n23, which limits
    no CSI key: x1 .. x6 with one private volume of key 6 each, lo1 and lo2 with a private EBS volume and
    a private volume of key 3 (keys 0-3 only).  attached[6][n23] loads 65530.  slices, as (first, n):
      A  the eight_keys pods and x1 x2 x3: adds 3 under key 6, in the form, ends on 65533
      B  x4: 65533 + 1 fits, in the form, ends on 65534
      C  x5: 65534 + 1 does not fit: k_schedule, leaves 65535
      D  lo1 lo2: nothing under key 6, but its loaded maximum is across: k_schedule, 65535 stays
         (a form run would pack the clamped 65534 and write it back)
      E  x6: after the count is taken back to 65533, in the form again, ends on 65534"""
    group = tuple("%s-k%d" % (p, LIFE_KEY) for p in ("p1", "p2", "p3", "pc"))
    fx = eight_keys(pin=True, soft=soft, drop=group)
    n0 = len(fx["pods"])
    pvs, pvcs = fx["storage"]["pvs"], fx["storage"]["pvcs"]

    def pinned(name, vols):
        p = vf.vpod(name, *vols)
        p["metadata"]["labels"] = {"app": "w"}
        p["spec"]["nodeSelector"] = {HOST: _name(LIFE_NODE)}
        fx["pods"].append(p)

    def own_claim(k, tag):
        nm = "k%d-only-%s" % (k, tag)
        pvs.append(vf.pv("pv-" + nm, _source(k, "id-" + nm)))
        pvcs.append(vf.pvc("c-" + nm, "pv-" + nm))
        return vf.claim("c-" + nm)

    for i in (1, 2, 3, 4, 5):
        pinned("x%d" % i, [own_claim(LIFE_KEY, "x%d" % i)])
    for i in (1, 2):
        pinned("lo%d" % i, [_source(0, "only-0-lo%d" % i), own_claim(3, "lo%d" % i)])
    pinned("x6", [own_claim(LIFE_KEY, "x6")])
    cc, cp = compiled(fx)
    assert cp.n == n0 + 8 and int(cc.arrays["vol_limit"][LIFE_KEY][LIFE_NODE]) == -1
    assert int(cc.arrays["vol_limit"][3][LIFE_NODE]) == -1 and int(cc.arrays["vol_attached"][LIFE_KEY][LIFE_NODE]) == 0
    cc.arrays["vol_attached"][LIFE_KEY][LIFE_NODE] = LIFE_LOAD
    for j in (n0 + 5, n0 + 6):  # lo1, lo2: keys 0 and 3 only
        assert vff.pod_masks(cc, cp, j)[3] == (1 << 0 | 1 << 3)
    slices = dict(A=(0, n0 + 3), B=(n0 + 3, 1), C=(n0 + 4, 1), D=(n0 + 5, 2), E=(n0 + 7, 1))
    return dict(cc=cc, cp=cp, slices=slices)
