"""Rollback programs over pods with WaitForFirstConsumer claims (test infrastructure): the step
lists the CPU and GPU tests share, both oracles run over them, and the assume cache decoded to
names.  A program is a list of steps: j >= 0 schedules and assumes pod j, -1 - j is pod j's
Unreserve (RevertAssumedPodVolumes and ForgetPod) -- tests/oracle_c.py schedule(ops=...)."""
import k8s_oracle
import k8s_volumes
import oracle_c
from kss import abi


def ops_immediate(n, every):
    """Commit, roll back, go on: every `every`-th pod is rolled back right after its commit."""
    ops = []
    for j in range(n):
        ops.append(j)
        if j % every == every - 1:
            ops.append(-1 - j)
    return ops


def ops_lifo(n, run, gap):
    """Commit a run, roll the run back in reverse, go on: after every `gap` pods the last `run`
    of them are rolled back, newest first."""
    ops = []
    for j in range(n):
        ops.append(j)
        if j % gap == gap - 1:
            ops += [-1 - i for i in range(j, j - run, -1)]
    return ops


def object_oracle(nodes, bound, st):
    return k8s_oracle.Oracle(nodes, bound, storage=k8s_volumes.Storage(
        st["pvs"], st["pvcs"], st["storage_classes"], st["csinodes"]))


def cache_of(o):
    """The object oracle's assume cache: ({PV: claim}, {claim: node name})."""
    return ({pv: ref[1] for pv, ref in o.storage.pv_ref.items()},
            {k[1]: v for k, v in o.storage.selected.items()})


def run_object_oracle(nodes, bound, pods, st, ops, on_rollback=None):
    """The object oracle over a program.  Per step a dict: chosen (node index or -1; for an Unreserve
    the node left), res (schedule_one's result, None for an Unreserve), ann (its annotations), and
    the assume cache after the step (bound, selected).  on_rollback(o, pod) is called before each
    Unreserve."""
    o = object_oracle(nodes, bound, st)
    on = {}
    out = []
    for op in ops:
        j = op if op >= 0 else -1 - op
        if op >= 0:
            r = o.schedule_one(pods[j])
            ch = -1 if r["selected"] is None else r["selected"]
            if ch >= 0:
                on[j] = ch
        else:
            r, ch = None, on.pop(j, -1)
            if ch >= 0:
                if on_rollback:
                    on_rollback(o, pods[j])
                o.forget(pods[j], ch)
        b, s = cache_of(o)
        out.append(dict(chosen=ch, res=r, ann=o.annotations(r) if r is not None else None, bound=b, selected=s))
    return out


def run_c_oracle(cc, cp, ops, record=True, skip_commit=None):
    return oracle_c.schedule(abi.default_profile(), cc.as_struct(), cp.as_struct(), cp.n, cc.n_nodes, record=record,
                             n_classes=len(cc.classes), n_terms=len(cc.terms), ops=ops, trace=True,
                             skip_commit=skip_commit)


def decode(cc, pv_owner, claim_node):
    """The compiled assume-cache columns as names: ({PV: claim}, {claim: node name, "" for a node
    outside the snapshot})."""
    bound = {cc.pvs[v]: cc.wclaims[int(o) - 1][1] for v, o in enumerate(pv_owner) if o}
    sel = {cc.wclaims[c][1]: (cc.node_names[int(n)] if n >= 0 else "") for c, n in enumerate(claim_node) if n != -1}
    return bound, sel


def restrict(cc, bound, selected):
    """The object oracle's cache over the PVs and claims the compiled cluster carries (those some
    pending pod's delayed claim can reach), nodes outside the snapshot as ""."""
    pvs, claims = set(cc.pvs), {k[1] for k in cc.wclaims}
    return ({pv: c for pv, c in bound.items() if pv in pvs},
            {c: (n if n in cc.node_names else "") for c, n in selected.items() if c in claims})
