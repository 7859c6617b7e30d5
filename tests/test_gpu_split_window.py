"""percentageOfNodesToScore < 100 on the split grid (kss/split.py): the
findNodesThatPassFilters window of k_simple (simple_sync_win) and k_spread (spread_schedule WIN)
with the grid's shards spread over several parts, against the C oracle's restatement of the window
(oracle_c.schedule(..., cursor=), st["next_start"]).

Every case starts from a set cursor inside the LAST part's rows, a third of a window before the
end of the node list, so the first pod's window wraps from the last part into part 0; it runs
twice (reset and the cursor set again between; the second run continues the inbox epochs) and
compares, on every part: the loop kernel, the shard count, the chosen nodes, the per-pod outcomes
(n_feasible = the kept nodes), the node state assembled from the parts' rows, and the cursor word
of every part.  Before this capability every case raised KssError ("split grid: the batch needs
k_schedule").

The oracle side of every case was run on the CPU first (the figures are its own, with "cut" a pod
whose search stopped early, F > K).  Each case takes under 0.4 s on 16 threads, the 100,000-node
one 1.4 s.  k_simple, config 2: 5,000 nodes pct 0 400/400 pods cut, pct 30 303/400; 3,000 nodes
242/300; 8,000 nodes 300/300; 180 nodes 225/300.  k_spread: config 4 6,000 nodes pct 0 200/200,
pct 30 165/200; 20,000 nodes 299/300; 100,000 nodes 200/200; config 3 3,000 nodes pct 0 216/300,
pct 30 134/300 (its pods with node selectors have fewer than K = 900 feasible nodes whatever the
pod count: 20 to 28 of every 50 pods cut).  In all of these st["next_start"] ends away from the
set cursor (asserted).  Two cases are edges of the other kind, F <= K: 101 nodes (K = 100; config
2 has at most 92 feasible nodes there, so no pod cuts and the cursor stays where it was set), and
the saturating batch (150 nodes, 5,000 pods: unschedulable from pod 4,005 on).
"""
import os

import numpy as np
import pytest

import oracle_c
from kss import abi, native, split
from kss.synth import SEED_BASE

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
CLEAN = {"reloads": 0, "shadow": 0, "final": 0}


def _prof(pct, custom=False):
    p = abi.default_profile()
    p.pct_nodes_to_score = pct
    if custom:
        p.weight[abi.KSS_S_TAINT_TOLERATION] = 5
    return p


def k_find(n, pct):
    """v1.26 numFeasibleNodesToFind."""
    if n < 100 or pct >= 100:
        return n
    if pct <= 0:
        pct = max(5, 50 - n // 125)
    return max(100, n * pct // 100)


def start_cursor(n_nodes, n_parts, wl, pct):
    """A start node inside the last part's rows, a third of a window before the end of the list."""
    lo, hi = split.part_rows(n_nodes, n_parts, wl, n_parts - 1)
    c = hi - max(1, min(k_find(n_nodes, pct), hi - lo) // 3)
    assert lo <= c < hi == n_nodes
    return c


_ORACLE = {}


def oracle(config, n_nodes, n_pods, pct, n_parts, wl, custom=False):
    """(synth, profile, cursor, chosen, results, final state), computed once per case."""
    key = (config, n_nodes, n_pods, pct, n_parts, wl, custom)
    if key not in _ORACLE:
        s = native.Synth(config, SEED_BASE + config, n_nodes, n_pods)
        prof = _prof(pct, custom)
        cur = start_cursor(n_nodes, n_parts, wl, pct)
        ch_o, res, st = oracle_c.schedule(prof, s.cluster, s.pods, n_pods, n_nodes, record="meta", threads=THREADS,
                                          n_classes=s.cluster.n_classes, n_terms=s.cluster.n_terms, cursor=cur)
        _ORACLE.clear()  # one case's arrays at a time
        _ORACLE[key] = (s, prof, cur, ch_o, res, st)
    return _ORACLE[key]


def _check_parts(sp, outs, kernel, s, n_pods, ch_o, res, st, tag):
    N = s.n_nodes
    want_meta = np.array([[res.meta(j)[k] for k in ("chosen", "n_feasible", "scored", "status")]
                          for j in range(n_pods)], dtype=np.int64)
    for p, (c, ch) in enumerate(zip(sp.ctxs, outs)):
        assert c.last_kernel() == kernel, (tag, p)
        assert c.last_geometry()["shards"] == sp.n_parts * sp.wl, (tag, p)
        np.testing.assert_array_equal(ch, ch_o, err_msg=f"{tag} part {p} chosen")
        np.testing.assert_array_equal(c.fetch_meta(n_pods)[:, :4], want_meta, err_msg=f"{tag} part {p} outcomes")
        assert c.next_start_node_index() == st["next_start"], (tag, p)
        if kernel == "k_spread":
            assert c.last_handoff_status() == CLEAN, (tag, p)
    assert sp.next_start_node_index() == st["next_start"], tag
    g = sp.node_state()
    np.testing.assert_array_equal(g["requested"][:, :N], st["requested"][:, :N], err_msg=tag)
    np.testing.assert_array_equal(g["pod_count"][:N], st["pod_count"][:N], err_msg=tag)
    ncl = s.cluster.n_classes
    if ncl:
        np.testing.assert_array_equal(g["class_count"][:ncl, :N], st["class_count"][:ncl, :N], err_msg=tag)


def _run_case(config, n_nodes, n_pods, n_parts, wl, pct, kernel, custom=False, n_chunks=0):
    s, prof, cur, ch_o, res, st = oracle(config, n_nodes, n_pods, pct, n_parts, wl, custom)
    sp = split.InProcessSplit(s.cluster, s.pods, n_parts, wl, profile=prof)
    try:
        for rep in range(2):
            sp.reset()
            sp.set_next_start_node_index(cur)
            outs = sp.run(n_pods)
            if n_chunks:
                for c in sp.ctxs:  # k_static + the loop kernel per chunk, on every part
                    assert c.last_timing()[1] == 2 * n_chunks
            _check_parts(sp, outs, kernel, s, n_pods, ch_o, res, st, f"run {rep}")
    finally:
        sp.close()
    return ch_o, st, cur


@pytest.mark.parametrize("n_nodes,n_pods,n_parts,wl,pct", [
    (5000, 400, 2, 16, 0),
    (5000, 400, 2, 16, 30),
    (3000, 300, 2, 2, 0),    # 750-node shards: per-thread mode
    (8000, 300, 2, 40, 0),   # 80 shards: the sweep's second chunk of 64
    (5000, 400, 4, 4, 0),    # four parts
    (101, 300, 2, 2, 0),     # K = 100 of 101 nodes, the last shard short (23 of 26 nodes); F <= K
    (180, 300, 2, 2, 0),     # K = 100 of 180 nodes: four shards of 45, most pods cut
])
def test_k_simple_window_across_parts(n_nodes, n_pods, n_parts, wl, pct):
    _, st, cur = _run_case(2, n_nodes, n_pods, n_parts, wl, pct, "k_simple")
    assert (st["next_start"] != cur) == (n_nodes != 101)  # (101 nodes: never more than K feasible)


def test_k_simple_window_saturating_batch():
    """150 nodes, 5,000 pods: the cluster fills up, the pods from 4,005 on are unschedulable and the
    ones before them see F <= K = 100 feasible nodes -- every node visited, the cursor stays."""
    ch_o, st, _ = _run_case(2, 150, 5000, 2, 2, 0, "k_simple")
    assert (ch_o < 0).any()


def test_k_simple_window_custom_profile():
    """One weight changed: k_simple<false, true>, the profile read from LDS."""
    _run_case(2, 5000, 400, 2, 16, 0, "k_simple", custom=True)


@pytest.mark.parametrize("config,n_nodes,n_pods,wl,pct", [
    (4, 6000, 200, 16, 0),
    (4, 6000, 200, 16, 30),
    (3, 3000, 300, 12, 0),
    (3, 3000, 300, 12, 30),
    (4, 20000, 300, 40, 0),     # 80 shards: every wave sweeps a share of the 81-value count vector
    (4, 100000, 200, 128, 0),   # the deployment shape: 256 shards, 257 values per shard
])
def test_k_spread_window_across_parts(config, n_nodes, n_pods, wl, pct):
    _, st, cur = _run_case(config, n_nodes, n_pods, 2, wl, pct, "k_spread")
    assert st["next_start"] != cur


@pytest.mark.parametrize("config,n_nodes,n_pods,per_chunk,wl,kernel", [
    (2, 3000, 240, 50, 8, "k_simple"),
    (4, 6000, 200, 40, 16, "k_spread"),
])
def test_window_across_parts_and_chunks(config, n_nodes, n_pods, per_chunk, wl, kernel):
    """Five chunk launches per run: every launch of every part reads the cursor word its own
    previous launch left, so a part whose word was not written between launches splits the next
    chunk's first pod at a stale start node."""
    native.set_option("static_bytes", 4 * n_nodes * per_chunk)
    n_chunks = -(-n_pods // per_chunk)
    assert n_chunks >= 4
    _run_case(config, n_nodes, n_pods, 2, wl, 0, kernel, n_chunks=n_chunks)


def test_name_listed_pods_stay_refused():
    """PreFilterResult name lists under a window need k_schedule: a split grid refuses the batch
    before it assigns any epoch.  The refusal leaves the parts armed (no re-arm asked for): the same
    contexts then run the batch without its name lists, windowed; and a pct-100 grid of the same
    shape (a context's profile is fixed when it is created) runs the name-listed batch."""
    from kss import synth
    from kss.compile import compile_cluster
    from test_oracle_crosscheck import with_name_sets
    nodes, bound, plain = synth.make_cluster(2, 900, 60)
    listed = with_name_sets(plain, [n["metadata"]["name"] for n in nodes], every=3, size=120)
    cc, cp, _ = compile_cluster(nodes, bound, listed)
    _, cq, _ = compile_cluster(nodes, bound, plain)
    N, n = cc.n_nodes, cp.n
    win, full = _prof(0), abi.default_profile()
    sp = split.InProcessSplit(cc.as_struct(), cp.as_struct(), 2, 4, profile=win)
    for c in sp.ctxs:
        with pytest.raises(native.KssError, match="k_schedule"):
            c.run_staged(n)
    cur = start_cursor(N, 2, 4, 0)
    ch_w, _, st_w = oracle_c.schedule(win, cc.as_struct(), cq.as_struct(), n, N, record="meta", threads=THREADS,
                                      cursor=cur)
    for c in sp.ctxs:
        c.stage(cq.as_struct())
    sp.set_next_start_node_index(cur)
    for p, ch in enumerate(sp.run(n)):
        np.testing.assert_array_equal(ch, ch_w, err_msg=f"part {p} after the refusal")
    assert sp.next_start_node_index() == st_w["next_start"]
    sp.close()
    ch_o, _, _ = oracle_c.schedule(full, cc.as_struct(), cp.as_struct(), n, N, record="meta", threads=THREADS)
    sp = split.InProcessSplit(cc.as_struct(), cp.as_struct(), 2, 4, profile=full)
    for p, ch in enumerate(sp.run(n)):
        np.testing.assert_array_equal(ch, ch_o, err_msg=f"part {p} at pct 100")
    sp.close()


def _rank_main(rank, world, port, config, n_nodes, n_pods, wl, cursor, q, device_of=None):
    import torch
    import torch.distributed as dist
    try:
        dev = device_of(rank) if device_of else 0
        torch.cuda.set_device(dev)
        torch.zeros(1, device="cuda")  # torch's HIP runtime before libkss's
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        s = native.Synth(config, SEED_BASE + config, n_nodes, n_pods)
        r = split.SplitRank(s.cluster, s.pods, wl, profile=_prof(0), device=dev)
        r.set_next_start_node_index(cursor)
        chosen = r.run(n_pods)
        q.put((rank, chosen.tolist(), r.next_start_node_index(), r.ctx.last_kernel(), r.ctx.last_handoff_status()))
        dist.barrier()
        r.close()
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001 - reported to the parent
        q.put((rank, repr(e), None, None, None))


def _identity(r):
    return r


def _n_devices():
    import torch
    return torch.cuda.device_count()


@pytest.mark.parametrize("two_gpus", [
    False,
    pytest.param(True, marks=pytest.mark.skipif(_n_devices() < 2, reason="needs 2 GPUs")),
])
def test_window_across_processes(two_gpus):
    """One part per process, inboxes through IPC handles exchanged over gloo: the chosen nodes and
    each rank's cursor word."""
    import multiprocessing as mp
    import socket
    world, config, n_nodes, n_pods, wl = 2, 4, 20000, 300, 32
    s, prof, cur, ch_o, res, st = oracle(config, n_nodes, n_pods, 0, world, wl)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_rank_main, args=(r, world, port, config, n_nodes, n_pods, wl, cur, q,
                                               _identity if two_gpus else None)) for r in range(world)]
    for p in ps:
        p.start()
    got = [q.get(timeout=240) for _ in ps]
    for p in ps:
        p.join(timeout=60)
    for rank, chosen, cursor, kernel, handoff in got:
        assert kernel is not None, chosen  # the child's exception
        assert kernel == "k_spread"
        assert handoff == CLEAN, (rank, handoff)
        np.testing.assert_array_equal(np.array(chosen), ch_o, err_msg=f"rank {rank}")
        assert cursor == st["next_start"], rank
