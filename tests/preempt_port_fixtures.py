"""DefaultPreemption with host ports (test infrastructure): preemptors whose NodePorts failure
is resolved by evicting the pod that holds the port.  The object-level restatement
(oracle/k8s_preemption.py) answers these; kss_postfilter_pod still refuses a preemptor with
host ports, so the fixtures are the reference a device dry run with UsedPorts has to meet
(DESIGN.md §8).

Hand-derived cases, in the style of preempt_fixtures.fixture (2-CPU nodes, every pending pod
selects one node group, so the other groups' nodes fail NodeAffinity and are never potential).
NodeInfo.UsedPorts is a set (framework.HostPortInfo): AddPod adds the pod's (ip, protocol, port)
entries, RemovePod removes them whoever else holds the same entry; a wanted port conflicts with a
used entry of the same protocol and port when either IP is 0.0.0.0 or both are equal.

  H1 eviction frees the port   a: a-web (prio 1, TCP 80, t0), a-other (prio 1, no port, t10);
                               b: b-web (prio 100, TCP 80).
       p1 (prio 10, 100m, TCP 80) fails NodePorts on both (Unschedulable: both potential).
       a: remove both -> port free; reprieve a-web -> TCP 80 held again -> victim; a-other is
       reprieved.  b has no lower-priority pod.  -> nominate a, victims [a-web], 1 candidate.
  H2 wildcard and protocol     c: c-ip (prio 1, 10.0.0.1 TCP 8080), c-udp (prio 1, UDP 8080).
       p2 (prio 10, TCP 8080 on 0.0.0.0) conflicts with c-ip (a wildcard wants every IP) and
       not with c-udp (another protocol) -> victims [c-ip], c-udp reprieved.
  H3 ports and resources       d: d-port (prio 1, 500m, TCP 443), d-big (prio 5, 1500m);
                               e: e-port (prio 1, 2000m, TCP 443).
       p3 (prio 10, 1000m, TCP 443).  d: reprieve d-big (1500 + 1000 > 2000) fails, reprieve
       d-port (port and 500 + 1000 fits, but TCP 443) fails -> [d-big, d-port]; e: [e-port].
       Highest victim priority 1 < 5 -> nominate e, 2 candidates.
  H4 a nominee's port          f: f-low (prio 1, TCP 53).  `nom` (prio 50, TCP 53) nominated to f:
       p4 (prio 10, TCP 53) sees the nominee's port in the first pass of every filter call, so
       even with f-low removed the node fails -> no candidate (1 potential node).  Without the
       nomination: nominate f, victims [f-low].
  H5 set semantics             g: g-hi (prio 100, TCP 9000, t0), g-lo (prio 1, TCP 9000, t10).
       p5 (prio 10, TCP 9000): removing g-lo removes the entry from the set although g-hi holds
       it too (HostPortInfo.Remove), so the node fits; the reprieve of g-lo adds it back ->
       nominate g, victims [g-lo].  A per-entry count would answer no candidate.
The nodes s0..s6 (group "spare") bring the cluster to 14 nodes; some hold ports of their own.

bit63(): a second cluster whose port dictionary has exactly 64 entries, the only conflicting
holder's entry being the last one (bit 63 of the UsedPorts word).
"""
import preempt_fixtures as pf

T0, T10 = pf.T0, pf.T10


def with_ports(pod, *ports):
    """ports: (hostPort, protocol, hostIP or None) added to the pod's only container."""
    out = []
    for port, proto, ip in ports:
        e = {"containerPort": port, "hostPort": port, "protocol": proto}
        if ip:
            e["hostIP"] = ip
        out.append(e)
    pod["spec"]["containers"][0]["ports"] = out
    return pod


def entries(pod):
    """The pod's (ip, protocol, port) entries as HostPortInfo keeps them."""
    return [(p.get("hostIP") or "0.0.0.0", p.get("protocol") or "TCP", int(p["hostPort"]))
            for c in pod["spec"]["containers"] for p in c.get("ports") or [] if int(p.get("hostPort") or 0) > 0]


def conflict(a, b):
    return a[1:] == b[1:] and (a[0] == "0.0.0.0" or b[0] == "0.0.0.0" or a[0] == b[0])


def fixture():
    """(nodes, bound, pods, cases); a case: pod name, nominations [(pod name, node name)] in the
    nominator during its dry run, and the expected (status, node, victims), n_potential and
    n_candidates (None: not stated).  Every dry run is against the unchanged snapshot."""
    P = with_ports
    nodes = [pf.node("a", "g1"), pf.node("b", "g1"), pf.node("c", "g2"), pf.node("d", "g3"), pf.node("e", "g3"),
             pf.node("f", "g4"), pf.node("g", "g5")] + [pf.node("s%d" % i, "spare") for i in range(7)]
    bound = [P(pf.pod("a-web", 1, "100m", "a", T0), (80, "TCP", None)), pf.pod("a-other", 1, "100m", "a", T10),
             P(pf.pod("b-web", 100, "100m", "b", T0), (80, "TCP", None)),
             P(pf.pod("c-ip", 1, "100m", "c", T0), (8080, "TCP", "10.0.0.1")),
             P(pf.pod("c-udp", 1, "100m", "c", T10), (8080, "UDP", None)),
             P(pf.pod("d-port", 1, "500m", "d", T0), (443, "TCP", None)), pf.pod("d-big", 5, "1500m", "d", T0),
             P(pf.pod("e-port", 1, "2000m", "e", T0), (443, "TCP", None)),
             P(pf.pod("f-low", 1, "100m", "f", T0), (53, "TCP", None)),
             P(pf.pod("g-hi", 100, "100m", "g", T0), (9000, "TCP", None)),
             P(pf.pod("g-lo", 1, "100m", "g", T10), (9000, "TCP", None)),
             P(pf.pod("s0-x", 1, "100m", "s0", T0), (80, "UDP", None), (443, "TCP", "10.0.0.2")),
             P(pf.pod("s3-x", 1000, "100m", "s3", T0), (53, "UDP", None)),
             pf.pod("s5-x", 1, "100m", "s5", T0)]
    pods = [P(pf.pod("p1", 10, "100m", group="g1"), (80, "TCP", None)),
            P(pf.pod("p2", 10, "100m", group="g2"), (8080, "TCP", None)),
            P(pf.pod("p3", 10, "1000m", group="g3"), (443, "TCP", None)),
            P(pf.pod("p4", 10, "100m", group="g4"), (53, "TCP", None)),
            P(pf.pod("p5", 10, "100m", group="g5"), (9000, "TCP", None)),
            P(pf.pod("nom", 50, "100m", group="g4"), (53, "TCP", None))]
    cases = [dict(name="H1", pod="p1", noms=[], expect=("nominated", "a", ["a-web"]), n_potential=2, n_candidates=1),
             dict(name="H2", pod="p2", noms=[], expect=("nominated", "c", ["c-ip"]), n_potential=None, n_candidates=None),
             dict(name="H3", pod="p3", noms=[], expect=("nominated", "e", ["e-port"]), n_potential=None, n_candidates=2),
             dict(name="H4", pod="p4", noms=[("nom", "f")], expect=("no_candidate", None, []), n_potential=1,
                  n_candidates=0),
             dict(name="H4-plain", pod="p4", noms=[], expect=("nominated", "f", ["f-low"]), n_potential=None,
                  n_candidates=None),
             dict(name="H5", pod="p5", noms=[], expect=("nominated", "g", ["g-lo"]), n_potential=None, n_candidates=None)]
    return nodes, bound, pods, cases


def bit63():
    """(nodes, bound, pods, holder entry): 62 filler entries (0.0.0.0 TCP 1000..1061) held by four
    pods of node x, two of them below the preemptor's priority (reprieved: their bits return to
    the dry-run word), the preemptor's own entry (0.0.0.0 TCP 60000) and the holder's
    (10.0.0.9 TCP 60000), which sorts last.  The expectation comes from the oracle."""
    nodes = [pf.node("x", "g1"), pf.node("y", "g1"), pf.node("z", "g2")]
    fill = [(1000 + i, "TCP", None) for i in range(62)]
    bound = [with_ports(pf.pod("x-f0", 100, "100m", "x", T0), *fill[0:16]),
             with_ports(pf.pod("x-f1", 1, "100m", "x", T0), *fill[16:32]),
             with_ports(pf.pod("x-hold", 1, "100m", "x", T10), (60000, "TCP", "10.0.0.9")),
             with_ports(pf.pod("x-f2", 1, "100m", "x", "2024-01-01T00:00:20Z"), *fill[32:47]),
             with_ports(pf.pod("x-f3", 100, "100m", "x", T10), *fill[47:62]),
             with_ports(pf.pod("y-hold", 100, "100m", "y", T0), (60000, "TCP", None)),
             pf.pod("z-1", 1, "100m", "z", T0)]
    pods = [with_ports(pf.pod("p63", 10, "100m", group="g1"), (60000, "TCP", None))]
    return nodes, bound, pods, ("10.0.0.9", "TCP", 60000)


# --------------------------------------------------------------------------------------
# Seeded saturated clusters with host ports: preempt_fixtures.saturated, then about 70 % of the
# bound pods hold one or two host ports (a pod's ports are dropped when they conflict with what
# its node already holds: a state the scheduler could have produced), about 70 % of the pending
# pods want such ports, and half of those ask for 250m only, so that the port and not the CPU
# decides their dry runs.  12 dictionary entries at most.
#
# The (seed, nodes, pods) meant for device parity tests; tests/test_preemption_ports.py checks on the
# oracle alone that each reaches host-port nominations whose victims hold a conflicting entry.  60
# and 130 nodes leave k_preempt_nodes' last 64-lane workgroup partial, 64 fills one exactly.
SEEDED = [(5, 60, 40), (4, 130, 60), (1, 64, 50)]
SEQUENCE = (1, 64, 50)      # the eval -> PostFilter -> evict -> nominate -> retry loop
BATCH = (2, 80, 60, 30)     # the first 30 pods placed by a recorded batch


def _draw(r):
    out = []
    for _ in range(r.choice([1, 2])):
        e = (r.choice([None, None, "10.0.0.1", "10.0.0.2"]) or "0.0.0.0", r.choice(["TCP", "UDP"]), r.choice([80, 443]))
        if not any(conflict(e, x) for x in out):
            out.append(e)
    return out


def _as_args(es):
    return [(port, proto, None if ip == "0.0.0.0" else ip) for ip, proto, port in es]


def saturated_ports(seed: int, n_nodes: int, n_pods: int):
    import random
    nodes, bound, pods = pf.saturated(seed, n_nodes, n_pods)
    r = random.Random(1000 + seed)
    held = {}
    for b in bound:
        if r.random() >= 0.7:
            continue
        es = _draw(r)
        mine = held.setdefault(b["spec"]["nodeName"], [])
        if any(conflict(e, x) for e in es for x in mine):
            continue
        mine.extend(es)
        with_ports(b, *_as_args(es))
    for p in pods:
        if r.random() >= 0.7:
            continue
        with_ports(p, *_as_args(_draw(r)))
        if r.random() < 0.5:
            p["spec"]["containers"][0]["resources"]["requests"]["cpu"] = "250m"
    return nodes, bound, pods


def strip_ports(pods):
    """The same pods without host ports (copies)."""
    import copy
    out = copy.deepcopy(pods)
    for p in out:
        for c in p["spec"]["containers"]:
            c.pop("ports", None)
    return out
