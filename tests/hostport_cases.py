"""Host ports: a Python restatement of the conflict rule and of the port-bit encoding, seeded generators, and the
reference for a problem with host ports — the CPU oracle (which knows nothing of host ports) run on a transformed
problem in which every port bit is a spare resource axis with one unit of capacity:

  every instance type has allocatable = capacity = 1000 on the axis; a pod of a class that owns the bit requests 1000;
  a NodePool's daemon overhead carries 1000 for its daemonset ports; an existing node has 1000 available, or 0 when the
  bit is in its bound pods' mask; no NodePool limit is set on the axis.

resources.Fits then rejects exactly the Adds the port check rejects, a failed Add leaves no state, the queue order
reads only cpu and memory, and requirements, prices and option lists never see the axis: every output that
parity.assert_same compares must be equal.

The catalogs leave seven axes free once they are zeroed (every axis but cpu, memory, ephemeral-storage, pods and
nvidia.com/gpu), so an oracle-checked problem carries at most seven port bits.
"""
import copy
import dataclasses
import ipaddress

import numpy as np

from kpsim import model
from kpsim.model import HostPort

KEPT = ("cpu", "memory", "ephemeral-storage", "pods", "nvidia.com/gpu")
SPARE = [model.RIDX[r] for r in model.RESOURCES if r not in KEPT]   # axis of port bit b: SPARE[b]
UNIT = 1000


# ------------------------------------------------------------------------------------------------
# the rule ([core] scheduling/hostportusage.go, recalled) and the encoding (kp_host.cpp solve_host_ports)
# ------------------------------------------------------------------------------------------------
def _ip(hp):
    """None for an unspecified IP ("", 0.0.0.0, ::), else the address (IPv4 as its IPv4-mapped IPv6 form, as Go's
    net.IP compares them)."""
    if not hp.ip:
        return None
    a = ipaddress.ip_address(hp.ip)
    if a.is_unspecified:
        return None
    if a.version == 4:
        a = ipaddress.IPv6Address("::ffff:" + str(a))
    elif a.ipv4_mapped is not None and a.ipv4_mapped.is_unspecified:
        return None
    return a


def entries_conflict(a, b):
    """Two host-port entries conflict iff protocol and port are equal and the IPs are equal or one is unspecified."""
    if a.protocol != b.protocol or a.port != b.port:
        return False
    ia, ib = _ip(a), _ip(b)
    return ia is None or ib is None or ia == ib


def sets_conflict(xs, ys):
    return any(entries_conflict(a, b) for a in xs for b in ys)


def encode(rows):
    """rows: lists of HostPort (every class, NodePool and node of one input).  Returns (n_bits, [frozenset of owned bits
    per row]): per (protocol, port) group one wildcard bit plus one bit per distinct specific IP; an entry with a
    specific IP owns that bit, an unspecified one every bit of its group."""
    groups = {}
    for r in rows:
        for hp in r:
            g = groups.setdefault((hp.protocol, hp.port), set())
            if _ip(hp) is not None:
                g.add(_ip(hp))
    base, n = {}, 0
    for key in sorted(groups):
        ips = sorted(groups[key])
        base[key] = (n, {ip: n + 1 + i for i, ip in enumerate(ips)})
        n += 1 + len(ips)
    out = []
    for r in rows:
        own = set()
        for hp in r:
            b0, ipbit = base[(hp.protocol, hp.port)]
            if _ip(hp) is None:
                own.update(range(b0, b0 + 1 + len(ipbit)))
            else:
                own.add(ipbit[_ip(hp)])
        out.append(frozenset(own))
    return n, out


def problem_bits(prob):
    """(n_bits, per class, per NodePool, per existing node) owned-bit sets of a Problem."""
    C, NP = len(prob.classes), len(prob.nodepools)
    n, own = encode([pc.host_ports for pc in prob.classes] + [p.daemon_host_ports for p in prob.nodepools] +
                    [e.host_ports for e in prob.existing])
    return n, own[:C], own[C:C + NP], own[C + NP:]


# ------------------------------------------------------------------------------------------------
# catalogs and the transformed problem
# ------------------------------------------------------------------------------------------------
def derive_catalogs(catalog):
    """(device catalog, oracle catalog): the spare axes at 0, resp. at UNIT, in capacity and allocatable of every type."""
    dev, orc = [], []
    for it in catalog:
        for out, v in ((dev, 0), (orc, UNIT)):
            cap, al = np.array(it.capacity, np.int64), np.array(it.allocatable, np.int64)
            cap[SPARE] = v
            al[SPARE] = v
            out.append(dataclasses.replace(it, capacity=cap, allocatable=al))
    return dev, orc


def device_problem(prob, dev_catalog):
    """The problem as the device sees it: the derived catalog, nothing requested or available on the spare axes."""
    q = copy.copy(prob)
    q.catalog = dev_catalog
    q.pods = dataclasses.replace(prob.pods, requests=np.array(prob.pods.requests, np.int64))
    q.pods.requests[:, SPARE] = 0
    q.nodepools = []
    for p in prob.nodepools:
        d = None if p.daemon_overhead is None else np.array(p.daemon_overhead, np.int64)
        if d is not None:
            d[SPARE] = 0
        q.nodepools.append(dataclasses.replace(p, daemon_overhead=d))
    q.existing = []
    for e in prob.existing:
        av = np.array(e.available, np.int64)
        av[SPARE] = 0
        rq = None if e.requests is None else np.array(e.requests, np.int64)
        if rq is not None:
            rq[SPARE] = 0
        q.existing.append(dataclasses.replace(e, available=av, requests=rq))
    return q


def strip(prob):
    """The same problem without any host port."""
    q = copy.copy(prob)
    q.classes = [dataclasses.replace(pc, host_ports=[]) for pc in prob.classes]
    q.nodepools = [dataclasses.replace(p, daemon_host_ports=[]) for p in prob.nodepools]
    q.existing = [dataclasses.replace(e, host_ports=[]) for e in prob.existing]
    return q


def transform(dprob, orc_catalog):
    """The oracle's problem for device problem dprob (device_problem's output): host ports as spare resource axes."""
    n, cown, pown, xown = problem_bits(dprob)
    assert n <= len(SPARE), "an oracle-checked problem carries at most %d port bits, not %d" % (len(SPARE), n)
    q = strip(dprob)
    q.catalog = orc_catalog
    q.pods = dataclasses.replace(dprob.pods, requests=np.array(dprob.pods.requests, np.int64))
    for c, own in enumerate(cown):
        for b in own:
            q.pods.requests[dprob.pods.class_id == c, SPARE[b]] = UNIT
    for p, own in zip(q.nodepools, pown):
        d = np.zeros(model.R, np.int64) if p.daemon_overhead is None else np.array(p.daemon_overhead, np.int64)
        for b in own:
            d[SPARE[b]] = UNIT
        p.daemon_overhead = d
    for e, own in zip(q.existing, xown):
        av = np.array(e.available, np.int64)
        av[SPARE] = UNIT
        for b in own:
            av[SPARE[b]] = 0
        e.available = av
    return q


# ------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------
# 7 bits: (TCP, 80) 1, (TCP, 443) wildcard + two IPs 3, (UDP, 53) 1, (TCP, 53) 1, (TCP, 9100) 1
POOL = [HostPort(80), HostPort(443, "TCP", "10.0.0.1"), HostPort(443, "TCP", "10.0.0.2"), HostPort(443, "TCP", "0.0.0.0"),
        HostPort(53, "UDP"), HostPort(53, "TCP", "::"), HostPort(9100)]


def add_ports(rng, prob, p_class=0.4, p_node=0.15, p_pool=0.2):
    """Random host ports from POOL on a problem's classes (one or two entries), NodePools' daemonsets and existing
    nodes' bound pods (one entry)."""
    def pick(k):
        return [copy.copy(POOL[int(i)]) for i in rng.choice(len(POOL), size=k, replace=False)]
    for pc in prob.classes:
        if rng.random() < p_class:
            pc.host_ports = pick(int(rng.integers(1, 3)))
    for p in prob.nodepools:
        if rng.random() < p_pool:
            p.daemon_host_ports = pick(1)
    for e in prob.existing:
        if rng.random() < p_node:
            e.host_ports = pick(1)
    return prob


# ------------------------------------------------------------------------------------------------
# the invariant of every result
# ------------------------------------------------------------------------------------------------
def assert_no_conflict(prob, res):
    """No NodeClaim and no existing node holds two pods whose classes conflict, nor a pod that conflicts with the
    NodeClaim's daemonset ports or the node's bound pods."""
    held = {}
    for p, r in enumerate(np.asarray(res.pod_result)):
        r = int(r)
        if r == -1:
            continue
        ports = prob.classes[int(prob.pods.class_id[p])].host_ports
        if not ports:
            continue
        if r not in held:
            held[r] = list(prob.existing[-2 - r].host_ports) if r <= -2 else \
                list(prob.nodepools[int(res.nodeclaim_nodepool[r])].daemon_host_ports)
        assert not sets_conflict(held[r], ports), (p, r)
        held[r] = held[r] + list(ports)


# ------------------------------------------------------------------------------------------------
# the Solve fuzz families (GPU: device against the transformed oracle; CPU: their non-vacuity)
# ------------------------------------------------------------------------------------------------
FAMILY_SEEDS = {"plain": range(12), "existing": range(100, 106), "topology": range(200, 204),
                "pref_respect": range(300, 304), "pref_ignore": range(400, 404), "reserved": range(500, 504)}
FAMILY_POLICY = {"pref_ignore": 1}   # KP_PREFERENCE_IGNORE; every other family: Respect


def sub_catalogs(golden):
    """{'base': (device, oracle), 'reserved': (device, oracle)}: 160 golden types, and the same with reserved
    offerings on 12 of them, each derived for the device and for the oracle."""
    from kpsim import synth
    rng = np.random.Generator(np.random.PCG64(4242))
    sub = [golden[int(i)] for i in sorted(rng.choice(len(golden), size=160, replace=False))]
    res = synth.config5_catalog(sub, n_default=8, n_block=4)
    return {"base": derive_catalogs(sub), "reserved": derive_catalogs(res)}


def family_problem(cats, family, seed):
    """(device problem, oracle problem, preference policy) of one seed of a family: about 250 pods in 8-12 classes."""
    import fuzzgen
    rng = np.random.Generator(np.random.PCG64(77000 + seed))
    dcat, ocat = cats["reserved" if family == "reserved" else "base"]
    n_classes = int(rng.integers(8, 13))
    prob = fuzzgen.fuzz_problem(dcat, seed, n_pods=250, n_classes=n_classes, n_existing=12 if family == "existing" else 0)
    if family == "topology":
        fuzzgen.add_topology(rng, prob)
    elif family in ("pref_respect", "pref_ignore"):
        fuzzgen.add_preferences(rng, prob)
    elif family == "reserved":
        cts = [["reserved"], ["reserved", "on-demand"], ["reserved", "spot", "on-demand"], ["spot", "on-demand"]]
        for p in prob.nodepools:
            p.requirements = [r for r in p.requirements if r.key != model.CAPACITY_TYPE]
            p.requirements.append(model.Requirement(model.CAPACITY_TYPE, "In", cts[int(rng.integers(len(cts)))]))
    add_ports(rng, prob)
    dprob = device_problem(prob, dcat)
    return dprob, transform(dprob, ocat), FAMILY_POLICY.get(family, 0)


def run_oracle(prob, policy=0):
    import pyoracle
    o = pyoracle.solve(prob, preference_policy=policy)
    return o.results, [model.parse_requirements_blob(o.requirements(i)) for i in range(o.results.n_nodeclaims)]


# ------------------------------------------------------------------------------------------------
# consolidation: generator, device / oracle problems
# ------------------------------------------------------------------------------------------------
CONS_SEEDS = range(8)


def cons_with(cp, cluster):
    """The consolidation problem cp over another rendering of its cluster (same nodes, pods, candidates)."""
    return model.ConsolidationProblem(cluster, cp.candidates, cp.pending, cp.initialized)


def cons_problem(cats, seed):
    """(device problem, oracle problem, port-stripped problem) of one consolidation seed: 24-40 nodes, 150 pods, host
    ports thin enough that probes still decide DELETE / REPLACE (two fifths of the classes carry one entry, few nodes
    and NodePools hold one).  A node's table holds the ports of all pods bound to it, so a candidate's node also holds
    its reschedulable pods' ports (it is an ordinary node for every probe that does not remove it)."""
    import fuzzgen
    rng = np.random.Generator(np.random.PCG64(88000 + seed))
    dcat, ocat = cats["base"]
    cp = fuzzgen.fuzz_consolidation(dcat, 9100 + seed, n_nodes=int(rng.integers(24, 41)), n_pods=150, pending_frac=0.0,
                                    n_candidates=int(rng.integers(16, 25)))
    prob = cp.cluster
    # roomy, untainted nodes: without host ports most probes can move their pods (DELETE / REPLACE), so that what the
    # ports change shows in the decisions
    for e in prob.existing:
        e.taints = []
        if rng.random() < 0.9:
            e.available = np.array(e.available, np.int64)
            e.available[model.RIDX["cpu"]] = int(rng.choice([16, 32, 64])) * 1000
            e.available[model.RIDX["memory"]] = int(rng.choice([64, 128, 256])) * 2 ** 30 * 1000
            e.available[model.RIDX["pods"]] = int(rng.choice([20, 50, 110])) * 1000
    for pc in prob.classes:
        if rng.random() < 0.6:
            pc.requirements = []   # most classes fit most nodes: the multi-node prefixes can decide too
        if rng.random() < 0.4:
            pc.host_ports = [copy.copy(POOL[int(rng.integers(len(POOL)))])]
    for p in prob.nodepools:
        if rng.random() < 0.1:
            p.daemon_host_ports = [copy.copy(POOL[int(rng.integers(len(POOL)))])]
    for e in prob.existing:
        if rng.random() < 0.1:
            e.host_ports = [copy.copy(POOL[int(rng.integers(len(POOL)))])]
    for c in cp.candidates:
        node = prob.existing[c.node]
        for p in c.pods:
            for hp in prob.classes[int(prob.pods.class_id[int(p)])].host_ports:
                if hp not in node.host_ports:
                    node.host_ports = node.host_ports + [copy.copy(hp)]
    dprob = device_problem(prob, dcat)
    return cons_with(cp, dprob), cons_with(cp, transform(dprob, ocat)), cons_with(cp, strip(dprob))
