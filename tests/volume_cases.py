"""Volume attach limits: a Python restatement of ExceedsLimits and of the private / shared encoding, seeded generators,
and the reference for a problem with volumes — the CPU oracle (which knows nothing of volumes) run on a transformed
problem in which every limited driver is a spare resource axis:

  every instance type has allocatable = capacity = HUGE on the axis, so NodeClaim.Add never sees it (it has no volume
  check either); a pod requests 1000 x (its claims of the driver); an existing node has 1000 x (limit - mounted)
  available, or HUGE where it has no limit; no NodePool limit or daemon overhead sits on the axis.

That is exact while every claim is private (at most one holder can meet it).  Two families keep it exact with shared
claims: A, the pods sharing a claim are pinned to disjoint node sets (zones), so they never meet and the claims count as
private; B, the shared claim is already mounted on every existing node, so it costs its pods nothing anywhere and is
dropped from them (the nodes' counts keep it).  Oracle-checked problems hold no node over a limit.
"""
import copy
import dataclasses

import numpy as np

import hostport_cases as HP
from kpsim import model

SPARE = HP.SPARE            # axis of limited driver k: SPARE[k]
UNIT = 1000
HUGE = 2 ** 50
EBS, PD, EFS = "ebs.csi.aws.com", "pd.csi.storage.gke.io", "efs.csi.aws.com"
DRIVERS = [EBS, PD, "disk.csi.azure.com", "csi.vsphere.vmware.com"]


# ------------------------------------------------------------------------------------------------
# the rule ([core] scheduling/volumeusage.go, recalled)
# ------------------------------------------------------------------------------------------------
def by_driver(volumes):
    out = {}
    for d, c in volumes:
        out.setdefault(d, set()).add(c)
    return out


def exceeds_limits(node_volumes, node_limits, pod_volumes):
    """ExistingNode.Add's volume check: for some driver of node ∪ pod with a limit on the node, the union of the claim
    sets is larger than the limit.  The loop runs over the union's drivers, so a node already over a limit refuses every
    pod; a driver without a limit on the node is unlimited there."""
    nv, pv = by_driver(node_volumes), by_driver(pod_volumes)
    for d in set(nv) | set(pv):
        if d in node_limits and len(nv.get(d, set()) | pv.get(d, set())) > node_limits[d]:
            return True
    return False


# ------------------------------------------------------------------------------------------------
# the encoding (kp_host.cpp solve_volumes)
# ------------------------------------------------------------------------------------------------
class Encoding:
    """limited: the drivers with a limit on some node, in order of first appearance in the driver table (the others are
    dropped).  A claim on a limited driver is shared when two or more pods reference it, or a pod and a node other than
    that pod's own candidate node (own_node, consolidation); shared claims take one bit each, in claim order.  Per pod:
    vcnt[k] private claims and a shared mask; per node: ex_vcnt[k] and a shared mask."""

    def __init__(self, pod_volumes, node_volumes, node_limits, own_node=None):
        own_node = own_node or {}
        order = []
        for rows in (pod_volumes, node_volumes):
            for r in rows:
                for d, _ in r:
                    if d not in order:
                        order.append(d)
        for lim in node_limits:
            for d in sorted(lim):
                if d not in order:
                    order.append(d)
        self.limited = [d for d in order if any(d in lim for lim in node_limits)]
        kidx = {d: k for k, d in enumerate(self.limited)}
        pods_of, nodes_of, first = {}, {}, []
        for p, r in enumerate(pod_volumes):
            for d, c in r:
                if d in kidx:
                    pods_of.setdefault(c, []).append(p)
                    if c not in first:
                        first.append(c)
        for j, r in enumerate(node_volumes):
            for d, c in r:
                if d in kidx:
                    nodes_of.setdefault(c, []).append(j)
                    if c not in first:
                        first.append(c)
        shared = []
        for c in first:
            ps = pods_of.get(c, [])
            if len(ps) >= 2 or (len(ps) == 1 and any(j != own_node.get(ps[0], -1) for j in nodes_of.get(c, []))):
                shared.append(c)
        self.bit = {c: i for i, c in enumerate(shared)}
        self.n_bits = len(shared)
        VD = len(self.limited)
        self.drv_mask = [0] * VD

        def enc(rows):
            out = []
            for r in rows:
                cnt, mask = [0] * VD, 0
                for d, c in r:
                    if d not in kidx:
                        continue
                    if c in self.bit:
                        mask |= 1 << self.bit[c]
                        self.drv_mask[kidx[d]] |= 1 << self.bit[c]
                    else:
                        cnt[kidx[d]] += 1
                out.append((cnt, mask))
            return out
        self.pods, self.nodes = enc(pod_volumes), enc(node_volumes)
        self.lim = [[lim.get(d) for d in self.limited] for lim in node_limits]

    def used(self, k, j, pod=None, extra_cnt=0, extra_mask=0):
        """Claims of driver k on node j (plus extra state placed there) with pod `pod` added."""
        cnt, mask = self.nodes[j]
        n, m = cnt[k] + extra_cnt, mask | extra_mask
        if pod is not None:
            n += self.pods[pod][0][k]
            m |= self.pods[pod][1]
        return n + bin(m & self.drv_mask[k]).count("1")

    def exceeds(self, j, pod=None):
        return any(self.lim[j][k] is not None and self.used(k, j, pod) > self.lim[j][k] for k in range(len(self.limited)))


def pod_volumes(prob):
    return prob.pods.volumes if prob.pods.volumes is not None else [[] for _ in range(prob.pods.n)]


def problem_encoding(prob, own_node=None):
    return Encoding(pod_volumes(prob), [e.volumes for e in prob.existing], [e.volume_limits for e in prob.existing], own_node)


# ------------------------------------------------------------------------------------------------
# catalogs and the transformed problem
# ------------------------------------------------------------------------------------------------
def derive_catalogs(catalog):
    """(device catalog, oracle catalog): the spare axes at 0, resp. at HUGE, in capacity and allocatable of every type."""
    dev, orc = [], []
    for it in catalog:
        for out, v in ((dev, 0), (orc, HUGE)):
            cap, al = np.array(it.capacity, np.int64), np.array(it.allocatable, np.int64)
            cap[SPARE] = v
            al[SPARE] = v
            out.append(dataclasses.replace(it, capacity=cap, allocatable=al))
    return dev, orc


def device_problem(prob, dev_catalog):
    return HP.device_problem(prob, dev_catalog)


def strip(prob):
    """The same problem without any volume."""
    q = copy.copy(prob)
    q.pods = dataclasses.replace(prob.pods, volumes=None)
    q.existing = [dataclasses.replace(e, volumes=[], volume_limits={}) for e in prob.existing]
    return q


def transform(dprob, orc_catalog, drop=()):
    """The oracle's problem for device problem dprob: limited drivers as spare resource axes.  drop: the family-B claims
    (mounted on every node), removed from the pods; every other claim counts for its pod as a private one."""
    limited = []
    for e in dprob.existing:
        for d in sorted(e.volume_limits):
            if d not in limited:
                limited.append(d)
    assert len(limited) <= len(SPARE)
    drop = set(drop)
    q = strip(dprob)
    q.catalog = orc_catalog
    q.pods = dataclasses.replace(q.pods, requests=np.array(dprob.pods.requests, np.int64))
    for p, r in enumerate(pod_volumes(dprob)):
        for d, cs in by_driver(r).items():
            if d in limited:
                q.pods.requests[p, SPARE[limited.index(d)]] = UNIT * len(cs - drop)
    for e, src in zip(q.existing, dprob.existing):
        av = np.array(e.available, np.int64)
        av[SPARE] = HUGE
        mounted = by_driver(src.volumes)
        for d, lim in src.volume_limits.items():
            left = lim - len(mounted.get(d, ()))
            assert left >= 0, "an oracle-checked problem holds no node over its limit"
            av[SPARE[limited.index(d)]] = UNIT * left
        e.available = av
    return q


# ------------------------------------------------------------------------------------------------
# the invariant of every result
# ------------------------------------------------------------------------------------------------
def assert_within_limits(prob, res):
    """Replaying the placements on existing nodes in pod_order: no Add exceeded a limit."""
    vols = pod_volumes(prob)
    held = [list(e.volumes) for e in prob.existing]
    pr, po = np.asarray(res.pod_result), np.asarray(res.pod_order)
    for p in sorted(np.nonzero(pr <= -2)[0].tolist(), key=lambda p: po[p]):
        j = -2 - int(pr[p])
        assert not exceeds_limits(held[j], prob.existing[j].volume_limits, vols[p]), (p, j)
        held[j] = held[j] + list(vols[p])


# ------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------
def roomy(rng, prob):
    """Untainted nodes with room: without volumes many pods land on them, so that what the limits change shows."""
    for e in prob.existing:
        e.taints = []
        e.available = np.array(e.available, np.int64)
        e.available[model.RIDX["cpu"]] = int(rng.choice([16, 32, 64])) * 1000
        e.available[model.RIDX["memory"]] = int(rng.choice([64, 128, 256])) * 2 ** 30 * 1000
        e.available[model.RIDX["pods"]] = int(rng.choice([20, 50, 110])) * 1000


def add_volumes(rng, prob, n_drivers, p_pod=0.6, a_pairs=0, a_claims=1, b_claims=0):
    """Private claims on a problem's pods and nodes, limits on the nodes (never below what is mounted), one driver
    without any limit; a_pairs pairs of pods pinned to two different zones share a_claims claims each (family A);
    b_claims claims mounted on every node are held by a few pods each (family B).  Returns the family-B claims."""
    drivers = DRIVERS[:n_drivers]
    P = prob.pods.n
    vols = [[] for _ in range(P)]
    for p in range(P):
        if rng.random() < p_pod:
            for i in range(int(rng.integers(1, 3))):
                vols[p].append((str(rng.choice(drivers + [EFS])), "default/data-%d-%d" % (p, i)))
    for j, e in enumerate(prob.existing):
        e.volumes = [(str(rng.choice(drivers + [EFS])), "bound/%d-%d" % (j, i)) for i in range(int(rng.integers(0, 4)))]
    if a_pairs:
        zones = sorted({e.labels[model.ZONE] for e in prob.existing})
        assert len(zones) >= 2
        za, zb = zones[0], zones[1]
        C = len(prob.classes)
        prob.classes = prob.classes + [model.PodClass([model.Requirement(model.ZONE, "In", [z])]) for z in (za, zb)]
        prob.pods = dataclasses.replace(prob.pods, class_id=np.array(prob.pods.class_id, np.int32))
        pick = rng.choice(P, size=2 * a_pairs, replace=False)
        for i in range(a_pairs):
            pa, pb = int(pick[2 * i]), int(pick[2 * i + 1])
            prob.pods.class_id[pa], prob.pods.class_id[pb] = C, C + 1
            for q in range(a_claims):
                v = (drivers[(i + q) % len(drivers)], "shared/a-%d-%d" % (i, q))
                vols[pa].append(v)
                vols[pb].append(v)
    drop = []
    for i in range(b_claims):
        v = (drivers[i % len(drivers)], "shared/b-%d" % i)
        drop.append(v[1])
        for e in prob.existing:
            e.volumes = e.volumes + [v]
        for p in rng.choice(P, size=min(P, 4), replace=False):
            vols[int(p)].append(v)
    for e in prob.existing:
        mounted = by_driver(e.volumes)
        e.volume_limits = {}
        for d in drivers:
            if rng.random() < 0.75:
                e.volume_limits[d] = len(mounted.get(d, ())) + int(rng.integers(0, 2 + 2 * a_claims))
    prob.pods.volumes = vols
    return drop


# ------------------------------------------------------------------------------------------------
# the Solve fuzz families (GPU: device against the transformed oracle; CPU: their non-vacuity)
# ------------------------------------------------------------------------------------------------
FAMILY_SEEDS = {"plain": range(6), "topology": range(200, 206), "pref_respect": range(300, 303),
                "pref_ignore": range(400, 403), "reserved": range(500, 506), "family_a": range(600, 606),
                "family_b": range(700, 706), "edge_64": [800, 801], "edge_65": [810, 811], "edge_256": [820, 821]}
FAMILY_POLICY = {"pref_ignore": 1}   # KP_PREFERENCE_IGNORE; every other family: Respect
EDGE = {"edge_64": (32, 2), "edge_65": (13, 5), "edge_256": (32, 8)}   # pairs x claims = shared bits


def sub_catalogs(golden):
    """{'base': (device, oracle), 'reserved': (device, oracle)}: 160 golden types, and the same with reserved
    offerings on 12 of them, each derived for the device and for the oracle."""
    from kpsim import synth
    rng = np.random.Generator(np.random.PCG64(4242))
    sub = [golden[int(i)] for i in sorted(rng.choice(len(golden), size=160, replace=False))]
    res = synth.config5_catalog(sub, n_default=8, n_block=4)
    return {"base": derive_catalogs(sub), "reserved": derive_catalogs(res)}


def family_problem(cats, family, seed):
    """(device problem, oracle problem, volume-stripped problem, preference policy) of one seed of a family: 60-300 pods,
    4-40 nodes, 1-4 limited drivers."""
    import fuzzgen
    rng = np.random.Generator(np.random.PCG64(99000 + seed))
    dcat, ocat = cats["reserved" if family == "reserved" else "base"]
    n_pods, n_nodes = int(rng.integers(60, 301)), int(rng.integers(4, 41))
    n_classes = int(rng.integers(6, 13))
    if family in EDGE:
        n_pods, n_nodes = max(n_pods, 100), max(n_nodes, 12)   # 2 x 32 pinned pods, and nodes in two zones
    if family == "topology":
        prob = fuzzgen.fuzz_topology_existing_problem(dcat, seed, n_pods=n_pods, n_classes=n_classes, n_existing=n_nodes,
                                                      n_bound=2 * n_nodes)
    else:
        prob = fuzzgen.fuzz_problem(dcat, seed, n_pods=n_pods, n_classes=n_classes, n_existing=n_nodes)
    if family in ("pref_respect", "pref_ignore"):
        fuzzgen.add_preferences(rng, prob)
    elif family == "reserved":
        cts = [["reserved"], ["reserved", "on-demand"], ["reserved", "spot", "on-demand"], ["spot", "on-demand"]]
        for p in prob.nodepools:
            p.requirements = [r for r in p.requirements if r.key != model.CAPACITY_TYPE]
            p.requirements.append(model.Requirement(model.CAPACITY_TYPE, "In", cts[int(rng.integers(len(cts)))]))
    roomy(rng, prob)
    kw = {}
    if family == "family_a":
        kw = dict(a_pairs=int(rng.integers(3, 9)), a_claims=int(rng.integers(1, 3)))
    elif family == "family_b":
        kw = dict(b_claims=int(rng.integers(1, 5)))
    elif family in EDGE:
        kw = dict(a_pairs=EDGE[family][0], a_claims=EDGE[family][1])
    drop = add_volumes(rng, prob, int(rng.integers(1, 5)), **kw)
    dprob = device_problem(prob, dcat)
    return dprob, transform(dprob, ocat, drop), strip(dprob), FAMILY_POLICY.get(family, 0)


def run_oracle(prob, policy=0):
    return HP.run_oracle(prob, policy)


# ------------------------------------------------------------------------------------------------
# consolidation: generator, device / oracle problems
# ------------------------------------------------------------------------------------------------
# seeds in which the volumes change some probe of each mode (test_volumes_cpu asserts it per seed and mode); the odd ones
# carry family-B shared claims
CONS_SEEDS = [0, 2, 5, 12, 13, 21, 25, 38]
CONS_MULTI_DEVICE_SEED = 13


def cons_with(cp, cluster):
    """The consolidation problem cp over another rendering of its cluster (same nodes, pods, candidates)."""
    return model.ConsolidationProblem(cluster, cp.candidates, cp.pending, cp.initialized)


def own_nodes(cp):
    """pod -> its candidate's node, for the reschedulable pods."""
    return {int(p): int(c.node) for c in cp.candidates for p in c.pods}


def cons_problem(cats, seed):
    """(device problem, oracle problem, volume-stripped problem) of one consolidation seed: 6-10 roomy nodes, 40 pods,
    private claims on most pods and nodes (odd seeds: family-B shared claims too), limits close to what is mounted.  A node's table holds the claims of all pods
    bound to it, so a candidate's node also holds its reschedulable pods' claims."""
    import fuzzgen
    rng = np.random.Generator(np.random.PCG64(98000 + seed))
    dcat, ocat = cats["base"]
    n_nodes = int(rng.integers(6, 11))
    cp = fuzzgen.fuzz_consolidation(dcat, 9300 + seed, n_nodes=n_nodes, n_pods=24, pending_frac=0.0,
                                    n_candidates=int(rng.integers(4, n_nodes + 1)))
    cp.initialized = np.ones(n_nodes, np.uint8)
    prob = cp.cluster
    roomy(rng, prob)
    for pc in prob.classes:
        if rng.random() < 0.85:
            pc.requirements = []   # most classes fit most nodes: the multi-node prefixes can decide too
    drivers = DRIVERS[:int(rng.integers(1, 3))]
    vols = [[] for _ in range(prob.pods.n)]
    for p in range(prob.pods.n):
        if rng.random() < 0.9:
            vols[p] = [(str(rng.choice(drivers + [EFS] if i else drivers)), "default/data-%d-%d" % (p, i))
                       for i in range(int(rng.integers(1, 3)))]
    # family B (odd seeds): claims every node mounts, held by a few reschedulable pods: they cost those pods nothing on
    # any node, and drive the shared-mask half of the probes' overlay
    drop = []
    for i in range(int(rng.integers(1, 3)) if seed % 2 else 0):
        v = (drivers[i % len(drivers)], "shared/b-%d" % i)
        drop.append(v[1])
        for p in rng.choice(prob.pods.n, size=4, replace=False):
            vols[int(p)].append(v)
    prob.pods.volumes = vols
    for j, e in enumerate(prob.existing):
        e.volumes = [(str(rng.choice(drivers)), "bound/%d-%d" % (j, i)) for i in range(int(rng.integers(0, 3)))]
        e.volumes += [(drivers[i % len(drivers)], c) for i, c in enumerate(drop)]
    for p, j in own_nodes(cp).items():
        prob.existing[j].volumes = prob.existing[j].volumes + [v for v in vols[p] if v not in prob.existing[j].volumes]
    # tight limits: room for zero to two more claims, so that the limits decide where the resources would not
    for e in prob.existing:
        mounted = by_driver(e.volumes)
        e.volume_limits = {d: len(mounted.get(d, ())) + int(rng.integers(0, 3)) for d in drivers}
    dprob = device_problem(prob, dcat)
    return cons_with(cp, dprob), cons_with(cp, transform(dprob, ocat, drop)), cons_with(cp, strip(dprob))
