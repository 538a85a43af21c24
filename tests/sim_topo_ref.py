"""Reference for kp_simulate_* over clusters with topology terms (kp_device_opts.simulate_topology = 1).

sim_ref.reference solves cons_explain_ref.reduced_problem, which drops the probe's candidate nodes and the pods of the
candidates the probe does not remove.  Topology counts both: a pod bound to a candidate's node stays counted (the node
is still in the cluster while the simulation runs), and so do the reschedulable pods of the other candidates, which sit
on their nodes (oracle/orc_solve.cpp orc_consolidate counts them there).  kept_node_problem builds the probe with those
kept:

  * every state node stays in `existing`; the probe's candidate nodes get available = -1 on every axis, so nothing can
    land on them (tests/test_simulate_topo_cpu.py asserts that nothing does);
  * all of cluster.bound stays, and (node, class) of every pod of the candidates outside the probe is appended;
  * node indices are the cluster's own.

reference() is sim_ref.reference over that problem: the same fold (AllNonPendingPodsScheduled with the uninitialized
nodes, the overflow row) and the same index mapping.  tests/test_simulate_topo_cpu.py pins its rows to
pyoracle.consolidate's on every probe of the corpus below.
"""
import dataclasses

import numpy as np

import cons_explain_ref as cxr
import sim_ref
from kpsim import model

SINGLE, MULTI = sim_ref.SINGLE, sim_ref.MULTI


_reduced = cxr.reduced_problem


def kept_node_problem(cp, cands):
    """(Problem, pods, nodes) as cons_explain_ref.reduced_problem returns them, with the candidates' nodes and every
    counted pod kept (see the module docstring)."""
    red, pods, _ = _reduced(cp, cands)
    prob = cp.cluster
    gone = {int(cp.candidates[c].node) for c in cands}
    existing = [dataclasses.replace(nd, available=np.full_like(np.asarray(nd.available, np.int64), -1)) if j in gone else nd
                for j, nd in enumerate(prob.existing)]
    bound = list(prob.bound)
    inside = set(cands)
    for c, cd in enumerate(cp.candidates):
        if c not in inside:
            bound += [(int(cd.node), int(prob.pods.class_id[p])) for p in cd.pods]
    return dataclasses.replace(red, existing=existing, bound=bound), pods, list(range(len(prob.existing)))


def reference(cp, mode, probe):
    """sim_ref.reference(cp, mode, probe) with kept_node_problem as the probe's problem: sim_ref's fold and index
    mapping, unchanged"""
    # sim_ref.py stays as it is, so its problem builder is swapped for the call.  This relies on sim_ref looking
    # reduced_problem up through the module attribute (cxr.reduced_problem) at call time; were it bound by name at import,
    # the swap would do nothing, and tests/test_simulate_topo_cpu.py::test_kept_node_affinity_case, where the two
    # references differ, would fail.  Not re-entrant.
    cxr.reduced_problem = kept_node_problem
    try:
        return sim_ref.reference(cp, mode, probe)
    finally:
        cxr.reduced_problem = _reduced


def on_kept_node(cp, mode, probe, ref):
    """pods of the reference's Results that landed on one of the probe's own candidate nodes (none may)"""
    gone = {int(cp.candidates[c].node) for c in cxr.probe_candidates(cp, mode, probe)}
    res = np.asarray(ref["results"].pod_result)
    return [int(i) for i in np.nonzero(res <= -2)[0] if -2 - int(res[i]) in gone]


def without_topology(cp):
    """the same cluster with every topology term removed (and so no counted bound pod)"""
    classes = [dataclasses.replace(pc, topology=[]) for pc in cp.cluster.classes]
    return dataclasses.replace(cp, cluster=dataclasses.replace(cp.cluster, classes=classes, bound=[]))


# ---- the corpus shared by tests/test_simulate_topo_cpu.py and tests/test_gpu_simulate_topo.py ----
# fuzzgen.fuzz_topology_consolidation with test_gpu_consolidation.py::test_fuzz_consolidation_topology's draw.  Seeds 0, 1,
# 5, 9, 11, 18 and 22 put 4 to 21 of their probes past 12 NodeClaims and are left out.
TOPO_SEEDS = [2, 3, 4, 6, 7, 8, 10, 13, 15, 16, 17, 19, 20, 21, 23]
HOST_AFF_SEEDS = [2, 6, 10, 15, 16, 17]
CORPUS = ["topo%d" % s for s in TOPO_SEEDS] + ["haff%d" % s for s in HOST_AFF_SEEDS]


def topo_case(golden, seed, host_affinity=False):
    import fuzzgen
    rng = np.random.Generator(np.random.PCG64(3100 + seed))
    sub = [golden[int(i)] for i in sorted(rng.choice(len(golden), size=int(rng.integers(60, 300)), replace=False))]
    return fuzzgen.fuzz_topology_consolidation(sub, 3100 + seed, n_nodes=int(rng.integers(4, 60)),
                                               n_pods=int(rng.integers(20, 250)), all_spot=seed % 4 == 0,
                                               host_affinity=host_affinity)


def corpus(golden, policy):
    """[(name, ConsolidationProblem)] under MIN_VALUES_POLICY `policy`"""
    out = [("topo%d" % s, topo_case(golden, s)) for s in TOPO_SEEDS]
    out += [("haff%d" % s, topo_case(golden, s, host_affinity=True)) for s in HOST_AFF_SEEDS]
    for _, cp in out:
        cp.cluster.min_values_policy = policy
    return out


def topo_pod_on_nodeclaim(cp, ref):
    """the reference placed a pod of a class with topology terms on a new NodeClaim"""
    res = np.asarray(ref["results"].pod_result)
    return any(res[li] >= 0 and cp.cluster.classes[int(cp.cluster.pods.class_id[p])].topology
               for li, p in enumerate(ref["pods"]))


# ---- hand clusters ----
def _zones(it, ct="on-demand"):
    return sorted({o.zone for o in it.offerings if o.available and o.capacity_type == ct})


def _node_in(name, it, zone, cpu_avail=None, ct="on-demand"):
    from kpsim import synth
    avail = np.array(it.allocatable, np.int64).copy()
    if cpu_avail is not None:
        avail[model.RIDX["cpu"]] = cpu_avail
    return model.ExistingNode(name, synth.node_labels(it, zone, ct, "default"), avail)


def _sel(app):
    return [model.Requirement("app", "In", [app])]


def _problem(cat, classes, specs, nodes, bound=()):
    from kpsim import synth
    return model.Problem(cat, [synth.default_nodepool()], classes, synth.pods_from_specs(specs), existing=nodes,
                         bound=list(bound))


def zonal_spread_case(cat):
    """One candidate with three pods of a class that spreads over zones with maxSkew 1, no other node: each pod opens a
    NodeClaim in another zone."""
    t0 = sim_ref.small_type(cat)
    z = _zones(cat[t0])
    cls = model.PodClass(labels={"app": "s"}, topology=[model.TopologyTerm("spread", model.ZONE, _sel("s"), max_skew=1)])
    prob = _problem(cat, [cls], [(0, {"cpu": "1"})] * 3, [_node_in("n0", cat[t0], z[0])])
    return model.ConsolidationProblem(prob, [sim_ref._cand(0, [0, 1, 2], t0)])


def hostname_anti_case(cat, n):
    """n pods that refuse each other's hostname: n NodeClaims (13: the overflow)"""
    t0 = sim_ref.small_type(cat)
    cls = model.PodClass(labels={"app": "a"}, topology=[model.TopologyTerm("anti", model.HOSTNAME, _sel("a"))])
    prob = _problem(cat, [cls], [(0, {"cpu": "1"})] * n, [_node_in("n0", cat[t0], _zones(cat[t0])[0])])
    return model.ConsolidationProblem(prob, [sim_ref._cand(0, list(range(n)), t0)])


def truncation_drop_case(cat):
    """hostname_anti_case(cat, 2) under a NodePool that wants 4 distinct instance-cpu values among at most 10 instance
    types: both NodeClaims are created, and TruncateInstanceTypes drops both (the 10 cheapest options hold fewer cpu
    sizes), so their pods count as unscheduled."""
    cp = hostname_anti_case(cat, 2)
    cp.cluster.nodepools[0].requirements.append(model.Requirement("karpenter.k8s.aws/instance-cpu", "Exists", [], 4))
    cp.cluster.max_instance_types = 10
    return cp


def hostname_spread_case(cat):
    """Four pods of a class with a hostname spread of maxSkew 1; node n1 has room, n2 has none.  The first pod takes n1,
    every later one skips n1 and each NodeClaim that holds a pod already: three NodeClaims of one pod."""
    t0 = sim_ref.small_type(cat)
    z = _zones(cat[t0])[0]
    cls = model.PodClass(labels={"app": "h"}, topology=[model.TopologyTerm("spread", model.HOSTNAME, _sel("h"), max_skew=1)])
    nodes = [_node_in("n0", cat[t0], z), _node_in("n1", cat[t0], z), _node_in("n2", cat[t0], z, cpu_avail=0)]
    prob = _problem(cat, [cls], [(0, {"cpu": "500m"})] * 4, nodes)
    return model.ConsolidationProblem(prob, [sim_ref._cand(0, [0, 1, 2, 3], t0)])


def kept_node_affinity_case(cat):
    """The candidate's pod needs the zone of a `db` pod, and the only one is bound to the candidate's own node n0 (zone
    z0).  That pod stays counted while n0 is simulated away: the pod passes over n1 (zone z1, room) and opens a NodeClaim
    in z0.  Without the pods of the kept node no zone holds a `db` pod and the pod has no place."""
    t0 = sim_ref.small_type(cat)
    z = _zones(cat[t0])
    assert len(z) >= 2
    classes = [model.PodClass(labels={"app": "db"}),
               model.PodClass(labels={"app": "web"}, topology=[model.TopologyTerm("affinity", model.ZONE, _sel("db"))])]
    nodes = [_node_in("n0", cat[t0], z[0]), _node_in("n1", cat[t0], z[1])]
    prob = _problem(cat, classes, [(1, {"cpu": "1"})], nodes, bound=[(0, 0)])
    return model.ConsolidationProblem(prob, [sim_ref._cand(0, [0], t0)])


def inverse_anti_case(cat):
    """A pod bound to n1 refuses `web` pods on its hostname; the candidate's `web` pod, which has no term of its own,
    passes over n1 and lands on n2."""
    t0 = sim_ref.small_type(cat)
    z = _zones(cat[t0])[0]
    classes = [model.PodClass(labels={"app": "lone"}, topology=[model.TopologyTerm("anti", model.HOSTNAME, _sel("web"))]),
               model.PodClass(labels={"app": "web"})]
    nodes = [_node_in("n%d" % i, cat[t0], z) for i in range(3)]
    prob = _problem(cat, classes, [(1, {"cpu": "1"})], nodes, bound=[(1, 0)])
    return model.ConsolidationProblem(prob, [sim_ref._cand(0, [0], t0)])


def drift_spread_case(cat, movable=True):
    """Three candidates, one pod each, on nodes without cpu left; every pod selects `s` pods and spreads them over zones
    with maxSkew 1 and minDomains 2.  The pods of candidates 0 and 2 are tied to zone z0, where a pod bound to node n3
    already counts: with one eligible domain of the two required the global minimum is 0, and 1 + 1 - 0 exceeds the skew:
    no place.  Candidate 1's pod is tied to z1, which is empty: one NodeClaim in z1.  movable=False: candidate 1's pod is
    tied to z0 as well."""
    t0 = sim_ref.small_type(cat)
    z = _zones(cat[t0])
    assert len(z) >= 2

    def tied(zone):
        return model.PodClass(requirements=[model.Requirement(model.ZONE, "In", [zone])], labels={"app": "s"},
                              topology=[model.TopologyTerm("spread", model.ZONE, _sel("s"), max_skew=1, min_domains=2)])
    classes = [tied(z[0]), tied(z[1]), model.PodClass(labels={"app": "s"})]
    specs = [(0, {"cpu": "1"}), (1 if movable else 0, {"cpu": "1"}), (0, {"cpu": "1"})]
    nodes = [_node_in("n%d" % i, cat[t0], z[0], cpu_avail=0) for i in range(4)]
    prob = _problem(cat, classes, specs, nodes, bound=[(3, 2)])
    return model.ConsolidationProblem(prob, [sim_ref._cand(i, [i], t0) for i in range(3)])


def drift_case(cat, movable=True):
    """Three candidates on nodes without cpu left.  Candidates 0 and 2 hold a pod that needs the zone of a `db` pod, and
    no such pod exists: no place.  Candidate 1 holds two pods that refuse each other's hostname: two NodeClaims, every
    pod scheduled.  movable=False: candidate 1's pods are of the first kind too."""
    t0 = sim_ref.small_type(cat)
    z = _zones(cat[t0])[0]
    classes = [model.PodClass(labels={"app": "web"}, topology=[model.TopologyTerm("affinity", model.ZONE, _sel("db"))]),
               model.PodClass(labels={"app": "a"}, topology=[model.TopologyTerm("anti", model.HOSTNAME, _sel("a"))])]
    mid = 1 if movable else 0
    specs = [(0, {"cpu": "1"}), (mid, {"cpu": "1"}), (mid, {"cpu": "1"}), (0, {"cpu": "1"})]
    nodes = [_node_in("n%d" % i, cat[t0], z, cpu_avail=0) for i in range(3)]
    prob = _problem(cat, classes, specs, nodes)
    return model.ConsolidationProblem(prob, [sim_ref._cand(0, [0], t0), sim_ref._cand(1, [1, 2], t0),
                                             sim_ref._cand(2, [3], t0)])


def nodeclaim_zones(ref):
    """the zone requirement's values of each NodeClaim of a reference() dict (or of parsed requirements)"""
    reqs = ref["reqs"] if isinstance(ref, dict) else ref
    return [tuple(sorted(r[model.ZONE][4])) if model.ZONE in r and not r[model.ZONE][0] else None for r in reqs]
