"""Solve problems in which a pod shape meets a run of full NodeClaims at the front of the slice (the headroom bound of
the slow path's candidate collection, DESIGN.md §4 "Headroom bound"), shared by the CPU (oracle) and GPU tests.

Construction (NodePool of three 8-vCPU types, as tests/same_shape_cases.py): F pods of 7 cpu open F NodeClaims that no
2-cpu pod fits any more (7 + 2 exceeds every option's allocatable cpu); G pods of 5 cpu open G NodeClaims that take one
2-cpu pod each.  The queue is sorted by size, so the 2-cpu pods come last and find the F full NodeClaims leading the
slice (sort.Slice by len(Pods) is stable here: every NodeClaim holds one pod).  The first of them is rejected by all F
on Fits alone, F candidates in rounds of 8, before it lands on the first 5-cpu NodeClaim, or, with G = 0, on a new one.
"""
from dataclasses import dataclass

import numpy as np

from kpsim import abi, model, synth
from kpsim.model import HostPort, PodClass, Requirement, TopologyTerm

import same_shape_cases as SC

FULL = {"cpu": "7", "memory": "1Gi"}
OPEN = {"cpu": "5", "memory": "1Gi"}
MED = {"cpu": "2", "memory": "1Gi"}
# both sides of a round of 8 candidates and of the 64-position scan window
FS = [7, 8, 9, 16, 17, 63, 64, 65, 130]


@dataclass
class Case:
    name: str
    problem: model.Problem
    n_nodeclaims: int
    min_skips: int  # candidates the bound must reject without an evaluation at the least (0: it must reject none)
    preference_policy: int = abi.KP_PREFERENCE_RESPECT
    skips: int = -1  # >= 0: the exact count the construction implies


def absorbed(cat, f, g=3, m=3):
    """(a) the 2-cpu pods' class has no requirement keys: every NodeClaim has absorbed it, the rejections replace
    fits-only sweeps (witness misses)"""
    specs = [(0, FULL)] * f + [(0, OPEN)] * g + [(1, MED)] * m
    prob = model.Problem(cat, [SC.pool(cat)], [PodClass(), PodClass(labels={"app": "med"})], synth.pods_from_specs(specs))
    return Case("absorbed_F%d" % f, prob, f + g, f)


def not_absorbed(cat, f, g=3, m=3):
    """(b) the 2-cpu pods' class carries a requirement key: no NodeClaim has absorbed it, candidate 0 is the
    block-evaluated first candidate unless the bound rejects it"""
    specs = [(0, FULL)] * f + [(0, OPEN)] * g + [(1, MED)] * m
    med = PodClass(labels={"app": "med"}, requirements=[Requirement(model.INSTANCE_TYPE, "In", SC.TYPES)])
    prob = model.Problem(cat, [SC.pool(cat)], [PodClass(), med], synth.pods_from_specs(specs))
    return Case("not_absorbed_F%d" % f, prob, f + g, f)


def no_fit(cat, f, m=2):
    """(c) no NodeClaim fits: the templates open one after rounds of rejected candidates alone (m <= 3 pods share it)"""
    specs = [(0, FULL)] * f + [(1, MED)] * m
    prob = model.Problem(cat, [SC.pool(cat)], [PodClass(), PodClass(labels={"app": "med"})], synth.pods_from_specs(specs))
    return Case("no_fit_F%d" % f, prob, f + 1, f)


def zero_axis(cat, f, g=2, m=2):
    """(f) the shape requests nothing on a staged axis (no memory): that axis never rejects"""
    specs = [(0, FULL)] * f + [(0, OPEN)] * g + [(1, {"cpu": "2"})] * m
    prob = model.Problem(cat, [SC.pool(cat)], [PodClass(), PodClass(labels={"app": "med"})], synth.pods_from_specs(specs))
    return Case("zero_axis_F%d" % f, prob, f + g, f)


def _alloc_max(cat, res):
    return max(int(cat[r].allocatable[model.RIDX[res]]) for r in SC.rows(cat))


def _set(pods, sel, res, milli):
    pods.requests[sel, model.RIDX[res]] = milli


def at_bound(cat, res, above, f=9, m=3):
    """(e) the F NodeClaims hold a pod that leaves exactly X on axis `res` (cpu: X = 2 cpu; memory: X = 4Gi, an axis
    with qshift > 0 on this catalog) under the largest option; the small pods request exactly X (each fits, one per
    NodeClaim: no NodeClaim may be rejected for it) or one milli-unit more (none fits: all F are rejected and one new
    NodeClaim takes the m pods).  The count is exact: big pod k >= 2 finds the NodeClaims of the pods before it marked
    in the shape's memo but the newest, which the bound rejects (f - 1 in all); the first small pod above the bound adds
    the f full NodeClaims, and the later ones find them marked."""
    x = 2000 if res == "cpu" else (4 << 30) * 1000
    big = {"cpu": "1", "memory": "1Gi"}
    small = {"cpu": "100m", "memory": "64Mi"}
    pods = synth.pods_from_specs([(0, big)] * f + [(1, small)] * m)
    _set(pods, pods.class_id == 0, res, _alloc_max(cat, res) - x)
    _set(pods, pods.class_id == 1, res, x + (1 if above else 0))
    prob = model.Problem(cat, [SC.pool(cat)], [PodClass(), PodClass(labels={"app": "med"})], pods)
    return Case("%s_%s_F%d" % ("above_bound" if above else "at_bound", res, f), prob, f + (1 if above else 0),
                f - 1, skips=2 * f - 1 if above else f - 1)


LOOSE_TYPES = ["c5.4xlarge", "r5.2xlarge"]  # 16 vCPU / 32 GiB and 8 vCPU / 64 GiB


def loose(cat, f=9, m=3):
    """(d) every NodeClaim keeps a cpu-rich and a memory-rich option.  A second pod passes the bound on each axis
    (13 or 14 cpu <= 16 vCPU's allocatable, 40 GiB <= 64 GiB's) but no single type fits both, so each NodeClaim is
    evaluated, rejected and marked, every pod gets its own NodeClaim, and the bound rejects nothing."""
    specs = [(0, {"cpu": "7", "memory": "20Gi"})] * f + [(1, {"cpu": "6", "memory": "20Gi"})] * m
    pool = synth.default_nodepool(instance_types=SC.rows(cat, LOOSE_TYPES))
    prob = model.Problem(cat, [pool], [PodClass(), PodClass(labels={"app": "med"})], synth.pods_from_specs(specs))
    return Case("loose_F%d" % f, prob, f + m, 0)


def min_values(cat, f=9, g=3, m=3):
    """(g) a minValues NodePool: its NodeClaims keep no quick-accept witness, so their rows give no bound"""
    specs = [(0, FULL)] * f + [(0, OPEN)] * g + [(1, MED)] * m
    pool = synth.default_nodepool(instance_types=SC.rows(cat),
                                  requirements=[Requirement(model.INSTANCE_TYPE, "Exists", [], min_values=2)])
    prob = model.Problem(cat, [pool], [PodClass(), PodClass(labels={"app": "med"})], synth.pods_from_specs(specs))
    return Case("min_values_F%d" % f, prob, f + g, 0)


def reserved(cat5, f=9, g=3, m=3):
    """(h) a catalog with reserved offerings and a NodePool open to them: the kernels for such catalogs carry no bound"""
    specs = [(0, FULL)] * f + [(0, OPEN)] * g + [(1, MED)] * m
    prob = model.Problem(cat5, [SC.pool(cat5, ("reserved", "on-demand", "spot"))],
                         [PodClass(), PodClass(labels={"app": "med"})], synth.pods_from_specs(specs))
    return Case("reserved_F%d" % f, prob, f + g, 0)


def _spread():
    # a zone spread that never binds (maxSkew 100): the class carries topology terms, the placement is the plain one
    return [TopologyTerm("spread", model.ZONE, selector=[Requirement("app", "In", ["med"])], max_skew=100)]


def topology(cat, f=9, g=3, m=3):
    """(i) the 2-cpu pods carry a topology term: a topology solve, whose kernels carry no bound"""
    specs = [(0, FULL)] * f + [(0, OPEN)] * g + [(1, MED)] * m
    prob = model.Problem(cat, [SC.pool(cat)], [PodClass(), PodClass(labels={"app": "med"}, topology=_spread())],
                         synth.pods_from_specs(specs))
    return Case("topology_F%d" % f, prob, f + g, 0)


def shared(cat, f=9, g=4, m=2):
    """(j) plain, topology and port-carrying 2-cpu pods in one solve (the PORTS topology kernel: no bound)"""
    specs = [(0, FULL)] * f + [(0, OPEN)] * g + [(1, MED)] * m + [(2, MED)] + [(3, MED)]
    classes = [PodClass(), PodClass(labels={"app": "med"}), PodClass(labels={"app": "med"}, topology=_spread()),
               PodClass(labels={"app": "port"}, host_ports=[HostPort(8080)])]
    return Case("shared_F%d" % f, model.Problem(cat, [SC.pool(cat)], classes, synth.pods_from_specs(specs)), f + g, 0)


def requeued(cat, f=9, g=3, m=3):
    """(k) PREF: the 2-cpu pods carry a preferred term no type satisfies: each fails once on every NodeClaim and the
    templates, is relaxed and requeued, and meets the full NodeClaims again"""
    specs = [(0, FULL)] * f + [(0, OPEN)] * g + [(1, MED)] * m
    med = PodClass(labels={"app": "med"},
                   preferred_terms=[(10, [Requirement(model.INSTANCE_TYPE, "In", ["no-such-type"])])])
    return Case("pref_requeued_F%d" % f, model.Problem(cat, [SC.pool(cat)], [PodClass(), med], synth.pods_from_specs(specs)),
                f + g, f)


def ports(cat, f=9, g=3, m=3):
    """(l) a port-carrying class is present: the PORTS kernel runs, with the bound compiled out"""
    specs = [(0, FULL)] * f + [(0, OPEN)] * g + [(1, MED)] * m + [(2, {"cpu": "100m", "memory": "64Mi"})]
    classes = [PodClass(), PodClass(labels={"app": "med"}), PodClass(labels={"app": "port"}, host_ports=[HostPort(8080)])]
    return Case("ports_F%d" % f, model.Problem(cat, [SC.pool(cat)], classes, synth.pods_from_specs(specs)), f + g, 0)


OTHER = ["loose_F9", "at_bound_cpu_F9", "above_bound_cpu_F9", "at_bound_memory_F9", "above_bound_memory_F9",
         "min_values_F9", "reserved_F9", "topology_F9", "shared_F9", "pref_requeued_F9", "ports_F9"]
NAMES = (["absorbed_F%d" % f for f in FS] + ["not_absorbed_F%d" % f for f in FS] +
         ["no_fit_F%d" % f for f in (7, 8, 9, 65)] + ["zero_axis_F9"] + OTHER)


def build(golden):
    """name -> Case, in a fixed order"""
    cases = [absorbed(golden, f) for f in FS] + [not_absorbed(golden, f) for f in FS]
    cases += [no_fit(golden, f) for f in (7, 8, 9, 65)] + [zero_axis(golden, 9)]
    cases += [loose(golden), at_bound(golden, "cpu", False), at_bound(golden, "cpu", True),
              at_bound(golden, "memory", False), at_bound(golden, "memory", True), min_values(golden),
              reserved(synth.config5_catalog(golden)), topology(golden), shared(golden), requeued(golden), ports(golden)]
    assert [c.name for c in cases] == NAMES
    return {c.name: c for c in cases}


# ---- fuzz seeds chosen on the CPU, from the oracle alone ----
# fuzzgen.fuzz_problem(golden, seed): the first 12 seeds from 7000 on with types_rejections_ahead > 0
PLAIN_SEEDS = [7000, 7001, 7003, 7004, 7006, 7007, 7011, 7012, 7014, 7015, 7017, 7019]


def _type_matches(it, req):
    """a NodePool requirement against an instance type's labels (offering keys are not type labels: no constraint)"""
    if req.key in model.OFFERING_KEYS or req.key not in it.labels:
        return True if req.key in model.OFFERING_KEYS else req.op in ("NotIn", "DoesNotExist")
    vals = it.labels[req.key]
    if vals is None:
        return req.op in ("NotIn", "DoesNotExist")
    if req.op == "In":
        return any(v in req.values for v in vals)
    if req.op == "NotIn":
        return any(v not in req.values for v in vals)
    if req.op == "Exists":
        return True
    if req.op == "DoesNotExist":
        return False
    try:
        nums = [int(v) for v in vals]
    except ValueError:
        return False
    return any(n > int(req.values[0]) for n in nums) if req.op == "Gt" else any(n < int(req.values[0]) for n in nums)


def pool_bounds(prob):
    """per NodePool: the largest allocatable per resource over a superset of the types its NodeClaims can keep (its
    rows, its label requirements, its initial limits), or None for a minValues pool (no bound rows there)"""
    out = []
    for np_ in prob.nodepools:
        if any(r.min_values for r in np_.requirements):
            out.append(None)
            continue
        rows = np_.instance_types if np_.instance_types is not None else range(len(prob.catalog))
        best = np.zeros(model.R, np.int64)
        for t in rows:
            it = prob.catalog[t]
            if not all(_type_matches(it, r) for r in np_.requirements):
                continue
            if np_.limits_remaining and any(int(it.capacity[model.RIDX[k]]) > v for k, v in np_.limits_remaining.items()):
                continue
            best = np.maximum(best, it.allocatable)
        out.append(best)
    return out


def types_rejections_ahead(prob, res):
    """Replays the oracle's placements (pod_result, pod_order) into per-NodeClaim request totals and counts the pairs
    (pod, NodeClaim ahead of the pod's fit in the slice: fewer pods, or any NodeClaim when the pod opens a new one) where
    total + request exceeds, on an axis the pod requests, the largest allocatable the NodeClaim's pool can offer: a
    rejection for lack of a fitting type in front of a fit, by the oracle's result alone."""
    bounds = pool_bounds(prob)
    N = res.n_nodeclaims
    total = np.zeros((N, model.R), np.int64)
    npods = np.zeros(N, np.int64)
    made = np.zeros(N, bool)
    hits = 0
    placed = [p for p in np.argsort(res.pod_order, kind="stable") if res.pod_order[p] >= 0 and res.pod_result[p] >= 0]
    for p in placed:
        n, req = int(res.pod_result[p]), prob.pods.requests[p]
        for m in np.nonzero(made)[0]:
            pool = int(res.nodeclaim_nodepool[m])
            if m == n or pool < 0 or bounds[pool] is None or (made[n] and npods[m] >= npods[n]):
                continue
            if ((req > 0) & (total[m] + req > bounds[pool])).any():
                hits += 1
        if not made[n]:
            made[n] = True
            d = prob.nodepools[int(res.nodeclaim_nodepool[n])].daemon_overhead if res.nodeclaim_nodepool[n] >= 0 else None
            if d is not None:
                total[n] += d
        total[n] += req
        npods[n] += 1
    return hits
