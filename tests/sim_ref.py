"""Reference for kp_simulate_*: a probe's SimulateScheduling is the CPU oracle's Solve of its reduced cluster.

cons_explain_ref.reduced_problem(cp, S) builds the probe over candidates S as a Problem: the state nodes minus the
candidates, the pending pods plus the candidates' pods, the candidates' capacity back in their NodePools' limits.  The
oracle's Solve of it is Solve(...).TruncateInstanceTypes(max_instance_types); here its indices are mapped back to the
cluster's (pods through the reduced problem's pod list, existing nodes through its node list) and the row is folded as
oracle/orc_solve.cpp:1552-1559 folds AllNonPendingPodsScheduled.  tests/test_simulate_cpu.py pins the fold to
pyoracle.consolidate's rows.

Scope: catalogs without reserved offerings (the strict and fallback reservation modes coincide), clusters without
topology terms or preferences.
"""
import numpy as np

import cons_explain_ref as cxr
from kpsim import abi, model

SINGLE, MULTI = abi.KP_CONSOLIDATE_SINGLE, abi.KP_CONSOLIDATE_MULTI
ROW_FIELDS = list(abi.SIM_DTYPE.names)


def n_probes(cp, mode):
    return model.consolidation_probe_count(len(cp.candidates), mode)


def reference(cp, mode, probe):
    """dict(row, pods, results, reqs, n_nodeclaims): the probe's kp_sim_result as a dict, its pods as indices into
    cp.cluster's, its Results with existing nodes as indices into cp.cluster.existing, the parsed requirements of each
    NodeClaim, and the NodeClaims the Solve created (dropped ones included)."""
    import pyoracle
    red, pods, nodes = cxr.reduced_problem(cp, cxr.probe_candidates(cp, mode, probe))
    o = pyoracle.solve(red)
    r = o.results
    n_pend = len(cp.pending)
    res = np.array(r.pod_result, np.int32).copy()
    ex = res <= -2
    res[ex] = -2 - np.array(nodes, np.int64)[-2 - res[ex]].astype(np.int32) if ex.any() else res[ex]
    all_ok, unsched = True, 0
    for li in range(n_pend, len(pods)):
        if res[li] == -1:
            all_ok = False
            unsched += 1
        elif res[li] <= -2 and cp.initialized is not None and not cp.initialized[-2 - res[li]]:
            all_ok = False
    n_nc = r.n_nodeclaims
    valid = int((np.asarray(r.nodeclaim_nodepool[:n_nc]) >= 0).sum())
    if n_nc > abi.KP_SIM_MAX_NODECLAIMS:
        row = dict.fromkeys(ROW_FIELDS, 0)
        row["status"] = abi.KP_SIM_NODECLAIM_OVERFLOW
    else:
        row = dict(status=abi.KP_SIM_OK, all_scheduled=int(all_ok), n_new_nodeclaims=valid, n_dropped=n_nc - valid,
                   n_pods=len(pods), n_unscheduled=unsched)
    mapped = model.Results(r.nodeclaim_nodepool, r.nodeclaim_n_pods, r.nodeclaim_slice_pos, r.nodeclaim_n_options,
                           r.nodeclaim_types, res, r.pod_order, {})
    reqs = [model.parse_requirements_blob(o.requirements(i)) for i in range(n_nc)]
    return dict(row=row, pods=pods, results=mapped, reqs=reqs, n_nodeclaims=n_nc)


def rows(cp, mode, refs=None):
    """The reference rows of every probe of `mode` as abi.SIM_DTYPE (refs: the probes' reference() dicts, if at hand)."""
    n = n_probes(cp, mode)
    out = np.zeros(n, abi.SIM_DTYPE)
    for i in range(n):
        ref = refs[i] if refs is not None else reference(cp, mode, i)
        for f in ROW_FIELDS:
            out[i][f] = ref["row"][f]
    return out


def assert_rows_equal(dev, ref):
    assert len(dev) == len(ref)
    for f in ROW_FIELDS:
        np.testing.assert_array_equal(dev[f], ref[f], err_msg=f)


def drift_replay(cp, ref_rows):
    """[core] disruption/drift.go ComputeCommand over reference single-node rows -> (decision, candidates)."""
    empty = [i for i, c in enumerate(cp.candidates) if len(c.pods) == 0]
    if empty:
        return abi.KP_DRIFT_DELETE_EMPTY, empty
    for i, r in enumerate(ref_rows):
        assert r["status"] == abi.KP_SIM_OK
        if r["all_scheduled"]:
            return abi.KP_DRIFT_REPLACE, [i]
    return abi.KP_DRIFT_NONE, []


def validate(ref, had_replacement, type_ids):
    """ValidateCommand's tail over a reference() dict -> abi.KP_VALIDATE_*."""
    row, r = ref["row"], ref["results"]
    assert row["status"] == abi.KP_SIM_OK
    if not row["all_scheduled"]:
        return abi.KP_VALIDATE_PODS_UNSCHEDULABLE
    if row["n_new_nodeclaims"] == 0:
        return abi.KP_VALIDATE_NO_NODECLAIM if had_replacement else abi.KP_VALIDATE_VALID
    if row["n_new_nodeclaims"] > 1:
        return abi.KP_VALIDATE_MULTIPLE_NODECLAIMS
    if not had_replacement:
        return abi.KP_VALIDATE_NEEDS_NODECLAIM
    nc = next(i for i in range(ref["n_nodeclaims"]) if int(r.nodeclaim_nodepool[i]) >= 0)
    return abi.KP_VALIDATE_VALID if set(type_ids) <= set(r.nodeclaim_types[nc]) else abi.KP_VALIDATE_NOT_SUBSET


# ---- the corpus shared by tests/test_simulate_cpu.py and tests/test_gpu_simulate.py ----
FUZZ_SEEDS = list(range(12))
# cons_explain_ref.min_values_case seeds, picked by running it: in seed 126 TruncateInstanceTypes drops NodeClaims (three
# multi-node probes under Strict), the others keep the share of probes past 12 NodeClaims low (seeds 1, 3, 9, 14, 19 put
# 8 to 15 of their multi-node probes there)
MIN_SEEDS = [0, 2, 4, 5, 6, 126]
DROP_CASE = "min126"


def corpus(golden, policy):
    """[(name, ConsolidationProblem)] of the fuzz tests under MIN_VALUES_POLICY `policy`"""
    out = []
    for s in FUZZ_SEEDS:
        cp, _ = cxr.fuzz_case(golden, s)
        out.append(("fuzz%d" % s, cp))
    for s in MIN_SEEDS:
        cp, _ = cxr.min_values_case(golden, s)
        out.append(("min%d" % s, cp))
    for _, cp in out:
        cp.cluster.min_values_policy = policy
    return out


# ---- hand clusters ----
def _node(name, it, ct="on-demand", pool="default", cpu_avail=None):
    from kpsim import synth
    zone = next(o.zone for o in it.offerings if o.capacity_type == ct)
    avail = np.array(it.allocatable, np.int64).copy()
    if cpu_avail is not None:
        avail[model.RIDX["cpu"]] = cpu_avail
    return model.ExistingNode(name, synth.node_labels(it, zone, ct, pool), avail)


def _cand(i, pods, it, price=1.0, pool=-1, cap=None):
    return model.Candidate(node=i, pods=np.array(pods, np.int32), price=price, capacity_type=abi.KP_CT_ON_DEMAND,
                           instance_type=it, nodepool=pool, capacity=cap)


def _has(it, ct):
    return any(o.available and o.capacity_type == ct for o in it.offerings)


def _arch(it):
    v = it.labels[model.ARCH]
    return v[0] if isinstance(v, (list, tuple)) else v


def small_type(cat):
    cpu = model.RIDX["cpu"]
    return next(t for t, it in enumerate(cat) if it.capacity[cpu] == 4000 and _has(it, "on-demand") and _has(it, "spot"))


def typed_rows(cat, n):
    """n catalog rows with an on-demand offering and room for a 1-cpu pod"""
    cpu = model.RIDX["cpu"]
    rows_ = [t for t, it in enumerate(cat) if _has(it, "on-demand") and it.allocatable[cpu] >= 2000][:n]
    assert len(rows_) == n
    return rows_


def per_type_case(cat, n):
    """One candidate whose n pods each select a different instance type: n NodeClaims (13: the overflow)."""
    from kpsim import synth
    from kpsim.model import INSTANCE_TYPE, PodClass, Requirement
    t0 = small_type(cat)
    rows_ = typed_rows(cat, n)
    classes = [PodClass([Requirement(INSTANCE_TYPE, "In", [cat[t].name])]) for t in rows_]
    prob = model.Problem(cat, [synth.default_nodepool()], classes,
                         synth.pods_from_specs([(i, {"cpu": "1"}) for i in range(n)]), existing=[_node("n0", cat[t0])])
    return model.ConsolidationProblem(prob, [_cand(0, list(range(n)), t0)])


def slice_order_case(cat):
    """Two NodeClaims with different pod counts and a last pod that fits both: sort.Slice by len(Pods) decides.  Zone a
    gets three pods, zone b one (queue order: by cpu descending), then an unconstrained pod arrives: ascending pod count
    puts zone b's NodeClaim first."""
    from kpsim import synth
    from kpsim.model import ZONE, PodClass, Requirement
    t0 = small_type(cat)
    zones = sorted({o.zone for o in cat[t0].offerings})[:2]
    classes = [PodClass([Requirement(ZONE, "In", [zones[0]])]), PodClass([Requirement(ZONE, "In", [zones[1]])]), PodClass()]
    specs = [(0, {"cpu": "1"})] * 3 + [(1, {"cpu": "900m"})] + [(2, {"cpu": "100m"})]
    prob = model.Problem(cat, [synth.default_nodepool()], classes, synth.pods_from_specs(specs),
                         existing=[_node("n0", cat[t0])])
    return model.ConsolidationProblem(prob, [_cand(0, list(range(len(specs))), t0)])


def empty_candidate_case(cat):
    from kpsim import synth
    from kpsim.model import PodClass
    t0 = small_type(cat)
    prob = model.Problem(cat, [synth.default_nodepool()], [PodClass()], synth.pods_from_specs([(0, {"cpu": "1"})]),
                         existing=[_node("n0", cat[t0]), _node("n1", cat[t0])])
    return model.ConsolidationProblem(prob, [_cand(0, [], t0), _cand(1, [0], t0)])


def pending_only_unscheduled_case(cat):
    """A pending pod nothing can take (arm64 against amd64-only pools) beside a candidate whose pod fits node n1."""
    from kpsim import synth
    from kpsim.model import ARCH, PodClass, Requirement
    t0 = small_type(cat)
    arch = _arch(cat[t0])
    other = "arm64" if arch == "amd64" else "amd64"
    pool = synth.default_nodepool(requirements=[Requirement(ARCH, "In", [arch])])
    classes = [PodClass(), PodClass([Requirement(ARCH, "In", [other])])]
    prob = model.Problem(cat, [pool], classes, synth.pods_from_specs([(0, {"cpu": "1"}), (1, {"cpu": "1"})]),
                         existing=[_node("n0", cat[t0]), _node("n1", cat[t0])])
    return model.ConsolidationProblem(prob, [_cand(0, [0], t0)], pending=np.array([1], np.int32))


def uninitialized_case(cat):
    """The candidate's pod fits only node n1, which is not initialized; the pool's limit forbids a NodeClaim."""
    from kpsim import synth
    from kpsim.model import PodClass
    t0 = small_type(cat)
    pool = synth.default_nodepool()
    pool.limits_remaining = {"cpu": 0}
    prob = model.Problem(cat, [pool], [PodClass()], synth.pods_from_specs([(0, {"cpu": "1"})]),
                         existing=[_node("n0", cat[t0]), _node("n1", cat[t0])])
    return model.ConsolidationProblem(prob, [_cand(0, [0], t0)], initialized=np.array([1, 0], np.uint8))


def limit_case(cat, returned):
    """A NodePool with no cpu left: the candidate's pod gets a NodeClaim only if its capacity comes back (returned)."""
    from kpsim import synth
    from kpsim.model import PodClass
    t0 = small_type(cat)
    pool = synth.default_nodepool()
    pool.limits_remaining = {"cpu": 0}
    prob = model.Problem(cat, [pool], [PodClass()], synth.pods_from_specs([(0, {"cpu": "1"})]),
                         existing=[_node("n0", cat[t0])])
    cap = np.array(cat[t0].capacity, np.int64) * 16 if returned else None
    return model.ConsolidationProblem(prob, [_cand(0, [0], t0, pool=0 if returned else -1, cap=cap)])


def drift_case(cat, with_empty=False, movable=True):
    """Four candidates on four nodes: candidate 0's pod needs arm64 where only amd64 pools exist (blocked); candidate 1
    holds three pods that each select a different instance type (3 NodeClaims); candidates 2 and 3 hold one plain pod.
    with_empty: a fifth node and candidate without pods.  movable=False: every pod is of the blocked kind."""
    from kpsim import synth
    from kpsim.model import ARCH, INSTANCE_TYPE, PodClass, Requirement
    t0 = small_type(cat)
    arch = _arch(cat[t0])
    other = "arm64" if arch == "amd64" else "amd64"
    same = [t for t, it in enumerate(cat) if _has(it, "on-demand") and it.allocatable[model.RIDX["cpu"]] >= 2000 and
            _arch(it) == arch][:3]
    assert len(same) == 3
    pool = synth.default_nodepool(requirements=[Requirement(ARCH, "In", [arch])])
    classes = [PodClass([Requirement(ARCH, "In", [other])])] + \
        [PodClass([Requirement(INSTANCE_TYPE, "In", [cat[t].name])]) for t in same] + [PodClass()]
    if movable:
        specs = [(0, {"cpu": "1"})] + [(1 + i, {"cpu": "1"}) for i in range(3)] + [(4, {"cpu": "3500m"})] * 2
        owner = [[0], [1, 2, 3], [4], [5]]
    else:
        specs = [(0, {"cpu": "1"})] * 4
        owner = [[0], [1], [2], [3]]
    nodes = [_node("n%d" % i, cat[t0], cpu_avail=0) for i in range(4)]
    if with_empty:
        nodes.append(_node("n4", cat[t0], cpu_avail=0))
        owner.append([])
    prob = model.Problem(cat, [pool], classes, synth.pods_from_specs(specs), existing=nodes)
    return model.ConsolidationProblem(prob, [_cand(i, p, t0) for i, p in enumerate(owner)])


# counts of the base pods per group, chosen by running tests/test_simulate_cpu.py::test_ladder_cases: each solves to
# exactly len(counts) NodeClaims, the final slice order is not the identity, and the floaters' destinations depend on
# both the stable sort's tie rule and the slice order.  LADDER_TIES: every count equal, so every comparison is a tie.
LADDERS = {"n12": [5, 3, 4, 1, 2, 6, 1, 3, 2, 4, 1, 2], "n9": [2, 2, 1, 3, 1, 1, 2, 3, 1], "n7": [1, 2, 3, 1, 2, 3, 1],
           "n12_ties": [2] * 12}
LADDER_FLOATERS = 14


def ladder_types(cat, n):
    """n distinct catalog rows with an on-demand offering and 16 or more cpu, of one architecture"""
    cpu = model.RIDX["cpu"]
    arch = _arch(cat[small_type(cat)])
    rows_ = [t for t, it in enumerate(cat) if _has(it, "on-demand") and it.allocatable[cpu] >= 16000 and _arch(it) == arch][:n]
    assert len(rows_) == n
    return rows_


def ladder_case(cat, counts, n_floaters=LADDER_FLOATERS, seed=0):
    """len(counts) NodeClaims whose sort.Slice order decides where pods go (slice_order_case at 7 to 12 elements).
    Group g's counts[g] base pods select instance type t_g alone (cpu 0.6 to 1.0, all different, so the queue interleaves
    the groups); then n_floaters pods with smaller requests, each selecting 2 to 4 of the types, are popped after every
    base pod and join the first compatible NodeClaim of the slice, which is re-sorted by pod count after every placement.
    One existing node without cpu left, one candidate owning every pod.
    -> (ConsolidationProblem, types per group, [(pod, groups it lists)] of the floaters)"""
    from kpsim import synth
    from kpsim.model import INSTANCE_TYPE, PodClass, Requirement
    n = len(counts)
    rng = np.random.Generator(np.random.PCG64(8100 + seed))
    t0 = small_type(cat)
    types = ladder_types(cat, n)
    classes = [PodClass([Requirement(INSTANCE_TYPE, "In", [cat[t].name])]) for t in types]
    base = [(g, j) for g in range(n) for j in range(counts[g])]
    cpus = rng.permutation(np.arange(600, 1001))[:len(base)]  # distinct millicpu values
    specs = [(g, {"cpu": "%dm" % int(c)}) for (g, _), c in zip(base, cpus)]
    floaters = []
    for f in range(n_floaters):
        groups = sorted(int(g) for g in rng.choice(n, size=int(rng.integers(2, 5)), replace=False))
        classes.append(PodClass([Requirement(INSTANCE_TYPE, "In", [cat[types[g]].name for g in groups])]))
        floaters.append((len(specs), groups))
        specs.append((len(classes) - 1, {"cpu": "%dm" % (500 - 20 * f)}))
    prob = model.Problem(cat, [synth.default_nodepool()], classes, synth.pods_from_specs(specs),
                         existing=[_node("n0", cat[t0], cpu_avail=0)])
    return model.ConsolidationProblem(prob, [_cand(0, list(range(len(specs))), t0)]), types, floaters


# queue ranks of bitmap_block_case's pods: both sides of every 64-bit word edge around the 4096-pod wave step
BITMAP_CAND_RANKS = [0, 63, 64, 4095, 4096, 4097, 4159, 4160, -1]
BITMAP_PEND_RANKS = [62, 4093, 4099]
# fuzzgen seeds picked by running tests/test_simulate_cpu.py::test_bitmap_block_case: in both, probes create up to 6
# NodeClaims and place pods on existing nodes; in the second some pods stay unscheduled (the queue cycles)
BITMAP_SEEDS = [7608, 7632]


def bitmap_block_case(cat, seed=BITMAP_SEEDS[0]):
    """A pass over more than 4096 pods (the queue bitmap has more than 64 words, the kernel's scan takes a second wave
    step) in which only the pods at chosen queue ranks take part: the candidates' pods at ranks BITMAP_CAND_RANKS (-1: the
    last) plus a few around them, dealt round-robin to 4 candidates; pending pods at BITMAP_PEND_RANKS; every other pod
    belongs to nobody.  The nodes keep little cpu, so pods open NodeClaims as well as land on nodes.
    -> (ConsolidationProblem, rank of each pod)"""
    import fuzzgen
    cp = fuzzgen.fuzz_consolidation(cat, seed, n_nodes=24, n_pods=4300, n_candidates=4)
    prob = cp.cluster
    P = prob.pods.n
    order = sorted(range(P), key=lambda p: cxr.queue_key(prob, p))
    rank = np.empty(P, np.int64)
    rank[order] = np.arange(P)
    want = [r % P for r in BITMAP_CAND_RANKS] + [1, 65, 2047, 4094, 4098, 4161, P - 2]
    owned = [[] for _ in cp.candidates]
    for i, r in enumerate(want):
        owned[i % len(owned)].append(order[r])
    for c, pods in zip(cp.candidates, owned):
        c.pods = np.array(sorted(pods), np.int32)
    cp.pending = np.array(sorted(order[r] for r in BITMAP_PEND_RANKS), np.int32)
    cpu = model.RIDX["cpu"]
    for j, node in enumerate(prob.existing):  # every third node keeps one small pod's worth of cpu, the others none
        node.available = node.available.copy()
        node.available[cpu] = min(int(node.available[cpu]), 300 if j % 3 == 0 else 0)
    return cp, rank
