"""GPU: kp_consolidate_explain — why each consolidation probe found no command.

Hand clusters with plain expectations (one per reason and flag), the fuzz seeds of tests/test_cons_explain_cpu.py
compared field by field with tests/cons_explain_ref.py (which that file pins to the oracle), the reason against the
same pass's kp_probe_result row over the reserved, topology and preference generators, the pod rows behind
PODS_UNSCHEDULABLE probes against tests/explain_ref.py with the probe's own remaining limits, and the call's contract
(states, buffers, ranges, nothing the pass keeps is touched).
"""
import numpy as np
import pytest

import cons_explain_ref as cxr
import explain_ref
import fuzzgen
from kpsim import abi, consolidation, model, native, synth
from kpsim.model import ARCH, CAPACITY_TYPE, INSTANCE_TYPE, ZONE, NodePool, PodClass, Requirement, Taint

pytestmark = pytest.mark.gpu

SINGLE, MULTI, BOTH = abi.KP_CONSOLIDATE_SINGLE, abi.KP_CONSOLIDATE_MULTI, abi.KP_CONSOLIDATE_BOTH
FAMILY = "karpenter.k8s.aws/instance-family"
CPU = model.RIDX["cpu"]
FIELDS = [f for f in abi.PROBE_EXPLANATION_DTYPE.names if f != "pad"]
PRICE_REASONS = (abi.KP_UNCONS_SPOT_TO_SPOT_DISABLED, abi.KP_UNCONS_MIN_VALUES, abi.KP_UNCONS_NOT_CHEAPER,
                 abi.KP_UNCONS_SPOT_TO_SPOT_TOO_FEW)
OD = {CAPACITY_TYPE: (False, "-", "-", "-", ("on-demand",))}
SPOT = {CAPACITY_TYPE: (False, "-", "-", "-", ("spot",))}


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cat(golden):
    return golden[:200]


def prepare(ctx, cp, s2s=False):
    ctx.upload_catalog(model.CatalogView(cp.cluster.catalog))
    ctx.consolidate_prepare(model.ConsolidateInputView(cp, SINGLE, spot_to_spot=s2s))


def n_probes(cp, mode):
    return model.consolidation_probe_count(len(cp.candidates), mode)


def explain(ctx, cp, mode=SINGLE, s2s=False):
    prepare(ctx, cp, s2s)
    return ctx.consolidate_explain(mode, n_probes(cp, mode))


def node(name, it, ct="on-demand", pool="default", zone=None, cpu_avail=None):
    zone = zone or next(o.zone for o in it.offerings if o.capacity_type == ct)
    avail = np.array(it.allocatable, np.int64).copy()
    if cpu_avail is not None:
        avail[CPU] = cpu_avail
    return model.ExistingNode(name, synth.node_labels(it, zone, ct, pool), avail)


def cand(i, pods, price, it, ct=abi.KP_CT_ON_DEMAND, pool=-1, cap=None):
    return model.Candidate(node=i, pods=np.array(pods, np.int32), price=price, capacity_type=ct, instance_type=it,
                           nodepool=pool, capacity=cap)


def has(it, ct):
    return any(o.available and o.capacity_type == ct for o in it.offerings)


def small_type(cat):
    """row of a 4-cpu type with on-demand and spot offerings"""
    return next(t for t, it in enumerate(cat) if it.capacity[CPU] == 4000 and has(it, "on-demand") and has(it, "spot"))


def one_pod_cluster(cat, pools, classes=None, ct="on-demand", price=1.0, specs=None, **kw):
    """node n0 (the candidate) holds the pods; nothing else has room, so they need a new NodeClaim"""
    t = small_type(cat)
    specs = specs or [(0, {"cpu": "1"})]
    prob = model.Problem(cat, pools, classes or [PodClass()], synth.pods_from_specs(specs),
                         existing=[node("n0", cat[t], ct)], **kw)
    kp_ct = abi.KP_CT_SPOT if ct == "spot" else abi.KP_CT_ON_DEMAND
    return model.ConsolidationProblem(prob, [cand(0, list(range(len(specs))), price, t, kp_ct)])


def fields(r):
    return (int(r["reason"]), int(r["flags"]), int(r["n_unscheduled"]), int(r["first_unscheduled"]))


# ------------------------------------------------------------------------------------------------
# hand clusters, one per reason and flag
# ------------------------------------------------------------------------------------------------
def test_not_cheaper(ctx, cat):
    cp = one_pod_cluster(cat, [synth.default_nodepool()], price=1e-4)
    r = explain(ctx, cp)[0]
    assert fields(r) == (abi.KP_UNCONS_NOT_CHEAPER, 0, 0, -1)
    assert r["n_options"] == 60 and r["n_cheaper"] == 0 and r["min_needed"] == 0
    assert r["candidate_price"] == 1e-4
    # the cheapest on-demand worst launch price of the whole catalog bounds it from below
    assert r["cheapest_price"] >= min(cxr.worst_launch_price(it, OD) for it in cat) > 1e-4


def test_spot_to_spot_disabled_and_enabled(ctx, cat):
    cp = one_pod_cluster(cat, [synth.default_nodepool(capacity_types=("spot", "on-demand"))], ct="spot", price=1e6)
    r = explain(ctx, cp, s2s=False)[0]
    assert fields(r) == (abi.KP_UNCONS_SPOT_TO_SPOT_DISABLED, abi.KP_UNCONS_F_SPOT_TO_SPOT, 0, -1)
    assert r["n_options"] == 60 and r["n_cheaper"] == 60
    r = explain(ctx, cp, s2s=True)[0]
    assert fields(r) == (abi.KP_UNCONS_NONE, abi.KP_UNCONS_F_SPOT_TO_SPOT, 0, -1)
    assert r["n_options"] == 60 and r["n_cheaper"] == 60
    assert ctx.consolidate_execute(SINGLE, 1)[0]["n_replacement_types"] == 15


@pytest.mark.parametrize("n_types,reason", [(10, abi.KP_UNCONS_SPOT_TO_SPOT_TOO_FEW), (15, abi.KP_UNCONS_NONE)])
def test_spot_to_spot_too_few(ctx, cat, n_types, reason):
    rows = [t for t, it in enumerate(cat) if has(it, "spot") and it.capacity[CPU] >= 2000][:n_types]
    pool = synth.default_nodepool(capacity_types=("spot",), instance_types=rows)
    cp = one_pod_cluster(cat, [pool], ct="spot", price=1e6)
    r = explain(ctx, cp, s2s=True)[0]
    assert fields(r) == (reason, abi.KP_UNCONS_F_SPOT_TO_SPOT, 0, -1)
    assert r["n_options"] == n_types and r["n_cheaper"] == n_types
    assert r["cheapest_price"] == min(cxr.worst_launch_price(cat[t], SPOT) for t in rows)


def _family(it):
    return it.labels[FAMILY][0]


def _od_rows(cat):
    """(worst on-demand launch price, row) of the types that take a 1-cpu pod, cheapest first"""
    return sorted((cxr.worst_launch_price(it, OD), t) for t, it in enumerate(cat)
                  if has(it, "on-demand") and it.capacity[CPU] >= 2000 and it.labels.get(FAMILY))


def test_min_values_after_the_price_filter(ctx, cat):
    """minValues 3 on instance-family; the candidate's price leaves three cheaper types of two families."""
    od = _od_rows(cat)
    fam = []
    for _w, t in od:
        if _family(cat[t]) not in fam:
            fam.append(_family(cat[t]))
    a, b, c = fam[0], fam[1], fam[-1]
    cheap = [(w, t) for w, t in od if _family(cat[t]) == a][:2] + [(w, t) for w, t in od if _family(cat[t]) == b][:1]
    dear = [(w, t) for w, t in od if _family(cat[t]) == c][-2:]
    assert max(w for w, _ in cheap) < min(w for w, _ in dear)
    price = (max(w for w, _ in cheap) + min(w for w, _ in dear)) / 2
    pool = synth.default_nodepool(instance_types=[t for _, t in cheap + dear],
                                  requirements=[Requirement(FAMILY, "Exists", [], 3)])
    cp = one_pod_cluster(cat, [pool], price=price)
    r = explain(ctx, cp)[0]
    assert fields(r) == (abi.KP_UNCONS_MIN_VALUES, 0, 0, -1)
    assert r["n_options"] == 5 and r["n_cheaper"] == 3 and r["min_needed"] == 0
    assert r["cheapest_price"] == min(w for w, _ in cheap)


def test_multiple_nodeclaims(ctx, cat):
    t = small_type(cat)
    zones = sorted({o.zone for o in cat[t].offerings})[:2]
    classes = [PodClass([Requirement(ZONE, "In", [z])]) for z in zones]
    cp = one_pod_cluster(cat, [synth.default_nodepool()], classes, specs=[(0, {"cpu": "1"}), (1, {"cpu": "1"})])
    r = explain(ctx, cp)[0]
    assert fields(r) == (abi.KP_UNCONS_MULTIPLE_NODECLAIMS, 0, 0, -1)
    assert r["n_options"] == 0 and r["n_cheaper"] == 0 and r["cheapest_price"] == 0.0
    assert len(ctx.consolidate_explain_pods(SINGLE, 0)) == 0


def test_pods_unschedulable_requirements(ctx, cat):
    amd = [Requirement(ARCH, "In", ["amd64"])]
    classes = [PodClass(), PodClass([Requirement(ARCH, "In", ["arm64"])])]
    pools = [synth.default_nodepool(requirements=list(amd)), synth.default_nodepool("second", weight=5, requirements=list(amd))]
    cp = one_pod_cluster(cat, pools, classes,
                         specs=[(0, {"cpu": "1"}), (1, {"cpu": "1"}), (0, {"cpu": "1"})])
    r = explain(ctx, cp)[0]
    assert fields(r) == (abi.KP_UNCONS_PODS_UNSCHEDULABLE, 0, 1, 1)
    assert r["n_options"] == 0
    rows = ctx.consolidate_explain_pods(SINGLE, 0)
    assert rows["pod"].tolist() == [1, 1] and rows["nodepool"].tolist() == [1, 0]  # template order: weight descending
    assert rows["reason"].tolist() == [abi.KP_WHY_REQUIREMENTS] * 2
    assert [ctx.consolidate_explain_key(int(k)) for k in rows["key"]] == [ARCH, ARCH]
    ms, ct = ctx.consolidate_explain_stats()
    assert ct == [1, 2] and ms[0] > 0


def test_pods_unschedulable_limits_of_the_probe(ctx, cat):
    """Pool a: tainted, cpu limit 4000 that the candidate's 4000 lifts to 8000: the pod's row there is TAINTS with the
    options within 8000, not within 4000.  Pool b: limit 500 (below the smallest type), LIMITS."""
    t = small_type(cat)
    pools = [NodePool("a", 50, [Requirement(CAPACITY_TYPE, "In", ["on-demand"])], taints=[Taint("k", "v", "NoSchedule")],
                      limits_remaining={"cpu": 4000}),
             NodePool("b", 10, [Requirement(CAPACITY_TYPE, "In", ["on-demand"])], limits_remaining={"cpu": 500})]
    prob = model.Problem(cat, pools, [PodClass()], synth.pods_from_specs([(0, {"cpu": "1"})]),
                         existing=[node("n0", cat[t], pool="a")])
    cp = model.ConsolidationProblem(prob, [cand(0, [0], 1.0, t, pool=0, cap=np.array(cat[t].capacity, np.int64))])
    r = explain(ctx, cp)[0]
    assert fields(r) == (abi.KP_UNCONS_PODS_UNSCHEDULABLE, 0, 1, 0)
    rows = ctx.consolidate_explain_pods(SINGLE, 0)
    assert rows["nodepool"].tolist() == [0, 1]
    assert rows["reason"].tolist() == [abi.KP_WHY_TAINTS, abi.KP_WHY_LIMITS]
    ref = explain_ref.Ref(prob)
    at = {lim: ref.explain(0, prob.pods.requests[0], 0, {"cpu": lim})["n_options"] for lim in (4000, 8000)}
    assert 0 < at[4000] < at[8000]
    assert rows["n_options"].tolist() == [at[8000], 0]


def test_uninitialized_node(ctx, cat):
    t = small_type(cat)
    pool = synth.default_nodepool(limits_remaining={"cpu": 0})
    prob = model.Problem(cat, [pool], [PodClass()], synth.pods_from_specs([(0, {"cpu": "1"})]),
                         existing=[node("n0", cat[t], cpu_avail=0), node("n1", cat[t])])
    cp = model.ConsolidationProblem(prob, [cand(0, [0], 1.0, t)], initialized=np.array([1, 0], np.uint8))
    r = explain(ctx, cp)[0]
    assert fields(r) == (abi.KP_UNCONS_PODS_UNSCHEDULABLE, abi.KP_UNCONS_F_UNINITIALIZED_NODE, 0, -1)
    assert len(ctx.consolidate_explain_pods(SINGLE, 0)) == 0


def test_truncated_nodeclaim(ctx, cat):
    """Five types, the four cheapest of one family, max_instance_types 4, Strict minValues 2 on instance-family: the
    NodeClaim starts with two families and TruncateInstanceTypes drops it."""
    od = _od_rows(cat)
    by = {}
    for w, t in od:
        by.setdefault(_family(cat[t]), []).append((w, t))
    a = next(f for f, v in by.items() if len(v) >= 4)
    four = by[a][:4]
    fifth = next((w, t) for w, t in reversed(od) if _family(cat[t]) != a and w > four[-1][0])
    pool = synth.default_nodepool(instance_types=[t for _, t in four + [fifth]],
                                  requirements=[Requirement(FAMILY, "Exists", [], 2)])
    cp = one_pod_cluster(cat, [pool], price=1e6, max_instance_types=4)
    r = explain(ctx, cp)[0]
    assert fields(r) == (abi.KP_UNCONS_PODS_UNSCHEDULABLE, abi.KP_UNCONS_F_TRUNCATED, 1, -1)
    assert r["n_options"] == 0 and r["n_cheaper"] == 0
    row = ctx.consolidate_execute(SINGLE, 1)[0]
    assert (row["decision"], row["all_scheduled"], row["n_new_nodeclaims"]) == (abi.KP_DECISION_NONE, 0, 0)


def test_same_instance_type(ctx, cat):
    """Two candidates of type T whose pods fit one T, the NodePool offers T alone: the replacement is cheaper than the
    pair, and no cheaper than the cheapest candidate of its own type."""
    t = small_type(cat)
    w = cxr.worst_launch_price(cat[t], OD)
    pool = synth.default_nodepool(instance_types=[t])
    prob = model.Problem(cat, [pool], [PodClass()], synth.pods_from_specs([(0, {"cpu": "1"})] * 2),
                         existing=[node("n0", cat[t]), node("n1", cat[t])])
    cp = model.ConsolidationProblem(prob, [cand(0, [0], w, t), cand(1, [1], w, t)])
    r = explain(ctx, cp, MULTI)[0]
    assert fields(r) == (abi.KP_UNCONS_SAME_INSTANCE_TYPE, 0, 0, -1)
    assert r["n_options"] == 1 and r["n_cheaper"] == 1 and r["cheapest_price"] == w and r["candidate_price"] == w + w
    row = ctx.consolidate_execute(MULTI, 1)[0]
    assert (row["decision"], row["valid"]) == (abi.KP_DECISION_REPLACE, 0)


# ------------------------------------------------------------------------------------------------
# fuzz, against cons_explain_ref
# ------------------------------------------------------------------------------------------------
def assert_rows_equal(dev, ref):
    assert len(dev) == len(ref)
    for f in FIELDS:
        np.testing.assert_array_equal(dev[f], ref[f], err_msg=f)


@pytest.mark.parametrize("family,seed", [("fuzz", s) for s in range(12)] + [("min", s) for s in range(8)])
def test_fuzz_against_reference(ctx, golden, family, seed):
    cp, s2s = (cxr.fuzz_case if family == "fuzz" else cxr.min_values_case)(golden, seed)
    ref = cxr.ConsRef(cp, s2s)
    prepare(ctx, cp, s2s)
    for mode in (SINGLE, MULTI):
        assert_rows_equal(ctx.consolidate_explain(mode, n_probes(cp, mode)), ref.rows(mode)[0])


# ------------------------------------------------------------------------------------------------
# the reason against the same pass's kp_probe_result row: reserved, topology and preference generators
# ------------------------------------------------------------------------------------------------
def check_against_rows(xr, rows, single):
    assert len(xr) == len(rows)
    for x, o in zip(xr, rows):
        r = int(x["reason"])
        assert (r == abi.KP_UNCONS_NONE) == (o["decision"] != abi.KP_DECISION_NONE and o["valid"] == 1), (x, o)
        assert (r == abi.KP_UNCONS_SAME_INSTANCE_TYPE) == (o["decision"] == abi.KP_DECISION_REPLACE and o["valid"] == 0)
        assert (r == abi.KP_UNCONS_MULTIPLE_NODECLAIMS) == (o["n_new_nodeclaims"] == 2)
        assert (r == abi.KP_UNCONS_PODS_UNSCHEDULABLE) == (o["n_new_nodeclaims"] < 2 and o["all_scheduled"] == 0)
        if r in PRICE_REASONS:
            assert o["all_scheduled"] == 1 and o["n_new_nodeclaims"] == 1 and o["decision"] == abi.KP_DECISION_NONE
        assert x["candidate_price"] == o["candidate_price"]
        if single and o["decision"] == abi.KP_DECISION_REPLACE and not (
                x["flags"] & abi.KP_UNCONS_F_SPOT_TO_SPOT and x["n_cheaper"] > o["n_replacement_types"]):
            assert x["n_cheaper"] == o["n_replacement_types"]
        if r != abi.KP_UNCONS_PODS_UNSCHEDULABLE:
            assert x["n_unscheduled"] == 0 and x["first_unscheduled"] == -1


def check_pod_rows(ctx, cp, mode, probe, x, max_pods=3):
    """shape of the pod rows behind one PODS_UNSCHEDULABLE probe; UNKNOWN rows carry nothing else"""
    rows = ctx.consolidate_explain_pods(mode, probe, max_pods)
    order = explain_ref.template_order(cp.cluster)
    if x["flags"] & abi.KP_UNCONS_F_TRUNCATED:
        # n_unscheduled also counts the dropped NodeClaim's pods (at least one), which are not listed; the pods the
        # queue still held are: there is one exactly when first_unscheduled names it
        assert len(rows) % len(order) == 0 and len(rows) // len(order) <= min(max_pods, int(x["n_unscheduled"]) - 1)
        assert (len(rows) > 0) == (x["first_unscheduled"] >= 0)
    else:
        assert len(rows) == min(max_pods, int(x["n_unscheduled"])) * len(order)
    pods = rows["pod"].tolist()[::len(order)]
    assert len(set(pods)) == len(pods)
    if pods:
        assert pods[0] == x["first_unscheduled"]
        key = [cxr.queue_key(cp.cluster, p) for p in pods]
        assert key == sorted(key)
    assert rows["nodepool"].tolist() == order * len(pods)
    mine = {int(p) for c in cxr.probe_candidates(cp, mode, probe) for p in cp.candidates[c].pods}
    assert set(pods) <= mine
    for r in rows[rows["reason"] == abi.KP_WHY_UNKNOWN]:
        assert (r["key"], r["criteria"], r["n_requirements"], r["n_fits"], r["n_offering"]) == (-1, 0, 0, 0, 0)
    return rows


def _generated(golden, kind, seed):
    rng = np.random.Generator(np.random.PCG64(9000 + seed))
    if kind == "reserved":
        from test_gpu_consolidation import _reserved_consolidation
        return _reserved_consolidation(golden, seed, full_cluster=seed % 2 == 0)
    sub = [golden[int(i)] for i in sorted(rng.choice(len(golden), size=int(rng.integers(60, 200)), replace=False))]
    if kind == "topology":
        return fuzzgen.fuzz_topology_consolidation(sub, 3100 + seed, n_nodes=int(rng.integers(4, 60)),
                                                   n_pods=int(rng.integers(20, 200)), all_spot=seed % 4 == 0)
    return fuzzgen.fuzz_preference_consolidation(sub, 4100 + seed, n_nodes=int(rng.integers(4, 60)),
                                                 n_pods=int(rng.integers(20, 200)))


def final_stage_problem(prob):
    """The cluster with every class at its last relaxation stage (preferences.Relax run to the end, which is where a pod
    a probe leaves without a place stands): the last of its ORed required node-affinity terms, no preferred term, no
    ScheduleAnyway spread, no preferred pod (anti-)affinity, and the PreferNoSchedule toleration when a NodePool carries
    such a taint."""
    import dataclasses
    pns = any(t.effect == "PreferNoSchedule" for pool in prob.nodepools for t in pool.taints)
    out = []
    for pc in prob.classes:
        topo = [t for t in pc.topology if (t.when_unsatisfiable == "DoNotSchedule" if t.kind == "spread" else t.weight == 0)]
        tol = list(pc.tolerations) + ([model.Toleration("", "Exists", "", "PreferNoSchedule")] if pns else [])
        out.append(dataclasses.replace(pc, required_terms=pc.required_terms[-1:], preferred_terms=[], topology=topo,
                                       tolerations=tol))
    return dataclasses.replace(prob, classes=out)


def _selects(owner, term, pc):
    """the term's selector and namespaces take a pod of class pc (spreads: the owner's namespace)"""
    if term.selector is None:
        return False
    ns_ok = pc.namespace == owner.namespace if term.kind == "spread" or not term.namespaces else pc.namespace in term.namespaces
    return ns_ok and all(synth._selector_ok(q, pc.labels) for q in term.selector)


def topology_status(prob, final, c):
    """"constrained": the final stage of class c owns a required topology term, or a required anti-affinity term of some
    class selects it (an inverse group): its rows must be KP_WHY_UNKNOWN.  "free": it owns none and no anti-affinity
    term of any stage of any class selects it: its rows must equal the reference.  "either": only a preferred
    anti-affinity term selects it; whether a group constrains it depends on how the classes' stages were expanded."""
    if final.classes[c].topology:
        return "constrained"
    status = "free"
    for owner in prob.classes:
        for t in owner.topology:
            if t.kind == "anti" and _selects(owner, t, final.classes[c]):
                if t.weight == 0:
                    return "constrained"
                status = "either"
    return status


def row_tuple(ctx, r):
    return (int(r["nodepool"]), int(r["reason"]), ctx.consolidate_explain_key(int(r["key"])) if r["key"] >= 0 else None,
            int(r["criteria"]), int(r["n_options"]), int(r["n_requirements"]), int(r["n_fits"]), int(r["n_offering"]))


def ref_rows(ref, c, requests, rem):
    """explain_ref's rows of one pod as tuples; None where the reference finds no failing stage (the residual)"""
    out = []
    for w in ref.rows(c, requests, rem):
        out.append(None if w["reason"] is None else (w["nodepool"], w["reason"], w["key"], w["criteria"], w["n_options"],
                                                    w["n_requirements"], w["n_fits"], w["n_offering"]))
    return out


@pytest.mark.parametrize("kind", ["reserved", "topology", "preference"])
def test_reason_agrees_with_probe_row(ctx, golden, kind):
    """Four seeds of the generator: every reason against the same pass's probe row; the pod rows of the
    PODS_UNSCHEDULABLE probes in shape, and, for the probes that made no NodeClaim (their remaining limits are the
    prepared ones plus the candidates' capacity), field by field: KP_WHY_UNKNOWN for a class a topology group constrains,
    explain_ref's row at the class's final relaxation stage for every other."""
    seen = dict(constrained=0, free=0, either=0, probes=0)
    for seed in range(4):
        cp = _generated(golden, kind, seed)
        s2s = seed % 2 == 0
        prob = cp.cluster
        final = final_stage_problem(prob)
        ref = explain_ref.Ref(final)
        has_groups = any(pc.topology for pc in prob.classes)
        prepare(ctx, cp, s2s)
        for mode in (SINGLE, MULTI):
            n = n_probes(cp, mode)
            rows = ctx.consolidate_execute(mode, n)
            xr = ctx.consolidate_explain(mode, n)
            check_against_rows(xr, rows, mode == SINGLE)
            uns = [i for i in range(n) if xr[i]["reason"] == abi.KP_UNCONS_PODS_UNSCHEDULABLE]
            for i in uns[:6]:
                got = check_pod_rows(ctx, cp, mode, i, xr[i])
                if rows[i]["n_new_nodeclaims"] != 0 or not len(got):
                    continue
                red, _pods, _nodes = cxr.reduced_problem(cp, cxr.probe_candidates(cp, mode, i))
                rem = {j: pool.limits_remaining for j, pool in enumerate(red.nodepools) if pool.limits_remaining}
                npools = len(prob.nodepools)
                seen["probes"] += 1
                for q in range(len(got) // npools):
                    mine = got[q * npools:(q + 1) * npools]
                    p = int(mine[0]["pod"])
                    c = int(prob.pods.class_id[p])
                    status = topology_status(prob, final, c) if has_groups else "free"
                    unknown = [int(r["reason"]) for r in mine] == [abi.KP_WHY_UNKNOWN] * npools
                    want = ref_rows(ref, c, prob.pods.requests[p], rem)
                    equal = all(int(r["reason"]) == abi.KP_WHY_UNKNOWN if w is None else row_tuple(ctx, r) == w
                                for r, w in zip(mine, want))
                    where = (kind, seed, mode, i, p, c, status, [row_tuple(ctx, r) for r in mine], want)
                    if status == "constrained":
                        assert unknown, where
                    elif status == "free":
                        assert equal, where
                    else:
                        assert unknown or equal, where
                    seen[status] += 1
    print(kind, seen)
    assert seen["probes"] > 0 and seen["free"] > 0, seen
    if kind == "topology":
        assert seen["constrained"] > 0, seen


# ------------------------------------------------------------------------------------------------
# pod rows on the fuzz seeds without topology, against explain_ref with the probe's remaining limits
# ------------------------------------------------------------------------------------------------
def test_pod_rows_against_reference(ctx, golden):
    n_checked = 0
    for seed in (1, 2, 3, 5, 6, 7):
        cp, s2s = cxr.fuzz_case(golden, seed)
        ref = cxr.ConsRef(cp, s2s)
        prepare(ctx, cp, s2s)
        xr = ctx.consolidate_explain(SINGLE, n_probes(cp, SINGLE))
        for i in np.nonzero(xr["reason"] == abi.KP_UNCONS_PODS_UNSCHEDULABLE)[0].tolist():
            sim = ref.simulate(SINGLE, i)
            if not sim["placeless"]:
                continue  # (an uninitialized-node placement alone: no pod to list)
            rows = check_pod_rows(ctx, cp, SINGLE, i, xr[i])
            pods = rows["pod"].tolist()[::len(cp.cluster.nodepools)]
            assert pods == sim["placeless"][:3]
            pref = explain_ref.Ref(sim["red"])
            rem = ref.remaining(sim)
            got = [(int(r["nodepool"]), int(r["reason"]),
                    ctx.consolidate_explain_key(int(r["key"])) if r["key"] >= 0 else None, int(r["criteria"]),
                    int(r["n_options"]), int(r["n_requirements"]), int(r["n_fits"]), int(r["n_offering"])) for r in rows]
            want = []
            for p in pods:
                for w in pref.rows(int(cp.cluster.pods.class_id[p]), cp.cluster.pods.requests[p], rem):
                    want.append((w["nodepool"], w["reason"], w["key"], w["criteria"], w["n_options"],
                                 w["n_requirements"], w["n_fits"], w["n_offering"]))
            assert got == want, (seed, i)
            n_checked += 1
    assert n_checked >= 10


# ------------------------------------------------------------------------------------------------
# contract
# ------------------------------------------------------------------------------------------------
def _contract_case(golden):
    return fuzzgen.fuzz_consolidation(golden[:200], 77, n_nodes=60, n_pods=250, n_candidates=40)


def test_state_errors(golden):
    c = native.Context(0)
    try:
        cp = _contract_case(golden)
        cv = model.CatalogView(cp.cluster.catalog)
        c.upload_catalog(cv)
        with pytest.raises(native.KpError) as e:
            c.consolidate_explain(SINGLE, 4)
        assert e.value.status == abi.KP_E_STATE
        with pytest.raises(native.KpError) as e:
            c.consolidate_explain_pods(SINGLE, 0)
        assert e.value.status == abi.KP_E_STATE
        c.consolidate_prepare(model.ConsolidateInputView(cp, SINGLE))
        assert len(c.consolidate_explain(SINGLE, 40)) == 40
        c.upload_catalog(cv)
        with pytest.raises(native.KpError) as e:
            c.consolidate_explain(SINGLE, 40)
        assert e.value.status == abi.KP_E_STATE
        with pytest.raises(native.KpError) as e:
            c.consolidate_explain_key(0)
        assert e.value.status == abi.KP_E_STATE
    finally:
        c.close()


def test_short_buffer_and_ranges(ctx, golden):
    import ctypes as C
    cp = _contract_case(golden)
    prepare(ctx, cp)
    buf = np.zeros(10, abi.PROBE_EXPLANATION_DTYPE)
    st = ctx.L.kp_consolidate_explain(ctx.h, SINGLE, 0, 0, buf.ctypes.data_as(C.POINTER(abi.kp_probe_explanation)), 10)
    assert st == abi.KP_E_BUFFER and "40 rows" in ctx.L.kp_last_error(ctx.h).decode()
    for mode in (SINGLE, MULTI):
        n = n_probes(cp, mode)
        full = ctx.consolidate_explain(mode, n)
        assert_rows_equal(ctx.consolidate_explain(mode, n), full)  # twice: equal rows
        assert_rows_equal(ctx.consolidate_explain(mode, n, 7, 19), full[7:19])
        assert_rows_equal(ctx.consolidate_explain(mode, n, 30, 0), full[30:])
    with pytest.raises(native.KpError) as e:
        ctx.consolidate_explain(BOTH, 79)
    assert e.value.status == abi.KP_E_INVALID


def test_explain_leaves_the_pass_alone(ctx, golden):
    cp, s2s = cxr.fuzz_case(golden, 2)
    prepare(ctx, cp, s2s)
    want = ctx.consolidate_command(BOTH)
    want_rows = ctx.consolidate_execute(SINGLE, n_probes(cp, SINGLE))
    prepare(ctx, cp, s2s)
    nb = n_probes(cp, BOTH)
    both = ctx.consolidate_execute(BOTH, nb)
    ms0, ct0 = ctx.consolidate_stats()
    xr = ctx.consolidate_explain(SINGLE, n_probes(cp, SINGLE))
    ctx.consolidate_explain(MULTI, n_probes(cp, MULTI))
    for i in np.nonzero(xr["reason"] == abi.KP_UNCONS_PODS_UNSCHEDULABLE)[0][:2].tolist():
        ctx.consolidate_explain_pods(SINGLE, i)
    ms1, ct1 = ctx.consolidate_stats()
    assert ct1 == ct0 and ms1 == ms0  # counters [18..19] included: no pass launched, no read-back
    got = ctx.consolidate_command(BOTH)
    assert got == want
    _, ct2 = ctx.consolidate_stats()
    assert ct2[18] == ct0[18]  # the command replayed the BOTH pass
    np.testing.assert_array_equal(ctx.consolidate_execute(BOTH, nb), both)
    np.testing.assert_array_equal(ctx.consolidate_execute(SINGLE, n_probes(cp, SINGLE)), want_rows)
    if want.decision == abi.KP_DECISION_REPLACE:
        assert ctx.consolidate_replacement(want.mode, want.probe) == want


def test_multi_device_ctx_runs_on_the_primary(ctx, golden):
    cp, s2s = cxr.fuzz_case(golden, 4)
    one = [explain(ctx, cp, mode, s2s) for mode in (SINGLE, MULTI)]
    c2 = native.Context(0, devices=[0, 0])
    try:
        for mode, want in zip((SINGLE, MULTI), one):
            assert_rows_equal(explain(c2, cp, mode, s2s), want)
    finally:
        c2.close()


def test_every_probe_has_a_command(ctx, cat):
    """three one-pod candidates next to an empty node with room for all: every probe deletes"""
    t = small_type(cat)
    prob = model.Problem(cat, [synth.default_nodepool()], [PodClass()], synth.pods_from_specs([(0, {"cpu": "1"})] * 3),
                         existing=[node("n%d" % i, cat[t]) for i in range(4)])
    cp = model.ConsolidationProblem(prob, [cand(i, [i], 1.0, t) for i in range(3)])
    for mode in (SINGLE, MULTI):
        xr = explain(ctx, cp, mode)
        assert xr["reason"].tolist() == [abi.KP_UNCONS_NONE] * n_probes(cp, mode)
        assert not xr["flags"].any() and not xr["n_options"].any()
        for i in range(len(xr)):
            assert len(ctx.consolidate_explain_pods(mode, i)) == 0


def test_consolidator_explain(golden):
    cp, s2s = cxr.fuzz_case(golden, 1)
    con = consolidation.Consolidator(cp.cluster.catalog, spot_to_spot=s2s)
    try:
        rows = con.probes(cp, SINGLE)
        xr = con.explain(cp, SINGLE)
        assert xr.dtype == abi.PROBE_EXPLANATION_DTYPE
        check_against_rows(xr, rows, True)
    finally:
        con.ctx.close()
