"""GPU: kp_solve_explain — why each NodePool refused the pods a Solve left unschedulable.

Hand-made cases with plain expectations (one reason each), the fuzz seeds of tests/test_explain_cpu.py compared field
by field with tests/explain_ref.py (which that file pins to the oracle), the word edges of the type sweep, the
work-unit bound (evaluated pairs = distinct shapes x NodePools) and the call's read-only contract.
"""
import copy
import dataclasses

import numpy as np
import pytest

import edge_cases
import explain_ref
import fuzzgen
import pyoracle
from kpsim import abi, model, native, scheduler, synth
from kpsim.model import (CAPACITY_TYPE, INSTANCE_TYPE, ZONE, HostPort, NodePool, PodClass, Requirement, Taint,
                         Toleration, TopologyTerm)

pytestmark = pytest.mark.gpu

AWS = "karpenter.k8s.aws/"
FAMILY = AWS + "instance-family"
CPU = model.RIDX["cpu"]
C_REQ, C_FIT, C_OFF = abi.KP_CRIT_REQUIREMENTS, abi.KP_CRIT_FITS, abi.KP_CRIT_OFFERING
C_RF, C_RO, C_FO = (abi.KP_CRIT_REQUIREMENTS_AND_FITS, abi.KP_CRIT_REQUIREMENTS_AND_OFFERING,
                    abi.KP_CRIT_FITS_AND_OFFERING)
ZONES = ["test-zone-1a", "test-zone-1b", "test-zone-1c"]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sub(golden):
    return explain_ref.catalog_of(golden)


def solve(ctx, prob, cv=None, upload=True):
    """Solve on the device (without the catalog upload when the caller patched it) -> model.Results."""
    if upload:
        ctx.upload_catalog(cv or model.CatalogView(prob.catalog))
    cap_nc = max(16, prob.pods.n + 1)
    m = prob.max_instance_types if prob.max_instance_types > 0 else len(prob.catalog)
    out = model.OutputBuffers(prob.pods.n, cap_nc, cap_nc * m)
    ctx.solve(model.SolveInputView(prob), out)
    return out.results()


def by_pod(rows):
    out = {}
    for r in rows:
        out.setdefault(int(r["pod"]), []).append(r)
    return out


def explain(ctx, prob, res):
    """explain() of every unschedulable pod, checked for shape: the pods are exactly the unschedulable ones, in
    ascending order, each with one row per NodePool in template order; UNKNOWN appears nowhere."""
    rows = ctx.explain()
    uns = np.nonzero(res.pod_result == abi.KP_POD_UNSCHEDULABLE)[0].tolist()
    order = explain_ref.template_order(prob)
    assert rows["pod"].tolist() == [p for p in uns for _ in order]
    assert rows["nodepool"].tolist() == order * len(uns)
    assert abi.KP_WHY_UNKNOWN not in rows["reason"].tolist()
    return by_pod(rows)


def key_name(ctx, r):
    return ctx.explain_key(int(r["key"])) if r["key"] >= 0 else None


def as_tuple(ctx, r):
    return (int(r["nodepool"]), int(r["reason"]), key_name(ctx, r), int(r["criteria"]), int(r["n_options"]),
            int(r["n_requirements"]), int(r["n_fits"]), int(r["n_offering"]))


def ref_tuple(row):
    return (row["nodepool"], row["reason"], row["key"], row["criteria"], row["n_options"], row["n_requirements"],
            row["n_fits"], row["n_offering"])


def assert_rows_equal_ref(ctx, prob, got, remaining=None):
    """Every row of every pod in `got` equals explain_ref, field by field."""
    ref = explain_ref.Ref(prob)
    cache = {}
    assert got
    for p, rows in got.items():
        shape = (int(prob.pods.class_id[p]), tuple(int(x) for x in prob.pods.requests[p]))
        if shape not in cache:
            cache[shape] = [ref_tuple(r) for r in ref.rows(shape[0], np.array(shape[1]), remaining)]
        assert [as_tuple(ctx, r) for r in rows] == cache[shape], (p, shape)


def pods(specs):
    return synth.pods_from_specs(specs)


def one_reason(ctx, prob, reason, pod=None, cv=None):
    res = solve(ctx, prob, cv)
    got = explain(ctx, prob, res)
    p = max(got) if pod is None else pod
    assert [int(r["reason"]) for r in got[p]] == [reason] * len(prob.nodepools), got[p]
    return res, got, got[p][0]


# ------------------------------------------------------------------------------------------------
# hand-made cases, one reason each
# ------------------------------------------------------------------------------------------------
def test_untolerated_taint(ctx, sub):
    pool = synth.default_nodepool(taints=[Taint("dedicated", "db", "NoSchedule")])
    prob = model.Problem(sub, [pool], [PodClass(), PodClass(tolerations=[Toleration("dedicated", "Exists")])],
                         pods([(0, {"cpu": "1"}), (1, {"cpu": "1"})]))
    res, got, r = one_reason(ctx, prob, abi.KP_WHY_TAINTS)
    assert list(got) == [0] and res.pod_result[1] >= 0
    assert r["key"] == -1 and r["criteria"] == 0 and r["n_options"] > 0 and r["n_fits"] == 0


def _type_with_cpu(sub, milli):
    return next(it for it in sub if it.capacity[CPU] == milli and any(o.available and o.capacity_type == "on-demand"
                                                                        for o in it.offerings))


def test_limit_used_up_by_the_same_solve(ctx, sub):
    """The final-state dependence: the NodePool's cpu limit admits two NodeClaims of the one type; the first two pods
    take them, the later ones find every type over the remaining limit."""
    it = _type_with_cpu(sub, 4000)
    pool = synth.default_nodepool(requirements=[Requirement(INSTANCE_TYPE, "In", [it.name])],
                                  limits_remaining={"cpu": 2 * 4000})
    prob = model.Problem(sub, [pool], [PodClass()], pods([(0, {"cpu": "3"})] * 5))
    assert explain_ref.Ref(prob).explain(0, prob.pods.requests[0], 0)["reason"] is None  # the input's limits admit it
    res, got, r = one_reason(ctx, prob, abi.KP_WHY_LIMITS)
    assert (res.pod_result >= 0).sum() == 2 and len(got) == 3
    assert r["n_options"] == 0 and r["key"] == -1


def test_daemonset_host_port(ctx, sub):
    pool = synth.default_nodepool(daemon_host_ports=[HostPort(8080)])
    prob = model.Problem(sub, [pool], [PodClass(host_ports=[HostPort(8080)]), PodClass(host_ports=[HostPort(8081)])],
                         pods([(0, {"cpu": "1"}), (1, {"cpu": "1"})]))
    res, got, r = one_reason(ctx, prob, abi.KP_WHY_HOST_PORTS)
    assert list(got) == [0]


def test_zone_outside_the_nodepool(ctx, sub):
    pool = synth.default_nodepool(requirements=[Requirement(ZONE, "In", [ZONES[0]])])
    prob = model.Problem(sub, [pool], [PodClass([Requirement(ZONE, "In", [ZONES[1]])])], pods([(0, {"cpu": "1"})]))
    _, _, r = one_reason(ctx, prob, abi.KP_WHY_REQUIREMENTS)
    assert key_name(ctx, r) == ZONE


def test_custom_key_the_template_lacks(ctx, sub):
    prob = model.Problem(sub, [synth.default_nodepool()], [PodClass([Requirement("example.com/team", "In", ["a"])])],
                         pods([(0, {"cpu": "1"})]))
    _, _, r = one_reason(ctx, prob, abi.KP_WHY_REQUIREMENTS)
    assert key_name(ctx, r) == "example.com/team"


def test_hostname_requirement_is_not_a_taint(ctx, sub):
    """A pod pinned to a hostname meets no new NodeClaim's placeholder: REQUIREMENTS on kubernetes.io/hostname at a
    NodePool it tolerates (tainted or not), TAINTS only where it does not tolerate the taint; with a second failing
    key the one whose name sorts first is named."""
    host = explain_ref.HOSTNAME
    pools = [NodePool("a-plain", 30, [Requirement(CAPACITY_TYPE, "In", ["on-demand"])]),
             NodePool("b-tainted", 20, [Requirement(CAPACITY_TYPE, "In", ["on-demand"])], taints=[Taint("k", "v")]),
             NodePool("c-zone", 10, [Requirement(CAPACITY_TYPE, "In", ["on-demand"]), Requirement(ZONE, "In", [ZONES[2]])])]
    pin = Requirement(host, "In", ["node-7"])
    classes = [PodClass([pin]), PodClass([pin], tolerations=[Toleration("k", "Exists")]),
               PodClass([pin, Requirement("example.com/team", "In", ["a"])]),
               PodClass([pin, Requirement(ZONE, "In", [ZONES[0]])]),
               PodClass([Requirement(host, "DoesNotExist")]), PodClass([Requirement(host, "Gt", ["3"])]),
               PodClass([Requirement(host, "NotIn", ["node-7"])])]
    prob = model.Problem(sub, pools, classes, pods([(c, {"cpu": "1"}) for c in range(len(classes))]))
    res = solve(ctx, prob)
    got = explain(ctx, prob, res)
    assert sorted(got) == [0, 1, 2, 3, 4, 5] and res.pod_result[6] >= 0
    R, T = abi.KP_WHY_REQUIREMENTS, abi.KP_WHY_TAINTS
    want = {0: [(R, host), (T, None), (R, host)], 1: [(R, host), (R, host), (R, host)],
            2: [(R, "example.com/team"), (T, None), (R, "example.com/team")],
            3: [(R, host), (T, None), (R, host)],   # "kubernetes.io/hostname" sorts before "topology.kubernetes.io/zone"
            4: [(R, host), (T, None), (R, host)], 5: [(R, host), (T, None), (R, host)]}
    for p, rows in got.items():
        assert [(int(r["reason"]), key_name(ctx, r)) for r in rows] == want[p], p
    assert_rows_equal_ref(ctx, prob, got)


def test_request_no_type_holds(ctx, sub):
    prob = model.Problem(sub, [synth.default_nodepool()], [PodClass()], pods([(0, {"cpu": "10000"})]))
    _, _, r = one_reason(ctx, prob, abi.KP_WHY_INSTANCE_TYPES)
    assert r["criteria"] == C_REQ | C_OFF | C_RO and r["n_fits"] == 0
    assert r["n_requirements"] == r["n_options"] > 0 and 0 < r["n_offering"] <= r["n_options"]


def test_label_value_no_type_carries(ctx, sub):
    prob = model.Problem(sub, [synth.default_nodepool()],
                         [PodClass([Requirement(AWS + "instance-category", "In", ["zz"])])], pods([(0, {"cpu": "1"})]))
    _, _, r = one_reason(ctx, prob, abi.KP_WHY_INSTANCE_TYPES)
    assert not r["criteria"] & C_REQ and r["n_requirements"] == 0
    assert r["criteria"] == C_FIT | C_OFF | C_FO


def test_spot_required_every_spot_offering_patched_unavailable(ctx, sub):
    cv = model.CatalogView(sub)
    ctx.upload_catalog(cv)
    avail = np.array([1 if (o.available and o.capacity_type != "spot") else 0 for it in sub for o in it.offerings], np.uint8)
    ctx.patch_avail(avail, 2)
    prob = model.Problem(sub, [synth.default_nodepool(capacity_types=("spot", "on-demand"))],
                         [PodClass([Requirement(CAPACITY_TYPE, "In", ["spot"])])], pods([(0, {"cpu": "1"})]))
    res = solve(ctx, prob, upload=False)
    got = explain(ctx, prob, res)
    r = got[0][0]
    assert r["reason"] == abi.KP_WHY_INSTANCE_TYPES
    assert not r["criteria"] & C_OFF and r["n_offering"] == 0
    assert r["criteria"] == C_REQ | C_FIT | C_RF and r["n_requirements"] > 0


def test_family_too_small_others_fit(ctx, sub):
    fams = {}
    for it in sub:
        if it.labels.get(FAMILY):
            fams.setdefault(it.labels[FAMILY][0], []).append(int(it.allocatable[CPU]))
    biggest = max(max(v) for v in fams.values())
    fam, top = min(((f, max(v)) for f, v in fams.items() if 2 * max(v) < biggest), key=lambda x: (x[1], x[0]))
    prob = model.Problem(sub, [synth.default_nodepool()], [PodClass([Requirement(FAMILY, "In", [fam])])],
                         pods([(0, {"cpu": top + 1000})]))
    _, _, r = one_reason(ctx, prob, abi.KP_WHY_INSTANCE_TYPES)
    assert r["criteria"] & (C_REQ | C_FIT | C_OFF) == C_REQ | C_FIT | C_OFF
    assert not r["criteria"] & C_RF
    assert 0 < r["n_requirements"] <= len(fams[fam]) and r["n_fits"] > 0


def test_strict_min_values_unmet_best_effort_schedules(ctx, sub):
    fam = sub[0].labels[FAMILY][0]
    pool = synth.default_nodepool(requirements=[Requirement(FAMILY, "Exists", [], 3)])
    prob = model.Problem(sub, [pool], [PodClass([Requirement(FAMILY, "In", [fam])])], pods([(0, {"cpu": "1"})]))
    _, _, r = one_reason(ctx, prob, abi.KP_WHY_MIN_VALUES)
    assert key_name(ctx, r) == FAMILY and r["criteria"] == 0 and r["n_fits"] > 0
    relaxed = dataclasses.replace(prob, min_values_policy=1)
    res = solve(ctx, relaxed)
    assert res.pod_result[0] >= 0 and len(ctx.explain()) == 0


def test_reservation_spent(ctx, sub):
    """Both pods require reserved capacity and fill a node each; the one reservation has capacity 1."""
    cat = copy.deepcopy(sub)
    it = next(t for t in cat if t.capacity[CPU] == 4000 and any(o.available and o.capacity_type == "on-demand"
                                                                for o in t.offerings))
    od = next(o for o in it.offerings if o.available and o.capacity_type == "on-demand")
    it.offerings.append(model.Offering("reserved", od.zone, od.price / 1e7, True, od.zone_id, "cr-1", "default", 1))
    it.labels[CAPACITY_TYPE] = list(it.labels[CAPACITY_TYPE]) + ["reserved"]
    it.labels[model.RESERVATION_ID] = ["cr-1"]
    it.labels[model.RESERVATION_TYPE] = ["default"]
    prob = model.Problem(cat, [synth.default_nodepool(capacity_types=("reserved",))], [PodClass()],
                         pods([(0, {"cpu": "3"})] * 2))
    res, got, r = one_reason(ctx, prob, abi.KP_WHY_RESERVED)
    assert res.pod_result[0] >= 0 and list(got) == [1]
    assert r["n_requirements"] == r["n_fits"] == r["n_offering"] == 1


def test_zonal_anti_affinity_more_pods_than_zones(ctx, sub):
    anti = TopologyTerm("anti", ZONE, selector=[Requirement("app", "In", ["a"])])
    prob = model.Problem(sub, [synth.default_nodepool()], [PodClass(labels={"app": "a"}, topology=[anti])],
                         pods([(0, {"cpu": "1"})] * 5))
    res, got, r = one_reason(ctx, prob, abi.KP_WHY_TOPOLOGY)
    # at most one pod per zone; core places fewer in one Solve (a NodeClaim not yet narrowed to one zone records the
    # anti-affinity in every zone it may land in): the oracle says how many, every other pod is the surplus
    np.testing.assert_array_equal(res.pod_result, pyoracle.solve(prob).results.pod_result)
    placed = int((res.pod_result >= 0).sum())
    assert 1 <= placed <= 3 and len(got) == 5 - placed
    for rows in got.values():
        assert [int(x["reason"]) for x in rows] == [abi.KP_WHY_TOPOLOGY]


def test_three_nodepools_three_reasons_in_template_order(ctx, sub):
    smallest = min(int(it.capacity[CPU]) for it in sub)
    pools = [NodePool("c-limits", 0, [Requirement(CAPACITY_TYPE, "In", ["on-demand"])],
                      limits_remaining={"cpu": smallest - 1}),
             NodePool("a-taint", 50, [Requirement(CAPACITY_TYPE, "In", ["on-demand"])], taints=[Taint("k", "v")]),
             NodePool("b-zone", 10, [Requirement(CAPACITY_TYPE, "In", ["on-demand"]), Requirement(ZONE, "In", [ZONES[2]])])]
    prob = model.Problem(sub, pools, [PodClass([Requirement(ZONE, "In", [ZONES[0]])])], pods([(0, {"cpu": "1"})]))
    res = solve(ctx, prob)
    rows = explain(ctx, prob, res)[0]
    assert [int(r["nodepool"]) for r in rows] == [1, 2, 0]
    assert [int(r["reason"]) for r in rows] == [abi.KP_WHY_TAINTS, abi.KP_WHY_REQUIREMENTS, abi.KP_WHY_LIMITS]
    assert key_name(ctx, rows[1]) == ZONE
    s = scheduler.Scheduler(sub, ctx=ctx)
    assert s.Solve(prob).pod_errors == [0]
    ex = s.explain()[0]
    assert [(e.nodepool, e.reason_name, e.key) for e in ex] == [("a-taint", "TAINTS", None), ("b-zone", "REQUIREMENTS", ZONE),
                                                               ("c-limits", "LIMITS", None)]


def test_final_relaxation_stage_is_explained(ctx, sub):
    """The preferred zone is outside the NodePool's (REQUIREMENTS while the preference stands); the pod ends without
    it, and its request is too large."""
    pool = synth.default_nodepool(requirements=[Requirement(ZONE, "In", ZONES)])
    cls = PodClass(preferred_terms=[(10, [Requirement(ZONE, "In", ["nowhere-1z"])])])
    prob = model.Problem(sub, [pool], [cls], pods([(0, {"cpu": "10000"})]))
    _, _, r = one_reason(ctx, prob, abi.KP_WHY_INSTANCE_TYPES)
    assert r["criteria"] == C_REQ | C_OFF | C_RO and r["n_fits"] == 0 and r["key"] == -1


# ------------------------------------------------------------------------------------------------
# fuzz: field by field against explain_ref
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", explain_ref.SEEDS)
def test_fuzz_rows_equal_the_reference(ctx, sub, seed):
    prob = explain_ref.problem(sub, seed)
    cv = model.CatalogView(sub)
    res = solve(ctx, prob, cv)
    orc = pyoracle.solve(prob, cv).results
    np.testing.assert_array_equal(res.pod_result, orc.pod_result)
    got = explain(ctx, prob, res)
    assert_rows_equal_ref(ctx, prob, got, explain_ref.Ref(prob).final_remaining(orc))


def topology_problem(sub, seed):
    """fuzzgen.fuzz_topology_problem without NodePool limits (their final state under topology narrowing is not
    something explain_ref replays)."""
    prob = fuzzgen.fuzz_problem(sub, seed, n_pods=150, n_classes=10, with_limits=False)
    return fuzzgen.add_topology(np.random.Generator(np.random.PCG64(seed + 99)), prob)


def check_topology_row(h, w, where):
    """A row `h` of a class under topology against the reference's row `w`, which knows no topology.

    Where the reference finds a stage before topology, the row equals it.  Otherwise the row is TOPOLOGY, or it equals
    what the reference finds for the later stages, or, the one case that rule cannot cover, Topology.AddRequirements
    passed and narrowed a key (a spread's next domain, an affinity's domain) and the later stages then fail under the
    narrowed requirements, which the reference never sees.  Narrowing can only remove instance types, and it touches
    neither the limits nor Fits.  So such a row is INSTANCE_TYPES or MIN_VALUES with the reference's n_options and
    n_fits exactly, n_requirements and n_offering no larger than the reference's, the single-criterion bits agreeing
    with the counts, and every pair bit backed by both of its single bits.  (The tuples: nodepool, reason, key,
    criteria, n_options, n_requirements, n_fits, n_offering.)"""
    early = (abi.KP_WHY_LIMITS, abi.KP_WHY_TAINTS, abi.KP_WHY_HOST_PORTS, abi.KP_WHY_REQUIREMENTS)
    if w[1] in early:
        assert h == w, where
        return "early"
    if h[1] == abi.KP_WHY_TOPOLOGY:
        assert h[2] is None and h[3] == 0 and h[4] == w[4] and h[5:] == (0, 0, 0), where
        return "topology"
    if h == w:
        return "same"
    assert h[1] in (abi.KP_WHY_INSTANCE_TYPES, abi.KP_WHY_MIN_VALUES), where
    assert h[0] == w[0] and h[4] == w[4] and h[6] == w[6] and h[5] <= w[5] and h[7] <= w[7], where
    if h[1] == abi.KP_WHY_INSTANCE_TYPES:
        crit = h[3]
        assert bool(crit & C_REQ) == (h[5] > 0) and bool(crit & C_FIT) == (h[6] > 0) and bool(crit & C_OFF) == (h[7] > 0), where
        for pair, a, b in ((C_RF, C_REQ, C_FIT), (C_RO, C_REQ, C_OFF), (C_FO, C_FIT, C_OFF)):
            assert not crit & pair or (crit & a and crit & b), where
        assert h[2] is None
    else:
        assert h[3] == 0 and h[2] is not None, where
    return "narrowed"


TOPOLOGY_SEEDS = range(8)


def test_fuzz_topology_rows(ctx, sub):
    """Topology problems: the device leaves the pods unschedulable that the oracle leaves; rows of classes no topology
    term can touch equal the reference field by field, rows of the others pass check_topology_row.  Over the seeds the
    strict outcomes carry the test: rows that are TOPOLOGY, rows that equal the reference at an earlier stage and rows
    that equal it at a later one all occur, and the narrowed rows are a minority."""
    cv = model.CatalogView(sub)
    kinds, free_rows = {}, 0
    for seed in TOPOLOGY_SEEDS:
        prob = topology_problem(sub, seed)
        res = solve(ctx, prob, cv)
        np.testing.assert_array_equal(res.pod_result, pyoracle.solve(prob, cv).results.pod_result)
        rows = ctx.explain()
        assert abi.KP_WHY_UNKNOWN not in rows["reason"].tolist()
        assert sorted(set(rows["pod"].tolist())) == np.nonzero(res.pod_result == abi.KP_POD_UNSCHEDULABLE)[0].tolist()
        ref = explain_ref.Ref(prob)
        any_anti = any(t.kind == "anti" for pc in prob.classes for t in pc.topology)  # inverse groups constrain other classes
        for p, prow in by_pod(rows).items():
            c = int(prob.pods.class_id[p])
            want = [ref_tuple(r) for r in ref.rows(c, prob.pods.requests[p])]
            have = [as_tuple(ctx, r) for r in prow]
            free = not prob.classes[c].topology and not any_anti
            for h, w in zip(have, want):
                if free:
                    assert h == w, (seed, p, c)
                    free_rows += 1
                else:
                    k = check_topology_row(h, w, (seed, p, c, h, w))
                    kinds[k] = kinds.get(k, 0) + 1
    print("topology rows by kind %s, rows of classes without topology %d" % (kinds, free_rows))
    # every strict kind occurs, and the one looser branch does not carry the test: it takes a minority of the rows
    assert kinds.get("topology", 0) > 0 and kinds.get("early", 0) > 0 and kinds.get("same", 0) > 0, kinds
    assert 2 * kinds.get("narrowed", 0) < sum(kinds.values()), kinds


# ------------------------------------------------------------------------------------------------
# word edges of the sweep
# ------------------------------------------------------------------------------------------------
def edge_problem(cat, pools=None):
    classes = [PodClass(), PodClass([Requirement(AWS + "instance-category", "In", ["zz"])]),
               PodClass([Requirement(ZONE, "In", [ZONES[0]]), Requirement(CAPACITY_TYPE, "In", ["spot"])])]
    specs = [(0, {"cpu": "10000"}), (1, {"cpu": "1"}), (2, {"cpu": "10000"}), (0, {"cpu": "1"})]
    return model.Problem(cat, pools or [synth.default_nodepool(capacity_types=("on-demand", "spot"))], classes, pods(specs))


@pytest.mark.parametrize("T", [1, 64, 65, 129])
def test_catalog_word_tails(ctx, golden, T):
    """1, 64, 65 and 129 types: the counts cover every option and no bit past T in the last word."""
    cat = edge_cases.sample(golden, T, 7 + T)
    prob = edge_problem(cat)
    res = solve(ctx, prob)
    got = explain(ctx, prob, res)
    assert sorted(got) == [0, 1, 2]
    assert_rows_equal_ref(ctx, prob, got)
    assert got[0][0]["n_requirements"] == got[0][0]["n_options"] <= T


def test_63_nodepools(ctx, sub):
    """Template 62 is the only one the pod tolerates (bit 62 of the class's toleration mask)."""
    pools = [synth.default_nodepool("p%02d" % j, taints=[] if j == 62 else [Taint("k", "v")]) for j in range(63)]
    prob = edge_problem(sub, pools)
    res = solve(ctx, prob)
    got = explain(ctx, prob, res)
    assert [int(r["reason"]) for r in got[0]] == [abi.KP_WHY_TAINTS] * 62 + [abi.KP_WHY_INSTANCE_TYPES]
    assert_rows_equal_ref(ctx, prob, got)


def test_eight_resource_axes(ctx, sub):
    """Eight requested axes: two more than the Solve stages; each class fails on one of the wide ones alone."""
    wide = ["nvidia.com/gpu", "vpc.amazonaws.com/efa", "aws.amazon.com/neuron", "vpc.amazonaws.com/pod-eni"]
    specs = [(0, {"cpu": "1", "memory": "1Gi", "ephemeral-storage": "1Gi", r: 1000 * 1000}) for r in wide]
    specs.append((0, {"cpu": "1", "memory": "1Gi"}))
    prob = model.Problem(sub, [synth.default_nodepool()], [PodClass()], pods(specs))
    assert (prob.pods.requests.sum(axis=0) > 0).sum() == 8
    res = solve(ctx, prob)
    got = explain(ctx, prob, res)
    assert sorted(got) == [0, 1, 2, 3] and res.pod_result[4] >= 0
    for p in got:
        assert got[p][0]["criteria"] == C_REQ | C_OFF | C_RO and got[p][0]["n_fits"] == 0
    assert_rows_equal_ref(ctx, prob, got)


def test_class_at_the_class_key_maximum(ctx, sub):
    keys = ["example.com/k%02d" % i for i in range(32)]
    every = PodClass([Requirement(k, "In", ["a"]) for k in keys])
    last = PodClass([Requirement(k, "NotIn", ["a"]) for k in keys[:31]] + [Requirement(keys[31], "In", ["a"])])
    prob = model.Problem(sub, [synth.default_nodepool()], [every, last], pods([(0, {"cpu": "1"}), (1, {"cpu": "1"})]))
    res = solve(ctx, prob)
    got = explain(ctx, prob, res)
    assert (got[0][0]["reason"], key_name(ctx, got[0][0])) == (abi.KP_WHY_REQUIREMENTS, keys[0])
    assert (got[1][0]["reason"], key_name(ctx, got[1][0])) == (abi.KP_WHY_REQUIREMENTS, keys[31])
    assert_rows_equal_ref(ctx, prob, got)


# ------------------------------------------------------------------------------------------------
# the work unit and the read-only contract
# ------------------------------------------------------------------------------------------------
def test_4000_pods_three_shapes_five_nodepools(ctx, sub):
    pools = [synth.default_nodepool("p%d" % j) for j in range(5)]
    classes = [PodClass(), PodClass([Requirement(AWS + "instance-category", "In", ["zz"])])]
    kinds = [(0, {"cpu": "10000"}), (0, {"cpu": "20000"}), (1, {"cpu": "1"})]
    prob = model.Problem(sub, pools, classes, pods([kinds[i % 3] for i in range(4000)]))
    res = solve(ctx, prob)
    assert (res.pod_result == abi.KP_POD_UNSCHEDULABLE).all()
    rows = ctx.explain()
    assert len(rows) == 20000
    ms, (pairs, shapes, n) = ctx.explain_stats()
    assert (pairs, shapes, n) == (15, 3, 4000)
    fields = [f for f in rows.dtype.names if f != "pod"]
    per_pod = rows.reshape(4000, 5)
    for k in range(3):
        block = per_pod[k::3][fields]
        assert (block == block[0]).all()
    assert abi.KP_WHY_UNKNOWN not in rows["reason"].tolist()
    print("explain of 4,000 pods: kernel %.3f ms, call %.3f ms; ffd %.3f ms" % (ms[0], ms[1], ctx.kernel_times_ms()[3]))


def test_explain_changes_nothing(ctx, sub):
    prob = explain_ref.problem(sub, 5)
    ctx.upload_catalog(model.CatalogView(sub))
    iv = model.SolveInputView(prob)

    def fetch():
        out = model.OutputBuffers(prob.pods.n, prob.pods.n + 1, (prob.pods.n + 1) * prob.max_instance_types)
        ctx.fetch(out)
        r = out.results()
        return (r.pod_result.tolist(), r.pod_order.tolist(), r.nodeclaim_nodepool.tolist(), r.nodeclaim_n_options.tolist(),
                [list(t) for t in r.nodeclaim_types], [ctx.nodeclaim_requirements(i) for i in range(r.n_nodeclaims)])

    ctx.prepare(iv)
    ctx.execute()
    before = fetch()
    first = ctx.explain()
    assert len(first) > 0
    assert fetch() == before                                   # fetch after explain is unchanged
    assert (ctx.explain() == first).all()                      # explain twice
    some = sorted(set(first["pod"].tolist()))[::2]
    assert (ctx.explain(some) == first[np.isin(first["pod"], some)]).all()
    scheduled = int(np.nonzero(np.array(before[0]) >= 0)[0][0])
    with pytest.raises(native.KpError) as e:
        ctx.explain([scheduled])
    assert e.value.status == abi.KP_E_INVALID
    ctx.execute()
    assert (ctx.explain() == first).all()                      # execute again, then explain
    assert fetch() == before
    ctx.prepare(iv)
    with pytest.raises(native.KpError) as e:
        ctx.explain()                                          # a new prepare without execute
    assert e.value.status == abi.KP_E_STATE


def test_nothing_unschedulable(ctx, sub):
    prob = model.Problem(sub, [synth.default_nodepool()], [PodClass()], pods([(0, {"cpu": "1"})] * 3))
    res = solve(ctx, prob)
    assert (res.pod_result >= 0).all() and len(ctx.explain()) == 0
    assert ctx.explain_stats()[1] == [0, 0, 0]
