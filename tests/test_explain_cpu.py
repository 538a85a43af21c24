"""CPU: the reference of kp_solve_explain (tests/explain_ref.py) pinned to the unmodified oracle, the conditions that
keep the GPU fuzz of tests/test_gpu_explain.py from being vacuous, and the call's argument handling through the CPU
stand-in of the HIP runtime.

The oracle reports no reasons.  What it does report is whether a pod gets a NodeClaim, so for every (class and
requests, NodePool) pair of the fuzz seeds a one-pod, one-NodePool oracle Solve must make a NodeClaim iff the ladder of
explain_ref finds no failing stage: with the NodePool's limits as the seed has them, and with the limits the full
oracle Solve left (explain_ref.final_remaining), which is what pins the limits stage at the final state.
"""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import explain_ref
import pyoracle
from kpsim import abi, model

SEEDS, catalog_of, problem, shapes_of = explain_ref.SEEDS, explain_ref.catalog_of, explain_ref.problem, explain_ref.shapes_of


@pytest.fixture(scope="module")
def corpus(golden):
    sub = catalog_of(golden)
    cv = model.CatalogView(sub)
    out = {}
    for seed in SEEDS:
        prob = problem(sub, seed)
        res = pyoracle.solve(prob, cv).results
        ref = explain_ref.Ref(prob)
        out[seed] = (prob, res, ref, ref.final_remaining(res), cv)
    return out


def one_pod_makes_nodeclaim(prob, cv, c, requests, npi, limits):
    pool = dataclasses.replace(prob.nodepools[npi], limits_remaining=limits)
    pods = model.Pods(np.array([c], np.int32), np.array([requests], np.int64), np.zeros(1, np.int64), ["pod-0"])
    one = model.Problem(prob.catalog, [pool], prob.classes, pods, max_instance_types=prob.max_instance_types,
                        min_values_policy=prob.min_values_policy)
    r = pyoracle.solve(one, cv).results
    return r.n_nodeclaims == 1 and int(r.pod_result[0]) == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_ladder_agrees_with_the_oracle(corpus, seed):
    prob, res, ref, final, cv = corpus[seed]
    checked = 0
    for c, rq in shapes_of(prob, range(prob.pods.n)):
        for npi, pool in enumerate(prob.nodepools):
            cases = [pool.limits_remaining]
            if npi in final:
                cases.append(final[npi])
            for limits in cases:
                row = ref.explain(c, np.array(rq), npi, limits if limits is not None else {})
                got = one_pod_makes_nodeclaim(prob, cv, c, rq, npi, limits)
                assert got == (row["reason"] is None), (seed, c, npi, limits, row)
                checked += 1
    assert checked >= 3 * len(prob.nodepools)


@pytest.mark.parametrize("seed", SEEDS)
def test_unschedulable_pods_fail_at_every_nodepool(corpus, seed):
    """The final state: a pod the oracle left pending has a failing stage at every NodePool under the limits the Solve
    left (a replay of the limits that erred would show here as a pod the ladder could still place)."""
    prob, res, ref, final, _ = corpus[seed]
    uns = np.nonzero(res.pod_result == abi.KP_POD_UNSCHEDULABLE)[0]
    assert len(uns) > 0
    for c, rq in shapes_of(prob, uns):
        for row in ref.rows(c, np.array(rq), final):
            assert row["reason"] is not None, (seed, c, row)


def test_seeds_are_not_vacuous(corpus):
    pairs, reasons, criteria, limits_by_solve = 0, set(), set(), 0
    for seed in SEEDS:
        prob, res, ref, final, _ = corpus[seed]
        uns = np.nonzero(res.pod_result == abi.KP_POD_UNSCHEDULABLE)[0]
        for c, rq in shapes_of(prob, uns):
            for row in ref.rows(c, np.array(rq), final):
                pairs += 1
                reasons.add(row["reason"])
                if row["reason"] == abi.KP_WHY_INSTANCE_TYPES:
                    criteria.add(row["criteria"])
                # a LIMITS row that the limits of the input would not give: the final-state dependence
                if row["reason"] == abi.KP_WHY_LIMITS and \
                        ref.explain(c, np.array(rq), row["nodepool"])["reason"] != abi.KP_WHY_LIMITS:
                    limits_by_solve += 1
    assert pairs >= 40, pairs
    wanted = {abi.KP_WHY_LIMITS, abi.KP_WHY_TAINTS, abi.KP_WHY_REQUIREMENTS, abi.KP_WHY_INSTANCE_TYPES,
              abi.KP_WHY_MIN_VALUES}
    assert len(reasons & wanted) >= 3, reasons
    assert len(criteria) >= 2, criteria
    assert limits_by_solve >= 1


HOSTNAME_CASES = [("In", ["node-7"], False), ("DoesNotExist", [], False), ("Gt", ["3"], False), ("Lt", ["3"], False),
                  ("NotIn", ["node-7"], True), ("Exists", [], True)]


@pytest.mark.parametrize("op,values,placed", HOSTNAME_CASES)
def test_hostname_requirement_against_the_placeholder(golden, op, values, placed):
    """A new NodeClaim carries kubernetes.io/hostname In [a fresh placeholder]: a pod's hostname In / DoesNotExist /
    Gt / Lt never meets it (core: incompatible requirements on that key), NotIn / Exists do.  Pinned to the oracle."""
    from kpsim import synth
    sub = catalog_of(golden)
    prob = model.Problem(sub, [synth.default_nodepool()],
                         [model.PodClass([model.Requirement(explain_ref.HOSTNAME, op, values)])],
                         synth.pods_from_specs([(0, {"cpu": "1"})]))
    row = explain_ref.Ref(prob).explain(0, prob.pods.requests[0], 0)
    got = one_pod_makes_nodeclaim(prob, model.CatalogView(sub), 0, prob.pods.requests[0], 0, None)
    assert got == placed == (row["reason"] is None), row
    if not placed:
        assert (row["reason"], row["key"]) == (abi.KP_WHY_REQUIREMENTS, explain_ref.HOSTNAME)


def test_algebra_corner_cases():
    R = explain_ref.Req
    assert R.new("k", "Gt", ["4"]).intersection(R.new("k", "Lt", ["4"])).operator() == "DoesNotExist"
    assert R.new("k", "Gt", ["4"]).has("5") and not R.new("k", "Gt", ["4"]).has("4") and not R.new("k", "Gt", ["4"]).has("x")
    assert R.new("k", "In", ["2", "8"]).intersection(R.new("k", "Gt", ["4"])).values == {"8"}
    assert R.new("k", "NotIn", ["a"]).intersection(R.new("k", "NotIn", ["b"])).values == {"a", "b"}
    a, b = explain_ref.Reqs(), explain_ref.Reqs()
    a.add(R.new("k", "DoesNotExist"))
    b.add(R.new("k", "NotIn", ["x"]))
    assert not explain_ref.intersect_failures(a, b)          # both NotIn / DoesNotExist: the exception
    b2 = explain_ref.Reqs()
    b2.add(R.new("k", "In", ["x"]))
    assert explain_ref.intersect_failures(a, b2) == ["k"]
    empty = explain_ref.Reqs()
    custom, known = explain_ref.Reqs(), explain_ref.Reqs()
    custom.add(R.new("example.com/team", "In", ["a"]))
    known.add(R.new(model.ZONE, "In", ["z"]))
    assert explain_ref.compatible_failures(empty, custom, True) == ["example.com/team"]
    assert not explain_ref.compatible_failures(empty, known, True)
    assert explain_ref.compatible_failures(empty, known, False) == [model.ZONE]


STUB_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import ctypes as C
import numpy as np
from kpsim import abi, catalog, model, native, synth
fake = catalog.fake_catalog(fx=catalog.load_fixtures())
ctx = native.Context(0)
ctx.upload_catalog(model.CatalogView(fake))
def status(f):
    try:
        f()
        return abi.KP_OK
    except native.KpError as e:
        return e.status
print("before any solve", status(lambda: ctx.explain()))
pools = [synth.default_nodepool(), synth.default_nodepool()]
pools[1].name, pools[1].weight = "heavy", 10
pods = synth.pods_from_specs([(0, {"cpu": "100m"})] * 3 + [(0, {"cpu": "200m"})] * 2)
prob = model.Problem(fake, pools, [model.PodClass()], pods)
iv = model.SolveInputView(prob)
ctx.prepare(iv)
print("prepared, not executed", status(lambda: ctx.explain()))
ctx.execute()          # the stand-in leaves every pod unschedulable and writes no reason
rows = ctx.explain()
print("rows", len(rows), rows["pod"].tolist(), rows["nodepool"].tolist(), sorted(set(rows["reason"].tolist())))
print("stats", ctx.explain_stats()[1])
print("listed", ctx.explain([4, 1, 4])["pod"].tolist(), ctx.explain_stats()[1])
print("out of range", status(lambda: ctx.explain([5])), status(lambda: ctx.explain([-1])))
need = C.c_int64(0)
buf = (abi.kp_pod_explanation * 4)()
print("small buffer", ctx.L.kp_solve_explain(ctx.h, 0, None, buf, 4, C.byref(need)), need.value)
print("key out of range", status(lambda: ctx.explain_key(10 ** 6)))
ctx.prepare(iv)
print("prepared again", status(lambda: ctx.explain()))
"""


def test_argument_handling_over_the_hip_stub():
    """kp_solve_explain's window and arguments need no kernel: KP_E_STATE before any solve and between a prepare and
    its execute, KP_E_INVALID for a pod index out of range, KP_E_BUFFER with the row count, rows grouped by pod with the
    NodePools in template order, a listed set of pods, and the evaluated pairs = distinct shapes x NodePools.  Run in a
    child process, which loads the host layer over the CPU stand-in instead of libkpsim.so."""
    here = os.path.dirname(os.path.abspath(__file__))
    stub = os.path.join(here, "cpu_stub")
    subprocess.check_call(["make", "-s", "-C", stub, "build/libkpsim_stub.so"], stdout=subprocess.DEVNULL)
    code = STUB_CHILD % (os.path.join(os.path.dirname(here), "karpenter-provider-aws_amd"), here)
    env = dict(os.environ, KPSIM_LIB=os.path.join(stub, "build", "libkpsim_stub.so"), KP_STUB_DEVICES="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.splitlines() == [
        "before any solve %d" % abi.KP_E_STATE,
        "prepared, not executed %d" % abi.KP_E_STATE,
        # template order: "heavy" (weight 10) is NodePool 1 of the input and comes first
        "rows 10 [0, 0, 1, 1, 2, 2, 3, 3, 4, 4] [1, 0, 1, 0, 1, 0, 1, 0, 1, 0] [%d]" % abi.KP_WHY_UNKNOWN,
        "stats [4, 2, 5]",
        "listed [1, 1, 4, 4] [4, 2, 2]",
        "out of range %d %d" % (abi.KP_E_INVALID, abi.KP_E_INVALID),
        "small buffer %d 10" % abi.KP_E_BUFFER,
        "key out of range %d" % abi.KP_E_INVALID,
        "prepared again %d" % abi.KP_E_STATE,
    ], r.stdout
