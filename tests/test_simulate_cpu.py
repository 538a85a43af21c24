"""CPU: the inputs of tests/test_gpu_simulate.py are not vacuous, shown on the oracle alone.

The device tests compare kp_simulate_* with tests/sim_ref.py, which solves each probe's reduced cluster on the CPU
oracle.  Here: the corpus reaches the cases the feature exists for (probes with 2 or more and 4 or more NodeClaims,
pods left unscheduled, a NodeClaim dropped at truncation, almost none past 12 NodeClaims), the helper's fold of
AllNonPendingPodsScheduled and its NodeClaim count equal pyoracle.consolidate's row wherever that row is not capped,
and the hand clusters give the NodeClaim counts the device tests state.
"""
import numpy as np
import pytest

import pyoracle
import sim_ref
from kpsim import abi

SINGLE, MULTI = sim_ref.SINGLE, sim_ref.MULTI


@pytest.fixture(scope="module")
def cat(golden):
    return golden[:200]


@pytest.fixture(scope="module")
def strict_refs(golden):
    """{name: (cp, {mode: [reference per probe]})} over the corpus under MIN_VALUES_POLICY=Strict, computed once"""
    out = {}
    for name, cp in sim_ref.corpus(golden, abi.KP_MIN_VALUES_STRICT):
        out[name] = (cp, {m: [sim_ref.reference(cp, m, i) for i in range(sim_ref.n_probes(cp, m))] for m in (SINGLE, MULTI)})
    return out


def test_corpus_is_not_vacuous(strict_refs):
    n2 = n4 = unsched = dropped = over = total = 0
    for cp, by_mode in strict_refs.values():
        for refs in by_mode.values():
            for ref in refs:
                total += 1
                n2 += ref["n_nodeclaims"] >= 2
                n4 += ref["n_nodeclaims"] >= 4
                over += ref["row"]["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW
                unsched += ref["row"]["n_unscheduled"] > 0
                dropped += ref["row"]["n_dropped"] > 0
    print("probes %d: >=2 NodeClaims %d, >=4 %d, unscheduled %d, dropped %d, overflow %d" %
          (total, n2, n4, unsched, dropped, over))
    assert n2 >= 30 and n4 >= 5 and unsched >= 5 and dropped >= 1
    assert over * 50 <= total  # at most 2 % of the rows may be the overflow


def test_helper_equals_orc_consolidate(strict_refs):
    """Every probe with at most one NodeClaim: the helper's all_scheduled and NodeClaim count are orc_consolidate's."""
    checked = 0
    for name, (cp, by_mode) in strict_refs.items():
        for mode, refs in by_mode.items():
            orc = pyoracle.consolidate(cp, mode)
            assert len(orc) == len(refs)
            for ref, o in zip(refs, orc):
                row = ref["row"]
                if row["status"] != abi.KP_SIM_OK:
                    continue
                assert min(row["n_new_nodeclaims"], 2) == o["n_new_nodeclaims"], name
                assert row["n_pods"] == o["n_pods"], name
                if row["n_new_nodeclaims"] <= 1:
                    assert row["all_scheduled"] == o["all_scheduled"], name
                    checked += 1
    assert checked > 100


def test_best_effort_overflow_share(golden):
    """The 2 % cap on rows past 12 NodeClaims holds under MIN_VALUES_POLICY=BestEffort too, and the drop case drops under
    Strict only where BestEffort relaxes."""
    over = total = 0
    for name, cp in sim_ref.corpus(golden, abi.KP_MIN_VALUES_BEST_EFFORT):
        for mode in (SINGLE, MULTI):
            for i in range(sim_ref.n_probes(cp, mode)):
                ref = sim_ref.reference(cp, mode, i)
                total += 1
                over += ref["row"]["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW
                if name == sim_ref.DROP_CASE:
                    assert ref["row"]["n_dropped"] == 0
    assert over * 50 <= total, (over, total)


def test_hand_cases(cat):
    r = sim_ref.reference(sim_ref.per_type_case(cat, 12), SINGLE, 0)
    assert r["row"] == dict(status=abi.KP_SIM_OK, all_scheduled=1, n_new_nodeclaims=12, n_dropped=0, n_pods=12,
                            n_unscheduled=0)
    assert sim_ref.reference(sim_ref.per_type_case(cat, 13), SINGLE, 0)["row"]["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW
    r = sim_ref.reference(sim_ref.slice_order_case(cat), SINGLE, 0)
    assert r["row"]["n_new_nodeclaims"] == 2 and r["row"]["all_scheduled"] == 1
    # the last pod (unconstrained) joins the NodeClaim with fewer pods: zone b's, created second
    assert sorted(r["results"].nodeclaim_n_pods.tolist()) == [2, 3] and int(r["results"].pod_result[4]) == 1
    cp = sim_ref.empty_candidate_case(cat)
    assert sim_ref.reference(cp, SINGLE, 0)["row"] == dict(status=abi.KP_SIM_OK, all_scheduled=1, n_new_nodeclaims=0,
                                                           n_dropped=0, n_pods=0, n_unscheduled=0)
    r = sim_ref.reference(sim_ref.pending_only_unscheduled_case(cat), SINGLE, 0)
    assert r["row"]["all_scheduled"] == 1 and r["row"]["n_unscheduled"] == 0 and int(r["results"].pod_result[0]) == -1
    r = sim_ref.reference(sim_ref.uninitialized_case(cat), SINGLE, 0)
    assert r["row"]["all_scheduled"] == 0 and r["row"]["n_unscheduled"] == 0 and int(r["results"].pod_result[0]) == -3
    assert sim_ref.reference(sim_ref.limit_case(cat, False), SINGLE, 0)["row"]["n_unscheduled"] == 1
    r = sim_ref.reference(sim_ref.limit_case(cat, True), SINGLE, 0)
    assert r["row"]["n_new_nodeclaims"] == 1 and r["row"]["all_scheduled"] == 1


def test_drift_cases(cat):
    cp = sim_ref.drift_case(cat)
    rows = sim_ref.rows(cp, SINGLE)
    assert rows["all_scheduled"].tolist() == [0, 1, 1, 1] and rows["n_new_nodeclaims"].tolist()[:2] == [0, 3]
    assert sim_ref.drift_replay(cp, rows) == (abi.KP_DRIFT_REPLACE, [1])
    cp = sim_ref.drift_case(cat, with_empty=True)
    assert sim_ref.drift_replay(cp, None) == (abi.KP_DRIFT_DELETE_EMPTY, [4])
    cp = sim_ref.drift_case(cat, movable=False)
    assert sim_ref.drift_replay(cp, sim_ref.rows(cp, SINGLE)) == (abi.KP_DRIFT_NONE, [])
