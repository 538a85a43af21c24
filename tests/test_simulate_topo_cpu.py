"""CPU: the reference and the inputs of tests/test_gpu_simulate_topo.py, shown on the oracle alone.

tests/sim_topo_ref.py solves each probe with its candidate nodes and every counted pod kept.  Here, over every probe of
its corpus (fuzz_topology_consolidation, 15 seeds plus 6 of them again with hostname pod affinity):

  * its rows equal pyoracle.consolidate's wherever that row is not capped, the uninitialized-node fold included;
  * no pod lands on a kept node;
  * at most 2 % of the rows are past 12 NodeClaims;
  * the corpus reaches the cases the feature exists for, with floors well under the counts this test prints: of 629
    probes 5 are past 12 NodeClaims; of the other 624, 257 create 2 or more NodeClaims, 137 create 4 or more, 52 create
    7 to 12, 43 schedule every non-pending pod, 185 place a pod of a class with topology terms on a new NodeClaim, and
    all 624 place pods on existing nodes.

Seeds 0, 1, 5, 9, 11, 18 and 22 of the draw are not in the corpus: 4 to 21 of their probes need more than 12 NodeClaims.
No seed was taken out for disagreeing with pyoracle.consolidate.

The hand clusters give the placements the device tests state, and solving them without their topology terms gives other
placements: topology decides.
"""
import numpy as np
import pytest

import pyoracle
import sim_ref
import sim_topo_ref as str_
from kpsim import abi, model

SINGLE, MULTI = sim_ref.SINGLE, sim_ref.MULTI
OK = abi.KP_SIM_OK


@pytest.fixture(scope="module")
def cat(golden):
    return golden[:200]


@pytest.fixture(scope="module")
def strict_refs(golden):
    """{name: (cp, {mode: [reference per probe]})} over the corpus under MIN_VALUES_POLICY=Strict, computed once"""
    out = {}
    for name, cp in str_.corpus(golden, abi.KP_MIN_VALUES_STRICT):
        out[name] = (cp, {m: [str_.reference(cp, m, i) for i in range(sim_ref.n_probes(cp, m))] for m in (SINGLE, MULTI)})
    return out


def test_reference_equals_orc_consolidate(strict_refs):
    """Zero disagreements on every probe: the NodeClaim count capped at 2, the pod count, and all_scheduled wherever at
    most one NodeClaim was created (orc_consolidate stops a probe at its second)."""
    checked = 0
    for name, (cp, by_mode) in strict_refs.items():
        for mode, refs in by_mode.items():
            orc = pyoracle.consolidate(cp, mode)
            assert len(orc) == len(refs)
            for i, (ref, o) in enumerate(zip(refs, orc)):
                row = ref["row"]
                if row["status"] != OK:
                    assert ref["n_nodeclaims"] > abi.KP_SIM_MAX_NODECLAIMS and o["n_new_nodeclaims"] == 2, (name, mode, i)
                    continue
                assert min(row["n_new_nodeclaims"], 2) == o["n_new_nodeclaims"], (name, mode, i)
                assert row["n_pods"] == o["n_pods"], (name, mode, i)
                if ref["n_nodeclaims"] <= 1:
                    assert row["all_scheduled"] == o["all_scheduled"], (name, mode, i)
                    checked += 1
    assert checked > 100


def test_no_pod_on_a_kept_node(strict_refs):
    for name, (cp, by_mode) in strict_refs.items():
        for mode, refs in by_mode.items():
            for i, ref in enumerate(refs):
                assert str_.on_kept_node(cp, mode, i, ref) == [], (name, mode, i)


def test_corpus_is_not_vacuous(strict_refs):
    total = over = n2 = n4 = n7 = sched = topo_nc = on_nodes = 0
    for cp, by_mode in strict_refs.values():
        for refs in by_mode.values():
            for ref in refs:
                total += 1
                if ref["row"]["status"] != OK:
                    over += 1
                    continue
                n = ref["n_nodeclaims"]
                n2 += n >= 2
                n4 += n >= 4
                n7 += 7 <= n <= 12
                sched += ref["row"]["all_scheduled"] == 1 and ref["row"]["n_unscheduled"] == 0
                topo_nc += bool(str_.topo_pod_on_nodeclaim(cp, ref))
                on_nodes += bool((np.asarray(ref["results"].pod_result) <= -2).any())
    print("probes %d: overflow %d, >=2 NodeClaims %d, >=4 %d, 7..12 %d, all scheduled %d, topology pod on a NodeClaim %d, "
          "pods on existing nodes %d" % (total, over, n2, n4, n7, sched, topo_nc, on_nodes))
    assert total >= 600
    assert over * 50 <= total  # at most 2 % of the rows may be the overflow
    assert n2 >= 100 and n4 >= 50 and n7 >= 20 and sched >= 20
    assert topo_nc >= 60 and on_nodes >= 300


def test_best_effort_overflow_share(golden):
    over = total = 0
    for name, cp in str_.corpus(golden, abi.KP_MIN_VALUES_BEST_EFFORT):
        for mode in (SINGLE, MULTI):
            for i in range(sim_ref.n_probes(cp, mode)):
                total += 1
                over += str_.reference(cp, mode, i)["row"]["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW
    assert over * 50 <= total, (over, total)


def _placements(ref):
    return np.asarray(ref["results"].pod_result).tolist()


def test_zonal_spread_case(cat):
    cp = str_.zonal_spread_case(cat)
    ref = str_.reference(cp, SINGLE, 0)
    assert ref["row"] == dict(status=OK, all_scheduled=1, n_new_nodeclaims=3, n_dropped=0, n_pods=3, n_unscheduled=0)
    zones = str_.nodeclaim_zones(ref)
    assert all(z is not None and len(z) == 1 for z in zones) and len(set(zones)) == 3
    plain = str_.reference(str_.without_topology(cp), SINGLE, 0)  # topology decides: one NodeClaim takes all three
    assert plain["n_nodeclaims"] == 1 and _placements(plain) != _placements(ref)


@pytest.mark.parametrize("n", [12, 13])
def test_hostname_anti_case(cat, n):
    cp = str_.hostname_anti_case(cat, n)
    ref = str_.reference(cp, SINGLE, 0)
    assert ref["n_nodeclaims"] == n
    if n == 12:
        assert ref["row"] == dict(status=OK, all_scheduled=1, n_new_nodeclaims=12, n_dropped=0, n_pods=12, n_unscheduled=0)
        assert sorted(_placements(ref)) == list(range(12))
    else:
        assert ref["row"]["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW
    assert str_.reference(str_.without_topology(cp), SINGLE, 0)["n_nodeclaims"] < n


def test_truncation_drop_case(cat):
    cp = str_.truncation_drop_case(cat)
    ref = str_.reference(cp, SINGLE, 0)
    assert ref["n_nodeclaims"] == 2
    assert ref["row"] == dict(status=OK, all_scheduled=0, n_new_nodeclaims=0, n_dropped=2, n_pods=2, n_unscheduled=2)
    o = pyoracle.consolidate(cp, SINGLE)[0]  # the comparison of test_reference_equals_orc_consolidate
    assert min(ref["row"]["n_new_nodeclaims"], 2) == o["n_new_nodeclaims"] == 0 and o["n_pods"] == 2
    assert o["all_scheduled"] == 0
    plain = str_.reference(str_.without_topology(cp), SINGLE, 0)  # one NodeClaim takes both pods (and is dropped alike)
    assert plain["n_nodeclaims"] == 1 and plain["row"]["n_dropped"] == 1


def test_hostname_spread_case(cat):
    cp = str_.hostname_spread_case(cat)
    ref = str_.reference(cp, SINGLE, 0)
    res = _placements(ref)
    assert sorted(res) == [-3, 0, 1, 2]  # node n1 once, three NodeClaims of one pod
    assert np.asarray(ref["results"].nodeclaim_n_pods[:3]).tolist() == [1, 1, 1]
    assert _placements(str_.reference(str_.without_topology(cp), SINGLE, 0)) == [-3] * 4


def test_kept_node_affinity_case(cat):
    cp = str_.kept_node_affinity_case(cat)
    ref = str_.reference(cp, SINGLE, 0)
    z0 = cp.cluster.existing[0].labels[model.ZONE]
    assert _placements(ref) == [0] and str_.nodeclaim_zones(ref) == [(z0,)]
    # the reduced cluster of sim_ref, which drops node n0 and the pod bound to it, has no `db` pod: no place
    assert _placements(sim_ref.reference(cp, SINGLE, 0)) == [-1]
    assert _placements(str_.reference(str_.without_topology(cp), SINGLE, 0)) == [-3]
    assert pyoracle.consolidate(cp, SINGLE)[0]["all_scheduled"] == 1


def test_inverse_anti_case(cat):
    cp = str_.inverse_anti_case(cat)
    assert _placements(str_.reference(cp, SINGLE, 0)) == [-4]  # node n2
    assert _placements(str_.reference(str_.without_topology(cp), SINGLE, 0)) == [-3]  # node n1


def test_drift_spread_case(cat):
    cp = str_.drift_spread_case(cat)
    refs = [str_.reference(cp, SINGLE, i) for i in range(3)]
    assert [r["row"]["all_scheduled"] for r in refs] == [0, 1, 0] and refs[1]["n_nodeclaims"] == 1
    assert str_.nodeclaim_zones(refs[1]) == [(str_._zones(cp.cluster.catalog[sim_ref.small_type(cp.cluster.catalog)])[1],)]
    assert sim_ref.drift_replay(cp, sim_ref.rows(cp, SINGLE, refs)) == (abi.KP_DRIFT_REPLACE, [1])
    orc = pyoracle.consolidate(cp, SINGLE)
    assert orc["all_scheduled"].tolist() == [0, 1, 0] and orc["n_new_nodeclaims"].tolist() == [0, 1, 0]
    plain = str_.without_topology(cp)  # without the spread every candidate's pod gets a NodeClaim: drift takes the first
    assert [str_.reference(plain, SINGLE, i)["row"]["all_scheduled"] for i in range(3)] == [1, 1, 1]
    cp = str_.drift_spread_case(cat, movable=False)
    refs = [str_.reference(cp, SINGLE, i) for i in range(3)]
    assert sim_ref.drift_replay(cp, sim_ref.rows(cp, SINGLE, refs)) == (abi.KP_DRIFT_NONE, [])


def test_drift_case(cat):
    cp = str_.drift_case(cat)
    refs = [str_.reference(cp, SINGLE, i) for i in range(3)]
    assert [r["row"]["all_scheduled"] for r in refs] == [0, 1, 0] and refs[1]["n_nodeclaims"] == 2
    assert sim_ref.drift_replay(cp, sim_ref.rows(cp, SINGLE, refs)) == (abi.KP_DRIFT_REPLACE, [1])
    cp = str_.drift_case(cat, movable=False)
    refs = [str_.reference(cp, SINGLE, i) for i in range(3)]
    assert sim_ref.drift_replay(cp, sim_ref.rows(cp, SINGLE, refs)) == (abi.KP_DRIFT_NONE, [])
