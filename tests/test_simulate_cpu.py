"""CPU: the inputs of tests/test_gpu_simulate.py are not vacuous, shown on the oracle alone.

The device tests compare kp_simulate_* with tests/sim_ref.py, which solves each probe's reduced cluster on the CPU
oracle.  Here: the corpus reaches the cases the feature exists for (probes with 2 or more and 4 or more NodeClaims,
pods left unscheduled, a NodeClaim dropped at truncation, almost none past 12 NodeClaims), the helper's fold of
AllNonPendingPodsScheduled and its NodeClaim count equal pyoracle.consolidate's row wherever that row is not capped,
and the hand clusters give the NodeClaim counts the device tests state.  The probe lists the device tests run in several
batches have the NodeClaim counts those tests rely on; the ladder clusters' placements follow from the slice order alone
and from nothing simpler; the cluster of more than 4096 pods queues pods from both sides of the bitmap's 64th word.
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


# ------------------------------------------------------------------------------------------------
# the probe lists of test_gpu_simulate.py::test_batches: per-probe NodeClaim counts, pinned so that a drift of the
# generators is noticed ("O": past 12 NodeClaims; (created, dropped) where TruncateInstanceTypes drops some)
# ------------------------------------------------------------------------------------------------
BATCH_LISTS = {
    ("fuzz5", MULTI): [4, 7, 7, 9, 11, "O", "O"],
    ("fuzz9", MULTI): [7, 7, 7, 12, "O"],
    ("min126", MULTI): [0, (1, 1), (8, 7), (9, 8)],
    ("min6", SINGLE): [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 1, 0, 0, 0],
}


def _count(ref):
    if ref["row"]["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW:
        return "O"
    d = ref["row"]["n_dropped"]
    return (ref["n_nodeclaims"], d) if d else ref["n_nodeclaims"]


def test_batch_lists(strict_refs):
    for (name, mode), want in BATCH_LISTS.items():
        got = [_count(r) for r in strict_refs[name][1][mode]]
        print(name, "MULTI" if mode == MULTI else "SINGLE", got)
        assert got == want, (name, mode)
    multi = [r["n_nodeclaims"] for r in strict_refs["fuzz4"][1][MULTI]]
    print("fuzz4 MULTI", multi)
    assert len(multi) == 22 and multi[0] == 2 and multi[-1] == 8 and multi == sorted(multi)
    assert len(strict_refs["fuzz4"][1][SINGLE]) == 23
    # what the caps of test_batches rest on: a last batch of overflow rows alone (fuzz5, caps 1 and 2), an overflow row
    # beside a full one (fuzz9, cap 2), dropped NodeClaims past the first batch (min126, cap 2), a first batch with
    # nothing to finalize (min6, cap 5)


def test_slice_sort_corpus_share(strict_refs):
    """The corpus alone barely checks the slice sort past six elements: the rows with 7 to 12 NodeClaims, and how many of
    them end with a slice order other than creation order."""
    n = moved = 0
    for cp, by_mode in strict_refs.values():
        for refs in by_mode.values():
            for ref in refs:
                if ref["row"]["status"] == abi.KP_SIM_OK and 7 <= ref["n_nodeclaims"] <= 12:
                    n += 1
                    pos = np.asarray(ref["results"].nodeclaim_slice_pos[:ref["n_nodeclaims"]]).tolist()
                    moved += pos != list(range(len(pos)))
    print("rows with 7 to 12 NodeClaims: %d, with a non-identity slice order: %d" % (n, moved))
    assert n >= 10 and moved >= 5


# ------------------------------------------------------------------------------------------------
# ladder cases: the slice model alone, replayed in a few lines, decides where the floaters go
# ------------------------------------------------------------------------------------------------
def _slice_replay(order, lists, key=None, by_id=False):
    """Where each pod goes if only the slice matters.  order: the pods in queue order; lists[pod]: the groups (types) it
    may join.  Before each pod the slice is stable-sorted by pod count as the last sort left it (key(count, id): another
    sort key); the pod joins the first NodeClaim of the slice (by_id: in id order) whose group it lists, else it opens
    a NodeClaim of its first group.  -> {pod: NodeClaim id}"""
    key = key or (lambda cnt, i: cnt)
    sl, count, group, dest = [], {}, {}, {}
    for p in order:
        sl = sorted(sl, key=lambda i: key(count[i], i))
        for i in (sorted(sl) if by_id else sl):
            if group[i] in lists[p]:
                break
        else:
            i = len(sl)
            sl.append(i)
            count[i], group[i] = 0, lists[p][0]
        count[i] += 1
        dest[p] = i
    return dest, sl


@pytest.mark.parametrize("name", list(sim_ref.LADDERS))
def test_ladder_cases(cat, name):
    import cons_explain_ref as cxr
    counts = sim_ref.LADDERS[name]
    n = len(counts)
    cp, types, floaters = sim_ref.ladder_case(cat, counts)
    ref = sim_ref.reference(cp, SINGLE, 0)
    npods = cp.cluster.pods.n
    assert ref["row"] == dict(status=abi.KP_SIM_OK, all_scheduled=1, n_new_nodeclaims=n, n_dropped=0, n_pods=npods,
                              n_unscheduled=0)
    res = ref["results"]
    pos = np.asarray(res.nodeclaim_slice_pos[:n]).tolist()
    assert sorted(pos) == list(range(n)) and pos != list(range(n))
    # NodeClaim ids are creation order: map them to groups through the single type each base pod selects
    lists = {p: [int(cp.cluster.pods.class_id[p])] for p in range(npods - len(floaters))}
    lists.update(dict(floaters))
    order = sorted(range(npods), key=lambda p: cxr.queue_key(cp.cluster, p))
    assert set(order[-len(floaters):]) == {p for p, _ in floaters}  # the floaters are popped after every base pod
    assert np.asarray(res.pod_order)[np.array(order)].tolist() == list(range(npods))
    got = {p: int(res.pod_result[p]) for p, _ in floaters}
    dest, sl = _slice_replay(order, lists)
    assert {p: dest[p] for p in got} == got
    assert [sl.index(i) for i in range(n)] == pos  # the slice as the last sort left it
    group_of = {dest[p]: lists[p][0] for p in range(npods - len(floaters))}
    assert sorted(group_of.values()) == list(range(n))
    # a sort that breaks ties by NodeClaim id, and a scan in id order, send floaters elsewhere
    by_tie, _ = _slice_replay(order, lists, key=lambda cnt, i: (cnt, i))
    by_id, _ = _slice_replay(order, lists, by_id=True)
    d_tie = sum(by_tie[p] != got[p] for p in got)
    d_id = sum(by_id[p] != got[p] for p in got)
    off_lowest = sum(got[p] != min(i for i, g in group_of.items() if g in gl) for p, gl in floaters)
    print("%s: slice order %s, floaters off the lowest-id NodeClaim they list %d of %d, tie-by-id replay differs in %d, "
          "id-order replay in %d" % (name, pos, off_lowest, len(floaters), d_tie, d_id))
    assert d_tie >= 1 and d_id >= 4


# ------------------------------------------------------------------------------------------------
# the queue bitmap past 4096 pods
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sim_ref.BITMAP_SEEDS)
def test_bitmap_block_case(cat, seed):
    cp, rank = sim_ref.bitmap_block_case(cat, seed)
    P = cp.cluster.pods.n
    assert P > 4096 + 64 and len(cp.candidates) == 4
    owned = sorted(int(rank[p]) for c in cp.candidates for p in c.pods)
    assert set(r % P for r in sim_ref.BITMAP_CAND_RANKS) <= set(owned) and len(owned) == len(set(owned))
    assert sorted(int(rank[p]) for p in cp.pending) == sim_ref.BITMAP_PEND_RANKS
    many = on_node = 0
    for mode in (SINGLE, MULTI):
        for i in range(sim_ref.n_probes(cp, mode)):
            ref = sim_ref.reference(cp, mode, i)
            assert ref["row"]["status"] == abi.KP_SIM_OK
            many += ref["n_nodeclaims"] >= 2
            on_node += bool((np.asarray(ref["results"].pod_result) <= -2).any())
            ranks = [int(rank[p]) for p in ref["pods"][len(cp.pending):]]
            if mode == MULTI:
                assert min(ranks) < 4096 <= max(ranks)
            print("bitmap case, mode %d probe %d: %d pods, %d NodeClaims, %d on nodes, %d unscheduled" %
                  (mode, i, len(ref["pods"]), ref["n_nodeclaims"],
                   int((np.asarray(ref["results"].pod_result) <= -2).sum()), ref["row"]["n_unscheduled"]))
    assert many >= 1 and on_node >= 1
