"""GPU: kp_simulate_* — SimulateScheduling's Results of a probe with up to 12 new NodeClaims, drift's command and
ValidateCommand's verdict over them.

The reference of a probe is the CPU oracle's Solve of its reduced cluster (tests/sim_ref.py; tests/test_simulate_cpu.py
shows on the oracle alone that the corpus reaches the cases that matter).  Rows are compared field by field, the
NodeClaims, placements and requirements of a probe with tests/parity.py::assert_same.
"""
import dataclasses

import numpy as np
import pytest

import cons_explain_ref as cxr
import edge_cases
import fuzzgen
import parity
import sim_ref
from kpsim import abi, consolidation, model, native, synth
from kpsim.model import ZONE, HostPort, PodClass, Requirement

pytestmark = pytest.mark.gpu

SINGLE, MULTI = sim_ref.SINGLE, sim_ref.MULTI
STRICT, BEST_EFFORT = abi.KP_MIN_VALUES_STRICT, abi.KP_MIN_VALUES_BEST_EFFORT
CORPUS = ["fuzz%d" % s for s in sim_ref.FUZZ_SEEDS] + ["min%d" % s for s in sim_ref.MIN_SEEDS]


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cat(golden):
    return golden[:200]


@pytest.fixture(scope="module")
def corpora(golden):
    return {pol: dict(sim_ref.corpus(golden, pol)) for pol in (STRICT, BEST_EFFORT)}


def prepare(ctx, cp, s2s=False):
    ctx.upload_catalog(model.CatalogView(cp.cluster.catalog))
    ctx.consolidate_prepare(model.ConsolidateInputView(cp, SINGLE, spot_to_spot=s2s))


def check_probe(ctx, cp, mode, i, ref=None):
    """kp_simulate_nodeclaims of one probe against its reference: row, pod list, Results and requirements."""
    ref = ref or sim_ref.reference(cp, mode, i)
    row, pods, res, reqs = ctx.simulate_nodeclaims(mode, i)
    assert row == ref["row"], (mode, i, row, ref["row"])
    if row["status"] != abi.KP_SIM_OK:
        assert len(pods) == 0 and res.n_nodeclaims == 0
        return ref
    assert pods.tolist() == ref["pods"]
    parity.assert_same((res, reqs), (ref["results"], ref["reqs"]))
    return ref


_REFS = {}


def cached_ref(key, cp, mode, i):
    """sim_ref.reference(cp, mode, i), computed once per module for the cluster named `key` (name and whatever else
    tells it from the others: the minValues policy, a seed); nothing changes a cached reference."""
    k = (key, mode, i)
    if k not in _REFS:
        _REFS[k] = sim_ref.reference(cp, mode, i)
    return _REFS[k]


def cached_refs(key, cp, mode):
    return [cached_ref(key, cp, mode, i) for i in range(sim_ref.n_probes(cp, mode))]


def batch_cap(monkeypatch, cap):
    """KPSIM_SIM_BATCH for the calls that follow (the host reads it on every call); None: unset"""
    if cap is None:
        monkeypatch.delenv("KPSIM_SIM_BATCH", raising=False)
    else:
        monkeypatch.setenv("KPSIM_SIM_BATCH", str(cap))


def check_pass(ctx, cp, every=3, key=None):
    """Both probe lists of a prepared pass: every row, and the Results of every probe with 2 or more NodeClaims and of
    every `every`-th other one.  key: the cluster's name in the reference cache, if it has one."""
    n_over = n_rows = 0
    for mode in (SINGLE, MULTI):
        n = sim_ref.n_probes(cp, mode)
        refs = cached_refs(key, cp, mode) if key else [sim_ref.reference(cp, mode, i) for i in range(n)]
        dev = ctx.simulate_execute(mode, n)
        sim_ref.assert_rows_equal(dev, sim_ref.rows(cp, mode, refs))
        for i, ref in enumerate(refs):
            if ref["n_nodeclaims"] >= 2 or i % every == 0:
                check_probe(ctx, cp, mode, i, ref)
        n_over += int((dev["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW).sum())
        n_rows += n
    return n_over, n_rows


# ------------------------------------------------------------------------------------------------
# fuzz: every row and the Results behind them, both minValues policies, both probe lists
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [STRICT, BEST_EFFORT])
@pytest.mark.parametrize("name", CORPUS)
def test_fuzz(ctx, corpora, name, policy):
    cp = corpora[policy][name]
    prepare(ctx, cp)
    check_pass(ctx, cp, key=(name, policy))


def test_fuzz_overflow_share(ctx, corpora):
    """Rows past 12 NodeClaims are the only ones test_fuzz cannot compare in full (it checks that they are exactly the
    reference's): at most 2 % of the corpus' rows, and no row is a probe the kernel does not cover."""
    over = rows = 0
    for pol in (STRICT, BEST_EFFORT):
        for name in CORPUS:
            cp = corpora[pol][name]
            prepare(ctx, cp)
            for mode in (SINGLE, MULTI):
                dev = ctx.simulate_execute(mode, sim_ref.n_probes(cp, mode))
                assert not (dev["status"] == abi.KP_SIM_UNSUPPORTED_PROBE).any()
                over += int((dev["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW).sum())
                rows += len(dev)
    assert over * 50 <= rows, (over, rows)


@pytest.mark.parametrize("name", ["fuzz1", "fuzz4", "fuzz5", "fuzz9", "min2", sim_ref.DROP_CASE])
def test_consistent_with_the_consolidation_pass(ctx, corpora, name):
    """kp_consolidate_execute's rows agree with the sim rows wherever fewer than two NodeClaims were created, report 2
    exactly where the simulation created two or more (or overflowed), and are the same before and after."""
    cp = corpora[STRICT][name]
    prepare(ctx, cp)
    for mode in (SINGLE, MULTI):
        n = sim_ref.n_probes(cp, mode)
        before = ctx.consolidate_execute(mode, n)
        stats = ctx.consolidate_stats()
        sim = ctx.simulate_execute(mode, n)
        for i in range(0, n, 4):
            ctx.simulate_nodeclaims(mode, i)
        assert ctx.consolidate_stats() == stats
        after = ctx.consolidate_execute(mode, n)
        assert before.tobytes() == after.tobytes()
        for r, s in zip(before, sim):
            assert s["status"] in (abi.KP_SIM_OK, abi.KP_SIM_NODECLAIM_OVERFLOW)
            created = s["n_new_nodeclaims"] + s["n_dropped"]
            many = s["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW or created >= 2
            assert (r["n_new_nodeclaims"] == 2) == many
            if not many:
                assert r["all_scheduled"] == s["all_scheduled"] and r["n_pods"] == s["n_pods"]
                # (a probe that left pods unscheduled counts its one NodeClaim before truncation: DESIGN §1 known gap)
                assert r["n_new_nodeclaims"] == s["n_new_nodeclaims"] or \
                    (s["n_dropped"] == 1 and not s["all_scheduled"] and r["n_new_nodeclaims"] == 1)


# ------------------------------------------------------------------------------------------------
# hand cases
# ------------------------------------------------------------------------------------------------
def test_twelve_nodeclaims_and_the_overflow(ctx, cat):
    cp = sim_ref.per_type_case(cat, 12)
    prepare(ctx, cp)
    row = ctx.simulate_execute(SINGLE, 1)[0]
    assert (row["status"], row["all_scheduled"], row["n_new_nodeclaims"], row["n_pods"]) == (abi.KP_SIM_OK, 1, 12, 12)
    ref = check_probe(ctx, cp, SINGLE, 0)
    assert ref["results"].n_nodeclaims == 12
    assert ctx.consolidate_execute(SINGLE, 1)[0]["n_new_nodeclaims"] == 2  # the consolidation row still caps at 2
    cp = sim_ref.per_type_case(cat, 13)
    prepare(ctx, cp)
    row = ctx.simulate_execute(SINGLE, 1)[0]
    assert row["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW
    assert [int(row[f]) for f in sim_ref.ROW_FIELDS[1:]] == [0] * 5
    check_probe(ctx, cp, SINGLE, 0)
    assert ctx.simulate_stats()[1][4] == 1


def test_slice_order_decides(ctx, cat):
    cp = sim_ref.slice_order_case(cat)
    prepare(ctx, cp)
    ref = check_probe(ctx, cp, SINGLE, 0)
    row, pods, res, _ = ctx.simulate_nodeclaims(SINGLE, 0)
    assert row["n_new_nodeclaims"] == 2 and sorted(res.nodeclaim_n_pods.tolist()) == [2, 3]
    assert int(res.pod_result[4]) == 1 == int(ref["results"].pod_result[4])  # the NodeClaim with fewer pods comes first


@pytest.mark.parametrize("case", ["empty_candidate_case", "pending_only_unscheduled_case", "uninitialized_case"])
def test_hand_case(ctx, cat, case):
    cp = getattr(sim_ref, case)(cat)
    prepare(ctx, cp)
    for mode in (SINGLE, MULTI):
        for i in range(sim_ref.n_probes(cp, mode)):
            check_probe(ctx, cp, mode, i)
    row = ctx.simulate_execute(SINGLE, len(cp.candidates))[0]
    if case == "empty_candidate_case":
        assert (row["status"], row["all_scheduled"], row["n_pods"], row["n_new_nodeclaims"]) == (0, 1, 0, 0)
    elif case == "pending_only_unscheduled_case":
        assert (row["all_scheduled"], row["n_unscheduled"], row["n_pods"]) == (1, 0, 2)
    else:
        assert (row["all_scheduled"], row["n_unscheduled"]) == (0, 0)


@pytest.mark.parametrize("returned", [False, True])
def test_limit_lifted_by_the_returned_capacity(ctx, cat, returned):
    cp = sim_ref.limit_case(cat, returned)
    prepare(ctx, cp)
    ref = check_probe(ctx, cp, SINGLE, 0)
    assert ref["row"]["n_new_nodeclaims"] == (1 if returned else 0)
    assert ref["row"]["n_unscheduled"] == (0 if returned else 1)


# ------------------------------------------------------------------------------------------------
# edges of the 64-lane words
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [63, 64, 65, 129])
def test_node_word_edges(ctx, cat, E):
    cp = fuzzgen.fuzz_consolidation(cat, 7100 + E, n_nodes=E, n_pods=90, n_candidates=4)
    assert len(cp.cluster.existing) == E
    want = [j for j in (0, 63, 64, E - 1) if j < E]
    want = list(dict.fromkeys(want))
    for c, j in zip(cp.candidates, want):
        c.node = j
    cp.candidates = cp.candidates[:len(want)]
    owned = {int(p) for c in cp.candidates for p in c.pods} | {int(p) for p in cp.pending}
    assert len({c.node for c in cp.candidates}) == len(cp.candidates) and len(owned) > 20
    prepare(ctx, cp)
    check_pass(ctx, cp, every=1)


@pytest.mark.parametrize("T", [64, 65, 129])
def test_type_word_edges(ctx, golden, T):
    cp = fuzzgen.fuzz_consolidation(golden[:T], 7200 + T, n_nodes=12, n_pods=80)
    prepare(ctx, cp)
    check_pass(ctx, cp, every=1)


def test_wide_axes(ctx, cat):
    rng = np.random.Generator(np.random.PCG64(7300))
    cp = fuzzgen.fuzz_consolidation(cat, 7300, n_nodes=20, n_pods=120)
    fuzzgen.add_extra_resources(rng, cp.cluster)
    assert (cp.cluster.pods.requests != 0).any(0).sum() >= 7
    prepare(ctx, cp)
    check_pass(ctx, cp, every=1)


def test_63_nodepools(ctx, cat):
    cp = fuzzgen.fuzz_consolidation(cat, 7400, n_nodes=20, n_pods=120, n_pools=63)
    assert len(cp.cluster.nodepools) == 63
    prepare(ctx, cp)
    check_pass(ctx, cp, every=1)


# ------------------------------------------------------------------------------------------------
# drift
# ------------------------------------------------------------------------------------------------
def test_drift_replaces_the_first_movable_candidate(ctx, cat):
    cp = sim_ref.drift_case(cat)
    prepare(ctx, cp)
    cmd = ctx.drift_command()
    assert (cmd["decision"], cmd["candidates"], cmd["n_nodeclaims"]) == (abi.KP_DRIFT_REPLACE, [1], 3)
    assert ctx.simulate_stats()[1][3] == 4  # one pass over the four single-node probes
    ref = check_probe(ctx, cp, SINGLE, 1)
    assert ref["results"].n_nodeclaims == 3 and cmd["row"] == ref["row"]


def test_drift_empty_candidates_need_no_simulation(ctx, cat):
    cp = sim_ref.drift_case(cat, with_empty=True)
    prepare(ctx, cp)
    cmd = ctx.drift_command()
    assert (cmd["decision"], cmd["candidates"], cmd["n_nodeclaims"]) == (abi.KP_DRIFT_DELETE_EMPTY, [4], 0)
    assert ctx.simulate_stats()[1] == [0] * 7  # nothing was simulated


def test_drift_nothing_can_move(ctx, cat):
    cp = sim_ref.drift_case(cat, movable=False)
    prepare(ctx, cp)
    cmd = ctx.drift_command()
    assert (cmd["decision"], cmd["candidates"]) == (abi.KP_DRIFT_NONE, [])


@pytest.mark.parametrize("name", ["fuzz1", "fuzz3", "fuzz5", "fuzz6", "fuzz8", "fuzz9"])
def test_drift_fuzz(ctx, corpora, name):
    cp = corpora[STRICT][name]
    prepare(ctx, cp)
    cmd = ctx.drift_command()
    refs = cached_refs((name, STRICT), cp, SINGLE)
    rows = sim_ref.rows(cp, SINGLE, refs)
    decision, cands = sim_ref.drift_replay(cp, rows)
    assert (cmd["decision"], cmd["candidates"]) == (decision, cands)
    if decision == abi.KP_DRIFT_REPLACE:
        assert cmd["n_nodeclaims"] == rows[cands[0]]["n_new_nodeclaims"]
        check_probe(ctx, cp, SINGLE, cands[0], refs[cands[0]])


# ------------------------------------------------------------------------------------------------
# validation
# ------------------------------------------------------------------------------------------------
def test_validate_verdicts(ctx, cat):
    V = abi
    cp = sim_ref.empty_candidate_case(cat)  # probe 1: the pod fits node n0's twin, no NodeClaim
    prepare(ctx, cp)
    assert ctx.consolidate_validate(SINGLE, 1, False) == V.KP_VALIDATE_VALID
    assert ctx.consolidate_validate(SINGLE, 1, True, [0]) == V.KP_VALIDATE_NO_NODECLAIM
    cp = sim_ref.limit_case(cat, False)
    prepare(ctx, cp)
    assert ctx.consolidate_validate(SINGLE, 0, True, [0]) == V.KP_VALIDATE_PODS_UNSCHEDULABLE
    cp = sim_ref.per_type_case(cat, 2)
    prepare(ctx, cp)
    assert ctx.consolidate_validate(SINGLE, 0, True, [0]) == V.KP_VALIDATE_MULTIPLE_NODECLAIMS
    cp = sim_ref.limit_case(cat, True)
    prepare(ctx, cp)
    ref = sim_ref.reference(cp, SINGLE, 0)
    types = ref["results"].nodeclaim_types[0]
    outside = next(t for t in range(len(cat)) if t not in types)
    assert ctx.consolidate_validate(SINGLE, 0, False) == V.KP_VALIDATE_NEEDS_NODECLAIM
    assert ctx.consolidate_validate(SINGLE, 0, True, types[:3]) == V.KP_VALIDATE_VALID
    assert ctx.consolidate_validate(SINGLE, 0, True, types[:3] + [outside]) == V.KP_VALIDATE_NOT_SUBSET
    for had, ids in ((False, []), (True, types[:3]), (True, [outside])):
        assert ctx.consolidate_validate(SINGLE, 0, had, ids) == sim_ref.validate(ref, had, ids)


def _replace_command(ctx, corpora):
    for name in CORPUS:
        cp, s2s = corpora[STRICT][name], False
        prepare(ctx, cp, s2s)
        cmd = ctx.consolidate_command(SINGLE)
        if cmd.decision == abi.KP_DECISION_REPLACE and len(cmd.type_ids) > 1:
            return cp, cmd
    raise AssertionError("no REPLACE command in the corpus")


def test_validate_round_trip(ctx, corpora):
    """A REPLACE command validates against its own pass (the price-filtered list is within the truncated list), and after
    an availability patch that takes its cheapest option away the verdict is the reference's."""
    cp, cmd = _replace_command(ctx, corpora)
    assert consolidation.validate_command(ctx, cmd) == abi.KP_VALIDATE_VALID
    assert sim_ref.validate(sim_ref.reference(cp, cmd.mode, cmd.probe), True, cmd.type_ids) == abi.KP_VALIDATE_VALID
    catalog = cp.cluster.catalog
    avail = edge_cases.availability(catalog)
    row = 0
    for t, it in enumerate(catalog):
        for _ in it.offerings:
            if t == cmd.type_ids[0]:
                avail[row] = 0
            row += 1
    ctx.patch_avail(avail, 2)
    ctx.consolidate_prepare(model.ConsolidateInputView(cp, SINGLE))
    cp2 = dataclasses.replace(cp, cluster=dataclasses.replace(cp.cluster, catalog=edge_cases.apply_patches(catalog, avail)))
    want = sim_ref.validate(sim_ref.reference(cp2, cmd.mode, cmd.probe), True, cmd.type_ids)
    assert consolidation.validate_command(ctx, cmd) == want
    assert want != abi.KP_VALIDATE_VALID  # the command's cheapest type is gone from every re-simulated list


# ------------------------------------------------------------------------------------------------
# contract
# ------------------------------------------------------------------------------------------------
def _raises(status, fn, *a):
    with pytest.raises(native.KpError) as e:
        fn(*a)
    assert e.value.status == status, e.value
    return str(e.value)


def test_state_errors(cat):
    c = native.Context(0)
    try:
        cp = sim_ref.limit_case(cat, True)
        c.upload_catalog(model.CatalogView(cat))
        for fn, a in ((c.simulate_execute, (SINGLE, 1)), (c.simulate_nodeclaims, (SINGLE, 0)), (c.drift_command, ()),
                      (c.consolidate_validate, (SINGLE, 0, False))):
            _raises(abi.KP_E_STATE, fn, *a)
        c.consolidate_prepare(model.ConsolidateInputView(cp, SINGLE))
        assert c.simulate_execute(SINGLE, 1)[0]["status"] == abi.KP_SIM_OK
        c.prepare(model.SolveInputView(cp.cluster))
        _raises(abi.KP_E_STATE, c.simulate_execute, SINGLE, 1)
        _raises(abi.KP_E_STATE, c.drift_command)
    finally:
        c.close()


def test_pass_wide_refusals(cat, golden):
    c = native.Context(0)
    try:
        cp = fuzzgen.fuzz_topology_consolidation(cat, 7500, n_nodes=10, n_pods=40)
        c.upload_catalog(model.CatalogView(cp.cluster.catalog))
        c.consolidate_prepare(model.ConsolidateInputView(cp, SINGLE))
        for fn, a in ((c.simulate_execute, (SINGLE, 1)), (c.drift_command, ()), (c.consolidate_validate, (SINGLE, 0, False))):
            assert "topology" in _raises(abi.KP_E_UNSUPPORTED, fn, *a)
        cp = sim_ref.limit_case(cat, True)
        zone = cat[0].offerings[0].zone
        cp.cluster.classes[0].preferred_terms = [(1, [Requirement(ZONE, "In", [zone])])]
        c.upload_catalog(model.CatalogView(cp.cluster.catalog))
        c.consolidate_prepare(model.ConsolidateInputView(cp, SINGLE))
        for fn, a in ((c.simulate_execute, (SINGLE, 1)), (c.drift_command, ()), (c.consolidate_validate, (SINGLE, 0, False))):
            assert "relax" in _raises(abi.KP_E_UNSUPPORTED, fn, *a)
        rcat = synth.config5_catalog(golden[:120], n_default=60, n_block=0, seed=3)
        cp = fuzzgen.fuzz_consolidation(rcat, 7502, n_nodes=10, n_pods=40)
        c.upload_catalog(model.CatalogView(rcat))
        c.consolidate_prepare(model.ConsolidateInputView(cp, SINGLE))
        for fn, a in ((c.simulate_execute, (SINGLE, 1)), (c.drift_command, ()), (c.consolidate_validate, (SINGLE, 0, False))):
            assert "reserved" in _raises(abi.KP_E_UNSUPPORTED, fn, *a)
    finally:
        c.close()


def test_unsupported_probe_beside_supported_ones(ctx, cat):
    """A candidate whose pod carries a host port is a probe the kernel does not cover; its neighbours are simulated."""
    cp = sim_ref.drift_case(cat)
    cp.cluster.classes.append(PodClass(host_ports=[HostPort(8080)]))
    cp.cluster.pods.class_id[4] = len(cp.cluster.classes) - 1  # candidate 2's pod
    prepare(ctx, cp)
    rows = ctx.simulate_execute(SINGLE, 4)
    assert rows["status"].tolist() == [0, 0, abi.KP_SIM_UNSUPPORTED_PROBE, 0]
    assert [int(rows[2][f]) for f in sim_ref.ROW_FIELDS[1:]] == [0] * 5
    assert ctx.simulate_stats()[1][5] == 1
    check_probe(ctx, cp, SINGLE, 1)
    row, pods, res, _ = ctx.simulate_nodeclaims(SINGLE, 2)
    assert row["status"] == abi.KP_SIM_UNSUPPORTED_PROBE and len(pods) == 0 and res.n_nodeclaims == 0
    assert "KP_E_UNSUPPORTED" in _raises(abi.KP_E_UNSUPPORTED, ctx.consolidate_validate, SINGLE, 2, False)


def test_short_buffers(ctx, cat):
    import ctypes as C
    cp = sim_ref.per_type_case(cat, 3)
    prepare(ctx, cp)
    L = ctx.L
    rows = np.zeros(1, abi.SIM_DTYPE)
    assert L.kp_simulate_execute(ctx.h, SINGLE, 0, 0, rows.ctypes.data_as(C.POINTER(abi.kp_sim_result)), 0) == abi.KP_E_BUFFER
    o = abi.kp_sim_nodeclaims()
    assert L.kp_simulate_nodeclaims(ctx.h, SINGLE, 0, C.byref(o)) == abi.KP_E_BUFFER
    assert o.n_nodeclaims == 3 and o.n_pods == 3 and o.n_type_ids > 0
    need = C.c_int64(0)
    assert L.kp_simulate_nodeclaim_requirements(ctx.h, 0, None, 0, C.byref(need)) == abi.KP_E_BUFFER and need.value > 1
    assert L.kp_simulate_nodeclaim_requirements(ctx.h, 3, None, 0, C.byref(need)) == abi.KP_E_INVALID
    d = abi.kp_drift_command_out()
    assert L.kp_drift_command(ctx.h, C.byref(d)) == abi.KP_E_BUFFER and d.n_candidates == 1
    _raises(abi.KP_E_INVALID, ctx.simulate_nodeclaims, SINGLE, 5)


def test_multi_device_ctx_same_rows(ctx, corpora):
    cp = corpora[STRICT]["fuzz5"]
    prepare(ctx, cp)
    want = {m: ctx.simulate_execute(m, sim_ref.n_probes(cp, m)) for m in (SINGLE, MULTI)}
    c = native.Context(0, devices=[0, 0])
    try:
        prepare(c, cp)
        for m in (SINGLE, MULTI):
            assert c.simulate_execute(m, sim_ref.n_probes(cp, m)).tobytes() == want[m].tobytes()
        check_probe(c, cp, MULTI, 1)
    finally:
        c.close()


def test_stats(ctx, corpora):
    cp = corpora[STRICT]["fuzz5"]
    prepare(ctx, cp)
    n = sim_ref.n_probes(cp, SINGLE)
    ctx.simulate_execute(SINGLE, n)
    ms, ct = ctx.simulate_stats()
    assert ms[0] > 0 and ms[1] > 0 and ms[2] >= ms[0] + ms[1]
    assert ct[3] == n and ct[0] >= sum(len(c.pods) for c in cp.candidates) and ct[2] > 0


# ------------------------------------------------------------------------------------------------
# more than one batch (KPSIM_SIM_BATCH caps the probes per batch; counter 6 of kp_simulate_stats counts the batches)
# ------------------------------------------------------------------------------------------------
# (cluster, mode, policy, caps); tests/test_simulate_cpu.py::test_batch_lists pins the NodeClaim counts per probe:
#   fuzz5 MULTI   4 7 7 9 11 O O (O: past 12)  caps 1, 2: a last batch of overflow rows alone; 3: a short last batch
#   fuzz9 MULTI   7 7 7 12 O                   cap 2: `most` 7, then 12; cap 4: the overflow row alone in the last batch
#   min126 MULTI  0, 1 (1 dropped), 8 (7 dropped), 9 (8 dropped): dropped NodeClaims past the first batch
#   fuzz4         22 MULTI probes from 2 to 8 NodeClaims, 23 SINGLE probes: `most` differs from batch to batch
#   min6 SINGLE   no NodeClaim among the first five probes: a first batch with nothing to finalize
BATCH_LISTS = [("fuzz5", MULTI, STRICT, (1, 2, 3)), ("fuzz9", MULTI, STRICT, (2, 4)), ("min126", MULTI, STRICT, (2, 3)),
               ("min126", MULTI, BEST_EFFORT, (2, 3)), ("fuzz4", MULTI, STRICT, (5, 7, 21)),
               ("fuzz4", SINGLE, STRICT, (5, 7, 21)), ("min6", SINGLE, STRICT, (5,))]
CS_MUT = 17  # kp_consolidate_stats: probes the MUT variant ran


def _batches(n, cap):
    return -(-n // cap)


@pytest.mark.parametrize("name,mode,policy,caps", BATCH_LISTS,
                         ids=["%s-%s-%d" % (b[0], "multi" if b[1] == MULTI else "single", b[2]) for b in BATCH_LISTS])
def test_batches(ctx, corpora, monkeypatch, name, mode, policy, caps):
    """A probe list in several batches gives the rows of the reference, byte for byte those of one batch, and the same
    counters; the consolidation pass's rows and figures are untouched."""
    cp = corpora[policy][name]
    prepare(ctx, cp)
    n = sim_ref.n_probes(cp, mode)
    want = sim_ref.rows(cp, mode, cached_refs((name, policy), cp, mode))
    before = ctx.consolidate_execute(mode, n)
    cstats = ctx.consolidate_stats()
    batch_cap(monkeypatch, None)
    whole = ctx.simulate_execute(mode, n)
    st0 = ctx.simulate_stats()[1]
    sim_ref.assert_rows_equal(whole, want)
    assert st0[3] == n and st0[6] == 1
    for cap in caps:
        batch_cap(monkeypatch, cap)
        got = ctx.simulate_execute(mode, n)
        st = ctx.simulate_stats()[1]
        print("%s mode %d cap %d: counters %s" % (name, mode, cap, st))
        sim_ref.assert_rows_equal(got, want)
        assert got.tobytes() == whole.tobytes()
        assert st[:6] == st0[:6]
        assert st[6] == _batches(n, cap) and st[6] > 1
    batch_cap(monkeypatch, None)
    assert ctx.simulate_execute(mode, n).tobytes() == whole.tobytes()
    assert ctx.simulate_stats()[1] == st0
    assert ctx.consolidate_stats() == cstats
    assert ctx.consolidate_execute(mode, n).tobytes() == before.tobytes()


def test_batch_lists_hold_mut_probes(ctx, corpora):
    """At least two of test_batches' passes run probes with per-probe node requirement copies (kp_cons.h MUT)."""
    with_mut = []
    for name, mode, policy, _ in BATCH_LISTS:
        cp = corpora[policy][name]
        prepare(ctx, cp)
        ctx.consolidate_execute(mode, sim_ref.n_probes(cp, mode))
        if ctx.consolidate_stats()[1][CS_MUT] > 0:
            with_mut.append((name, mode, policy))
    print("passes with MUT probes:", with_mut)
    assert len(with_mut) >= 2


@pytest.mark.parametrize("name", ["fuzz5", "fuzz9"])
def test_nodeclaims_after_capped_and_uncapped_calls(ctx, corpora, monkeypatch, name):
    """The workers' slabs are strided by the batch's size and zeroed only when they grow: whole lists in one batch, lists
    in batches of 3 and single probes (a batch of one) alternate over the same buffers, and every result stays right."""
    cp = corpora[STRICT][name]
    prepare(ctx, cp)
    refs = {m: cached_refs((name, STRICT), cp, m) for m in (SINGLE, MULTI)}
    want = {m: sim_ref.rows(cp, m, refs[m]) for m in (SINGLE, MULTI)}

    def lists(cap):
        batch_cap(monkeypatch, cap)
        for m in (SINGLE, MULTI):
            sim_ref.assert_rows_equal(ctx.simulate_execute(m, len(refs[m])), want[m])
            assert ctx.simulate_stats()[1][6] == (_batches(len(refs[m]), cap) if cap else 1)
        batch_cap(monkeypatch, None)

    big = next(i for i, r in enumerate(refs[MULTI]) if r["row"]["status"] == abi.KP_SIM_OK and r["n_nodeclaims"] >= 7)
    last = len(refs[MULTI]) - 1
    assert refs[MULTI][last]["row"]["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW
    for _ in range(2):
        lists(None)
        lists(3)
        for i in (big, last):
            check_probe(ctx, cp, MULTI, i, refs[MULTI][i])
            lists(None)
    batch_cap(monkeypatch, 3)  # a single probe is a batch of one whatever the cap
    check_probe(ctx, cp, MULTI, big, refs[MULTI][big])
    assert ctx.simulate_stats()[1][6] == 1


# ------------------------------------------------------------------------------------------------
# sub-ranges of the probe lists
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [None, 3])
@pytest.mark.parametrize("mode", [SINGLE, MULTI])
@pytest.mark.parametrize("name", ["fuzz4", "fuzz5"])
def test_sub_ranges(ctx, corpora, monkeypatch, name, mode, cap):
    """simulate_execute(mode, n, begin, end) is the whole list's rows [begin, end): ranges that start past 0, end before
    the list does, hold one probe or none; a begin past the end is refused."""
    cp = corpora[STRICT][name]
    prepare(ctx, cp)
    n = sim_ref.n_probes(cp, mode)
    want = sim_ref.rows(cp, mode, cached_refs((name, STRICT), cp, mode))
    batch_cap(monkeypatch, None)
    whole = ctx.simulate_execute(mode, n)
    sim_ref.assert_rows_equal(whole, want)
    batch_cap(monkeypatch, cap)
    mid = n // 2
    parts = [(0, 2), (2, n - 2), (n - 2, n)]
    assert 2 < mid < n - 2
    for b, e in parts + [(1, n), (mid, mid + 1), (3, n - 2), (mid, mid), (n - 1, n)]:
        got = ctx.simulate_execute(mode, n, begin=b, end=e)
        st = ctx.simulate_stats()[1]
        assert len(got) == e - b and got.tobytes() == whole[b:e].tobytes(), (b, e)
        sim_ref.assert_rows_equal(got, want[b:e])
        if b == e:
            assert st == [0] * 7  # KP_OK, no rows, nothing simulated
        else:
            assert st[3] == e - b and st[6] == (_batches(e - b, cap) if cap else 1), (b, e, st)
    assert b"".join(ctx.simulate_execute(mode, n, begin=b, end=e).tobytes() for b, e in parts) == whole.tobytes()
    _raises(abi.KP_E_INVALID, ctx.simulate_execute, mode, n, mid, mid - 1)
    _raises(abi.KP_E_INVALID, ctx.simulate_execute, mode, n, n - 1, 1)


# ------------------------------------------------------------------------------------------------
# drift over more candidates than one batch holds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fuzz1", "fuzz3", "fuzz5", "fuzz6", "fuzz8", "fuzz9", "drift_case"])
def test_drift_under_a_batch_cap(ctx, corpora, cat, monkeypatch, name):
    cp = sim_ref.drift_case(cat) if name == "drift_case" else corpora[STRICT][name]
    prepare(ctx, cp)
    NC = len(cp.candidates)
    refs = cached_refs((name, STRICT), cp, SINGLE)
    rows = sim_ref.rows(cp, SINGLE, refs)
    decision, cands = sim_ref.drift_replay(cp, rows)
    batch_cap(monkeypatch, None)
    whole = ctx.drift_command()
    assert ctx.simulate_stats()[1][6] == (0 if decision == abi.KP_DRIFT_DELETE_EMPTY else 1)
    batch_cap(monkeypatch, 2)
    cmd = ctx.drift_command()
    st = ctx.simulate_stats()[1]
    assert cmd == whole
    assert (cmd["decision"], cmd["candidates"]) == (decision, cands)
    assert decision != abi.KP_DRIFT_DELETE_EMPTY  # every candidate of these clusters holds pods: all are simulated
    assert st[3] == NC and st[6] == _batches(NC, 2) and st[6] > 1
    if decision == abi.KP_DRIFT_REPLACE:
        assert cmd["n_nodeclaims"] == rows[cands[0]]["n_new_nodeclaims"] and cmd["row"] == refs[cands[0]]["row"]
    else:
        assert cmd["n_nodeclaims"] == 0 and cmd["row"] == dict.fromkeys(sim_ref.ROW_FIELDS, 0)


# ------------------------------------------------------------------------------------------------
# seven to twelve NodeClaims whose slice order decides
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sim_ref.LADDERS))
def test_slice_order_at_seven_to_twelve(ctx, cat, name):
    """sim_ref.ladder_case: every floater joins the first NodeClaim of the re-sorted slice that lists its type
    (tests/test_simulate_cpu.py::test_ladder_cases shows that a tie broken by id or a scan in id order goes elsewhere)."""
    counts = sim_ref.LADDERS[name]
    cp, _, floaters = sim_ref.ladder_case(cat, counts)
    prepare(ctx, cp)
    ref = cached_ref(("ladder", name), cp, SINGLE, 0)
    n = len(counts)
    pos = np.asarray(ref["results"].nodeclaim_slice_pos[:n]).tolist()
    assert ref["n_nodeclaims"] == n and sorted(pos) == list(range(n)) and pos != list(range(n))
    row = ctx.simulate_execute(SINGLE, 1)[0]
    assert (row["status"], row["all_scheduled"], row["n_new_nodeclaims"], row["n_pods"]) == \
        (abi.KP_SIM_OK, 1, n, sum(counts) + len(floaters))
    check_probe(ctx, cp, SINGLE, 0, ref)
    _, _, res, _ = ctx.simulate_nodeclaims(SINGLE, 0)
    assert res.nodeclaim_slice_pos.tolist() == pos
    for p, _ in floaters:
        assert int(res.pod_result[p]) == int(ref["results"].pod_result[p])


# ------------------------------------------------------------------------------------------------
# the queue bitmap past 4096 pods
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sim_ref.BITMAP_SEEDS)
def test_queue_bitmap_second_block(ctx, cat, seed):
    """sim_ref.bitmap_block_case: 4300 pods, so the queue bitmap has 68 words and the kernel's scan takes a second step;
    the probes' pods sit at queue ranks on both sides of 4096 and of the word edges around it.  kp_consolidate_prepare
    takes the cluster as it is, with most of its pods owned by no candidate and not pending: no extra candidate and no
    sub-range was needed."""
    cp, rank = sim_ref.bitmap_block_case(cat, seed)
    assert cp.cluster.pods.n > 4096 + 64
    prepare(ctx, cp)
    for mode in (SINGLE, MULTI):
        refs = cached_refs(("bitmap", seed), cp, mode)
        sim_ref.assert_rows_equal(ctx.simulate_execute(mode, len(refs)), sim_ref.rows(cp, mode, refs))
        for i, ref in enumerate(refs):
            assert ref["row"]["status"] == abi.KP_SIM_OK
            check_probe(ctx, cp, mode, i, ref)  # the row, the pods list, the Results and the requirements
            _, pods, _, _ = ctx.simulate_nodeclaims(mode, i)
            assert pods.tolist() == ref["pods"]
            if mode == MULTI:
                ranks = rank[pods[len(cp.pending):]]
                assert ranks.min() < 4096 <= ranks.max()
