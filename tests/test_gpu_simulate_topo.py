"""GPU: kp_simulate_*, kp_drift_command and kp_consolidate_validate over clusters with topology terms, behind
kp_device_opts.simulate_topology (simulate_topo_kernel).

The reference of a probe is tests/sim_topo_ref.py: the CPU oracle's Solve of the probe with its candidate nodes and every
counted pod kept (tests/test_simulate_topo_cpu.py pins it to pyoracle.consolidate on the oracle alone and shows that the
corpus and the hand clusters are not vacuous).  Rows are compared field by field, the NodeClaims, placements and
requirements of a probe with tests/parity.py::assert_same.  Every context here is created with simulate_topology=1
except where the gate itself is under test.
"""
import numpy as np
import pytest

import fuzzgen
import parity
import sim_ref
import sim_topo_ref as str_
from kpsim import abi, model, native, synth
from kpsim.model import ZONE, Requirement

pytestmark = pytest.mark.gpu

SINGLE, MULTI = sim_ref.SINGLE, sim_ref.MULTI
STRICT, BEST_EFFORT = abi.KP_MIN_VALUES_STRICT, abi.KP_MIN_VALUES_BEST_EFFORT
OK = abi.KP_SIM_OK


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0, simulate_topology=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cat(golden):
    return golden[:200]


@pytest.fixture(scope="module")
def corpora(golden):
    return {pol: dict(str_.corpus(golden, pol)) for pol in (STRICT, BEST_EFFORT)}


def prepare(ctx, cp):
    ctx.upload_catalog(model.CatalogView(cp.cluster.catalog))
    ctx.consolidate_prepare(model.ConsolidateInputView(cp, SINGLE))


_REFS = {}


def cached_ref(key, cp, mode, i):
    """sim_topo_ref.reference(cp, mode, i), computed once per module for the cluster named `key`; nothing changes a
    cached reference"""
    k = (key, mode, i)
    if k not in _REFS:
        _REFS[k] = str_.reference(cp, mode, i)
    return _REFS[k]


def cached_refs(key, cp, mode):
    return [cached_ref(key, cp, mode, i) for i in range(sim_ref.n_probes(cp, mode))]


def check_probe(ctx, cp, mode, i, ref=None):
    """kp_simulate_nodeclaims of one probe against its reference: row, pod list, Results and requirements"""
    ref = ref or str_.reference(cp, mode, i)
    row, pods, res, reqs = ctx.simulate_nodeclaims(mode, i)
    assert row == ref["row"], (mode, i, row, ref["row"])
    if row["status"] != OK:
        assert len(pods) == 0 and res.n_nodeclaims == 0
        return ref
    assert pods.tolist() == ref["pods"]
    parity.assert_same((res, reqs), (ref["results"], ref["reqs"]))
    return ref


def batch_cap(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("KPSIM_SIM_BATCH", raising=False)
    else:
        monkeypatch.setenv("KPSIM_SIM_BATCH", str(cap))


def _raises(status, fn, *a):
    with pytest.raises(native.KpError) as e:
        fn(*a)
    assert e.value.status == status, e.value
    return str(e.value)


# ------------------------------------------------------------------------------------------------
# fuzz: every row and the Results behind them, both minValues policies, both probe lists
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [STRICT, BEST_EFFORT])
@pytest.mark.parametrize("name", str_.CORPUS)
def test_fuzz(ctx, corpora, name, policy):
    """Every row of both probe lists; the Results and requirements of every probe with 2 or more NodeClaims and of a third
    of the rest; and the same pass's kp_consolidate_execute rows agree wherever they are not capped at 2 NodeClaims."""
    cp = corpora[policy][name]
    prepare(ctx, cp)
    for mode in (SINGLE, MULTI):
        refs = cached_refs((name, policy), cp, mode)
        n = len(refs)
        cons = ctx.consolidate_execute(mode, n)
        dev = ctx.simulate_execute(mode, n)
        sim_ref.assert_rows_equal(dev, sim_ref.rows(cp, mode, refs))
        assert not (dev["status"] == abi.KP_SIM_UNSUPPORTED_PROBE).any()
        for i, ref in enumerate(refs):
            if ref["n_nodeclaims"] >= 2 or i % 3 == 0:
                check_probe(ctx, cp, mode, i, ref)
        assert ctx.consolidate_execute(mode, n).tobytes() == cons.tobytes()  # the pass's own counts were not touched
        for r, s in zip(cons, dev):
            created = s["n_new_nodeclaims"] + s["n_dropped"]
            many = s["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW or created >= 2
            assert (r["n_new_nodeclaims"] == 2) == many
            if not many:
                assert r["all_scheduled"] == s["all_scheduled"] and r["n_pods"] == s["n_pods"]
                # (a probe that left pods unscheduled counts its one NodeClaim before truncation: DESIGN §1 known gap)
                assert r["n_new_nodeclaims"] == s["n_new_nodeclaims"] or \
                    (s["n_dropped"] == 1 and not s["all_scheduled"] and r["n_new_nodeclaims"] == 1)


# ------------------------------------------------------------------------------------------------
# hand clusters
# ------------------------------------------------------------------------------------------------
def test_zonal_spread_three_zones(ctx, cat):
    cp = str_.zonal_spread_case(cat)
    prepare(ctx, cp)
    check_probe(ctx, cp, SINGLE, 0)
    row, _, res, reqs = ctx.simulate_nodeclaims(SINGLE, 0)
    assert (row["status"], row["all_scheduled"], row["n_new_nodeclaims"]) == (OK, 1, 3)
    assert sorted(res.pod_result.tolist()) == [0, 1, 2]
    zones = str_.nodeclaim_zones(reqs)
    assert all(z is not None and len(z) == 1 for z in zones) and len(set(zones)) == 3


@pytest.mark.parametrize("n", [12, 13])
def test_hostname_anti_affinity_columns(ctx, cat, n):
    """n pods, n NodeClaims: hostname columns E .. E + 11, and at 13 the template evaluation with host E + 12"""
    cp = str_.hostname_anti_case(cat, n)
    prepare(ctx, cp)
    check_probe(ctx, cp, SINGLE, 0)
    row = ctx.simulate_execute(SINGLE, 1)[0]
    if n == 12:
        assert (row["status"], row["all_scheduled"], row["n_new_nodeclaims"], row["n_pods"]) == (OK, 1, 12, 12)
        _, _, res, _ = ctx.simulate_nodeclaims(SINGLE, 0)
        assert sorted(res.pod_result.tolist()) == list(range(12)) and res.nodeclaim_n_pods.tolist() == [1] * 12
    else:
        assert row["status"] == abi.KP_SIM_NODECLAIM_OVERFLOW
        assert [int(row[f]) for f in sim_ref.ROW_FIELDS[1:]] == [0] * 5
        assert ctx.simulate_stats()[1][4] == 1


def test_nodeclaims_dropped_at_truncation(ctx, cat):
    """The topology-narrowed NodeClaims go through finalize_kernel's truncation and the host's fold of the dropped ones."""
    cp = str_.truncation_drop_case(cat)
    prepare(ctx, cp)
    ref = check_probe(ctx, cp, SINGLE, 0)
    assert ref["n_nodeclaims"] == 2
    row = ctx.simulate_execute(SINGLE, 1)[0]
    assert (row["status"], row["all_scheduled"], row["n_new_nodeclaims"], row["n_dropped"], row["n_unscheduled"]) == \
        (OK, 0, 0, 2, 2)


def test_hostname_spread_over_nodes_and_nodeclaims(ctx, cat):
    cp = str_.hostname_spread_case(cat)
    prepare(ctx, cp)
    check_probe(ctx, cp, SINGLE, 0)
    _, _, res, _ = ctx.simulate_nodeclaims(SINGLE, 0)
    assert sorted(res.pod_result.tolist()) == [-3, 0, 1, 2] and res.nodeclaim_n_pods.tolist() == [1, 1, 1]


def test_affinity_to_a_pod_on_the_candidate_node(ctx, cat):
    cp = str_.kept_node_affinity_case(cat)
    prepare(ctx, cp)
    check_probe(ctx, cp, SINGLE, 0)
    row, _, res, reqs = ctx.simulate_nodeclaims(SINGLE, 0)
    assert row["all_scheduled"] == 1 and res.pod_result.tolist() == [0]
    assert str_.nodeclaim_zones(reqs) == [(cp.cluster.existing[0].labels[ZONE],)]


def test_inverse_anti_affinity_of_a_bound_pod(ctx, cat):
    cp = str_.inverse_anti_case(cat)
    prepare(ctx, cp)
    check_probe(ctx, cp, SINGLE, 0)
    _, _, res, _ = ctx.simulate_nodeclaims(SINGLE, 0)
    assert res.pod_result.tolist() == [-4]  # node n2: n1 holds the pod that refuses it


# ------------------------------------------------------------------------------------------------
# more than one batch: the per-worker topology buffers start afresh for every probe
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,caps", [("topo4", MULTI, (1, 3)), ("haff6", SINGLE, (2, 5))])
def test_batches(ctx, corpora, monkeypatch, name, mode, caps):
    cp = corpora[STRICT][name]
    prepare(ctx, cp)
    n = sim_ref.n_probes(cp, mode)
    want = sim_ref.rows(cp, mode, cached_refs((name, STRICT), cp, mode))
    batch_cap(monkeypatch, None)
    whole = ctx.simulate_execute(mode, n)
    st0 = ctx.simulate_stats()[1]
    sim_ref.assert_rows_equal(whole, want)
    assert st0[3] == n and st0[6] == 1
    for cap in caps:
        batch_cap(monkeypatch, cap)
        got = ctx.simulate_execute(mode, n)
        st = ctx.simulate_stats()[1]
        assert got.tobytes() == whole.tobytes()
        assert st[:6] == st0[:6]
        assert st[6] == -(-n // cap) and st[6] > 1
    batch_cap(monkeypatch, None)
    assert ctx.simulate_execute(mode, n).tobytes() == whole.tobytes()


# ------------------------------------------------------------------------------------------------
# drift and validation
# ------------------------------------------------------------------------------------------------
def test_drift_replaces_the_first_candidate_whose_spread_can_be_satisfied(ctx, cat):
    cp = str_.drift_spread_case(cat)
    prepare(ctx, cp)
    cmd = ctx.drift_command()
    assert (cmd["decision"], cmd["candidates"], cmd["n_nodeclaims"]) == (abi.KP_DRIFT_REPLACE, [1], 1)
    assert cmd["row"] == check_probe(ctx, cp, SINGLE, 1)["row"]
    for i in (0, 2):
        assert check_probe(ctx, cp, SINGLE, i)["row"]["all_scheduled"] == 0
    cp = str_.drift_spread_case(cat, movable=False)
    prepare(ctx, cp)
    cmd = ctx.drift_command()
    assert (cmd["decision"], cmd["candidates"], cmd["n_nodeclaims"]) == (abi.KP_DRIFT_NONE, [], 0)


def test_drift_replaces_the_first_candidate_topology_lets_move(ctx, cat):
    cp = str_.drift_case(cat)
    prepare(ctx, cp)
    cmd = ctx.drift_command()
    assert (cmd["decision"], cmd["candidates"], cmd["n_nodeclaims"]) == (abi.KP_DRIFT_REPLACE, [1], 2)
    assert cmd["row"] == check_probe(ctx, cp, SINGLE, 1)["row"]
    cp = str_.drift_case(cat, movable=False)
    prepare(ctx, cp)
    cmd = ctx.drift_command()
    assert (cmd["decision"], cmd["candidates"]) == (abi.KP_DRIFT_NONE, [])


@pytest.mark.parametrize("name", ["topo2", "topo7", "topo13", "haff10", "haff16"])
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


def test_validate_verdicts(ctx, cat):
    V = abi
    cp = str_.kept_node_affinity_case(cat)  # one NodeClaim, in the zone of the pod on the candidate's node
    prepare(ctx, cp)
    ref = str_.reference(cp, SINGLE, 0)
    types = list(ref["results"].nodeclaim_types[0])
    outside = next(t for t in range(len(cat)) if t not in types)
    assert ctx.consolidate_validate(SINGLE, 0, True, types[:3]) == V.KP_VALIDATE_VALID
    assert ctx.consolidate_validate(SINGLE, 0, True, types[:3] + [outside]) == V.KP_VALIDATE_NOT_SUBSET
    assert ctx.consolidate_validate(SINGLE, 0, False) == V.KP_VALIDATE_NEEDS_NODECLAIM
    for had, ids in ((False, []), (True, types[:3]), (True, [outside])):
        assert ctx.consolidate_validate(SINGLE, 0, had, ids) == sim_ref.validate(ref, had, ids)
    cp = str_.hostname_anti_case(cat, 2)
    prepare(ctx, cp)
    assert ctx.consolidate_validate(SINGLE, 0, True, [0]) == V.KP_VALIDATE_MULTIPLE_NODECLAIMS
    cp = str_.drift_case(cat)
    prepare(ctx, cp)
    assert ctx.consolidate_validate(SINGLE, 0, True, [0]) == V.KP_VALIDATE_PODS_UNSCHEDULABLE


@pytest.mark.parametrize("name", ["topo3", "topo8", "haff2"])
def test_validate_fuzz(ctx, corpora, name):
    cp = corpora[STRICT][name]
    prepare(ctx, cp)
    for mode in (SINGLE, MULTI):
        for i, ref in enumerate(cached_refs((name, STRICT), cp, mode)):
            if ref["row"]["status"] != OK:
                continue
            valid = [q for q in range(ref["n_nodeclaims"]) if int(ref["results"].nodeclaim_nodepool[q]) >= 0]
            ids = [int(t) for t in ref["results"].nodeclaim_types[valid[0]][:3]] if valid else [0]
            for had in (False, True):
                assert ctx.consolidate_validate(mode, i, had, ids if had else []) == \
                    sim_ref.validate(ref, had, ids if had else []), (mode, i, had)


# ------------------------------------------------------------------------------------------------
# the gate
# ------------------------------------------------------------------------------------------------
def test_gate_off_refuses(cat):
    c = native.Context(0, simulate_topology=0)
    try:
        cp = str_.zonal_spread_case(cat)
        prepare(c, cp)
        for fn, a in ((c.simulate_execute, (SINGLE, 1)), (c.simulate_nodeclaims, (SINGLE, 0)), (c.drift_command, ()),
                      (c.consolidate_validate, (SINGLE, 0, False))):
            assert "topology" in _raises(abi.KP_E_UNSUPPORTED, fn, *a)
    finally:
        c.close()


def test_gate_on_keeps_the_other_refusals(ctx, cat, golden):
    cp = str_.zonal_spread_case(cat)
    zone = cat[0].offerings[0].zone
    cp.cluster.classes[0].preferred_terms = [(1, [Requirement(ZONE, "In", [zone])])]
    prepare(ctx, cp)
    for fn, a in ((ctx.simulate_execute, (SINGLE, 1)), (ctx.simulate_nodeclaims, (SINGLE, 0)), (ctx.drift_command, ()),
                  (ctx.consolidate_validate, (SINGLE, 0, False))):
        assert "relax" in _raises(abi.KP_E_UNSUPPORTED, fn, *a)
    rcat = synth.config5_catalog(golden[:120], n_default=60, n_block=0, seed=3)
    cp = fuzzgen.fuzz_consolidation(rcat, 7502, n_nodes=10, n_pods=40)
    ctx.upload_catalog(model.CatalogView(rcat))
    ctx.consolidate_prepare(model.ConsolidateInputView(cp, SINGLE))
    for fn, a in ((ctx.simulate_execute, (SINGLE, 1)), (ctx.simulate_nodeclaims, (SINGLE, 0)), (ctx.drift_command, ()),
                  (ctx.consolidate_validate, (SINGLE, 0, False))):
        assert "reserved" in _raises(abi.KP_E_UNSUPPORTED, fn, *a)


def test_gate_on_leaves_plain_passes_alone(ctx, golden):
    """A cluster without topology terms: the rows of a gated context are byte for byte those of a default one."""
    name, cp = sim_ref.corpus(golden, STRICT)[4]
    plain = native.Context(0)
    try:
        prepare(plain, cp)
        prepare(ctx, cp)
        for mode in (SINGLE, MULTI):
            n = sim_ref.n_probes(cp, mode)
            assert ctx.simulate_execute(mode, n).tobytes() == plain.simulate_execute(mode, n).tobytes()
            a, b = ctx.simulate_nodeclaims(mode, 1), plain.simulate_nodeclaims(mode, 1)
            assert a[0] == b[0] and a[1].tolist() == b[1].tolist()
            parity.assert_same((a[2], a[3]), (b[2], b[3]))
    finally:
        plain.close()
