"""CPU companions of tests/test_gpu_word_edges.py: the oracle alone over the same inputs (tests/edge_cases.py), so the
GPU parity tests cannot pass vacuously and a mistake in a hand KAT's plain expectation shows without a device.

  * the fuzz generators' default path still makes the rng draws it made before they learned `zones=` (committed digests,
    tests/golden/fuzz_digests.json, re-derived here);
  * per zoned catalog (32 x 2, 64 x 1, 63 x 1 slots) and fuzz family: enough pods schedule, NodeClaims sit in the upper
    half of the zone words, single-zone NodeClaims occur at several upper-half zones, the consolidation probes decide
    REPLACE, DELETE and NONE;
  * the hand KATs' expectations (every zone once, spread over all zones, availability and price at the top slot and at
    slots 31 / 32) hold for the oracle."""
import dataclasses
import json
import os

import numpy as np
import pytest

import edge_cases as EC
import launch_cases as LC
import parity
import pyoracle
from kpsim import abi, launch, model

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cats(fx):
    return {name: EC.named_catalog(fx, name) for name in EC.NAMES}


def test_fuzz_default_path_unchanged(golden):
    """seeds 0-3 of fuzz_problem, fuzz_topology_problem, fuzz_topology_existing_problem and fuzz_consolidation without
    zones=: the oracle's result digests (and the consolidation candidates) equal the ones committed before the keyword
    was added (tests/golden/gen_fuzz_digests.py)"""
    with open(os.path.join(HERE, "golden", "fuzz_digests.json")) as f:
        want = json.load(f)
    assert EC.fuzz_default_digests(golden) == want


@pytest.mark.parametrize("name", EC.NAMES)
def test_catalog_shapes(cats, name):
    nz, cts = EC.CATALOGS[name]
    cat = cats[name]
    assert len(cat) == 160 and len(EC.zones_of(cat)) == nz and len(EC.slots(cat)) == nz * len(cts)
    assert EC.zones_of(cat)[:3] == ["test-zone-1a", "test-zone-1b", "test-zone-1c"]
    assert all(len(it.offerings) == nz * len(cts) for it in cat)


# ---- fuzz families: not vacuous -------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["requirements", "topology", "topology_existing"])
@pytest.mark.parametrize("name", EC.NAMES)
def test_solve_families_not_vacuous(cats, name, family):
    cat = cats[name]
    zs = EC.zones_of(cat)
    upper = set(zs[len(zs) // 2:])
    sched = total = 0
    single = set()
    for seed in range(EC.FAMILY_SEEDS[family]):
        prob = EC.family_problem(cat, family, seed)
        r, reqs = parity.run_oracle(prob)
        sched += int((r.pod_result != -1).sum())
        total += prob.pods.n
        for i in range(r.n_nodeclaims):
            comp, _, _, _, vals = reqs[i][model.ZONE]
            # every NodeClaim's zone requirement lies wholly in the upper half (the NodePools are pinned there)
            assert not comp and vals and set(vals) <= upper, (seed, i, reqs[i][model.ZONE])
            z = EC.single_zone(reqs[i], zs)
            if z is not None:
                single.add(z)
        if len(zs) < 64:  # the pod zone value no catalog has: 63 zones + 1 = a full 64-value dictionary
            assert any(r_.key == model.ZONE and EC.FOREIGN_ZONE in r_.values for pc in prob.classes
                       for r_ in pc.requirements)
    assert 4 * sched >= total, (sched, total)
    if family == "topology":
        assert len(single) >= 3, sorted(single)


@pytest.mark.parametrize("family", ["consolidation", "topology_consolidation"])
@pytest.mark.parametrize("name", EC.NAMES)
def test_consolidation_families_not_vacuous(cats, name, family):
    cat = cats[name]
    zs = EC.zones_of(cat)
    upper = set(zs[len(zs) // 2:])
    seen = set()
    for seed in range(EC.FAMILY_SEEDS[family]):
        cp = EC.family_problem(cat, family, seed)
        assert all(n.labels[model.ZONE] in upper for n in cp.cluster.existing)
        for mode in (abi.KP_CONSOLIDATE_SINGLE, abi.KP_CONSOLIDATE_MULTI):
            seen |= set(int(d) for d in pyoracle.consolidate(cp, mode, spot_to_spot=seed % 2 == 0)["decision"])
    assert {abi.KP_DECISION_REPLACE, abi.KP_DECISION_DELETE, abi.KP_DECISION_NONE} <= seen, seen


# ---- hand KATs: the plain expectations hold for the oracle ----------------------------------------------------
@pytest.mark.parametrize("name", EC.NAMES)
def test_kat_every_zone_once(cats, name):
    prob, expect = EC.kat_every_zone(cats[name])
    assert min(n for _, n in expect) > 60  # the lists are truncated
    EC.check_every_zone(prob, parity.run_oracle(prob), expect)


@pytest.mark.parametrize("min_domains", [False, True])
@pytest.mark.parametrize("name", EC.NAMES)
def test_kat_spread_over_all_zones(cats, name, min_domains):
    prob = EC.kat_spread(cats[name], min_domains)
    EC.check_spread(prob, parity.run_oracle(prob))


@pytest.mark.parametrize("name", EC.NAMES)
def test_kat_availability_at_slot(cats, name):
    for slot in EC.top_slots(cats[name]):
        prob, A, B, zone, ct, ra, rb = EC.kat_two_types(cats[name], slot, a_available=False)
        assert A // 64 != B // 64
        r, _ = parity.run_oracle(prob)
        assert r.nodeclaim_types == [[B]], (slot, r.nodeclaim_types)
        avail = EC.availability(prob.catalog)
        avail[ra], avail[rb] = 1, 0
        r, _ = parity.run_oracle(dataclasses.replace(prob, catalog=EC.apply_patches(prob.catalog, avail)))
        assert r.nodeclaim_types == [[A]], (slot, r.nodeclaim_types)


@pytest.mark.parametrize("name", EC.NAMES)
def test_kat_price_at_top_slot(cats, name):
    prob, lr, steps = EC.price_steps(cats[name])
    for patches, order, rows in steps:
        cat = EC.apply_patches(prob.catalog, prices=patches)
        assert EC.by_price_then_name(cat, order[::-1], *EC.slots(cat)[-1]) == order
        r, _ = parity.run_oracle(dataclasses.replace(prob, catalog=cat))
        assert r.nodeclaim_types == [order]
        st, res = pyoracle.launch_select(model.CatalogView(cat), model.LaunchBatchView([lr]), 60)
        assert st == abi.KP_OK
        LC.check(cat, res, [{"types": [cat[t].name for t in order]}])
        assert list(res.offerings(0)) == rows
        assert int(res.rows[0]["fleet_pick"]) == launch.fleet_pick(cat, res, 0)[1]


@pytest.mark.parametrize("name", EC.NAMES)
def test_launch_batch_reaches_upper_zones(cats, name):
    """the rewritten launch requests select offerings in the upper half of the slot word, and some launch"""
    cat = cats[name]
    reqs = EC.launch_requests(cat, 300, 11)
    st, res = pyoracle.launch_select(model.CatalogView(cat), model.LaunchBatchView(reqs), 60)
    assert st == abi.KP_OK
    ok = res.rows["status"] == abi.KP_OK
    assert ok.sum() >= 75
    flat = [o for it in cat for o in it.offerings]
    zs = EC.zones_of(cat)
    upper = set(zs[len(zs) // 2:])
    hit = {flat[int(o)].zone for i in np.nonzero(ok)[0] for o in res.offerings(int(i))}
    assert zs[-1] in hit and len(hit & upper) >= len(upper) // 2


@pytest.mark.parametrize("T", [1, 64, 65])
def test_launch_requests_clamp_to_catalog(golden, T):
    cat = EC.tail_catalog(golden, T)
    reqs = EC.launch_requests(cat, 100, T, source=golden)
    names = {it.name for it in cat}
    for lr in reqs:
        for r in lr.requirements:
            if r.key == model.INSTANCE_TYPE:
                assert 1 <= len(r.values) <= T and set(r.values) <= names
    st, res = pyoracle.launch_select(model.CatalogView(cat), model.LaunchBatchView(reqs), 60)
    assert st == abi.KP_OK and (res.rows["status"] == abi.KP_OK).sum() > 0


def test_option_lists_exceed_200(golden):
    """group C's premise: the 300-pod config-2 sample has a NodeClaim with more than 200 options, so max_instance_types
    200 truncates and 2000 / 0 / -1 do not"""
    from kpsim import synth
    prob = synth.subsample(synth.config2(catalog=golden), 300)
    prob.max_instance_types = 0
    r, _ = parity.run_oracle(prob)
    assert int(r.nodeclaim_n_options.max()) > 200
    assert max(len(t) for t in r.nodeclaim_types) == int(r.nodeclaim_n_options.max())


def test_min_values_fail_at_one(golden):
    """group C's second premise: minValues on instance-family holds on the list truncated at 60 and fails at 1"""
    sched = {M: int((parity.run_oracle(EC.min_values_problem(golden, M))[0].pod_result != -1).sum()) for M in (1, 60)}
    assert sched[1] < sched[60], sched


@pytest.mark.parametrize("M", [1, 64])
def test_replace_command_fills_the_list(golden, M):
    """group C's replacement command: the hand cluster's KP_CONSOLIDATE_BOTH command is a REPLACE of both candidates with
    exactly M options (64: a full replacement list), the M cheapest fitting types by (price, name); each single-node
    probe is a REPLACE with M options too"""
    cp, want = EC.replace_cluster(golden, M)
    cmd = pyoracle.consolidate_command(cp, abi.KP_CONSOLIDATE_BOTH)
    assert cmd.decision == abi.KP_DECISION_REPLACE and cmd.candidates == [0, 1]
    assert cmd.n_replacement_types == M and list(cmd.type_ids) == want and len(want) == M
    single = pyoracle.consolidate(cp, abi.KP_CONSOLIDATE_SINGLE)
    assert (single["decision"] == abi.KP_DECISION_REPLACE).all() and (single["n_replacement_types"] == M).all()
