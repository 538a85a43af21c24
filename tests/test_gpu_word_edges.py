"""GPU: the device at the edges of its 64-bit mask words, bit-exact against the oracle and against plain expectations.

Every other GPU test runs three zones x two capacity types (offering-slot bits 0..5), max_instance_types 60, catalogs
of 17 or 160..2048 types and a few hundred pods; here (inputs: tests/edge_cases.py; CPU companions that prove them
non-vacuous: tests/test_word_edges_cpu.py):

  A  64 offering slots (32 zones x 2 capacity types, 64 zones x 1) and a 64-value zone dictionary (63 zones + one pod
     value): hand KATs with plain expectations (every zone once, spread over all zones, availability and price patches
     at the top slot and at slots 31 / 32), fuzz parity of the Solve, consolidation and launch selection with the
     NodePools and nodes in the upper half of the zone list, and the refusals one past each limit;
  B  catalogs of 1, 2, 63, 64, 65, 127, 128, 129 types (type-word tails);
  C  max_instance_types 0, -1, 1, 59, 61, 64, 65, 200, 2000 (Truncate's write bound), and launch / consolidation at
     1 and 64 with their refusals outside 1..64;
  D  0, 1, 2, 63..65, 255..257 pods, 1..129 existing nodes, 63 NodePools;
  E  kp_solve_prepare's two-thread split feeding the device (child process with KPSIM_PREP_SPLIT_MIN=1).
"""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_cases as EC
import fuzzgen
import launch_cases as LC
import parity
import pyoracle
import test_gpu_consolidation as TGC
from kpsim import abi, launch, model, native, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOTH = abi.KP_CONSOLIDATE_BOTH


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cats(fx):
    return {name: EC.named_catalog(fx, name) for name in EC.NAMES}


def solve_prepared_catalog(ctx, prob):
    """parity.run_device without the catalog upload: the Solve sees the ctx's catalog as the patches left it"""
    iv = model.SolveInputView(prob)
    cap_nc = max(16, prob.pods.n + 1)
    out = model.OutputBuffers(prob.pods.n, cap_nc, cap_nc * 60)
    ctx.solve(iv, out)
    r = out.results()
    return r, [model.parse_requirements_blob(ctx.nodeclaim_requirements(i)) for i in range(r.n_nodeclaims)]


def solve_parity(ctx, prob):
    dev = parity.run_device(ctx, prob)
    parity.assert_same(dev, parity.run_oracle(prob))
    return dev


def consolidation_parity(ctx, cp, s2s=False):
    """one KP_CONSOLIDATE_BOTH pass: its multi-node and single-node probes against the oracle's, then the command"""
    n_s = model.consolidation_probe_count(len(cp.candidates), abi.KP_CONSOLIDATE_SINGLE)
    n_m = model.consolidation_probe_count(len(cp.candidates), abi.KP_CONSOLIDATE_MULTI)
    ctx.upload_catalog(model.CatalogView(cp.cluster.catalog))
    ctx.consolidate_prepare(model.ConsolidateInputView(cp, abi.KP_CONSOLIDATE_SINGLE, spot_to_spot=s2s))
    both = ctx.consolidate_execute(BOTH, n_m + n_s)
    TGC.assert_probes_equal(both[:n_m], pyoracle.consolidate(cp, abi.KP_CONSOLIDATE_MULTI, spot_to_spot=s2s))
    TGC.assert_probes_equal(both[n_m:], pyoracle.consolidate(cp, abi.KP_CONSOLIDATE_SINGLE, spot_to_spot=s2s))
    TGC.assert_commands_equal(ctx.consolidate_command(BOTH), pyoracle.consolidate_command(cp, BOTH, spot_to_spot=s2s))
    return both


def launch_parity(ctx, cat, reqs, M=60):
    cv = model.CatalogView(cat)
    ctx.upload_catalog(cv)
    b = model.LaunchBatchView(reqs)
    dev = ctx.launch_select(b, M)
    st, orc = pyoracle.launch_select(cv, b, M)
    assert st == abi.KP_OK
    LC.assert_same(dev, orc)
    return dev


def valid_problem(golden):
    return fuzzgen.fuzz_problem(EC.sample(golden, 160, 31), 31, n_pods=80)


# ================================================================================================================
# A. zones and slots
# ================================================================================================================
@pytest.mark.parametrize("name", EC.NAMES)
def test_kat_every_zone_once(ctx, cats, name):
    """one NodeClaim per zone, a single bit of the zone word and of finalize_kernel's slot ballot (mzc) at every
    position: the option list of NodeClaim z is the plain expectation (fit, available in z, cheapest price in z then
    name, first 60) — lanes 6..63 of `lane < d.n_slots` and the high half of avail_zc decide zones 3.."""
    prob, expect = EC.kat_every_zone(cats[name])
    dev = parity.run_device(ctx, prob)
    EC.check_every_zone(prob, dev, expect)
    parity.assert_same(dev, parity.run_oracle(prob))


@pytest.mark.parametrize("min_domains", [False, True])
@pytest.mark.parametrize("name", EC.NAMES)
def test_kat_spread_over_all_zones(ctx, cats, name, min_domains):
    """maxSkew 1 over 32 / 64 / 63 zone domains: one NodeClaim per zone, counts within 1 (the min-count scan sees every
    domain); minDomains = the zone count with one pod fewer than zones"""
    prob = EC.kat_spread(cats[name], min_domains)
    dev = parity.run_device(ctx, prob)
    EC.check_spread(prob, dev)
    parity.assert_same(dev, parity.run_oracle(prob))


@pytest.mark.parametrize("name", EC.NAMES)
def test_kat_availability_at_slot(ctx, cats, name):
    """A is unavailable in one slot only (the last, 31, 32) and the pod is pinned to that slot: [B]; after
    kp_catalog_patch_avail flips both: [A]"""
    for slot in EC.top_slots(cats[name]):
        prob, A, B, zone, ct, ra, rb = EC.kat_two_types(cats[name], slot, a_available=False)
        dev = parity.run_device(ctx, prob)
        assert dev[0].nodeclaim_types == [[B]], (slot, dev[0].nodeclaim_types)
        parity.assert_same(dev, parity.run_oracle(prob))
        avail = EC.availability(prob.catalog)
        avail[ra], avail[rb] = 1, 0
        ctx.patch_avail(avail, 2)
        dev = solve_prepared_catalog(ctx, prob)
        assert dev[0].nodeclaim_types == [[A]], (slot, dev[0].nodeclaim_types)
        parity.assert_same(dev, parity.run_oracle(dataclasses.replace(prob, catalog=EC.apply_patches(prob.catalog, avail))))


@pytest.mark.parametrize("name", EC.NAMES)
def test_kat_price_at_top_slot(ctx, cats, name):
    """kp_catalog_patch_price on A's offering in the last slot, below then above B's price there: the Solve's option
    order and launch selection's type order, overrides and fleet pick follow"""
    prob, lr, steps = EC.price_steps(cats[name])
    cv = model.CatalogView(prob.catalog)
    ctx.upload_catalog(cv)
    batch = model.LaunchBatchView([lr])
    for epoch, (patches, order, rows) in enumerate(steps):
        ctx.patch_price([r for r, _ in patches], [p for _, p in patches], 2 + epoch)
        cat = EC.apply_patches(prob.catalog, prices=patches)
        dev = solve_prepared_catalog(ctx, prob)
        assert dev[0].nodeclaim_types == [order]
        parity.assert_same(dev, parity.run_oracle(dataclasses.replace(prob, catalog=cat)))
        res = ctx.launch_select(batch, 60)
        LC.check(cat, res, [{"types": [cat[t].name for t in order]}])
        assert list(res.offerings(0)) == rows
        assert int(res.rows[0]["fleet_pick"]) == launch.fleet_pick(cat, res, 0)[1]
        st, orc = pyoracle.launch_select(model.CatalogView(cat), batch, 60)
        assert st == abi.KP_OK
        LC.assert_same(res, orc)


@pytest.mark.parametrize("family,seed", [(f, s) for f in ("requirements", "topology", "topology_existing")
                                         for s in range(EC.FAMILY_SEEDS[f])])
@pytest.mark.parametrize("name", EC.NAMES)
def test_fuzz_solve_high_zones(ctx, cats, name, family, seed):
    solve_parity(ctx, EC.family_problem(cats[name], family, seed))


@pytest.mark.parametrize("family,seed", [(f, s) for f in ("consolidation", "topology_consolidation")
                                         for s in range(EC.FAMILY_SEEDS[f])])
@pytest.mark.parametrize("name", EC.NAMES)
def test_fuzz_consolidation_high_zones(ctx, cats, name, family, seed):
    consolidation_parity(ctx, EC.family_problem(cats[name], family, seed), s2s=seed % 2 == 0)


@pytest.mark.parametrize("name", EC.NAMES)
def test_launch_batch_high_zones(ctx, cats, name):
    cat = cats[name]
    dev = launch_parity(ctx, cat, EC.launch_requests(cat, 300, 11))
    for i in range(len(dev.rows)):
        want = launch.fleet_pick(cat, dev, i)
        assert int(dev.rows[i]["fleet_pick"]) == (want[1] if want else -1), i


def test_reserved_solve_32_zones(ctx, cats):
    """reserved offerings (ResvTab rows) in zones drawn over all 32, next to 64 od / spot slots"""
    c5 = synth.config5_catalog(cats["Z32x2"])
    zs = EC.zones_of(cats["Z32x2"])
    assert {o.zone for it in c5 for o in it.offerings if o.capacity_type == "reserved"} & set(zs[16:])
    prob = synth.config5(n_pods=300, catalog=c5)
    cv = model.CatalogView(c5)
    parity.assert_same(parity.run_device(ctx, prob, cv), parity.run_oracle(prob, cv))


@pytest.mark.parametrize("n_zones,cts", [(33, ("on-demand", "spot")), (65, ("on-demand",))])
def test_too_many_slots_refused(ctx, fx, golden, n_zones, cts):
    cat = EC.zoned_catalog(fx, n_zones, cts, 40, seed=n_zones)
    with pytest.raises(native.KpError) as e:
        ctx.upload_catalog(model.CatalogView(cat))
    assert e.value.status == abi.KP_E_UNSUPPORTED and "64 zone x capacity-type" in str(e.value)
    solve_parity(ctx, valid_problem(golden))  # the refusal leaves the ctx usable


def test_65th_zone_value_refused(ctx, cats, golden):
    """64 catalog zones + a pod value no catalog has: 65 values of a multi-valued label; 63 + 1 is accepted (every
    Z63x1 fuzz problem carries that requirement)"""
    prob, _ = EC.kat_every_zone(cats["Z64x1"])
    prob.classes[0].requirements = prob.classes[0].requirements + [model.Requirement(model.ZONE, "NotIn", [EC.FOREIGN_ZONE])]
    with pytest.raises(native.KpError) as e:
        parity.run_device(ctx, prob)
    assert e.value.status == abi.KP_E_UNSUPPORTED and "> 64 values" in str(e.value)
    solve_parity(ctx, valid_problem(golden))
    prob, _ = EC.kat_every_zone(cats["Z63x1"])
    prob.classes[0].requirements = prob.classes[0].requirements + [model.Requirement(model.ZONE, "NotIn", [EC.FOREIGN_ZONE])]
    solve_parity(ctx, prob)


# ================================================================================================================
# B. type-word tails
# ================================================================================================================
TAILS = [1, 2, 63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize("T", TAILS)
def test_tail_catalog_solve(ctx, golden, T):
    cat = EC.tail_catalog(golden, T)
    solve_parity(ctx, fuzzgen.fuzz_problem(cat, 9000 + T, n_pods=150))
    solve_parity(ctx, fuzzgen.fuzz_topology_problem(cat, 9100 + T, n_pods=150))


@pytest.mark.parametrize("T", [64, 65])
def test_tail_catalog_consolidation(ctx, golden, T):
    consolidation_parity(ctx, fuzzgen.fuzz_consolidation(EC.tail_catalog(golden, T), 9200 + T, n_nodes=30, n_pods=150))


@pytest.mark.parametrize("T", [1, 64, 65])
def test_tail_catalog_launch(ctx, golden, T):
    cat = EC.tail_catalog(golden, T)
    launch_parity(ctx, cat, EC.launch_requests(cat, 100, T, source=golden))


# ================================================================================================================
# C. max_instance_types
# ================================================================================================================
MS = [0, -1, 1, 59, 61, 64, 65, 200, 2000]


@pytest.fixture(scope="module")
def config2_300(golden):
    return synth.subsample(synth.config2(catalog=golden), 300)


@pytest.mark.parametrize("M", MS)
def test_max_instance_types_config2(ctx, config2_300, M):
    """Truncate at M: finalize_kernel's `r < M` write bound with nc_types strided by M (M <= 0: by T); the sample has
    option lists longer than 200 (test_word_edges_cpu.test_option_lists_exceed_200), so 200 truncates and 2000, 0 and
    -1 keep every option"""
    prob = dataclasses.replace(config2_300, max_instance_types=M)
    dev = solve_parity(ctx, prob)
    cap = M if M > 0 else len(prob.catalog)
    r = dev[0]
    assert all(len(t) == min(cap, int(n)) for t, n in zip(r.nodeclaim_types, r.nodeclaim_n_options))
    assert int(r.nodeclaim_n_options.max()) > 200


@pytest.mark.parametrize("M", MS)
def test_max_instance_types_min_values(ctx, golden, M):
    """SatisfiesMinValues on the list truncated at M (minValues 2..5 on instance-family fail at M = 1)"""
    solve_parity(ctx, EC.min_values_problem(golden, M))


def test_max_instance_types_launch(ctx, golden):
    cat = synth.config5_catalog(golden)
    reqs = synth.launch_requests(cat, n=200, seed=9400)
    for M in (1, 64):
        dev = launch_parity(ctx, cat, reqs, M)
        assert int(dev.rows["n_types"].max()) == M
    for M in (0, 65):
        with pytest.raises(native.KpError) as e:
            ctx.launch_select(model.LaunchBatchView(reqs), M)
        assert e.value.status == abi.KP_E_UNSUPPORTED and "1..64" in str(e.value)
    launch_parity(ctx, cat, reqs, 60)


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("M", [1, 64])
def test_max_instance_types_consolidation(ctx, golden, M, seed):
    """cluster.max_instance_types 1 and 64 over three fuzzed clusters, every probe of a KP_CONSOLIDATE_BOTH pass and the
    command.  Seed 2's NodePools carry minValues 2..5 on instance-family: a one-type list cannot hold them, so
    TruncateInstanceTypes drops every NodeClaim of those NodePools, while consolidate_kernel counts the NodeClaims it
    opened (and stops at the second) before that drop (at M = 1 the device gave n_new_nodeclaims 1, 1, 2, ... on the 39
    multi-node probes where the oracle has 0 x 26, 1 x 13; decisions equal).  The pass is refused instead, and the ctx
    evaluates the same cluster at 60 afterwards."""
    cp = fuzzgen.fuzz_consolidation(EC.sample(golden, 160, 9500 + seed), 9500 + seed, n_nodes=40, n_pods=200,
                                    n_candidates=40, pending_frac=0.0, with_min=seed == 2)
    cp.cluster.max_instance_types = M
    most = max([r.min_values or 0 for np_ in cp.cluster.nodepools for r in np_.requirements] + [0])
    assert (most >= 2) == (seed == 2)
    if most > M:
        with pytest.raises(native.KpError) as e:
            consolidation_parity(ctx, cp, s2s=seed % 2 == 0)
        assert e.value.status == abi.KP_E_UNSUPPORTED and "below a NodePool's minValues" in str(e.value)
        cp.cluster.max_instance_types = 60
    consolidation_parity(ctx, cp, s2s=seed % 2 == 0)


@pytest.mark.parametrize("M", [1, 64])
def test_max_instance_types_replace_command(ctx, golden, M):
    """a REPLACE command whose replacement list holds exactly M types (64: every slot of the kernel's replacement record,
    rec_i[4 .. 4 + 63], with the held-reservation count behind it): the plain expectation (the M cheapest fitting types by
    price then name), the oracle's command, and each single-node probe's replacement"""
    cp, want = EC.replace_cluster(golden, M)
    both = consolidation_parity(ctx, cp)
    assert (both["decision"] == abi.KP_DECISION_REPLACE).all() and (both["n_replacement_types"] == M).all()
    cmd = ctx.consolidate_command(BOTH)
    assert cmd.decision == abi.KP_DECISION_REPLACE and cmd.candidates == [0, 1]
    assert list(cmd.type_ids) == want and cmd.n_replacement_types == M and cmd.n_reserved == 0
    for probe in range(2):
        TGC.assert_commands_equal(ctx.consolidate_replacement(abi.KP_CONSOLIDATE_SINGLE, probe),
                                  pyoracle.consolidate_replacement(cp, abi.KP_CONSOLIDATE_SINGLE, probe))


def test_max_instance_types_at_largest_min_values(ctx, golden):
    """the smallest max_instance_types the host accepts next to Strict minValues: equal to the largest minValues"""
    cp = fuzzgen.fuzz_consolidation(EC.sample(golden, 160, 9502), 9502, n_nodes=40, n_pods=200, n_candidates=40,
                                    pending_frac=0.0, with_min=True)
    most = max(r.min_values or 0 for np_ in cp.cluster.nodepools for r in np_.requirements)
    assert 2 <= most <= 5
    cp.cluster.max_instance_types = most
    consolidation_parity(ctx, cp, s2s=True)


@pytest.mark.parametrize("M", [65, 0])
def test_max_instance_types_consolidation_refused(ctx, golden, M):
    """outside 1..64 (0 = the whole 160-type catalog) the probes' option lists do not fit their 64-bit rows"""
    cp = fuzzgen.fuzz_consolidation(EC.sample(golden, 160, 9500), 9500, n_nodes=20, n_pods=80)
    cp.cluster.max_instance_types = M
    with pytest.raises(native.KpError) as e:
        TGC.device_probes(ctx, cp, abi.KP_CONSOLIDATE_SINGLE)
    assert e.value.status == abi.KP_E_UNSUPPORTED and "1..64" in str(e.value)
    cp.cluster.max_instance_types = 60
    consolidation_parity(ctx, cp)


# ================================================================================================================
# D. pod and node counts
# ================================================================================================================
@pytest.fixture(scope="module")
def count_base(golden):
    return fuzzgen.fuzz_problem(EC.sample(golden, 160, 9600), 9600, n_pods=300)


@pytest.mark.parametrize("P", [0, 1, 2, 63, 64, 65, 255, 256, 257])
def test_pod_counts(ctx, count_base, golden, P):
    prob = synth.subsample(count_base, P)
    assert prob.pods.n == P
    dev = solve_parity(ctx, prob)
    if P == 0:
        assert dev[0].n_nodeclaims == 0
        solve_parity(ctx, valid_problem(golden))


@pytest.mark.parametrize("P", [1, 64, 65])
def test_pod_counts_equal_creation_time(ctx, count_base, P):
    """every creation timestamp equal: the queue's UID order decides"""
    prob = synth.subsample(count_base, P)
    prob.pods.creation_ns[:] = prob.pods.creation_ns[0]
    prob.pods.uids = prob.pods.uids[::-1]
    solve_parity(ctx, prob)


def test_no_pod_schedules(ctx, count_base):
    prob = synth.subsample(count_base, 100)
    prob.pods.requests[:, model.RIDX["cpu"]] = 10 ** 9  # a million cores each
    dev = solve_parity(ctx, prob)
    assert dev[0].n_nodeclaims == 0 and (dev[0].pod_result == -1).all()


@pytest.mark.parametrize("E", [1, 63, 64, 65, 128, 129])
def test_existing_node_counts(ctx, golden, E):
    """E existing nodes (EW = ceil(E / 64) node words): the Solve, and a consolidation pass with every node a candidate"""
    sub = EC.sample(golden, 160, 9700)
    solve_parity(ctx, fuzzgen.fuzz_problem(sub, 9700 + E, n_pods=200, n_existing=E))
    consolidation_parity(ctx, fuzzgen.fuzz_consolidation(sub, 9800 + E, n_nodes=E, n_pods=200, n_candidates=E))


def test_63_nodepools(ctx, golden):
    sub = EC.sample(golden, 160, 9900)
    prob = fuzzgen.fuzz_problem(sub, 9900, n_pods=200, n_classes=20, n_pools=63)
    assert len(prob.nodepools) == 63
    solve_parity(ctx, prob)
    consolidation_parity(ctx, fuzzgen.fuzz_consolidation(sub, 9901, n_nodes=30, n_pods=150, n_pools=63))


# ================================================================================================================
# E. the prepare split on the device path
# ================================================================================================================
def test_prepare_split_feeds_device(golden):
    """kp_solve_prepare with its pod_rows / pod_keys passes on two threads (KPSIM_PREP_SPLIT_MIN=1, read once per
    process: a child) gives the device the same rows: every result digest equals the oracle's"""
    import prep_split_child
    env = dict(os.environ, KPSIM_PREP_SPLIT_MIN="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "prep_split_child.py")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    probs = prep_split_child.prep_split_problems(golden)
    assert sorted(got) == sorted(probs)
    for name, prob in probs.items():
        assert got[name] == parity.result_digest(parity.run_oracle(prob)), name
