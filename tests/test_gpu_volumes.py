"""GPU: volume attach limits in Solve (kpsim.h kp_volume / kp_volume_limit; DESIGN.md §4 "Volume limits").

Hand cases with plain expectations (e1-e8, the two caps and the malformed tables), then seeded fuzz families bit-exact
against the reference of tests/volume_cases.py: the CPU oracle run on the transformed problem (each limited driver a
spare resource axis).  Every result is also replayed against the restated ExceedsLimits rule.  Consolidation: three hand
clusters, then 8 fuzz seeds (SINGLE, MULTI, BOTH, the command, a multi-device ctx) against the oracle's probes and
command on the transformed cluster.
"""
import numpy as np
import pytest

import parity
import volume_cases as VC
from kpsim import abi, model, native, synth
from kpsim.abi import KP_POD_EXISTING
from kpsim.model import HostPort, PodClass
from volume_cases import EBS, EFS, PD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fakes(fake):
    return VC.derive_catalogs(fake)


@pytest.fixture(scope="module")
def cats(golden):
    return VC.sub_catalogs(golden)


def solve(ctx, fakes, prob, check_oracle=False, drop=()):
    """The device result of prob over the derived fake catalog, replayed against the rule; check_oracle: also compared
    with the transformed oracle (problems whose claims are private, or of family A / B)."""
    dprob = VC.device_problem(prob, fakes[0])
    dev = parity.run_device(ctx, dprob)
    VC.assert_within_limits(dprob, dev[0])
    if check_oracle:
        parity.assert_same(dev, VC.run_oracle(VC.transform(dprob, fakes[1], drop)))
    return dev[0]


def problem(fake, volumes, existing=(), classes=None, pod_classes=None, cpu=None):
    """One pod per entry of volumes, popped in list order (descending cpu unless given)."""
    n = len(volumes)
    cpu = cpu or [100 * (n - i) for i in range(n)]
    pods = synth.pods_from_specs([((pod_classes or [0] * n)[i], {"cpu": "%dm" % cpu[i]}) for i in range(n)])
    pods.volumes = [list(v) for v in volumes]
    return model.Problem(fake, [synth.default_nodepool()], classes or [PodClass()], pods, list(existing))


def node(name, it, volumes=(), limits=None, zone="test-zone-1a", ports=()):
    avail = np.array(it.allocatable, np.int64).copy()
    lab = {model.ZONE: zone, model.CAPACITY_TYPE: "on-demand", model.INSTANCE_TYPE: it.name}
    return model.ExistingNode(name=name, labels=lab, available=avail, volumes=list(volumes), volume_limits=dict(limits or {}),
                              host_ports=list(ports))


def pvc(i):
    return (EBS, "default/pvc-%d" % i)


# ------------------------------------------------------------------------------------------------
# hand cases
# ------------------------------------------------------------------------------------------------
def test_e1_storage_suite_second_pod_takes_a_second_node(ctx, fake, fakes):
    """An EBS limit of 1: pod 0 opens a NodeClaim; with that node in the cluster (claim 0 mounted), pod 1 with its own
    claim cannot join it and opens another (fails without volume limits: pod 1 lands on the node).  Limit 2: it joins."""
    r = solve(ctx, fakes, problem(fake, [[pvc(0)]]), check_oracle=True)
    assert r.n_nodeclaims == 1 and r.pod_result.tolist() == [0]
    n0 = node("node-0", fake[0], [pvc(0)], {EBS: 1})
    r = solve(ctx, fakes, problem(fake, [[pvc(1)]], [n0]), check_oracle=True)
    assert r.n_nodeclaims == 1 and r.pod_result.tolist() == [0]
    n0 = node("node-0", fake[0], [pvc(0)], {EBS: 2})
    r = solve(ctx, fakes, problem(fake, [[pvc(1)]], [n0]), check_oracle=True)
    assert r.n_nodeclaims == 0 and r.pod_result.tolist() == [KP_POD_EXISTING(0)]


def test_e2_shared_claim_counts_once(ctx, fake, fakes):
    """Three pods of a Deployment share one claim; the node's limit is 1: the second pod finds the claim mounted by the
    first (the dynamic union), so all three land on the node.  A fourth pod with one more claim is refused by it."""
    shared = (EBS, "default/shared")
    n0 = node("node-0", fake[0], [], {EBS: 1})
    r = solve(ctx, fakes, problem(fake, [[shared]] * 3 + [[shared, pvc(9)]], [n0], cpu=[200, 200, 200, 100]))
    assert r.pod_result.tolist() == [KP_POD_EXISTING(0)] * 3 + [0] and r.n_nodeclaims == 1
    # limit 2: the fourth joins too
    n0 = node("node-0", fake[0], [], {EBS: 2})
    r = solve(ctx, fakes, problem(fake, [[shared]] * 3 + [[shared, pvc(9)]], [n0], cpu=[200, 200, 200, 100]))
    assert r.pod_result.tolist() == [KP_POD_EXISTING(0)] * 4


def test_e3_node_over_its_limit_refuses_a_pod_without_volumes(ctx, fake, fakes):
    over = node("node-0", fake[0], [pvc(0), pvc(1)], {EBS: 1})
    r = solve(ctx, fakes, problem(fake, [[]], [over]))
    assert r.pod_result.tolist() == [0] and r.n_nodeclaims == 1
    r = solve(ctx, fakes, problem(fake, [[]], [over, node("node-1", fake[0], [pvc(2)], {EBS: 1})]))
    assert r.pod_result.tolist() == [KP_POD_EXISTING(1)]
    at = node("node-0", fake[0], [pvc(0), pvc(1)], {EBS: 2})   # at the limit, not over it
    r = solve(ctx, fakes, problem(fake, [[]], [at]), check_oracle=True)
    assert r.pod_result.tolist() == [KP_POD_EXISTING(0)]


def test_e4_two_drivers_one_limited(ctx, fake, fakes):
    """EBS is at its limit on the node, EFS has none: three EFS claims join the node, one EBS claim does not."""
    n0 = node("node-0", fake[0], [pvc(0), (EFS, "default/fs-0")], {EBS: 1})
    vols = [[(EFS, "default/fs-%d" % i) for i in (1, 2, 3)], [pvc(1)], [(EFS, "default/fs-4"), pvc(2)]]
    r = solve(ctx, fakes, problem(fake, vols, [n0]), check_oracle=True)
    assert r.pod_result.tolist() == [KP_POD_EXISTING(0), 0, 0]
    # a limit on the other driver alone (PD: 0) does not touch EBS pods, and refuses a PD pod
    n0 = node("node-0", fake[0], [pvc(0)], {PD: 0})
    r = solve(ctx, fakes, problem(fake, [[pvc(1), pvc(2)], [(PD, "default/pd-0")]], [n0]), check_oracle=True)
    assert r.pod_result.tolist() == [KP_POD_EXISTING(0), 0]


def test_e5_mounted_claim_fits_at_the_limit(ctx, fake, fakes):
    n0 = node("node-0", fake[0], [pvc(0)], {EBS: 1})
    r = solve(ctx, fakes, problem(fake, [[pvc(0)], [pvc(0), pvc(1)]], [n0]), check_oracle=True, drop=[pvc(0)[1]])
    assert r.pod_result.tolist() == [KP_POD_EXISTING(0), 0]


def test_e6_same_shape_run_fills_the_headroom(ctx, fake, fakes):
    """Six identical one-claim pods; node-0 has headroom for exactly two, node-1 for one: the run's pending placements
    on a node count before they are flushed."""
    nodes = [node("node-0", fake[0], [pvc(100)], {EBS: 3}), node("node-1", fake[0], [], {EBS: 1}),
             node("node-2", fake[0], [pvc(101)], {EBS: 1})]
    r = solve(ctx, fakes, problem(fake, [[pvc(i)] for i in range(6)], nodes, cpu=[100] * 6), check_oracle=True)
    assert r.pod_result.tolist() == [KP_POD_EXISTING(0)] * 2 + [KP_POD_EXISTING(1)] + [0] * 3 and r.n_nodeclaims == 1


def test_e7_topology_pod_with_a_claim(ctx, fake, fakes):
    """Zonal spread over a cluster: the block's existing-node walk applies the volume check and commits the claims."""
    spread = model.TopologyTerm("spread", model.ZONE, [model.Requirement("app", "In", ["db"])])
    cls = [PodClass(labels={"app": "db"}, topology=[spread])]
    nodes = [node("node-0", fake[0], [], {EBS: 1}, "test-zone-1a"), node("node-1", fake[0], [], {EBS: 1}, "test-zone-1a"),
             node("node-2", fake[0], [pvc(100)], {EBS: 2}, "test-zone-1b")]
    r = solve(ctx, fakes, problem(fake, [[pvc(i)] for i in range(5)], nodes, classes=cls, cpu=[100] * 5), check_oracle=True)
    on = [int((r.pod_result == KP_POD_EXISTING(j)).sum()) for j in range(3)]
    assert max(on) == 1 and sum(on) >= 2 and r.n_nodeclaims >= 1   # every node has headroom for one claim
    # the same pods without limits: some node takes a second pod
    free = [node(n.name, fake[0], n.volumes, {}, n.labels[model.ZONE]) for n in nodes]
    r = solve(ctx, fakes, problem(fake, [[pvc(i)] for i in range(5)], free, classes=cls, cpu=[100] * 5), check_oracle=True)
    assert max(int((r.pod_result == KP_POD_EXISTING(j)).sum()) for j in range(3)) >= 2


def test_e8_port_pod_and_volume_pod(ctx, fake, fakes):
    """Host ports and volumes in one Solve: the node holds port 80 and has room for one more EBS claim."""
    cls = [PodClass(host_ports=[HostPort(80)]), PodClass()]
    n0 = node("node-0", fake[0], [pvc(100)], {EBS: 2}, ports=[HostPort(80)])
    r = solve(ctx, fakes, problem(fake, [[], [pvc(0)], [pvc(1)]], [n0], classes=cls, pod_classes=[0, 1, 1]))
    assert r.pod_result.tolist() == [0, KP_POD_EXISTING(0), 0] and r.n_nodeclaims == 1


def test_unlimited_drivers_are_dropped(ctx, fake, fakes):
    """Claims of drivers without a limit anywhere change nothing: the result of the volume-stripped problem."""
    n0 = node("node-0", fake[0], [(EFS, "default/fs-0")])
    prob = problem(fake, [[(EFS, "default/fs-%d" % i), (PD, "default/pd-%d" % i)] for i in range(1, 5)], [n0])
    r = solve(ctx, fakes, prob)
    parity.assert_same((r, None), (solve(ctx, fakes, VC.strip(prob)), None), check_reqs=False)
    assert r.pod_result.tolist() == [KP_POD_EXISTING(0)] * 4


def test_diagnostic_twin_with_volumes(ctx, fake, fakes, monkeypatch):
    monkeypatch.setenv("KPSIM_PROFILE", "1")
    n0 = node("node-0", fake[0], [pvc(100)], {EBS: 2})
    r = solve(ctx, fakes, problem(fake, [[pvc(0)], [pvc(1)]], [n0]), check_oracle=True)
    assert r.pod_result.tolist() == [KP_POD_EXISTING(0), 0]


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def _prepare(ctx, fakes, prob, patch=None):
    dprob = VC.device_problem(prob, fakes[0])
    ctx.upload_catalog(model.CatalogView(dprob.catalog))
    iv = model.SolveInputView(dprob)
    if patch:
        patch(iv.view)
    ctx.prepare(iv)


def test_nine_limited_drivers_are_refused(ctx, fake, fakes):
    lim = {"drv-%d" % i: 4 for i in range(9)}
    with pytest.raises(native.KpError) as e:
        _prepare(ctx, fakes, problem(fake, [[pvc(0)]], [node("node-0", fake[0], [], lim)]))
    assert e.value.status == abi.KP_E_UNSUPPORTED and "9" in str(e.value)
    lim.pop("drv-8")
    _prepare(ctx, fakes, problem(fake, [[pvc(0)]], [node("node-0", fake[0], [], lim)]))


def test_257_shared_claims_are_refused(ctx, fake, fakes):
    n0 = node("node-0", fake[0], [], {EBS: 1000})
    with pytest.raises(native.KpError) as e:
        _prepare(ctx, fakes, problem(fake, [[pvc(i) for i in range(257)]] * 2, [n0]))
    assert e.value.status == abi.KP_E_UNSUPPORTED and "257" in str(e.value)
    # 256 shared claims: both pods land on the node, which then holds 256 claims
    r = solve(ctx, fakes, problem(fake, [[pvc(i) for i in range(256)]] * 2, [node("node-0", fake[0], [], {EBS: 256})]))
    assert r.pod_result.tolist() == [KP_POD_EXISTING(0)] * 2


def _set(table, i, field, v):
    def f(view):
        setattr(getattr(view, table)[i], field, v)
    return f


def _same_id(driver):
    def f(view):
        view.pod_volumes[1].id = view.pod_volumes[0].id
        view.pod_volumes[1].driver = driver
    return f


@pytest.mark.parametrize("patch", [_set("pod_volumes", 0, "driver", 7), _set("pod_volumes", 0, "driver", -1),
                                   _set("existing_volumes", 0, "driver", 7), _set("existing_limits", 0, "limit", -1),
                                   _set("existing_limits", 0, "driver", 9), _set("pod_volumes", 0, "id", -1),
                                   _same_id(0), _same_id(1)],
                         ids=["pod-driver-range", "pod-driver-negative", "node-driver-range", "negative-limit",
                              "limit-driver-range", "negative-id", "duplicate-in-row", "one-id-two-drivers"])
def test_malformed_tables_are_invalid(ctx, fake, fakes, patch):
    prob = problem(fake, [[pvc(0), pvc(1)]], [node("node-0", fake[0], [(PD, "default/pd-0")], {EBS: 3})])
    _prepare(ctx, fakes, prob)   # well-formed as built
    with pytest.raises(native.KpError) as e:
        _prepare(ctx, fakes, prob, patch)
    assert e.value.status == abi.KP_E_INVALID


# ------------------------------------------------------------------------------------------------
# consolidation
# ------------------------------------------------------------------------------------------------
PROBE_FIELDS = ["decision", "valid", "n_new_nodeclaims", "n_replacement_types", "n_pods", "candidate_price",
                "replacement_price"]
CMD_FIELDS = ["decision", "mode", "probe", "candidates", "n_replacement_types", "candidate_price", "replacement_price",
              "nodepool", "type_ids", "requirements", "n_reserved"]


def assert_probes_equal(dev, orc):
    assert len(dev) == len(orc)
    for f in PROBE_FIELDS:
        np.testing.assert_array_equal(dev[f], orc[f], err_msg=f)
    done = orc["n_new_nodeclaims"] < 2
    np.testing.assert_array_equal(dev["all_scheduled"][done], orc["all_scheduled"][done], err_msg="all_scheduled")


def device_probes(ctx, cp, mode):
    ctx.upload_catalog(model.CatalogView(cp.cluster.catalog))
    return ctx.consolidate(model.ConsolidateInputView(cp, mode))


def _cons_kat(fake, fakes, nodes, volumes, cand_pods):
    """Candidate node-0 with pods cand_pods over `nodes` (node-0 mounts their claims): device and oracle problem."""
    prob = VC.device_problem(problem(fake, volumes, nodes, cpu=[100] * len(volumes)), fakes[0])
    cand = [model.Candidate(node=0, pods=np.array(cand_pods, np.int32), price=10.0, instance_type=0, nodepool=0,
                            capacity=np.array(fakes[0][0].capacity, np.int64))]
    cp = model.ConsolidationProblem(prob, cand)
    return cp


def test_probe_remaining_nodes_at_their_attach_limit(ctx, fake, fakes):
    """The candidate's pod fits every other node but for their attach limit: REPLACE or NONE where limit + 1 decides
    DELETE.  Both against the oracle on the transformed cluster."""
    import pyoracle
    for extra, want_delete in ((0, False), (1, True)):
        nodes = [node("node-0", fake[0], [pvc(0)], {EBS: 5})] + \
                [node("node-%d" % j, fake[0], [pvc(100 + j)], {EBS: 1 + extra}) for j in range(1, 6)]
        cp = _cons_kat(fake, fakes, nodes, [[pvc(0)]], [0])
        got = device_probes(ctx, cp, abi.KP_CONSOLIDATE_SINGLE)
        _, counters = ctx.consolidate_stats()
        assert counters[17] >= 1   # the probe ran with per-probe node state
        assert (got["decision"][0] == abi.KP_DECISION_DELETE) == want_delete
        if not want_delete:
            assert got["n_new_nodeclaims"][0] == 1
        ocp = VC.cons_with(cp, VC.transform(cp.cluster, fakes[1]))
        assert_probes_equal(got, pyoracle.consolidate(ocp, abi.KP_CONSOLIDATE_SINGLE))


def test_probe_shared_claim_counts_once(ctx, fake, fakes):
    """Two rescheduled pods share a claim; the only node with headroom has room for one claim: both land on it (DELETE).
    With a claim each, the second pod needs a NodeClaim."""
    full = [node("node-%d" % j, fake[0], [], {EBS: 0}) for j in range(2, 6)]
    shared = (EBS, "default/shared")
    nodes = [node("node-0", fake[0], [shared], {EBS: 5}), node("node-1", fake[0], [], {EBS: 1})] + full
    got = device_probes(ctx, _cons_kat(fake, fakes, nodes, [[shared], [shared]], [0, 1]), abi.KP_CONSOLIDATE_SINGLE)
    assert got["decision"][0] == abi.KP_DECISION_DELETE and got["n_new_nodeclaims"][0] == 0
    nodes = [node("node-0", fake[0], [pvc(0), pvc(1)], {EBS: 5}), node("node-1", fake[0], [], {EBS: 1})] + full
    got = device_probes(ctx, _cons_kat(fake, fakes, nodes, [[pvc(0)], [pvc(1)]], [0, 1]), abi.KP_CONSOLIDATE_SINGLE)
    assert got["decision"][0] != abi.KP_DECISION_DELETE and got["n_new_nodeclaims"][0] == 1


def test_probe_same_class_pods_with_different_claims(ctx, fake, fakes):
    """Two pods of one class and one size, with two claims and with one: node-1 has room for one claim, node-2 for two.
    The first pod passes node-1 by and takes node-2; the second must still be offered node-1 (what the first pod's
    claims ruled out is not ruled out for its class): DELETE, as the oracle on the transformed cluster decides."""
    import pyoracle
    nodes = [node("node-0", fake[0], [pvc(0), pvc(1), pvc(2)], {EBS: 5}), node("node-1", fake[0], [pvc(100)], {EBS: 2}),
             node("node-2", fake[0], [pvc(101)], {EBS: 3})]
    nodes += [node("node-%d" % j, fake[0], [], {EBS: 0}) for j in range(3, 6)]
    cp = _cons_kat(fake, fakes, nodes, [[pvc(0), pvc(1)], [pvc(2)]], [0, 1])
    got = device_probes(ctx, cp, abi.KP_CONSOLIDATE_SINGLE)
    assert got["decision"][0] == abi.KP_DECISION_DELETE and got["n_new_nodeclaims"][0] == 0
    ocp = VC.cons_with(cp, VC.transform(cp.cluster, fakes[1]))
    assert_probes_equal(got, pyoracle.consolidate(ocp, abi.KP_CONSOLIDATE_SINGLE))


def _command(ctx, cp, mode):
    ctx.upload_catalog(model.CatalogView(cp.cluster.catalog))
    ctx.consolidate_prepare(model.ConsolidateInputView(cp, abi.KP_CONSOLIDATE_SINGLE))
    return ctx.consolidate_command(mode)


@pytest.mark.parametrize("seed", list(VC.CONS_SEEDS))
def test_fuzz_consolidation(ctx, cats, seed):
    """SINGLE, MULTI and BOTH probes and the command of each method against the oracle on the transformed cluster."""
    import pyoracle
    cp, ocp, _ = VC.cons_problem(cats, seed)
    want = {m: pyoracle.consolidate(ocp, m) for m in (abi.KP_CONSOLIDATE_SINGLE, abi.KP_CONSOLIDATE_MULTI)}
    for m in want:
        assert_probes_equal(device_probes(ctx, cp, m), want[m])
    ctx.consolidate_prepare(model.ConsolidateInputView(cp, abi.KP_CONSOLIDATE_SINGLE))
    both = ctx.consolidate_execute(abi.KP_CONSOLIDATE_BOTH, sum(len(w) for w in want.values()))
    assert_probes_equal(both, np.concatenate([want[abi.KP_CONSOLIDATE_MULTI], want[abi.KP_CONSOLIDATE_SINGLE]]))
    for m in (abi.KP_CONSOLIDATE_SINGLE, abi.KP_CONSOLIDATE_MULTI, abi.KP_CONSOLIDATE_BOTH):
        dev, orc = _command(ctx, cp, m), pyoracle.consolidate_command(ocp, m)
        for f in CMD_FIELDS:
            assert getattr(dev, f) == getattr(orc, f), (m, f, dev, orc)


def test_consolidation_multi_device_ctx(cats):
    """One ctx over two device streams (the same ordinal repeated): the sharded pass equals the oracle."""
    import pyoracle
    cp, ocp, _ = VC.cons_problem(cats, VC.CONS_MULTI_DEVICE_SEED)
    multi = native.Context(devices=[0, 0])
    try:
        for m in (abi.KP_CONSOLIDATE_SINGLE, abi.KP_CONSOLIDATE_MULTI):
            assert_probes_equal(device_probes(multi, cp, m), pyoracle.consolidate(ocp, m))
    finally:
        multi.close()


# ------------------------------------------------------------------------------------------------
# Solve fuzz, bit-exact against the transformed oracle
# ------------------------------------------------------------------------------------------------
def _family_cases():
    return [pytest.param(f, s, id="%s-%d" % (f, s)) for f, seeds in VC.FAMILY_SEEDS.items() for s in seeds]


@pytest.mark.parametrize("family,seed", _family_cases())
def test_fuzz_family(cats, family, seed):
    dprob, oprob, _, policy = VC.family_problem(cats, family, seed)
    c = native.Context(0, preference_policy=policy)
    try:
        dev = parity.run_device(c, dprob)
    finally:
        c.close()
    VC.assert_within_limits(dprob, dev[0])
    parity.assert_same(dev, VC.run_oracle(oprob, policy))
