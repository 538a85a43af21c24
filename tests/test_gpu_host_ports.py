"""GPU: host ports in Solve (kpsim.h kp_host_port; DESIGN.md §4 "Host ports").

Hand cases with plain expectations, then seeded fuzz families bit-exact against the reference of
tests/hostport_cases.py: the CPU oracle run on the transformed problem (each port bit a spare resource axis with one
unit of capacity).  Every result is also checked for the invariant that no NodeClaim or node holds two conflicting pods.
Word edges (65 / 256 / 257 distinct ports, a 4,200-pod same-port Deployment) have plain expectations: the oracle has
only seven spare axes.  Consolidation: three hand cases, then 8 fuzz seeds (SINGLE, MULTI, BOTH, the command, a
multi-device ctx) against the oracle's probes and command on the transformed cluster.
"""
import numpy as np
import pytest

import hostport_cases as HP
import parity
from kpsim import abi, model, native, synth
from kpsim.abi import KP_POD_EXISTING
from kpsim.model import HostPort, PodClass

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fakes(fake):
    return HP.derive_catalogs(fake)


@pytest.fixture(scope="module")
def cats(golden):
    return HP.sub_catalogs(golden)


def solve(ctx, fakes, prob, check_oracle=True):
    """The device result of prob over the derived fake catalog; checked against the transformed oracle and the invariant."""
    dprob = HP.device_problem(prob, fakes[0])
    dev = parity.run_device(ctx, dprob)
    HP.assert_no_conflict(dprob, dev[0])
    if check_oracle:
        parity.assert_same(dev, HP.run_oracle(HP.transform(dprob, fakes[1])))
    return dev[0]


def small_pods(classes):
    return synth.pods_from_specs([(c, {"cpu": "100m"}) for c in classes])


def problem(fake, classes, pod_classes, pools=None, existing=None):
    return model.Problem(fake, pools or [synth.default_nodepool()], classes, small_pods(pod_classes), existing or [])


# ------------------------------------------------------------------------------------------------
# hand cases
# ------------------------------------------------------------------------------------------------
def test_same_port_two_nodeclaims(ctx, fake, fakes):
    """Two pods that bind the same hostPort cannot share a NodeClaim (fails without host-port support: 1 NodeClaim)."""
    r = solve(ctx, fakes, problem(fake, [PodClass(host_ports=[HostPort(80)])], [0, 0]))
    assert r.n_nodeclaims == 2 and sorted(r.pod_result.tolist()) == [0, 1]


def test_same_port_two_classes_two_nodeclaims(ctx, fake, fakes):
    cls = [PodClass(host_ports=[HostPort(80)]), PodClass(host_ports=[HostPort(80), HostPort(81)])]
    r = solve(ctx, fakes, problem(fake, cls, [0, 1]))
    assert r.n_nodeclaims == 2


def test_different_ports_one_nodeclaim(ctx, fake, fakes):
    cls = [PodClass(host_ports=[HostPort(80)]), PodClass(host_ports=[HostPort(81)])]
    r = solve(ctx, fakes, problem(fake, cls, [0, 1]))
    assert r.n_nodeclaims == 1 and r.pod_result.tolist() == [0, 0]


def test_tcp_and_udp_one_nodeclaim(ctx, fake, fakes):
    cls = [PodClass(host_ports=[HostPort(53, "TCP")]), PodClass(host_ports=[HostPort(53, "UDP")])]
    r = solve(ctx, fakes, problem(fake, cls, [0, 1]))
    assert r.n_nodeclaims == 1


def test_specific_ips_then_wildcard(ctx, fake, fakes):
    cls = [PodClass(host_ports=[HostPort(80, "TCP", "10.0.0.1")]), PodClass(host_ports=[HostPort(80, "TCP", "10.0.0.2")]),
           PodClass(host_ports=[HostPort(80, "TCP", "0.0.0.0")])]
    r = solve(ctx, fakes, problem(fake, cls[:2], [0, 1]))
    assert r.n_nodeclaims == 1
    r = solve(ctx, fakes, problem(fake, cls, [0, 1, 2]))
    assert r.n_nodeclaims == 2
    # the wildcard pod is alone on its NodeClaim
    assert (r.pod_result == r.pod_result[2]).sum() == 1 and r.pod_result[0] == r.pod_result[1]


def test_daemonset_port_sends_pod_to_next_pool(ctx, fake, fakes):
    """A pod whose port a NodePool's daemonset holds is unschedulable on that pool and lands on the next one."""
    first = synth.default_nodepool("first", weight=50)
    first.daemon_host_ports = [HostPort(9100)]
    second = synth.default_nodepool("second", weight=10)
    cls = [PodClass(), PodClass(host_ports=[HostPort(9100)])]
    # the port-free pod opens a NodeClaim of the heavier pool; the port pod can join neither it nor a new one of its pool
    r = solve(ctx, fakes, problem(fake, cls, [0, 1], pools=[first, second]))
    assert r.n_nodeclaims == 2 and r.pod_result.tolist() == [0, 1]
    assert r.nodeclaim_nodepool.tolist() == [0, 1]
    # ... and unschedulable when no other pool exists
    r = solve(ctx, fakes, problem(fake, cls, [0, 1], pools=[first]))
    assert r.pod_result.tolist() == [0, -1]


def _node(name, it, ports=()):
    avail = np.array(it.allocatable, np.int64).copy()
    lab = {model.ZONE: "test-zone-1a", model.CAPACITY_TYPE: "on-demand", model.INSTANCE_TYPE: it.name}
    return model.ExistingNode(name=name, labels=lab, available=avail, host_ports=list(ports))


def test_existing_node_holding_the_port_is_skipped(ctx, fake, fakes):
    nodes = [_node("node-0", fake[0], [HostPort(80)]), _node("node-1", fake[0])]
    cls = [PodClass(host_ports=[HostPort(80, "TCP", "10.1.2.3")]), PodClass()]
    r = solve(ctx, fakes, problem(fake, cls, [0, 1], existing=nodes))
    assert r.pod_result.tolist() == [KP_POD_EXISTING(1), KP_POD_EXISTING(0)]
    r = solve(ctx, fakes, problem(fake, cls, [0], existing=nodes[:1]))
    assert r.pod_result.tolist() == [0] and r.n_nodeclaims == 1


def test_two_same_port_pods_one_free_node(ctx, fake, fakes):
    """One pod takes the node, the other a NodeClaim; a third, port-free pod still fits the node afterwards."""
    cls = [PodClass(host_ports=[HostPort(443)]), PodClass()]
    r = solve(ctx, fakes, problem(fake, cls, [0, 0, 1], existing=[_node("node-0", fake[0])]))
    assert sorted(r.pod_result[:2].tolist()) == [KP_POD_EXISTING(0), 0] and r.n_nodeclaims == 1
    assert r.pod_result[2] == KP_POD_EXISTING(0)


def test_zero_ports_is_the_port_free_solve(ctx, golden):
    """A problem whose tables are all empty takes the port-free path and equals the plain oracle."""
    prob = synth.subsample(synth.config2(catalog=golden), 300)
    parity.assert_same(parity.run_device(ctx, prob), parity.run_oracle(prob))
    assert ctx.kernel_times_ms()[3] > 0


def test_diagnostic_twin_with_host_ports(ctx, fake, fakes, monkeypatch):
    """KPSIM_PROFILE launches the diagnostic twin of the host-port entry point: same placements."""
    monkeypatch.setenv("KPSIM_PROFILE", "1")
    cls = [PodClass(host_ports=[HostPort(80)]), PodClass(host_ports=[HostPort(81)])]
    r = solve(ctx, fakes, problem(fake, cls, [0, 0, 1, 1]))
    assert r.n_nodeclaims == 2 and r.pod_result.tolist() == [0, 1, 0, 1]


def test_bad_tables_are_invalid(ctx, fake, fakes):
    for hp in (HostPort(0), HostPort(70000), HostPort(80, "TCP", "not-an-ip")):
        with pytest.raises(native.KpError) as e:
            solve(ctx, fakes, problem(fake, [PodClass(host_ports=[hp])], [0]), check_oracle=False)
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


def _cons_kat(fake, fakes, nodes, cand_nodes, n_pods):
    """Candidates cand_nodes with one port-80 pod each over `nodes`: (device problem, oracle problem, stripped problem)."""
    import pyoracle  # noqa: F401
    prob = HP.device_problem(problem(fake, [PodClass(host_ports=[HostPort(80)])], [0] * n_pods, existing=nodes), fakes[0])
    cands = [model.Candidate(node=j, pods=np.array([i], np.int32), price=10.0, instance_type=0, nodepool=0,
                             capacity=np.array(fakes[0][0].capacity, np.int64)) for i, j in enumerate(cand_nodes)]
    cp = model.ConsolidationProblem(prob, cands)
    return cp, HP.cons_with(cp, HP.transform(prob, fakes[1])), HP.cons_with(cp, HP.strip(prob))


def test_probe_only_fitting_node_holds_the_port(ctx, fake, fakes):
    """The candidate's pod fits one other node, whose bound pod holds its port: REPLACE or NONE, where the port-free
    twin decides DELETE."""
    import pyoracle
    nodes = [_node("node-0", fake[0], [HostPort(80)]), _node("node-1", fake[0], [HostPort(80)])]
    cp, ocp, scp = _cons_kat(fake, fakes, nodes, [0], 1)
    got = device_probes(ctx, cp, abi.KP_CONSOLIDATE_SINGLE)
    assert got["decision"][0] in (abi.KP_DECISION_REPLACE, abi.KP_DECISION_NONE) and got["n_new_nodeclaims"][0] == 1
    assert_probes_equal(got, pyoracle.consolidate(ocp, abi.KP_CONSOLIDATE_SINGLE))
    assert device_probes(ctx, scp, abi.KP_CONSOLIDATE_SINGLE)["decision"][0] == abi.KP_DECISION_DELETE


def test_probe_private_port_state(ctx, fake, fakes):
    """Two candidates with one port-80 pod each and one free node: each single-node probe moves its pod there (DELETE),
    the two-node probe can move only one (the node then holds the port for that probe alone), so it needs a NodeClaim."""
    import pyoracle
    nodes = [_node("node-0", fake[0], [HostPort(80)]), _node("node-1", fake[0], [HostPort(80)]), _node("node-2", fake[0])]
    cp, ocp, scp = _cons_kat(fake, fakes, nodes, [0, 1], 2)
    single = device_probes(ctx, cp, abi.KP_CONSOLIDATE_SINGLE)
    assert single["decision"].tolist() == [abi.KP_DECISION_DELETE, abi.KP_DECISION_DELETE]
    multi = device_probes(ctx, cp, abi.KP_CONSOLIDATE_MULTI)
    assert multi["decision"][0] != abi.KP_DECISION_DELETE and multi["n_new_nodeclaims"][0] == 1
    for mode, got in ((abi.KP_CONSOLIDATE_SINGLE, single), (abi.KP_CONSOLIDATE_MULTI, multi)):
        assert_probes_equal(got, pyoracle.consolidate(ocp, mode))
    assert device_probes(ctx, scp, abi.KP_CONSOLIDATE_MULTI)["decision"][0] == abi.KP_DECISION_DELETE


def test_probe_mutated_node_keeps_its_bound_port(ctx, fake, fakes):
    """A probe that reschedules a mutator's pod and a port pod: node-1 lacks the label the mutator's DoesNotExist
    requirement names, so the mutator's Add changes node-1's requirements and the probe re-derives node-1's
    compatibility from its copy.  The bound pod's port 80 must survive that: the port pod still cannot join node-1."""
    import pyoracle
    team = "example.com/team"
    cls = [PodClass([model.Requirement(team, "DoesNotExist")]), PodClass(host_ports=[HostPort(80)]),
           PodClass([model.Requirement(team, "In", ["a"])])]   # a positive use of the key makes class 0 a mutator
    pods = synth.pods_from_specs([(0, {"cpu": "200m"}), (1, {"cpu": "100m"})])   # the mutator is popped first
    nodes = [_node("node-0", fake[0], [HostPort(80)]), _node("node-1", fake[0], [HostPort(80)])]
    prob = HP.device_problem(model.Problem(fake, [synth.default_nodepool()], cls, pods, nodes), fakes[0])
    cand = [model.Candidate(node=0, pods=np.array([0, 1], np.int32), price=10.0, instance_type=0, nodepool=0,
                            capacity=np.array(fakes[0][0].capacity, np.int64))]
    cp = model.ConsolidationProblem(prob, cand)
    got = device_probes(ctx, cp, abi.KP_CONSOLIDATE_SINGLE)
    _, counters = ctx.consolidate_stats()
    assert counters[17] >= 1   # the probe ran with per-probe node state
    assert got["decision"][0] != abi.KP_DECISION_DELETE and got["n_new_nodeclaims"][0] == 1
    assert_probes_equal(got, pyoracle.consolidate(HP.cons_with(cp, HP.transform(prob, fakes[1])), abi.KP_CONSOLIDATE_SINGLE))
    twin = device_probes(ctx, HP.cons_with(cp, HP.strip(prob)), abi.KP_CONSOLIDATE_SINGLE)
    assert twin["decision"][0] == abi.KP_DECISION_DELETE


def _command(ctx, cp, mode):
    ctx.upload_catalog(model.CatalogView(cp.cluster.catalog))
    ctx.consolidate_prepare(model.ConsolidateInputView(cp, abi.KP_CONSOLIDATE_SINGLE))
    return ctx.consolidate_command(mode)


@pytest.mark.parametrize("seed", list(HP.CONS_SEEDS))
def test_fuzz_consolidation(ctx, cats, seed):
    """SINGLE, MULTI and BOTH probes and the command of each method against the oracle on the transformed cluster."""
    import pyoracle
    cp, ocp, _ = HP.cons_problem(cats, seed)
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
    cp, ocp, _ = HP.cons_problem(cats, 1)
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
    return [pytest.param(f, s, id="%s-%d" % (f, s)) for f, seeds in HP.FAMILY_SEEDS.items() for s in seeds]


@pytest.mark.parametrize("family,seed", _family_cases())
def test_fuzz_family(cats, family, seed):
    dprob, oprob, policy = HP.family_problem(cats, family, seed)
    c = native.Context(0, preference_policy=policy)
    try:
        dev = parity.run_device(c, dprob)
    finally:
        c.close()
    HP.assert_no_conflict(dprob, dev[0])
    parity.assert_same(dev, HP.run_oracle(oprob, policy))


# ------------------------------------------------------------------------------------------------
# word edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ports", [65, 256])
def test_many_distinct_ports(ctx, fake, fakes, n_ports):
    """n distinct ports, one class each, plus a second class on the first, the 65th and the last port: the pods that
    pairwise share a port end on different NodeClaims, all others pack together (bits in word 1 and the last word decide)."""
    ports = [1000 + i for i in range(n_ports)]
    shared = sorted({0, 64, n_ports - 1})
    cls = [PodClass(host_ports=[HostPort(p)]) for p in ports] + [PodClass(host_ports=[HostPort(ports[i])]) for i in shared]
    prob = problem(fake, cls, list(range(len(cls))))
    r = solve(ctx, fakes, prob, check_oracle=False)
    assert (r.pod_result >= 0).all()
    for k, i in enumerate(shared):
        assert r.pod_result[i] != r.pod_result[n_ports + k]
    # first fit: the n distinct ports share the first NodeClaim, the three repeats the second
    assert r.n_nodeclaims == 2
    assert len(set(r.pod_result[:n_ports].tolist())) == 1 and len(set(r.pod_result[n_ports:].tolist())) == 1


def test_257_distinct_ports_are_refused(ctx, fake, fakes):
    cls = [PodClass(host_ports=[HostPort(1000 + i)]) for i in range(257)]
    with pytest.raises(native.KpError) as e:
        solve(ctx, fakes, problem(fake, cls, list(range(257))), check_oracle=False)
    assert e.value.status == abi.KP_E_UNSUPPORTED and "257" in str(e.value)


def test_same_port_deployment_is_node_dense(ctx, fake, fakes):
    """4,200 pods of one port-carrying class: 4,200 NodeClaims of one pod each — more than the first plan's 4,096, so
    the port bit's pod count must enter the NodeClaim plan (the node-dense layout): one prepare / execute / fetch, which
    unlike kp_solve never plans again after an overflow, must hold them all."""
    n = 4200
    prob = problem(fake, [PodClass(host_ports=[HostPort(8080)])], [0] * n)
    # the split form has no overflow rerun: without the port term in the plan, fetch reports the overflow
    dprob = HP.device_problem(prob, fakes[0])
    ctx.upload_catalog(model.CatalogView(dprob.catalog))
    ctx.prepare(model.SolveInputView(dprob))
    ctx.execute()
    out = model.OutputBuffers(n, n + 1, (n + 1) * 60)
    ctx.fetch(out)
    assert out.results().n_nodeclaims == n
    r = solve(ctx, fakes, prob, check_oracle=False)
    assert r.n_nodeclaims == n
    assert sorted(r.pod_result.tolist()) == list(range(n))
    assert (np.asarray(r.nodeclaim_n_pods) == 1).all()
