"""CPU: host ports — the bit encoding against the conflict rule, the marshalling of the three CSR side tables, and the
non-vacuity of every fuzz family the GPU tests use (hostport_cases.family_problem), proven with the oracle alone: the
oracle on the transformed problem (hostport_cases.transform) must differ from the port-stripped run often enough, and
pods must still land on existing nodes after a port pod did.
"""
import ctypes as C

import numpy as np
import pytest

import hostport_cases as HP
import parity
from kpsim import abi, model
from kpsim.model import HostPort


# ------------------------------------------------------------------------------------------------
# the rule and the encoding
# ------------------------------------------------------------------------------------------------
def test_conflict_rule_cases():
    tcp80 = HostPort(80)
    assert HP.entries_conflict(tcp80, HostPort(80, "TCP", "0.0.0.0"))
    assert HP.entries_conflict(tcp80, HostPort(80, "TCP", "::"))
    assert HP.entries_conflict(tcp80, HostPort(80, "TCP", "10.0.0.1"))              # wildcard with a specific IP
    assert not HP.entries_conflict(HostPort(80, "TCP", "10.0.0.1"), HostPort(80, "TCP", "10.0.0.2"))
    assert HP.entries_conflict(HostPort(80, "TCP", "10.0.0.1"), HostPort(80, "TCP", "10.0.0.1"))
    assert not HP.entries_conflict(tcp80, HostPort(80, "UDP"))                       # UDP against TCP
    assert not HP.entries_conflict(tcp80, HostPort(81))
    assert HP.entries_conflict(HostPort(80, "TCP", "fd00::1"), HostPort(80, "TCP", "FD00:0::1"))
    assert HP.entries_conflict(HostPort(80, "TCP", "10.0.0.1"), HostPort(80, "TCP", "::ffff:10.0.0.1"))


@pytest.mark.parametrize("seed", range(40))
def test_encoding_matches_rule(seed):
    """own(a) & own(b) != 0 iff the sets conflict, over random entry sets drawn from few ports, protocols and IPs
    (unspecified ones in all three spellings)."""
    rng = np.random.Generator(np.random.PCG64(9000 + seed))
    ips = ["", "0.0.0.0", "::", "10.0.0.1", "10.0.0.2", "fd00::1"]
    rows = [[HostPort(int(rng.choice([80, 443, 53])), str(rng.choice(["TCP", "UDP", "SCTP"])), str(rng.choice(ips)))
             for _ in range(int(rng.integers(0, 4)))] for _ in range(24)]
    n, own = HP.encode(rows)
    assert n <= sum(len(r) for r in rows) * 2
    for i, a in enumerate(rows):
        for j, b in enumerate(rows):
            assert bool(own[i] & own[j]) == HP.sets_conflict(a, b), (a, b)


# ------------------------------------------------------------------------------------------------
# marshalling
# ------------------------------------------------------------------------------------------------
def _small_problem(fake):
    from kpsim import synth
    pods = synth.pods_from_specs([(0, {"cpu": "1"}), (1, {"cpu": "1"}), (2, {"cpu": "1"})])
    classes = [model.PodClass(host_ports=[HostPort(80), HostPort(53, "UDP", "10.0.0.1")]), model.PodClass(),
               model.PodClass(host_ports=[HostPort(8080, "SCTP", "::")])]
    np0, np1 = synth.default_nodepool(), synth.default_nodepool()
    np1.name = "other"
    np1.daemon_host_ports = [HostPort(9100)]
    ex = [model.ExistingNode("n0", {}, np.zeros(model.R, np.int64)),
          model.ExistingNode("n1", {}, np.zeros(model.R, np.int64), host_ports=[HostPort(80, "TCP", "10.0.0.2")])]
    return model.Problem(fake, [np0, np1], classes, pods, ex)


def test_csr_tables_round_trip(fake):
    prob = _small_problem(fake)
    v = model.SolveInputView(prob).view

    def want(rows):
        return [[(h.ip, abi.PROTOCOLS[h.protocol], h.port) for h in r] for r in rows]
    assert abi.host_port_rows(v.class_port_offsets, v.class_ports, 3) == want([c.host_ports for c in prob.classes])
    assert abi.host_port_rows(v.nodepool_port_offsets, v.nodepool_ports, 2) == want([[], [HostPort(9100)]])
    assert abi.host_port_rows(v.existing_port_offsets, v.existing_ports, 2) == want([e.host_ports for e in prob.existing])
    assert [v.class_port_offsets[i] for i in range(4)] == [0, 2, 2, 3]


def test_no_ports_marshal_as_null(fake):
    """A problem without host ports leaves the six fields NULL: the zero-initialised input of every existing caller."""
    prob = HP.strip(_small_problem(fake))
    v = model.SolveInputView(prob).view
    for f in ("class_port_offsets", "class_ports", "nodepool_port_offsets", "nodepool_ports", "existing_port_offsets",
              "existing_ports"):
        assert not getattr(v, f), f
    cv = model.ConsolidateInputView(model.ConsolidationProblem(prob, []), abi.KP_CONSOLIDATE_SINGLE).view
    assert not cv.cluster.class_port_offsets


def test_struct_tail_layout():
    """The tables are appended: every earlier field of kp_solve_input keeps its offset."""
    names = [f[0] for f in abi.kp_solve_input._fields_]
    assert names[-6:] == ["class_port_offsets", "class_ports", "nodepool_port_offsets", "nodepool_ports",
                          "existing_port_offsets", "existing_ports"]
    assert abi.kp_solve_input.bound_class.offset + C.sizeof(C.c_void_p) == abi.kp_solve_input.class_port_offsets.offset
    assert C.sizeof(abi.kp_host_port) == 16


# ------------------------------------------------------------------------------------------------
# the fuzz families of the GPU tests are not vacuous
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cats(golden):
    return HP.sub_catalogs(golden)


def _differs(a, b):
    try:
        parity.assert_same(a, b)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("family", ["plain", "existing", "topology", "pref_respect", "pref_ignore", "reserved"])
def test_family_is_not_vacuous(cats, family):
    """In at least half of the family's seeds the host ports change the Solve's result."""
    seeds = HP.FAMILY_SEEDS[family]
    changed = 0
    for seed in seeds:
        dprob, oprob, policy = HP.family_problem(cats, family, seed)
        assert any(pc.host_ports for pc in dprob.classes)
        with_ports = HP.run_oracle(oprob, policy)
        without = HP.run_oracle(HP.strip(dprob), policy)
        HP.assert_no_conflict(dprob, with_ports[0])
        changed += _differs(with_ports, without)
    assert 2 * changed >= len(seeds), (changed, len(seeds))


def test_existing_family_carries_per_node_port_state(cats):
    """The state the device must carry is per node: after a port pod landed on node j, some later pod that does not
    conflict with it still lands on j, and some later pod whose class conflicts with it was offered j (j was compatible
    and had room before the port pod came) and went elsewhere."""
    joined = skipped = 0
    for seed in HP.FAMILY_SEEDS["existing"]:
        dprob, oprob, policy = HP.family_problem(cats, "existing", seed)
        r = HP.run_oracle(oprob, policy)[0]
        ports = [dprob.classes[int(c)].host_ports for c in dprob.pods.class_id]
        first = {}   # node -> (order, pod) of the first port pod placed on it
        for p in np.argsort(r.pod_order):
            if r.pod_order[p] >= 0 and r.pod_result[p] <= -2 and ports[p]:
                first.setdefault(int(r.pod_result[p]), (int(r.pod_order[p]), int(p)))
        for node, (o, pp) in first.items():
            for p in range(dprob.pods.n):
                if r.pod_order[p] <= o:
                    continue
                if r.pod_result[p] == node and not HP.sets_conflict(ports[pp], ports[p]):
                    joined += 1
                if r.pod_result[p] != node and HP.sets_conflict(ports[pp], ports[p]) and \
                        dprob.pods.class_id[p] == dprob.pods.class_id[pp]:
                    skipped += 1   # same class, same requests: node j took pp, so it was offered to p first
    assert joined >= 1 and skipped >= 1, (joined, skipped)


# ------------------------------------------------------------------------------------------------
# consolidation family
# ------------------------------------------------------------------------------------------------
def test_consolidation_family_is_not_vacuous(cats):
    """With the oracle alone: in each mode some probe's row differs from the port-stripped run, and at least a quarter
    of all probes still decide DELETE or REPLACE with host ports (the family is not too dense to test anything)."""
    import pyoracle
    total = decided = 0
    for mode in (abi.KP_CONSOLIDATE_SINGLE, abi.KP_CONSOLIDATE_MULTI):
        differ = 0
        for seed in HP.CONS_SEEDS:
            _, ocp, scp = HP.cons_problem(cats, seed)
            a, b = pyoracle.consolidate(ocp, mode), pyoracle.consolidate(scp, mode)
            assert len(a) == len(b)
            differ += sum(tuple(x) != tuple(y) for x, y in zip(a.tolist(), b.tolist()))
            total += len(a)
            decided += int((a["decision"] != abi.KP_DECISION_NONE).sum())
        assert differ >= 1, mode
    assert 4 * decided >= total, (decided, total)


def test_257_ports_refused_by_the_host_layer():
    """The host layer over the CPU stand-in of the HIP runtime (tests/cpu_stub) reaches kp_solve_prepare: 257 distinct
    ports are KP_E_UNSUPPORTED with the count in the message, 256 are accepted.  Run in a child process, which loads the
    stub library instead of libkpsim.so."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    stub = os.path.join(here, "cpu_stub")
    subprocess.check_call(["make", "-s", "-C", stub, "build/libkpsim_stub.so"], stdout=subprocess.DEVNULL)
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from kpsim import abi, catalog, model, native, synth\n"
        "from kpsim.model import HostPort, PodClass\n"
        "fake = catalog.fake_catalog(fx=catalog.load_fixtures())\n"
        "ctx = native.Context(0)\n"
        "ctx.upload_catalog(model.CatalogView(fake))\n"
        "for n in (256, 257):\n"
        "    cls = [PodClass(host_ports=[HostPort(1000 + i)]) for i in range(n)]\n"
        "    pods = synth.pods_from_specs([(i, {'cpu': '100m'}) for i in range(n)])\n"
        "    prob = model.Problem(fake, [synth.default_nodepool()], cls, pods)\n"
        "    try:\n"
        "        ctx.prepare(model.SolveInputView(prob))\n"
        "        print(n, 'ok')\n"
        "    except native.KpError as e:\n"
        "        print(n, e.status, '257' in str(e))\n"
    ) % (os.path.join(os.path.dirname(here), "karpenter-provider-aws_amd"), here)
    env = dict(os.environ, KPSIM_LIB=os.path.join(stub, "build", "libkpsim_stub.so"), KP_STUB_DEVICES="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:2] == ["256 ok", "257 %d True" % abi.KP_E_UNSUPPORTED], r.stdout
