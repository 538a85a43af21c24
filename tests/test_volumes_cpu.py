"""CPU: volume attach limits — the restated ExceedsLimits rule, the private / shared encoding against it, the marshalling
of the three CSR side tables, the host layer's refusals (over the CPU stand-in of the HIP runtime), and the non-vacuity
of every oracle-checked seed the GPU tests use (volume_cases.family_problem), proven with the oracle alone.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import parity
import volume_cases as VC
from kpsim import abi, model
from volume_cases import EBS, EFS, PD


# ------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------
def test_exceeds_limits_cases():
    ex = VC.exceeds_limits
    assert not ex([], {EBS: 1}, [(EBS, "a")])
    assert ex([(EBS, "a")], {EBS: 1}, [(EBS, "b")])                     # the storage-suite scenario
    assert not ex([(EBS, "a")], {EBS: 2}, [(EBS, "b")])
    assert not ex([(EBS, "a")], {EBS: 1}, [(EBS, "a")])                 # a set union: the claim is mounted already
    assert not ex([(EBS, "a")], {EBS: 1}, [])
    assert ex([(EBS, "a"), (EBS, "b")], {EBS: 1}, [])                   # a node over its limit refuses every pod
    assert ex([(EBS, "a"), (EBS, "b")], {EBS: 1}, [(PD, "c")])
    assert not ex([(EBS, "a"), (EBS, "b")], {}, [(EBS, "c")])           # a driver without a limit is unlimited
    assert not ex([(EBS, "a")], {EBS: 1}, [(EFS, "c"), (EFS, "d")])     # ... also beside a limited one
    assert ex([(EBS, "a")], {EBS: 1, PD: 0}, [(PD, "c")])               # a limit of 0
    assert not ex([], {EBS: 0}, [])
    assert ex([(EBS, "a")], {EBS: 2}, [(EBS, "b"), (EBS, "c")])         # two claims of one pod
    assert not ex([(EBS, "a")], {EBS: 2}, [(EBS, "b"), (PD, "c")])      # per driver, not in total


# ------------------------------------------------------------------------------------------------
# the encoding against the rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_encoding_matches_rule(seed):
    """Random pods and nodes over few claims (so many are shared), some pods with an own node (consolidation): replaying
    random Adds, the encoded test (private counts + popcount of the shared mask) decides every Add as the rule does, and
    the encoded node state after the Adds counts what the claim sets hold."""
    rng = np.random.Generator(np.random.PCG64(5000 + seed))
    drivers = [EBS, PD, EFS]
    claims = [(drivers[i % 3], "c%d" % i) for i in range(int(rng.integers(4, 30)))]

    def row(n):
        return [claims[int(i)] for i in rng.choice(len(claims), size=min(n, len(claims)), replace=False)]
    P, E = 20, 6
    pods = [row(int(rng.integers(0, 4))) for _ in range(P)]
    nodes = [row(int(rng.integers(0, 4))) for _ in range(E)]
    own = {}
    for p in range(0, P, 4):   # a reschedulable pod: its own node mounts its claims, and the pod never meets that node
        j = int(rng.integers(E))
        own[p] = j
        nodes[j] = nodes[j] + [v for v in pods[p] if v not in nodes[j]]
    limits = [{d: int(rng.integers(0, 6)) for d in drivers[:2] if rng.random() < 0.7} for _ in range(E)]
    enc = VC.Encoding(pods, nodes, limits, own)
    assert EFS not in enc.limited                      # no limit anywhere: dropped
    for c, ps in ((c, [p for p in range(P) if c in pods[p]]) for c in claims):
        if c[0] in enc.limited and len(ps) >= 2:
            assert c[1] in enc.bit
    held = [list(n) for n in nodes]
    extra = [([0] * len(enc.limited), 0) for _ in range(E)]
    for j in range(E):
        assert enc.exceeds(j) == VC.exceeds_limits(nodes[j], limits[j], [])
    for p in rng.permutation(P):
        p = int(p)
        for j in rng.permutation(E):
            j = int(j)
            if own.get(p) == j:
                continue
            want = VC.exceeds_limits(held[j], limits[j], pods[p])
            got = any(enc.lim[j][k] is not None and enc.used(k, j, p, extra[j][0][k], extra[j][1]) > enc.lim[j][k]
                      for k in range(len(enc.limited)))
            assert got == want, (p, j)
            if not want:
                held[j] = held[j] + [v for v in pods[p] if v not in held[j]]
                extra[j] = ([a + b for a, b in zip(extra[j][0], enc.pods[p][0])], extra[j][1] | enc.pods[p][1])
                break
    for j in range(E):
        for k, d in enumerate(enc.limited):
            assert enc.used(k, j, None, extra[j][0][k], extra[j][1]) == len(VC.by_driver(held[j]).get(d, ()))


# ------------------------------------------------------------------------------------------------
# marshalling
# ------------------------------------------------------------------------------------------------
def _small_problem(fake):
    from kpsim import synth
    pods = synth.pods_from_specs([(0, {"cpu": "1"}), (0, {"cpu": "1"}), (0, {"cpu": "1"})])
    pods.volumes = [[(EBS, "default/a"), (PD, "default/b")], [], [(EBS, "default/a")]]
    ex = [model.ExistingNode("n0", {}, np.zeros(model.R, np.int64), volumes=[(EFS, "default/c")]),
          model.ExistingNode("n1", {}, np.zeros(model.R, np.int64), volumes=[(EBS, "default/a")], volume_limits={EBS: 25})]
    return model.Problem(fake, [synth.default_nodepool()], [model.PodClass()], pods, ex)


def test_csr_tables(fake):
    v = model.SolveInputView(_small_problem(fake)).view
    assert v.n_volume_drivers == 3
    assert [v.volume_drivers[i].decode() for i in range(3)] == [EBS, PD, EFS]
    assert [v.pod_volume_offsets[i] for i in range(4)] == [0, 2, 2, 3]
    assert [(v.pod_volumes[i].driver, v.pod_volumes[i].id) for i in range(3)] == [(0, 0), (1, 1), (0, 0)]
    assert [v.existing_volume_offsets[i] for i in range(3)] == [0, 1, 2]
    assert [(v.existing_volumes[i].driver, v.existing_volumes[i].id) for i in range(2)] == [(2, 2), (0, 0)]
    assert [v.existing_limit_offsets[i] for i in range(3)] == [0, 0, 1]
    assert (v.existing_limits[0].driver, v.existing_limits[0].limit) == (0, 25)


def test_no_volumes_marshal_as_null(fake):
    """A problem without volumes leaves the offsets NULL: the zero-initialised input of every existing caller."""
    v = model.SolveInputView(VC.strip(_small_problem(fake))).view
    for f in ("pod_volume_offsets", "pod_volumes", "existing_volume_offsets", "existing_volumes", "existing_limit_offsets",
              "existing_limits"):
        assert not getattr(v, f), f
    assert v.n_volume_drivers == 0


def test_struct_tail_layout():
    """The volume tables are appended behind the host-port tables: every earlier field keeps its offset."""
    full = abi.kp_solve_input_full
    assert [f[0] for f in full._fields_] == ["n_volume_drivers", "volume_drivers", "pod_volume_offsets", "pod_volumes",
                                             "existing_volume_offsets", "existing_volumes", "existing_limit_offsets",
                                             "existing_limits"]
    assert full.n_volume_drivers.offset == C.sizeof(abi.kp_solve_input)
    assert full.existing_ports.offset == abi.kp_solve_input.existing_ports.offset
    assert C.sizeof(full) == C.sizeof(abi.kp_solve_input) + 8 * C.sizeof(C.c_void_p)
    assert C.sizeof(abi.kp_volume) == 8 and C.sizeof(abi.kp_volume_limit) == 8
    assert abi.kp_consolidate_input.initialized.offset == C.sizeof(full)


# ------------------------------------------------------------------------------------------------
# the host layer (kp_solve_prepare over the CPU stand-in of the HIP runtime)
# ------------------------------------------------------------------------------------------------
HOST_CASES = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from kpsim import abi, catalog, model, native, synth
fake = catalog.fake_catalog(fx=catalog.load_fixtures())
ctx = native.Context(0)
ctx.upload_catalog(model.CatalogView(fake))

def node(name, volumes=(), limits=None):
    return model.ExistingNode(name, {}, np.array(fake[0].allocatable, np.int64), volumes=list(volumes), volume_limits=limits or {})

def run(tag, vols, nodes, patch=None):
    pods = synth.pods_from_specs([(0, {'cpu': '100m'})] * len(vols))
    pods.volumes = vols
    iv = model.SolveInputView(model.Problem(fake, [synth.default_nodepool()], [model.PodClass()], pods, nodes))
    if patch:
        patch(iv.view)
    try:
        ctx.prepare(iv)
        print(tag, 'ok')
    except native.KpError as e:
        print(tag, e.status, str(e).replace('\n', ' '))

def drivers(n):
    return {'drv-%%d' %% i: 5 for i in range(n)}
run('d8', [[('drv-0', 'a')]], [node('n0', limits=drivers(8))])
run('d9', [[('drv-0', 'a')]], [node('n0', limits=drivers(9))])
# unlimited drivers do not count towards the cap
run('d8+unlimited', [[('x-%%d' %% i, 'c%%d' %% i) for i in range(20)]], [node('n0', limits=drivers(8))])
for n in (256, 257):   # n claims, each held by both pods: n shared bits
    run('s%%d' %% n, [[('drv-0', 'c%%d' %% i) for i in range(n)]] * 2, [node('n0', limits={'drv-0': 1000})])
# 300 claims shared on a driver without any limit are dropped, not counted
run('s300-unlimited', [[('x', 'c%%d' %% i) for i in range(300)]] * 2, [node('n0', limits={'drv-0': 3})])
# 300 private claims take no bit
run('p300', [[('drv-0', 'c%%d' %% i) for i in range(300)]], [node('n0', limits={'drv-0': 3})])

def set_driver(i, v):
    def f(view):
        view.pod_volumes[i].driver = v
    return f
def set_limit(field, v):
    def f(view):
        setattr(view.existing_limits[0], field, v)
    return f
def dup(view):
    view.pod_volumes[1].id = view.pod_volumes[0].id
def two_drivers(view):
    view.pod_volumes[1].id = view.pod_volumes[0].id
    view.pod_volumes[1].driver = 1
def neg_id(view):
    view.pod_volumes[0].id = -1
two = [[('drv-0', 'a'), ('drv-0', 'b')]]
lim = [node('n0', [('drv-1', 'z')], limits={'drv-0': 3})]
run('valid', two, lim)
run('driver-range', two, lim, set_driver(0, 7))
run('driver-negative', two, lim, set_driver(0, -1))
run('limit-negative', two, lim, set_limit('limit', -1))
run('limit-driver-range', two, lim, set_limit('driver', 9))
run('duplicate', two, lim, dup)
run('two-drivers', two, lim, two_drivers)
run('negative-id', two, lim, neg_id)
"""


def test_host_layer_caps_and_invalid_tables():
    here = os.path.dirname(os.path.abspath(__file__))
    stub = os.path.join(here, "cpu_stub")
    subprocess.check_call(["make", "-s", "-C", stub, "build/libkpsim_stub.so"], stdout=subprocess.DEVNULL)
    code = HOST_CASES % (os.path.join(os.path.dirname(here), "karpenter-provider-aws_amd"), here)
    env = dict(os.environ, KPSIM_LIB=os.path.join(stub, "build", "libkpsim_stub.so"), KP_STUB_DEVICES="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in r.stdout.strip().split("\n")}
    for tag in ("d8", "d8+unlimited", "s256", "s300-unlimited", "p300", "valid"):
        assert got[tag] == "ok", (tag, got[tag])
    for tag, word in (("d9", "9"), ("s257", "257")):
        st, msg = got[tag].split(" ", 1)
        assert int(st) == abi.KP_E_UNSUPPORTED and word in msg, (tag, got[tag])
    for tag in ("driver-range", "driver-negative", "limit-negative", "limit-driver-range", "duplicate", "two-drivers",
                "negative-id"):
        assert int(got[tag].split(" ", 1)[0]) == abi.KP_E_INVALID, (tag, got[tag])


# ------------------------------------------------------------------------------------------------
# the fuzz seeds of the GPU tests are not vacuous
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cats(golden):
    return VC.sub_catalogs(golden)


def _differs(a, b):
    try:
        parity.assert_same(a, b)
    except AssertionError:
        return True
    return False


def _cases():
    return [pytest.param(f, s, id="%s-%d" % (f, s)) for f, seeds in VC.FAMILY_SEEDS.items() for s in seeds]


@pytest.mark.parametrize("family,seed", _cases())
def test_seed_is_not_vacuous(cats, family, seed):
    """The volumes change the Solve's result in every seed, the reference keeps every node within its limits, and the
    shared-claim dictionary of the word-edge seeds has exactly the size their name says."""
    dprob, oprob, sprob, policy = VC.family_problem(cats, family, seed)
    enc = VC.problem_encoding(dprob)
    assert 1 <= len(enc.limited) <= 4
    assert not any(enc.exceeds(j) for j in range(len(dprob.existing)))
    with_vol = VC.run_oracle(oprob, policy)
    VC.assert_within_limits(dprob, with_vol[0])
    assert _differs(with_vol, VC.run_oracle(sprob, policy))
    if family in VC.EDGE:
        assert enc.n_bits == VC.EDGE[family][0] * VC.EDGE[family][1] == int(family.split("_")[1])
    if family in ("family_a", "family_b"):
        assert enc.n_bits >= 1


@pytest.mark.parametrize("seed", list(VC.CONS_SEEDS))
def test_consolidation_seed_is_not_vacuous(cats, seed):
    """With the oracle alone, per seed and per mode: some probe's row differs from the volume-stripped run, and some
    probe still decides DELETE or REPLACE in the seed (it is not too dense to test anything).  No node is over a limit;
    the odd seeds carry shared claims (family B), the even ones none."""
    import pyoracle
    cp, ocp, scp = VC.cons_problem(cats, seed)
    assert 6 <= len(cp.cluster.existing) <= 10
    enc = VC.problem_encoding(cp.cluster, VC.own_nodes(cp))
    assert (enc.n_bits >= 1) == (seed % 2 == 1)
    assert not any(enc.exceeds(j) for j in range(len(cp.cluster.existing)))
    decided = 0
    for mode in (abi.KP_CONSOLIDATE_SINGLE, abi.KP_CONSOLIDATE_MULTI):
        a, b = pyoracle.consolidate(ocp, mode), pyoracle.consolidate(scp, mode)
        assert len(a) == len(b)
        assert sum(tuple(x) != tuple(y) for x, y in zip(a.tolist(), b.tolist())) >= 1, mode
        decided += int((a["decision"] != abi.KP_DECISION_NONE).sum())
    assert decided >= 1


def test_multi_device_seed_is_a_checked_seed():
    assert VC.CONS_MULTI_DEVICE_SEED in VC.CONS_SEEDS


# ------------------------------------------------------------------------------------------------
# the host's private / shared split (kp_host.cpp solve_volumes) against the rule and the restatement
# ------------------------------------------------------------------------------------------------
HOST_ENCODING = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import volume_cases as VC
from kpsim import abi, catalog, model, native, synth
from volume_cases import EBS, EFS, PD
fake = catalog.fake_catalog(fx=catalog.load_fixtures())
ctx = native.Context(0)
ctx.upload_catalog(model.CatalogView(fake))

def mask_int(words):
    return sum(int(w) << (64 * i) for i, w in enumerate(words))

def check(tag, pods, nodes, limits, own, host):
    # the restatement, field by field
    enc = VC.Encoding(pods, nodes, limits, own)
    P, E, VD = len(pods), len(nodes), len(enc.limited)
    assert host["VD"] == VD and host["bits"] == enc.n_bits and host["VW"] == (enc.n_bits + 63) // 64, (tag, host["VD"], host["bits"])
    if VD == 0:
        return 0
    names = []
    for rows in (pods, nodes):
        for r in rows:
            for d, _ in r:
                if d not in names:
                    names.append(d)
    for lim in limits:
        for d in sorted(lim):
            if d not in names:
                names.append(d)
    assert [names[int(k)] for k in host["limited_driver"]] == enc.limited, tag
    sig = host["pod_signature"]
    assert (sig[[p for p in range(P) if not any(enc.pods[p][0]) and not enc.pods[p][1]]] == 0).all(), tag
    for p in range(P):
        s = int(sig[p])
        assert host["signature_count"][s].tolist() == enc.pods[p][0], (tag, p)
        assert mask_int(host["signature_mask"][s]) == enc.pods[p][1], (tag, p)
    for p in range(P):       # equal signatures <=> equal (counts, mask)
        for q in range(p):
            assert (sig[p] == sig[q]) == (enc.pods[p] == enc.pods[q]), (tag, p, q)
    for k in range(VD):
        assert mask_int(host["driver_mask"][k]) == enc.drv_mask[k], (tag, k)
    for j in range(E):
        assert host["node_count"][:, j].tolist() == enc.nodes[j][0], (tag, j)
        assert mask_int(host["node_mask"][j]) == enc.nodes[j][1], (tag, j)
        want = [2 ** 31 - 1 if x is None else x for x in enc.lim[j]]
        assert host["node_limit"][:, j].tolist() == want, (tag, j)
        # ... and the rule itself, from the host's numbers alone
        assert bool(host["node_over_limit"][j]) == VC.exceeds_limits(nodes[j], limits[j], []), (tag, j)
        for p in range(P):
            if own.get(p) == j:
                continue
            s = int(sig[p])
            over = False
            for k in range(VD):
                m = mask_int(host["node_mask"][j]) | mask_int(host["signature_mask"][s])
                used = int(host["node_count"][k, j]) + int(host["signature_count"][s, k]) + \
                    bin(m & mask_int(host["driver_mask"][k])).count("1")
                over = over or used > int(host["node_limit"][k, j])
            assert over == VC.exceeds_limits(nodes[j], limits[j], pods[p]), (tag, p, j)
    return enc.n_bits

def node(name, volumes, limits):
    return model.ExistingNode(name, {}, np.array(fake[0].allocatable, np.int64), volumes=list(volumes), volume_limits=dict(limits))

n_shared = n_private_own = 0
for seed in range(24):
    rng = np.random.Generator(np.random.PCG64(6000 + seed))
    drivers = [EBS, PD, EFS]
    n_claims = int(rng.integers(4, 30)) if seed %% 6 else 200      # every sixth seed: more than one mask word
    claims = [(drivers[i %% 3], "c%%d" %% i) for i in range(n_claims)]
    def row(n):
        return [claims[int(i)] for i in rng.choice(len(claims), size=min(n, len(claims)), replace=False)]
    P, E = 20, 6
    big = 40 if n_claims == 200 else 4
    pods = [row(int(rng.integers(0, big))) for _ in range(P)]
    nodes = [row(int(rng.integers(0, big))) for _ in range(E)]
    limits = [{d: int(rng.integers(0, 6 * big // 4)) for d in drivers[:2] if rng.random() < 0.7} for _ in range(E)]
    if seed == 5:
        limits = [{} for _ in range(E)]                             # no limit anywhere: nothing is encoded
    cons = seed %% 2 == 1
    own = {}
    if cons:   # reschedulable pods: the own node mounts the pod's claims and is no holder for the split
        for p in range(0, P, 2):
            j = int(rng.integers(3))
            own[p] = j
            pods[p] = pods[p] + [(EBS, "own-%%d" %% p)]   # a StatefulSet claim: only this pod and its own node hold it
            nodes[j] = nodes[j] + [v for v in pods[p] if v not in nodes[j]]
    podv = synth.pods_from_specs([(0, {'cpu': '100m'})] * P)
    podv.volumes = pods
    prob = model.Problem(fake, [synth.default_nodepool()], [model.PodClass()], podv,
                         [node("node-%%d" %% j, nodes[j], limits[j]) for j in range(E)])
    if cons:
        cands = [model.Candidate(node=j, pods=np.array([p for p in own if own[p] == j], np.int32), price=10.0,
                                 instance_type=0, nodepool=0, capacity=np.array(fake[0].capacity, np.int64)) for j in range(3)]
        ctx.consolidate_prepare(model.ConsolidateInputView(model.ConsolidationProblem(prob, cands), abi.KP_CONSOLIDATE_SINGLE))
    else:
        ctx.prepare(model.SolveInputView(prob))
    host = ctx.volume_encoding()
    n_shared += check("seed %%d" %% seed, pods, nodes, limits, own, host)
    if cons and host["VD"]:
        enc = VC.Encoding(pods, nodes, limits, own)
        plain = VC.Encoding(pods, nodes, limits, {})
        n_private_own += plain.n_bits - enc.n_bits   # claims the own-node exception keeps private
        assert host["bits"] == enc.n_bits
print("ok", n_shared, n_private_own)
"""


def test_host_split_matches_rule_and_restatement():
    """kp_solve_prepare and kp_consolidate_prepare over the CPU stand-in of the HIP runtime, 24 seeded inputs (half of
    them consolidation passes with own nodes, every sixth with a dictionary of several words): the host's limited
    drivers, shared bits, per-pod signatures, driver masks, node counts / masks / limits and over-limit flags
    (kp_solve_volume_encoding) equal the restatement field by field, and the test computed from the host's numbers alone
    decides every (pod, node) pair as the rule does.  The own-node exception must have kept some claims private."""
    here = os.path.dirname(os.path.abspath(__file__))
    stub = os.path.join(here, "cpu_stub")
    subprocess.check_call(["make", "-s", "-C", stub, "build/libkpsim_stub.so"], stdout=subprocess.DEVNULL)
    code = HOST_ENCODING % (os.path.join(os.path.dirname(here), "karpenter-provider-aws_amd"), here)
    env = dict(os.environ, KPSIM_LIB=os.path.join(stub, "build", "libkpsim_stub.so"), KP_STUB_DEVICES="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    tag, n_shared, n_private_own = r.stdout.strip().split("\n")[-1].split()
    assert tag == "ok" and int(n_shared) > 100 and int(n_private_own) >= 10, r.stdout
