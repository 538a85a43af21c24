"""CPU: what tests/test_gpu_dense_plans.py rests on, from the oracle alone.  For every family and size of
tests/dense_cases.py (dense_cases.check): more than 4,096 NodeClaims and no pod unschedulable; the NodeClaims' pod counts
take at least three values, each on at least 5 % of them (unequal slice keys); the pod count is in the range that
selects the size's plan; the layered feature took effect (preferences kept by some pods and relaxed for others,
reservations held by some NodeClaims only, small pods per zone within 1, one port pod per NodeClaim).

The plan thresholds themselves (slice_hbm, lds_nq of kp_last_solve_plan) are asserted by the GPU tests only: the CPU
stand-in of the host layer (tests/cpu_stub) has its own kp_ffd_plan_lds and does not link the kernels' one.  What the
accessor needs no kernel for runs over that stand-in here: its window, its short reads, the planned capacity and the
selection bits, which the host derives from the input.
"""
import os
import subprocess
import sys

import pytest

import dense_cases as DC
from kpsim import abi


@pytest.fixture(scope="module")
def cats(golden):
    return DC.Catalogs(golden)


@pytest.mark.parametrize("name", DC.NAMES)
def test_dense_case(cats, name):
    family, size = name.rsplit("-", 1)
    case = DC.build(cats, family, size)
    DC.check(case, DC.run_oracle(case))


def test_families_cover_the_entry_points():
    """seven families x two sizes; the four selection bits differ between any two families"""
    assert len(DC.NAMES) == 14
    bits = [tuple(sorted(b.items())) for b in DC.FAMILIES.values()]
    assert len(set(bits)) == len(bits)


STUB_CHILD = r"""
import os, sys
sys.path[:0] = [%r, %r]
import ctypes as C
from kpsim import abi, catalog, model, native, synth
from kpsim.model import HostPort, PodClass, Requirement, TopologyTerm
fake = catalog.fake_catalog(fx=catalog.load_fixtures())
ctx = native.Context(0)
ctx.upload_catalog(model.CatalogView(fake))
def status(f):
    try:
        f()
        return abi.KP_OK
    except native.KpError as e:
        return e.status
def plan(classes, n=5):
    pods = synth.pods_from_specs([(i %% len(classes), {"cpu": "100m"}) for i in range(n)])
    ctx.prepare(model.SolveInputView(model.Problem(fake, [synth.default_nodepool()], classes, pods)))
    ctx.execute()
    p = ctx.solve_plan()
    return [p[k] for k in ("NCcap", "ports", "pref", "resv", "topo", "twin", "slice_hbm")]
print("before any solve", status(lambda: ctx.solve_plan()))
print("plain", plan([PodClass()]))
a = (C.c_int32 * 3)(-7, -7, -7)
print("short read", ctx.L.kp_last_solve_plan(ctx.h, a, 2), list(a))
print("null", ctx.L.kp_last_solve_plan(ctx.h, None, 2))
print("pref", plan([PodClass(preferred_terms=[(1, [Requirement(model.ZONE, "In", ["test-zone-1a"])])])]))
spread = TopologyTerm("spread", model.ZONE, [Requirement("a", "In", ["b"])])
print("topo", plan([PodClass(labels={"a": "b"}, topology=[spread])]))
print("ports", plan([PodClass(host_ports=[HostPort(80)]), PodClass()]))
os.environ["KPSIM_PROFILE"] = "1"
print("twin", plan([PodClass()], n=7))
"""


def test_plan_accessor_over_the_hip_stub():
    """kp_last_solve_plan over the CPU stand-in of the HIP runtime, in a child process: KP_E_STATE before the first
    execute, a short read copies that many values, the capacity of a first plan is the pod count for a small solve, and
    each feature of the input sets its selection bit (the twin bit follows KPSIM_PROFILE)."""
    here = os.path.dirname(os.path.abspath(__file__))
    stub = os.path.join(here, "cpu_stub")
    subprocess.check_call(["make", "-s", "-C", stub, "build/libkpsim_stub.so"], stdout=subprocess.DEVNULL)
    code = STUB_CHILD % (os.path.join(os.path.dirname(here), "karpenter-provider-aws_amd"), here)
    env = dict(os.environ, KPSIM_LIB=os.path.join(stub, "build", "libkpsim_stub.so"), KP_STUB_DEVICES="1")
    env.pop("KPSIM_PROFILE", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    #                NCcap ports pref resv topo twin slice_hbm
    assert r.stdout.splitlines() == [
        "before any solve %d" % abi.KP_E_STATE,
        "plain [5, 0, 0, 0, 0, 0, 0]",
        "short read 0 [5, 5, -7]",
        "null %d" % abi.KP_E_INVALID,
        "pref [5, 0, 1, 0, 0, 0, 0]",
        "topo [5, 0, 0, 0, 1, 0, 0]",
        "ports [5, 1, 0, 0, 0, 0, 0]",
        "twin [7, 0, 0, 0, 0, 1, 0]",
    ], r.stdout
