"""GPU: runs of same-shape pods that walk the NodeClaim slice level by level (wave 0's same-shape inner loop, DESIGN.md
§4 item 4a; inputs: tests/same_shape_cases.py, CPU companion: tests/test_same_shape_runs_cpu.py).

Every case is bit-exact against the oracle (parity.assert_same), yields the NodeClaim count its construction intends
and places every pod.  The inner loop must leave the always-on statistics what the general loop made them: pods_popped,
nodeclaim_candidates_scanned (+N per pop that reaches the NodeClaims), sorts_fast, sorts_full, quick_accepts and
slow_pods are compared with PARENT, recorded from a build of the commit before the inner loop (PARENT_COMMIT;
tools/build_commit.sh builds it, KPSIM_LIB selects it) on these same inputs, never from the build under test.
"""
import ctypes as C

import pytest

import parity
import same_shape_cases as SC
from kpsim import native

pytestmark = pytest.mark.gpu

PARENT_COMMIT = "adaca95"
# case -> (pods_popped, nodeclaim_candidates_scanned, sorts_fast, sorts_full, quick_accepts, slow_pods) of the parent build
PARENT = {
    "walk_N1": (21, 20, 0, 0, 20, 1),
    "walk_N12": (54, 570, 38, 0, 42, 12),
    "walk_N13": (59, 676, 0, 42, 46, 13),
    "walk_N49": (221, 9604, 0, 168, 172, 49),
    "walk_N50": (225, 9975, 171, 0, 175, 50),
    "walk_N64": (288, 16352, 220, 0, 224, 64),
    "walk_N65": (293, 16900, 224, 0, 228, 65),
    "walk_N130": (585, 67535, 451, 0, 455, 130),
    "walk_N65_M1": (66, 2145, 0, 0, 1, 65),
    "walk_N65_M2": (67, 2210, 1, 0, 2, 65),
    "walk_N65_M63": (128, 6175, 62, 0, 63, 65),
    "walk_N65_M64": (129, 6240, 63, 0, 64, 65),
    "walk_N65_M65": (130, 6305, 64, 0, 65, 65),
    "walk_N65_M129": (194, 10465, 127, 0, 129, 65),
    "alternating_shapes_N12": (82, 906, 64, 0, 70, 12),
    "witness_fails_N12_E0": (159, 1830, 131, 0, 146, 13),
    "witness_fails_N12_E3": (174, 1830, 131, 0, 146, 13),
    "pref_requeued_N12": (58, 618, 37, 0, 41, 17),
    "reserved_N12": (65, 702, 48, 0, 53, 12),
    "alternating_shapes_N56": (346, 17780, 284, 0, 290, 56),
    "witness_fails_N56_E0": (731, 39340, 523, 137, 674, 57),
    "witness_fails_N56_E3": (746, 39340, 523, 137, 674, 57),
    "pref_requeued_N56": (248, 12292, 169, 0, 173, 75),
    "reserved_N56": (285, 14364, 224, 0, 229, 56),
}

NAMES = SC.NAMES


@pytest.fixture(scope="module")
def cases(golden):
    return SC.build(golden)


def counters(ctx):
    a = (C.c_double * 19)()
    ctx.check(ctx.L.kp_last_kernel_times(ctx.h, a, len(a)), "kp_last_kernel_times")
    return int(a[17]), int(a[18])  # quick accepts, slow-path pods (kpsim.h)


def solve(case):
    ctx = native.Context(0, preference_policy=case.preference_policy)
    try:
        dev = parity.run_device(ctx, case.problem)
        return dev, counters(ctx)
    finally:
        ctx.close()


def test_names_cover_the_cases(cases):
    assert sorted(NAMES) == sorted(cases) and sorted(PARENT) == sorted(cases)


@pytest.mark.parametrize("name", NAMES)
def test_same_shape_runs(cases, name):
    case = cases[name]
    orc = parity.run_oracle(case.problem)
    assert orc[0].n_nodeclaims == case.n_nodeclaims
    assert (orc[0].pod_result != -1).all()
    dev, (quick, slow) = solve(case)
    st = dev[0].stats
    got = (st["pods_popped"], st["nodeclaim_candidates_scanned"], st["sorts_fast"], st["sorts_full"], quick, slow)
    print(name, got)
    parity.assert_same(dev, orc)
    assert got == PARENT[name]
