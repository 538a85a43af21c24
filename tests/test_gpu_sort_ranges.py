"""GPU: the full pdqsort emulation with short ranges finished in registers (csrc/kp_gosort.h WaveLds::hand_over, DESIGN.md
§4 step 3; inputs: tests/sort_ranges_cases.py, CPU companion: tests/test_gosort_ranges_cpu.py).

Every case is bit-exact against the oracle (parity.assert_same, requirement blobs included) and yields the NodeClaim
count its construction intends.  mixed_N40 and mixed_N60 never exceed 64 NodeClaims (the whole slice is the register
range); the others grow past 64, 128 and 256.  Every case takes full sorts.

The always-on statistics must be what they were before short ranges left LDS: pods_popped,
nodeclaim_candidates_scanned, sorts_fast, sorts_full, quick accepts and slow-path pods are compared with PARENT, recorded
on an MI355X from a library built from the parent commit (PARENT_COMMIT; KPSIM_LIB selected it) on these same inputs,
never from the build under test.

The diagnostic twin (KPSIM_PROFILE=1) counts the full sorts that start over LDS (n > 64, kp_last_kernel_times [52]): every
case meant to pass 64 must have some, the two others none, and the twin's result must equal the production build's.
"""
import ctypes as C
import os

import pytest

import parity
import sort_ranges_cases as RC
from kpsim import abi, native

pytestmark = pytest.mark.gpu

PARENT_COMMIT = "7994610"
# case -> (pods_popped, nodeclaim_candidates_scanned, sorts_fast, sorts_full, quick_accepts, slow_pods) of the parent build
PARENT = {
    "mixed_N40": (225, 8184, 0, 176, 179, 46),
    "mixed_N60": (330, 17970, 142, 121, 269, 61),
    "mixed_N68": (374, 23086, 159, 141, 305, 69),
    "mixed_N132": (792, 95766, 399, 247, 650, 142),
    "mixed_N260": (1560, 371670, 793, 487, 1283, 277),
    "mixed_N448": (2688, 1103648, 1370, 841, 2213, 475),
}

NAMES = RC.NAMES


@pytest.fixture(scope="module")
def cases(golden):
    return RC.build(golden)


@pytest.fixture(scope="module")
def oracle(cases):
    """name -> the oracle's result, computed once"""
    return {name: parity.run_oracle(c.problem) for name, c in cases.items()}


def solve(case, profile=False):
    old = os.environ.pop("KPSIM_PROFILE", None)
    if profile:
        os.environ["KPSIM_PROFILE"] = "1"
    ctx = native.Context(0, preference_policy=case.preference_policy)
    try:
        dev = parity.run_device(ctx, case.problem)
        a = (C.c_double * 54)()
        ctx.check(ctx.L.kp_last_kernel_times(ctx.h, a, len(a)), "kp_last_kernel_times")
        return dev, [int(x) for x in a]
    finally:
        ctx.close()
        os.environ.pop("KPSIM_PROFILE", None)
        if old is not None:
            os.environ["KPSIM_PROFILE"] = old


def observed(dev, a):
    st = dev[0].stats
    return (st["pods_popped"], st["nodeclaim_candidates_scanned"], st["sorts_fast"], st["sorts_full"], a[17], a[18])


def test_names_cover_the_cases(cases):
    assert sorted(NAMES) == sorted(cases) and sorted(PARENT) == sorted(cases)
    assert [c.passes for c in cases.values()] == [0, 0, 64, 128, 256, 256]


@pytest.mark.parametrize("name", NAMES)
def test_sort_ranges(cases, oracle, name):
    case, orc = cases[name], oracle[name]
    assert orc[0].n_nodeclaims == case.n_nodeclaims
    assert case.n_nodeclaims > case.passes and (case.passes or case.n_nodeclaims <= 64)
    dev, a = solve(case)
    got = observed(dev, a)
    print(name, got)
    parity.assert_same(dev, orc)
    assert got[3] > 0  # sorts_full
    assert got == PARENT[name]
    assert a[52] == 0 and a[53] == 0  # the split is the twin's alone


@pytest.mark.parametrize("name", NAMES)
def test_twin_counts_the_sorts_that_start_over_lds(cases, oracle, name):
    case = cases[name]
    plain, ap = solve(case)
    twin, at = solve(case, profile=True)
    print(name, observed(twin, at), "full sorts at n > 64:", at[52], "cycles", at[53], "of", at[10])
    parity.assert_same(twin, plain)
    parity.assert_same(twin, oracle[name])
    for f, _ in abi.kp_solve_stats._fields_:
        if not f.startswith("ns_"):
            assert plain[0].stats[f] == twin[0].stats[f], f
    assert observed(twin, at) == observed(plain, ap)
    full = twin[0].stats["sorts_full"]
    if case.passes:
        assert 0 < at[52] <= full and 0 < at[53] <= at[10]
    else:
        assert at[52] == 0 and at[53] == 0 and at[10] > 0
