"""GPU: the headroom bound of the slow path's candidate collection (DESIGN.md §4 "Headroom bound"; inputs:
tests/headroom_bound_cases.py, CPU companion: tests/test_headroom_bound_cpu.py).

Every case is bit-exact against the oracle (parity.assert_same) and yields the NodeClaim count its construction intends.
A case meant to skip rejects at least the F full NodeClaims of its construction by the bound (kp_last_kernel_times [49],
bound skips; the cases at the bound: exactly the count they imply); a case whose NodeClaims are ineligible, whose bound
passes or whose kernel is built without the bound skips none.  The
bound replaces evaluations and nothing else: the always-on statistics (every count field of kp_solve_stats, quick
accepts, slow-path pods) equal PARENT, and witness misses + evaluation calls + bound skips equal the parent's witness
misses + evaluation calls.  PARENT was recorded from a build of the commit before the bound (PARENT_COMMIT;
tools/build_commit.sh builds it, KPSIM_LIB selects it) on these same inputs, never from the build under test.

The plain and the preference fuzz families are bit-exact per seed and skip some candidate on at least three quarters of
their seeds; the reserved family is bit-exact and skips none; the per-seed counts are printed.  The kernels for catalogs with reserved offerings and for topology solves are built without
the bound, so they have no case here.
"""
import ctypes as C

import pytest

import fuzzgen
import headroom_bound_cases as HC
import parity
from kpsim import abi, native

pytestmark = pytest.mark.gpu

PARENT_COMMIT = "1f4f7e8"
STAT_FIELDS = ("pods_popped", "nodeclaim_evals", "nodeclaim_candidates_scanned", "template_evals", "existing_evals",
               "sorts_fast", "sorts_full")
# case -> (the STAT_FIELDS of kp_solve_stats, quick accepts, slow-path pods, witness misses + evaluation calls) of the parent
PARENT = {
    "absorbed_F7": (13, 23, 75, 10, 0, 1, 0, 2, 11, 23),
    "absorbed_F8": (14, 28, 88, 11, 0, 1, 0, 2, 12, 28),
    "absorbed_F9": (15, 31, 102, 12, 0, 1, 0, 2, 13, 31),
    "absorbed_F16": (22, 52, 228, 19, 0, 0, 2, 2, 20, 52),
    "absorbed_F17": (23, 55, 250, 20, 0, 0, 2, 2, 21, 55),
    "absorbed_F63": (69, 191, 2343, 66, 0, 1, 0, 2, 67, 191),
    "absorbed_F64": (70, 196, 2412, 67, 0, 1, 0, 2, 68, 196),
    "absorbed_F65": (71, 199, 2482, 68, 0, 1, 0, 2, 69, 199),
    "absorbed_F130": (136, 394, 9177, 133, 0, 1, 0, 2, 134, 394),
    "not_absorbed_F7": (13, 25, 75, 10, 0, 0, 0, 0, 13, 25),
    "not_absorbed_F8": (14, 30, 88, 11, 0, 0, 0, 0, 14, 30),
    "not_absorbed_F9": (15, 33, 102, 12, 0, 0, 0, 0, 15, 33),
    "not_absorbed_F16": (22, 54, 228, 19, 0, 0, 2, 0, 22, 54),
    "not_absorbed_F17": (23, 57, 250, 20, 0, 0, 2, 0, 23, 57),
    "not_absorbed_F63": (69, 193, 2343, 66, 0, 0, 0, 0, 69, 193),
    "not_absorbed_F64": (70, 198, 2412, 67, 0, 0, 0, 0, 70, 198),
    "not_absorbed_F65": (71, 201, 2482, 68, 0, 0, 0, 0, 71, 201),
    "not_absorbed_F130": (136, 396, 9177, 133, 0, 0, 0, 0, 136, 396),
    "no_fit_F7": (9, 13, 36, 8, 0, 0, 0, 1, 8, 13),
    "no_fit_F8": (10, 15, 45, 9, 0, 0, 0, 1, 9, 15),
    "no_fit_F9": (11, 17, 55, 10, 0, 0, 0, 1, 10, 17),
    "no_fit_F65": (67, 129, 2211, 66, 0, 0, 0, 1, 66, 129),
    "zero_axis_F9": (13, 29, 77, 11, 0, 0, 0, 1, 12, 29),
    "loose_F9": (12, 19, 66, 12, 0, 0, 0, 0, 12, 19),
    "at_bound_cpu_F9": (12, 8, 63, 9, 0, 2, 0, 3, 9, 8),
    "above_bound_cpu_F9": (12, 17, 65, 10, 0, 0, 0, 2, 10, 17),
    "at_bound_memory_F9": (12, 8, 63, 9, 0, 2, 0, 3, 9, 8),
    "above_bound_memory_F9": (12, 17, 65, 10, 0, 0, 0, 2, 10, 17),
    "min_values_F9": (15, 36, 102, 12, 0, 0, 0, 0, 15, 36),
    "reserved_F9": (15, 31, 102, 12, 0, 1, 0, 2, 13, 31),
    "topology_F9": (15, 49, 102, 12, 0, 0, 0, 0, 15, 49),
    "shared_F9": (17, 53, 130, 13, 0, 0, 3, 0, 17, 53),
    "pref_requeued_F9": (18, 43, 138, 15, 0, 1, 0, 2, 16, 43),
    "ports_F9": (16, 39, 114, 12, 0, 1, 0, 2, 14, 39),
}
NAMES = HC.NAMES
PREF_SEEDS = list(range(7100, 7106))


@pytest.fixture(scope="module")
def cases(golden):
    return HC.build(golden)


def counters(ctx):
    a = (C.c_double * 50)()
    ctx.check(ctx.L.kp_last_kernel_times(ctx.h, a, len(a)), "kp_last_kernel_times")
    # evaluation calls, quick accepts, slow-path pods, witness misses, bound skips (kpsim.h)
    return int(a[16]), int(a[17]), int(a[18]), int(a[19]), int(a[49])


def solve(prob, policy=abi.KP_PREFERENCE_RESPECT):
    ctx = native.Context(0, preference_policy=policy)
    try:
        dev = parity.run_device(ctx, prob)
        return dev, counters(ctx)
    finally:
        ctx.close()


def test_names_cover_the_cases(cases):
    assert sorted(NAMES) == sorted(cases) and sorted(PARENT) == sorted(cases)


@pytest.mark.parametrize("name", NAMES)
def test_bound_case(cases, name):
    case = cases[name]
    orc = parity.run_oracle(case.problem)
    assert orc[0].n_nodeclaims == case.n_nodeclaims
    assert (orc[0].pod_result != -1).all()
    dev, (calls, quick, slow, miss, skips) = solve(case.problem, case.preference_policy)
    st = dev[0].stats
    got = tuple(st[f] for f in STAT_FIELDS) + (quick, slow)
    print(name, got, "witness misses", miss, "evaluation calls", calls, "bound skips", skips)
    parity.assert_same(dev, orc)
    assert got == PARENT[name][:-1]
    assert miss + calls + skips == PARENT[name][-1]
    if case.skips >= 0:
        assert skips == case.skips
    elif case.min_skips == 0:  # ineligible NodeClaims, a kernel built without the bound, or a bound that passes
        assert skips == 0
    else:
        assert skips >= case.min_skips


def _family(golden, seeds, make, skipping=True):
    total, zero = 0, 0
    for seed in seeds:
        prob, policy, cv = make(golden, seed)
        ctx = native.Context(0, preference_policy=policy)
        try:
            dev = parity.run_device(ctx, prob, cv)
            skips = counters(ctx)[4]
        finally:
            ctx.close()
        parity.assert_same(dev, parity.run_oracle(prob, cv))
        print("seed", seed, "bound skips", skips)
        total += skips
        zero += skips == 0
    if skipping:
        assert total > 0
        assert zero * 4 <= len(seeds)
    else:  # a family whose kernels are built without the bound
        assert total == 0


def test_fuzz_plain(golden):
    """fuzzgen's plain Solve family at its own size, on the seeds HC.PLAIN_SEEDS: chosen on the CPU, the first 12 from
    7000 on in which the oracle's result alone shows a rejection for lack of a fitting type in front of a fit
    (HC.types_rejections_ahead; tests/test_headroom_bound_cpu.py holds the list to that)"""
    _family(golden, HC.PLAIN_SEEDS, lambda g, s: (fuzzgen.fuzz_problem(g, s), abi.KP_PREFERENCE_RESPECT, None))


def test_fuzz_preferences(golden):
    def make(g, s):
        import numpy as np
        prob = fuzzgen.fuzz_problem(g, s)
        fuzzgen.add_preferences(np.random.default_rng(s), prob, p_topo=0.0)  # (no topology: those kernels carry no bound)
        return prob, abi.KP_PREFERENCE_RESPECT, None
    _family(golden, PREF_SEEDS, make)


def test_fuzz_reserved(golden):
    """the reserved family of tests/test_gpu_reserved.py (scarce reservations), 6 seeds: bit-exact, and no skip, because
    the kernels for catalogs with reserved offerings are built without the bound"""
    from kpsim import model
    from test_gpu_reserved import scarce_problem

    def make(g, s):
        prob = scarce_problem(g, s)
        return prob, abi.KP_PREFERENCE_RESPECT, model.CatalogView(prob.catalog)
    _family(golden, range(6), make, skipping=False)
