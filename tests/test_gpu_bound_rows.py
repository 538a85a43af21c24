"""GPU: the headroom bound's rows across commits (DESIGN.md §4 "Headroom bound": the unchanged-row rule; inputs and the
parent's statistics: tests/bound_rows_cases.py, CPU companion: tests/test_bound_rows_cpu.py).

An in-flight commit leaves its NodeClaim's row alone while the accepted options still hold the type that gave each axis'
maximum.  narrowed: every commit of the requirement-carrying class removes the cpu axis' largest type, so its row must be
stored again: the pods behind it pass the old maximum, exceed the new one and are skipped, G exactly.  kept: the same
commits remove nothing, the rows stay, nothing is skipped.  Two solves in turn on one context: the second creates its
NodeClaims at the indices whose rows the first left tighter, and must not be judged by them.  Rank edges (BC.rank_edge):
NodePools of the one type at positions 63, 64 and 896 of the cpu or memory rank table, whose NodeClaims find their option
in the last lane of the walk's first step, the first lane of its second, or only in its last step; pods one milli-unit
above what the largest option leaves are skipped (2 F - 1 exactly), pods at it are not.  Their templates' walks start
at the host's per-template step (KpDev::tmpl_bstep: the smallest step over the axes, so above 0 for the pools of small types), on an idle wave.  The row cases' own NodePool
ranks below the first step, so their narrowing commits resume from a stored step above 0.

No case flips a witness flag: in the kernels that carry the bound the flag of a NodeClaim is fixed by its template
(minValues) for the whole solve, and a new solve stores every row afresh, so no input reaches that half of
kp_bound_axis_kept with a change; tests/cpu_stub/test_bound_tail.cpp covers it exhaustively, and HC.min_values
(tests/test_gpu_headroom_bound.py) runs in-flight commits on rows stored without a witness.

Every case is bit-exact against the oracle, and every always-on statistic (BC.observe: the count fields of
kp_solve_stats and the exact counters of kp_last_kernel_times, bound skips among them) equals the parent commit's.
"""
import pytest

import bound_rows_cases as BC
import parity
from kpsim import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(golden):
    return BC.build(golden)


def run(ctx, case):
    orc = parity.run_oracle(case.problem)
    assert orc[0].n_nodeclaims == case.n_nodeclaims
    dev = parity.run_device(ctx, case.problem)
    got = BC.observe(ctx, dev[0])
    print(case.name, got)
    parity.assert_same(dev, orc)
    return got


@pytest.mark.parametrize("name", BC.ROWS + BC.RANKS)
def test_rows_case(cases, name):
    case = cases[name]
    ctx = native.Context(0)
    try:
        got = run(ctx, case)
    finally:
        ctx.close()
    assert got == BC.PARENT[name]
    assert got[-1] == case.skips


def test_second_solve_reuses_nodeclaim_indices(cases):
    """narrowed_G3 leaves the rows of NodeClaims 0..2 at the 8-vCPU maximum; kept_G3 on the same context opens its
    NodeClaims at those indices with both options: 8.5 cpu fits them, and a row left over would reject it"""
    ctx = native.Context(0)
    try:
        first = run(ctx, cases["narrowed_G3"])
        second = run(ctx, cases["kept_G3"])
    finally:
        ctx.close()
    assert first == BC.PARENT["narrowed_G3"]
    assert second == BC.PARENT["narrowed_then_kept"] == BC.PARENT["kept_G3"]
    assert second[-1] == 0
