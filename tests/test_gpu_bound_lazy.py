"""GPU: the headroom bound at the hand-off when the pod's first candidate is evaluated by the block before the round's
other candidates (DESIGN.md §4 "Headroom bound"; inputs and the parent's statistics: tests/bound_rows_cases.py, CPU
companion: tests/test_bound_rows_cpu.py).

The round's gather runs at the hand-off.  A variant that deferred it to the first candidate's rejection was measured
slower and is not in the tree; these are the inputs it was held to, kept as the hand-off's own cases:
the marks the gather leaves and the counts are the parent's.  Every case opens its NodeClaims from templates: an idle wave
computes their rows beside the commit, and with KPSIM_NO_TEAM_FIRST the committing wave does.
* not_absorbed_F0: the first candidate has room (its witness covers the pod), has not absorbed the class and accepts:
  no mark of its round is ever applied, and the 2-cpu pods skip nothing.
* disjoint_F7_G3 / F8_G3 / F9_G0: the first candidate has room and rejects on requirements (disjoint instance-type
  sets); the first 2-cpu pod skips the F full NodeClaims behind it, F exactly: they fill its round (7), reach into the
  next beside open NodeClaims (8), or leave a next round of full ones alone (9).
* absorbed_F0: a first candidate that has absorbed the class is fits-only, never the block's: the old order.
* BC.NO_TEAM_FIRST: three of the cases again with the block's first evaluation off (KPSIM_NO_TEAM_FIRST=1): the old
  order, against the parent's statistics under the same setting.

Every case is bit-exact against the oracle, every always-on statistic (BC.observe) equals the parent commit's, and the
bound skips are the count the construction implies (BC's docstring: the pods that open the NodeClaims skip some too).
"""
import pytest

import bound_rows_cases as BC
import parity
from kpsim import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(golden):
    return BC.build(golden)


@pytest.mark.parametrize("name", BC.NO_TEAM_FIRST)
def test_handoff_case_without_team_first(cases, name, monkeypatch):
    """KPSIM_NO_TEAM_FIRST=1 (read at prepare): no first candidate is evaluated by the block, every round is evaluated
    one candidate per wave and the gather stays at the hand-off: the old order, with the statistics the parent commit
    gives under the same setting (PARENT[name + "@no_team_first"])"""
    monkeypatch.setenv("KPSIM_NO_TEAM_FIRST", "1")
    test_handoff_case(cases, name, key=name + "@no_team_first")


@pytest.mark.parametrize("name", BC.LAZY)
def test_handoff_case(cases, name, key=None):
    key = key or name
    case = cases[name]
    orc = parity.run_oracle(case.problem)
    assert orc[0].n_nodeclaims == case.n_nodeclaims
    ctx = native.Context(0)
    try:
        dev = parity.run_device(ctx, case.problem)
        got = BC.observe(ctx, dev[0])
    finally:
        ctx.close()
    print(key, got)
    parity.assert_same(dev, orc)
    assert got == BC.PARENT[key]
    if key == name:  # (BC's count is for the default order; without the block's first evaluation the parent's holds)
        assert got[-1] == case.skips
