"""CPU: the same-shape walk cases (tests/same_shape_cases.py) do what their construction intends on the oracle: N
NodeClaims, every pod placed, the small pods spread level by level, and the special cases reach what they are for."""
import numpy as np
import pytest

import pyoracle
import same_shape_cases as SC


@pytest.fixture(scope="module")
def solved(golden):
    out = {}
    for name, c in SC.build(golden).items():
        out[name] = (c, pyoracle.solve(c.problem, preference_policy=c.preference_policy).results)
    return out


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_yields_its_nodeclaims(solved, name):
    c, r = solved[name]
    assert r.n_nodeclaims == c.n_nodeclaims
    assert (r.pod_result != -1).all()
    assert r.stats["pods_popped"] >= c.problem.pods.n


@pytest.mark.parametrize("name", [n for n in SC.NAMES if n.startswith("walk_")])
def test_walk_fills_level_by_level(solved, name):
    c, r = solved[name]
    n_pods = np.asarray(r.nodeclaim_n_pods[:r.n_nodeclaims])
    assert n_pods.max() - n_pods.min() <= 1


def test_special_cases_reach_their_paths(solved):
    for n in SC.SPECIAL_NS:
        c, r = solved["witness_fails_N%d_E0" % n]
        n_pods = np.asarray(r.nodeclaim_n_pods[:r.n_nodeclaims])
        assert n_pods.min() == 10 and n_pods.max() > 10      # the 7-cpu NodeClaims stopped at 1 + 9 pods
        c, r = solved["witness_fails_N%d_E3" % n]
        assert int((r.pod_result < -1).sum()) == 15          # the existing nodes took the first small pods
        c, r = solved["pref_requeued_N%d" % n]
        assert r.stats["pods_popped"] > c.problem.pods.n     # relaxed pods came round again
