"""CPU: the headroom bound (DESIGN.md §4 "Headroom bound"; GPU companion: tests/test_gpu_headroom_bound.py).

The row entry / reject test pair of csrc/kp_bound.h is checked exhaustively over small ranges by a stand-alone C++
program (tests/cpu_stub/test_bound.cpp).  The constructed inputs (tests/headroom_bound_cases.py) are checked against the
oracle: each yields the NodeClaim count its construction intends, places every pod, and its F full NodeClaims do reject
the 2-cpu shape for lack of a fitting type — the oracle evaluates at least F in-flight NodeClaims more than the same
input without the 2-cpu pods.
"""
import os
import shutil
import subprocess

import pytest

import headroom_bound_cases as HC
import parity
from kpsim import model

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_stub")


def test_bound_pair_exhaustive(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_bound")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "test_bound.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("ok:")


@pytest.fixture(scope="module")
def cases(golden):
    return HC.build(golden)


@pytest.mark.parametrize("name", HC.NAMES)
def test_constructed_inputs(cases, name):
    case = cases[name]
    orc = parity.run_oracle(case.problem)[0]
    assert orc.n_nodeclaims == case.n_nodeclaims
    assert (orc.pod_result != -1).all()
    # the same input without the last shape's pods (class 1): what the 2-cpu pods add in NodeClaim evaluations
    p = case.problem
    keep = p.pods.class_id != 1
    base = model.Problem(p.catalog, p.nodepools, p.classes,
                         model.Pods(p.pods.class_id[keep], p.pods.requests[keep], p.pods.creation_ns[keep],
                                    [u for u, k in zip(p.pods.uids, keep) if k]), p.existing)
    orb = parity.run_oracle(base)[0]
    if not name.startswith("at_bound"):  # (there the small pods fit: the rejections are among the big pods themselves)
        assert orc.stats["nodeclaim_evals"] - orb.stats["nodeclaim_evals"] >= case.min_skips


def test_full_nodeclaims_reject_on_fits(golden):
    """The rejections of the F full NodeClaims are types-rejections by arithmetic: the classes carry no requirement
    (nothing else can reject), 7 + 2 cpu exceeds the allocatable cpu of every type of the pool, and 5 + 2 fits each."""
    cpu = model.RIDX["cpu"]
    alloc = [int(golden[r].allocatable[cpu]) for r in HC.SC.rows(golden)]
    assert 7000 + 2000 > max(alloc) and 5000 + 2000 <= min(alloc)
    # the loose-bound case: each axis passes the bound, no single type fits both
    a = {n: golden[r].allocatable for n, r in zip(HC.LOOSE_TYPES, HC.SC.rows(golden, HC.LOOSE_TYPES))}
    mem = model.RIDX["memory"]
    for c in (13000, 14000):
        assert c <= max(int(v[cpu]) for v in a.values()) and (40 << 30) * 1000 <= max(int(v[mem]) for v in a.values())
        assert not any(c <= int(v[cpu]) and (40 << 30) * 1000 <= int(v[mem]) for v in a.values())


def test_plain_seeds_are_the_first_twelve_with_a_types_rejection(golden):
    """HC.PLAIN_SEEDS is what the rule gives: scanning from 7000, the seeds whose oracle result shows a types-rejection in
    front of a fit, until there are 12 (the seeds passed over show none)"""
    import fuzzgen
    got, s = [], 7000
    while len(got) < len(HC.PLAIN_SEEDS) and s < 7100:
        prob = fuzzgen.fuzz_problem(golden, s)
        if HC.types_rejections_ahead(prob, parity.run_oracle(prob)[0]) > 0:
            got.append(s)
        s += 1
    assert got == HC.PLAIN_SEEDS
