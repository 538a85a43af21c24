"""CPU: the tail of a headroom bound row and the unchanged-row test of a commit (DESIGN.md §4 "Headroom bound";
csrc/kp_bound.h: kp_bound_tail_*, kp_bound_axis_kept; GPU companion: tests/test_gpu_bound_rows.py).

A stand-alone C++ program (tests/cpu_stub/test_bound_tail.cpp) checks the packing and, exhaustively over small type sets,
that a commit leaves a row alone exactly when the walk would have stored the same row.  It is built once plainly and once
with the host sanitizers (address, undefined); the sanitized build is skipped where the compiler has no runtime for them.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_stub")
SRC = os.path.join(HERE, "test_bound_tail.cpp")


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("ok:")


def test_bound_tail_exhaustive(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_bound_tail")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, SRC])
    _run(exe)


@pytest.fixture(scope="module")
def cases(golden):
    import bound_rows_cases as BC
    return BC.build(golden)


def _names():
    import bound_rows_cases as BC
    return BC.NAMES


@pytest.mark.parametrize("name", _names())
def test_constructed_inputs(cases, name):
    """each input yields the NodeClaim count its construction intends and places every pod, and its last shape (the
    1.5-cpu pods of the row cases, the 2-cpu pods of the others) adds at least the intended rejections in NodeClaim
    evaluations over the same input without those pods"""
    import parity
    from kpsim import model
    case = cases[name]
    orc = parity.run_oracle(case.problem)[0]
    assert orc.n_nodeclaims == case.n_nodeclaims
    assert (orc.pod_result != -1).all()
    p = case.problem
    keep = p.pods.class_id != (2 if name.startswith(("narrowed", "kept")) else 1)
    base = model.Problem(p.catalog, p.nodepools, p.classes,
                         model.Pods(p.pods.class_id[keep], p.pods.requests[keep], p.pods.creation_ns[keep],
                                    [u for u, k in zip(p.pods.uids, keep) if k]), p.existing)
    orb = parity.run_oracle(base)[0]
    if not name.endswith("_at"):  # (there the small pods fit: the rejections are among the big pods themselves)
        assert orc.stats["nodeclaim_evals"] - orb.stats["nodeclaim_evals"] >= case.min_skips


def test_rank_edges(golden):
    """the rank-edge pools hold the type at positions 63, 64 and 896 of their axis' rank table, the step edges of a
    64-rank walk over 918 types; the row cases' NodePool (BC.HC.LOOSE_TYPES) ranks below the first step on cpu and
    memory, so its NodeClaims' rows keep a resume step above 0 and their narrowing commits resume from it"""
    import bound_rows_cases as BC
    from kpsim import model
    assert len(golden) == 918 and (len(golden) + 63) // 64 * 64 == 960 and BC.EDGES == {"r63": 63, "r64": 64, "last": 896}
    for res in ("cpu", "memory"):
        a = [int(it.allocatable[model.RIDX[res]]) for it in golden]
        for pos in BC.EDGES.values():
            t = BC.rank_position(golden, res, pos)
            above = sum(1 for v in a if v > a[t])
            ties_before = sum(1 for u in range(t) if a[u] == a[t])
            assert above + ties_before == pos
        for r in BC.HC.SC.rows(golden, BC.HC.LOOSE_TYPES):
            assert sum(1 for v in a if v > a[r]) >= 64


def test_row_cases_by_arithmetic(golden):
    """narrowed: 7 + 1.5 cpu passes the cpu-rich type's allocatable and exceeds the memory-rich type's; a second opener
    passes each axis' maximum and fits neither type.  disjoint: the 13-cpu NodeClaim keeps room for a 2-cpu pod and for
    no 5- or 7-cpu pod"""
    import bound_rows_cases as BC
    from kpsim import model
    cpu, mem = model.RIDX["cpu"], model.RIDX["memory"]
    rich, memr = (golden[r].allocatable for r in BC.HC.SC.rows(golden, BC.HC.LOOSE_TYPES))
    gi = (1 << 30) * 1000
    assert 7000 + 1500 <= int(rich[cpu]) and 7000 + 1500 > int(memr[cpu]) and 7000 <= int(memr[cpu])
    assert 22 * gi <= int(rich[mem]) and 21 * gi <= int(memr[mem])
    assert 10000 <= int(rich[cpu]) and 40 * gi <= int(memr[mem])
    assert 10000 > int(memr[cpu]) and 40 * gi > int(rich[mem])
    assert 13000 + 2000 <= int(rich[cpu]) < 13000 + 5000


def test_bound_tail_sanitized(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    san = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(san + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("g++ has no address / undefined sanitizer runtime")
    exe = str(tmp_path / "test_bound_tail_san")
    c = subprocess.run(san + ["-o", exe, SRC], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    _run(exe)
