"""CPU: the full pdqsort emulation's short ranges and its sampled choosePivot (csrc/kp_gosort_core.h; DESIGN.md §4
step 3; GPU companion: tests/test_gpu_sort_ranges.py).

A stand-alone C++ program (tests/cpu_stub/test_gosort_ranges.cpp) runs the core header on the host: the driver that hands
short popped ranges to a range policy (threshold 63 as on the device, and 20 and 13) against the plain sorter and against
GoSlice (csrc/kp_gosort_host.h), on every n from 13 to 600 with one changed element at every position, on random and
adversarial arrays, and the (value, index) pivot network against go_choose_pivot.  It is built once plainly and once with
the host sanitizers (address, undefined); the sanitized build is skipped where the compiler has no runtime for them.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_stub")
SRC = os.path.join(HERE, "test_gosort_ranges.cpp")


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("pivot network:") and lines[-1].startswith("ok:"), r.stdout[-2000:]


def test_gosort_ranges(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_gosort_ranges")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, SRC])
    _run(exe)


def test_gosort_ranges_sanitized(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    san = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(san + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("g++ has no address / undefined sanitizer runtime")
    exe = str(tmp_path / "test_gosort_ranges_san")
    c = subprocess.run(san + ["-o", exe, SRC], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    _run(exe)
