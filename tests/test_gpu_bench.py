"""GPU: a plain bench.py run — its result line, and --dump-outputs against a kp_solve of the same seeded input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import parity
from kpsim import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PODS = 3000  # several NodeClaims and both NodePools of config2; one run takes about a second


def test_plain_run_dumps_the_last_step(tmp_path, golden):
    d = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--pods", str(PODS), "--dump-outputs", d], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "pods/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(PODS / (line["ms_per_step"] / 1e3), rel=1e-9)
    # the other legs, baselines and checks belong to --full
    for k in ("consolidation", "launch", "topology", "reserved", "cpu_baseline", "roofline", "solve_call_warm"):
        assert k not in line

    from kpsim import native
    ctx = native.Context(0)
    try:
        r, _ = parity.run_device(ctx, synth.config2(n_pods=PODS, catalog=golden))
    finally:
        ctx.close()
    assert r.n_nodeclaims > 1
    off = np.concatenate([[0], np.cumsum([len(t) for t in r.nodeclaim_types])])
    want = {"pod_result": r.pod_result, "pod_order": r.pod_order, "nodeclaim_nodepool": r.nodeclaim_nodepool,
            "nodeclaim_n_pods": r.nodeclaim_n_pods, "nodeclaim_slice_pos": r.nodeclaim_slice_pos,
            "nodeclaim_n_options": r.nodeclaim_n_options, "nodeclaim_type_offset": off,
            "type_ids": np.array([t for ts in r.nodeclaim_types for t in ts])}
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in want)
    for k, w in want.items():
        got = np.load(os.path.join(d, k + ".npy"))
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, np.asarray(w, np.float64), err_msg=k)
