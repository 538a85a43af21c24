"""Run by tests/test_gpu_word_edges.py in a child process with KPSIM_PREP_SPLIT_MIN=1, so kp_solve_prepare takes its
two-thread pod_rows / pod_keys split at these pod counts: solves the problems of prep_split_problems() on cuda:0 and
prints one JSON object, name -> parity.result_digest of the device result.  The parent compares with the oracle."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "karpenter-provider-aws_amd"), HERE, os.path.join(HERE, "..", "oracle")]

import edge_cases  # noqa: E402
import fuzzgen  # noqa: E402
import parity  # noqa: E402
from kpsim import catalog, native  # noqa: E402


def prep_split_problems(golden):
    sub = edge_cases.sample(golden, 160, 8800)
    out = {"fuzz_%d" % s: fuzzgen.fuzz_problem(sub, s, n_pods=300) for s in range(4)}
    out["topology_existing"] = fuzzgen.fuzz_topology_existing_problem(sub, 8801, n_pods=200)
    return out


def main():
    golden = catalog.golden_catalog(fx=catalog.load_fixtures())
    ctx = native.Context(0)
    out = {}
    try:
        for name, prob in prep_split_problems(golden).items():
            out[name] = parity.result_digest(parity.run_device(ctx, prob))
    finally:
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
