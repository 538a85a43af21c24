#!/usr/bin/env python3
"""Digests of the fuzz generators' default path (tests/fuzzgen.py without a zones= argument): seeds 0-3 of
fuzz_problem, fuzz_topology_problem, fuzz_topology_existing_problem and fuzz_consolidation over a seeded 160-type
sample of the golden catalog, each solved by the CPU oracle (edge_cases.fuzz_default_digests).  Written to
tests/golden/fuzz_digests.json; tests/test_word_edges_cpu.py re-derives them, so a change of the generators that moves
an rng draw of the default path (and with it every committed fuzz seed of the suite) shows.

    python tests/golden/gen_fuzz_digests.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "karpenter-provider-aws_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

from kpsim import catalog  # noqa: E402
import edge_cases  # noqa: E402


def main():
    cat = catalog.golden_catalog(fx=catalog.load_fixtures())
    with open(os.path.join(HERE, "fuzz_digests.json"), "w") as f:
        json.dump(edge_cases.fuzz_default_digests(cat), f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
