"""CPU: tests/cons_explain_ref.py (the expectation for kp_consolidate_explain) pinned to the unmodified oracle, and the
bindings of the four entry points.

For every probe of both modes over the corpus, the restated (decision, valid, n_replacement_types, replacement_price)
equals pyoracle.consolidate's row and the restated reason is consistent with it.  The corpus must produce every reason.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cons_explain_ref as cxr
import pyoracle
from kpsim import abi, model

MODES = (abi.KP_CONSOLIDATE_SINGLE, abi.KP_CONSOLIDATE_MULTI)
PRICE_REASONS = (abi.KP_UNCONS_SPOT_TO_SPOT_DISABLED, abi.KP_UNCONS_MIN_VALUES, abi.KP_UNCONS_NOT_CHEAPER,
                 abi.KP_UNCONS_SPOT_TO_SPOT_TOO_FEW)
CASES = [("fuzz", s) for s in range(24)] + [("min", s) for s in range(8)]

_golden = None


@functools.lru_cache(maxsize=None)
def restated(family, seed):
    """{mode: (rows, decisions, oracle rows)} of one corpus case, computed once"""
    cp, s2s = (cxr.fuzz_case if family == "fuzz" else cxr.min_values_case)(_golden, seed)
    ref = cxr.ConsRef(cp, s2s)
    out = {}
    for mode in MODES:
        rows, dec = ref.rows(mode)
        out[mode] = (rows, dec, pyoracle.consolidate(cp, mode, spot_to_spot=s2s))
    return out


def check_consistent(row, orc):
    """the reason against the oracle's kp_probe_result row of the same probe"""
    r = int(row["reason"])
    assert (r == abi.KP_UNCONS_NONE) == (orc["decision"] != abi.KP_DECISION_NONE and orc["valid"] == 1)
    assert (r == abi.KP_UNCONS_SAME_INSTANCE_TYPE) == (orc["decision"] == abi.KP_DECISION_REPLACE and orc["valid"] == 0)
    assert (r == abi.KP_UNCONS_MULTIPLE_NODECLAIMS) == (orc["n_new_nodeclaims"] == 2)
    assert (r == abi.KP_UNCONS_PODS_UNSCHEDULABLE) == (orc["n_new_nodeclaims"] < 2 and orc["all_scheduled"] == 0)
    if r in PRICE_REASONS:
        assert orc["all_scheduled"] == 1 and orc["n_new_nodeclaims"] == 1 and orc["decision"] == abi.KP_DECISION_NONE
    assert row["candidate_price"] == orc["candidate_price"]


@pytest.mark.parametrize("family,seed", CASES)
def test_restatement_matches_oracle(golden, family, seed):
    global _golden
    _golden = golden
    for mode, (rows, dec, orc) in restated(family, seed).items():
        assert len(rows) == len(orc)
        for i in range(len(orc)):
            o = orc[i]
            check_consistent(rows[i], o)
            if o["n_new_nodeclaims"] == 2:
                continue  # (the oracle goes on past the second NodeClaim; the decision is NONE either way)
            assert dec[i] == (o["decision"], o["valid"], o["n_replacement_types"], o["replacement_price"]), (mode, i)


def test_corpus_produces_every_reason(golden):
    global _golden
    _golden = golden
    seen = {m: set() for m in MODES}
    flags = 0
    for family, seed in CASES:
        for mode, (rows, _dec, _orc) in restated(family, seed).items():
            seen[mode] |= set(int(x) for x in rows["reason"])
            flags |= int(np.bitwise_or.reduce(rows["flags"])) if len(rows) else 0
    single = seen[abi.KP_CONSOLIDATE_SINGLE]
    assert single >= {abi.KP_UNCONS_NONE, abi.KP_UNCONS_PODS_UNSCHEDULABLE, abi.KP_UNCONS_MULTIPLE_NODECLAIMS,
                      abi.KP_UNCONS_SPOT_TO_SPOT_DISABLED, abi.KP_UNCONS_MIN_VALUES, abi.KP_UNCONS_NOT_CHEAPER,
                      abi.KP_UNCONS_SPOT_TO_SPOT_TOO_FEW}, sorted(single)
    assert abi.KP_UNCONS_SAME_INSTANCE_TYPE not in single
    multi = seen[abi.KP_CONSOLIDATE_MULTI]
    assert multi & {abi.KP_UNCONS_SAME_INSTANCE_TYPE, abi.KP_UNCONS_NONE}, sorted(multi)
    assert flags & abi.KP_UNCONS_F_SPOT_TO_SPOT


def test_first_family_single_mode_counts(golden):
    """The oracle's own single-mode rows over the first family's 24 seeds: 51 commands, 93 not-all-scheduled, 112 with a
    second NodeClaim (counted first, as the device stops there), 32 NONE for a price reason, and the restatement splits
    exactly those 32 into the four price reasons."""
    global _golden
    _golden = golden
    cmd = unsched = second = other = price = 0
    for seed in range(24):
        rows, _dec, orc = restated("fuzz", seed)[abi.KP_CONSOLIDATE_SINGLE]
        for i in range(len(orc)):
            o = orc[i]
            if o["decision"] != abi.KP_DECISION_NONE:
                cmd += 1
            elif o["n_new_nodeclaims"] == 2:
                second += 1
            elif not o["all_scheduled"]:
                unsched += 1
            else:
                other += 1
            price += int(rows[i]["reason"]) in PRICE_REASONS
    assert (cmd, unsched, second, other) == (51, 93, 112, 32)
    assert price == other


def test_bindings():
    from kpsim import native
    for f in ("kp_consolidate_explain", "kp_consolidate_explain_pods", "kp_consolidate_explain_key",
              "kp_consolidate_explain_stats"):
        assert f in native.EXPORTS
    # the header's struct: eight int32 and two doubles
    assert C.sizeof(abi.kp_probe_explanation) == 8 * 4 + 2 * 8
    assert abi.PROBE_EXPLANATION_DTYPE.itemsize == C.sizeof(abi.kp_probe_explanation)
    assert (abi.KP_UNCONS_NONE, abi.KP_UNCONS_SAME_INSTANCE_TYPE) == (0, 7)
    assert (abi.KP_UNCONS_F_UNINITIALIZED_NODE, abi.KP_UNCONS_F_TRUNCATED, abi.KP_UNCONS_F_SPOT_TO_SPOT) == (1, 2, 4)
    assert model.consolidation_probe_count(5, abi.KP_CONSOLIDATE_MULTI) == 4
