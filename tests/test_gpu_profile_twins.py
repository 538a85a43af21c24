"""GPU: the Solve kernels' production entry points against their diagnostic twins (ffd_solve PROF, launched when
KPSIM_PROFILE is set at prepare).  One small seeded problem per instantiation family — plain, topology, reserved
offerings, preference relaxation — solved once by each: identical results, identical kp_solve_stats (timings aside) and
always-on counters; the stage cycles and n_* counters are written by the twin alone and read 0 from the production
kernel.  Each problem reaches the block path and the templates (asserted on the oracle's result and the device's
slow-path count).

The *_hbm_kernel twins run in tests/test_gpu_dense_plans.py (test_dense_twin: base and topology at 18,100 pods): the
slice arrays move to HBM only for solves planned for more NodeClaims than LDS holds, which no problem of a few hundred
pods reaches."""
import ctypes as C
import os

import numpy as np
import pytest

import fuzzgen
import parity
import pyoracle
from kpsim import abi, model, native, synth

pytestmark = pytest.mark.gpu

# kp_last_kernel_times [5..]: the FFD kernel's counters (tools/prof_solve.py NAMES), then the failed evaluations by
# stage and the hand-off stamps
NAMES = ["cyc_fast_loop", "cyc_sort", "cyc_slow_eval", "cyc_templates", "-", "cyc_sort_full", "ev_req", "ev_mask",
         "ev_off", "ev_types", "ev_min", "ev_calls", "quick_accepts", "slow_pods", "witness_misses", "cyc_q_pop",
         "cyc_q_scan", "cyc_q_check", "cyc_q_commit", "n_noinv", "n_winmove", "n_ldssort", "n_pivot", "n_winload",
         "n_flush", "n_shape", "n_lds_append", "n_lds_nowin", "n_lds_outside", "n_batches", "topo_quick",
         "cyc_topo_setup", "cyc_topo_scan", "rej_requirements", "rej_topology", "rej_types", "rej_min_values",
         "cyc_ho_entry", "cyc_ho_failed_check", "cyc_ho_flush_collect", "cyc_ho_writeback"]
ALWAYS = ["quick_accepts", "slow_pods", "witness_misses", "ev_calls", "topo_quick", "rej_requirements", "rej_topology",
          "rej_types", "rej_min_values"]
# written by the twin alone: the stage cycles (cyc_*, and ev_req .. ev_min) and the n_* counters
PROFILING_ONLY = [n for n in NAMES if n.startswith(("cyc_", "n_"))] + ["ev_req", "ev_mask", "ev_off", "ev_types", "ev_min"]


def _sub(cat, seed, n):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [cat[int(i)] for i in sorted(rng.choice(len(cat), size=n, replace=False))]


def plain_problem(golden):
    return fuzzgen.fuzz_problem(_sub(golden, 9101, 160), 9101, n_pods=300), abi.KP_PREFERENCE_RESPECT


def topology_problem(golden):
    return fuzzgen.fuzz_topology_problem(_sub(golden, 9102, 160), 9102, n_pods=200), abi.KP_PREFERENCE_RESPECT


def reserved_problem(golden):
    """fuzz_problem over a catalog with reserved offerings, its NodePools open to them (the RESV instantiations with the
    ReservationManager on)."""
    cat = synth.config5_catalog(golden)
    held = [it for it in cat if any(o.capacity_type == "reserved" for o in it.offerings)]
    rest = [it for it in cat if not any(o.capacity_type == "reserved" for o in it.offerings)]
    sub = held[:40] + _sub(rest, 9103, 120)
    prob = fuzzgen.fuzz_problem(sub, 9103, n_pods=300)
    for np_ in prob.nodepools:
        np_.requirements = [r for r in np_.requirements if r.key != model.CAPACITY_TYPE]
        np_.requirements.append(model.Requirement(model.CAPACITY_TYPE, "In", ["reserved", "on-demand", "spot"]))
    return prob, abi.KP_PREFERENCE_RESPECT


def preference_problem(golden):
    prob = fuzzgen.fuzz_problem(_sub(golden, 9104, 160), 9104, n_pods=300)
    fuzzgen.add_preferences(np.random.Generator(np.random.PCG64(9104)), prob)
    assert any(pc.preferred_terms for pc in prob.classes)
    return prob, abi.KP_PREFERENCE_RESPECT


FAMILIES = {"plain": plain_problem, "topology": topology_problem, "reserved": reserved_problem,
            "preference": preference_problem}


def _counters(ctx):
    a = (C.c_double * (5 + len(NAMES)))()
    ctx.check(ctx.L.kp_last_kernel_times(ctx.h, a, len(a)), "kp_last_kernel_times")
    return dict(zip(NAMES, list(a)[5:]))


def _solve(prob, policy, profile, want_plan=False):
    """(result, counters) of one solve on a fresh ctx, KPSIM_PROFILE set or unset at prepare; want_plan: and the plan
    of the solve (Context.solve_plan)"""
    old = os.environ.pop("KPSIM_PROFILE", None)
    if profile:
        os.environ["KPSIM_PROFILE"] = "1"
    ctx = native.Context(0, preference_policy=policy)
    try:
        dev = parity.run_device(ctx, prob)
        return (dev, _counters(ctx), ctx.solve_plan()) if want_plan else (dev, _counters(ctx))
    finally:
        ctx.close()
        os.environ.pop("KPSIM_PROFILE", None)
        if old is not None:
            os.environ["KPSIM_PROFILE"] = old


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_production_kernel_matches_its_twin(golden, family):
    prob, policy = FAMILIES[family](golden)
    o = pyoracle.solve(prob, preference_policy=policy)
    orc = o.results, [model.parse_requirements_blob(o.requirements(i)) for i in range(o.results.n_nodeclaims)]
    # the problem reaches the templates (a new NodeClaim) and, below, the block path (a slow-path pod)
    assert orc[0].n_nodeclaims >= 1 and (orc[0].pod_result >= 0).any()

    plain, cp = _solve(prob, policy, profile=False)
    twin, ct = _solve(prob, policy, profile=True)
    print(family, {k: (cp[k], ct[k]) for k in NAMES if k != "-"})
    parity.assert_same(plain, orc)
    parity.assert_same(twin, plain)
    for f, _ in abi.kp_solve_stats._fields_:
        if not f.startswith("ns_"):
            assert plain[0].stats[f] == twin[0].stats[f], f
    assert cp["slow_pods"] >= 1
    for k in ALWAYS:
        assert cp[k] == ct[k], k
    assert ct["cyc_fast_loop"] > 0
    for k in PROFILING_ONLY:
        assert cp[k] == 0, k
    if family == "preference":
        assert plain[0].stats["pods_popped"] > prob.pods.n  # a pod was requeued (relaxed, or retried after a failure)
