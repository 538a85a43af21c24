#!/usr/bin/env python3
"""FFD-kernel phase profile of one Solve (KPSIM_PROFILE=1: s_memtime cycle counters inside ffd_kernel).

    KPSIM_PROFILE=1 python tools/prof_solve.py [config2|config3|config5] [n_pods]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "karpenter-provider-aws_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

from kpsim import catalog, model, native, synth  # noqa: E402

NAMES = ["cyc_fast_loop", "cyc_sort", "cyc_slow_eval", "cyc_templates", "-", "cyc_sort_full", "ev_req", "ev_mask",
         "ev_off", "ev_types", "ev_min", "ev_calls", "quick_accepts", "slow_pods", "witness_misses", "cyc_q_pop",
         "cyc_q_scan", "cyc_q_check", "cyc_q_commit", "n_noinv", "n_winmove", "n_ldssort", "n_pivot", "n_winload",
         "n_flush", "n_shape", "n_lds_append", "n_lds_nowin", "n_lds_outside", "n_batches", "topo_quick",
         "cyc_topo_setup", "cyc_topo_scan", "rej_requirements", "rej_topology", "rej_types", "rej_min_values",
         # wave 0's hand-off of a pod to the block, by part (kp_layout.h ST_HANDOFF)
         "cyc_ho_entry", "cyc_ho_failed_check", "cyc_ho_flush_collect", "cyc_ho_writeback",
         # wave 0's same-shape inner loop (kp_layout.h ST_N_INNER): pods it took without a pass through the general loop
         # and the cycles of their steps; cyc_q_check holds the checks and batches of both loops
         "n_inner", "cyc_q_inner", "n_multi",
         # slow-path candidates the headroom bound rejected without an evaluation (kp_layout.h ST_BOUND_SKIPS, always
         # exact), the candidate rounds made of them alone and the rounds that mix them with evaluated candidates
         "bound_skips", "rounds_all_virtual", "rounds_mixed",
         # the full pdqsort emulations of a slice longer than 64 (they start over LDS) and their share of cyc_sort_full
         # (kp_layout.h ST_SORT_FULL_WIDE; a solve with topology groups reports its topology quick-accept iterations here)
         "sorts_full_n_gt_64", "cyc_sort_full_n_gt_64"]


def ffd_counters(ctx):
    """kp_last_kernel_times [5..]: every FFD-kernel counter, the hand-off stamps past Context.ffd_cycles()'s 37 included."""
    import ctypes as C
    a = (C.c_double * (5 + len(NAMES)))()
    ctx.check(ctx.L.kp_last_kernel_times(ctx.h, a, len(a)), "kp_last_kernel_times")
    return list(a)[5:]


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "config3"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 50_000
    cat = catalog.golden_catalog()
    if which == "config5":
        cat = synth.config5_catalog(cat)
    prob = getattr(synth, which)(n_pods=n, catalog=cat)
    ctx = native.Context(0)
    ctx.upload_catalog(model.CatalogView(cat))
    iv = model.SolveInputView(prob)
    out = model.OutputBuffers(prob.pods.n, prob.pods.n + 16, (prob.pods.n + 16) * 60)
    import time
    t = time.perf_counter()
    ctx.solve(iv, out)
    wall = (time.perf_counter() - t) * 1e3
    r = out.results()
    kt = ctx.kernel_times_ms()
    ffd = dict(zip(NAMES, ffd_counters(ctx)))
    # entries to wave 0's general loop: one per batch that the inner loop did not start, one per pod handed to the block
    ffd["general_loop_entries"] = ffd["n_batches"] - ffd["n_inner"] + ffd["slow_pods"]
    # the kernels that carry the headroom bound have no topology section and count, in the slot of its setup cycles, the
    # in-flight commits that stored their NodeClaim's bound row again (kp_layout.h ST_BOUND_ROWS, kpsim.h [36])
    if which == "config2":
        ffd["bound_rows_stored"] = ffd.pop("cyc_topo_setup")
    # the split of the full sorts: the ones of at most 64 elements run in registers from the start
    ffd["sorts_full_n_le_64"] = r.stats["sorts_full"] - ffd["sorts_full_n_gt_64"]
    ffd["cyc_sort_full_n_le_64"] = ffd["cyc_sort_full"] - ffd["cyc_sort_full_n_gt_64"]
    print(json.dumps({"config": which, "pods": n, "wall_ms": wall, "kernel_ms": kt, "nodeclaims": r.n_nodeclaims, "stats": r.stats,
                      "ffd": ffd}, indent=1))
    ctx.close()


if __name__ == "__main__":
    main()
