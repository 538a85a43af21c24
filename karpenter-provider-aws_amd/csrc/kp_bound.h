// kp_bound.h — the Solve's headroom bound of an in-flight NodeClaim (DESIGN.md §4 "Headroom bound"): the row the
// slow path's commits keep per NodeClaim and the test the candidate collection applies to it.  Plain C++ on both sides,
// so the pair is checked exhaustively on the CPU (tests/cpu_stub/test_bound.cpp).
//
// NodeClaim.Add keeps an instance type only when resources.Fits(requests + pod, Allocatable): on every axis the total
// is <= the type's allocatable (an axis with a total <= 0 is not compared).  The options of a NodeClaim only shrink and
// its total only grows, so once total + pod exceeds, on one axis, the largest allocatable any option has there, no
// option can fit the pod: the Add rejects, and keeps rejecting pods of that shape.
//
// The row holds that largest allocatable itself, unscaled, and the test reads the NodeClaim's exact request total (the
// one the evaluation would read).  The quick-accept witness rows are no base for it: they are decremented by the
// rounded-up request of every quick accept, so they fall below the true headroom on an axis with qshift > 0 — safe for
// accepting, wrong by any number of quanta for rejecting.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KP_BOUND_HD __host__ __device__ inline
#else
#define KP_BOUND_HD inline
#endif

#define KP_BOUND_STRIDE 8       // entries per row (> KP_LDS_AXES): a row is one 64-byte line; the last two keep the commit's tail
#define KP_NO_BOUND INT64_MAX  // row entry of an axis that gives no bound (a NodeClaim without a quick-accept witness)

// The row's tail, entries KP_BOUND_STRIDE - 2 and - 1 (no axis is staged there): per staged axis the type that gave the
// axis' maximum, 16 bits each (axes 0-3 in the first entry, axes 4-5 in the low half of the second), and in the top 16
// bits of the second the step of the rank table at which the commit's walk resumes.  A commit whose accepted options still
// hold every one of those types leaves every maximum as it is, and with it the step: the row is not computed again
// (checked against a brute-force walk by tests/cpu_stub/test_bound_tail.cpp).
#define KP_BOUND_TAIL_AXES 6
#define KP_BOUND_NO_TYPE 0xFFFFu  // tail entry of an axis no option was found on (alloc_rank's padding value)
struct KpBoundTail {
    uint64_t lo, hi;
};
KP_BOUND_HD KpBoundTail kp_bound_tail_empty(unsigned step) {
    return KpBoundTail{~0ull, 0x0000FFFFFFFFFFFFull | ((uint64_t)(step & 0xFFFFu) << 48)};
}
KP_BOUND_HD void kp_bound_tail_set(KpBoundTail& t, int axis, unsigned type) {
    uint64_t& w = axis < 4 ? t.lo : t.hi;
    const int sh = 16 * (axis & 3);
    w = (w & ~(0xFFFFull << sh)) | ((uint64_t)(type & 0xFFFFu) << sh);
}
KP_BOUND_HD unsigned kp_bound_tail_type(uint64_t lo, uint64_t hi, int axis) {
    return (unsigned)(((axis < 4 ? lo : hi) >> (16 * (axis & 3))) & 0xFFFFu);
}
KP_BOUND_HD unsigned kp_bound_tail_step(uint64_t hi) { return (unsigned)(hi >> 48); }
// The first step (64 ranks each) of one axis' rank table (rank[TP]: type ids by allocatable, largest first, KP_BOUND_NO_TYPE
// padding) at which a type of the set (bit t of set: type t) appears; TP / 64 when none does.  The host takes the
// minimum over the staged axes for each template's instance types (KpDev::tmpl_bstep): the walk of a NodeClaim being
// created from the template finds nothing before that step, so it starts there.
KP_BOUND_HD int kp_bound_first_step(const uint16_t* rank, int TP, const uint64_t* set) {
    for (int k = 0; k < TP; k++) {
        const unsigned t = rank[k];
        if (t != KP_BOUND_NO_TYPE && ((set[t >> 6] >> (t & 63)) & 1ull)) return k >> 6;
    }
    return TP >> 6;
}
// One axis of the unchanged-row test: the type that gave the maximum is still an option (opts: the accepted Add's option
// words, nw of them) and the witness flag the entry was stored with (kp_bound_entry) is the one the Add leaves.
KP_BOUND_HD bool kp_bound_axis_kept(unsigned type, const uint64_t* opts, int nw, int64_t entry, bool witness) {
    return type < (unsigned)(64 * nw) && ((opts[type >> 6] >> (type & 63)) & 1ull) && ((entry != KP_NO_BOUND) == witness);
}

// Row entry of one staged axis: max_alloc = the largest allocatable on the axis over the NodeClaim's options; witness:
// the commit left a quick-accept witness on the axis (WaveScratch.hr >= 0; not so for minValues templates and
// NodeClaims that hold reserved offerings, whose every Add runs in full).
KP_BOUND_HD int64_t kp_bound_entry(int64_t max_alloc, bool witness) { return witness ? max_alloc : KP_NO_BOUND; }

// The pod (request pod on the axis) cannot be added to the NodeClaim (request total `total`, row entry `bound`) whatever
// option is tried.  Never true when some option has total + pod <= allocatable on the axis.
KP_BOUND_HD bool kp_bound_rejects(int64_t bound, int64_t total, int64_t pod) {
    return pod > 0 && bound != KP_NO_BOUND && total > bound - pod;
}
