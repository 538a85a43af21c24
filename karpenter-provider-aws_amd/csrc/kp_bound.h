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

#define KP_BOUND_STRIDE 8       // entries per row (> KP_LDS_AXES): a row is one 64-byte line; the last keeps the commit's walk step
#define KP_NO_BOUND INT64_MAX  // row entry of an axis that gives no bound (a NodeClaim without a quick-accept witness)

// Row entry of one staged axis: max_alloc = the largest allocatable on the axis over the NodeClaim's options; witness:
// the commit left a quick-accept witness on the axis (WaveScratch.hr >= 0; not so for minValues templates and
// NodeClaims that hold reserved offerings, whose every Add runs in full).
KP_BOUND_HD int64_t kp_bound_entry(int64_t max_alloc, bool witness) { return witness ? max_alloc : KP_NO_BOUND; }

// The pod (request pod on the axis) cannot be added to the NodeClaim (request total `total`, row entry `bound`) whatever
// option is tried.  Never true when some option has total + pod <= allocatable on the axis.
KP_BOUND_HD bool kp_bound_rejects(int64_t bound, int64_t total, int64_t pod) {
    return pod > 0 && bound != KP_NO_BOUND && total > bound - pod;
}
