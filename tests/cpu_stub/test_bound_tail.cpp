// TEST INFRASTRUCTURE: the tail of a headroom bound row and the unchanged-row test of a commit
// (karpenter-provider-aws_amd/csrc/kp_bound.h: kp_bound_tail_*, kp_bound_axis_kept) against a brute-force walk.
//
// 1. Packing: every axis keeps its own 16-bit type and the step keeps its 16 bits, whatever the others hold.
// 2. The rule the commit relies on, exhaustively over small type sets: T = 8 types, three axes with ties in their
//    allocatables, a rank table per axis (stable sort, largest first, as the host builds it), steps of STEP ranks.  For
//    every option set O and every subset O' of it (an Add only removes options) with every pair of witness flags per
//    axis: all axes kept  <=>  the walk over O', started from the top, finds the same type on every axis; and then it also
//    gives the same maxima, the same first step and the same stored entries, so the row the commit skips is the row it
//    would have stored.  The walk resumed at O's first step finds what the walk from the top finds.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../karpenter-provider-aws_amd/csrc/kp_bound.h"

static const int T = 8, AX = 3, STEP = 2;
static const int64_t ALLOC[AX][T] = {
    {4, 9, 9, 1, 7, 7, 3, 0},  // ties at the top and in the middle
    {5, 5, 5, 5, 5, 5, 5, 5},  // one value: the rank is the type order
    {0, 1, 2, 3, 4, 5, 6, 8},  // the best type ranks last in type order
};
static int RANK[AX][T];

struct Row {
    int64_t mx[AX];
    unsigned type[AX];
    int first;
};

// the commit's walk: per axis the first option in rank order, from step `start` on; first = the first step at which
// any axis found its option (start when none did)
static Row walk(unsigned opts, int start) {
    Row r;
    r.first = -1;
    for (int a = 0; a < AX; a++) {
        r.mx[a] = KP_NO_BOUND;
        r.type[a] = KP_BOUND_NO_TYPE;
    }
    for (int s = start; s * STEP < T; s++)
        for (int a = 0; a < AX; a++) {
            if (r.type[a] != KP_BOUND_NO_TYPE) continue;
            for (int k = s * STEP; k < (s + 1) * STEP && k < T; k++)
                if ((opts >> RANK[a][k]) & 1u) {
                    r.type[a] = (unsigned)RANK[a][k];
                    r.mx[a] = ALLOC[a][RANK[a][k]];
                    if (r.first < 0) r.first = s;
                    break;
                }
        }
    if (r.first < 0) r.first = start;
    return r;
}

static int fail(const char* what, unsigned o, unsigned o2) { return printf("%s: options %#x -> %#x\n", what, o, o2), 1; }

int main() {
    long long checked = 0;
    // ---- 1. packing ----
    static const unsigned V[] = {0, 1, 63, 64, 917, 959, 0x7FFF, 0xFFFE, KP_BOUND_NO_TYPE};
    for (int a = 0; a < KP_BOUND_TAIL_AXES; a++)
        for (unsigned v : V)
            for (unsigned bg : V)
                for (unsigned step : {0u, 1u, 14u, 0xFFFFu}) {
                    KpBoundTail t = kp_bound_tail_empty(step);
                    for (int b = 0; b < KP_BOUND_TAIL_AXES; b++) {
                        if (kp_bound_tail_type(t.lo, t.hi, b) != KP_BOUND_NO_TYPE) return printf("empty tail names a type\n"), 1;
                        kp_bound_tail_set(t, b, bg);
                    }
                    kp_bound_tail_set(t, a, v);
                    for (int b = 0; b < KP_BOUND_TAIL_AXES; b++)
                        if (kp_bound_tail_type(t.lo, t.hi, b) != (b == a ? v : bg)) return printf("axis %d reads axis %d\n", b, a), 1;
                    if (kp_bound_tail_step(t.hi) != step) return printf("the step moved\n"), 1;
                    checked++;
                }
    // ---- 2. the unchanged-row rule ----
    for (int a = 0; a < AX; a++) {
        for (int i = 0; i < T; i++) RANK[a][i] = i;
        std::stable_sort(RANK[a], RANK[a] + T, [&](int x, int y) { return ALLOC[a][x] > ALLOC[a][y]; });
    }
    for (unsigned o = 1; o < (1u << T); o++) {
        const Row r = walk(o, 0);
        for (int a = 0; a < AX; a++) {  // the walk's maximum is the brute-force maximum
            int64_t m = INT64_MIN;
            for (int t = 0; t < T; t++)
                if ((o >> t) & 1u) m = std::max(m, ALLOC[a][t]);
            if (r.mx[a] != m) return fail("walk max", o, o);
        }
        for (unsigned o2 = o;; o2 = (o2 - 1) & o) {  // every subset of o, the empty one last
            if (!o2) break;
            const Row top = walk(o2, 0), res = walk(o2, r.first);
            for (int a = 0; a < AX; a++)
                if (top.type[a] != res.type[a] || top.mx[a] != res.mx[a]) return fail("resumed walk differs", o, o2);
            if (top.first != res.first) return fail("resumed walk's first step differs", o, o2);
            const uint64_t w = o2;
            for (unsigned wf = 0; wf < (1u << (2 * AX)); wf++) {  // witness flags: stored (low AX bits) and new
                KpBoundTail t = kp_bound_tail_empty((unsigned)r.first);
                bool kept = true, same = true;
                for (int a = 0; a < AX; a++) kp_bound_tail_set(t, a, r.type[a]);
                for (int a = 0; a < AX; a++) {
                    const bool was = (wf >> a) & 1u, now = (wf >> (AX + a)) & 1u;
                    const int64_t entry = kp_bound_entry(r.mx[a], was);
                    kept = kept && kp_bound_axis_kept(kp_bound_tail_type(t.lo, t.hi, a), &w, 1, entry, now);
                    same = same && top.type[a] == r.type[a] && entry == kp_bound_entry(top.mx[a], now);
                }
                if (kept != same) return fail(kept ? "skips a row that changes" : "stores a row that does not change", o, o2);
                if (kept && top.first != (int)kp_bound_tail_step(t.hi)) return fail("kept row, other first step", o, o2);
                checked++;
            }
        }
    }
    // ---- 3. the host's per-template step (kp_bound_first_step) against a brute-force walk ----
    // 130 types with ties in three axes, rank tables padded to 192 as the host pads them; every single type, every pair
    // and sets drawn by a fixed generator: the step is the first 64-rank step in which a brute-force scan of the whole
    // table meets a type of the set, on each axis, and no step before the minimum over the axes holds one on any axis
    {
        const int T2 = 130, TP2 = 192, NW = (T2 + 63) / 64;
        static int64_t al[AX][130];
        static uint16_t rk[AX][192];
        uint32_t g = 12345u;
        auto rnd = [&]() { return g = g * 1664525u + 1013904223u, g >> 8; };
        for (int a = 0; a < AX; a++) {
            int ord[130];
            for (int t = 0; t < T2; t++) al[a][t] = (int64_t)(rnd() % (a == 0 ? 9 : a == 1 ? 40 : 1000)), ord[t] = t;
            std::stable_sort(ord, ord + T2, [&](int x, int y) { return al[a][x] > al[a][y]; });
            for (int k = 0; k < TP2; k++) rk[a][k] = k < T2 ? (uint16_t)ord[k] : (uint16_t)KP_BOUND_NO_TYPE;
        }
        auto check = [&](const uint64_t* set) -> bool {
            int mn = TP2 / 64;
            for (int a = 0; a < AX; a++) {
                int brute = TP2 / 64;
                for (int s = TP2 / 64 - 1; s >= 0; s--)
                    for (int k = 64 * s; k < 64 * s + 64; k++)
                        if (rk[a][k] != KP_BOUND_NO_TYPE && ((set[rk[a][k] >> 6] >> (rk[a][k] & 63)) & 1ull)) brute = s;
                if (kp_bound_first_step(rk[a], TP2, set) != brute) return false;
                mn = std::min(mn, brute);
            }
            for (int a = 0; a < AX; a++)  // nothing of the set before the minimum, on any axis
                for (int k = 0; k < 64 * mn && k < TP2; k++)
                    if (rk[a][k] != KP_BOUND_NO_TYPE && ((set[rk[a][k] >> 6] >> (rk[a][k] & 63)) & 1ull)) return false;
            checked++;
            return true;
        };
        uint64_t set[NW];
        for (int i = 0; i < T2; i++)
            for (int j = i; j < T2; j++) {
                for (int w = 0; w < NW; w++) set[w] = 0;
                set[i >> 6] |= 1ull << (i & 63);
                set[j >> 6] |= 1ull << (j & 63);
                if (!check(set)) return printf("per-template step differs: types %d %d\n", i, j), 1;
            }
        for (int n = 0; n < 20000; n++) {
            for (int w = 0; w < NW; w++) set[w] = 0;
            const int cnt = (int)(rnd() % 12);
            for (int i = 0; i < cnt; i++) {
                const int t = (int)(rnd() % T2);
                set[t >> 6] |= 1ull << (t & 63);
            }
            if (!check(set)) return printf("per-template step differs: drawn set %d\n", n), 1;
        }
        for (int w = 0; w < NW; w++) set[w] = 0;
        if (kp_bound_first_step(rk[0], TP2, set) != TP2 / 64) return printf("empty set finds a step\n"), 1;
    }
    // a tail that names no type, or a type past the option words, is never kept
    const uint64_t all = ~0ull;
    if (kp_bound_axis_kept(KP_BOUND_NO_TYPE, &all, 1, 5, true) || kp_bound_axis_kept(64, &all, 1, 5, true))
        return printf("keeps a type outside the option words\n"), 1;
    printf("ok: %lld combinations\n", checked);
    return 0;
}
