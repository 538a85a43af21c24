// TEST INFRASTRUCTURE: the pdqsort_func emulation of karpenter-provider-aws_amd/csrc/kp_gosort_core.h on the host.
//
// 1. Short ranges (kp_gosort_core.h "Short ranges", the device's WaveLds::hand_over): a driver over a bounds-checked
//    array hands every popped range that fits CAP = T + 1 elements with its predecessor to a range policy, a copy of
//    [a-1, b) (or [0, b)) that fails on any index outside it and on any write to a-1, runs pdqsort_from on it from the
//    popped entry with the stack continuing at the same depth, and copies [a, b) back.  T = 63 is the device's; 20 and
//    13 make small n take nested hand-overs.  The driver's own choosePivot is the sampled-value network (2.), as on the
//    device.  The final ord permutation must equal the plain pdqsort_full's and GoSlice's (kp_gosort_host.h, the
//    independent restatement).  The stack is a heap block of the kernel's 64 entries, so a deeper stack is an error
//    under the address sanitizer.
//    Inputs: every n in [13, 600]; per n a sorted key array in runs of equal keys (run lengths 1, 2, 7, 64, random) with
//    one element bumped by one, at every position (kind 1: a NodeClaim gained a pod), and with a key of 1 appended
//    (kind 2: a NodeClaim was appended); seeded random arrays over small and large alphabets, reversed, all equal and
//    organ-pipe arrays; and the same arrays entered with limit 0, 1 and 2, which reach heapSort on the whole slice and on
//    sub-ranges.
// 2. go_choose_pivot_vals, the (value, index) network, against go_choose_pivot for pivot and hint: every assignment of
//    a 3-symbol alphabet to the 9 (l >= 50) or 3 (8 <= l < 50) sampled positions, plus random keys, at several (a, b).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../karpenter-provider-aws_amd/csrc/kp_gosort_core.h"
#include "../../karpenter-provider-aws_amd/csrc/kp_gosort_host.h"

#define KEYMASK 0x7FFFFFFFu  // bit 31 carries a memo on the device and takes no part in the order

struct Elem {
    uint32_t key, ord;
};

[[noreturn]] static void die(const char* what, long a = 0, long b = 0, long c = 0) {
    printf("FAIL: %s (%ld, %ld, %ld)\n", what, a, b, c);
    exit(1);
}

struct Arr {
    Elem* e;
    int n;
    Elem& at(int i) const {
        if (i < 0 || i >= n) die("index outside the slice", i, n);
        return e[i];
    }
};

static long g_handovers, g_nested, g_swaps_range;

// the plain sorter's policy
struct Plain {
    Arr d;
    static constexpr bool kRanges = false;
    static int uni(int v) { return v; }
    bool less(int i, int j) const { return (d.at(i).key & KEYMASK) < (d.at(j).key & KEYMASK); }
    void swap(int i, int j) {
        const Elem t = d.at(i);
        d.at(i) = d.at(j);
        d.at(j) = t;
    }
};

// the register-range policy: CAP "lanes" holding [base, b); index i is lane i - base
struct Range {
    Elem lane[64];
    int base, a, b;
    static constexpr bool kRanges = false;
    static int uni(int v) { return v; }
    const Elem& rd(int i) const {
        if (i < base || i >= b || i < a - 1) die("range policy reads outside [a-1, b)", i, a, b);
        return lane[i - base];
    }
    bool less(int i, int j) const { return (rd(i).key & KEYMASK) < (rd(j).key & KEYMASK); }
    void swap(int i, int j) {
        if (i < a || i >= b || j < a || j >= b) die("range policy writes outside [a, b)", i, j, a);
        const Elem t = lane[i - base];
        lane[i - base] = lane[j - base];
        lane[j - base] = t;
        g_swaps_range++;
    }
    // the scans the device answers with one ballot over its lanes (kp_gosort_core.h "scans"), here as loops
    uint32_t key_at(int i) const { return rd(i).key & KEYMASK; }
    template <class F>
    int find_first(int lo, int hi, F pred) const {
        if (lo > hi + 1) die("scan bounds", lo, hi);
        for (int q = lo; q <= hi; q++)
            if (pred(key_at(q))) return q;
        return hi + 1;
    }
    template <class F>
    int find_last(int lo, int hi, F pred) const {
        if (lo > hi + 1) die("scan bounds", lo, hi);
        for (int q = hi; q >= lo; q--)
            if (pred(key_at(q))) return q;
        return lo - 1;
    }
    int first_descent(int i, int e) const {
        if (i <= base && i < e) die("first_descent asks the first lane for its predecessor", i, base);
        for (int q = i; q < e; q++)
            if (key_at(q) < key_at(q - 1)) return q;
        return e;
    }
};
// the register sorter's scan functions (kp_gosort.h KP_SORT_REG_SCANS)
static int go_partition(Range& d, int a, int b, int pivot, bool& already) { return go_partition_scans(d, a, b, pivot, already); }
static int go_partition_equal(Range& d, int a, int b, int pivot) { return go_partition_equal_scans(d, a, b, pivot); }
static bool go_partial_insertion_sort(Range& d, int a, int b) { return go_partial_insertion_sort_scans(d, a, b); }
static void go_insertion_sort(Range& d, int a, int b) { go_insertion_sort_scans(d, a, b); }

// the driver: the slice itself, with the hand-over of short ranges
struct Driver {
    Arr d;
    int cap;  // elements a range policy holds (the device: 64 lanes)
    int depth;
    static constexpr bool kRanges = true;
    static int uni(int v) { return v; }
    bool less(int i, int j) const { return (d.at(i).key & KEYMASK) < (d.at(j).key & KEYMASK); }
    void swap(int i, int j) {
        const Elem t = d.at(i);
        d.at(i) = d.at(j);
        d.at(j) = t;
    }
    bool hand_over(int a, int b, int limit, bool wb, bool wp, int* stk, int sp) {
        const int base = a > 0 ? a - 1 : 0;
        if (b - base > cap) return false;
        if (b - a < 2) return true;
        Range r;
        r.base = base;
        r.a = a;
        r.b = b;
        for (int p = base; p < b; p++) r.lane[p - base] = d.at(p);
        g_handovers++;
        if (sp > 0) g_nested++;
        pdqsort_from(r, stk, sp, a, b, limit, wb, wp);
        if (a > 0 && (r.lane[0].key != d.at(base).key || r.lane[0].ord != d.at(base).ord)) die("a-1 changed", a, b);
        for (int p = a; p < b; p++) d.at(p) = r.lane[p - base];
        return true;
    }
};
// the driver's choosePivot: the sampled-value network, as WaveLds's on the device
static void go_choose_pivot(const Driver& d, int a, int b, int& pivot, int& hint) {
    const int l = b - a;
    uint32_t v[9] = {};
    if (l >= 8)
        for (int q = 0; q < (l >= 50 ? 9 : 3); q++) v[q] = d.d.at(go_pivot_sample_pos(a, b, q)).key & KEYMASK;
    go_choose_pivot_vals(v, a, b, pivot, hint);
}

static const int STK = 64 * 5;  // FfdShared::sstack
static const int MAXN = 640;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

static long g_cases;
static Elem g_in[MAXN], g_w[MAXN], g_ref[MAXN];

// keys in g_in[0..n): all sorters from the entry (0, n, limit, true, true); limit < 0: bits.Len(n)
static void check(int n, int limit) {
    if (limit < 0) limit = go_bits_len((unsigned)n);
    g_cases++;
    int* stk = (int*)malloc(STK * sizeof(int));
    for (int i = 0; i < n; i++) g_in[i].ord = (uint32_t)i;
    // GoSlice
    for (int i = 0; i < n; i++) g_ref[i] = g_in[i];
    {
        Arr r{g_ref, n};
        auto less = [&](int i, int j) { return (r.at(i).key & KEYMASK) < (r.at(j).key & KEYMASK); };
        auto swap = [&](int i, int j) {
            const Elem t = r.at(i);
            r.at(i) = r.at(j);
            r.at(j) = t;
        };
        GoSlice<decltype(less), decltype(swap)> s{less, swap};
        s.pdq(0, n, limit);
    }
    for (int i = 1; i < n; i++)
        if ((g_ref[i].key & KEYMASK) < (g_ref[i - 1].key & KEYMASK)) die("GoSlice left the slice unsorted", n, i);
    // the plain sorter
    for (int i = 0; i < n; i++) g_w[i] = g_in[i];
    {
        Plain p{Arr{g_w, n}};
        pdqsort_from(p, stk, 0, 0, n, limit, true, true);
    }
    for (int i = 0; i < n; i++)
        if (g_w[i].ord != g_ref[i].ord || g_w[i].key != g_ref[i].key) die("plain pdqsort_full differs from GoSlice", n, i, limit);
    // the driver at each threshold
    for (int T : {63, 20, 13}) {
        for (int i = 0; i < n; i++) g_w[i] = g_in[i];
        Driver dr{Arr{g_w, n}, T + 1, 0};
        pdqsort_from(dr, stk, 0, 0, n, limit, true, true);
        for (int i = 0; i < n; i++)
            if (g_w[i].ord != g_ref[i].ord || g_w[i].key != g_ref[i].key) die("driver differs from GoSlice", n, i, T);
    }
    free(stk);
}

// sorted keys in runs of equal keys; run length rl (0: random 1..9)
static void runs(int n, int rl) {
    uint32_t k = 1;
    for (int i = 0; i < n;) {
        const int len = rl ? rl : 1 + (int)(rnd() % 9);
        for (int q = 0; q < len && i < n; q++, i++) g_in[i].key = k;
        k += 1 + (rl == 0 ? rnd() % 2 : 0);
    }
}

static void pivot_network() {
    long cases = 0;
    static Elem e[MAXN];
    const int AB[][2] = {{0, 8}, {0, 13}, {5, 54}, {0, 49}, {0, 50}, {3, 53}, {0, 64}, {17, 130}, {0, 449}, {101, 600}, {7, 12}};
    for (const auto& ab : AB) {
        const int a = ab[0], b = ab[1], l = b - a, ns = l >= 50 ? 9 : 3;
        int total = 1;
        for (int q = 0; q < ns; q++) total *= 3;
        for (int round = 0; round < total + 2000; round++) {
            for (int i = 0; i < b; i++) e[i].key = 1000 + rnd() % 5;  // the other positions take no part
            uint32_t v[9] = {};
            int code = round;
            for (int q = 0; q < ns; q++) {
                const uint32_t val = round < total ? (uint32_t)(code % 3) : rnd() % (round % 2 ? 4 : 1000);
                code /= 3;
                if (l >= 8) {
                    const int p = go_pivot_sample_pos(a, b, q);
                    if (p < a || p >= b) die("sample outside [a, b)", p, a, b);
                    e[p].key = val;
                    v[q] = val;
                }
            }
            Plain pl{Arr{e, b}};
            int p0, h0, p1, h1;
            go_choose_pivot(pl, a, b, p0, h0);
            go_choose_pivot_vals(v, a, b, p1, h1);
            if (p0 != p1 || h0 != h1) die("pivot network differs from go_choose_pivot", a, b, round);
            cases++;
        }
    }
    printf("pivot network: %ld cases\n", cases);
}

int main() {
    pivot_network();
    const int RL[5] = {1, 2, 7, 64, 0};
    for (int n = 13; n <= 600; n++)
        for (int rl : RL) {
            // kind 1: the element at pos gained a pod
            for (int pos = 0; pos < n; pos++) {
                runs(n, rl);
                g_in[pos].key += 1;
                if (pos % 5 == 0) g_in[(pos * 7) % n].key |= 0x80000000u;  // the memo bit takes no part
                check(n, -1);
            }
            // kind 2: an element with one pod was appended
            if (n < 600) {
                runs(n, rl);
                g_in[n].key = 1;
                check(n + 1, -1);
            }
        }
    const long structured = g_cases;
    for (int it = 0; it < 6000; it++) {
        const int n = 13 + (int)(rnd() % 588);
        const int kind = it % 6;
        const uint32_t alpha = (it / 6) % 3 == 0 ? 3 : (it / 6) % 3 == 1 ? 40 : 100000;
        for (int i = 0; i < n; i++) {
            switch (kind) {
            case 0:
            case 1: g_in[i].key = rnd() % alpha; break;
            case 2: g_in[i].key = (uint32_t)(n - i) / (alpha == 3 ? 5 : 1); break;          // reversed (with runs)
            case 3: g_in[i].key = 7; break;                                                   // all equal
            case 4: g_in[i].key = (uint32_t)(i < n / 2 ? i : n - i); break;                   // organ pipe
            default: g_in[i].key = (uint32_t)i + (rnd() % 16 == 0 ? rnd() % 50 : 0); break;   // nearly sorted
            }
        }
        check(n, -1);
        if (it % 3 == 0) check(n, it % 9 / 3);  // limit 0, 1, 2: heapSort on the slice or on sub-ranges
    }
    printf("ok: %ld structured + %ld random / adversarial inputs; %ld hand-overs (%ld below the root entry), %ld swaps in ranges\n",
           structured, g_cases - structured, g_handovers, g_nested, g_swaps_range);
    if (!g_nested || !g_swaps_range) die("no nested hand-over exercised");
    return 0;
}
