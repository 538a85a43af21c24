// kp_gosort_core.h — Go 1.24's pdqsort_func (src/sort/zsortfunc.go), operation for operation, over a data policy D.
// Plain C++ on both sides: kp_gosort.h supplies the device policies (RegSlice: one element per lane; WaveLds: the
// slice in LDS), tests/cpu_stub/test_gosort_ranges.cpp a bounds-checking host array.  kp_gosort_host.h is not built on
// this header: it stays the independent restatement the CPU test compares against.
//
// A policy provides
//   bool less(int i, int j) const;  void swap(int i, int j);          index-based, as sort.Slice's callbacks
//   static int uni(int v);                                            a wave-uniform copy of v (host: v itself)
//   static constexpr bool kRanges;                                    whether popped ranges are offered to hand_over
//   bool hand_over(int a, int b, int limit, bool wb, bool wp, int* stk, int sp);   (kRanges only)
//
// Short ranges (KP_SORT_REG_RANGES).  pdqsort's sub-ranges are disjoint: once [a, b) is popped with its state (limit,
// wasBalanced, wasPartitioned), everything Go does before the next older stack entry is popped — the range's own loop and
// all the entries it pushes, which are popped first (LIFO) — swaps only positions in [a, b) and reads, besides them, only
// data[a-1] (the `a > 0 && !less(data[a-1], data[pivot])` test).  data[a-1] is an ancestor's pivot, or the last element
// partitionEqual set aside: it is final, it is <= every element of [a, b), and nothing writes it again; for the same
// reason partialInsertionSort's `k >= 1` loop, which Go does not bound by a, stops at k = a (less(data[a], data[a-1]) is
// false).  So a policy may take the popped entry, copy [a-1, b) somewhere faster, run pdqsort_from on the copy from
// that same entry with the stack continuing at the same depth, and copy [a, b) back: the comparisons, their outcomes
// and the swaps are those of the plain sorter, in the same order, hence the same permutation.  hand_over returns true
// when it did so.  The CPU test checks the claim (no index outside [a-1, b), no write to a-1) and the permutation
// against the plain sorter and kp_gosort_host.h.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KP_SORT_HD __device__ inline
#else
#define KP_SORT_HD inline
#endif

KP_SORT_HD int go_bits_len(unsigned x) { return x ? 32 - __builtin_clz(x) : 0; }

// order2_func / median_func / medianAdjacent_func / choosePivot_func (one lane)
template <class D>
KP_SORT_HD void go_order2(const D& d, int a, int b, int& swaps, int& x, int& y) {
    if (d.less(b, a)) {
        swaps++;
        x = b;
        y = a;
    } else {
        x = a;
        y = b;
    }
}
template <class D>
KP_SORT_HD int go_median(const D& d, int a, int b, int c, int& swaps) {
    int x, y;
    go_order2(d, a, b, swaps, x, y);
    a = x;
    b = y;
    go_order2(d, b, c, swaps, x, y);
    b = x;
    c = y;
    go_order2(d, a, b, swaps, x, y);
    return y;
}
// hint: 0 unknown, 1 increasing, 2 decreasing
template <class D>
KP_SORT_HD void go_choose_pivot(const D& d, int a, int b, int& pivot, int& hint) {
    const int l = b - a;
    int swaps = 0;
    int i = a + l / 4 * 1, j = a + l / 4 * 2, k = a + l / 4 * 3;
    if (l >= 8) {
        if (l >= 50) {
            i = go_median(d, i - 1, i, i + 1, swaps);
            j = go_median(d, j - 1, j, j + 1, swaps);
            k = go_median(d, k - 1, k, k + 1, swaps);
        }
        j = go_median(d, i, j, k, swaps);
    }
    pivot = j;
    hint = swaps == 0 ? 1 : (swaps == 12 ? 2 : 0);
}

// choosePivot_func of [a, b) on sampled values (KP_SORT_PIVOT_LANES): v[3g + q] = key of position a + l/4·(g+1) - 1 + q
// for l >= 50, v[g] = key of a + l/4·(g+1) for 8 <= l < 50 (unused below 8).  The order2 / median network runs on
// (value, index) pairs: each step makes the strict `less` decision go_choose_pivot makes on the same two positions, so
// the swap count and the index that comes out are the same.
struct GoPivotVI {
    uint32_t v;
    int i;
};
KP_SORT_HD GoPivotVI go_median_vi(GoPivotVI a, GoPivotVI b, GoPivotVI c, int& swaps) {
    GoPivotVI t;
    if (b.v < a.v) { swaps++; t = a; a = b; b = t; }
    if (c.v < b.v) { swaps++; t = b; b = c; c = t; }
    if (b.v < a.v) { swaps++; t = a; a = b; b = t; }
    return b;
}
KP_SORT_HD void go_choose_pivot_vals(const uint32_t* v, int a, int b, int& pivot, int& hint) {
    const int l = b - a;
    int swaps = 0;
    const int i = a + l / 4 * 1, j = a + l / 4 * 2, k = a + l / 4 * 3;
    pivot = j;
    if (l >= 8) {
        GoPivotVI mi, mj, mk;
        if (l >= 50) {
            mi = go_median_vi({v[0], i - 1}, {v[1], i}, {v[2], i + 1}, swaps);
            mj = go_median_vi({v[3], j - 1}, {v[4], j}, {v[5], j + 1}, swaps);
            mk = go_median_vi({v[6], k - 1}, {v[7], k}, {v[8], k + 1}, swaps);
        } else {
            mi = {v[0], i};
            mj = {v[1], j};
            mk = {v[2], k};
        }
        pivot = go_median_vi(mi, mj, mk, swaps).i;
    }
    hint = swaps == 0 ? 1 : (swaps == 12 ? 2 : 0);
}
// position of sample q (see go_choose_pivot_vals) of [a, b)
KP_SORT_HD int go_pivot_sample_pos(int a, int b, int q) {
    const int l = b - a;
    return l >= 50 ? a + l / 4 * (q / 3 + 1) - 1 + q % 3 : a + l / 4 * (q + 1);
}

template <class D>
KP_SORT_HD void go_insertion_sort(D& d, int a, int b) {
    for (int i = a + 1; i < b; i++)
        for (int j = i; j > a && d.less(j, j - 1); j--) d.swap(j, j - 1);
}
template <class D>
KP_SORT_HD void go_sift_down(D& d, int lo, int hi, int first) {
    int root = lo;
    for (;;) {
        int child = 2 * root + 1;
        if (child >= hi) return;
        if (child + 1 < hi && d.less(first + child, first + child + 1)) child++;
        if (!d.less(first + root, first + child)) return;
        d.swap(first + root, first + child);
        root = child;
    }
}
template <class D>
KP_SORT_HD void go_heap_sort(D& d, int a, int b) {
    const int first = a, lo = 0, hi = b - a;
    for (int i = (hi - 1) / 2; i >= 0; i--) go_sift_down(d, i, hi, first);
    for (int i = hi - 1; i >= 0; i--) {
        d.swap(first, first + i);
        go_sift_down(d, lo, i, first);
    }
}
template <class D>
KP_SORT_HD int go_partition(D& d, int a, int b, int pivot, bool& already) {
    d.swap(a, pivot);
    int i = a + 1, j = b - 1;
    while (i <= j && d.less(i, a)) i++;
    while (i <= j && !d.less(j, a)) j--;
    if (i > j) {
        d.swap(j, a);
        already = true;
        return j;
    }
    d.swap(i, j);
    i++;
    j--;
    for (;;) {
        while (i <= j && d.less(i, a)) i++;
        while (i <= j && !d.less(j, a)) j--;
        if (i > j) break;
        d.swap(i, j);
        i++;
        j--;
    }
    d.swap(j, a);
    already = false;
    return j;
}
template <class D>
KP_SORT_HD int go_partition_equal(D& d, int a, int b, int pivot) {
    d.swap(a, pivot);
    int i = a + 1, j = b - 1;
    for (;;) {
        while (i <= j && !d.less(a, i)) i++;
        while (i <= j && d.less(a, j)) j--;
        if (i > j) break;
        d.swap(i, j);
        i++;
        j--;
    }
    return i;
}
template <class D>
KP_SORT_HD bool go_partial_insertion_sort(D& d, int a, int b) {
    int i = a + 1;
    for (int j = 0; j < 5; j++) {
        while (i < b && !d.less(i, i - 1)) i++;
        if (i == b) return true;
        if (b - a < 50) return false;
        d.swap(i, i - 1);
        if (i - a >= 2) {
            for (int k = i - 1; k >= 1; k--) {  // Go bounds this loop by 1, not a
                if (!d.less(k, k - 1)) break;
                d.swap(k, k - 1);
            }
        }
        if (b - i >= 2) {
            for (int k = i + 1; k < b; k++) {
                if (!d.less(k, k - 1)) break;
                d.swap(k, k - 1);
            }
        }
    }
    return false;
}
template <class D>
KP_SORT_HD void go_break_patterns(D& d, int a, int b) {
    const int length = b - a;
    if (length >= 8) {
        uint64_t random = (uint64_t)length;  // xorshift(length)
        const uint64_t modulus = 1ull << go_bits_len((unsigned)length);
        const int idx = a + (length / 4) * 2 - 1;
        for (int i = 0; i < 3; i++) {
            random ^= random << 13;
            random ^= random >> 7;
            random ^= random << 17;
            int other = (int)(random & (modulus - 1));
            if (other >= length) other -= length;
            d.swap(idx - 1 + i, a + other);
        }
    }
}
template <class D>
KP_SORT_HD void go_reverse_range(D& d, int a, int b) {
    int i = a, j = b - 1;
    while (i < j) {
        d.swap(i, j);
        i++;
        j--;
    }
}

// ---- the same functions over a policy with scans ----
// A scan policy adds  uint32_t key_at(int i) (the compared key of position i),
//   int find_first(int lo, int hi, F pred)   first q in [lo, hi] with pred(key_at(q)), hi + 1 if none
//   int find_last(int lo, int hi, F pred)    last q in [lo, hi] with pred(key_at(q)), lo - 1 if none
//   int first_descent(int i, int b)          first q in [i, b) with key_at(q) < key_at(q-1), b if none
// which a wave answers with one ballot per 64 positions.  Go's scan loops compare and do not swap, so replacing a loop by
// the position it stops at leaves the comparison outcomes that matter and the swap sequence what they were.
template <class D>
KP_SORT_HD int go_partition_scans(D& d, int a, int b, int pivot, bool& already) {
    d.swap(a, pivot);
    const uint32_t pk = d.key_at(a);
    int i = a + 1, j = b - 1;
    i = d.find_first(i, j, [&](uint32_t x) { return !(x < pk); });  // while i <= j && less(data[i], data[a]) i++
    j = d.find_last(i, j, [&](uint32_t x) { return x < pk; });      // while i <= j && !less(data[j], data[a]) j--
    if (i > j) {
        d.swap(j, a);
        already = true;
        return j;
    }
    d.swap(i, j);
    i++;
    j--;
    for (;;) {
        i = d.find_first(i, j, [&](uint32_t x) { return !(x < pk); });
        j = d.find_last(i, j, [&](uint32_t x) { return x < pk; });
        if (i > j) break;
        d.swap(i, j);
        i++;
        j--;
    }
    d.swap(j, a);
    already = false;
    return j;
}
template <class D>
KP_SORT_HD int go_partition_equal_scans(D& d, int a, int b, int pivot) {
    d.swap(a, pivot);
    const uint32_t pk = d.key_at(a);
    int i = a + 1, j = b - 1;
    for (;;) {
        i = d.find_first(i, j, [&](uint32_t x) { return pk < x; });    // while i <= j && !less(data[a], data[i]) i++
        j = d.find_last(i, j, [&](uint32_t x) { return !(pk < x); });  // while i <= j && less(data[a], data[j]) j--
        if (i > j) break;
        d.swap(i, j);
        i++;
        j--;
    }
    return i;
}
// partialInsertionSort_func: the search for the next descent is a scan, the two shift loops stay Go's
template <class D>
KP_SORT_HD bool go_partial_insertion_sort_scans(D& d, int a, int b) {
    int i = a + 1;
    for (int j = 0; j < 5; j++) {
        i = d.first_descent(i, b);  // while i < b && !less(data[i], data[i-1]) i++
        if (i == b) return true;
        if (b - a < 50) return false;
        d.swap(i, i - 1);
        if (i - a >= 2) {
            for (int k = i - 1; k >= 1; k--) {
                if (!d.less(k, k - 1)) break;
                d.swap(k, k - 1);
            }
        }
        if (b - i >= 2) {
            for (int k = i + 1; k < b; k++) {
                if (!d.less(k, k - 1)) break;
                d.swap(k, k - 1);
            }
        }
    }
    return false;
}
// insertionSort_func: the outer iterations before the first descent find data[i-1] <= data[i] and swap nothing
template <class D>
KP_SORT_HD void go_insertion_sort_scans(D& d, int a, int b) {
    for (int i = d.first_descent(a + 1, b); i < b; i++)
        for (int j = i; j > a && d.less(j, j - 1); j--) d.swap(j, j - 1);
}

// pdqsort_func(data, a, b, limit) entered with the loop state (wasBalanced, wasPartitioned), Go's recursion order
// (smaller side first) on an explicit stack: entries below sp0 belong to the caller and are left alone.
template <class D>
KP_SORT_HD void pdqsort_from(D& d, int* stk, int sp0, int a0, int b0, int limit0, bool wb0, bool wp0) {
    int sp = sp0;
    auto push = [&](int a, int b, int limit, int wb, int wp) {
        stk[sp * 5 + 0] = a;
        stk[sp * 5 + 1] = b;
        stk[sp * 5 + 2] = limit;
        stk[sp * 5 + 3] = wb;
        stk[sp * 5 + 4] = wp;
        sp++;
    };
    push(a0, b0, limit0, wb0, wp0);
    while (sp > sp0) {
        sp--;
        int a = D::uni(stk[sp * 5 + 0]), b = D::uni(stk[sp * 5 + 1]);
        int limit = D::uni(stk[sp * 5 + 2]);
        bool wasBalanced = D::uni(stk[sp * 5 + 3]) != 0;
        bool wasPartitioned = D::uni(stk[sp * 5 + 4]) != 0;
        if constexpr (D::kRanges) {
            if (d.hand_over(a, b, limit, wasBalanced, wasPartitioned, stk, sp)) continue;
        }
        for (;;) {
            const int length = b - a;
            if (length <= 12) {
                go_insertion_sort(d, a, b);
                break;
            }
            if (limit == 0) {
                go_heap_sort(d, a, b);
                break;
            }
            if (!wasBalanced) {
                go_break_patterns(d, a, b);
                limit--;
            }
            int pivot, hint;
            go_choose_pivot(d, a, b, pivot, hint);
            if (hint == 2) {
                go_reverse_range(d, a, b);
                pivot = (b - 1) - (pivot - a);
                hint = 1;
            }
            if (wasBalanced && wasPartitioned && hint == 1) {
                if (go_partial_insertion_sort(d, a, b)) break;
            }
            if (a > 0 && !d.less(a - 1, pivot)) {
                a = go_partition_equal(d, a, b, pivot);
                continue;
            }
            bool already = false;
            const int mid = go_partition(d, a, b, pivot, already);
            wasPartitioned = already;
            const int leftLen = mid - a, rightLen = b - mid;
            const int balanceThreshold = length / 8;
            if (leftLen < rightLen) {
                wasBalanced = leftLen >= balanceThreshold;
                push(mid + 1, b, limit, wasBalanced, wasPartitioned);  // the loop continues here afterwards
                push(a, mid, limit, 1, 1);                             // recursive pdqsort_func first
            } else {
                wasBalanced = rightLen >= balanceThreshold;
                push(a, mid, limit, wasBalanced, wasPartitioned);
                push(mid + 1, b, limit, 1, 1);
            }
            break;
        }
    }
}
// pdqsort_func(data, 0, n, bits.Len(n))
template <class D>
KP_SORT_HD void pdqsort_full(D& d, int n, int* stk) {
    pdqsort_from(d, stk, 0, 0, n, go_bits_len((unsigned)n), true, true);
}
