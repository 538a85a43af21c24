// TEST INFRASTRUCTURE: the headroom bound's row entry and reject test (karpenter-provider-aws_amd/csrc/kp_bound.h)
// against NodeClaim.Add's Fits rule, exhaustively over small ranges: allocatable 0..40 per option, two to four options,
// request totals and pod requests 0..44.  For every combination: the test never rejects when some option fits the total
// plus the pod, and rejects whenever the pod is positive and no option does (the row is unscaled, so it is exact: in
// particular it rejects a request two quanta or more above the true bound for every quick-accept scale 0..3).  A row
// entry without a witness never rejects.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../karpenter-provider-aws_amd/csrc/kp_bound.h"

// resources.Fits on one axis as the evaluation applies it: an axis with a total <= 0 is not compared
static bool fits(int64_t total, int64_t alloc) { return !(total > 0) || total <= alloc; }

int main() {
    long long checked = 0;
    int64_t a[4];
    for (int n = 2; n <= 4; n++)
        for (a[0] = 0; a[0] <= 40; a[0] += (n == 4 ? 5 : 1))
            for (a[1] = 0; a[1] <= 40; a[1] += (n >= 3 ? 4 : 1))
                for (a[2] = 0; a[2] <= (n >= 3 ? 40 : 0); a[2] += 3)
                    for (a[3] = 0; a[3] <= (n >= 4 ? 40 : 0); a[3] += 7) {
                        const int64_t mx = *std::max_element(a, a + n);
                        const int64_t row = kp_bound_entry(mx, true);
                        for (int64_t tot = 0; tot <= 44; tot++)
                            for (int64_t p = 0; p <= 44; p++) {
                                bool some = false;
                                for (int i = 0; i < n; i++) some |= fits(tot + p, a[i]);
                                const bool rej = kp_bound_rejects(row, tot, p);
                                if (rej && some) return printf("rejects a fitting pod: max %lld tot %lld p %lld\n", (long long)mx, (long long)tot, (long long)p), 1;
                                if (p > 0 && !some && !rej) return printf("misses: max %lld tot %lld p %lld\n", (long long)mx, (long long)tot, (long long)p), 1;
                                for (int q = 0; q <= 3; q++)  // two quanta above the true bound, at every scale
                                    if (p > 0 && tot + p >= mx + 2 * (1ll << q) && !rej) return printf("loose at scale %d\n", q), 1;
                                if (kp_bound_rejects(kp_bound_entry(mx, false), tot, p)) return printf("no-bound entry rejects\n"), 1;
                                checked++;
                            }
                    }
    printf("ok: %lld combinations\n", checked);
    return 0;
}
