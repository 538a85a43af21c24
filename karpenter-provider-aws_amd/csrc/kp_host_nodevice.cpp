// kp_host_nodevice.cpp — the host layer built WITHOUT a device compiler (g++ over a CPU stand-in of the HIP runtime:
// tests/cpu_stub, whose Makefile takes every csrc/kp_host*.cpp): the launchers of kernel units younger than that
// stand-in.  Under hipcc this unit is empty and the launchers are the kernel units' own, so libkpsim.so never holds a
// stand-in: there a missing kernel stays a link error.
#ifndef __HIPCC__
#include "kp_host.h"

// kp_explain.hip's launcher: nothing is evaluated, every row says that no reason is known (KPX_UNKNOWN).
hipError_t kp_launch_explain(const KpDev& d, const KpExplain& x, hipStream_t) {
    for (int i = 0; i < x.n_shapes * d.NT; i++) x.rows[i] = KpExplainRow{};
    return hipSuccess;
}

// kp_consolidate.hip's explain launcher: the probes run as the stand-in of kp_launch_consolidate runs them, and every row
// says that the probe has a command (KP_UNCONS_NONE); no pod is recorded.
hipError_t kp_launch_consolidate_explain(const KpDev& d, const KpCons& k, const KpConsExplain& x, int n_workers,
                                         hipStream_t s, KpDev* d_dev, KpCons* d_k) {
    const hipError_t e = kp_launch_consolidate(d, k, n_workers, s, d_dev, d_k);
    for (int i = 0; i < k.n_probes; i++) {
        kp_probe_explanation r{};
        r.first_unscheduled = -1;
        r.candidate_price = k.out[i].candidate_price;
        x.rows[i] = r;
    }
    if (x.n_rec) x.n_rec[0] = 0;
    return e;
}

// kp_simulate.hip's launchers: nothing is simulated, every probe reports an empty queue with everything scheduled and no
// NodeClaim, except that in a pass with host ports or volume limits its MUT probes count as the probes the kernel does
// not cover (the host layer's batching, row folding and decoding still run end to end).
bool kp_sim_plan_lds(const KpDev&, KpSim& x, int, int, int) {
    x.lds_bytes = 1024;
    return true;
}
hipError_t kp_launch_simulate(const KpCons& k, const KpSim& x, hipStream_t, const KpDev* d_dev, const KpCons*,
                              const KpSim*) {
    for (int i = 0; i < k.n_probes; i++) {
        x.rows[i] = KpSimRow{};
        const int gp = k.probe0 + i;
        if (k.mut && (d_dev->PW > 0 || d_dev->VD > 0) && (k.mode == KP_CONSOLIDATE_SINGLE ? k.mut_s[gp] : k.mut_m[gp]) != 0)
            x.rows[i].status = KP_SIM_UNSUPPORTED_PROBE;
        x.n_log[i] = 0;
        for (int q = 0; q < KP_SIM_MAX_NODECLAIMS; q++) {
            const size_t e = (size_t)q * k.n_probes + i;
            x.nc_nonpend[e] = 0;
            d_dev->nc_tmpl[e] = 0;
            d_dev->nc_npods[e] = 0;
            d_dev->nc_slice_pos[e] = -1;
        }
    }
    x.stats[SS_PROBES] += k.n_probes;
    return hipSuccess;
}
#endif
