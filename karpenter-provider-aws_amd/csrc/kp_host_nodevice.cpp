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
#endif
