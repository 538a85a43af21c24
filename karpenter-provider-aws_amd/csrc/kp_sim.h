// kp_sim.h — operands of simulate_kernel (kp_simulate.hip), shared with the C-ABI host (kp_host.cpp).
//
// simulate_kernel is SimulateScheduling alone ([core] pkg/controllers/disruption/helpers.go, recalled): the probe of
// kp_cons.h without computeConsolidation, run to the end of its queue with up to KP_SIM_MAX_NODECLAIMS in-flight
// NodeClaims.  It reads the tables of a prepared consolidation pass (KpDev, KpCons) and writes only what is named here
// and the per-worker scratch the host hands it in its own KpCons copy (ring, ring_last, delta, pbits) and KpDev copy
// (the nc_* slabs, [KP_SIM_MAX_NODECLAIMS][workers] entries in the Solve's layout, which finalize_kernel then reads).
#pragma once
#include <stdint.h>

#include "../../include/kpsim.h"
#include "kp_layout.h"

enum { SS_POPS = 0, SS_NC_EVALS, SS_TMPL_EVALS, SS_PROBES, SS_COUNT };

// Device row of one probe, before TruncateInstanceTypes (the host folds finalize_kernel's nc_valid into kp_sim_result).
struct KpSimRow {
    int32_t status;   // KP_SIM_*
    int32_t bad;      // a non-pending pod landed on an uninitialized node
    int32_t n_nc;     // NodeClaims created
    int32_t n_pods;   // pods in the probe's queue
    int32_t n_np;     // non-pending pods among them
    int32_t ok_np;    // non-pending pods with a place (existing node or NodeClaim)
};

struct KpSim {
    KpSimRow* rows;        // [n_probes of the batch]
    int32_t* nc_nonpend;   // [KP_SIM_MAX_NODECLAIMS][workers] non-pending pods of each NodeClaim
    int32_t* log;          // [workers][ring_cap][2] placements in order (Results pod_order): pod, pod_result
    int32_t* n_log;        // [workers]
    int64_t* stats;        // [SS_COUNT]
    int32_t* err;          // [1] 2: a probe exceeded its pop bound
    // a MUT probe's copies of the nodes whose requirements it changed (as KpCons::ov_*): slot of node j (valid while the
    // probe's LDS bit for j is set), the copies' digests; ov_cap >= the pods of any probe
    int32_t* ov_slot;      // [workers][E]
    ReqHdr* ov_hdr;        // [workers][ov_cap][K]
    uint64_t* ov_words;    // [workers][ov_cap][DW]
    int32_t ov_cap;
    // dynamic LDS plan (kp_sim_plan_lds)
    int32_t off_hdr, off_words, off_rem, off_excl, off_mod, off_mutn;
    int32_t lds_bytes;
    // simulate_topo_kernel (a pass with topology groups, kp_device_opts::simulate_topology): each worker's ProbeTopo
    // (kp_eval.h), as consolidate_body's but with a hostname column per NodeClaim id.  The prepared pass's own pt_*
    // buffers are not used; its base counts, decrements and hostname-affinity tables are read through KpDev / KpCons.
    int32_t* pt_cnt;       // [workers][G][64]
    uint64_t* pt_known;    // [workers][G]
    int32_t* pt_hd;        // [workers][HG][E + KP_SIM_MAX_NODECLAIMS]
    int32_t off_touch, off_hmod, off_hpos, off_born;  // LDS: touched rows [ceil(G / 64)], node columns [EW], hpos [n_ha], born
};
