// kp_host.h — internal header of the C-ABI host (kp_host.cpp; not installed): the prototypes of the kernel units' launchers,
// stated once.  tests/cpu_stub/hip_stub.cpp includes it: a stand-in that drifts in its return type no longer compiles.
#pragma once
#include <hip/hip_runtime.h>

#include "kp_cons.h"
#include "kp_explain.h"
#include "kp_launch.h"
#include "kp_layout.h"
#include "kp_sim.h"

size_t kp_ffd_shared_bytes();
size_t kp_ffd_shared_bytes_topo();
bool kp_ffd_plan_lds(KpDev& d, int max_bytes);
hipError_t kp_launch_class_mask(const KpDev& d, hipStream_t s);
hipError_t kp_launch_template_init(const KpDev& d, hipStream_t s);
hipError_t kp_launch_existing(const KpDev& d, hipStream_t s);
hipError_t kp_launch_ffd(const KpDev& d, hipStream_t s);
hipError_t kp_launch_explain(const KpDev& d, const KpExplain& x, hipStream_t s);
hipError_t kp_ffd_set_attributes();
hipError_t kp_cons_set_attributes();
hipError_t kp_launch_finalize(const KpDev& d, int n_nodeclaims, hipStream_t s);
bool kp_cons_plan_lds(const KpDev& d, KpCons& k, int max_bytes);
hipError_t kp_launch_select_kernel(const KpLaunch& g, hipStream_t s);
hipError_t kp_launch_consolidate(const KpDev& d, const KpCons& k, int n_workers, hipStream_t s, KpDev* d_dev,
                                 KpCons* d_k);
hipError_t kp_launch_consolidate_explain(const KpDev& d, const KpCons& k, const KpConsExplain& x, int n_workers,
                                         hipStream_t s, KpDev* d_dev, KpCons* d_k);
hipError_t kp_launch_cons_chunk_max(const KpDev& d, int64_t* cmax0, hipStream_t s);
hipError_t kp_launch_multi_union(const KpCons& k, int nu, uint64_t* ubits, int32_t* rcand, int2* ulist, int32_t* ulen,
                                 const int32_t* queue0, hipStream_t s);
hipError_t kp_launch_cons_prep(const int32_t* queue0, int P, int32_t* rank, const int32_t* pending, int n_pending,
                               uint64_t* pend_bits, hipStream_t s);
hipError_t kp_queue_sort(const int64_t* fields, int n, int32_t* perm_a, int32_t* perm_b, uint64_t* keys_a,
                         uint64_t* keys_b, void* temp, size_t* temp_bytes, hipStream_t s, int32_t** result);
bool kp_sim_plan_lds(const KpDev& d, KpSim& x, int max_bytes, int G = 0, int n_ha = 0);
hipError_t kp_launch_simulate(const KpCons& k, const KpSim& x, hipStream_t s, const KpDev* d_dev, const KpCons* d_k,
                              const KpSim* d_x);
