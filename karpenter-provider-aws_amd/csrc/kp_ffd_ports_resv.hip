// kp_ffd_ports_resv.hip — Solve kernel entry points for solves with node-side state: host ports, volume limits (ffd_solve PORTS, preference code on): reserved offerings, no topology groups,
// with the slice arrays in LDS or HBM.
#include "kp_ffd.h"

KP_FFD_ENTRY_PORTS(ffd_ports_resv_kernel, true, false, false)
KP_FFD_ENTRY_PORTS(ffd_ports_resv_hbm_kernel, true, false, true)
