// kp_ffd_ports.hip — Solve kernel entry points for solves with node-side state: host ports, volume limits (ffd_solve PORTS, preference code on): no reserved offerings, no topology groups,
// with the slice arrays in LDS or HBM.
#include "kp_ffd.h"

KP_FFD_ENTRY_PORTS(ffd_ports_kernel, false, false, false)
KP_FFD_ENTRY_PORTS(ffd_ports_hbm_kernel, false, false, true)
