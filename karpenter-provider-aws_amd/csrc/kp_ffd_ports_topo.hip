// kp_ffd_ports_topo.hip — Solve kernel entry points for solves with node-side state: host ports, volume limits (ffd_solve PORTS, preference code on): topology groups, no reserved offerings,
// with the slice arrays in LDS or HBM.  Built with KP_NWAVES_TOPO waves like the other topology units (kp_ffd_base_topo.hip).
#ifndef KP_NWAVES_TOPO
#define KP_NWAVES_TOPO 4  // kp_layout.h
#endif
#define KP_NWAVES KP_NWAVES_TOPO
#include "kp_ffd.h"

KP_FFD_ENTRY_PORTS(ffd_ports_topo_kernel, false, true, false)
KP_FFD_ENTRY_PORTS(ffd_ports_topo_hbm_kernel, false, true, true)
