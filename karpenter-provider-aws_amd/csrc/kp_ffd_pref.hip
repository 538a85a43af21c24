// kp_ffd_pref.hip — Solve kernel entry points: preference relaxation / MIN_VALUES_POLICY=BestEffort (each with and without topology groups, and
// with the slice arrays in LDS or HBM).  ffd_solve is in kp_ffd.h; the launcher is kp_launch_ffd (kp_kernels.hip).
#include "kp_ffd.h"

KP_FFD_ENTRY(ffd_pref_kernel, false, false, true, false)
KP_FFD_ENTRY(ffd_pref_hbm_kernel, false, false, true, true)
