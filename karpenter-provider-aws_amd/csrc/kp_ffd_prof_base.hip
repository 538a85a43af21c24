// kp_ffd_prof_base.hip — the diagnostic twins (ffd_solve PROF: stage stamps, n_* counters, trace records) of the entry
// points of kp_ffd_base.hip, named <entry>_prof; kp_launch_ffd launches them under KPSIM_PROFILE / KPSIM_TRACE_POD.
#define KP_FFD_PROF 1
#include "kp_ffd_base.hip"
