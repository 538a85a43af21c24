// kp_ffd_prof_ports.hip — the diagnostic twins (ffd_solve PROF) of the entry points of kp_ffd_ports.hip, named <entry>_prof.
#define KP_FFD_PROF 1
#include "kp_ffd_ports.hip"
