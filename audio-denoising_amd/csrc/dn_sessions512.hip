// n_fft 512 one-launch form of the session pool under the default scheduling strategy (Makefile; see dn_sessions.hip)
#define DN_SESS_TU_512 1
#include "dn_sessions.hip"
