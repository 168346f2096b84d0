// n_fft 1536 one-launch form of the session pool under the default scheduling strategy (Makefile; see dn_sessions.hip)
#define DN_SESS_TU_1536 1
#include "dn_sessions.hip"
