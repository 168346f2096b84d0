// the two-launch form of the session pool under iterative-ILP scheduling, as the wavefront-per-stream hop kernels (Makefile; see dn_sessions.hip)
#define DN_SESS_TU_GLW 1
#include "dn_sessions.hip"
