// the wavefront-per-frame chains of clip mode under iterative-ILP scheduling, as the other kernels built on glw_body (Makefile; see dn_clip.hip)
#define DN_CLIP_TU_GLW 1
#include "dn_clip.hip"
