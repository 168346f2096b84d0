// dn_hop_glw.hip -- the wavefront-per-stream instantiations of hop_kernel (n_fft 1024: deep pipes, the saturated regime, the front-only launch of a
// split hop) as a translation unit of their own, compiled with LLVM's iterative-ILP scheduling strategy (dn_hop_kernels.hpp, Makefile).  The stamped
// diagnostic build keeps them in dn_hop.hip: this file is empty there.
#ifndef DN_PROBE
#include "dn_hop_kernels.hpp"

namespace dn {

void launch_hop_glw(const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st) { launch_hop_of<1024, true>(d, c, a, bf16, st); }

}  // namespace dn
#endif
