// dn_hop1536.hip -- the n_fft-1536 instantiations of hop_kernel and frame_kernel as a translation unit of their own, compiled with the default
// scheduling strategy (dn_hop_kernels.hpp, Makefile).  The stamped diagnostic build keeps them in dn_hop.hip: this file is empty there.
#ifndef DN_PROBE
#include "dn_hop_kernels.hpp"

namespace dn {

void launch_hop_unit(Size<1536>, const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st) { launch_hop_of<1536, false>(d, c, a, bf16, st); }
void launch_frame_unit(Size<1536>, const DspDev& d, const CellDev& c, const FrameArgs& a, int B, bool bf16, hipStream_t st) { launch_frame_of<1536>(d, c, a, B, bf16, st); }

}  // namespace dn
#endif
