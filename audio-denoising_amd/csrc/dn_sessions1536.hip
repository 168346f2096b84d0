// n_fft 1536 one-launch form of the session pool under the default scheduling strategy (Makefile; see dn_sess_kernels.hpp)
#include "dn_sess_kernels.hpp"

namespace dn {

void launch_sess_frame_unit(Size<1536>, const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in) {
    launch_sess_frame_of<1536>(d, c, a, bf16, st, phase_in);
}

}  // namespace dn
