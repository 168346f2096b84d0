// dn_api.hip -- the C ABI of include/dn_denoise.h, its part that belongs to no handle: the per-thread error string, the ABI version and the
// helpers the other host units share (dn_host.hpp).  The handles: dn_api_model.hip, dn_api_dsp.hip, dn_api_pipe.hip, dn_api_sessions.hip.
// No kernel code in any of them.
#include "dn_host.hpp"

static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int launch_failed(const char* what, hipError_t e) { return fail(DN_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e)); }

int bad_momentum() { return fail(DN_ERR_INVALID, "momentum must be in [0, 1)"); }

int check_hop_args(const char* who, const dn_model* m, const dn_dsp* d, int32_t B, int32_t n_iter, float momentum, uint32_t flags, float* mom) {
    if (!m || !d) return fail(DN_ERR_INVALID, std::string(who) + ": null handle");
    if (d->cfg.n_mels <= 0 || d->cfg.n_mels % 16) return fail(DN_ERR_INVALID, "n_mels must be a positive multiple of 16");
    if (B < 0 || n_iter < 0) return fail(DN_ERR_INVALID, std::string(who) + ": negative size");
    DN_TRY(check_momentum(momentum, mom));
    if (d->cfg.n_mels / 16 > dn::kMaxC) return fail(DN_ERR_UNSUPPORTED, "n_mels/16 exceeds the cell kernel's limit");
    if (flags & ~kHopFlags) return fail(DN_ERR_INVALID, std::string(who) + ": unknown flag bits");
    return DN_OK;
}

int refuse_not_1024(const std::string& what) {
    return fail(DN_ERR_UNSUPPORTED, what + " for n_fft 1024 (at 1536 the per-lane state of a stream does not fit a wavefront's registers; at 512 the schedule is not built)");
}

size_t phasor_bytes(const dn_dsp* d, size_t frames) {
    return (frames * 3 * ((size_t)d->cfg.n_fft / 2 + 1) * sizeof(float2) + 255) & ~size_t(255);
}

extern "C" {

const char* dn_last_error(void) { return g_err.c_str(); }
int dn_abi_version(void) { return DN_ABI_VERSION; }

}  // extern "C"
