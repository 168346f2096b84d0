// dn_api_dsp.hip -- dn_dsp: the plan's tables (pure host functions, then one arena), the stateless DSP and server entry points, and the
// one-launch hop (dn_process_frame, dn_stream_step, clip mode).  No kernel code here.
#include <math.h>
#include <stdlib.h>

#include "dn_host.hpp"

namespace {

const double PI = 3.14159265358979323846;

// Cholesky solve of the SPD system G X = R in double; G is n x n (row-major), R is n x m. In place.
bool chol_solve(std::vector<double>& G, std::vector<double>& R, int n, int m) {
    for (int j = 0; j < n; ++j) {
        double d = G[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= G[(size_t)j * n + k] * G[(size_t)j * n + k];
        if (!(d > 0.0)) return false;
        d = sqrt(d);
        G[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; ++i) {
            double s = G[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= G[(size_t)i * n + k] * G[(size_t)j * n + k];
            G[(size_t)i * n + j] = s / d;
        }
    }
    for (int c = 0; c < m; ++c) {
        for (int i = 0; i < n; ++i) {           // L y = r
            double s = R[(size_t)i * m + c];
            for (int k = 0; k < i; ++k) s -= G[(size_t)i * n + k] * R[(size_t)k * m + c];
            R[(size_t)i * m + c] = s / G[(size_t)i * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {      // L^T x = y
            double s = R[(size_t)i * m + c];
            for (int k = i + 1; k < n; ++k) s -= G[(size_t)k * n + i] * R[(size_t)k * m + c];
            R[(size_t)i * m + c] = s / G[(size_t)i * n + i];
        }
    }
    return true;
}

// ---- the tables of a plan.  Several are bit-matched to what the kernels form per lane: every fp32 operation below is where it has to be.
// window (the caller's, or torch.hann_window periodic) and the reciprocal of its istft envelope; false: the envelope is ~0 somewhere
bool window_tables(int N, const float* window_in, std::vector<float>& window, std::vector<float>& inv_env) {
    window.resize(N);
    for (int n = 0; n < N; ++n) window[n] = window_in ? window_in[n] : (float)(0.5 - 0.5 * cos(2.0 * PI * n / N));
    inv_env.resize(N);
    for (int i = 0; i < N; ++i) {
        const float a = window[i], b = window[(i + N / 2) % N];
        const float env = a * a + b * b;
        if (!(env > 1e-11f)) return false;
        inv_env[i] = (float)(1.0 / (double)env);
    }
    return true;
}

// exp(-2 pi i k / period), k = 0 .. count - 1, interleaved
std::vector<float> twiddles(int count, int period) {
    std::vector<float> tw(2 * count);
    for (int k = 0; k < count; ++k) { tw[2 * k] = (float)cos(2.0 * PI * k / period); tw[2 * k + 1] = (float)-sin(2.0 * PI * k / period); }
    return tw;
}

// n_fft 1024, a wavefront per stream: the same fp32 products the three-wave Griffin-Lim forms per lane (dn_gl_body.hpp: cw, wsyn), so the two
// schedules stay bit-identical
std::vector<float> glw_tables(int N, const std::vector<float>& window, const std::vector<float>& inv_env) {
    const int H = N / 2, NC = N / 2;
    std::vector<float> t((size_t)4 * NC * 2);
    for (int m = 0; m < NC; ++m) {
        const float w0 = window[2 * m], w1 = window[2 * m + 1];
        const int n0 = 2 * m, n1 = n0 + 1;
        for (int c = 0; c < 3; ++c) {
            int i0, i1;
            if (c == 1) { i0 = n0; i1 = n1; }
            else if (c == 0) { i0 = n0 < H ? H - n0 : n0 - H; i1 = n1 < H ? H - n1 : n1 - H; }
            else { i0 = n0 < H ? n0 + H : 3 * H - 2 - n0; i1 = n1 < H ? n1 + H : 3 * H - 2 - n1; }
            t[((size_t)c * NC + m) * 2] = w0 * inv_env[i0];
            t[((size_t)c * NC + m) * 2 + 1] = w1 * inv_env[i1];
        }
        t[((size_t)3 * NC + m) * 2] = w0 * (1.0f / (float)NC);
        t[((size_t)3 * NC + m) * 2 + 1] = w1 * (1.0f / (float)NC);
    }
    return t;
}

// HTK triangles [K][M], f_min 0, f_max sr//2, norm None
std::vector<float> htk_filterbank(int sample_rate, int K, int M) {
    std::vector<float> fb((size_t)K * M);
    const double f_hi = (double)(sample_rate / 2);
    const double mmax = 2595.0 * log10(1.0 + f_hi / 700.0);
    std::vector<double> fp(M + 2);
    for (int i = 0; i < M + 2; ++i) fp[i] = 700.0 * (pow(10.0, (mmax * i / (M + 1)) / 2595.0) - 1.0);
    for (int k = 0; k < K; ++k) {
        const double f = f_hi * k / (K - 1);
        for (int mm = 0; mm < M; ++mm) {
            const double up = (f - fp[mm]) / (fp[mm + 1] - fp[mm]), down = (fp[mm + 2] - f) / (fp[mm + 2] - fp[mm + 1]);
            fb[(size_t)k * M + mm] = (float)fmax(0.0, fmin(up, down));
        }
    }
    return fb;
}

// band structure: [first nonzero bin, last nonzero bin] of each filter, and the weights of the bands [maxlen][M]
struct MelBands {
    std::vector<int> start, len;
    int maxlen = 0;
    std::vector<float> mw;
};
MelBands mel_bands(const std::vector<float>& fb, int K, int M) {
    MelBands b;
    b.start.resize(M);
    b.len.resize(M);
    for (int mm = 0; mm < M; ++mm) {
        int lo = K, hi = -1;
        for (int k = 0; k < K; ++k)
            if (fb[(size_t)k * M + mm] != 0.0f) { lo = k < lo ? k : lo; hi = k; }
        b.start[mm] = hi < 0 ? 0 : lo;
        b.len[mm] = hi < 0 ? 0 : hi - lo + 1;
        b.maxlen = b.len[mm] > b.maxlen ? b.len[mm] : b.maxlen;
    }
    b.mw.assign((size_t)(b.maxlen ? b.maxlen : 1) * M, 0.0f);
    for (int mm = 0; mm < M; ++mm)
        for (int i = 0; i < b.len[mm]; ++i) b.mw[(size_t)i * M + mm] = fb[(size_t)(b.start[mm] + i) * M + mm];
    return b;
}

// pseudo-inverse of fb^T: fb (fb^T fb)^-1, the minimum-norm least-squares operator (Appendix B.4), and -- where the filterbank allows it -- its
// factored form: the band of (fb^T fb)^-1 (ginv) and the at most two filters of every bin (fb2); both empty otherwise.  false: rank deficient
struct MelInverse {
    std::vector<float> pinv, ginv, fb2;
};
bool mel_inverse(const std::vector<float>& fb, int K, int M, MelInverse& out) {
    std::vector<double> G((size_t)M * M, 0.0), R((size_t)M * K);
    for (int a = 0; a < M; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = 0.0;
            for (int k = 0; k < K; ++k) s += (double)fb[(size_t)k * M + a] * fb[(size_t)k * M + b];
            G[(size_t)a * M + b] = G[(size_t)b * M + a] = s;
        }
    for (int a = 0; a < M; ++a)
        for (int k = 0; k < K; ++k) R[(size_t)a * K + k] = fb[(size_t)k * M + a];   // fb^T
    std::vector<double> G2 = G, I((size_t)M * M, 0.0);
    for (int a = 0; a < M; ++a) I[(size_t)a * M + a] = 1.0;
    if (!chol_solve(G, R, M, K)) return false;
    // the factored form needs at most two filters a bin
    bool two = chol_solve(G2, I, M, M);
    std::vector<float>& f2 = out.fb2;
    f2.assign((size_t)K * 4, 0.0f);
    for (int k = 0; k < K && two; ++k) {
        int n = 0;
        for (int a = 0; a < M; ++a) {
            const float wv = fb[(size_t)k * M + a];
            if (wv == 0.0f) continue;
            if (n == 2) { two = false; break; }
            f2[(size_t)k * 4 + n] = wv;
            memcpy(&f2[(size_t)k * 4 + 2 + n], &a, 4);
            ++n;
        }
    }
    if (two) {   // the diagonals beyond the band must be below fp32 resolution
        double big = 0.0, beyond = 0.0;
        for (int a = 0; a < M; ++a)
            for (int c = 0; c < M; ++c) {
                const double v = fabs(I[(size_t)a * M + c]);
                big = v > big ? v : big;
                if (abs(a - c) > dn::kInvBand) beyond = v > beyond ? v : beyond;
            }
        two = beyond <= 1e-8 * big;
    }
    if (two) {
        const int taps = 2 * dn::kInvBand + 1;
        out.ginv.assign((size_t)taps * M, 0.0f);
        for (int t = 0; t < taps; ++t)
            for (int a = 0; a < M; ++a) {
                const int c = a - dn::kInvBand + t;
                if (c >= 0 && c < M) out.ginv[(size_t)t * M + a] = (float)I[(size_t)a * M + c];
            }
    } else f2.clear();
    out.pinv.resize((size_t)K * M);
    for (int k = 0; k < K; ++k)
        for (int a = 0; a < M; ++a) out.pinv[(size_t)k * M + a] = (float)R[(size_t)a * K + k];
    return true;
}

// packed mel schedule: groups of 16 filters, four lanes a filter, lane l of step u of a group takes tap 4 u + l % 4.  steps == 0 (and q empty):
// the filterbank needs more steps than the kernels unroll
struct MelSchedule {
    std::vector<float> q;
    int steps = 0;
    unsigned long long last = 0;      // bit s: step s is the last of its group
};
MelSchedule mel_schedule(const MelBands& b, int N, int M) {
    MelSchedule s;
    for (int g = 0; g < (M + 15) / 16; ++g) {       // the last group may be partial: lanes of filters that do not exist carry zero weights
        int gl = 0;
        for (int f = 0; f < 16 && 16 * g + f < M; ++f) gl = b.len[16 * g + f] > gl ? b.len[16 * g + f] : gl;
        const int steps = gl ? (gl + 3) / 4 : 1;
        for (int u = 0; u < steps; ++u)
            for (int l = 0; l < 64; ++l) {
                const int mm = 16 * g + l / 4, i = 4 * u + l % 4;
                const bool tap = mm < M && i < b.len[mm];
                const int bin = tap ? b.start[mm] + i : 0;
                float bits;
                memcpy(&bits, &bin, 4);
                s.q.push_back(tap ? b.mw[(size_t)i * M + mm] : 0.0f);
                s.q.push_back(bits);
            }
        s.steps += steps;
        if (s.steps <= dn::mel_q_steps(N)) s.last |= 1ull << (s.steps - 1);
    }
    if (s.steps > dn::mel_q_steps(N)) return MelSchedule();
    s.q.resize((size_t)dn::mel_q_steps(N) * 64 * 2, 0.0f);         // padded to the full schedule with (weight 0, bin 0): the kernel loads every step unconditionally
    return s;
}

// the checks the stateless wrappers start with, in their order: null arguments, (need_mel) a plan with mel stages, negative sizes ("batch" / "size")
int check_dsp_args(const char* who, const dn_dsp* d, bool pointers, bool need_mel, bool sizes, const char* size_word) {
    if (!d || !pointers) return fail(DN_ERR_INVALID, std::string(who) + ": null argument");
    if (need_mel && d->cfg.n_mels <= 0) return fail(DN_ERR_INVALID, "plan was created without mel stages");
    if (!sizes) return fail(DN_ERR_INVALID, std::string(who) + ": negative " + size_word);
    return DN_OK;
}

constexpr long long kGlgMaxRows = 1ll << 22;          // B x T of one dn_griffinlim_general call: every grid and 32-bit index stays in range

int refuse_init_angles(const char* who) { return fail(DN_ERR_INVALID, std::string(who) + ": DN_PHASE_FROM_INPUT takes the phases from the input: init_angles must be NULL"); }

// The workspace of dn_process_frame / dn_stream_step, in floats: mel [B][3][M] | residual [B][3][M] | linear magnitude [B][3][K] | peak [B], then (each
// from a 256-byte boundary) one denoised frame for dn_stream_step and -- DN_PHASE_FROM_INPUT -- the phasor rows
struct FrameWs {
    size_t diff, peak;      // floats from the start
    size_t phas;            // bytes from the start: what the entry points needed before input-phase mode
};
FrameWs frame_ws(const dn_dsp* d, int32_t B) {
    const size_t M = (size_t)d->cfg.n_mels, K = (size_t)d->cfg.n_fft / 2 + 1, b = (size_t)B;
    FrameWs w;
    w.diff = b * 3 * M;
    w.peak = b * 6 * M + b * 3 * K;
    w.phas = ((b * (6 * M + 3 * K + 1) * sizeof(float) + 255) & ~size_t(255)) + ((b * d->cfg.n_fft * sizeof(float) + 255) & ~size_t(255));
    return w;
}

// what dn_process_frame and dn_stream_step share once their own pointers are checked: the remaining checks, the bias tables and the common arguments
int frame_args(const char* who, const dn_model* m, const dn_dsp* d, float* hx, const float* init_angles, uint64_t seed, uint64_t stream_id0,
               int32_t n_iter, float momentum, void* workspace, int32_t B, uint32_t flags, dn::FrameArgs& a, const BiasSet** bs) {
    DN_TRY(check_hop_args(who, m, d, B, n_iter, momentum, flags, &a.mom));
    if ((flags & DN_PHASE_FROM_INPUT) && init_angles) return refuse_init_angles(who);
    a.C = d->cfg.n_mels / 16;
    DN_TRY(build_bias(m, a.C, bs));
    const FrameWs w = frame_ws(d, B);
    float* ws = static_cast<float*>(workspace);
    a.hx = hx;
    a.mel = ws; a.diff = ws + w.diff; a.peak = ws + w.peak;
    a.init = init_angles; a.seed = seed; a.sid0 = stream_id0;
    a.n_iter = n_iter;
    if (flags & DN_PHASE_FROM_INPUT) a.phas = reinterpret_cast<float*>(static_cast<char*>(workspace) + w.phas);
    return DN_OK;
}

}  // namespace

extern "C" {

int dn_dsp_create(const dn_dsp_cfg* cfg, const float* fb_in, const float* pinv_in, const float* window_in, dn_dsp** out) {
    if (!cfg || !out) return fail(DN_ERR_INVALID, "dn_dsp_create: null argument");
    if ((cfg->n_fft != 512 && cfg->n_fft != 1024 && cfg->n_fft != 1536) || cfg->hop != cfg->n_fft / 2)
        return fail(DN_ERR_UNSUPPORTED, "kernels are built for n_fft 512, 1024 or 1536 with hop = n_fft/2 (got n_fft " +
                                            std::to_string(cfg->n_fft) + ", hop " + std::to_string(cfg->hop) + ")");
    const int N = cfg->n_fft, K = N / 2 + 1, M = cfg->n_mels, NC = N / 2;
    if (M < 0 || M > 128) return fail(DN_ERR_UNSUPPORTED, "n_mels must be in 0..128");
    if (M > 0 && cfg->sample_rate <= 0) return fail(DN_ERR_INVALID, "sample_rate must be positive");
    std::unique_ptr<dn_dsp> d(new dn_dsp());
    d->cfg = *cfg;
    DevArena& ar = d->arena;
    std::vector<float> inv_env;
    if (!window_tables(N, window_in, d->window, inv_env)) return fail(DN_ERR_INVALID, "window overlap-add envelope is ~0 (torch.istft would raise)");
    const size_t o_twc = ar.add(twiddles(NC, NC)), o_twr = ar.add(twiddles(NC / 2 + 1, N));      // exp(-2 pi i k / (n_fft/2)), exp(-2 pi i k / n_fft)
    const size_t o_win = ar.add(d->window), o_env = ar.add(inv_env);
    const size_t o_glw = N == 1024 ? ar.add(glw_tables(N, d->window, inv_env)) : 0;
    size_t o_q = 0, o_ms = 0, o_ml = 0, o_mw = 0, o_pinv = 0, o_ginv = 0, o_fb2 = 0;
    MelBands bands;
    MelInverse inv;
    MelSchedule sched;
    const int pstride = ((K + 767) / 768) * 768;      // the contraction kernels stream rows in rounds of 192 or 256 bins (zero padded: tail loads stay in bounds)
    if (M > 0) {
        d->fb = fb_in ? std::vector<float>(fb_in, fb_in + (size_t)K * M) : htk_filterbank(cfg->sample_rate, K, M);
        bands = mel_bands(d->fb, K, M);
        if (pinv_in) inv.pinv.assign(pinv_in, pinv_in + (size_t)K * M);      // (the caller's operator: no factored form)
        else if (!mel_inverse(d->fb, K, M, inv)) return fail(DN_ERR_INVALID, "mel filterbank is rank deficient; pass pinv explicitly");
        d->pinv = inv.pinv;
        std::vector<float> pt((size_t)((M + 15) / 16 * 16) * pstride, 0.0f);      // zero rows up to a multiple of 16: the dense loop walks 16 filters a round
        for (int k = 0; k < K; ++k)
            for (int a = 0; a < M; ++a) pt[(size_t)a * pstride + k] = d->pinv[(size_t)k * M + a];
        sched = mel_schedule(bands, N, M);
        if (sched.steps) o_q = ar.add(sched.q);
        o_ms = ar.add(bands.start);
        o_ml = ar.add(bands.len);
        o_mw = ar.add(bands.mw);
        o_pinv = ar.add(pt);
        if (!inv.ginv.empty()) { o_ginv = ar.add(inv.ginv); o_fb2 = ar.add(inv.fb2); }
    }
    hipError_t e = ar.upload();
    if (e != hipSuccess) return fail(DN_ERR_HIP, std::string("plan upload: ") + hipGetErrorString(e));
    dn::DspDev& v = d->view;
    const bool has_factors = !inv.ginv.empty();
    v.n_fft = N; v.n_mels = M; v.mel_maxlen = bands.maxlen; v.pinv_stride = pstride;
    v.twc = ar.ptr<float2>(o_twc); v.twr = ar.ptr<float2>(o_twr);
    v.window = ar.ptr<float>(o_win); v.inv_env = ar.ptr<float>(o_env);
    v.glw_tables = N == 1024 ? ar.ptr<float2>(o_glw) : nullptr;
    v.mel_q = sched.steps ? ar.ptr<float2>(o_q) : nullptr; v.mel_qsteps = sched.steps; v.mel_qlast = sched.last;
    v.mel_start = M ? ar.ptr<int>(o_ms) : nullptr; v.mel_len = M ? ar.ptr<int>(o_ml) : nullptr;
    v.mel_w = M ? ar.ptr<float>(o_mw) : nullptr; v.pinv_t = M ? ar.ptr<float>(o_pinv) : nullptr;
    v.ginv_band = has_factors ? ar.ptr<float>(o_ginv) : nullptr; v.fb2 = has_factors ? ar.ptr<float4>(o_fb2) : nullptr;
    e = d->view_dev.alloc_copy(&d->view, sizeof(d->view));
    if (e != hipSuccess) return fail(DN_ERR_HIP, std::string("plan view: ") + hipGetErrorString(e));
    *out = d.release();
    return DN_OK;
}

void dn_dsp_destroy(dn_dsp* d) { Ref<dn_dsp>::drop(d); }

int dn_dsp_get_tables(const dn_dsp* d, float* fb, float* pinv, float* window) {
    if (!d) return fail(DN_ERR_INVALID, "dn_dsp_get_tables: null plan");
    if (fb && !d->fb.empty()) memcpy(fb, d->fb.data(), d->fb.size() * 4);
    if (pinv && !d->pinv.empty()) memcpy(pinv, d->pinv.data(), d->pinv.size() * 4);
    if (window) memcpy(window, d->window.data(), d->window.size() * 4);
    return DN_OK;
}

// ---- stateless stages.  An empty batch is nothing to do (pointers of empty tensors are null); B == 0 returns before the arguments are looked at,
// B x T == 0 after
int dn_stft(const dn_dsp* d, const float* frames, float* spec, int32_t B, uint32_t flags, void* stream) {
    if (B == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_stft", d, frames && spec, false, B >= 0, "batch"));
    dn::launch_stft(d->view, frames, spec, nullptr, nullptr, B, flags, as_stream(stream));
    return check_launch("stft_kernel");
}

int dn_stft_mel_log1p(const dn_dsp* d, const float* frames, float* mel, float* peak, int32_t B, uint32_t flags, void* stream) {
    if (B == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_stft_mel_log1p", d, frames && mel, true, B >= 0, "batch"));
    dn::launch_stft(d->view, frames, nullptr, mel, peak, B, flags, as_stream(stream));
    return check_launch("stft_kernel");
}

int dn_stft_phasors(const dn_dsp* d, const float* frames, float* phasors, int32_t B, uint32_t flags, void* stream) {
    if (B == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_stft_phasors", d, frames && phasors, false, B >= 0, "batch"));
    dn::launch_stft_phasors(d->view, frames, phasors, B, flags, as_stream(stream));
    return check_launch("stft_phasor_kernel");
}

int dn_mel_scale(const dn_dsp* d, const float* mag, float* mel, int32_t B, int32_t T, void* stream) {
    int rc = check_dsp_args("dn_mel_scale", d, mag && mel, true, B >= 0 && T >= 0, "size");
    if (rc != DN_OK || (int64_t)B * T == 0) return rc;
    dn::launch_mel(d->view, mag, mel, B * T, as_stream(stream));
    return check_launch("mel_kernel");
}

int dn_invmel(const dn_dsp* d, const float* mel_mag, float* lin, int32_t B, int32_t T, void* stream) {
    int rc = check_dsp_args("dn_invmel", d, mel_mag && lin, true, B >= 0 && T >= 0, "size");
    if (rc != DN_OK || (int64_t)B * T == 0) return rc;
    dn::launch_invmel(d->view, mel_mag, nullptr, lin, B * T, as_stream(stream));
    return check_launch("invmel_kernel");
}

int dn_residual_invmel(const dn_dsp* d, const float* x, const float* diff, float* lin, int32_t B, int32_t T, void* stream) {
    int rc = check_dsp_args("dn_residual_invmel", d, x && diff && lin, true, B >= 0 && T >= 0, "size");
    if (rc != DN_OK || (int64_t)B * T == 0) return rc;
    dn::launch_invmel(d->view, x, diff, lin, B * T, as_stream(stream));
    return check_launch("invmel_kernel");
}

int dn_griffinlim(const dn_dsp* d, const float* mag, const float* init_angles, uint64_t seed, uint64_t stream_id0,
                  const float* scale, float* wave, int32_t B, int32_t n_iter, float momentum, void* stream) {
    if (B == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_griffinlim", d, mag && wave, false, B >= 0 && n_iter >= 0, "size"));
    DN_TRY(check_momentum(momentum, nullptr));
    dn::launch_griffinlim(d->view, mag, init_angles, seed, stream_id0, scale, wave, B, n_iter, momentum, as_stream(stream));
    return check_launch("griffinlim_kernel");
}

int dn_griffinlim_draw_phases(const dn_dsp* d, uint64_t seed, uint64_t stream_id0, float* angles_out, int32_t B, void* stream) {
    if (B == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_griffinlim_draw_phases", d, angles_out != nullptr, false, B >= 0, "batch"));
    dn::launch_draw_phases(d->view, angles_out, seed, stream_id0, B, as_stream(stream));
    return check_launch("draw_phases_kernel");
}

int dn_synthesis(const dn_dsp* d, const float* x, const float* diff, const float* init_angles, uint64_t seed, uint64_t stream_id0,
                 const float* scale, float* wave, int32_t B, int32_t n_iter, float momentum, void* stream) {
    if (B == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_synthesis", d, x && diff && wave, true, B >= 0 && n_iter >= 0, "size"));
    DN_TRY(check_momentum(momentum, nullptr));
    dn::launch_synthesis(d->view, x, diff, init_angles, seed, stream_id0, scale, wave, B, n_iter, momentum, as_stream(stream));
    return check_launch("griffinlim_kernel<from mel>");
}

int dn_istft(const dn_dsp* d, const float* spec, float* wave, int32_t B, void* stream) {
    if (B == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_istft", d, spec && wave, false, B >= 0, "batch"));
    dn::launch_griffinlim(d->view, nullptr, spec, 0, 0, nullptr, wave, B, 0, 0.0f, as_stream(stream));
    return check_launch("griffinlim_kernel(istft)");
}

// ---- server (any-length) stages
int dn_stft_general(const dn_dsp* d, const float* x, float* spec, float* logmel, int32_t B, int32_t L, void* stream) {
    if (B == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_stft_general", d, x && (spec || logmel), false, B >= 0, "batch"));
    if (L <= d->cfg.n_fft / 2) return fail(DN_ERR_INVALID, "dn_stft_general: reflect padding needs more than n_fft/2 samples (as torch.stft)");
    if (logmel && d->cfg.n_mels <= 0) return fail(DN_ERR_INVALID, "plan was created without mel stages");
    dn::launch_stft_general(d->view, x, spec, logmel, B, L, as_stream(stream));
    return check_launch("stft_general_kernel");
}

int dn_server_rows(const dn_dsp* d, const float* logmel, const float* model_out, const float* spec_in, float* spec_out, int32_t rows, void* stream) {
    if (rows == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_server_rows", d, logmel && model_out && spec_in && spec_out, false, rows >= 0, "size"));
    if (d->cfg.n_mels <= 0) return fail(DN_ERR_INVALID, "plan was created without mel stages");
    dn::launch_server_rows(d->view, logmel, model_out, spec_in, spec_out, rows, as_stream(stream));
    return check_launch("server_rows_kernel");
}

int dn_istft_general(const dn_dsp* d, const float* spec, float* wave, int32_t B, int32_t T, void* stream) {
    if (B == 0) return DN_OK;
    if (!d || !spec || !wave) return fail(DN_ERR_INVALID, "dn_istft_general: null argument");
    if (B < 0 || T < 2) return fail(DN_ERR_INVALID, "dn_istft_general: need B >= 0 and at least 2 columns");
    dn::launch_istft_general(d->view, spec, wave, B, T, as_stream(stream));
    return check_launch("istft_general_kernel");
}

// ---- Griffin-Lim on any number of columns.  The workspace is the caller's: X | prev ([B][T][K] complex each) | the rebuilt signal [B][hop (T - 1)]
int32_t dn_griffinlim_general_whole_max(const dn_dsp* d) { return d ? dn::kGlgWholeMax : 0; }

size_t dn_griffinlim_general_workspace_bytes(const dn_dsp* d, int32_t B, int32_t T) {
    if (!d || B <= 0 || T < 3 || (long long)B * T > kGlgMaxRows) return 0;
    const size_t rows = (size_t)B * (size_t)T, K = (size_t)d->cfg.n_fft / 2 + 1;
    return ((2 * rows * K * 2 + (size_t)B * (size_t)(T - 1) * (d->cfg.n_fft / 2)) * sizeof(float) + 255) & ~size_t(255);
}

int dn_griffinlim_general(const dn_dsp* d, const float* mag, const float* init_angles, uint64_t seed, uint64_t stream_id0, float* wave,
                          void* workspace, int32_t B, int32_t T, int32_t n_iter, float momentum, uint32_t flags, void* stream) {
    if (B == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_griffinlim_general", d, mag && wave && workspace, false, B >= 0 && n_iter >= 0, "size"));
    if (T < 3) return fail(DN_ERR_INVALID, "dn_griffinlim_general: needs at least 3 columns (reflect padding needs hop*(T-1) > n_fft/2, as torch.stft)");
    if ((long long)B * T > kGlgMaxRows) return fail(DN_ERR_INVALID, "dn_griffinlim_general: B x T exceeds " + std::to_string(kGlgMaxRows) + " columns a call");
    dn::GlgArgs a{};
    DN_TRY(check_momentum(momentum, &a.mom));
    if (flags & ~(uint32_t)(DN_GLG_WHOLE | DN_GLG_STEPS | DN_GL_INIT_NORMALIZE)) return fail(DN_ERR_INVALID, "dn_griffinlim_general: unknown flag bits");
    const uint32_t form = flags & (uint32_t)(DN_GLG_WHOLE | DN_GLG_STEPS);
    if (form == (uint32_t)(DN_GLG_WHOLE | DN_GLG_STEPS)) return fail(DN_ERR_INVALID, "dn_griffinlim_general: DN_GLG_WHOLE and DN_GLG_STEPS exclude each other");
    if ((flags & DN_GL_INIT_NORMALIZE) && !init_angles) return fail(DN_ERR_INVALID, "dn_griffinlim_general: DN_GL_INIT_NORMALIZE needs init_angles (the spectrum to take the phases from)");
    if ((form & DN_GLG_WHOLE) && T > dn::kGlgWholeMax)
        return fail(DN_ERR_UNSUPPORTED, "dn_griffinlim_general: DN_GLG_WHOLE holds at most " + std::to_string(dn::kGlgWholeMax) + " columns on chip (got " + std::to_string(T) + ")");
    const size_t rows = (size_t)B * (size_t)T, K = (size_t)d->cfg.n_fft / 2 + 1;
    a.mag = mag; a.init = init_angles; a.normalize = (flags & DN_GL_INIT_NORMALIZE) != 0; a.seed = seed; a.sid0 = stream_id0; a.wave = wave;
    a.x = static_cast<float*>(workspace); a.prev = a.x + rows * K * 2; a.sig = a.prev + rows * K * 2;
    a.B = B; a.T = T; a.n_iter = n_iter;
    if (form == DN_GLG_STEPS || (form == 0 && T > dn::kGlgWholeMax)) {
        dn::launch_glg_steps(d->view, a, as_stream(stream));
        return check_launch("glg_step_kernel");
    }
    dn::launch_glg_whole(d->view, a, as_stream(stream));
    return check_launch("glg_whole_kernel");
}

int dn_griffinlim_draw_phases_general(const dn_dsp* d, uint64_t seed, uint64_t stream_id0, float* angles_out, int32_t B, int32_t T, void* stream) {
    if (B == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_griffinlim_draw_phases_general", d, angles_out != nullptr, false, B >= 0 && T >= 1 && (long long)B * T <= kGlgMaxRows, "size"));
    dn::launch_draw_phases_general(d->view, angles_out, seed, stream_id0, B, T, as_stream(stream));
    return check_launch("glg_draw_kernel");
}

int dn_server_mag(const dn_dsp* d, const float* logmel, const float* model_out, float* mag_out, int32_t rows, void* stream) {
    if (rows == 0) return DN_OK;
    DN_TRY(check_dsp_args("dn_server_mag", d, logmel && model_out && mag_out, true, rows >= 0, "size"));
    dn::launch_server_mag(d->view, logmel, model_out, mag_out, rows, as_stream(stream));
    return check_launch("server_rows_kernel<magnitude>");
}

// ---- the whole hop in one launch
size_t dn_workspace_bytes(const dn_dsp* d, int32_t B) { return !d || B <= 0 ? 0 : frame_ws(d, B).phas; }

size_t dn_workspace_bytes_ex(const dn_dsp* d, int32_t B, uint32_t flags) {
    if (flags & ~kHopFlags) return 0;
    const size_t base = dn_workspace_bytes(d, B);
    return base == 0 || !(flags & DN_PHASE_FROM_INPUT) ? base : base + phasor_bytes(d, (size_t)B);
}

int dn_process_frame(const dn_model* m, const dn_dsp* d, const float* frames, float* hx, float* out, float* mel_residual_out, const float* init_angles, uint64_t seed, uint64_t stream_id0,
                     int32_t n_iter, float momentum, void* workspace, int32_t B, uint32_t flags, void* stream) {
    if (B == 0) return DN_OK;      // empty batch: nothing to do (pointers of empty tensors are null)
    if (!frames || !hx || !out || !workspace) return fail(DN_ERR_INVALID, "dn_process_frame: null argument");
    dn::FrameArgs a{};
    const BiasSet* bs = nullptr;
    DN_TRY(frame_args("dn_process_frame", m, d, hx, init_angles, seed, stream_id0, n_iter, momentum, workspace, B, flags, a, &bs));
    a.frames = frames; a.out = out;
    if (mel_residual_out) a.diff = mel_residual_out;
    dn::launch_frame(d->view, bs->view, a, B, (flags & DN_CONV_BF16) != 0, as_stream(stream));      // P1-P12, one launch
    return check_launch("frame_kernel");
}

int dn_stream_step(const dn_model* m, const dn_dsp* d, const float* hop_in, float* ring, float* ola, float* hx, float* hop_out, const float* init_angles, uint64_t seed, uint64_t stream_id0,
                   int32_t n_iter, float momentum, void* workspace, int32_t B, uint32_t flags, void* stream) {
    if (B == 0) return DN_OK;      // empty batch: nothing to do (pointers of empty tensors are null)
    // every argument is validated before the first (and only) launch, so a failed call leaves ring, ola and hx untouched
    if (!hop_in || !ring || !ola || !hx || !hop_out || !workspace) return fail(DN_ERR_INVALID, "dn_stream_step: null argument");
    dn::FrameArgs a{};
    const BiasSet* bs = nullptr;
    DN_TRY(frame_args("dn_stream_step", m, d, hx, init_angles, seed, stream_id0, n_iter, momentum, workspace, B, flags, a, &bs));
    a.hop_in = hop_in; a.ring = ring; a.ola = ola; a.hop_out = hop_out;
    dn::launch_frame(d->view, bs->view, a, B, (flags & DN_CONV_BF16) != 0, as_stream(stream));
    return check_launch("frame_kernel(stream)");
}

// ------------------------------------------------------------------ clip mode: N hops per call
// frame rows | mel | residual | peak, in floats per frame (dn_clip.hip)
static size_t clip_row_floats(const dn_dsp* d) { return d->cfg.n_fft == 1024 ? (size_t)dn::kClipRow1024 : (size_t)d->cfg.n_fft; }
constexpr long long kClipMaxFrames = 1ll << 22;          // B x N of one call: every grid and every 32-bit index of the kernels stays in range

size_t dn_clip_workspace_bytes(const dn_dsp* d, int32_t B, int32_t N) {
    if (!d || B <= 0 || N <= 0 || d->cfg.n_mels <= 0 || (long long)B * N > kClipMaxFrames) return 0;
    const size_t frames = (size_t)B * (size_t)N;
    return ((frames * (clip_row_floats(d) + 6 * (size_t)d->cfg.n_mels + 1) * sizeof(float) + 255) & ~size_t(255)) + 256;
}

size_t dn_clip_workspace_bytes_ex(const dn_dsp* d, int32_t B, int32_t N, uint32_t flags) {
    if (flags & ~(kHopFlags | DN_CLIP_GL_PER_COLUMN | DN_CLIP_GL_PER_STREAM)) return 0;
    const size_t base = dn_clip_workspace_bytes(d, B, N);
    return base == 0 || !(flags & DN_PHASE_FROM_INPUT) ? base : base + phasor_bytes(d, (size_t)B * (size_t)N);
}

// the rows of a call's workspace, F frames from `rows` on: frame rows | mel | residual | peak, then the phasor rows of an input-phase call (the
// uniform call's layout, F = B x N; a ragged call's behind its table)
static void clip_carve(dn::ClipArgs& a, const dn_dsp* d, void* rows, size_t F, uint32_t flags) {
    const int M = d->cfg.n_mels;
    a.frames = F;
    a.fr = static_cast<float*>(rows); a.fr_stride = clip_row_floats(d);
    a.mel = a.fr + F * a.fr_stride; a.diff = a.mel + F * 3 * M; a.peak = a.diff + F * 3 * M;
    if (flags & DN_PHASE_FROM_INPUT) a.phas = reinterpret_cast<float*>(static_cast<char*>(rows) + dn_clip_workspace_bytes(d, 1, (int32_t)F));
}

int dn_clip_process(const dn_model* m, const dn_dsp* d, const void* hops_in, int32_t in_s16, float* ring, float* ola, float* hx, void* hops_out, int32_t out_s16, const float* init_angles,
                    uint64_t seed, uint64_t stream_id0, int32_t n_iter, float momentum, void* workspace, int32_t B, int32_t N, uint32_t flags, void* stream) {
    // every argument is validated before the first launch, so a failed call leaves ring, ola and hx untouched
    if (B < 1 || N < 1) return fail(DN_ERR_INVALID, "dn_clip_process: needs B >= 1 streams and N >= 1 hops");
    if (!hops_in || !ring || !ola || !hx || !hops_out || !workspace) return fail(DN_ERR_INVALID, "dn_clip_process: null argument");
    const uint32_t gl = flags & (uint32_t)(DN_CLIP_GL_PER_COLUMN | DN_CLIP_GL_PER_STREAM);
    dn::ClipArgs a{};
    DN_TRY(check_hop_args("dn_clip_process", m, d, B, n_iter, momentum, flags & ~gl, &a.mom));
    if (gl == (uint32_t)(DN_CLIP_GL_PER_COLUMN | DN_CLIP_GL_PER_STREAM)) return fail(DN_ERR_INVALID, "dn_clip_process: DN_CLIP_GL_PER_COLUMN and DN_CLIP_GL_PER_STREAM exclude each other");
    if ((gl & DN_CLIP_GL_PER_STREAM) && d->cfg.n_fft != 1024) return refuse_not_1024("the wavefront-per-stream Griffin-Lim is built");
    if ((flags & DN_PHASE_FROM_INPUT) && init_angles) return refuse_init_angles("dn_clip_process");
    if ((long long)B * N > kClipMaxFrames) return fail(DN_ERR_INVALID, "dn_clip_process: B x N exceeds " + std::to_string(kClipMaxFrames) + " frames a call (tile the clip)");
    const int M = d->cfg.n_mels, C = M / 16;
    const BiasSet* bs = nullptr;
    DN_TRY(build_bias(m, C, &bs));
    a.hops_in = hops_in; a.in_s16 = in_s16 != 0; a.ring = ring; a.ola = ola; a.hx = hx; a.hops_out = hops_out; a.out_s16 = out_s16 != 0;
    a.init = init_angles; a.seed = seed; a.sid0 = stream_id0; a.n_iter = n_iter;
    a.C = C; a.B = B; a.N = N; a.n_fft = d->cfg.n_fft; a.n_mels = M;
    clip_carve(a, d, workspace, (size_t)B * (size_t)N, flags);
    a.per_stream = d->cfg.n_fft == 1024 && ((gl & DN_CLIP_GL_PER_STREAM) || (gl == 0 && (long)a.frames >= dn::kClipGlwAutoFrames));
    dn::launch_clip(d->view, bs->view_dev.get(), a, (flags & DN_CONV_BF16) != 0, as_stream(stream));
    return check_launch("dn_clip_process");
}

// ---- ragged: stream b runs n_hops[b] hops.  The table -- off [B + 1] int32 (to an 8-byte boundary), frame0 [B] uint64 -- heads the workspace, rounded
// up to 256 bytes; the uniform call's layout for F = sum n_hops frames follows
static size_t clip_table_bytes(int32_t B) {
    const size_t off = ((size_t)B + 1) * sizeof(int32_t);
    return ((((off + 7) & ~size_t(7)) + (size_t)B * sizeof(uint64_t)) + 255) & ~size_t(255);
}

size_t dn_clip_ragged_workspace_bytes(const dn_dsp* d, int32_t B, int64_t total_hops, uint32_t flags) {
    if (B < 1 || total_hops < 1 || total_hops > kClipMaxFrames) return 0;
    const size_t rows = dn_clip_workspace_bytes_ex(d, 1, (int32_t)total_hops, flags);          // (0: a null plan, one without mel stages, unknown flag bits)
    return rows == 0 ? 0 : clip_table_bytes(B) + rows;
}

int dn_clip_process_ragged(const dn_model* m, const dn_dsp* d, const void* hops_in, int32_t in_s16, float* ring, float* ola, float* hx, void* hops_out, int32_t out_s16,
                           const float* init_angles, uint64_t seed, uint64_t stream_id0, const int32_t* n_hops, const uint64_t* frame0, int32_t n_iter, float momentum,
                           void* workspace, int32_t B, uint32_t flags, void* stream) {
    // every argument is validated before the table is copied and the first kernel launched, so a failed call leaves ring, ola, hx, hops_out and the
    // workspace untouched
    if (B < 1) return fail(DN_ERR_INVALID, "dn_clip_process_ragged: needs B >= 1 streams");
    if (!n_hops) return fail(DN_ERR_INVALID, "dn_clip_process_ragged: null n_hops");
    long long F = 0;
    for (int32_t b = 0; b < B; ++b) {
        if (n_hops[b] < 0) return fail(DN_ERR_INVALID, "dn_clip_process_ragged: n_hops[" + std::to_string(b) + "] is negative");
        F += n_hops[b];
    }
    if (F > kClipMaxFrames) return fail(DN_ERR_INVALID, "dn_clip_process_ragged: sum n_hops exceeds " + std::to_string(kClipMaxFrames) + " frames a call (tile the clips)");
    const uint32_t gl = flags & (uint32_t)(DN_CLIP_GL_PER_COLUMN | DN_CLIP_GL_PER_STREAM);
    dn::ClipArgs a{};
    DN_TRY(check_hop_args("dn_clip_process_ragged", m, d, B, n_iter, momentum, flags & ~gl, &a.mom));
    if (gl == (uint32_t)(DN_CLIP_GL_PER_COLUMN | DN_CLIP_GL_PER_STREAM)) return fail(DN_ERR_INVALID, "dn_clip_process_ragged: DN_CLIP_GL_PER_COLUMN and DN_CLIP_GL_PER_STREAM exclude each other");
    if ((gl & DN_CLIP_GL_PER_STREAM) && d->cfg.n_fft != 1024) return refuse_not_1024("the wavefront-per-stream Griffin-Lim is built");
    if ((flags & DN_PHASE_FROM_INPUT) && init_angles) return refuse_init_angles("dn_clip_process_ragged");
    if (F == 0) return DN_OK;          // no stream has a hop: nothing is enqueued
    if (!hops_in || !ring || !ola || !hx || !hops_out || !workspace) return fail(DN_ERR_INVALID, "dn_clip_process_ragged: null argument");
    const int M = d->cfg.n_mels, C = M / 16;
    const BiasSet* bs = nullptr;
    DN_TRY(build_bias(m, C, &bs));
    // the table, built in a vector of the library's own (the caller's arrays are free again when the call returns) and copied in stream order to
    // the head of the workspace: the source is pageable, so the copy has left it when hipMemcpyAsync returns
    const size_t off_bytes = ((((size_t)B + 1) * sizeof(int32_t)) + 7) & ~size_t(7), table = off_bytes + (size_t)B * sizeof(uint64_t);
    thread_local std::vector<uint64_t> host;          // (kept from call to call: no allocation once it has grown)
    host.assign(table / sizeof(uint64_t), 0);
    int32_t* off = reinterpret_cast<int32_t*>(host.data());
    uint64_t* f0 = host.data() + off_bytes / sizeof(uint64_t);
    off[0] = 0;
    for (int32_t b = 0; b < B; ++b) {
        off[b + 1] = off[b] + n_hops[b];
        f0[b] = frame0 ? frame0[b] : 0;
    }
    DN_HIP(hipMemcpyAsync(workspace, host.data(), table, hipMemcpyHostToDevice, as_stream(stream)));
    a.off = static_cast<const int*>(workspace);
    a.frame0 = reinterpret_cast<const uint64_t*>(static_cast<const char*>(workspace) + off_bytes);
    a.hops_in = hops_in; a.in_s16 = in_s16 != 0; a.ring = ring; a.ola = ola; a.hx = hx; a.hops_out = hops_out; a.out_s16 = out_s16 != 0;
    a.init = init_angles; a.seed = seed; a.sid0 = stream_id0; a.n_iter = n_iter;
    a.C = C; a.B = B; a.N = 0; a.n_fft = d->cfg.n_fft; a.n_mels = M;
    clip_carve(a, d, static_cast<char*>(workspace) + clip_table_bytes(B), (size_t)F, flags);
    a.per_stream = d->cfg.n_fft == 1024 && ((gl & DN_CLIP_GL_PER_STREAM) || (gl == 0 && (long)a.frames >= dn::kClipGlwAutoFrames));
    dn::launch_clip(d->view, bs->view_dev.get(), a, (flags & DN_CONV_BF16) != 0, as_stream(stream));
    return check_launch("dn_clip_process_ragged");
}

}  // extern "C"
