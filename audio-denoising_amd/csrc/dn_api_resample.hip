// dn_api_resample.hip -- dn_resample: the geometry and the sinc table of a rate pair (pure host functions, then one arena) and the two entry
// points, the whole-signal call and the push of a stream.  No kernel code here.
#include <math.h>

#include "dn_host.hpp"

namespace {

const double PI = 3.14159265358979323846;
constexpr int kMaxRate = 1024;                   // o and n of the reduced pair
constexpr long long kMaxTable = 1ll << 19;       // n x KW floats (2 MB)

int gcd(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

int bad_rows(const char* who, const char* what, long long stride, long long need) {
    return fail(DN_ERR_INVALID, std::string(who) + ": " + what + " " + std::to_string(stride) + " is shorter than the " + std::to_string(need) + " samples of a row");
}

// what both entry points fill in the same way once their sizes are checked
void common_args(const dn_resampler* r, const void* x, int32_t in_s16, void* y, int32_t out_s16, int32_t B, int64_t x_stride, int64_t y_stride, dn::ResampleArgs& a) {
    a.x = x; a.in_s16 = in_s16 != 0; a.x_stride = x_stride;
    a.y = y; a.out_s16 = out_s16 != 0; a.y_stride = y_stride;
    a.table = r->table; a.o = r->o; a.n = r->n; a.KW = r->KW; a.np = r->np; a.B = B; a.small = r->small;
    const uintptr_t xe = a.in_s16 ? 2 : 4, ye = a.out_s16 ? 2 : 4;
    a.x_vec = reinterpret_cast<uintptr_t>(x) % (4 * xe) == 0 && x_stride % 4 == 0;
    a.y_pair = reinterpret_cast<uintptr_t>(y) % (2 * ye) == 0 && y_stride % 2 == 0;
}

// the work-items of launch_resample's grid must fit 32 bits (workgroups x work-items a workgroup: what the runtime takes)
int check_grid(const char* who, const dn_resampler* r, int32_t B, long long nblk) {
    const long long per_row = r->small ? (nblk + dn::kRsTileQ - 1) / dn::kRsTileQ : ((nblk + dn::kRsGenBlocks - 1) / dn::kRsGenBlocks) * ((r->np + dn::kRsGenPhases - 1) / dn::kRsGenPhases);
    if ((long long)B * per_row > 0xffffffffll / (r->small ? dn::kRsThreads : dn::kRsGenThreads)) return fail(DN_ERR_INVALID, std::string(who) + ": B x the row length exceeds what one launch carries (split the batch)");
    return DN_OK;
}

}  // namespace

// ---- the geometry and the Hann table of a rate pair: shared with the rate banks (dn_api_ratebank.hip)
int resample_design(const char* who_, int orig, int rate, int lpw, double rolloff, ResampleDesign* out) {
    const std::string who = who_;
    if (orig < 1 || rate < 1) return fail(DN_ERR_INVALID, who + ": rates must be positive");
    if (orig == rate) return fail(DN_ERR_INVALID, who + ": equal rates need no resampler (torchaudio returns the input)");
    if (lpw < 1) return fail(DN_ERR_INVALID, who + ": lowpass_filter_width must be at least 1");
    if (!(rolloff > 0.0 && rolloff <= 1.0)) return fail(DN_ERR_INVALID, who + ": rolloff must be in (0, 1]");
    const int g = gcd(orig, rate), o = orig / g, n = rate / g;
    const std::string limits = "the kernels take reduced rates o, n <= " + std::to_string(kMaxRate) + " and tables n x taps <= " + std::to_string(kMaxTable) + " floats";
    if (o > kMaxRate || n > kMaxRate)
        return fail(DN_ERR_UNSUPPORTED, who + ": " + limits + " (got " + std::to_string(o) + " : " + std::to_string(n) + ")");
    const double base = (o < n ? o : n) * rolloff;
    const double w = ceil(lpw * (double)o / base);
    if (!((2.0 * w + o) * n <= (double)kMaxTable)) {          // (w may be huge, or infinite with a tiny rolloff: the taps are named only where they fit an integer)
        const double taps = 2.0 * w + o;
        return fail(DN_ERR_UNSUPPORTED, who + ": " + limits + " (got " + std::to_string(n) + " x " +
                                            (taps < 1e15 ? std::to_string((long long)taps) : std::string("more than 10^15")) + ")");
    }
    out->o = o; out->n = n; out->width = (int)w; out->KW = 2 * out->width + o;
    out->D = (out->width + o - 1) / o; out->H = out->D * o + out->width;
    out->base = base;
    return DN_OK;
}

// torchaudio's _get_sinc_resample_kernel with the Hann window, in double, rounded once: [n][KW]
std::vector<float> resample_hann_table(const ResampleDesign& g, int lpw) {
    const int o = g.o, n = g.n, width = g.width, KW = g.KW;
    const double base = g.base, scale = base / o;
    std::vector<float> k((size_t)n * KW);
    for (int p = 0; p < n; ++p)
        for (int j = 0; j < KW; ++j) {
            double t = (-(double)p / n + (double)(j - width) / o) * base;
            t = fmax(-(double)lpw, fmin((double)lpw, t));
            const double c = cos(t * PI / lpw / 2), window = c * c;
            t *= PI;
            const double sinc = t == 0.0 ? 1.0 : sin(t) / t;
            k[(size_t)p * KW + j] = (float)(sinc * (window * scale));
        }
    return k;
}

extern "C" {

int dn_resample_create(const dn_resample_cfg* cfg, const float* kernel, dn_resampler** out) {
    if (!cfg || !out) return fail(DN_ERR_INVALID, "dn_resample_create: null argument");
    ResampleDesign g;
    DN_TRY(resample_design("dn_resample_create", cfg->orig_freq, cfg->new_freq, cfg->lowpass_filter_width, cfg->rolloff, &g));
    std::unique_ptr<dn_resampler> r(new dn_resampler());
    r->cfg = *cfg;
    const int o = g.o, n = g.n;
    r->o = o; r->n = n; r->width = g.width; r->KW = g.KW; r->D = g.D; r->H = g.H;
    const size_t KW = (size_t)r->KW;
    r->kernel = kernel ? std::vector<float>(kernel, kernel + (size_t)n * KW) : resample_hann_table(g, cfg->lowpass_filter_width);
    r->small = g.small();
    size_t off;
    if (r->small) {
        off = r->arena.add(r->kernel);
    } else {          // tap-major, rows padded to an even number of phases: a lane loads the coefficients of its two phases as one pair
        r->np = (n + 1) & ~1;
        std::vector<float> t(KW * (size_t)r->np, 0.0f);
        for (int p = 0; p < n; ++p)
            for (size_t j = 0; j < KW; ++j) t[j * r->np + p] = r->kernel[(size_t)p * KW + j];
        off = r->arena.add(t);
    }
    const hipError_t e = r->arena.upload();
    if (e != hipSuccess) return fail(DN_ERR_HIP, std::string("resampler upload: ") + hipGetErrorString(e));
    r->table = r->arena.ptr<float>(off);
    *out = r.release();
    return DN_OK;
}

void dn_resample_destroy(dn_resampler* r) { delete r; }

int dn_resample_geometry(const dn_resampler* r, int32_t* o, int32_t* n, int32_t* width, int32_t* taps, int32_t* delay_blocks) {
    if (!r) return fail(DN_ERR_INVALID, "dn_resample_geometry: null handle");
    if (o) *o = r->o;
    if (n) *n = r->n;
    if (width) *width = r->width;
    if (taps) *taps = r->KW;
    if (delay_blocks) *delay_blocks = r->D;
    return DN_OK;
}

int dn_resample_get_kernel(const dn_resampler* r, float* kernel) {
    if (!r || !kernel) return fail(DN_ERR_INVALID, "dn_resample_get_kernel: null argument");
    memcpy(kernel, r->kernel.data(), r->kernel.size() * sizeof(float));
    return DN_OK;
}

int64_t dn_resample_out_len(const dn_resampler* r, int64_t L) {
    if (!r || L < 1 || L > (int64_t)1 << 40) return 0;
    return (L * r->n + r->o - 1) / r->o;
}

int dn_resample(const dn_resampler* r, const void* x, int32_t in_s16, void* y, int32_t out_s16, int32_t B, int64_t L, int64_t x_stride,
                int64_t y_stride, void* stream) {
    if (B == 0) return DN_OK;      // empty batch: nothing to do (pointers of empty tensors are null)
    if (!r || !x || !y) return fail(DN_ERR_INVALID, "dn_resample: null argument");
    if (B < 0 || L < 1) return fail(DN_ERR_INVALID, "dn_resample: needs B >= 0 rows of L >= 1 samples");
    const int64_t Ly = dn_resample_out_len(r, L);
    if (L > dn::kRsMaxLen || Ly > dn::kRsMaxLen) return fail(DN_ERR_INVALID, "dn_resample: a row is at most " + std::to_string(dn::kRsMaxLen) + " samples, in and out (tile the signal with dn_resample_push)");
    if (x_stride < L) return bad_rows("dn_resample", "x_stride", x_stride, L);
    if (y_stride < Ly) return bad_rows("dn_resample", "y_stride", y_stride, Ly);
    const long long nblk = (Ly + r->n - 1) / r->n;
    DN_TRY(check_grid("dn_resample", r, B, nblk));
    dn::ResampleArgs a{};
    common_args(r, x, in_s16, y, out_s16, B, x_stride, y_stride, a);
    a.Lx = (int)L; a.hist = nullptr; a.lead = r->width; a.Ly = (int)Ly; a.nblk = (int)nblk;
    dn::launch_resample(a, as_stream(stream));
    return check_launch("resample_kernel");
}

size_t dn_resample_state_bytes(const dn_resampler* r, int32_t B) { return !r || B < 1 ? 0 : (size_t)B * (size_t)r->H * sizeof(float); }

int dn_resample_push(const dn_resampler* r, float* state, const void* x, int32_t in_s16, void* y, int32_t out_s16, int32_t B, int64_t blocks,
                     int64_t x_stride, int64_t y_stride, void* stream) {
    if (B == 0) return DN_OK;
    // every argument is validated before the first launch, so a failed call leaves y and state untouched
    if (!r || !state || !x || !y) return fail(DN_ERR_INVALID, "dn_resample_push: null argument");
    if (B < 0 || blocks < 1) return fail(DN_ERR_INVALID, "dn_resample_push: needs B >= 0 streams and blocks >= 1");
    if (blocks > dn::kRsMaxLen / (r->o > r->n ? r->o : r->n))
        return fail(DN_ERR_INVALID, "dn_resample_push: a push is at most " + std::to_string(dn::kRsMaxLen) + " samples a stream, in and out");
    const int64_t Lx = blocks * r->o, Ly = blocks * r->n;
    if (x_stride < Lx) return bad_rows("dn_resample_push", "x_stride", x_stride, Lx);
    if (y_stride < Ly) return bad_rows("dn_resample_push", "y_stride", y_stride, Ly);
    DN_TRY(check_grid("dn_resample_push", r, B, blocks));
    dn::ResampleArgs a{};
    common_args(r, x, in_s16, y, out_s16, B, x_stride, y_stride, a);
    a.Lx = (int)Lx; a.hist = state; a.lead = r->H; a.Ly = (int)Ly; a.nblk = (int)blocks;
    dn::launch_resample(a, as_stream(stream));
    DN_TRY(check_launch("resample_kernel(push)"));
    // a second launch, not a second copy of the state: every workgroup of the first one has read the old state when this one starts
    dn::launch_resample_state(state, r->H, x, a.in_s16, x_stride, (int)Lx, B, as_stream(stream));
    return check_launch("resample_state_kernel");
}

}  // extern "C"
