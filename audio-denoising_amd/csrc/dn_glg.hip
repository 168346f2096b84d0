// dn_glg.hip -- Griffin-Lim on magnitudes [B][T][K] for any number of columns T >= 3 (the any-length / server path).
//
// torchaudio's arithmetic, as dn_gl_body.hpp states it:  X = init * mag, prev = 0;  every iteration  s = istft(X) (hop (T - 1) samples),
// reb = stft(s) (centred, reflect padded),  a = reb - mu prev,  prev = reb,  X = mag a rsq(|a|^2 + 1e-32);  then one more istft.
// Two forms that give THE SAME BITS:
//   WHOLE (T <= kGlgWholeMax): glg_whole_kernel.  One workgroup per stream, one wavefront per column, every iteration on chip.  Per lane the NP bin
//          pairs and the middle bin of mag, X and prev (as gl_body).  The rebuilt signal lives in LDS as T - 1 hop blocks, each as its two
//          addends: seg[0] block j = second half of column j, seg[1] block j = first half of column j + 1 (the first half of column 0 and the
//          second of column T - 1 fall outside the samples the istft trim keeps and are not stored).  The blocks ping-pong, so an iteration has
//          one workgroup barrier, and that one orders LDS only.
//   STEPS (any T): two launches an iteration -- istft_general_kernel (dn_general.hip, unchanged): X -> s in the workspace, then
//          glg_step_kernel: one wavefront per (stream, column) windows s, transforms, splits, updates and writes ITS column's X and prev in
//          place -- plus glg_init_kernel in front (X = init * mag, prev = 0) and one istft_general_kernel behind, into `wave`.  No column
//          writes what another reads within a launch: no halos, no second copy of X.
// Why they round alike.  Every value either form computes is formed by the same operations in the same order:
//   block addends  v * w * (1 / NC)                               (istft_general_kernel's expression)
//   signal sample  (seg[0][i] + seg[1][i]) * inv_env[i % hop]     (istft_general_kernel's; WHOLE forms it where a column reads it)
//   segment        sample x window[m], one ROUNDED product (cmul_elem: never contracted into the transform's first add)
//   update         glg_update below, spelled with fmaf
// and the transforms, the split and the merge are the shared inline-assembly bodies of dn_wavefft.hpp.  The window and 1/envelope are NOT folded
// into one table here: one multiply a sample is noise next to the transforms, and the envelope index of a reflected sample stays in plain sight.
// Reflections (L = hop (T - 1); column t, window sample n):
//   t = 0,     n < hop:   s[hop - n]            n = 0 reads s[hop], the first sample of block 1
//   t = T - 1, n >= hop:  s[L - 2 - (n - hop)]  n = 2 hop - 1 reads s[(T - 2) hop - 1], the last sample of block T - 3
// With T = 3 both land in blocks 0 and 1.  T >= 3 is what keeps every index in range (hop (T - 1) > n_fft / 2, torch.stft's own condition).
#include "dn_dispatch.hpp"
#include "dn_gl_body.hpp"
#include "dn_stft_body.hpp"

namespace dn {

__device__ __forceinline__ void glg_update(v2f reb, v2f& prev, v2f& x, float m, float mom) {
    const v2f a = mk2(fmaf(-mom, prev[0], reb[0]), fmaf(-mom, prev[1], reb[1]));
    prev = reb;
    const float inv = __builtin_amdgcn_rsqf(fmaf(a[0], a[0], fmaf(a[1], a[1], 1e-32f)));
    x = a * (inv * m);
}

// The initial phases of one bin pair: injected (as they are, or -- normalize -- the unit phasors of an arbitrary spectrum), or drawn.
struct GlgInit {
    const v2f* init;      // [B][T][K] complex, or null: draw
    int normalize;
    uint64_t seed, sid0;
};

// This lane's magnitudes and X = init * mag of column `col` of stream `b` (row = (b T + col) K), in pair order.
template <int NFFT>
__device__ __forceinline__ void glg_first_x(const GlgInit& gi, const float* __restrict__ mag, size_t b, int col, size_t row, int lane,
                                            float (&mlo)[Geo<NFFT>::kNP], float (&mhi)[Geo<NFFT>::kNP], float& mmid,
                                            v2f (&xlo)[Geo<NFFT>::kNP], v2f (&xhi)[Geo<NFFT>::kNP], v2f& xmid) {
    constexpr int kNP = Geo<NFFT>::kNP, kNC = Geo<NFFT>::kNC;
#pragma unroll
    for (int t = 0; t < kNP; ++t) {
        const int k = lane + 64 * t, kh = kNC - k;
        mlo[t] = mag[row + k];
        mhi[t] = mag[row + kh];
        v2f alo, ahi;
        if (gi.init != nullptr) {
            alo = gi.init[row + k];
            ahi = gi.init[row + kh];
            if (gi.normalize) { alo = unit_phasor(alo); ahi = unit_phasor(ahi); }
        } else {
            rand_angle_pair(gi.seed, gi.sid0 + b, col, k, alo, ahi);
        }
        xlo[t] = alo * mlo[t];
        xhi[t] = ahi * mhi[t];
    }
    mmid = mag[row + kNC / 2];
    v2f amid;
    if (gi.init != nullptr) {
        amid = gi.init[row + kNC / 2];
        if (gi.normalize) amid = unit_phasor(amid);
    } else {
        amid = rand_angle_mid(gi.seed, gi.sid0 + b, col, kNC);
    }
    xmid = amid * mmid;
}

// The windowed segment of column t of a T-column signal, as v[s] = (sample 2 m, sample 2 m + 1) x window, m = lane + 64 s.  `src.pair(i, e, a0, a1)`
// yields s[i], s[i + 1] (i even) and `src.one(i, e)` yields s[i]; e = i % hop, the envelope index, is passed along so that nobody divides.
template <int NFFT, typename SRC, typename WIN>
__device__ __forceinline__ void glg_segment(v2f (&v)[Geo<NFFT>::kNV], int t, int T, int lane, const SRC& src, const WIN& win) {
    constexpr int kNV = Geo<NFFT>::kNV, kNP = Geo<NFFT>::kNP, kHop = Geo<NFFT>::kHop;
    const int L = kHop * (T - 1);
#pragma unroll
    for (int s = 0; s < kNV; ++s) {
        const int m = lane + 64 * s;
        float a0, a1;
        if (s < kNP) {                       // window samples n0 = 2 m, n0 + 1 < hop: signal index (t - 1) hop + n
            const int n0 = 2 * m;
            if (t > 0) {
                src.pair((t - 1) * kHop + n0, n0, a0, a1);
            } else {                         // reflected: s[hop - n]
                a0 = src.one(kHop - n0, n0 == 0 ? 0 : kHop - n0);
                a1 = src.one(kHop - n0 - 1, kHop - n0 - 1);
            }
        } else {                             // window samples hop + n0, hop + n0 + 1: signal index t hop + n
            const int n0 = 2 * m - kHop;
            if (t < T - 1) {
                src.pair(t * kHop + n0, n0, a0, a1);
            } else {                         // reflected: s[2 L - 2 - (L + n)] = s[L - 2 - n]
                a0 = src.one(L - 2 - n0, kHop - 2 - n0);
                a1 = src.one(L - 3 - n0, n0 == kHop - 2 ? kHop - 1 : kHop - 3 - n0);
            }
        }
        v[s] = cmul_elem(mk2(a0, a1), win(s, m));
    }
}

constexpr int kGlgThreads = 64 * kGlgWholeMax;

template <int NFFT> struct GlgLds {
    using G = Geo<NFFT>;
    static constexpr bool kLean = gl_lean<NFFT>();
    static constexpr int kSig = (kGlgWholeMax - 1) * G::kHop;       // floats of one line of block addends
    v2f tile[kGlgWholeMax][G::kTile];                               // exchange tile of each column's transforms and hand-offs
    float seg[2][2][kSig];                                          // [ping-pong][0: second halves, 1: first halves][block j][n]
    float env[G::kHop];                                             // 1 / envelope (hop-periodic: the table's first half)
    v2f win[kLean ? G::kNC : 1];                                    // n_fft 1536: the window, and the radix-12 twiddles (as gl_body)
    v2f pd[kLean ? G::Fft::kPdTable : 1];
};
// 46,080 B at n_fft 512, 96,256 B at 1024, 162,304 B at 1536 (of 163,840)
static_assert(sizeof(GlgLds<512>) <= 160 * 1024 && sizeof(GlgLds<1024>) <= 160 * 1024 && sizeof(GlgLds<1536>) <= 160 * 1024, "the ping-pong fits the LDS of a CU");

template <int NFFT>
__global__ __launch_bounds__(kGlgThreads) void glg_whole_kernel(DspDev d, const float* __restrict__ mag, GlgInit gi, float* __restrict__ wave,
                                                                int T, int n_iter, float mom) {
    using G = Geo<NFFT>;
    constexpr int kNC = G::kNC, kHop = G::kHop, kBins = G::kBins, kNV = G::kNV, kNP = G::kNP;
    constexpr bool kLean = GlgLds<NFFT>::kLean;
    __shared__ GlgLds<NFFT> lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int t = __builtin_amdgcn_readfirstlane(tid >> 6);          // this wavefront's column
    const size_t b = blockIdx.x;
    v2f* mytile = lds.tile[t];
    const v2f* pd_t = kLean ? lds.pd : nullptr;

    typename G::Fft::Tw tw;
    G::Fft::template load<!kLean>(tw, reinterpret_cast<const v2f*>(d.twc), lane);
    if (kLean && t == 1) G::Fft::fill_pd(lds.pd, reinterpret_cast<const v2f*>(d.twc), lane);
    for (int n = tid; n < kHop; n += 64 * T) lds.env[n] = d.inv_env[n];
    v2f wkh[kNP], wreg[kLean ? 1 : kNV];
#pragma unroll
    for (int s = 0; s < kNP; ++s) wkh[s] = cscale(reinterpret_cast<const v2f*>(d.twr)[lane + 64 * s], 0.5f);
    if (kLean) {
        for (int m = tid; m < kNC; m += 64 * T) lds.win[m] = reinterpret_cast<const v2f*>(d.window)[m];
    } else {
#pragma unroll
        for (int s = 0; s < kNV; ++s) wreg[kLean ? 0 : s] = reinterpret_cast<const v2f*>(d.window)[lane + 64 * s];
    }
    auto win = [&](int s, int m) { return kLean ? lds.win[m] : wreg[kLean ? 0 : s]; };

    float mlo[kNP], mhi[kNP], mmid;
    v2f xlo[kNP], xhi[kNP], xmid, plo[kNP], phi[kNP], pmid;
    glg_first_x<NFFT>(gi, mag, b, t, (b * T + t) * kBins, lane, mlo, mhi, mmid, xlo, xhi, xmid);
#pragma unroll
    for (int s = 0; s < kNP; ++s) { plo[s] = mk2(0.0f, 0.0f); phi[s] = mk2(0.0f, 0.0f); }
    pmid = mk2(0.0f, 0.0f);
    __syncthreads();                                                 // the shared tables are complete

    struct Src {
        const float* s0; const float* s1; const float* env;
        __device__ __forceinline__ float one(int i, int e) const { return (s0[i] + s1[i]) * env[e]; }
        __device__ __forceinline__ void pair(int i, int e, float& a0, float& a1) const {
            const v2f p = *reinterpret_cast<const v2f*>(s0 + i), q = *reinterpret_cast<const v2f*>(s1 + i), r = *reinterpret_cast<const v2f*>(env + e);
            a0 = (p[0] + q[0]) * r[0];
            a1 = (p[1] + q[1]) * r[1];
        }
    };

    v2f v[kNV], rlo[kNP], rhi[kNP], rmid;
    for (int it = 0;; ++it) {
        // ---- istft of X: Hermitian merge, inverse transform, synthesis window / NC into the block addends
        irfft_merge_pairs<kNV>(xlo, xhi, xmid, wkh, lane, mytile, v);
        G::Fft::template run<true>(v, tw, mytile, lane, pd_t);
        float* s0 = lds.seg[it & 1][0];
        float* s1 = lds.seg[it & 1][1];
        if (t > 0) {                       // first half -> block t - 1
#pragma unroll
            for (int s = 0; s < kNP; ++s) {
                const int m = lane + 64 * s;
                *reinterpret_cast<v2f*>(s1 + (t - 1) * kHop + 2 * m) = v[s] * win(s, m) * (1.0f / (float)kNC);
            }
        }
        if (t < T - 1) {                   // second half -> block t
#pragma unroll
            for (int s = kNP; s < kNV; ++s) {
                const int m = lane + 64 * s;
                *reinterpret_cast<v2f*>(s0 + t * kHop + 2 * m - kHop) = v[s] * win(s, m) * (1.0f / (float)kNC);
            }
        }
        DN_LDS_BARRIER();
        if (it == n_iter) {                // the final istft: sum, divide by the envelope, store
            float* out = wave + b * (size_t)(T - 1) * kHop;
            for (int j = 0; j < T - 1; ++j)
                for (int n = tid; n < kHop; n += 64 * T) out[j * kHop + n] = (s0[j * kHop + n] + s1[j * kHop + n]) * lds.env[n];
            break;
        }
        // ---- stft of the rebuilt signal: this column's segment, transform, split, phase update
        glg_segment<NFFT>(v, t, T, lane, Src{s0, s1, lds.env}, win);
        G::Fft::template run<false>(v, tw, mytile, lane, pd_t);
        rfft_split_pairs<kNV>(v, wkh, lane, mytile, rlo, rhi, rmid);
#pragma unroll
        for (int s = 0; s < kNP; ++s) {
            glg_update(rlo[s], plo[s], xlo[s], mlo[s], mom);
            glg_update(rhi[s], phi[s], xhi[s], mhi[s], mom);
        }
        glg_update(rmid, pmid, xmid, mmid, mom);
    }
}

// ---- STEPS.  X and prev rows in the workspace are [B][T][K] complex, the layout of a spectrum.
template <int NFFT>
__global__ __launch_bounds__(64) void glg_init_kernel(const float* __restrict__ mag, GlgInit gi, int T, v2f* __restrict__ x, v2f* __restrict__ prev) {
    using G = Geo<NFFT>;
    constexpr int kNC = G::kNC, kBins = G::kBins, kNP = G::kNP;
    const int lane = threadIdx.x;
    const size_t blk = blockIdx.x;
    const size_t b = blk / T;
    const int t = (int)(blk - b * T);
    float mlo[kNP], mhi[kNP], mmid;
    v2f xlo[kNP], xhi[kNP], xmid;
    glg_first_x<NFFT>(gi, mag, b, t, blk * kBins, lane, mlo, mhi, mmid, xlo, xhi, xmid);
    v2f* xr = x + blk * kBins;
    v2f* pr = prev + blk * kBins;
#pragma unroll
    for (int s = 0; s < kNP; ++s) {
        const int k = lane + 64 * s;
        xr[k] = xlo[s]; xr[kNC - k] = xhi[s];
        pr[k] = mk2(0.0f, 0.0f); pr[kNC - k] = mk2(0.0f, 0.0f);
    }
    if (lane == 0) { xr[kNC / 2] = xmid; pr[kNC / 2] = mk2(0.0f, 0.0f); }
}

// One wavefront per (stream, column): segment of the rebuilt signal `sig` [B][hop (T - 1)] -> transform -> split -> update of this column's X, prev.
template <int NFFT>
__global__ __launch_bounds__(64) void glg_step_kernel(DspDev d, const float* __restrict__ mag, const float* __restrict__ sig, int T,
                                                      v2f* __restrict__ x, v2f* __restrict__ prev, float mom) {
    using G = Geo<NFFT>;
    constexpr int kNC = G::kNC, kHop = G::kHop, kBins = G::kBins, kNV = G::kNV, kNP = G::kNP;
    __shared__ v2f tile[G::kTile];
    const int lane = threadIdx.x;
    const size_t blk = blockIdx.x;
    const size_t b = blk / T;
    const int t = (int)(blk - b * T);
    typename G::Fft::Tw tw;
    G::Fft::load(tw, reinterpret_cast<const v2f*>(d.twc), lane);
    v2f wkh[kNP], v[kNV];
#pragma unroll
    for (int s = 0; s < kNP; ++s) wkh[s] = cscale(reinterpret_cast<const v2f*>(d.twr)[lane + 64 * s], 0.5f);
    struct Src {
        const float* s;
        __device__ __forceinline__ float one(int i, int) const { return s[i]; }
        __device__ __forceinline__ void pair(int i, int, float& a0, float& a1) const { a0 = s[i]; a1 = s[i + 1]; }
    };
    const v2f* wtab = reinterpret_cast<const v2f*>(d.window);
    glg_segment<NFFT>(v, t, T, lane, Src{sig + b * (size_t)(T - 1) * kHop}, [&](int, int m) { return wtab[m]; });
    G::Fft::template run<false>(v, tw, tile, lane);
    v2f rlo[kNP], rhi[kNP], rmid;
    rfft_split_pairs<kNV>(v, wkh, lane, tile, rlo, rhi, rmid);
    const float* mr = mag + blk * kBins;
    v2f* xr = x + blk * kBins;
    v2f* pr = prev + blk * kBins;
#pragma unroll
    for (int s = 0; s < kNP; ++s) {
        const int k = lane + 64 * s, kh = kNC - k;
        v2f p = pr[k], xn;
        glg_update(rlo[s], p, xn, mr[k], mom);
        pr[k] = p; xr[k] = xn;
        p = pr[kh];
        glg_update(rhi[s], p, xn, mr[kh], mom);
        pr[kh] = p; xr[kh] = xn;
    }
    if (lane == 0) {
        v2f p = pr[kNC / 2], xn;
        glg_update(rmid, p, xn, mr[kNC / 2], mom);
        pr[kNC / 2] = p; xr[kNC / 2] = xn;
    }
}

// The phases a launch with init_angles == NULL draws: [B][T][K] complex, column t of stream b from rand_angle_pair(seed, sid0 + b, t, m) -- the
// numbering of draw_phases_kernel (dn_griffinlim.hip), so columns 0..2 are what dn_griffinlim draws.
__global__ void glg_draw_kernel(float2* __restrict__ out, uint64_t seed, uint64_t sid0, int bins, int T) {
    const size_t b = blockIdx.x / T;
    const int col = (int)(blockIdx.x - b * T);
    const int nc = bins - 1;
    float2* row = out + (size_t)blockIdx.x * bins;
    for (int m = threadIdx.x; m <= nc / 2; m += blockDim.x) {
        v2f lo, hi;
        rand_angle_pair(seed, sid0 + b, col, m, lo, hi);
        row[m] = make_float2(lo[0], lo[1]);
        if (2 * m != nc) row[nc - m] = make_float2(hi[0], hi[1]);
    }
}

static GlgInit glg_init_of(const GlgArgs& a) { return GlgInit{reinterpret_cast<const v2f*>(a.init), a.normalize, a.seed, a.sid0}; }

void launch_glg_whole(const DspDev& d, const GlgArgs& a, hipStream_t st) {
    const GlgInit gi = glg_init_of(a);
    const dim3 grid(a.B), block(64 * a.T);
    with_nfft(d.n_fft, [&](auto n) { hipLaunchKernelGGL(glg_whole_kernel<decltype(n)::value>, grid, block, 0, st, d, a.mag, gi, a.wave, a.T, a.n_iter, a.mom); });
}

void launch_glg_steps(const DspDev& d, const GlgArgs& a, hipStream_t st) {
    const GlgInit gi = glg_init_of(a);
    const dim3 grid(a.B * a.T), block(64);
    v2f* x = reinterpret_cast<v2f*>(a.x);
    v2f* prev = reinterpret_cast<v2f*>(a.prev);
    with_nfft(d.n_fft, [&](auto n) {
        constexpr int kN = decltype(n)::value;
        hipLaunchKernelGGL(glg_init_kernel<kN>, grid, block, 0, st, a.mag, gi, a.T, x, prev);
        for (int it = 0; it < a.n_iter; ++it) {
            launch_istft_general(d, reinterpret_cast<const float*>(a.x), a.sig, a.B, a.T, st);
            hipLaunchKernelGGL(glg_step_kernel<kN>, grid, block, 0, st, d, a.mag, (const float*)a.sig, a.T, x, prev, a.mom);
        }
    });
    launch_istft_general(d, reinterpret_cast<const float*>(a.x), a.wave, a.B, a.T, st);
}

void launch_draw_phases_general(const DspDev& d, float* out, uint64_t seed, uint64_t sid0, int B, int T, hipStream_t st) {
    hipLaunchKernelGGL(glg_draw_kernel, dim3(B * T), dim3(256), 0, st, reinterpret_cast<float2*>(out), seed, sid0, d.n_fft / 2 + 1, T);
}

}  // namespace dn
