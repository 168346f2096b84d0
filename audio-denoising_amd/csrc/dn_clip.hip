// dn_clip.hip -- clip mode's call (launch_clip) and the kernels that belong to this unit alone (dn_clip_kernels.hpp: the launches of a call, the
// workspace, the two units).
#include "dn_clip_kernels.hpp"

namespace dn {

// ---- 3b. n_fft 1024, in front of the wavefront-per-frame chains: P8-P10 of frame f into its frame row (the samples are not needed any more)
__global__ __launch_bounds__(kHopPipeThreads) void clip_invmel_kernel(DspDev d, ClipArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[kInvSmem];
    const size_t f = blockIdx.x;
    const size_t M3 = 3 * (size_t)d.n_mels;
    invmel_body<1024, true, kHopPipeThreads>(smem, d, a.mel + f * M3, a.diff + f * M3, a.fr + f * a.fr_stride, 3, 0, threadIdx.x);
}

// ---- 4. fold: the overlap-add across hops.  E_i = frame row of hop i (frame x 1/envelope), s_i its peak, lo = [:hop], hi = [hop:]:
//   out_0 = ola_in.lo     out_1 = fma(E_0.lo, s_0, ola_in.hi)     out_i = fma(E_{i-1}.lo, s_{i-1}, fma(E_{i-2}.hi, s_{i-2}, 0))
//   ola.lo = fma(E_{N-1}.lo, s_{N-1}, h), h = fma(E_{N-2}.hi, s_{N-2}, 0) (N = 1: ola_in.hi)     ola.hi = fma(E_{N-1}.hi, s_{N-1}, 0)
// which is what N applications of the epilogue of gl_body<.., STREAM> leave, operation for operation.  A thread owns one sample pair of one job
// of one stream; job 0 is everything that touches the stream's overlap-add line (out_0, out_1, the new line: the pair's old samples are in
// registers before the thread rewrites them, and no other thread reads them), job j >= 1 is out_{j+1}.
constexpr int kClipFoldThreads = 256;
// A ragged call (a.off non-null) has one job per frame instead, found from off alone: thread u owns pair u % pairs of frame f = u / pairs, hop i of
// the stream b that owns f (clip_owner; f differs within a workgroup here, so these loads are per lane).  Frame 0 of a stream is its job 0, frame i
// in 1 .. N_b - 2 is job i (out_{i+1}), and the stream's last frame idles when N_b > 1.  The jobs themselves are the ones below, N = N_b.
__global__ __launch_bounds__(kClipFoldThreads) void clip_fold_kernel(ClipArgs a) {
    const int hop = a.n_fft / 2, pairs = hop / 2;
    const size_t u = (size_t)blockIdx.x * kClipFoldThreads + threadIdx.x;
    const int m = (int)(u % pairs);
    size_t b, j, f0;
    int N;
    if (a.off != nullptr) {
        const size_t f = u / pairs;
        if (f >= a.frames) return;
        const int o = clip_owner(a.off, a.B, (int)f);
        b = (size_t)o; f0 = (size_t)a.off[o]; j = f - f0; N = a.off[o + 1] - a.off[o];
        if (j != 0 && j + 1 >= (size_t)N) return;          // the last frame of a stream with more than one
    } else {
        const size_t jobs = a.N > 1 ? (size_t)a.N - 1 : 1;
        if (u >= (size_t)a.B * jobs * pairs) return;
        const size_t bj = u / pairs;
        b = bj / jobs; j = bj - b * jobs; f0 = b * (size_t)a.N; N = a.N;
    }
    const int n = 2 * m;
    auto pair = [&](size_t i, int off) { return *reinterpret_cast<const v2f*>(a.fr + (f0 + i) * a.fr_stride + off + n); };
    const v2f zero = mk2(0.0f, 0.0f);
    const size_t out0 = f0 * hop + n;          // the pair in hop 0 of the stream's output row
    if (j == 0) {
        float* orow = a.ola + b * (size_t)a.n_fft;
        const v2f lo = *reinterpret_cast<const v2f*>(orow + n), hi = *reinterpret_cast<const v2f*>(orow + hop + n);
        pcm_store_pair(a.hops_out, a.out_s16, out0, lo);
        const v2f first = ola_term(pair(0, 0), a.peak[f0], hi);          // hop 0's frame on the old line
        v2f nlo = first;
        if (N > 1) {
            pcm_store_pair(a.hops_out, a.out_s16, out0 + hop, first);
            const size_t l = (size_t)N - 1;
            nlo = ola_term(pair(l, 0), a.peak[f0 + l], ola_term(pair(l - 1, hop), a.peak[f0 + l - 1], zero));
        }
        const size_t l = (size_t)N - 1;
        const v2f nhi = ola_term(pair(l, hop), a.peak[f0 + l], zero);
        *reinterpret_cast<v2f*>(orow + n) = nlo;
        *reinterpret_cast<v2f*>(orow + hop + n) = nhi;
    } else {
        const size_t i = j + 1;
        pcm_store_pair(a.hops_out, a.out_s16, out0 + i * hop, ola_term(pair(i - 1, 0), a.peak[f0 + i - 1], ola_term(pair(i - 2, hop), a.peak[f0 + i - 2], zero)));
    }
}

void launch_clip(const DspDev& d, const CellDev* c_dev, const ClipArgs& args, bool bf16, hipStream_t st) {
    ClipArgs a = args;
    if (a.phas != nullptr) a.init = a.phas;          // input-phase mode: the chains start from the phasors the analysis stores
    const dim3 frames((unsigned)a.frames), block(kHopPipeThreads);
    with_nfft(d.n_fft, [&](auto n) {
        constexpr int kN = decltype(n)::value;
        with_bool(a.phas != nullptr, [&](auto phin) {
            hipLaunchKernelGGL((clip_analysis_kernel<kN, decltype(phin)::value>), frames, block, 0, st, d, a);
        });
        with_model<kN>(bf16, a.C, [&](auto bf, auto ct) {
            hipLaunchKernelGGL((clip_model_kernel<decltype(bf)::value, decltype(ct)::value>), dim3(a.B), block, 0, st, c_dev, a);
        });
        if (a.per_stream) {
            hipLaunchKernelGGL(clip_invmel_kernel, frames, block, 0, st, d, a);
            launch_clip_chains_glw(d, a, st);
        } else {
            hipLaunchKernelGGL(clip_chain_kernel<kN>, frames, dim3(kHopThreads), 0, st, d, a);
        }
    });
    const size_t jobs = a.N > 1 ? (size_t)a.N - 1 : 1;
    const size_t units = (a.off != nullptr ? a.frames : (size_t)a.B * jobs) * (a.n_fft / 4);          // ragged: a job per frame
    hipLaunchKernelGGL(clip_fold_kernel, dim3((unsigned)((units + kClipFoldThreads - 1) / kClipFoldThreads)), dim3(kClipFoldThreads), 0, st, a);
}

}  // namespace dn

