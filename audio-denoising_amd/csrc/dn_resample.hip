// dn_resample.hip -- polyphase sinc resampling (dn_resample, dn_resample_push): torchaudio.transforms.Resample on the device, the transform the
// reference builds at utils.py:48-49 and replaces with librosa.resample at app.py:181.
//
// With o : n the reduced rate pair, output q n + p of a row is the dot product of phase p's KW taps with the KW input samples from q o - width on
// (dn_internal.hpp: ResampleArgs gives the row as a virtual input v, so a whole signal and a push of a stream are the same body).  One output is
// ONE chain acc = fmaf(k[p][j], v[q o + j], acc), j ascending from acc = 0, in every form below: that is what makes a push equal the whole-signal
// call, a zero-padded row equal the row alone and an impulse row equal a table column, bit for bit.
//
// Two forms, chosen when the handle is created:
//   small (n <= 4, o <= 8, n KW <= 512: 48 -> 16 kHz, 16 -> 48, 8 -> 16)   lanes along consecutive blocks q.  A workgroup stages the input of its
//       kRsTileQ blocks, aprons included, and the table in LDS; a lane walks the taps of its block with n accumulators.  The table reads are
//       broadcasts.  The x reads have stride o across lanes: odd o touches every ds_read_b32 bank (a/4 mod 32 within a 32-lane half) once; even o
//       would hit every o-th bank o times over (o = 2: 2-way, o = 4: 4-way, o = 8: 8-way), so for even o the tile is stored skewed, sample i at
//       i + i / 32 -- the lanes of a half then read 32 different banks again (o = 4: lane l reads bank (4 l + l / 8) mod 32).
//   general (44.1 <-> 48 kHz, 44.1 -> 16)   lanes along consecutive phases p of kRsGenBlocks blocks, two phases a lane.  The table is tap-major
//       [KW][np] in global memory (up to 2 MB: it lives in L2), so a tap's coefficients are one coalesced row of 8-byte loads, used for
//       kRsGenBlocks blocks each; for a fixed tap the x value is the same for every lane, an LDS broadcast out of the staged input of the tap chunk.
// Neither form divides per output: a workgroup finds its row and tile with divisions of its own index, once.
//
// int16 is converted at the load and at the store by the conventions of the hop path (dn_pcm.hpp).
#include <type_traits>

#include "dn_resample_body.hpp"

namespace dn {

constexpr int kRsGenTaps = 128;                                                         // general form: taps staged at a time
constexpr int kRsGenTile = (kRsGenBlocks - 1) * 1024 + kRsGenTaps;                      // samples of a staged chunk at most (o <= 1024)

__device__ __forceinline__ const void* rs_xrow(const ResampleArgs& a, int row) {
    const long long at = (long long)row * a.x_stride;
    return a.in_s16 ? static_cast<const void*>(static_cast<const short*>(a.x) + at) : static_cast<const void*>(static_cast<const float*>(a.x) + at);
}
__device__ __forceinline__ void* rs_yrow(const ResampleArgs& a, int row) {
    const long long at = (long long)row * a.y_stride;
    return a.out_s16 ? static_cast<void*>(static_cast<short*>(a.y) + at) : static_cast<void*>(static_cast<float*>(a.y) + at);
}

// ---- small ratios: workgroup = (row, tile of kRsTileQ blocks), lane = block
template <int N, bool SKEW, bool S16>
__global__ __launch_bounds__(kRsThreads) void resample_small_kernel(ResampleArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[kRsTileMax + kRsTileMax / 32 + 1];
    __shared__ float ks[kRsSmallMaxTable];
    const int tid = threadIdx.x;
    const int tiles = (a.nblk + kRsTileQ - 1) / kRsTileQ;
    const int row = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)row * (unsigned)tiles);
    const int q0 = tile * kRsTileQ, nq = min(kRsTileQ, a.nblk - q0);
    const int o = a.o, KW = a.KW;
    const void* xrow = rs_xrow(a, row);
    const float* hrow = a.hist ? a.hist + (size_t)row * a.lead : nullptr;
    auto pos = [](int i) { return rs_pos<SKEW>(i); };
    for (int i = tid; i < N * KW; i += kRsThreads) ks[i] = a.table[i];
    rs_stage<S16>(xs, pos, a, xrow, hrow, q0 * o, (nq - 1) * o + KW, tid, kRsThreads);
    __syncthreads();
    void* yrow = rs_yrow(a, row);
    for (int ql = tid; ql < nq; ql += kRsThreads) {
        float acc[N];
        rs_small_block<N, SKEW>(xs, ks, ql * o, KW, acc);
        const int m = (q0 + ql) * N;          // the block's first output; the last block of a whole signal may be partial
        if (N == 1) {
            if (m < a.Ly) rs_store2(a, yrow, m, acc[0], 0.0f, false);
        } else {
            for (int p = 0; p < N; p += 2)
                if (m + p < a.Ly) rs_store2(a, yrow, m + p, acc[p], p + 1 < N ? acc[p + 1] : 0.0f, p + 1 < N && m + p + 1 < a.Ly);
        }
    }
}

// ---- general ratios: workgroup = (row, kRsGenBlocks blocks, kRsGenPhases phases), lane = two consecutive phases
template <bool S16>
__global__ __launch_bounds__(kRsGenThreads) void resample_general_kernel(ResampleArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[kRsGenTile];
    const int tid = threadIdx.x;
    const int btiles = (a.nblk + kRsGenBlocks - 1) / kRsGenBlocks, ptiles = (a.np + kRsGenPhases - 1) / kRsGenPhases;
    const unsigned per_row = (unsigned)btiles * (unsigned)ptiles;
    const int row = (int)(blockIdx.x / per_row);
    const unsigned rest = blockIdx.x - (unsigned)row * per_row;
    const int bt = (int)(rest / (unsigned)ptiles), pt = (int)(rest - (unsigned)bt * (unsigned)ptiles);          // phase tiles of a block tile are neighbours: they share x
    const int q0 = bt * kRsGenBlocks;
    const int o = a.o, KW = a.KW, half = a.np / 2;
    const int lp = pt * kRsGenThreads + tid;          // the lane's phase pair: phases 2 lp, 2 lp + 1
    const bool active = lp < half;
    const void* xrow = rs_xrow(a, row);
    const float* hrow = a.hist ? a.hist + (size_t)row * a.lead : nullptr;
    const float2* tab = reinterpret_cast<const float2*>(a.table) + lp;
    auto pos = [](int i) { return i; };
    float acc[kRsGenBlocks][2];
    for (int r = 0; r < kRsGenBlocks; ++r) acc[r][0] = acc[r][1] = 0.0f;
    for (int c0 = 0; c0 < KW; c0 += kRsGenTaps) {
        const int jn = min(kRsGenTaps, KW - c0);
        __syncthreads();          // the chunk before has been read
        rs_stage<S16>(xs, pos, a, xrow, hrow, q0 * o + c0, (kRsGenBlocks - 1) * o + jn, tid, kRsGenThreads);
        __syncthreads();
        if (active) {
            for (int jj = 0; jj < jn; ++jj) {
                const float2 k = tab[(size_t)(c0 + jj) * half];
                for (int r = 0; r < kRsGenBlocks; ++r) {
                    const float xv = xs[r * o + jj];
                    acc[r][0] = fmaf(k.x, xv, acc[r][0]);
                    acc[r][1] = fmaf(k.y, xv, acc[r][1]);
                }
            }
        }
    }
    if (!active) return;
    void* yrow = rs_yrow(a, row);
    const int p = 2 * lp;
    for (int r = 0; r < kRsGenBlocks; ++r) {
        const int m = (q0 + r) * a.n + p;          // (blocks beyond the row's last: m >= Ly)
        if (q0 + r < a.nblk && m < a.Ly) rs_store2(a, yrow, m, acc[r][0], acc[r][1], p + 1 < a.n && m + 1 < a.Ly);
    }
}

// ---- the state of a push: the last H samples of [state | chunk].  A short chunk (Lc < H) shifts the state down by Lc: tile by tile in ascending
// order, a tile read whole before it is written (its source overlaps its destination; the sources of later tiles lie above everything written so
// far), then the chunk goes behind it.
template <bool S16>
__global__ __launch_bounds__(kRsThreads) void resample_state_kernel(float* state, int H, const void* x, long long x_stride, int Lc) {
    const int tid = threadIdx.x;
    float* srow = state + (size_t)blockIdx.x * H;
    const long long at = (long long)blockIdx.x * x_stride;
    auto chunk = [&](int k) { return pcm_load(x, S16, at + k); };
    const int keep = Lc < H ? H - Lc : 0;
    for (int t0 = 0; t0 < keep; t0 += kRsThreads) {
        const int i = t0 + tid;
        const float v = i < keep ? srow[i + Lc] : 0.0f;
        __syncthreads();
        if (i < keep) srow[i] = v;
    }
    for (int i = keep + tid; i < H; i += kRsThreads) srow[i] = chunk(Lc - H + i);
}

void launch_resample(const ResampleArgs& a, hipStream_t st) {
    const bool s16 = a.in_s16 != 0;
    if (a.small) {
        const unsigned grid = (unsigned)a.B * (unsigned)((a.nblk + kRsTileQ - 1) / kRsTileQ);
        auto go = [&](auto n, auto skew) {
            if (s16) hipLaunchKernelGGL((resample_small_kernel<decltype(n)::value, decltype(skew)::value, true>), dim3(grid), dim3(kRsThreads), 0, st, a);
            else hipLaunchKernelGGL((resample_small_kernel<decltype(n)::value, decltype(skew)::value, false>), dim3(grid), dim3(kRsThreads), 0, st, a);
        };
        auto by_skew = [&](auto n) {
            if (a.o % 2 == 0) go(n, std::true_type{});
            else go(n, std::false_type{});
        };
        switch (a.n) {
            case 1: by_skew(std::integral_constant<int, 1>{}); break;
            case 2: by_skew(std::integral_constant<int, 2>{}); break;
            case 3: by_skew(std::integral_constant<int, 3>{}); break;
            default: by_skew(std::integral_constant<int, 4>{}); break;
        }
        return;
    }
    const unsigned grid = (unsigned)a.B * (unsigned)((a.nblk + kRsGenBlocks - 1) / kRsGenBlocks) * (unsigned)((a.np + kRsGenPhases - 1) / kRsGenPhases);
    if (s16) hipLaunchKernelGGL(resample_general_kernel<true>, dim3(grid), dim3(kRsGenThreads), 0, st, a);
    else hipLaunchKernelGGL(resample_general_kernel<false>, dim3(grid), dim3(kRsGenThreads), 0, st, a);
}

void launch_resample_state(float* state, int H, const void* x, int in_s16, long long x_stride, int Lc, int B, hipStream_t st) {
    if (in_s16) hipLaunchKernelGGL(resample_state_kernel<true>, dim3(B), dim3(kRsThreads), 0, st, state, H, x, x_stride, Lc);
    else hipLaunchKernelGGL(resample_state_kernel<false>, dim3(B), dim3(kRsThreads), 0, st, state, H, x, x_stride, Lc);
}

}  // namespace dn
