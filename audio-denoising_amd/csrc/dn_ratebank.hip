// dn_ratebank.hip -- rate banks (dn_ratebank_ingest, dn_ratebank_emit): the rate adapters on either side of a session pool's push, ONE launch a
// side for a list of sessions of different rates.
//
// One workgroup handles one listed row.  Row i carries (slot_i, rate_i); its rate's geometry (o : n, KW, H, blocks a hop) and table come from
// RateBankArgs, so they differ across the rows of a launch and are uniform within a workgroup: the dispatch on n and on the parity of o is a
// workgroup-uniform branch into rb_row<N, SKEW>.  The workgroup stages the row's table and [state[slot][:H] | x_i[:blocks o]] in LDS -- the tile of
// the small form of dn_resample.hip with the same layout (sample i at i + i / 32 for even o: the lanes' stride-o reads touch 32 different banks a
// half wave; plain for odd o) and the same staging (rs_stage: 16-byte loads of the row where it is aligned, element-wise at the edges) -- and
// every lane walks the taps of its blocks with rs_small_block, the chain of resample_small_kernel.  The outputs are therefore dn_resample_push's
// of the same stream, bit for bit.
//
// After the barrier behind the staging nobody reads state[slot] any more, and no other workgroup ever touches it (a slot is listed once), so the
// same workgroup writes the new state -- the last H samples of the tile, float32 -- without a second launch.  chunk_in >= H (checked when the bank
// is created), so the new state is the chunk's tail.
//
// A row at the plan's own rate (rate index -1) is the conversion copy of the PCM conventions (dn_pcm.hpp).  Nothing divides per output, no
// workgroup reads beyond its row's chunk_in or writes beyond its chunk_out.
#include "dn_resample_body.hpp"

namespace dn {

template <int N, bool SKEW, bool S16>
__device__ __forceinline__ void rb_row(const RateBankArgs& a, const RateBankRate& g, const void* xrow, void* yrow, float* srow, float* xs, float* ks) {
    const int tid = threadIdx.x;
    const int o = g.o, KW = g.KW, H = g.H, nq = g.blocks, chunk = nq * o;
    ResampleArgs v{};          // the row as the shared staging and store see it: lead = H samples of history, then the chunk
    v.lead = H; v.Lx = chunk; v.Ly = nq * N; v.out_s16 = a.out_s16;
    v.x_vec = reinterpret_cast<uintptr_t>(xrow) % (S16 ? 8 : 16) == 0;
    v.y_pair = reinterpret_cast<uintptr_t>(yrow) % (a.out_s16 ? 4 : 8) == 0;
    auto pos = [](int i) { return rs_pos<SKEW>(i); };
    const float* table = a.tables + g.table;
    for (int i = tid; i < N * KW; i += kRsThreads) ks[i] = table[i];
    rs_stage<S16>(xs, pos, v, xrow, srow, 0, H + chunk, tid, kRsThreads);
    __syncthreads();          // the tile is whole: the old state has been read
    for (int i = tid; i < H; i += kRsThreads) srow[i] = xs[pos(chunk + i)];
    for (int ql = tid; ql < nq; ql += kRsThreads) {
        float acc[N];
        rs_small_block<N, SKEW>(xs, ks, ql * o, KW, acc);
        const int m = ql * N;
        if (N == 1) rs_store2(v, yrow, m, acc[0], 0.0f, false);
        else
            for (int p = 0; p < N; p += 2) rs_store2(v, yrow, m + p, acc[p], p + 1 < N ? acc[p + 1] : 0.0f, p + 1 < N);
    }
}

template <bool SKEW, bool S16>
__device__ __forceinline__ void rb_by_n(const RateBankArgs& a, const RateBankRate& g, const void* xrow, void* yrow, float* srow, float* xs, float* ks) {
    switch (g.n) {
        case 1: rb_row<1, SKEW, S16>(a, g, xrow, yrow, srow, xs, ks); break;
        case 2: rb_row<2, SKEW, S16>(a, g, xrow, yrow, srow, xs, ks); break;
        case 3: rb_row<3, SKEW, S16>(a, g, xrow, yrow, srow, xs, ks); break;
        default: rb_row<4, SKEW, S16>(a, g, xrow, yrow, srow, xs, ks); break;
    }
}

template <bool S16>
__global__ __launch_bounds__(kRsThreads) void ratebank_kernel(RateBankArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[kRbTile + kRbTile / 32 + 1];
    __shared__ float ks[kRsSmallMaxTable];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int slot = a.rows[2 * row], rate = a.rows[2 * row + 1];
    const long long xat = (long long)row * a.x_stride, yat = (long long)row * a.y_stride;
    const void* xrow = S16 ? static_cast<const void*>(static_cast<const short*>(a.x) + xat) : static_cast<const void*>(static_cast<const float*>(a.x) + xat);
    void* yrow = a.out_s16 ? static_cast<void*>(static_cast<short*>(a.y) + yat) : static_cast<void*>(static_cast<float*>(a.y) + yat);
    if (rate < 0) {          // the plan's own rate: x / 32767 in, clip * 32767 truncate out
        for (int i = tid; i < a.copy; i += kRsThreads) {
            const float v = pcm_load(xrow, S16, i);
            if (a.out_s16) static_cast<short*>(yrow)[i] = pcm_s16(v);
            else static_cast<float*>(yrow)[i] = v;
        }
        return;
    }
    const RateBankRate& g = a.r[rate];
    float* srow = a.state + (size_t)slot * a.state_stride;
    if (g.o % 2 == 0) rb_by_n<true, S16>(a, g, xrow, yrow, srow, xs, ks);
    else rb_by_n<false, S16>(a, g, xrow, yrow, srow, xs, ks);
}

void launch_ratebank(const RateBankArgs& a, int n, hipStream_t st) {
    if (a.in_s16) hipLaunchKernelGGL(ratebank_kernel<true>, dim3(n), dim3(kRsThreads), 0, st, a);
    else hipLaunchKernelGGL(ratebank_kernel<false>, dim3(n), dim3(kRsThreads), 0, st, a);
}

}  // namespace dn
