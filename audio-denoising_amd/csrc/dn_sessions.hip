// dn_sessions.hip -- the session pool's dispatch over its units (dn_sess_kernels.hpp: the schedules, which unit holds what), the n_fft-1024
// one-launch instantiations (max-ILP scheduling, Makefile) and the open and record kernels.
#include "dn_sess_kernels.hpp"

namespace dn {

void launch_sess_frame_unit(Size<1024>, const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in) {
    launch_sess_frame_of<1024>(d, c, a, bf16, st, phase_in);
}

void launch_sess_frame(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in) {
    with_nfft(d.n_fft, [&](auto n) { launch_sess_frame_unit(n, d, c, a, bf16, st, phase_in); });
}

// (re)open: slot ids[i] gets a zero ring, overlap-add line and hx, zero counters and the stream id sids_in[i]
__global__ void sess_open_kernel(SessArgs a, const uint64_t* sids_in, int n_fft) {
    const size_t s = (size_t)a.ids[blockIdx.x];
    for (int k = threadIdx.x; k < n_fft; k += blockDim.x) {
        a.ring[s * n_fft + k] = 0.0f;
        a.ola[s * n_fft + k] = 0.0f;
    }
    for (int k = threadIdx.x; k < kHidden * a.C; k += blockDim.x) a.hx[s * kHidden * a.C + k] = 0.0f;
    if (threadIdx.x == 0) {
        a.frames[s] = 0;
        a.pushes[s] = 0;
        a.sids[s] = sids_in[blockIdx.x];
    }
}
void launch_sess_open(const SessArgs& a, const uint64_t* sids_in, int n_fft, hipStream_t st) {
    hipLaunchKernelGGL(sess_open_kernel, dim3(a.n), dim3(256), 0, st, a, sids_in, n_fft);
}

// ---- session records (dn_sessions_export / dn_sessions_import).  Workgroup i moves the record of row i: slot ids[i] <-> records + i * stride.
// The lines go 16 bytes a lane (n_fft % 4 == 0, the pool's lines and the records 16-byte aligned); hx is [17][C] at a slot stride of 68 C bytes,
// not 16-byte aligned, so it goes a float a lane.  Header and counters are plain stores of thread 0.
constexpr int kSessRecThreads = 256;

// export: the slot's state into its record; the pool is only read
__global__ __launch_bounds__(kSessRecThreads) void sess_export_kernel(SessArgs a, SessRec r, int n_fft, char* records) {
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    const size_t s = (size_t)a.ids[i];
    char* rec = records + i * r.stride;
    const float4* ring = reinterpret_cast<const float4*>(a.ring + s * n_fft);
    const float4* ola = reinterpret_cast<const float4*>(a.ola + s * n_fft);
    float4* ring_r = reinterpret_cast<float4*>(rec + kSessRecHead);
    float4* ola_r = reinterpret_cast<float4*>(rec + r.ola_off);
    for (int k = tid; k < n_fft / 4; k += kSessRecThreads) {
        ring_r[k] = ring[k];
        ola_r[k] = ola[k];
    }
    const int nh = kHidden * a.C;
    const float* hx = a.hx + s * nh;
    float* hx_r = reinterpret_cast<float*>(rec + r.hx_off);
    for (int k = tid; k < nh; k += kSessRecThreads) hx_r[k] = hx[k];
    // the padding behind hx is zero: a record's bytes are a function of the session's state alone
    uint32_t* tail = reinterpret_cast<uint32_t*>(rec);
    for (size_t k = (r.hx_off + 4 * (size_t)nh) / 4 + tid; k < r.stride / 4; k += kSessRecThreads) tail[k] = 0u;
    if (tid == 0) {
        dn_session_record_header h = r.want;
        h.pushes = a.pushes[s];
        h.reserved0 = 0;
        h.frames = a.frames[s];
        h.stream_id = a.sids[s];
        h.reserved1 = 0;
        *reinterpret_cast<dn_session_record_header*>(rec) = h;
    }
}

// check: thread i compares record i's header with the pool's and leaves 0 or the first fault in status[i] (page-locked: the host reads it
// after one synchronisation)
__global__ __launch_bounds__(kSessRecThreads) void sess_check_kernel(SessRec r, int n, const char* records, uint32_t* status) {
    const size_t i = (size_t)blockIdx.x * kSessRecThreads + threadIdx.x;
    if (i >= (size_t)n) return;
    const uint4* hv = reinterpret_cast<const uint4*>(records + i * r.stride);
    const uint4 w0 = hv[0], w1 = hv[1], w2 = hv[2];              // magic version sr n_fft | hop n_mels hidden C | pushes ...
    uint32_t bad = 0;
    if (w0.x != r.want.magic) bad = kSessRecBadMagic;
    else if (w0.y != r.want.version) bad = kSessRecBadVersion;
    else if (w0.z != r.want.sample_rate || w0.w != r.want.n_fft || w1.x != r.want.hop || w1.y != r.want.n_mels || w1.z != r.want.hidden ||
             w1.w != r.want.C) bad = kSessRecBadGeometry;
    else if (w2.x > r.prime) bad = kSessRecBadPushes;
    status[i] = bad;
}

// import: record i's state into slot ids[i] (sids_in: the caller's stream ids, or null: the recorded ones)
__global__ __launch_bounds__(kSessRecThreads) void sess_import_kernel(SessArgs a, SessRec r, int n_fft, const char* records, const uint64_t* sids_in) {
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    const size_t s = (size_t)a.ids[i];
    const char* rec = records + i * r.stride;
    const float4* ring_r = reinterpret_cast<const float4*>(rec + kSessRecHead);
    const float4* ola_r = reinterpret_cast<const float4*>(rec + r.ola_off);
    float4* ring = reinterpret_cast<float4*>(a.ring + s * n_fft);
    float4* ola = reinterpret_cast<float4*>(a.ola + s * n_fft);
    for (int k = tid; k < n_fft / 4; k += kSessRecThreads) {
        ring[k] = ring_r[k];
        ola[k] = ola_r[k];
    }
    const int nh = kHidden * a.C;
    const float* hx_r = reinterpret_cast<const float*>(rec + r.hx_off);
    float* hx = a.hx + s * nh;
    for (int k = tid; k < nh; k += kSessRecThreads) hx[k] = hx_r[k];
    if (tid == 0) {
        const dn_session_record_header* h = reinterpret_cast<const dn_session_record_header*>(rec);
        a.pushes[s] = h->pushes;
        a.frames[s] = h->frames;
        a.sids[s] = sids_in != nullptr ? sids_in[i] : h->stream_id;
    }
}

void launch_sess_export(const SessArgs& a, const SessRec& r, int n_fft, void* records, hipStream_t st) {
    hipLaunchKernelGGL(sess_export_kernel, dim3(a.n), dim3(kSessRecThreads), 0, st, a, r, n_fft, static_cast<char*>(records));
}
void launch_sess_check(const SessArgs& a, const SessRec& r, const void* records, uint32_t* status, hipStream_t st) {
    hipLaunchKernelGGL(sess_check_kernel, dim3((a.n + kSessRecThreads - 1) / kSessRecThreads), dim3(kSessRecThreads), 0, st, r, a.n,
                       static_cast<const char*>(records), status);
}
void launch_sess_import(const SessArgs& a, const SessRec& r, int n_fft, const void* records, const uint64_t* sids_in, hipStream_t st) {
    hipLaunchKernelGGL(sess_import_kernel, dim3(a.n), dim3(kSessRecThreads), 0, st, a, r, n_fft, static_cast<const char*>(records), sids_in);
}

}  // namespace dn
