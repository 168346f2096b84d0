// dn_host.hpp -- private to the host layer (dn_api*.hip and the host half of dn_momo.hip): one owner per HIP resource, the shared
// helpers and the handle structs.  Host only: no kernel file includes it.
#pragma once
#include <string.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "dn_internal.hpp"

// ------------------------------------------------------------------ shared helpers (defined in dn_api.hip)
int fail(int code, const std::string& msg);       // sets the calling thread's dn_last_error(); callers build `msg` only on a failure path

#define DN_HIP(call)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) return fail(DN_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define DN_TRY(call) do { const int rc_ = (call); if (rc_ != DN_OK) return rc_; } while (0)      // for calls that have set the message themselves

int launch_failed(const char* what, hipError_t e);
inline int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DN_OK : launch_failed(what, e);
}
inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ------------------------------------------------------------------ owners: a std::unique_ptr with the resource's release call (move-only, one
// pointer, get() / swap() / reset() / explicit bool) and the call that creates the resource; a failed creation leaves the owner empty
struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
struct PinnedFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct StreamFree { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct EventFree { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };

template <typename T>
struct DevBuf : std::unique_ptr<T, DevFree> {       // device memory
    hipError_t alloc(size_t bytes) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) this->reset(static_cast<T*>(p));
        return e;
    }
    hipError_t alloc_zeroed(size_t bytes) {
        const hipError_t e = alloc(bytes);
        return e == hipSuccess ? hipMemset(this->get(), 0, bytes) : e;
    }
    hipError_t alloc_copy(const void* host, size_t bytes) {
        const hipError_t e = alloc(bytes);
        return e == hipSuccess ? hipMemcpy(this->get(), host, bytes, hipMemcpyHostToDevice) : e;
    }
};

template <typename T>
struct PinnedBuf : std::unique_ptr<T, PinnedFree> {  // page-locked host memory, mapped into the device's address space
    hipError_t alloc(size_t bytes) {
        void* p = nullptr;
        const hipError_t e = hipHostMalloc(&p, bytes, 0);
        if (e == hipSuccess) this->reset(static_cast<T*>(p));
        return e;
    }
    hipError_t device_view(T** out) const {  // the device's address of the buffer (the handle structs keep it beside the owner)
        void* dv = nullptr;
        const hipError_t e = hipHostGetDevicePointer(&dv, this->get(), 0);
        *out = static_cast<T*>(dv);
        return e;
    }
};

struct Stream : std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamFree> {
    hipError_t create(unsigned flags) {
        hipStream_t s{};
        const hipError_t e = hipStreamCreateWithFlags(&s, flags);
        if (e == hipSuccess) reset(s);
        return e;
    }
};

struct Event : std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventFree> {
    hipError_t create(unsigned flags) {
        hipEvent_t ev{};
        const hipError_t e = hipEventCreateWithFlags(&ev, flags);
        if (e == hipSuccess) reset(ev);
        return e;
    }
};

// A counted reference to a dn_model / dn_dsp (`std::atomic<int> refs`, created at 1: the creator's): retains on copy, releases on destruction;
// the last release deletes the handle.  dn_*_destroy drops the creator's reference with drop().
template <typename T>
class Ref {
public:
    Ref() = default;
    explicit Ref(const T* p) : p_(const_cast<T*>(p)) { if (p_) p_->refs.fetch_add(1); }
    Ref(const Ref& o) : Ref(o.p_) {}
    Ref& operator=(Ref o) noexcept { std::swap(p_, o.p_); return *this; }
    ~Ref() { drop(p_); }
    static void drop(T* p) { if (p && p->refs.fetch_sub(1) == 1) delete p; }
    T* get() const { return p_; }
    T* operator->() const { return p_; }
private:
    T* p_ = nullptr;
};

// One device allocation holding several arrays, 256-byte aligned slots.
struct DevArena {
    DevBuf<char> base;
    std::vector<char> host;
    template <typename T>
    size_t add(const std::vector<T>& v) {
        const size_t off = (host.size() + 255) & ~size_t(255), bytes = v.size() * sizeof(T);
        host.resize(off + bytes);
        memcpy(host.data() + off, v.data(), bytes);
        return off;
    }
    hipError_t upload() {
        host.resize(host.size() + dn::kArenaSlack);     // zeros: kernels that move whole rounds of an array read past its end (dn_cell_body.hpp)
        const hipError_t e = base.alloc_copy(host.data(), host.size());
        host.clear();
        host.shrink_to_fit();
        return e;
    }
    template <typename T>
    const T* ptr(size_t off) const { return reinterpret_cast<const T*>(base.get() + off); }
};

// ------------------------------------------------------------------ handles
struct BiasSet {
    DevArena arena;
    dn::CellDev view;
    DevBuf<dn::CellDev> view_dev;         // the same view in device memory (group_kernel reads its pointers where it needs them: no kernel-argument copy)
};

struct dn_model {
    std::atomic<int> refs{1};  // the creator's reference + one per dn_pipe / dn_sessions bound to it (dn_model_destroy only drops the creator's)
    dn_model_cfg cfg;
    std::vector<float> w;      // the caller's flat state_dict
    DevArena packed;           // MFMA weight fragments (fp32 and bf16), recurrent and last-level weights
    size_t off_down[4], off_gh, off_up[4];
    size_t offb_down[4], offb_up[3];
    mutable std::mutex mu;
    mutable std::map<int, std::unique_ptr<BiasSet>> bias;   // per number of compressed bins C (built on first use: build_bias)
};

struct dn_dsp {
    std::atomic<int> refs{1};
    dn_dsp_cfg cfg;
    DevArena arena;
    dn::DspDev view;
    DevBuf<dn::DspDev> view_dev;           // the same view in device memory (group_kernel)
    std::vector<float> fb, pinv, window;   // host copies [K][M], [K][M], [N]
};

// host-buffer transport of a streaming pipe (dn_pipe_stream_push_host): two copy queues beside the caller's compute stream, device staging
// double-buffered, everything ordered by events on the device -- the host never blocks inside a push
struct HostIo {
    static constexpr int kRing = 4;           // pushes whose events are kept (the host may run this far ahead of the result it waits for)
    Stream h2d, d2h;                          // (declared first: destroyed after the events and buffers that were used on them)
    Event ev_h2d[kRing], ev_k[kRing], ev_d2h[kRing];
    DevBuf<void> d_in[2], d_out[2];
    unsigned long long pushes = 0;
    // zero copy: the launch itself publishes "push n is in host memory" in this page-locked word (no HIP event, no barrier packet between hops)
    PinnedBuf<unsigned long long> done_host;
    unsigned long long* done_dev = nullptr;
    bool last_zero_copy[kRing] = {};               // pushes whose completion is published there (the others: ev_d2h)
    // DN_HOST_DEFER: the emitted hop of the newest push waits in z_out[ticket & 1] until the next launch (or dn_pipe_stream_host_wait) moves it out
    DevBuf<void> z_out[2];
    bool defer_pending = false;
    unsigned long long defer_ticket = 0;
    void* defer_dst = nullptr;                     // device view of that push's hop_out_host
    size_t defer_bytes = 0;
    hipStream_t defer_stream = nullptr;
};

struct dn_pipe {
    Ref<dn_model> m;                          // the pipe keeps the packed weights and the plan alive (its launches read their device arenas);
    Ref<dn_dsp> d;                            // declared first: released after everything below
    std::unique_ptr<HostIo> hio;
    int B = 0, C = 0;
    bool bf16 = false;                        // DN_CONV_BF16: bf16 MFMA conv tiles in the front half
    bool phase_in = false;                    // DN_PHASE_FROM_INPUT: every frame's chain starts from the unit phasors of its analysis STFT (scratch_init exists from create on)
    DevBuf<dn::PipeCtl> ctl;                  // device-resident hop counter / pending flag (what makes a captured launch replayable)
    // scratch slots, used round robin by consecutive frames: depth + 1 of them (a frame's slot is read by every segment of its chain)
    int depth = 1, n_slots = 2;                     // hops of one stream in flight (dn_pipe_set_depth)
    DevBuf<float> scratch;                          // [n_slots] x { mel [B][3][M], residual [B][3][M], peak [B], meta [B][kSlotMeta], lin [B][3][K] }
    DevBuf<float2> scratch_init;                    // [n_slots] x the frame's initial phases [B][3][K] complex (allocated on first parity-mode use)
    DevBuf<float2> gl_state;                        // [n_slots] x a parked Griffin-Lim chain ([B][3][2 NV + 2][64] complex: head start, chain segments)
    size_t slot_floats = 0, init_elems = 0, state_elems = 0;
    int group = 0;                                  // hop groups (dn_pipe_set_group): hops a launch carries, 0 = single hops
    unsigned long long group_pushes = 0;            // hops pushed into a streaming group pipe by this host (priming bookkeeping of *hops_valid)
    int group_pending = 0;                          // frames the last group push fronted, as far as this host's own calls tell
    int gl_split = 0;                               // iterations of head start (0 = none)
    int gl_schedule = DN_GL_AUTO;                   // Griffin-Lim schedule of the back half (dn_pipe_set_gl_schedule)
    int split = DN_SPLIT_AUTO;                      // a hop as two launches, chains then front halves (dn_pipe_set_split)
    const BiasSet* bs = nullptr;
    bool submitted = false;                   // frame mode: a hop may be pending (its destination travels in the slot, not here)
    // streaming mode: per-stream state owned by the pipe
    DevBuf<float> ring;                       // [B][n_fft] last n_fft input samples
    DevBuf<float> ola;                        // [B][n_fft] output overlap-add line
    DevBuf<float> hx;                         // [B][17][C]
};

struct dn_sessions {
    Ref<dn_model> m;
    Ref<dn_dsp> d;
    const BiasSet* bs = nullptr;
    int cap = 0, C = 0;
    bool bf16 = false;
    int schedule = DN_SESS_AUTO;
    // per-slot state [cap][...], and the per-row workspace of a push (rows in list order)
    DevBuf<float> ring, ola, hx;
    DevBuf<unsigned long long> counters;      // frames [cap] | stream ids [cap] | pushes [cap] (u32)
    DevBuf<float> ws;                         // mel [cap][3][M] | residual [cap][3][M] | lin [cap][3][K] | peak [cap] | meta [cap][kSessMeta]
    DevBuf<float> phas;                       // DN_PHASE_FROM_INPUT: phasor rows [cap][3][K] complex of a push (list order), else empty
    std::vector<char> open;                   // host bookkeeping: which slots are open
    // the id lists (and the stream ids of an open) on their way to the kernels: kRing entries of a page-locked staging ring, entry k reused only
    // after the event recorded behind the last launch that read it has completed
    static constexpr int kRing = 4;
    PinnedBuf<char> stage_host;
    DevBuf<char> stage_ring;                  // the device ring of a DN_SESS_IDS_COPY build; empty otherwise
    char* stage_dev = nullptr;                // the device's view of the entries: stage_ring, or the pinned ring's mapping
    size_t stage_bytes = 0;                   // one entry: ids [cap] i32, then stream ids [cap] u64 (8-byte aligned)
    Event ev[kRing];
    bool ev_live[kRing] = {};
    unsigned long long calls = 0;
    std::vector<char> seen;                   // scratch of the duplicate check
    // dn_sessions_import: the header check of each record [cap] u32, written by the device into page-locked memory, read after one synchronisation
    PinnedBuf<uint32_t> chk_host;
    uint32_t* chk_dev = nullptr;
};

struct dn_resampler {
    dn_resample_cfg cfg;
    int o = 0, n = 0, width = 0, KW = 0, D = 0, H = 0;     // reduced rates; taps 2 width + o; delay blocks ceil(width / o); history D o + width
    bool small = false;                       // the block-per-lane kernel (dn_resample.hip), else the phase-per-lane one
    int np = 0;                               // general form: phases of a device table row (n rounded up to even)
    std::vector<float> kernel;                // host copy [n][KW], what dn_resample_get_kernel returns
    DevArena arena;                           // the table as the handle's kernel form reads it
    const float* table = nullptr;
};

// A page-locked staging ring for small host lists that kernels read straight from host memory: kRing entries of `entry` bytes, entry k handed out
// again only after the event recorded behind the last launch that read it has completed (the discipline of dn_sessions' id lists).
struct StageRing {
    static constexpr int kRing = 4;
    PinnedBuf<char> host;
    char* dev = nullptr;                      // the device's view of the entries
    size_t entry = 0;
    Event ev[kRing];
    bool live[kRing] = {};
    unsigned long long calls = 0;
    hipError_t create(size_t entry_bytes) {
        entry = (entry_bytes + 255) & ~size_t(255);
        hipError_t e = host.alloc(kRing * entry);
        if (e == hipSuccess) e = host.device_view(&dev);
        for (int k = 0; k < kRing && e == hipSuccess; ++k) { e = ev[k].create(hipEventDisableTiming); live[k] = false; }
        return e;
    }
    // the next entry, free again: *h to fill on the host, *d what the launch reads
    hipError_t next(char** h, const char** d) {
        const int k = (int)(calls % kRing);
        if (live[k]) { const hipError_t e = hipEventSynchronize(ev[k].get()); if (e != hipSuccess) return e; }
        *h = host.get() + (size_t)k * entry;
        *d = dev + (size_t)k * entry;
        return hipSuccess;
    }
    // behind the launch that read the entry next() gave
    hipError_t staged(hipStream_t st) {
        const int k = (int)(calls % kRing);
        const hipError_t e = hipEventRecord(ev[k].get(), st);
        if (e == hipSuccess) { live[k] = true; ++calls; }
        return e;
    }
    void drain() {                            // the launches that read the ring finish before it goes
        for (int k = 0; k < kRing; ++k)
            if (live[k]) (void)hipEventSynchronize(ev[k].get());
    }
};

struct dn_ratebank {
    dn_ratebank_cfg cfg;
    int n_rates = 0;
    dn::RateBankRate side[2][dn::kRbMaxRates];     // [0]: down (session rate -> plan, ingest), [1]: up (plan -> session rate, emit)
    int D[2][dn::kRbMaxRates];                     // delay blocks of each table
    int stride[2] = {0, 0};                        // floats a slot of each side's state: the largest H, rounded up to 4
    DevArena arena;                                // every table, [n][KW] each
    const float* tables = nullptr;
    StageRing ring;                                // the (slot, rate index) pairs of a call
    size_t ring_rows = 0;                          // rows an entry holds (grown on demand)
    std::vector<char> seen;                        // scratch of the duplicate check
};

// ------------------------------------------------------------------ shared between the units
// dn_api_resample.hip: the geometry of a rate pair (refusals as dn_resample_create's, under the caller's name) and its Hann table [n][KW]
struct ResampleDesign {
    int o, n, width, KW, D, H;
    double base;
    bool small() const { return n <= dn::kRsSmallMaxN && o <= dn::kRsSmallMaxO && (size_t)n * KW <= (size_t)dn::kRsSmallMaxTable; }
};
int resample_design(const char* who, int orig, int rate, int lpw, double rolloff, ResampleDesign* out);
std::vector<float> resample_hann_table(const ResampleDesign& g, int lpw);

constexpr uint32_t kHopFlags = DN_CONV_BF16 | DN_PHASE_FROM_INPUT;      // the flag bits of a hop, a pipe and a pool

// dn_api_model.hip: the bias tables of a model for C compressed bins, built and cached on first use
int build_bias(const dn_model* m, int C, const BiasSet** out);
// dn_api.hip
int bad_momentum();
inline int check_momentum(float momentum, float* mapped) {      // refuses what is outside [0, 1); *mapped (unless null) = m / (1 + m), what the kernels take
    if (!(momentum >= 0.0f && momentum < 1.0f)) return bad_momentum();
    if (mapped) *mapped = momentum / (1.0f + momentum);
    return DN_OK;
}
// what every hop, pipe and pool checks of its handles, sizes, momentum (*mom as check_momentum's) and flags, in that order
int check_hop_args(const char* who, const dn_model* m, const dn_dsp* d, int32_t B, int32_t n_iter, float momentum, uint32_t flags, float* mom = nullptr);
int refuse_not_1024(const std::string& what);           // DN_ERR_UNSUPPORTED: "<what> is built for n_fft 1024 (at 1536 ...; at 512 ...)"
size_t phasor_bytes(const dn_dsp* d, size_t frames);    // the phasor rows of input-phase mode: 3 K complex values a frame
