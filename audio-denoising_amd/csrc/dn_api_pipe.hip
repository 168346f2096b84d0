// dn_api_pipe.hip -- dn_pipe: software-pipelined hops (frame mode, streaming mode, hop groups) and the host-buffer transport of a streaming
// pipe.  No kernel code here.
#include <thread>

#include "dn_host.hpp"

namespace {

// the head start a one-hop pipe runs with unless told otherwise (measured optima; n_fft 512 takes 1024's, not swept yet; none above 256 streams, none on a deep pipe)
int default_head_start(const dn_pipe* p) { return p->depth == 1 && p->B <= 256 ? (p->d->cfg.n_fft == 1536 ? 12 : 8) : 0; }

// Re-lays out the pipe for n_slots scratch slots (dn_pipe_set_depth, dn_pipe_set_group).  Nothing may be in flight: the device is drained and the
// control block read into `h`, which the caller uploads again once its own fields are set.  Everything new is allocated before anything old is given
// up: a failure leaves the pipe as it was.
int relayout(dn_pipe* p, const char* who, int n_slots, bool with_state, bool with_init, dn::PipeCtl& h) {
    DN_HIP(hipDeviceSynchronize());
    DN_HIP(hipMemcpy(&h, p->ctl.get(), sizeof(h), hipMemcpyDeviceToHost));
    if (h.pending != 0) return fail(DN_ERR_INVALID, std::string(who) + ": hops are in flight (flush first)");
    DevBuf<float> scratch;
    DevBuf<float2> state, init;
    hipError_t e = scratch.alloc(n_slots * p->slot_floats * sizeof(float));
    if (e == hipSuccess && with_state) e = state.alloc(n_slots * p->state_elems * sizeof(float2));
    if (e == hipSuccess && with_init) e = init.alloc(n_slots * p->init_elems * sizeof(float2));
    if (e != hipSuccess) return fail(DN_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    p->scratch.swap(scratch); p->gl_state.swap(state); p->scratch_init.swap(init);      // (the old ones go with the locals)
    p->n_slots = n_slots;
    p->gl_split = 0;                            // (a head start is set per depth: dn_pipe_set_head_start)
    h.slot_next = 0;
    return DN_OK;
}

// what a zero-copy host push adds to its launch (dn_pipe_stream_push_host)
struct HostCarry {
    unsigned long long* done; unsigned long long done_value;       // the launch publishes done_value in *done (null: it publishes nothing)
    const void* copy_src; void* copy_dst; size_t copy_bytes;       // the deferred output of the previous push, which the launch carries to the host (null: none)
};

}  // namespace

extern "C" {

int dn_pipe_create(const dn_model* m, const dn_dsp* d, int32_t B, uint32_t flags, dn_pipe** out) {
    if (!out) return fail(DN_ERR_INVALID, "dn_pipe_create: null argument");
    if (B <= 0) return fail(DN_ERR_INVALID, "dn_pipe_create: batch must be positive");
    DN_TRY(check_hop_args("dn_pipe_create", m, d, B, 0, 0.0f, flags));
    std::unique_ptr<dn_pipe> p(new dn_pipe());
    p->m = Ref<dn_model>(m); p->d = Ref<dn_dsp>(d); p->B = B; p->C = d->cfg.n_mels / 16;
    p->bf16 = (flags & DN_CONV_BF16) != 0;
    p->phase_in = (flags & DN_PHASE_FROM_INPUT) != 0;
    DN_TRY(build_bias(m, p->C, &p->bs));
    p->slot_floats = (dn::SlotLayout(B, d->cfg.n_mels, d->cfg.n_fft / 2 + 1).floats + 63) & ~size_t(63);
    p->init_elems = (size_t)B * 3 * (d->cfg.n_fft / 2 + 1);
    p->state_elems = (size_t)B * dn::parked_elems(d->cfg.n_fft);
    static_assert(sizeof(dn::PipeCtl) <= 256, "the control block fits its allocation");
    hipError_t e = p->ctl.alloc_zeroed(256);
    if (e == hipSuccess) e = p->scratch.alloc(p->n_slots * p->slot_floats * sizeof(float));
    // an input-phase pipe keeps every frame's phasors in its slot: the init area exists from the start (a captured push allocates nothing), and
    // dn_pipe_set_depth / dn_pipe_set_group re-allocate it with the slots
    if (e == hipSuccess && p->phase_in) e = p->scratch_init.alloc(p->n_slots * p->init_elems * sizeof(float2));
    if (e != hipSuccess) return fail(DN_ERR_HIP, std::string("dn_pipe_create: ") + hipGetErrorString(e));
    // Griffin-Lim head start: with at most one stream per CU (MI355X: 256 CUs) a front workgroup has slack at the end of a launch that
    // the pending hop's chain does not -- measured best at 8 iterations for n_fft 1024 (65.0 -> 56.0 us per batch-256 hop) and 12 for
    // n_fft 1536 (131 -> 97 us; round 3, profiles/r03_head_start_sweep.txt); with more streams than CUs every workgroup is busy throughout and it only adds traffic.
    // (The optimum moves up whenever the front half gets shorter: re-run tools/head_start_sweep.sh after changing either half.)
    const int it = default_head_start(p.get());       // (experiments: dn_pipe_set_head_start, tools/head_start_sweep.sh)
    if (it > 0) DN_TRY(dn_pipe_set_head_start(p.get(), it));
    *out = p.release();
    return DN_OK;
}

void dn_pipe_destroy(dn_pipe* p) {
    if (p && p->hio) {          // the two copy queues drain before their staging buffers and events go
        (void)hipStreamSynchronize(p->hio->h2d.get());
        (void)hipStreamSynchronize(p->hio->d2h.get());
    }
    delete p;
}

int dn_pipe_set_head_start(dn_pipe* p, int32_t iterations) {
    if (!p || iterations < 0) return fail(DN_ERR_INVALID, "dn_pipe_set_head_start: bad argument");
    if (iterations > 0 && p->group > 0) return fail(DN_ERR_INVALID, "dn_pipe_set_head_start: a group pipe never parks a chain");
    if (iterations > 0 && p->split == DN_SPLIT_ON) return fail(DN_ERR_INVALID, "dn_pipe_set_head_start: the pipe splits every hop into two launches (dn_pipe_set_split(p, DN_SPLIT_OFF or DN_SPLIT_AUTO) first)");
    if (iterations > 0 && !p->gl_state) DN_HIP(p->gl_state.alloc(p->n_slots * p->state_elems * sizeof(float2)));
    if (iterations > 0 && p->d->cfg.n_fft == 1536) DN_TRY(dn_pipe_reserve_parity(p));      // n_fft 1536: the front workgroup's spare wave draws the head start's initial phases into the slot
    p->gl_split = iterations;
    return DN_OK;
}

int dn_pipe_set_depth(dn_pipe* p, int32_t depth) {
    if (!p) return fail(DN_ERR_INVALID, "dn_pipe_set_depth: null pipe");
    if (depth < 1 || depth > DN_PIPE_MAX_DEPTH) return fail(DN_ERR_INVALID, "dn_pipe_set_depth: depth must be in 1.." + std::to_string(DN_PIPE_MAX_DEPTH));
    if (depth > 1 && p->d->cfg.n_fft != 1024) return refuse_not_1024("pipes deeper than one hop are built");
    if (depth > 1 && p->group > 0) return fail(DN_ERR_INVALID, "dn_pipe_set_depth: a group pipe runs whole chains per launch (dn_pipe_set_group(p, 0) first)");
    if (depth == p->depth) return DN_OK;
    dn::PipeCtl h{};
    DN_TRY(relayout(p, "dn_pipe_set_depth", depth + 1, depth > 1, depth > 1 || p->phase_in, h));      // (a deep pipe parks chain segments, and its front workgroups leave every frame's initial phases in its slot: dn_hop.hip)
    p->depth = depth;
    DN_HIP(hipMemcpy(p->ctl.get(), &h, sizeof(h), hipMemcpyHostToDevice));
    return dn_pipe_set_head_start(p, default_head_start(p));      // back to depth 1: the one-hop pipe's default head start again
}

int dn_pipe_set_group(dn_pipe* p, int32_t hops) {
    if (!p) return fail(DN_ERR_INVALID, "dn_pipe_set_group: null pipe");
    if (hops < 0 || hops > DN_PIPE_MAX_GROUP) return fail(DN_ERR_INVALID, "dn_pipe_set_group: hops must be in 0.." + std::to_string(DN_PIPE_MAX_GROUP));
    if (hops > 0 && p->d->cfg.n_fft != 1024)
        return fail(DN_ERR_UNSUPPORTED, "hop groups run whole Griffin-Lim chains one wavefront per stream, which is built for n_fft 1024 (at 1536 that form measured slower than a wavefront per column; at 512 it is not built)");
    if (hops > 0 && p->depth > 1) return fail(DN_ERR_INVALID, "dn_pipe_set_group: the pipe is deeper than one hop (dn_pipe_set_depth(p, 1) first)");
    if (hops > 0 && p->hio) return fail(DN_ERR_UNSUPPORTED, "dn_pipe_set_group: the host-buffer transport moves single hops");
    if (hops == p->group) return DN_OK;
    dn::PipeCtl h{};
    // two groups of the largest size: one being fronted, one whose chains run.  No chain is ever parked: the old state area goes, none comes
    DN_TRY(relayout(p, "dn_pipe_set_group", hops > 0 ? 2 * DN_PIPE_MAX_GROUP : p->depth + 1, false, static_cast<bool>(p->scratch_init), h));
    p->group = hops; p->group_pending = 0;
    p->group_pushes = h.pushes;                     // single pushes, replays and restores before this count towards priming: the control block is the record
    DN_HIP(hipMemcpy(p->ctl.get(), &h, sizeof(h), hipMemcpyHostToDevice));
    return hops > 0 ? DN_OK : dn_pipe_set_head_start(p, default_head_start(p));
}

int dn_pipe_set_gl_schedule(dn_pipe* p, int32_t schedule) {
    if (!p) return fail(DN_ERR_INVALID, "dn_pipe_set_gl_schedule: null pipe");
    if (schedule != DN_GL_AUTO && schedule != DN_GL_WAVE_PER_COLUMN && schedule != DN_GL_WAVE_PER_STREAM) return fail(DN_ERR_INVALID, "dn_pipe_set_gl_schedule: unknown schedule");
    if (schedule == DN_GL_WAVE_PER_STREAM && p->d->cfg.n_fft != 1024) return refuse_not_1024("the wavefront-per-stream Griffin-Lim is built");
    if (schedule == DN_GL_WAVE_PER_COLUMN && p->depth > 1) return fail(DN_ERR_INVALID, "a pipe deeper than one hop runs a wavefront per stream and chain segment");
    if (schedule == DN_GL_WAVE_PER_COLUMN && p->group > 0) return fail(DN_ERR_INVALID, "a group pipe runs whole chains a wavefront per stream (dn_pipe_set_group(p, 0) first)");
    p->gl_schedule = schedule;
    return DN_OK;
}

int dn_pipe_set_split(dn_pipe* p, int32_t mode) {
    if (!p) return fail(DN_ERR_INVALID, "dn_pipe_set_split: null pipe");
    if (mode != DN_SPLIT_AUTO && mode != DN_SPLIT_OFF && mode != DN_SPLIT_ON) return fail(DN_ERR_INVALID, "dn_pipe_set_split: unknown mode");
    if (mode == DN_SPLIT_ON && p->d->cfg.n_fft != 1024)
        return fail(DN_ERR_UNSUPPORTED, "the split hop belongs to the wavefront-per-stream Griffin-Lim, which is built for n_fft 1024 (not for 512 or 1536)");
    if (mode == DN_SPLIT_ON && p->gl_split > 0)
        return fail(DN_ERR_INVALID, "dn_pipe_set_split: the pipe runs a head start (a front workgroup that goes on with its frame's chain cannot be a launch of its own): "
                                    "dn_pipe_set_head_start(p, 0) first");
    if (mode == DN_SPLIT_ON && p->group > 0) return fail(DN_ERR_INVALID, "dn_pipe_set_split: a group pipe is one launch per group");
    p->split = mode;
    return DN_OK;
}

int dn_pipe_set_model(dn_pipe* p, const dn_model* m) {
    if (!p || !m) return fail(DN_ERR_INVALID, "dn_pipe_set_model: null argument");
    if (m == p->m.get()) return DN_OK;
    const BiasSet* bs = nullptr;
    DN_TRY(build_bias(m, p->C, &bs));
    p->m = Ref<dn_model>(m);       // launches already enqueued read the old arenas: the caller keeps the old model alive until they ran
    p->bs = bs;
    return DN_OK;
}

int dn_pipe_stream_create(const dn_model* m, const dn_dsp* d, int32_t B, uint32_t flags, dn_pipe** out) {
    dn_pipe* created = nullptr;
    DN_TRY(dn_pipe_create(m, d, B, flags, &created));
    std::unique_ptr<dn_pipe> p(created);
    const size_t line = (size_t)B * d->cfg.n_fft * sizeof(float), hxb = (size_t)B * dn::kHidden * p->C * sizeof(float);
    hipError_t e = p->ring.alloc_zeroed(line);
    if (e == hipSuccess) e = p->ola.alloc_zeroed(line);
    if (e == hipSuccess) e = p->hx.alloc_zeroed(hxb);
    if (e != hipSuccess) return fail(DN_ERR_HIP, std::string("dn_pipe_stream_create: ") + hipGetErrorString(e));
    *out = p.release();
    return DN_OK;
}

static int stream_state_copy(dn_pipe* p, float* ring, float* ola, float* hx, bool to_pipe, void* stream) {
    if (!p || !p->ring) return fail(DN_ERR_INVALID, "not a streaming pipe");
    const size_t line = (size_t)p->B * p->d->cfg.n_fft * sizeof(float), hxb = (size_t)p->B * dn::kHidden * p->C * sizeof(float);
    hipStream_t st = as_stream(stream);
    if (ring) DN_HIP(hipMemcpyAsync(to_pipe ? p->ring.get() : ring, to_pipe ? ring : p->ring.get(), line, hipMemcpyDeviceToDevice, st));
    if (ola) DN_HIP(hipMemcpyAsync(to_pipe ? p->ola.get() : ola, to_pipe ? ola : p->ola.get(), line, hipMemcpyDeviceToDevice, st));
    if (hx) DN_HIP(hipMemcpyAsync(to_pipe ? p->hx.get() : hx, to_pipe ? hx : p->hx.get(), hxb, hipMemcpyDeviceToDevice, st));
    return DN_OK;
}

int dn_pipe_stream_get_state(dn_pipe* p, float* ring, float* ola, float* hx, void* stream) { return stream_state_copy(p, ring, ola, hx, false, stream); }

int dn_pipe_stream_set_state(dn_pipe* p, const float* ring, const float* ola, const float* hx, uint64_t frames_done, void* stream) {
    DN_TRY(stream_state_copy(p, const_cast<float*>(ring), const_cast<float*>(ola), const_cast<float*>(hx), true, stream));
    // a restored ring is a primed ring; a hop that was pending is dropped (flush before taking a snapshot)
    p->group_pushes = (unsigned long long)(p->d->cfg.n_fft / p->d->cfg.hop - 1);          // (the host's own bookkeeping of a group pipe: primed, nothing pending)
    p->group_pending = 0;
    dn::launch_ctl_set(p->ctl.get(), (unsigned long long)(p->d->cfg.n_fft / p->d->cfg.hop - 1), frames_done, 0, as_stream(stream));
    return check_launch("ctl_set_kernel");
}

int dn_pipe_get_counters(dn_pipe* p, uint64_t* pushes, uint64_t* frames, int32_t* pending, void* stream) {
    if (!p) return fail(DN_ERR_INVALID, "dn_pipe_get_counters: null pipe");
    dn::PipeCtl h{};
    DN_HIP(hipMemcpyAsync(&h, p->ctl.get(), sizeof(h), hipMemcpyDeviceToHost, as_stream(stream)));
    DN_HIP(hipStreamSynchronize(as_stream(stream)));
    if (pushes) *pushes = h.pushes;
    if (frames) *frames = h.frames;
    if (pending) *pending = (int32_t)h.pending;
    return DN_OK;
}

// parity mode: a frame's injected phases travel with its scratch slot (so the caller's buffer is free again after the push)
int dn_pipe_reserve_parity(dn_pipe* p) {
    if (!p) return fail(DN_ERR_INVALID, "dn_pipe_reserve_parity: null pipe");
    if (!p->scratch_init) DN_HIP(p->scratch_init.alloc(p->n_slots * p->init_elems * sizeof(float2)));
    return DN_OK;
}

// the parts of a launch that are the same for every kind of push/submit/flush
static int fill_hop_args(dn_pipe* p, dn::HopArgs& a, const float* init_angles, uint64_t seed, uint64_t stream_id0, int32_t n_iter, float momentum) {
    if (n_iter < 0) return fail(DN_ERR_INVALID, "negative n_iter");
    DN_TRY(check_momentum(momentum, &a.mom));
    if (init_angles && p->phase_in) return fail(DN_ERR_INVALID, "this pipe was created with DN_PHASE_FROM_INPUT: it takes the phases from the input, init_angles must be NULL");
    if (init_angles && !p->scratch_init) {
        DN_TRY(dn_pipe_reserve_parity(p));
    }
    const dn_dsp_cfg& cfg = p->d->cfg;
    a.ctl = p->ctl.get();
    a.slots = p->scratch.get(); a.slot_stride = p->slot_floats;
    a.slot_init = p->scratch_init.get(); a.init_stride = p->init_elems;
    a.gl_state = p->gl_state.get(); a.state_stride = p->state_elems;
    a.n_slots = p->n_slots;
    a.gl_split = p->gl_split;
    a.init_in = init_angles; a.seed = seed; a.sid0 = stream_id0;
    a.phase_in = p->phase_in ? 1 : 0;
    a.n_iter = n_iter;
    a.B = p->B; a.C = p->C; a.back_B = p->B;
    // a wavefront per stream (four streams a workgroup) from four streams per CU up; a wavefront per column (the shortest chain) below
    const bool per_stream = p->depth > 1 || (cfg.n_fft == 1024 && (p->gl_schedule == DN_GL_WAVE_PER_STREAM ||
                                                                   (p->gl_schedule == DN_GL_AUTO && p->B >= dn::kGlwAutoStreams)));
    a.glw = per_stream ? 1 : 0;
    a.depth = p->depth;
    a.spb = per_stream ? 4 / p->depth : 1;          // a workgroup is four wavefronts: streams x chain segments
    a.back_blocks = (p->B + a.spb - 1) / a.spb;
    // two launches per hop where the chip holds only a fraction of a launch's workgroups at once (its chains and its front halves then run as
    // two phases anyway): from dn::kSplitAutoChains chain wavefronts on -- 2,048 fill every SIMD of an MI355X twice
    const bool can_split = per_stream && p->gl_split == 0;
    a.split = can_split && (p->split == DN_SPLIT_ON || (p->split == DN_SPLIT_AUTO && (long)p->B * p->depth >= dn::kSplitAutoChains)) ? 1 : 0;
    a.prime = cfg.n_fft / cfg.hop - 1;
    a.n_mels = cfg.n_mels; a.d_dev = p->d->view_dev.get(); a.c_dev = p->bs->view_dev.get();          // (the views in device memory: what the front halves read)
    if (p->group > 0) {          // whole chains (group_kernel): a workgroup's four wavefronts = spb streams x the pending frames of each
        a.glw = 1; a.depth = 1; a.split = 0; a.gl_split = 0;
        a.spb = p->group == 1 ? 4 : p->group == 2 ? 2 : 1;
        a.back_blocks = (p->B + a.spb - 1) / a.spb;
    }
    return DN_OK;
}

// one hop of a streaming pipe; `carry`: what a zero-copy host push adds (null for a plain push)
static int stream_push(dn_pipe* p, const void* hop_in, int32_t in_is_s16, void* hop_out, int32_t out_is_s16, const float* init_angles,
                       uint64_t seed, uint64_t stream_id0, int32_t n_iter, float momentum, void* stream, const HostCarry* carry) {
    if (!p || !p->ring) return fail(DN_ERR_INVALID, "dn_pipe_stream_push: not a streaming pipe");
    if (!hop_in || !hop_out) return fail(DN_ERR_INVALID, "dn_pipe_stream_push: null argument");
    if (p->group > 0) return fail(DN_ERR_INVALID, "dn_pipe_stream_push: this pipe takes groups of hops (dn_pipe_stream_push_group)");
    dn::HopArgs a{};
    DN_TRY(fill_hop_args(p, a, init_angles, seed, stream_id0, n_iter, momentum));
    a.front_B = p->B; a.hx = p->hx.get();
    if (carry) {
        a.host_done = carry->done; a.host_done_value = carry->done_value;
        a.host_copy_src = static_cast<const uint4*>(carry->copy_src); a.host_copy_dst = static_cast<uint4*>(carry->copy_dst);
        a.host_copy_n16 = (unsigned int)(carry->copy_bytes / 16);
    }
    a.hop_in = hop_in; a.ring = p->ring.get(); a.in_s16 = in_is_s16;
    a.ola = p->ola.get(); a.hop_out = hop_out; a.out_s16 = out_is_s16;
    dn::launch_hop(p->d->view, p->bs->view, a, p->bf16, as_stream(stream));
    DN_TRY(check_launch("hop_kernel(stream)"));
    ++p->group_pushes;              // (what *hops_valid of a later group flush charges to priming; the host-buffer pushes come through here too)
    return DN_OK;
}

int dn_pipe_stream_push(dn_pipe* p, const void* hop_in, int32_t in_is_s16, void* hop_out, int32_t out_is_s16,
                        const float* init_angles, uint64_t seed, uint64_t stream_id0, int32_t n_iter, float momentum, void* stream) {
    return stream_push(p, hop_in, in_is_s16, hop_out, out_is_s16, init_angles, seed, stream_id0, n_iter, momentum, stream, nullptr);
}

// ---- host-buffer transport (app3.py:168-172,189,215,244-250: the reference crosses host <-> device every hop)
// built completely, then attached: a failure leaves the pipe without one, and the next push tries again
static int host_io_init(dn_pipe* p) {
    if (p->hio) return DN_OK;
    std::unique_ptr<HostIo> h(new HostIo());
    const size_t bytes = (size_t)p->B * p->d->cfg.hop * sizeof(float);
    DN_HIP(h->h2d.create(hipStreamNonBlocking));
    DN_HIP(h->d2h.create(hipStreamNonBlocking));
    for (int i = 0; i < HostIo::kRing; ++i) {
        DN_HIP(h->ev_h2d[i].create(hipEventDisableTiming));
        DN_HIP(h->ev_k[i].create(hipEventDisableTiming));
        DN_HIP(h->ev_d2h[i].create(hipEventDisableTiming));
    }
    for (int i = 0; i < 2; ++i) {
        DN_HIP(h->d_in[i].alloc(bytes));
        DN_HIP(h->d_out[i].alloc(bytes));
    }
    DN_HIP(h->done_host.alloc(64));
    *h->done_host.get() = 0;
    DN_HIP(h->done_host.device_view(&h->done_dev));
    p->hio = std::move(h);
    return DN_OK;
}

// the device's own address of page-locked host memory, or null when `host` is pageable
static void* device_view(const void* host) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (at.type != hipMemoryTypeHost) return nullptr;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, const_cast<void*>(host), 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return dp;
}

// the deferred output of the newest push, when no further launch will carry it: a copy launch and a one-thread launch that publishes it
static int host_defer_drain(HostIo* h, hipStream_t st) {
    if (!h->defer_pending) return DN_OK;
    dn::launch_host_copy(static_cast<const uint4*>(h->z_out[h->defer_ticket & 1].get()), static_cast<uint4*>(h->defer_dst), (unsigned int)(h->defer_bytes / 16),
                         h->done_dev, h->defer_ticket + 1, st);
    h->defer_pending = false;
    return check_launch("host_copy_kernel");
}

int dn_pipe_stream_push_host(dn_pipe* p, const void* hop_in_host, int32_t in_is_s16, void* hop_out_host, int32_t out_is_s16, uint64_t seed,
                             uint64_t stream_id0, int32_t n_iter, float momentum, uint32_t flags, void* stream, uint64_t* ticket) {
    // everything is validated before the transport is built: a refused call leaves the pipe as it was
    if (!p || !p->ring) return fail(DN_ERR_INVALID, "dn_pipe_stream_push_host: not a streaming pipe");
    if (!hop_in_host || !hop_out_host) return fail(DN_ERR_INVALID, "dn_pipe_stream_push_host: null argument");
    if (flags & ~(uint32_t)(DN_HOST_STAGED | DN_HOST_DEFER)) return fail(DN_ERR_INVALID, "dn_pipe_stream_push_host: unknown flag bits");
    if (p->group > 0) return fail(DN_ERR_UNSUPPORTED, "dn_pipe_stream_push_host: the host-buffer transport moves single hops (dn_pipe_set_group(p, 0))");
    DN_TRY(host_io_init(p));
    HostIo* h = p->hio.get();
    hipStream_t cs = as_stream(stream);
    const size_t out_bytes = (size_t)p->B * p->d->cfg.hop * (out_is_s16 ? sizeof(short) : sizeof(float));
    if (!(flags & DN_HOST_STAGED)) {
        // zero copy: page-locked host memory is in the device's address space.  The front workgroups read their stream's hop (1 KB) straight from it
        // and the Griffin-Lim workgroups store the emitted hop straight into it -- no copy engine, no second queue, no cross-queue event.
        void* din = device_view(hop_in_host);
        void* dout = device_view(hop_out_host);
        if (din && dout) {
            const bool defer = (flags & DN_HOST_DEFER) != 0 && out_bytes % 16 == 0;
            void* kout = dout;
            if (defer) {
                // the launch leaves its emitted hop in a device staging buffer; the NEXT launch (or dn_pipe_stream_host_wait) moves it to dout
                DevBuf<void>& z = h->z_out[h->pushes & 1];
                if (!z) DN_HIP(z.alloc((size_t)p->B * p->d->cfg.hop * sizeof(float)));
                kout = z.get();
            }
            HostCarry carry{};
            if (h->defer_pending) {                              // this launch carries the previous push's hop out, spread over its threads
                carry.copy_src = h->z_out[h->defer_ticket & 1].get();
                carry.copy_dst = h->defer_dst;
                carry.copy_bytes = h->defer_bytes;
            }
            // the launch's last workgroup publishes how many pushes have their samples in host memory once it returns
            carry.done = defer && !h->defer_pending ? nullptr : h->done_dev;
            carry.done_value = defer ? h->pushes : h->pushes + 1;
            DN_TRY(stream_push(p, din, in_is_s16, kout, out_is_s16, nullptr, seed, stream_id0, n_iter, momentum, stream, &carry));
            h->defer_pending = defer;
            h->defer_stream = cs;                                  // (also what dn_pipe_stream_host_wait polls for errors)
            if (defer) { h->defer_ticket = h->pushes; h->defer_dst = dout; h->defer_bytes = out_bytes; }
            h->last_zero_copy[h->pushes % HostIo::kRing] = true;
            if (ticket) *ticket = h->pushes;
            ++h->pushes;
            return DN_OK;
        }
    }
    DN_TRY(host_defer_drain(h, cs));                             // (a staged push behind a deferred one: its hop leaves first)
    const int s = (int)(h->pushes & 1);                                  // device staging buffer
    const int e = (int)(h->pushes % HostIo::kRing), e2 = (int)((h->pushes + HostIo::kRing - 2) % HostIo::kRing);      // this push's events; those of two pushes ago
    const size_t n = (size_t)p->B * p->d->cfg.hop;
    const size_t bin = n * (in_is_s16 ? sizeof(short) : sizeof(float)), bout = n * (out_is_s16 ? sizeof(short) : sizeof(float));
    const hipStream_t h2d = h->h2d.get(), d2h = h->d2h.get();
    h->last_zero_copy[h->pushes % HostIo::kRing] = false;
    // upload: the staging buffer was read by the launch two pushes ago
    if (h->pushes >= 2) DN_HIP(hipStreamWaitEvent(h2d, h->ev_k[e2].get(), 0));
    DN_HIP(hipMemcpyAsync(h->d_in[s].get(), hop_in_host, bin, hipMemcpyHostToDevice, h2d));
    DN_HIP(hipEventRecord(h->ev_h2d[e].get(), h2d));
    // the hop: after its samples arrived, and after the download of the result it is about to overwrite
    DN_HIP(hipStreamWaitEvent(cs, h->ev_h2d[e].get(), 0));
    if (h->pushes >= 2) DN_HIP(hipStreamWaitEvent(cs, h->ev_d2h[e2].get(), 0));
    DN_TRY(stream_push(p, h->d_in[s].get(), in_is_s16, h->d_out[s].get(), out_is_s16, nullptr, seed, stream_id0, n_iter, momentum, stream, nullptr));
    DN_HIP(hipEventRecord(h->ev_k[e].get(), cs));
    // download
    DN_HIP(hipStreamWaitEvent(d2h, h->ev_k[e].get(), 0));
    DN_HIP(hipMemcpyAsync(hop_out_host, h->d_out[s].get(), bout, hipMemcpyDeviceToHost, d2h));
    DN_HIP(hipEventRecord(h->ev_d2h[e].get(), d2h));
    if (ticket) *ticket = h->pushes;
    ++h->pushes;
    return DN_OK;
}

int dn_pipe_stream_host_wait(dn_pipe* p, uint64_t ticket) {
    if (!p || !p->hio) return fail(DN_ERR_INVALID, "dn_pipe_stream_host_wait: no host push was made on this pipe");
    HostIo* h = p->hio.get();
    if (ticket >= h->pushes) return fail(DN_ERR_INVALID, "dn_pipe_stream_host_wait: no such push");
    if (h->defer_pending && ticket >= h->defer_ticket) {         // its samples are still in the staging buffer and no launch is queued to move them
        DN_TRY(host_defer_drain(h, h->defer_stream));
    }
    // Wait for one push by its own transport: a zero-copy push through the completion word its launch (or the launch that carried its deferred
    // samples out) publishes, a staged one through the event behind its download.
    auto wait_entry = [&](uint64_t e) -> int {
        if (h->last_zero_copy[e % HostIo::kRing]) {
            // launches of one stream complete in order: the word only grows.  Spin briefly, then yield (a hop is tens of microseconds); a launch that
            // faulted or hangs never publishes, so the stream is polled beside the word: anything but "not ready yet" ends the wait, and "idle" with
            // the word still short of the ticket (the launches ran, the publication did not) is an error too
            const volatile unsigned long long* w = h->done_host.get();
            for (unsigned spins = 0; __atomic_load_n(w, __ATOMIC_ACQUIRE) < e + 1; ++spins) {
                if (spins > 2000) std::this_thread::yield();
                if ((spins & 0x3fff) == 0x3fff) {
                    const hipError_t q = hipStreamQuery(h->defer_stream);
                    if (q == hipSuccess) {
                        if (__atomic_load_n(w, __ATOMIC_ACQUIRE) >= e + 1) break;
                        return fail(DN_ERR_HIP, "dn_pipe_stream_host_wait: the stream is idle but push " + std::to_string(e) + " was never published");
                    }
                    (void)hipGetLastError();          // (hipErrorNotReady is sticky in the thread's last-error slot)
                    if (q != hipErrorNotReady) return fail(DN_ERR_HIP, std::string("dn_pipe_stream_host_wait: ") + hipGetErrorString(q));
                }
            }
            return DN_OK;
        }
        DN_HIP(hipEventSynchronize(h->ev_d2h[e % HostIo::kRing].get()));
        return DN_OK;
    };
    // Only the last kRing pushes still own their events and their transport flag.  Either transport completes in order, so an older ticket is
    // complete once the OLDEST surviving push of EACH transport is -- and where the ring holds no staged push any more, once the download queue has
    // drained (a zero-copy launch says nothing about a download on another queue; a staged push does cover the zero-copy launches before it: its
    // download follows its own launch on the caller's stream).
    const uint64_t oldest = h->pushes > (uint64_t)HostIo::kRing ? h->pushes - HostIo::kRing : 0;
    if (ticket >= oldest) return wait_entry(ticket);
    bool seen[2] = {false, false};
    for (uint64_t e = oldest; e < h->pushes; ++e) {
        const int kind = h->last_zero_copy[e % HostIo::kRing] ? 1 : 0;
        if (seen[kind]) continue;
        seen[kind] = true;
        DN_TRY(wait_entry(e));
    }
    if (!seen[0] && h->d2h) DN_HIP(hipStreamSynchronize(h->d2h.get()));
    return DN_OK;
}

int dn_pipe_stream_flush(dn_pipe* p, void* hop_out, int32_t out_is_s16, int32_t n_iter, float momentum, void* stream) {
    if (!p || !p->ring) return fail(DN_ERR_INVALID, "dn_pipe_stream_flush: not a streaming pipe");
    if (!hop_out) return fail(DN_ERR_INVALID, "dn_pipe_stream_flush: null argument");
    if (p->group > 0) return fail(DN_ERR_INVALID, "dn_pipe_stream_flush: this pipe emits groups of hops (dn_pipe_stream_flush_group)");
    dn::HopArgs a{};
    DN_TRY(fill_hop_args(p, a, nullptr, 0, 0, n_iter, momentum));
    a.front_B = 0;
    a.ola = p->ola.get(); a.hop_out = hop_out; a.out_s16 = out_is_s16;
    dn::launch_hop(p->d->view, p->bs->view, a, p->bf16, as_stream(stream));
    return check_launch("hop_kernel(stream flush)");
}

int dn_pipe_submit(dn_pipe* p, const float* frames, float* hx, float* out, const float* init_angles, uint64_t seed, uint64_t stream_id0, int32_t n_iter, float momentum, void* stream) {
    if (!p || !frames || !hx || !out) return fail(DN_ERR_INVALID, "dn_pipe_submit: null argument");
    if (p->ring) return fail(DN_ERR_INVALID, "dn_pipe_submit: this is a streaming pipe (use dn_pipe_stream_push)");
    if (p->group > 0) return dn_pipe_submit_group(p, frames, 0, hx, out, 0, init_angles, 0, seed, stream_id0, 1, n_iter, momentum, stream);
    dn::HopArgs a{};
    DN_TRY(fill_hop_args(p, a, init_angles, seed, stream_id0, n_iter, momentum));
    a.front_B = p->B; a.frames = frames; a.hx = hx;
    a.gl_out = out;                  // THIS hop's destination: its front workgroups leave it in the slot for the Griffin-Lim workgroups of the next launch
    dn::launch_hop(p->d->view, p->bs->view, a, p->bf16, as_stream(stream));
    DN_TRY(check_launch("hop_kernel"));
    p->submitted = true;
    return DN_OK;
}

int dn_pipe_flush(dn_pipe* p, int32_t n_iter, float momentum, void* stream) {
    if (!p) return fail(DN_ERR_INVALID, "dn_pipe_flush: null pipe");
    if (p->ring) return fail(DN_ERR_INVALID, "dn_pipe_flush: this is a streaming pipe (use dn_pipe_stream_flush)");
    if (!p->submitted) return DN_OK; // nothing was ever submitted
    dn::HopArgs a{};
    DN_TRY(fill_hop_args(p, a, nullptr, 0, 0, n_iter, momentum));
    a.front_B = 0;
    if (p->group > 0) {                             // one launch: the whole chains of the group in flight
        dn::launch_group(p->d->view, p->bs->view, a, p->bf16, as_stream(stream));
        return check_launch("group_kernel(flush)");
    }
    for (int i = 0; i < p->depth; ++i) {            // every launch advances each hop in flight by one chain segment
        dn::launch_hop(p->d->view, p->bs->view, a, p->bf16, as_stream(stream));
        DN_TRY(check_launch("hop_kernel(flush)"));
    }
    return DN_OK;
}

int dn_pipe_submit_group(dn_pipe* p, const float* frames, int64_t frames_stride, float* hx, float* out, int64_t out_stride, const float* init_angles, int64_t init_stride, uint64_t seed,
                         uint64_t stream_id0, int32_t hops, int32_t n_iter, float momentum, void* stream) {
    if (!p || !frames || !hx || !out) return fail(DN_ERR_INVALID, "dn_pipe_submit_group: null argument");
    if (p->ring) return fail(DN_ERR_INVALID, "dn_pipe_submit_group: this is a streaming pipe (use dn_pipe_stream_push_group)");
    if (p->group <= 0) return fail(DN_ERR_INVALID, "dn_pipe_submit_group: not a group pipe (dn_pipe_set_group)");
    if (hops < 1 || hops > p->group) return fail(DN_ERR_INVALID, "dn_pipe_submit_group: hops must be in 1.." + std::to_string(p->group));
    if (frames_stride < 0 || out_stride < 0 || init_stride < 0) return fail(DN_ERR_INVALID, "dn_pipe_submit_group: negative stride");
    const int64_t line = (int64_t)p->B * p->d->cfg.n_fft;
    if (hops > 1 && out_stride < line) return fail(DN_ERR_INVALID, "dn_pipe_submit_group: the output frames of a group overlap (out_stride < B * n_fft)");
    dn::HopArgs a{};
    DN_TRY(fill_hop_args(p, a, init_angles, seed, stream_id0, n_iter, momentum));
    a.front_B = p->B; a.frames = frames; a.hx = hx; a.gl_out = out;
    a.group_hops = hops; a.frames_stride = frames_stride; a.out_stride = out_stride; a.init_in_stride = init_stride;
    dn::launch_group(p->d->view, p->bs->view, a, p->bf16, as_stream(stream));
    DN_TRY(check_launch("group_kernel"));
    p->submitted = true;
    return DN_OK;
}

int dn_pipe_stream_push_group(dn_pipe* p, const void* hop_in, int64_t in_stride, int32_t in_is_s16, void* hop_out, int64_t out_stride, int32_t out_is_s16, const float* init_angles,
                              int64_t init_stride, uint64_t seed, uint64_t stream_id0, int32_t n_iter, float momentum, void* stream) {
    if (!p || !p->ring) return fail(DN_ERR_INVALID, "dn_pipe_stream_push_group: not a streaming pipe");
    if (!hop_in || !hop_out) return fail(DN_ERR_INVALID, "dn_pipe_stream_push_group: null argument");
    if (p->group <= 0) return fail(DN_ERR_INVALID, "dn_pipe_stream_push_group: not a group pipe (dn_pipe_set_group)");
    const int64_t row = (int64_t)p->B * p->d->cfg.hop;
    if (in_stride < 0 || init_stride < 0 || (p->group > 1 && out_stride < row))
        return fail(DN_ERR_INVALID, "dn_pipe_stream_push_group: bad stride (the emitted hops of a group must not overlap)");
    dn::HopArgs a{};
    DN_TRY(fill_hop_args(p, a, init_angles, seed, stream_id0, n_iter, momentum));
    a.front_B = p->B; a.hx = p->hx.get();
    a.hop_in = hop_in; a.ring = p->ring.get(); a.in_s16 = in_is_s16;
    a.ola = p->ola.get(); a.hop_out = hop_out; a.out_s16 = out_is_s16;
    a.group_hops = p->group; a.group_out = p->group; a.filler_first = 1;
    a.hop_in_stride = in_stride; a.hop_out_stride = out_stride; a.init_in_stride = init_stride;
    dn::launch_group(p->d->view, p->bs->view, a, p->bf16, as_stream(stream));
    DN_TRY(check_launch("group_kernel(stream)"));
    const unsigned long long before = p->group_pushes;
    p->group_pushes += (unsigned long long)p->group;
    const unsigned long long prime = (unsigned long long)a.prime;
    const unsigned long long primed_before = before < prime ? before : prime, primed_after = p->group_pushes < prime ? p->group_pushes : prime;
    p->group_pending = p->group - (int)(primed_after - primed_before);
    return DN_OK;
}

int dn_pipe_stream_flush_group(dn_pipe* p, void* hop_out, int64_t out_stride, int32_t out_is_s16, int32_t* hops_valid, void* stream) {
    if (!p || !p->ring) return fail(DN_ERR_INVALID, "dn_pipe_stream_flush_group: not a streaming pipe");
    if (!hop_out) return fail(DN_ERR_INVALID, "dn_pipe_stream_flush_group: null argument");
    if (p->group <= 0) return fail(DN_ERR_INVALID, "dn_pipe_stream_flush_group: not a group pipe (dn_pipe_set_group)");
    if (p->group > 1 && out_stride < (int64_t)p->B * p->d->cfg.hop) return fail(DN_ERR_INVALID, "dn_pipe_stream_flush_group: the emitted hops overlap");
    dn::HopArgs a{};
    DN_TRY(fill_hop_args(p, a, nullptr, 0, 0, 0, 0.0f));
    a.front_B = 0;
    a.ola = p->ola.get(); a.hop_out = hop_out; a.out_s16 = out_is_s16;
    a.group_hops = 0; a.group_out = p->group; a.filler_first = 0; a.hop_out_stride = out_stride;
    dn::launch_group(p->d->view, p->bs->view, a, p->bf16, as_stream(stream));
    DN_TRY(check_launch("group_kernel(stream flush)"));
    if (hops_valid) *hops_valid = p->group_pending;
    p->group_pending = 0;
    return DN_OK;
}

}  // extern "C"
