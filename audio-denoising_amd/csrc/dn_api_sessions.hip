// dn_api_sessions.hip -- dn_sessions: session pools (kernels: dn_sessions.hip).  No kernel code here.
#include "dn_host.hpp"

namespace {

// DN_SESS_AUTO: two launches (front halves, then a wavefront per chain) from this many listed slots per push on, n_fft 1024 (measured: DESIGN.md)
constexpr int kSessSplitAuto = 1024;

dn::SessArgs sess_args(dn_sessions* s) {
    dn::SessArgs a{};
    const int M = s->d->cfg.n_mels, K = s->d->cfg.n_fft / 2 + 1;
    const size_t cap = (size_t)s->cap;
    unsigned long long* counters = s->counters.get();
    a.ring = s->ring.get(); a.ola = s->ola.get(); a.hx = s->hx.get();
    a.frames = counters; a.sids = counters + cap; a.pushes = reinterpret_cast<unsigned int*>(counters + 2 * cap);
    a.prime = s->d->cfg.n_fft / s->d->cfg.hop - 1;
    a.mel = s->ws.get(); a.diff = a.mel + cap * 3 * M; a.lin = a.diff + cap * 3 * M; a.peak = a.lin + cap * 3 * K;
    a.meta = reinterpret_cast<uint32_t*>(a.peak + cap);
    a.C = s->C;
    return a;
}

// every id in range, none twice, and (need_open) every slot open; nothing is changed on failure
int sess_check_ids(dn_sessions* s, const char* who, const int32_t* ids, int32_t n, bool need_open) {
    if (n < 0) return fail(DN_ERR_INVALID, std::string(who) + ": negative count");
    if (n > s->cap) return fail(DN_ERR_INVALID, std::string(who) + ": " + std::to_string(n) + " ids for a pool of " + std::to_string(s->cap) + " slots");
    if (n > 0 && !ids) return fail(DN_ERR_INVALID, std::string(who) + ": null id list");
    int rc = DN_OK;
    int32_t i = 0;
    for (; i < n; ++i) {
        const int32_t id = ids[i];
        if (id < 0 || id >= s->cap) { rc = fail(DN_ERR_INVALID, std::string(who) + ": id " + std::to_string(id) + " (position " + std::to_string(i) + ") is out of range [0, " + std::to_string(s->cap) + ")"); break; }
        if (s->seen[id]) { rc = fail(DN_ERR_INVALID, std::string(who) + ": id " + std::to_string(id) + " appears twice in the list"); break; }
        if (need_open && !s->open[id]) { rc = fail(DN_ERR_INVALID, std::string(who) + ": slot " + std::to_string(id) + " is not open"); break; }
        s->seen[id] = 1;
    }
    for (int32_t j = 0; j < i; ++j) s->seen[ids[j]] = 0;
    return rc;
}

// the next staging entry, free again: its event (recorded behind the last launch that read it) has completed.  The kernels read the entry
// straight from page-locked host memory (one 4-byte load per workgroup; measured: a copy to the device ahead of the launch cost small ticks
// 5-9 us); DN_SESS_IDS_COPY builds the copying form.  `a`: the pool's arguments with this list.
int sess_stage(dn_sessions* s, const int32_t* ids, int32_t n, const uint64_t* sids, hipStream_t st, dn::SessArgs& a, const uint64_t** sids_dev) {
    a = sess_args(s);
    const int k = (int)(s->calls % dn_sessions::kRing);
    if (s->ev_live[k]) DN_HIP(hipEventSynchronize(s->ev[k].get()));
    char* h = s->stage_host.get() + (size_t)k * s->stage_bytes;
    char* dv = s->stage_dev + (size_t)k * s->stage_bytes;
    const size_t sid_off = ((size_t)s->cap * sizeof(int32_t) + 7) & ~size_t(7);
    memcpy(h, ids, (size_t)n * sizeof(int32_t));
    if (sids_dev) {
        uint64_t* hs = reinterpret_cast<uint64_t*>(h + sid_off);
        for (int32_t i = 0; i < n; ++i) hs[i] = sids ? sids[i] : (uint64_t)ids[i];
        *sids_dev = reinterpret_cast<const uint64_t*>(dv + sid_off);
    }
#ifdef DN_SESS_IDS_COPY
    DN_HIP(hipMemcpyAsync(dv, h, sids_dev ? sid_off + (size_t)n * sizeof(uint64_t) : (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
#else
    (void)st;
#endif
    a.ids = reinterpret_cast<const int32_t*>(dv);
    a.n = n;
    return DN_OK;
}

// the record geometry of a pool (include/dn_denoise.h: record layout version 1)
dn::SessRec sess_rec(const dn_sessions* s) {
    const dn_dsp_cfg& c = s->d->cfg;
    const auto a16 = [](size_t x) { return (x + 15) & ~size_t(15); };
    dn::SessRec r{};
    r.ola_off = dn::kSessRecHead + a16((size_t)c.n_fft * sizeof(float));
    r.hx_off = r.ola_off + a16((size_t)c.n_fft * sizeof(float));
    r.stride = (r.hx_off + (size_t)dn::kHidden * s->C * sizeof(float) + 255) & ~size_t(255);
    r.want.magic = DN_SESS_RECORD_MAGIC; r.want.version = DN_SESS_RECORD_VERSION;
    r.want.sample_rate = (uint32_t)c.sample_rate; r.want.n_fft = (uint32_t)c.n_fft; r.want.hop = (uint32_t)c.hop;
    r.want.n_mels = (uint32_t)c.n_mels; r.want.hidden = (uint32_t)dn::kHidden; r.want.C = (uint32_t)s->C;
    r.prime = (uint32_t)(c.n_fft / c.hop - 1);
    return r;
}

std::string sess_geometry(uint32_t sr, uint32_t n_fft, uint32_t hop, uint32_t n_mels, uint32_t hidden, uint32_t C) {
    return "sample_rate " + std::to_string(sr) + ", n_fft " + std::to_string(n_fft) + ", hop " + std::to_string(hop) + ", n_mels " +
           std::to_string(n_mels) + ", hidden " + std::to_string(hidden) + ", C " + std::to_string(C);
}

int sess_staged(dn_sessions* s, hipStream_t st) {
    const int k = (int)(s->calls % dn_sessions::kRing);
    DN_HIP(hipEventRecord(s->ev[k].get(), st));
    s->ev_live[k] = true;
    ++s->calls;
    return DN_OK;
}

}  // namespace

extern "C" {

void dn_sessions_destroy(dn_sessions* s) {
    if (!s) return;
    for (int k = 0; k < dn_sessions::kRing; ++k)       // the launches that read the staging ring finish before it goes
        if (s->ev_live[k]) (void)hipEventSynchronize(s->ev[k].get());
    delete s;
}

int dn_sessions_create(const dn_model* m, const dn_dsp* d, int32_t capacity, uint32_t flags, dn_sessions** out) {
    if (!out) return fail(DN_ERR_INVALID, "dn_sessions_create: null argument");
    if (capacity <= 0) return fail(DN_ERR_INVALID, "dn_sessions_create: capacity must be positive");
    DN_TRY(check_hop_args("dn_sessions_create", m, d, capacity, 0, 0.0f, flags));
    std::unique_ptr<dn_sessions> s(new dn_sessions());
    s->m = Ref<dn_model>(m); s->d = Ref<dn_dsp>(d);
    s->cap = capacity; s->C = d->cfg.n_mels / 16;
    s->bf16 = (flags & DN_CONV_BF16) != 0;
    s->open.assign(capacity, 0);
    s->seen.assign(capacity, 0);
    DN_TRY(build_bias(m, s->C, &s->bs));
    const size_t cap = (size_t)capacity, N = d->cfg.n_fft, M = d->cfg.n_mels, K = N / 2 + 1;
    const size_t line = cap * N * sizeof(float), hxb = cap * dn::kHidden * s->C * sizeof(float);
    const size_t ws = (cap * (6 * M + 3 * K + 1) + cap * dn::kSessMeta) * sizeof(float);
    s->stage_bytes = ((cap * sizeof(int32_t) + 7) & ~size_t(7)) + cap * sizeof(uint64_t);
    s->stage_bytes = (s->stage_bytes + 255) & ~size_t(255);
    hipError_t e = s->ring.alloc_zeroed(line);
    if (e == hipSuccess) e = s->ola.alloc_zeroed(line);
    if (e == hipSuccess) e = s->hx.alloc_zeroed(hxb);
    if (e == hipSuccess) e = s->counters.alloc_zeroed(3 * cap * sizeof(unsigned long long));
    if (e == hipSuccess) e = s->ws.alloc_zeroed(ws);
    if (e == hipSuccess && (flags & DN_PHASE_FROM_INPUT)) e = s->phas.alloc(phasor_bytes(d, cap));
    if (e == hipSuccess) e = s->stage_host.alloc(dn_sessions::kRing * s->stage_bytes);
    if (e == hipSuccess) e = s->chk_host.alloc(cap * sizeof(uint32_t));
    if (e == hipSuccess) e = s->chk_host.device_view(&s->chk_dev);
#ifdef DN_SESS_IDS_COPY
    if (e == hipSuccess) e = s->stage_ring.alloc(dn_sessions::kRing * s->stage_bytes);
    s->stage_dev = s->stage_ring.get();
#else
    if (e == hipSuccess) e = s->stage_host.device_view(&s->stage_dev);
#endif
    for (int k = 0; k < dn_sessions::kRing && e == hipSuccess; ++k) e = s->ev[k].create(hipEventDisableTiming);
    if (e != hipSuccess) return fail(DN_ERR_HIP, std::string("dn_sessions_create: ") + hipGetErrorString(e));
    *out = s.release();
    return DN_OK;
}

int dn_sessions_open(dn_sessions* s, const int32_t* ids, int32_t n, const uint64_t* stream_ids, void* stream) {
    if (!s) return fail(DN_ERR_INVALID, "dn_sessions_open: null pool");
    int rc = sess_check_ids(s, "dn_sessions_open", ids, n, false);
    if (rc != DN_OK || n == 0) return rc;
    hipStream_t st = as_stream(stream);
    dn::SessArgs a;
    const uint64_t* sids_dev = nullptr;
    DN_TRY(sess_stage(s, ids, n, stream_ids, st, a, &sids_dev));
    dn::launch_sess_open(a, sids_dev, s->d->cfg.n_fft, st);
    DN_TRY(check_launch("sess_open_kernel"));
    for (int32_t i = 0; i < n; ++i) s->open[ids[i]] = 1;
    return sess_staged(s, st);
}

int dn_sessions_close(dn_sessions* s, const int32_t* ids, int32_t n) {
    if (!s) return fail(DN_ERR_INVALID, "dn_sessions_close: null pool");
    DN_TRY(sess_check_ids(s, "dn_sessions_close", ids, n, true));
    for (int32_t i = 0; i < n; ++i) s->open[ids[i]] = 0;
    return DN_OK;
}

int dn_sessions_set_schedule(dn_sessions* s, int32_t schedule) {
    if (!s) return fail(DN_ERR_INVALID, "dn_sessions_set_schedule: null pool");
    if (schedule != DN_SESS_AUTO && schedule != DN_SESS_ONE_LAUNCH && schedule != DN_SESS_TWO_LAUNCHES) return fail(DN_ERR_INVALID, "dn_sessions_set_schedule: unknown schedule");
    if (schedule == DN_SESS_TWO_LAUNCHES && s->d->cfg.n_fft != 1024)
        return fail(DN_ERR_UNSUPPORTED, "dn_sessions_set_schedule: the two-launch form runs a wavefront per Griffin-Lim chain, which is built for n_fft 1024 (not for 512 or 1536)");
    s->schedule = schedule;
    return DN_OK;
}

int dn_sessions_push(dn_sessions* s, const int32_t* ids, int32_t n, const void* hop_in, int32_t in_is_s16, void* hop_out,
                     int32_t out_is_s16, const float* init_angles, uint64_t seed, int32_t n_iter, float momentum, void* stream) {
    // everything is validated before the first launch: a failed call leaves every slot as it was
    if (!s) return fail(DN_ERR_INVALID, "dn_sessions_push: null pool");
    int rc = sess_check_ids(s, "dn_sessions_push", ids, n, true);
    if (rc != DN_OK || n == 0) return rc;
    if (!hop_in || !hop_out) return fail(DN_ERR_INVALID, "dn_sessions_push: null argument");
    if (init_angles && s->phas) return fail(DN_ERR_INVALID, "dn_sessions_push: this pool was created with DN_PHASE_FROM_INPUT: it takes the phases from the input, init_angles must be NULL");
    float mom = 0.0f;
    DN_TRY(check_hop_args("dn_sessions_push", s->m.get(), s->d.get(), n, n_iter, momentum, 0, &mom));
    hipStream_t st = as_stream(stream);
    dn::SessArgs a;
    DN_TRY(sess_stage(s, ids, n, nullptr, st, a, nullptr));
    a.hop_in = hop_in; a.in_s16 = in_is_s16 ? 1 : 0; a.hop_out = hop_out; a.out_s16 = out_is_s16 ? 1 : 0;
    const bool phase_in = static_cast<bool>(s->phas);
    a.init = phase_in ? s->phas.get() : init_angles; a.seed = seed; a.n_iter = n_iter; a.mom = mom;
    const bool two = s->d->cfg.n_fft == 1024 && (s->schedule == DN_SESS_TWO_LAUNCHES || (s->schedule == DN_SESS_AUTO && n >= kSessSplitAuto));
    if (two) dn::launch_sess_split(s->d->view, s->bs->view, a, s->bf16, st, phase_in);
    else dn::launch_sess_frame(s->d->view, s->bs->view, a, s->bf16, st, phase_in);
    DN_TRY(check_launch(two ? "sess_front_kernel / sess_chain_kernel" : "sess_frame_kernel"));
    return sess_staged(s, st);
}

size_t dn_sessions_record_bytes(const dn_sessions* s) { return s ? sess_rec(s).stride : 0; }

int dn_sessions_export(dn_sessions* s, const int32_t* ids, int32_t n, void* records, void* stream) {
    if (!s) return fail(DN_ERR_INVALID, "dn_sessions_export: null pool");
    int rc = sess_check_ids(s, "dn_sessions_export", ids, n, true);
    if (rc != DN_OK || n == 0) return rc;
    if (!records) return fail(DN_ERR_INVALID, "dn_sessions_export: null records");
    if (reinterpret_cast<uintptr_t>(records) % 16 != 0) return fail(DN_ERR_INVALID, "dn_sessions_export: records must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    dn::SessArgs a;
    DN_TRY(sess_stage(s, ids, n, nullptr, st, a, nullptr));
    dn::launch_sess_export(a, sess_rec(s), s->d->cfg.n_fft, records, st);
    DN_TRY(check_launch("sess_export_kernel"));
    return sess_staged(s, st);
}

int dn_sessions_import(dn_sessions* s, const int32_t* ids, int32_t n, const void* records, const uint64_t* stream_ids, void* stream) {
    // ids on the host, then every record's header on the device into page-locked memory and one synchronisation: no slot changes unless all pass
    if (!s) return fail(DN_ERR_INVALID, "dn_sessions_import: null pool");
    int rc = sess_check_ids(s, "dn_sessions_import", ids, n, false);
    if (rc != DN_OK || n == 0) return rc;
    if (!records) return fail(DN_ERR_INVALID, "dn_sessions_import: null records");
    if (reinterpret_cast<uintptr_t>(records) % 16 != 0) return fail(DN_ERR_INVALID, "dn_sessions_import: records must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    dn::SessArgs a;
    const uint64_t* sids_dev = nullptr;
    DN_TRY(sess_stage(s, ids, n, stream_ids, st, a, stream_ids ? &sids_dev : nullptr));
    const dn::SessRec r = sess_rec(s);
    dn::launch_sess_check(a, r, records, s->chk_dev, st);
    DN_TRY(check_launch("sess_check_kernel"));
    DN_HIP(hipStreamSynchronize(st));          // (the staging entry is free again after this: no event needed until the import launch)
    for (int32_t i = 0; i < n; ++i) {
        const uint32_t bad = s->chk_host.get()[i];
        if (bad == 0) continue;
        std::string who = "dn_sessions_import: record " + std::to_string(i) + " (for slot " + std::to_string(ids[i]) + ")";
        if (bad == dn::kSessRecBadMagic) return fail(DN_ERR_INVALID, who + " is not a session record (bad magic)");
        dn_session_record_header h{};
        DN_HIP(hipMemcpy(&h, static_cast<const char*>(records) + (size_t)i * r.stride, sizeof(h), hipMemcpyDeviceToHost));
        if (bad == dn::kSessRecBadVersion)
            return fail(DN_ERR_INVALID, who + " has record version " + std::to_string(h.version) + ", this library reads version " +
                                            std::to_string(DN_SESS_RECORD_VERSION));
        if (bad == dn::kSessRecBadGeometry)
            return fail(DN_ERR_INVALID, who + " has geometry " + sess_geometry(h.sample_rate, h.n_fft, h.hop, h.n_mels, h.hidden, h.C) +
                                            "; this pool's is " + sess_geometry(r.want.sample_rate, r.want.n_fft, r.want.hop, r.want.n_mels,
                                                                                 r.want.hidden, r.want.C));
        return fail(DN_ERR_INVALID, who + " has priming count " + std::to_string(h.pushes) + " > n_fft/hop - 1 = " + std::to_string(r.prime));
    }
    dn::launch_sess_import(a, r, s->d->cfg.n_fft, records, sids_dev, st);
    DN_TRY(check_launch("sess_import_kernel"));
    for (int32_t i = 0; i < n; ++i) s->open[ids[i]] = 1;
    return sess_staged(s, st);
}

int dn_sessions_get_counters(dn_sessions* s, int32_t id, uint64_t* frames, int32_t* pushes, void* stream) {
    if (!s) return fail(DN_ERR_INVALID, "dn_sessions_get_counters: null pool");
    if (id < 0 || id >= s->cap) return fail(DN_ERR_INVALID, "dn_sessions_get_counters: id out of range");
    const dn::SessArgs a = sess_args(s);
    unsigned long long f = 0;
    unsigned int p = 0;
    hipStream_t st = as_stream(stream);
    DN_HIP(hipMemcpyAsync(&f, a.frames + id, sizeof(f), hipMemcpyDeviceToHost, st));
    DN_HIP(hipMemcpyAsync(&p, a.pushes + id, sizeof(p), hipMemcpyDeviceToHost, st));
    DN_HIP(hipStreamSynchronize(st));
    if (frames) *frames = f;
    if (pushes) *pushes = (int32_t)p;
    return DN_OK;
}

}  // extern "C"
