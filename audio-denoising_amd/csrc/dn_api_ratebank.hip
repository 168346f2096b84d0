// dn_api_ratebank.hip -- dn_ratebank: the rate adapters of a session pool (kernels: dn_ratebank.hip).  The tables and geometries are
// dn_resample_create's (resample_design, resample_hann_table); this unit adds the accepted-rate rule, the argument checks and the staging of a
// call's (slot, rate) pairs.  No kernel code here.
#include "dn_host.hpp"

namespace {

const char* const kRule = "; a session rate is accepted when both directions lie inside the small kernel form (n <= 4, o <= 8, n x taps <= 512), tile the hop "
                          "(n_d | hop, o_u | hop), bring a history per hop (chunk_in >= H) and fit the staged tile (chunk_in <= 1536)";

int unsupported(int rate, const std::string& why) {
    return fail(DN_ERR_UNSUPPORTED, "dn_ratebank_create: rate " + std::to_string(rate) + " " + why + kRule);
}

std::string pair_of(const ResampleDesign& g) { return std::to_string(g.o) + " : " + std::to_string(g.n); }

// one direction of a session rate against one condition of the accepted-rate rule (0: tiles the hop, 1: the small form, 2: a history per hop,
// 3: the staged tile).  The conditions are walked in that order over both directions, so the message names the first one a rate fails.
int check_side(const dn_ratebank_cfg& c, int rate, bool up, const ResampleDesign& g, int cond) {
    const std::string dir = (up ? "up (plan -> session, " : "down (session -> plan, ") + pair_of(g) + ")";
    const int per = up ? g.o : g.n;          // plan-rate samples of a block
    if (cond == 0)
        return c.hop % per == 0 ? DN_OK : unsupported(rate, dir + " does not tile a hop of " + std::to_string(c.hop) + ": " + (up ? "o_u = " : "n_d = ") +
                                                                std::to_string(per) + " does not divide it");
    if (cond == 1)
        return g.small() ? DN_OK : unsupported(rate, dir + " is outside the small kernel form: " + (up ? "n_u = " : "n_d = ") + std::to_string(g.n) + ", " +
                                                         (up ? "o_u = " : "o_d = ") + std::to_string(g.o) + ", table " + std::to_string(g.n) + " x " + std::to_string(g.KW));
    const int chunk = c.hop / per * g.o;
    if (cond == 2)
        return chunk >= g.H ? DN_OK : unsupported(rate, dir + " brings " + std::to_string(chunk) + " samples a hop, fewer than its history H = " + std::to_string(g.H));
    return chunk <= dn::kRbMaxChunk && g.H <= dn::kRbMaxHist
               ? DN_OK
               : unsupported(rate, dir + " brings " + std::to_string(chunk) + " samples a hop with a history of " + std::to_string(g.H) +
                                       ", more than the staged tile of " + std::to_string(dn::kRbMaxChunk) + " + " + std::to_string(dn::kRbMaxHist));
}

// an accepted direction: its kernel geometry, and its table appended to `tables`
void add_side(const dn_ratebank_cfg& c, bool up, const ResampleDesign& g, dn::RateBankRate* out, int* D, std::vector<float>& tables) {
    out->o = g.o; out->n = g.n; out->KW = g.KW; out->H = g.H; out->blocks = c.hop / (up ? g.o : g.n);
    out->table = (int)tables.size();
    *D = g.D;
    const std::vector<float> k = resample_hann_table(g, c.lowpass_filter_width);
    tables.insert(tables.end(), k.begin(), k.end());
    tables.resize((tables.size() + 3) & ~size_t(3));
}

int chunk_of(const dn_ratebank* b, int side, int rate, bool in) {      // samples a row of that rate index reads (in) or writes on that side
    if (rate < 0) return b->cfg.hop;
    const dn::RateBankRate& g = b->side[side][rate];
    return g.blocks * (in ? g.o : g.n);
}

// the checks both calls share (`stride` is x_stride on the way in, y_stride on the way out), then the pairs staged and the arguments filled
int prepare(dn_ratebank* b, const char* who_, int side, const int32_t* slots, const int32_t* rate_idx, int32_t n, int32_t capacity, float* state,
            const void* in, void* out, int64_t stride, bool stride_is_in, dn::RateBankArgs& a) {
    const std::string who = who_;
    if (!b) return fail(DN_ERR_INVALID, who + ": null bank");
    if (n < 0) return fail(DN_ERR_INVALID, who + ": negative count");
    if (capacity < 1) return fail(DN_ERR_INVALID, who + ": capacity must be positive");
    if (n > capacity) return fail(DN_ERR_INVALID, who + ": " + std::to_string(n) + " rows for a state of " + std::to_string(capacity) + " slots");
    if (!slots || !rate_idx || !state || !in || !out) return fail(DN_ERR_INVALID, who + ": null argument");
    if ((size_t)capacity > b->seen.size()) b->seen.resize(capacity, 0);
    int rc = DN_OK, longest = 0;
    int32_t i = 0;
    for (; i < n; ++i) {
        const int32_t s = slots[i], r = rate_idx[i];
        if (s < 0 || s >= capacity) { rc = fail(DN_ERR_INVALID, who + ": slot " + std::to_string(s) + " (position " + std::to_string(i) + ") is out of range [0, " + std::to_string(capacity) + ")"); break; }
        if (b->seen[s]) { rc = fail(DN_ERR_INVALID, who + ": slot " + std::to_string(s) + " appears twice in the list"); break; }
        if (r < -1 || r >= b->n_rates) { rc = fail(DN_ERR_INVALID, who + ": rate index " + std::to_string(r) + " (position " + std::to_string(i) + ") is out of range [-1, " + std::to_string(b->n_rates) + ")"); break; }
        b->seen[s] = 1;
        longest = std::max(longest, chunk_of(b, side, r, stride_is_in));
    }
    for (int32_t j = 0; j < i; ++j) b->seen[slots[j]] = 0;
    DN_TRY(rc);
    if (stride < longest)
        return fail(DN_ERR_INVALID, who + ": " + (stride_is_in ? "x_stride " : "y_stride ") + std::to_string(stride) + " is shorter than the longest listed chunk, " + std::to_string(longest) + " samples");
    if ((size_t)n > b->ring_rows) {          // a longer list than any before: a larger ring, once the launches that read the old one are through
        b->ring.drain();
        const size_t rows = std::max<size_t>(256, 2 * (size_t)n);
        const hipError_t e = b->ring.create(rows * 2 * sizeof(int32_t));
        if (e != hipSuccess) { b->ring_rows = 0; return fail(DN_ERR_HIP, who + ": staging ring: " + hipGetErrorString(e)); }
        b->ring_rows = rows;
    }
    char* h = nullptr;
    const char* d = nullptr;
    DN_HIP(b->ring.next(&h, &d));
    int32_t* pairs = reinterpret_cast<int32_t*>(h);
    for (int32_t k = 0; k < n; ++k) { pairs[2 * k] = slots[k]; pairs[2 * k + 1] = rate_idx[k]; }
    a = dn::RateBankArgs{};
    a.state = state; a.state_stride = b->stride[side];
    a.rows = reinterpret_cast<const int*>(d);
    a.tables = b->tables;
    a.copy = b->cfg.hop;
    for (int k = 0; k < b->n_rates; ++k) a.r[k] = b->side[side][k];
    return DN_OK;
}

}  // namespace

extern "C" {

int dn_ratebank_create(const dn_ratebank_cfg* cfg, dn_ratebank** out) {
    if (!cfg || !out) return fail(DN_ERR_INVALID, "dn_ratebank_create: null argument");
    if (cfg->plan_rate < 1 || cfg->hop < 1) return fail(DN_ERR_INVALID, "dn_ratebank_create: the plan's rate and hop must be positive");
    if (cfg->n_rates < 1 || cfg->n_rates > dn::kRbMaxRates) return fail(DN_ERR_INVALID, "dn_ratebank_create: a bank holds 1 to " + std::to_string(dn::kRbMaxRates) + " rates");
    for (int i = 0; i < cfg->n_rates; ++i) {
        if (cfg->rates[i] < 1) return fail(DN_ERR_INVALID, "dn_ratebank_create: rates must be positive");
        if (cfg->rates[i] == cfg->plan_rate) return fail(DN_ERR_INVALID, "dn_ratebank_create: rate " + std::to_string(cfg->rates[i]) + " is the plan's own (rate index -1), it needs no table");
        for (int j = 0; j < i; ++j)
            if (cfg->rates[j] == cfg->rates[i]) return fail(DN_ERR_INVALID, "dn_ratebank_create: rate " + std::to_string(cfg->rates[i]) + " is listed twice");
    }
    std::unique_ptr<dn_ratebank> b(new dn_ratebank());
    b->cfg = *cfg;
    b->n_rates = cfg->n_rates;
    std::vector<float> tables;
    for (int i = 0; i < cfg->n_rates; ++i) {
        const int rate = cfg->rates[i];
        ResampleDesign g[2];
        DN_TRY(resample_design("dn_ratebank_create", rate, cfg->plan_rate, cfg->lowpass_filter_width, cfg->rolloff, &g[DN_RATEBANK_IN]));
        DN_TRY(resample_design("dn_ratebank_create", cfg->plan_rate, rate, cfg->lowpass_filter_width, cfg->rolloff, &g[DN_RATEBANK_OUT]));
        for (int cond = 0; cond < 4; ++cond)
            for (int side = 0; side < 2; ++side) DN_TRY(check_side(*cfg, rate, side == DN_RATEBANK_OUT, g[side], cond));
        for (int side = 0; side < 2; ++side) {
            add_side(*cfg, side == DN_RATEBANK_OUT, g[side], &b->side[side][i], &b->D[side][i], tables);
            b->stride[side] = std::max(b->stride[side], (b->side[side][i].H + 3) & ~3);
        }
    }
    const size_t off = b->arena.add(tables);
    const hipError_t e = b->arena.upload();
    if (e != hipSuccess) return fail(DN_ERR_HIP, std::string("dn_ratebank_create: upload: ") + hipGetErrorString(e));
    b->tables = b->arena.ptr<float>(off);
    *out = b.release();
    return DN_OK;
}

void dn_ratebank_destroy(dn_ratebank* b) {
    if (!b) return;
    b->ring.drain();
    delete b;
}

int dn_ratebank_geometry(const dn_ratebank* b, int32_t rate_index, int32_t* chunk_in, int32_t* chunk_out, int32_t* hist_in, int32_t* hist_out,
                         int32_t* delay_in, int32_t* delay_out) {
    if (!b) return fail(DN_ERR_INVALID, "dn_ratebank_geometry: null bank");
    if (rate_index < 0 || rate_index >= b->n_rates) return fail(DN_ERR_INVALID, "dn_ratebank_geometry: rate index out of range");
    const dn::RateBankRate& dn_ = b->side[DN_RATEBANK_IN][rate_index];
    const dn::RateBankRate& up = b->side[DN_RATEBANK_OUT][rate_index];
    if (chunk_in) *chunk_in = dn_.blocks * dn_.o;
    if (chunk_out) *chunk_out = up.blocks * up.n;
    if (hist_in) *hist_in = dn_.H;
    if (hist_out) *hist_out = up.H;
    if (delay_in) *delay_in = b->D[DN_RATEBANK_IN][rate_index] * dn_.n;
    if (delay_out) *delay_out = b->D[DN_RATEBANK_OUT][rate_index] * up.n;
    return DN_OK;
}

int32_t dn_ratebank_state_stride(const dn_ratebank* b, int32_t side) {
    return !b || (side != DN_RATEBANK_IN && side != DN_RATEBANK_OUT) ? 0 : b->stride[side];
}

int dn_ratebank_ingest(dn_ratebank* b, const int32_t* slots, const int32_t* rate_idx, int32_t n, int32_t capacity, float* state_in, const void* x,
                       int32_t in_s16, int64_t x_stride, float* hop_in, void* stream) {
    if (b && n == 0) return DN_OK;
    dn::RateBankArgs a;
    DN_TRY(prepare(b, "dn_ratebank_ingest", DN_RATEBANK_IN, slots, rate_idx, n, capacity, state_in, x, hop_in, x_stride, true, a));
    a.x = x; a.in_s16 = in_s16 != 0; a.x_stride = x_stride;
    a.y = hop_in; a.out_s16 = 0; a.y_stride = b->cfg.hop;
    hipStream_t st = as_stream(stream);
    dn::launch_ratebank(a, n, st);
    DN_TRY(check_launch("ratebank_kernel(ingest)"));
    DN_HIP(b->ring.staged(st));
    return DN_OK;
}

int dn_ratebank_emit(dn_ratebank* b, const int32_t* slots, const int32_t* rate_idx, int32_t n, int32_t capacity, float* state_out,
                     const float* hop_out, void* y, int32_t out_s16, int64_t y_stride, void* stream) {
    if (b && n == 0) return DN_OK;
    dn::RateBankArgs a;
    DN_TRY(prepare(b, "dn_ratebank_emit", DN_RATEBANK_OUT, slots, rate_idx, n, capacity, state_out, hop_out, y, y_stride, false, a));
    a.x = hop_out; a.in_s16 = 0; a.x_stride = b->cfg.hop;
    a.y = y; a.out_s16 = out_s16 != 0; a.y_stride = y_stride;
    hipStream_t st = as_stream(stream);
    dn::launch_ratebank(a, n, st);
    DN_TRY(check_launch("ratebank_kernel(emit)"));
    DN_HIP(b->ring.staged(st));
    return DN_OK;
}

}  // extern "C"
