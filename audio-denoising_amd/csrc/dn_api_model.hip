// dn_api_model.hip -- dn_model: host-side packing of the reference's tensors into kernel-friendly layouts (MFMA weight fragments, the
// position-code bias tables), and the stand-alone cell entry points.  No kernel code here.
#include <math.h>

#include "dn_host.hpp"

namespace {

// state_dict order, SURVEY.md Appendix A.4 (offsets in floats)
struct StateLayout {
    size_t dw[4], db[4], off_in, gw, gb, off_rs, uw[4], ub[4], off_out, total;
    StateLayout() {
        size_t o = 0;
        const int dco[4] = {17, 17, 17, 51}, dci[4] = {7, 23, 23, 23};
        for (int l = 0; l < 4; ++l) { dw[l] = o; o += (size_t)dco[l] * dci[l] * 3; db[l] = o; o += dco[l]; }
        off_in = o; o += 6;
        gw = o; o += 51 * 23 * 3; gb = o; o += 51;
        off_rs = o; o += 6;
        const int uci[4] = {23, 40, 40, 40}, uco[4] = {17, 17, 17, 1};
        for (int l = 0; l < 4; ++l) { uw[l] = o; o += (size_t)uci[l] * uco[l] * 3; ub[l] = o; o += uco[l]; }
        off_out = o; o += 6;
        total = o;
    }
};

// torch.linspace(0, 1, n) in fp32 (symmetric two-sided formula of the CPU kernel)
std::vector<float> linspace01(int n) {
    std::vector<float> v(n);
    if (n == 1) { v[0] = 0.0f; return v; }
    const float step = 1.0f / (float)(n - 1);
    const int half = n / 2;
    for (int i = 0; i < n; ++i) v[i] = i < half ? 0.0f + step * (float)i : 1.0f - step * (float)(n - 1 - i);
    return v;
}

// GaussianSmearing table S[g][l], gruunet2.py:54-68 on linspace(0,1,L).  The reference fixes `coeff` at construction from its own
// linspace(0, 1, num_gaussians) (gruunet2.py:62-63) and never recomputes it after load_state_dict: only `dist - offset` uses the
// loaded buffer.
std::vector<float> smear_table(const float* offset, int L) {
    const std::vector<float> o6 = linspace01(dn::kGauss);
    const float diff = o6[1] - o6[0];
    const double coeff = -0.5 / ((double)diff * (double)diff);
    const float cf = (float)coeff;
    std::vector<float> pos = linspace01(L), s((size_t)dn::kGauss * L);
    for (int g = 0; g < dn::kGauss; ++g)
        for (int l = 0; l < L; ++l) {
            const float d = pos[l] - offset[g];
            s[(size_t)g * L + l] = expf(cf * (d * d));
        }
    return s;
}

// The bias tables: the six position-code channels of every conv see the same input at every step, so their contribution is folded into a
// per-position bias bt[o][j] (accumulated in double).
// encoder level l: Lin = F >> l, Lout = Lin/2, stride 2, left pad 1
std::vector<float> bias_down(const float* W, const StateLayout& sl, int l, int F) {
    const int cd = l == 0 ? 1 : 17, ct = cd + 6, co = l == 3 ? 51 : 17;
    const int lin = F >> l, lout = lin / 2;
    std::vector<float> S = smear_table(W + sl.off_in, lin), bt((size_t)co * lout);
    for (int o = 0; o < co; ++o)
        for (int j = 0; j < lout; ++j) {
            double acc = W[sl.db[l] + o];
            for (int g = 0; g < 6; ++g)
                for (int k = 0; k < 3; ++k) {
                    const int p = 2 * j - 1 + k;
                    if (p >= 0 && p < lin) acc += (double)W[sl.dw[l] + ((size_t)o * ct + cd + g) * 3 + k] * S[(size_t)g * lin + p];
                }
            bt[(size_t)o * lout + j] = (float)acc;
        }
    return bt;
}

// hidden gates: stride 1, pad 1 on both sides, length C
std::vector<float> bias_gates(const float* W, const StateLayout& sl, int C) {
    std::vector<float> S = smear_table(W + sl.off_rs, C), bt((size_t)51 * C);
    for (int o = 0; o < 51; ++o)
        for (int p = 0; p < C; ++p) {
            double acc = W[sl.gb + o];
            for (int g = 0; g < 6; ++g)
                for (int k = 0; k < 3; ++k) {
                    const int q = p - 1 + k;
                    if (q >= 0 && q < C) acc += (double)W[sl.gw + ((size_t)o * 23 + 17 + g) * 3 + k] * S[(size_t)g * C + q];
                }
            bt[(size_t)o * C + p] = (float)acc;
        }
    return bt;
}

// decoder level l: Lin = C << l, Lout = 2 Lin; output j = 2 i - 1 + k
std::vector<float> bias_up(const float* W, const StateLayout& sl, int l, int C) {
    const int cd = l == 0 ? 17 : 34, co = l == 3 ? 1 : 17;
    const int lin = C << l, lout = 2 * lin;
    std::vector<float> S = smear_table(W + sl.off_out, lin), bt((size_t)co * lout);
    for (int o = 0; o < co; ++o)
        for (int j = 0; j < lout; ++j) {
            double acc = W[sl.ub[l] + o];
            for (int g = 0; g < 6; ++g)
                for (int k = 0; k < 3; ++k) {
                    const int num = j + 1 - k;          // 2 i
                    if (num < 0 || (num & 1)) continue;
                    const int i = num >> 1;
                    if (i < lin) acc += (double)W[sl.uw[l] + ((size_t)(cd + g) * co + o) * 3 + k] * S[(size_t)g * lin + i];
                }
            bt[(size_t)o * lout + j] = (float)acc;
        }
    return bt;
}

// MFMA A fragments (v_mfma_f32_16x16x4_f32): lane l of k-step ks supplies W[o = 16 mt + (l & 15)][K slot 4 ks + (l >> 4)].
// Conv1d weight (Cout, Ct, 3) of encoder level l: K order tap-major, channels in fours -> [mt][ks][64].  In front of the last, partial row tile
// (channel 16; rows 48..50 of the 51-row level) lies the table of the same rows for the VALU lanes that compute them (dn_cell_body.hpp: rows_down):
// [row][ks] float4 = the weights of the four K slots of k-step ks, zero-padded to whole 256-byte lines.
std::vector<float> pack_down(const float* W, const StateLayout& sl, int l) {
    const int cd = l == 0 ? 1 : 17, ct = cd + 6, co = l == 3 ? 51 : 17;
    const int cs = (cd + 3) / 4, ks_n = cd == 1 ? 1 : 3 * cs, mtiles = (co + 15) / 16;
    const int rows = co % 16, row0 = co - rows, rt = dn::cell_rowtab_floats(rows, ks_n);
    const auto weight = [&](int o, int ks, int q) {
        const int tap = cd == 1 ? q : ks / cs, c = cd == 1 ? 0 : 4 * (ks % cs) + q;
        return o < co && tap < 3 && c < cd ? W[sl.dw[l] + ((size_t)o * ct + c) * 3 + tap] : 0.0f;
    };
    std::vector<float> p((size_t)mtiles * ks_n * 64 + rt, 0.0f);
    for (int mt = 0; mt < mtiles; ++mt)
        for (int ks = 0; ks < ks_n; ++ks)
            for (int ln = 0; ln < 64; ++ln)
                p[((size_t)mt * ks_n + ks) * 64 + ln + (mt == mtiles - 1 ? rt : 0)] = weight(mt * 16 + (ln & 15), ks, ln >> 4);
    for (int r = 0; r < rows; ++r)
        for (int ks = 0; ks < ks_n; ++ks)
            for (int q = 0; q < 4; ++q) p[(size_t)(mtiles - 1) * ks_n * 64 + ((size_t)r * ks_n + ks) * 4 + q] = weight(row0 + r, ks, q);
    return p;
}

// hidden-gate conv (51, 17 data channels, 3) as A fragments too: [mt 4][ks 13][64], K slot = 3 c + tap (51 slots + 1 zero)
std::vector<float> pack_gates(const float* W, const StateLayout& sl) {
    std::vector<float> p((size_t)4 * 13 * 64, 0.0f);
    for (int mt = 0; mt < 4; ++mt)
        for (int ks = 0; ks < 13; ++ks)
            for (int ln = 0; ln < 64; ++ln) {
                const int o = mt * 16 + (ln & 15), kk = 4 * ks + (ln >> 4), c = kk / 3, k = kk % 3;
                if (o < 51 && c < 17) p[((size_t)mt * 13 + ks) * 64 + ln] = W[sl.gw + ((size_t)o * 23 + c) * 3 + k];
            }
    return p;
}

constexpr int kTapOfSet[3] = {1, 2, 0};

// ConvTranspose1d weight (Ct, Cout, 3) of decoder level l -> [mt][tap set: k=1,k=2,k=0][ks][64], parts of 17 channels in fours
std::vector<float> pack_up(const float* W, const StateLayout& sl, int l) {
    if (l == 3) {   // the last level (one output channel) runs on the VALU: [part: a, skip][17 channels][4] = w[k=1], w[k=2], w[k=0], 0
        std::vector<float> p((size_t)2 * 17 * 4, 0.0f);
        for (int part = 0; part < 2; ++part)
            for (int c = 0; c < 17; ++c)
                for (int set = 0; set < 3; ++set) p[((size_t)part * 17 + c) * 4 + set] = W[sl.uw[3] + ((size_t)(part * 17 + c)) * 3 + kTapOfSet[set]];
        return p;
    }
    // in front of the second row tile (channel 16): that channel's table for rows_up, [ks][tap set] float4 = the four K slots of k-step ks
    const int parts = l == 0 ? 1 : 2, co = 17, ksu = parts * 5, mtiles = (co + 15) / 16, rt = dn::cell_rowtab_floats(1, 3 * ksu);
    const auto weight = [&](int o, int set, int ks, int q) {
        const int cp = 4 * (ks % 5) + q, c = (ks / 5) * 17 + cp;
        return o < co && cp < 17 ? W[sl.uw[l] + ((size_t)c * co + o) * 3 + kTapOfSet[set]] : 0.0f;
    };
    std::vector<float> p((size_t)mtiles * 3 * ksu * 64 + rt, 0.0f);
    for (int mt = 0; mt < mtiles; ++mt)
        for (int set = 0; set < 3; ++set)
            for (int ks = 0; ks < ksu; ++ks)
                for (int ln = 0; ln < 64; ++ln)
                    p[(((size_t)mt * 3 + set) * ksu + ks) * 64 + ln + (mt == mtiles - 1 ? rt : 0)] = weight(mt * 16 + (ln & 15), set, ks, ln >> 4);
    for (int ks = 0; ks < ksu; ++ks)
        for (int set = 0; set < 3; ++set)
            for (int q = 0; q < 4; ++q) p[(size_t)(mtiles - 1) * 3 * ksu * 64 + ((size_t)ks * 3 + set) * 4 + q] = weight(16, set, ks, q);
    return p;
}

// bf16 fragments for v_mfma_f32_16x16x32_bf16 (config 3): lane l of k-step ks supplies 8 consecutive K slots
// 8 (l >> 4) + j = channels of one tap (level 0: the taps themselves); round to nearest even.
uint16_t bf16(float f) {
    uint32_t u; memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

std::vector<uint16_t> pack_down_bf16(const float* W, const StateLayout& sl, int l) {
    const int cd = l == 0 ? 1 : 17, ct = cd + 6, co = l == 3 ? 51 : 17, ks_n = cd == 1 ? 1 : 3, mtiles = (co + 15) / 16;
    std::vector<uint16_t> p((size_t)mtiles * ks_n * 64 * 8, 0);
    for (int mt = 0; mt < mtiles; ++mt)
        for (int ks = 0; ks < ks_n; ++ks)
            for (int ln = 0; ln < 64; ++ln)
                for (int j = 0; j < 8; ++j) {
                    const int o = mt * 16 + (ln & 15), q = ln >> 4;
                    const int tap = cd == 1 ? j : ks, c = cd == 1 ? 0 : 8 * q + j;
                    const bool ok = o < co && (cd == 1 ? (q == 0 && j < 3) : c < cd);
                    if (ok) p[(((size_t)mt * ks_n + ks) * 64 + ln) * 8 + j] = bf16(W[sl.dw[l] + ((size_t)o * ct + c) * 3 + tap]);
                }
    return p;
}

std::vector<uint16_t> pack_up_bf16(const float* W, const StateLayout& sl, int l) {
    const int parts = l == 0 ? 1 : 2, co = 17;
    std::vector<uint16_t> p((size_t)2 * 3 * parts * 64 * 8, 0);
    for (int mt = 0; mt < 2; ++mt)
        for (int set = 0; set < 3; ++set)
            for (int part = 0; part < parts; ++part)
                for (int ln = 0; ln < 64; ++ln)
                    for (int j = 0; j < 8; ++j) {
                        const int o = mt * 16 + (ln & 15), cp = 8 * (ln >> 4) + j, c = part * 17 + cp;
                        if (o < co && cp < 17)
                            p[((((size_t)mt * 3 + set) * parts + part) * 64 + ln) * 8 + j] = bf16(W[sl.uw[l] + ((size_t)c * co + o) * 3 + kTapOfSet[set]]);
                    }
    return p;
}

}  // namespace

int build_bias(const dn_model* m, int C, const BiasSet** out) {
    std::lock_guard<std::mutex> lock(m->mu);
    auto it = m->bias.find(C);
    if (it != m->bias.end()) { *out = it->second.get(); return DN_OK; }
    const StateLayout sl;
    const float* W = m->w.data();
    auto bs = std::make_unique<BiasSet>();
    size_t o_down[4], o_gh, o_up[4];
    for (int l = 0; l < 4; ++l) o_down[l] = bs->arena.add(bias_down(W, sl, l, 16 * C));
    o_gh = bs->arena.add(bias_gates(W, sl, C));
    for (int l = 0; l < 4; ++l) o_up[l] = bs->arena.add(bias_up(W, sl, l, C));
    hipError_t e = bs->arena.upload();
    if (e != hipSuccess) return fail(DN_ERR_HIP, std::string("bias table upload: ") + hipGetErrorString(e));
    for (int l = 0; l < 4; ++l) {
        bs->view.w_down[l] = m->packed.ptr<float>(m->off_down[l]);
        bs->view.w_up[l] = m->packed.ptr<float>(m->off_up[l]);
        bs->view.wb_down[l] = m->packed.ptr<char>(m->offb_down[l]);
        if (l < 3) bs->view.wb_up[l] = m->packed.ptr<char>(m->offb_up[l]);
        bs->view.bt_down[l] = bs->arena.ptr<float>(o_down[l]);
        bs->view.bt_up[l] = bs->arena.ptr<float>(o_up[l]);
    }
    bs->view.w_gh = m->packed.ptr<float>(m->off_gh);
    bs->view.bt_gh = bs->arena.ptr<float>(o_gh);
    e = bs->view_dev.alloc_copy(&bs->view, sizeof(bs->view));
    if (e != hipSuccess) return fail(DN_ERR_HIP, std::string("bias table view: ") + hipGetErrorString(e));
    *out = (m->bias[C] = std::move(bs)).get();
    return DN_OK;
}

namespace {

enum CellKind { kCellFp32, kCellEx, kCellBf16, kCellParentTiles };

int cell_forward(CellKind kind, const dn_model* m, const float* x, const float* hx_in, float* out, float* hx_out, int32_t B, int32_t T,
                 int32_t F, int32_t C, float hx_out_scale, void* stream) {
    static const char* const kWho[] = {"dn_cell_forward", "dn_cell_forward_ex", "dn_cell_forward_bf16", "dn_cell_forward_parent_tiles"};
    static const char* const kKernel[] = {"cell_kernel", "cell_kernel_ex", "cell_kernel_bf16", "cell_kernel (parent tiles)"};
    if (B == 0) return DN_OK;      // empty batch: nothing to do (pointers of empty tensors are null)
    if (!m || !x || !out || !hx_out) return fail(DN_ERR_INVALID, std::string(kWho[kind]) + ": null argument");
    if (B < 0 || T < 0) return fail(DN_ERR_INVALID, std::string(kWho[kind]) + ": negative size");
    if (C < 1 || C > dn::kMaxC) return fail(DN_ERR_UNSUPPORTED, "compressed bins C must be in 1.." + std::to_string(dn::kMaxC));
    if (F != 16 * C)
        return fail(DN_ERR_INVALID, kind != kCellFp32 ? std::string("need F == 16*C")
                                                      : "input has " + std::to_string(F) + " bins, which compress to " + std::to_string(F / 16) +
                                                            ", but hx has " + std::to_string(C) + " compressed bins (need F == 16*C)");
    const BiasSet* bs = nullptr;
    DN_TRY(build_bias(m, C, &bs));
    if (kind == kCellFp32) dn::launch_cell(bs->view, x, hx_in, out, hx_out, B, T, C, as_stream(stream));
    else if (kind == kCellParentTiles) dn::launch_cell_parent_tiles(bs->view, x, hx_in, out, hx_out, B, T, C, as_stream(stream));
    else if (kind == kCellEx) dn::launch_cell_ex(bs->view, x, hx_in, out, hx_out, B, T, C, hx_out_scale, as_stream(stream));
    else dn::launch_cell_bf16(bs->view, x, hx_in, out, hx_out, B, T, C, as_stream(stream));
    return check_launch(kKernel[kind]);
}

}  // namespace

extern "C" {

int dn_model_create(const float* weights, size_t n_floats, const dn_model_cfg* cfg, dn_model** out) {
    if (!weights || !cfg || !out) return fail(DN_ERR_INVALID, "dn_model_create: null argument");
    const StateLayout sl;
    if (cfg->in_size != 1) return fail(DN_ERR_INVALID, "in_size must be 1 (gruunet2.py:257)");
    if (cfg->n_levels != 4 || cfg->hidden_size != 17 || cfg->kernel_size != 3 || cfg->stride != 2 ||
        cfg->padding != 1 || cfg->num_gaussians != 6)
        return fail(DN_ERR_UNSUPPORTED, "kernels are built for 4 levels, hidden 17, k3 s2 p1, 6 gaussians");
    if (cfg->num_compressed_bins < 1 || cfg->num_compressed_bins > dn::kMaxC) return fail(DN_ERR_UNSUPPORTED, "num_compressed_bins must be in 1.." + std::to_string(dn::kMaxC));
    if (n_floats != sl.total) return fail(DN_ERR_INVALID, "expected " + std::to_string(sl.total) + " weight floats, got " + std::to_string(n_floats));
    std::unique_ptr<dn_model> m(new dn_model());
    m->cfg = *cfg;
    m->w.assign(weights, weights + n_floats);
    const float* W = m->w.data();
    for (int l = 0; l < 4; ++l) m->off_down[l] = m->packed.add(pack_down(W, sl, l));
    m->off_gh = m->packed.add(pack_gates(W, sl));
    for (int l = 0; l < 4; ++l) m->off_up[l] = m->packed.add(pack_up(W, sl, l));
    for (int l = 0; l < 4; ++l) m->offb_down[l] = m->packed.add(pack_down_bf16(W, sl, l));
    for (int l = 0; l < 3; ++l) m->offb_up[l] = m->packed.add(pack_up_bf16(W, sl, l));
    hipError_t e = m->packed.upload();
    if (e != hipSuccess) return fail(DN_ERR_HIP, std::string("weight upload: ") + hipGetErrorString(e));
    const BiasSet* bs = nullptr;
    DN_TRY(build_bias(m.get(), cfg->num_compressed_bins, &bs));
    *out = m.release();
    return DN_OK;
}

// Drops the creator's reference; the device arenas are freed once no dn_pipe or dn_sessions is bound to the model any more.
void dn_model_destroy(dn_model* m) { Ref<dn_model>::drop(m); }

int dn_cell_forward(const dn_model* m, const float* x, const float* hx_in, float* out, float* hx_out, int32_t B, int32_t T, int32_t F, int32_t C, void* stream) {
    return cell_forward(kCellFp32, m, x, hx_in, out, hx_out, B, T, F, C, 0.0f, stream);
}

int dn_cell_forward_ex(const dn_model* m, const float* x, const float* hx_in, float* out, float* hx_out, int32_t B, int32_t T, int32_t F, int32_t C, float hx_out_scale, void* stream) {
    return cell_forward(kCellEx, m, x, hx_in, out, hx_out, B, T, F, C, hx_out_scale, stream);
}

int dn_cell_forward_bf16(const dn_model* m, const float* x, const float* hx_in, float* out, float* hx_out, int32_t B, int32_t T, int32_t F, int32_t C, void* stream) {
    return cell_forward(kCellBf16, m, x, hx_in, out, hx_out, B, T, F, C, 0.0f, stream);
}

// dn_cell_forward on the conv tiles as they were before the live-row / lane-geometry change (dn_cell_body.hpp: TILES = 0).  For comparisons (tests,
// tools/): declared in dn_internal.hpp, not part of include/dn_denoise.h, and nothing in the product calls it.
int dn_cell_forward_parent_tiles(const dn_model* m, const float* x, const float* hx_in, float* out, float* hx_out, int32_t B, int32_t T, int32_t F, int32_t C, void* stream) {
    return cell_forward(kCellParentTiles, m, x, hx_in, out, hx_out, B, T, F, C, 0.0f, stream);
}

}  // extern "C"
