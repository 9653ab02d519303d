// The four weight-stream packers (decoder_pack.h).
#include "decoder_pack.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

using namespace dsp;

// ------------------------------------------------------------------------------------------------
// decoder packing: weights -> chunk stream in MFMA operand order (see mlp_kernel.hip / DESIGN.md)
// ------------------------------------------------------------------------------------------------
namespace {

struct NetView {
    int n_layers, hidden, lat;
    int code_len = CODE_LEN, in_dim = IN_DIM;   // of the decoder (code_len 32 or 64)
    int width = WIDTH;                           // hidden width of the decoder (<= 512: narrower nets are embedded with zero rows / columns)
    std::vector<int> out_dims, in_dims;
    std::vector<const float*> w, b;
    // layer k: input-slab row -> original weight column (or -1).  The code columns of the latent_in layer are not part
    // of the forward stream (they are a per-object bias, k_code_bias) but their gradient rows 448..511 are produced by the
    // backward pass; layer 0 never goes through the forward stream at all and only its 64 code rows through the backward one.
    int lat_row0() const { return WIDTH - in_dim; }
    std::vector<int> colmap(int k, bool backward) const {
        std::vector<int> m(WIDTH, -1);
        if (k == 0) {
            if (backward) for (int r = 0; r < code_len; ++r) m[r] = r;
        } else if (k == lat) {
            const int p = lat_row0();                                        // slab row of x: 445 (code_len 64) or 477 (32)
            const int hr = width - in_dim;                                   // rows of the previous layer's output
            for (int r = 0; r < hr; ++r) m[r] = r;
            for (int r = 0; r < 3; ++r) m[p + r] = hr + code_len + r;        // xyz re-injected at slab rows p .. p+2
            if (backward) for (int r = 0; r < code_len; ++r) m[p + 3 + r] = hr + r;   // code gradient rows p+3 ..
        } else {
            for (int r = 0; r < in_dims[k]; ++r) m[r] = r;
        }
        return m;
    }
};

template <class F>
void pack_pass(std::vector<float>& stream, int nog, int nchunks, F value) {
    const size_t base = stream.size();
    stream.resize(base + (size_t)nog * nchunks * (CHUNK_BYTES / 4));
    float* dst = stream.data() + base;
    for (int og = 0; og < nog; ++og)
        for (int c = 0; c < nchunks; ++c) {
            float* ch = dst + ((size_t)og * nchunks + c) * (CHUNK_BYTES / 4);
            for (int sl = 0; sl < KSTEPS_PER_CHUNK; ++sl)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const int s = KSTEPS_PER_CHUNK * c + sl;
                        const int krow = 16 * (s >> 2) + 4 * (lane >> 4) + (s & 3);
                        const int orow = 64 * og + 16 * j + (lane & 15);
                        ch[(sl * 64 + lane) * 4 + j] = value(orow, krow);
                    }
        }
}

}  // namespace

namespace dsp_host {

void pack_decoder_host(PackedNet* h, const dsp_decoder_desc* d) {
    NetView nv;
    nv.n_layers = d->n_layers;
    nv.hidden = d->n_layers - 1;
    nv.lat = d->latent_in;
    if (d->code_len != 64 && d->code_len != 32) throw std::invalid_argument("code_len must be 64 or 32");
    if (nv.hidden < 2 || nv.hidden > 8) throw std::invalid_argument("need 2..8 hidden layers");
    if (nv.lat < 2 || nv.lat >= nv.hidden) throw std::invalid_argument("latent_in must name one hidden layer >= 2");
    nv.code_len = d->code_len;
    nv.in_dim = d->code_len + 3;
    nv.width = d->out_dims[0];
    // Narrower decoders run embedded in the 512-row slabs (zero rows / columns: an fmaf with a zero weight leaves the accumulator
    // unchanged, so the results are those of a kernel built for the narrow width).  The re-injected input of the latent_in layer
    // sits at fixed slab rows (445.. or 477..), so the previous layer's output must end below them.
    if (nv.width < 16 || nv.width > WIDTH || nv.width % 16) throw std::invalid_argument("hidden width must be a multiple of 16, at most 512");
    if (nv.width - nv.in_dim > nv.lat_row0()) throw std::invalid_argument("hidden width too large for this code length");
    for (int k = 0; k < d->n_layers; ++k) {
        nv.out_dims.push_back(d->out_dims[k]);
        nv.in_dims.push_back(d->in_dims[k]);
        nv.w.push_back(d->weights[k]);
        nv.b.push_back(d->biases[k]);
        const int want_in = (k == 0) ? nv.in_dim : nv.width;
        const int want_out = (k == nv.hidden) ? 1 : (k + 1 == nv.lat ? nv.width - nv.in_dim : nv.width);
        if (d->in_dims[k] != want_in || d->out_dims[k] != want_out)
            throw std::invalid_argument("unsupported decoder geometry (one hidden width, input code_len + 3, output 1, one latent_in layer)");
    }
    h->lat_tile = nv.lat_row0() / 16;
    h->code_len = nv.code_len;
    std::vector<float>& stream = h->stream;
    std::vector<float>& bias = h->bias;
    stream.clear();
    bias.assign((size_t)(nv.hidden + 3) * WIDTH, 0.f);
    memset(h->pass, 0, sizeof h->pass);
    int np = 0, chunk = 0;
    // forward passes (layer 0 is evaluated on the VALU from the per-object code bias + the xyz columns)
    for (int k = 1; k < nv.hidden; ++k) {
        const std::vector<int> cm = nv.colmap(k, false);
        const int od = nv.out_dims[k], id = nv.in_dims[k];
        const float* W = nv.w[k];
        PassDesc& p = h->pass[np++];
        p.nog = (int16_t)((std::max(od, 1) + 63) / 64);
        p.nchunks = (int16_t)(k == nv.lat ? (nv.lat_row0() + 3 + 63) / 64 : 8);          // latent_in: K = 445 + 3 rows (7 chunks) or 477 + 3 (8)
        p.bias_row = (int16_t)(k == nv.lat ? -2 : k - 1);    // -2: per-object bias (code contribution + b_lat)
        p.relu = 1;
        p.mask_slot = (int16_t)k;
        p.kind = (int16_t)(k == nv.lat ? 2 : 1);
        p.chunk_base = chunk;
        pack_pass(stream, p.nog, p.nchunks, [&](int orow, int krow) -> float {
            if (orow >= od || krow >= WIDTH || cm[krow] < 0) return 0.f;
            return W[(size_t)orow * id + cm[krow]];
        });
        chunk += p.nog * p.nchunks;
        if (k != nv.lat) for (int o = 0; o < od; ++o) bias[(size_t)(k - 1) * WIDTH + o] = nv.b[k][o];
    }
    h->n_fwd = np;
    h->chunks_fwd = chunk;
    h->wlast_row = nv.hidden - 1;
    h->w0_row = nv.hidden;
    for (int o = 0; o < nv.width; ++o) bias[(size_t)h->wlast_row * WIDTH + o] = nv.w[nv.hidden][o];
    for (int c3 = 0; c3 < 3; ++c3)
        for (int o = 0; o < nv.width; ++o) bias[(size_t)(h->w0_row + c3) * WIDTH + o] = nv.w[0][(size_t)o * nv.in_dim + nv.code_len + c3];
    h->b_last = nv.b[nv.hidden][0];
    h->n_bias_rows = nv.hidden + 3;
    // code columns of layer 0 and of the latent_in layer, for the per-object bias
    h->codew.assign((size_t)2 * WIDTH * CODE_LEN, 0.f);
    h->b0.assign(WIDTH, 0.f);
    h->blat.assign(WIDTH, 0.f);
    std::copy(nv.b[0], nv.b[0] + nv.width, h->b0.begin());
    std::copy(nv.b[nv.lat], nv.b[nv.lat] + nv.width, h->blat.begin());
    for (int o = 0; o < nv.width; ++o)
        for (int c = 0; c < nv.code_len; ++c) {       // code columns beyond code_len stay zero: the optimiser carries 64-entry codes
            h->codew[(size_t)o * CODE_LEN + c] = nv.w[0][(size_t)o * nv.in_dim + c];
            h->codew[(size_t)(WIDTH + o) * CODE_LEN + c] = nv.w[nv.lat][(size_t)o * nv.width + (nv.width - nv.in_dim) + c];
        }
    // backward passes (transposed weights): output rows = the forward layer's INPUT slab rows
    for (int k = nv.hidden - 1; k >= 0; --k) {
        const std::vector<int> cm = nv.colmap(k, true);
        const int od = nv.out_dims[k], id = nv.in_dims[k];
        const float* W = nv.w[k];
        PassDesc& p = h->pass[np++];
        p.nog = (int16_t)(k == 0 ? 1 : 8);                   // layer 0: only the 64 code rows (xyz on the VALU)
        p.nchunks = (int16_t)((od + 63) / 64);
        p.bias_row = -1;
        p.relu = 0;
        p.mask_slot = (int16_t)(k - 1);
        p.kind = (int16_t)(k == nv.lat ? 4 : (k == 0 ? 5 : 3));
        p.chunk_base = chunk;
        pack_pass(stream, p.nog, p.nchunks, [&](int orow, int krow) -> float {
            if (krow >= od || orow >= WIDTH || cm[orow] < 0) return 0.f;
            return W[(size_t)krow * id + cm[orow]];
        });
        chunk += p.nog * p.nchunks;
    }
    h->n_pass_all = np;
    h->chunks_all = chunk;
}

}  // namespace dsp_host

namespace {

// ---- low-precision prepass stream (mlp_lp_kernel.hip) --------------------------------------------------------------------
uint16_t lp_bits(float v, bool bf) {      // fp32 -> f16 / bf16 bits, round to nearest even (= v_cvt_pk_{f16,bf16}_f32)
    uint16_t r;
    if (bf) {
        uint32_t u;
        memcpy(&u, &v, 4);
        u += 0x7fffu + ((u >> 16) & 1u);
        r = (uint16_t)(u >> 16);
    } else {
        const _Float16 h = (_Float16)v;
        memcpy(&r, &h, 2);
    }
    return r;
}
float lp_value(uint16_t b, bool bf) {
    if (bf) { const uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }
    _Float16 h;
    memcpy(&h, &b, 2);
    return (float)h;
}
// part p (1..3) of the split w = w1 + w2 + w3 (each a 16-bit value)
float lp_part(float w, int p, bool bf) {
    const float w1 = lp_value(lp_bits(w, bf), bf);
    if (p == 1) return w1;
    const float w2 = lp_value(lp_bits(w - w1, bf), bf);
    if (p == 2) return w2;
    return lp_value(lp_bits(w - w1 - w2, bf), bf);
}

}  // namespace

namespace dsp_host {

// Returns false when the decoder's geometry is outside what mlp_lp_kernel<*, 4> is built for (the prepass is then off and
// every sample goes through the fp32 kernel, as in round 1).
bool pack_decoder_lp_host(PackedLp* out, const dsp_decoder_desc* d, bool bf) {
    const int hidden = d->n_layers - 1, lat = d->latent_in;
    constexpr int NCH = 4, NOG = 2 * NCH;
    if (hidden < 2 || hidden > LP_MAX_PASSES || lat < 2 || lat >= hidden) return false;
    if (hidden & 1) return false;      // the kernel's last-layer body reads slab X: an even number of passes (DeepSDF's 8)
    const int in_dim = d->code_len + 3, width = d->out_dims[0];            // narrower nets are embedded with zero rows / columns
    if (width < 16 || width > WIDTH) return false;
    for (int k = 0; k < d->n_layers; ++k) {
        const int want_in = k == 0 ? in_dim : width;
        const int want_out = k == hidden ? 1 : (k + 1 == lat ? width - in_dim : width);
        if (d->in_dims[k] != want_in || d->out_dims[k] != want_out) return false;
    }
    const int lat_rows = width - in_dim;                                  // slab rows of the latent_in layer (445 / 477 for width 512)
    const int lat_ksteps = (lat_rows + 15) / 16;
    const int xyz0 = LP_KSTEPS_PER_CHUNK * NCH - LP_XYZ_KSTEPS;           // first xyz k-step of the latent_in layer
    if (lat_ksteps > xyz0) return false;
    const int tsel = bf ? 1 : 0;
    out->stream.clear();
    memset(out->pass, 0, sizeof out->pass);
    int chunk = 0;
    for (int k = 0; k < hidden; ++k) {
        LpPass& p = out->pass[k];
        const int od = d->out_dims[k], id = d->in_dims[k];
        const float* W = d->weights[k];
        p.kind = (int16_t)(k == 0 ? 0 : (k == lat ? 2 : 1));
        p.nog = NOG;               // layers with fewer than 512 outputs are padded with zero rows: every pass is the same straight-line code
        p.nchunks = (int16_t)(k == 0 ? 1 : NCH);
        p.bias_row = (int16_t)(k == 0 ? -3 : (k == lat ? -2 : k - 1));
        p.npad = (int16_t)(k == lat ? std::min(3, xyz0 - lat_ksteps) : 0);   // (a narrower net's unused slab rows are zero anyway: every layer writes them)
        p.last = (int16_t)(k == hidden - 1);
        p.chunk_base = chunk;
        const int slab_rows = k == 0 ? 0 : (k == lat ? lat_rows : id);
        const int xyz_col = k == 0 ? d->code_len : lat_rows + d->code_len;   // first of the three xyz columns of W
        const int xyz_first = k == 0 ? 0 : (k == lat ? xyz0 : 1 << 20);       // k-step of the first xyz operand
        const size_t base = out->stream.size();
        out->stream.resize(base + (size_t)p.nog * p.nchunks * (CHUNK_BYTES / 2), 0);
        uint16_t* dst = out->stream.data() + base;
        // chunk = [step of 32 k: 4][16-row tile: 4][lane 64][8 halves]: the A fragments of v_mfma_f32_16x16x32 (lane = row l & 15, k slots
        // 8 (l >> 4) + e).  Slot (gq, e) of step ks carries slab row 32 ks + 16 (e >> 2) + 4 gq + (e & 3): what the D registers of row tiles
        // 2 ks, 2 ks + 1 hold in lane group gq after v_cvt_pk (mlp_lp_kernel.hip).  The xyz step (two 16-slot halves u = slot >> 4 of
        // LP_XYZ_TERMS): slot 16 u + 3 t + c carries part wpart(u, t) of W[:, xyz c].
        const int xyz_step = xyz_first >= (1 << 20) ? (1 << 20) : xyz_first / 2;     // xyz_first is even (0 or 30): the xyz 16-slot k-steps form ONE 32-slot step
        constexpr int KQ = LP_KSTEPS_PER_CHUNK / 2;
        for (int g = 0; g < p.nog; ++g)
            for (int c = 0; c < p.nchunks; ++c)
                for (int kq = 0; kq < KQ; ++kq)
                    for (int rt = 0; rt < 4; ++rt)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 8; ++e) {
                                const int ks = KQ * c + kq, gq = lane >> 4;
                                const int orow = 64 * g + 16 * rt + (lane & 15);
                                float v = 0.f;
                                if (orow < od) {
                                    if (ks == xyz_step) {
                                        const int kk = 8 * gq + e, u = kk >> 4, k16 = kk & 15, t = k16 / 3;
                                        const int ent = t < 5 ? LP_XYZ_TERMS[tsel][u][t] : 0;
                                        if (ent) v = lp_part(W[(size_t)orow * id + xyz_col + k16 % 3], ent & 3, bf);
                                    } else if (ks < xyz_step) {
                                        const int krow = 32 * ks + 16 * (e >> 2) + 4 * gq + (e & 3);
                                        if (krow < slab_rows) v = W[(size_t)orow * id + krow];
                                    }
                                }
                                dst[((((size_t)(g * p.nchunks + c) * KQ + kq) * 4 + rt) * 64 + lane) * 8 + e] = lp_bits(v, bf);
                            }
        chunk += p.nog * p.nchunks;
    }
    out->n_pass = hidden;
    out->chunks = chunk;
    return true;
}

// Backward stream of the low-precision compute mode (mlp_lpj_bwd_kernel): for hidden layer k = hidden - 1 .. 0 the TRANSPOSED weights as A
// fragments in the prepass stream's slot order -- output row = a row of the layer's INPUT slab, k slot (gq, e) of step ks = row
// 32 ks + 16 (e >> 2) + 4 gq + (e & 3) of its OUTPUT.  Input-slab rows: hidden layers 0 .. in_dim - 1; the latent_in layer [h (width - in_dim) |
// xyz at rows 512 - in_dim .. + 2 | code behind them] (the fp32 kernel's order: NetView::colmap); the first layer code at rows 0 .. code_len - 1
// and xyz at rows 77 .. 79 (row 13 of 16-row tile 4: the lane position the latent_in pass leaves its xyz rows in).  Only DeepSDF's geometry
// (eight hidden layers, the latent_in layer fourth): the kernel's pass sequence is written out for it.
bool pack_decoder_lpj_host(PackedLp* out, const dsp_decoder_desc* d, bool bf) {
    const int hidden = d->n_layers - 1, lat = d->latent_in;
    if (hidden != 8 || lat != 4) return false;
    const int in_dim = d->code_len + 3, width = d->out_dims[0];
    if (width < 96 || width > WIDTH) return false;
    const int lat_rows = width - in_dim, p0 = WIDTH - in_dim;      // rows of h in the latent_in layer's input; slab row of its xyz
    out->stream.clear();
    memset(out->pass, 0, sizeof out->pass);
    int chunk = 0, np = 0;
    constexpr int KQ = LP_KSTEPS_PER_CHUNK / 2, NCH = 4;
    for (int k = hidden - 1; k >= 0; --k) {
        LpPass& p = out->pass[np++];
        const int od = d->out_dims[k], id = d->in_dims[k];
        const float* W = d->weights[k];
        std::vector<int> cm(WIDTH, -1);             // input-slab row -> column of W
        if (k == 0) {
            for (int r = 0; r < d->code_len; ++r) cm[r] = r;
            for (int c = 0; c < 3; ++c) cm[77 + c] = d->code_len + c;
        } else if (k == lat) {
            for (int r = 0; r < lat_rows; ++r) cm[r] = r;
            for (int c = 0; c < 3; ++c) cm[p0 + c] = lat_rows + d->code_len + c;
            for (int r = 0; r < d->code_len; ++r) cm[p0 + 3 + r] = lat_rows + r;
        } else {
            for (int r = 0; r < id; ++r) cm[r] = r;
        }
        p.kind = (int16_t)(k == lat ? 4 : (k == 0 ? 5 : 3));
        p.nog = (int16_t)(k == 0 ? 2 : 8);
        p.nchunks = NCH;
        p.bias_row = -1;
        p.chunk_base = chunk;
        const size_t base = out->stream.size();
        out->stream.resize(base + (size_t)p.nog * p.nchunks * (CHUNK_BYTES / 2), 0);
        uint16_t* dst = out->stream.data() + base;
        for (int g = 0; g < p.nog; ++g)
            for (int c = 0; c < p.nchunks; ++c)
                for (int kq = 0; kq < KQ; ++kq)
                    for (int rt = 0; rt < 4; ++rt)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 8; ++e) {
                                const int ks = KQ * c + kq, gq = lane >> 4;
                                const int orow = 64 * g + 16 * rt + (lane & 15);
                                const int krow = 32 * ks + 16 * (e >> 2) + 4 * gq + (e & 3);
                                float v = 0.f;
                                if (krow < od && cm[orow] >= 0) v = W[(size_t)krow * id + cm[orow]];
                                dst[((((size_t)(g * p.nchunks + c) * KQ + kq) * 4 + rt) * 64 + lane) * 8 + e] = lp_bits(v, bf);
                            }
        chunk += p.nog * p.nchunks;
    }
    out->n_pass = np;
    out->chunks = chunk;
    return true;
}

// Latency form (mlp_split_kernel): wave w of a workgroup produces output groups 2w and 2w+1 of every pass and streams only
// their chunks.  Returns the chunk ids of the throughput stream in the order the four waves consume them (wave 0's whole
// stream, then wave 1's, ...; inside a wave: pass, own group, chunk -- forward passes first, then backward), and each wave's
// offset / length / forward-prefix length in chunks.
std::vector<int> split_chunk_order(const PackedNet& pn, int off[4], int len[4], int len_fwd[4]) {
    std::vector<int> order;
    for (int w = 0; w < 4; ++w) {
        off[w] = (int)order.size();
        len_fwd[w] = 0;
        for (int ps = 0; ps < pn.n_pass_all; ++ps) {
            if (ps == pn.n_fwd) len_fwd[w] = (int)order.size() - off[w];
            for (int ol = 0; ol < 2; ++ol) {
                const int og = 2 * w + ol;
                if (og >= pn.pass[ps].nog) continue;
                for (int c = 0; c < pn.pass[ps].nchunks; ++c) order.push_back(pn.pass[ps].chunk_base + og * pn.pass[ps].nchunks + c);
            }
        }
        len[w] = (int)order.size() - off[w];
    }
    return order;
}

// Cluster form (mlp_cluster_kernel): wave slot u (16 per cluster of four workgroups) produces row tiles 2u, 2u + 1 of every pass, i.e.
// float4 components 2 (u & 1), 2 (u & 1) + 1 of output group u / 2, and streams only those.  Its stream: for every pass whose output
// group exists, the pass's chunks in order, each re-laid as 8 k-step PAIRS x 64 lanes x {tile 0 @ k-step 2p, tile 1 @ 2p, tile 0 @ 2p + 1,
// tile 1 @ 2p + 1} = 8 KiB = two 4 KiB mini-chunks.  Returns the 16 streams back to back; off / len in mini-chunks.
std::vector<float> cluster_stream(const PackedNet& pn, int off[16], int len[16]) {
    const size_t cf = CHUNK_BYTES / 4;
    std::vector<float> out;
    out.reserve(pn.stream.size());
    for (int u = 0; u < 16; ++u) {
        off[u] = (int)(out.size() * 4 / 4096);
        const int og = u >> 1, half = u & 1;
        for (int ps = 0; ps < pn.n_pass_all; ++ps) {
            if (og >= pn.pass[ps].nog) continue;
            for (int c = 0; c < pn.pass[ps].nchunks; ++c) {
                const float* ch = pn.stream.data() + (size_t)(pn.pass[ps].chunk_base + og * pn.pass[ps].nchunks + c) * cf;
                for (int p2 = 0; p2 < KSTEPS_PER_CHUNK / 2; ++p2)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e) {
                            const int sl = 2 * p2 + (e >> 1), j = 2 * half + (e & 1);
                            out.push_back(ch[(sl * 64 + lane) * 4 + j]);
                        }
            }
        }
        len[u] = (int)(out.size() * 4 / 4096) - off[u];
    }
    return out;
}

// per-object code bias on the host (single-shot calls); same arithmetic as k_code_bias
void code_bias_host(const std::vector<float>& codew, const std::vector<float>& b0, const std::vector<float>& blat, const float* code,
                    float* out /*1024*/) {
    for (int which = 0; which < 2; ++which)
        for (int o = 0; o < WIDTH; ++o) {
            float acc = which == 0 ? b0[o] : blat[o];
            const float* w = codew.data() + ((size_t)which * WIDTH + o) * CODE_LEN;
            for (int c = 0; c < CODE_LEN; ++c) acc = fmaf(w[c], code[c], acc);
            out[which * WIDTH + o] = acc;
        }
}

}  // namespace dsp_host
