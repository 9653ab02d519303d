// The decoder on a handle: the upload of the packed weight streams (decoder_pack.hip packs them), the argument blocks of the decoder launches,
// the single-shot decoder calls, the prepass calibration, and their C ABI.
#include "decoder_calls.h"
#include "decoder_pack.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <vector>

namespace {

// Prepass margins are calibrated per decoder at dsp_create (calibrate_prepass): delta = 6 x the largest |sdf_lp - sdf_fp32| over
// 64 k unit-ball points x 4 codes, not below these floors (what the cars fixture needs: measured 1.05e-4 f16, 6.8e-4 bf16 over the
// 38 M audited samples of the bench workload, profiles/parity_r02.md).
constexpr float PREPASS_DELTA_F16 = 5e-4f, PREPASS_DELTA_BF16 = 3e-3f;

}  // namespace

namespace dsp_host {

void pack_decoder(dsp_handle* h, const dsp_decoder_desc* d) {
    PackedNet pn;
    pack_decoder_host(&pn, d);
    h->b_last = pn.b_last; h->n_bias_rows = pn.n_bias_rows; h->n_fwd = pn.n_fwd; h->n_pass_all = pn.n_pass_all;
    h->chunks_fwd = pn.chunks_fwd; h->chunks_all = pn.chunks_all;
    h->wlast_row = pn.wlast_row; h->w0_row = pn.w0_row;
    h->lat_tile = pn.lat_tile; h->code_len = pn.code_len;
    h->h_codew = pn.codew; h->h_b0 = pn.b0; h->h_blat = pn.blat;
    h->codew.alloc(pn.codew.size());
    HIP_TRY(hipMemcpy(h->codew.p, pn.codew.data(), pn.codew.size() * 4, hipMemcpyHostToDevice));
    h->b0.alloc(WIDTH); h->blat.alloc(WIDTH);
    HIP_TRY(hipMemcpy(h->b0.p, pn.b0.data(), WIDTH * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->blat.p, pn.blat.data(), WIDTH * 4, hipMemcpyHostToDevice));
    memcpy(h->pass, pn.pass, sizeof h->pass);
    h->wstream.alloc(pn.stream.size());
    HIP_TRY(hipMemcpy(h->wstream.p, pn.stream.data(), pn.stream.size() * 4, hipMemcpyHostToDevice));
    {   // latency form: per-wave copy of the stream (split_chunk_order)
        const size_t cf = CHUNK_BYTES / 4;
        const std::vector<int> order = split_chunk_order(pn, h->split_off, h->split_len, h->split_len_fwd);
        std::vector<float> split;
        split.reserve(pn.stream.size());
        for (int chunk : order) split.insert(split.end(), pn.stream.begin() + (size_t)chunk * cf, pn.stream.begin() + (size_t)(chunk + 1) * cf);
        if (split.size() != pn.stream.size()) throw std::logic_error("split weight stream does not cover the stream");
        h->wsplit.alloc(split.size());
        HIP_TRY(hipMemcpy(h->wsplit.p, split.data(), split.size() * 4, hipMemcpyHostToDevice));
    }
    {   // cluster form: per-wave-slot copy of the stream (cluster_stream)
        const std::vector<float> cs = cluster_stream(pn, h->cl_off, h->cl_len);
        if (cs.size() != pn.stream.size()) throw std::logic_error("cluster weight stream does not cover the stream");
        h->wcluster.alloc(cs.size());
        HIP_TRY(hipMemcpy(h->wcluster.p, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
    }
    h->bias_tab.alloc(pn.bias.size());
    HIP_TRY(hipMemcpy(h->bias_tab.p, pn.bias.data(), pn.bias.size() * 4, hipMemcpyHostToDevice));
    h->lp_ok = true;
    for (int bf = 0; bf < 2 && h->lp_ok; ++bf) {
        PackedLp pl;
        if (!pack_decoder_lp_host(&pl, d, bf != 0)) { h->lp_ok = false; break; }
        h->wlp[bf].alloc(pl.stream.size());
        HIP_TRY(hipMemcpy(h->wlp[bf].p, pl.stream.data(), pl.stream.size() * 2, hipMemcpyHostToDevice));
        memcpy(h->lp_pass, pl.pass, sizeof h->lp_pass);
        h->lp_n_pass = pl.n_pass;
        h->lp_chunks = pl.chunks;
    }
    h->lpj_ok = h->lp_ok;
    for (int bf = 0; bf < 2 && h->lpj_ok; ++bf) {
        PackedLp pl;
        if (!pack_decoder_lpj_host(&pl, d, bf != 0)) { h->lpj_ok = false; break; }
        h->wlpj[bf].alloc(pl.stream.size());
        HIP_TRY(hipMemcpy(h->wlpj[bf].p, pl.stream.data(), pl.stream.size() * 2, hipMemcpyHostToDevice));
        memcpy(h->lpj_pass, pl.pass, sizeof h->lpj_pass);
        h->lpj_chunks = pl.chunks;
    }
}

// which: 0 = forward with mask export (the prepass stream), 1 = backward from the masks (the transposed stream)
LpjArgs make_lpj_args(const dsp_handle* h, bool bf, int which) {
    LpjArgs a;
    memset(&a, 0, sizeof a);
    a.bias_tab = h->bias_tab.p;
    a.b_last = h->b_last;
    a.n_bias_rows = h->n_bias_rows;
    a.wlast_row = h->wlast_row;
    a.lat_tile = h->lat_tile;
    if (which == 0) {
        a.wstream = h->wlp[bf ? 1 : 0].p;
        a.total_chunks = h->lp_chunks;
        memcpy(a.pass, h->lp_pass, sizeof a.pass);
    } else {
        a.wstream = h->wlpj[bf ? 1 : 0].p;
        a.total_chunks = h->lpj_chunks;
        memcpy(a.pass, h->lpj_pass, sizeof a.pass);
    }
    return a;
}

LpArgs make_lp_args(const dsp_handle* h, bool bf) {
    LpArgs a;
    memset(&a, 0, sizeof a);
    a.wstream = h->wlp[bf ? 1 : 0].p;
    a.bias_tab = h->bias_tab.p;
    a.b_last = h->b_last;
    a.n_bias_rows = h->n_bias_rows;
    a.wlast_row = h->wlast_row;
    a.n_pass = h->lp_n_pass;
    a.total_chunks = h->lp_chunks;
    memcpy(a.pass, h->lp_pass, sizeof a.pass);
    return a;
}

MlpArgs make_mlp_args(const dsp_handle* h, int mode) {   // mode: 0/1 forward, 2 forward+backward, 3 backward only (mlp_kernel)
    MlpArgs a;
    memset(&a, 0, sizeof a);
    a.bias_tab = h->bias_tab.p;
    a.b_last = h->b_last;
    a.n_bias_rows = h->n_bias_rows;
    a.wlast_row = h->wlast_row;
    a.w0_row = h->w0_row;
    a.seed_slot = h->n_fwd;        // mask slot of the last hidden layer (slot = layer index, layer 0 has slot 0)
    a.lat_tile = h->lat_tile;
    a.wsplit = h->wsplit.p;
    memcpy(a.split_off, h->split_off, sizeof a.split_off);
    memcpy(a.split_len, h->split_len, sizeof a.split_len);
    memcpy(a.split_len_fwd, h->split_len_fwd, sizeof a.split_len_fwd);
    a.wcluster = h->wcluster.p;
    memcpy(a.cl_off, h->cl_off, sizeof a.cl_off);
    memcpy(a.cl_len, h->cl_len, sizeof a.cl_len);
    a.cl_xbuf = h->cl_xbuf.p;
    if (mode == 3) {               // only the backward half of the stream and of the pass table
        const int n_bwd = h->n_pass_all - h->n_fwd;
        a.wstream = h->wstream.p + (size_t)h->chunks_fwd * (CHUNK_BYTES / 4);
        a.n_fwd = 0;
        a.n_pass = n_bwd;
        a.total_chunks = h->chunks_all - h->chunks_fwd;
        memcpy(a.pass, h->pass + h->n_fwd, n_bwd * sizeof(PassDesc));
    } else {
        a.wstream = h->wstream.p;
        a.n_fwd = h->n_fwd;
        a.n_pass = mode == 2 ? h->n_pass_all : h->n_fwd;
        a.total_chunks = mode == 2 ? h->chunks_all : h->chunks_fwd;
        memcpy(a.pass, h->pass, sizeof a.pass);
    }
    return a;
}

// n_codes objects x the same n points, already in h->s_pts (device): decoder forward or forward+gradient into h->s_out,
// output row = code * n + point.  Asynchronous on h->stream.
// lp: 0 = fp32 kernels, 1 = f16 prepass kernel, 2 = bf16 prepass kernel (forward only).  out: forward sdf into this device buffer
// (n_codes x n floats) instead of h->s_out
void decode_resident_points(dsp_handle* h, const float* codes, int64_t n_codes, int64_t n, bool bwd, int lp, float* out) {
    const int lpj = lp >= 5 ? lp - 4 : 0;         // 5 / 6: forward + gradient through the 16-bit jacobian kernels (f16 / bf16)
    if (lpj) lp = lpj;
    if (lp && bwd && !lpj) throw std::invalid_argument("low-precision decode is forward only");
    if (lp && !h->lp_ok) throw std::invalid_argument("this decoder's geometry has no prepass kernel (it needs an even number of hidden layers, one latent_in layer, width <= 512)");
    const bool lp_small = lp >= 3;                // testing: the prepass kernel's 64-point-tile form (dtype | DSP_PREPASS_SMALL_TILES)
    if (lp_small) lp -= 2;
    const int tile_pts = lp ? (lp_small ? LP_TILE_PTS_SMALL : LP_TILE_PTS) : TILE_PTS;
    const int64_t ntile = (n + tile_pts - 1) / tile_pts;
    if (ntile * n_codes > (int64_t)1 << 30 || n * n_codes > (int64_t)1 << 31) throw std::invalid_argument("decode request too large");
    const int nt = (int)(ntile * n_codes);
    std::vector<int4> tiles(nt);
    for (int64_t c = 0; c < n_codes; ++c)
        for (int64_t i = 0; i < ntile; ++i)
            tiles[c * ntile + i] = make_int4((int)(i * tile_pts), (int)std::min<int64_t>(tile_pts, n - i * tile_pts), (int)c, (int)(c * n));
    const size_t n_out = (size_t)n * n_codes;
    h->s_code.ensure((size_t)CODE_LEN * n_codes);
    h->s_cbias.ensure((size_t)2 * WIDTH * n_codes);
    std::vector<float> cb((size_t)2 * WIDTH * n_codes);
    for (int64_t c = 0; c < n_codes; ++c) code_bias_host(h->h_codew, h->h_b0, h->h_blat, codes + c * CODE_LEN, cb.data() + c * 2 * WIDTH);
    HIP_TRY(hipMemcpyAsync(h->s_cbias.p, cb.data(), cb.size() * 4, hipMemcpyHostToDevice, h->stream));
    h->s_tiles.ensure(nt);
    h->s_ntiles.ensure(1);
    if (bwd || !out) h->s_out.ensure(bwd ? n_out * GRAD_STRIDE : n_out);
    float* const sdf_dst = (bwd || !out) ? h->s_out.p : out;
    HIP_TRY(hipMemcpyAsync(h->s_code.p, codes, (size_t)CODE_LEN * n_codes * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->s_tiles.p, tiles.data(), nt * sizeof(int4), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->s_ntiles.p, &nt, 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));     // the staging vectors above go out of scope
    h->s_clk.ensure(4);
    if (lpj) {
        h->s_lpj_masks.ensure((size_t)nt * 16 * 256);
        for (int which = 0; which < 2; ++which) {
            LpjArgs ja = make_lpj_args(h, lpj == 2, which);
            ja.n_tiles = h->s_ntiles.p;
            ja.tiles = h->s_tiles.p;
            ja.pts = h->s_pts.p;
            ja.code_bias = h->s_cbias.p;
            ja.code_bias_stride = 2 * WIDTH;
            ja.out_grad = h->s_out.p;
            ja.mask_buf = h->s_lpj_masks.p;
            ja.clk = which ? h->s_clk.p : nullptr;
            HIP_TRY(launch_mlp_lpj(which, lpj == 2, ja, std::min(nt, h->n_cu), h->stream));
        }
        return;
    }
    if (lp) {
        LpArgs la = make_lp_args(h, lp == 2);
        la.n_tiles = h->s_ntiles.p;
        la.tiles = h->s_tiles.p;
        la.pts = h->s_pts.p;
        la.code_bias = h->s_cbias.p;
        la.code_bias_stride = 2 * WIDTH;
        la.out_sdf = sdf_dst;
        la.clk = h->s_clk.p;
        HIP_TRY(launch_mlp_lp(lp == 2, la, std::min(nt, h->n_cu), h->stream, tile_pts));
        return;
    }
    MlpArgs a = make_mlp_args(h, bwd ? 2 : 0);
    a.n_tiles = h->s_ntiles.p;
    a.tiles = h->s_tiles.p;
    a.pts = h->s_pts.p;
    a.code_bias = h->s_cbias.p;
    a.code_bias_stride = 2 * WIDTH;
    a.out_sdf = sdf_dst;
    a.out_grad = h->s_out.p;
    h->s_clk.ensure(4);
    a.clk = h->s_clk.p;
    HIP_TRY(launch_mlp(bwd ? 2 : 0, a, std::min(nt, h->n_cu), h->stream));
}

}  // namespace dsp_host

namespace {

// n_codes objects x the same n host points (object frame): forward or forward+gradient.  Output row = code * n + point.
void run_decoder_points(dsp_handle* h, const float* codes, int64_t n_codes, const float* pts, int64_t n, bool bwd, float* sdf_out,
                        float* grad_out, int lp = 0) {
    if (n <= 0 || n_codes <= 0) return;
    HIP_TRY(hipSetDevice(h->device));
    std::vector<float4> p4((size_t)n);
    for (int64_t i = 0; i < n; ++i) p4[i] = make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], 0.f);
    h->s_pts.ensure(n);
    HIP_TRY(hipMemcpyAsync(h->s_pts.p, p4.data(), n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    decode_resident_points(h, codes, n_codes, n, bwd, lp);
    const size_t n_out = (size_t)n * n_codes;
    if (!bwd) {
        HIP_TRY(hipMemcpyAsync(sdf_out, h->s_out.p, n_out * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    } else {
        std::vector<float> tmp(n_out * GRAD_STRIDE);
        HIP_TRY(hipMemcpyAsync(tmp.data(), h->s_out.p, tmp.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < n_out; ++i) {
            if (grad_out) memcpy(grad_out + i * DSP_GRAD_DIM, tmp.data() + i * GRAD_STRIDE, DSP_GRAD_DIM * 4);
            if (sdf_out) sdf_out[i] = tmp[i * GRAD_STRIDE + 67];
        }
    }
}

// Prepass margins of THIS decoder, as a function of the code's magnitude.  The 16-bit error is dominated by rounding the hidden
// activations once per layer, and the activations grow with the code: a margin measured on small codes says nothing about the codes
// a warm start hands over (LocalMapping_util.cc:391-392) or the optimiser reaches.  So the calibration decodes seeded unit-ball points
// through the fp32 kernel and through both low-precision kernels with codes drawn uniformly in +-mag on every entry, for each mag of
// LP_MAGS (|z|_inf = mag, |z|_2 ~ 4.6 mag: far larger in norm than a real code with the same largest entry), and keeps
// delta(mag) = max(floor, 6 x worst error up to that magnitude), capped at 0.5.  An object's margin is then read off its CURRENT code
// every iteration (lp_delta_of, gn_kernels.hip).  dsp_prepass_calibration reports the table.
constexpr float LP_MAGS[LP_NMAG] = {0.f, 0.15f, 0.5f, 1.0f, 2.0f};

}  // namespace

namespace dsp_host {

void calibrate_prepass(dsp_handle* h) {
    if (!h->lp_ok) return;
    constexpr int N = 32768, PER_MAG = 2, NCODE = LP_NMAG * PER_MAG;
    std::vector<float> pts((size_t)N * 3), codes((size_t)NCODE * CODE_LEN, 0.f), ref((size_t)N * NCODE), lp((size_t)N * NCODE);
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (float)((st >> 40) & 0xFFFFFF) / 16777216.f; };
    for (int i = 0; i < N;) {                      // uniform in the unit ball (the optimiser only decodes in-sphere samples)
        const float x = 2.f * rnd() - 1.f, y = 2.f * rnd() - 1.f, z = 2.f * rnd() - 1.f;
        if (x * x + y * y + z * z >= 1.f) continue;
        pts[3 * i] = x; pts[3 * i + 1] = y; pts[3 * i + 2] = z;
        ++i;
    }
    for (int c = 0; c < NCODE; ++c) {
        const float mag = LP_MAGS[c / PER_MAG];
        for (int k = 0; k < h->code_len; ++k) codes[(size_t)c * CODE_LEN + k] = mag * (2.f * rnd() - 1.f);
        if (mag > 0.f) codes[(size_t)c * CODE_LEN + (c % h->code_len)] = (c & 1) ? mag : -mag;     // the largest entry IS mag
    }
    run_decoder_points(h, codes.data(), NCODE, pts.data(), N, false, ref.data(), nullptr, 0);
    for (int bf = 0; bf < 2; ++bf) {
        run_decoder_points(h, codes.data(), NCODE, pts.data(), N, false, lp.data(), nullptr, bf ? DSP_PREPASS_BF16 : DSP_PREPASS_F16);
        float running = 0.f;
        for (int m = 0; m < LP_NMAG; ++m) {
            float worst = 0.f;
            for (size_t i = (size_t)m * PER_MAG * N; i < (size_t)(m + 1) * PER_MAG * N; ++i) {
                const float d = std::fabs(lp[i] - ref[i]);
                if (!(d <= worst)) worst = std::isfinite(d) ? d : 1.f;      // a non-finite prepass value: make the band cover everything
            }
            h->lp_err[bf][m] = worst;
            running = std::max(running, worst);
            h->lp_tab[bf].mag[m] = LP_MAGS[m];
            // 6 x: the largest error over 38 M samples of the bench workload is 1.4 x the largest over these 65 k points (audit,
            // profiles/parity_r03.md), and the guard trips at HALF the margin -- a healthy run stays 2x below the trip point
            h->lp_tab[bf].delta[m] = std::min(0.5f, std::max(6.f * running, bf ? PREPASS_DELTA_BF16 : PREPASS_DELTA_F16));
        }
    }
}

// host copy of lp_delta_of (gn_kernels.hip) for states that are written from the host (stand-alone terms)
float lp_delta_host(const float* code, const LpDeltaTab& t) {
    float zmax = 0.f;
    for (int i = 0; i < CODE_LEN; ++i) { const float a = std::fabs(code[i]); if (!(a <= zmax)) zmax = a; }
    if (!(zmax < 1e30f)) return 0.5f;
    float d = t.delta[0];
    for (int i = 0; i + 1 < LP_NMAG; ++i) {
        const float m0 = t.mag[i], m1 = t.mag[i + 1];
        if (zmax > m0 && (zmax <= m1 || i + 2 == LP_NMAG)) d = t.delta[i] + (t.delta[i + 1] - t.delta[i]) * ((zmax - m0) / (m1 - m0));
    }
    return std::min(std::max(d, t.delta[0]), 0.5f);
}

}  // namespace dsp_host

extern "C" {

/* Development aid: {shader-clock ticks, 100 MHz wall ticks} spent by workgroup 0 of the last dsp_decode_sdf /
 * dsp_sdf_jacobian launch -> effective shader clock under load. */
int dsp_debug_last_clocks(dsp_handle* h, uint64_t* out4) {
    if (!h || !out4 || !h->s_clk.p) return DSP_E_ARG;
    return guarded(h, [&] { HIP_TRY(hipSetDevice(h->device)); HIP_TRY(hipMemcpy(out4, h->s_clk.p, 32, hipMemcpyDeviceToHost)); });
}

int dsp_decode_sdf(dsp_handle* h, const float* code, const float* pts, int64_t n, float* sdf_out) {
    if (!h || !code || (n > 0 && (!pts || !sdf_out)) || n < 0) return DSP_E_ARG;
    return guarded(h, [&] { run_decoder_points(h, code, 1, pts, n, false, sdf_out, nullptr); });
}

int dsp_decode_sdf_prepass(dsp_handle* h, int dtype, const float* code, const float* pts, int64_t n, float* sdf_out) {
    const int small = dtype & DSP_PREPASS_SMALL_TILES;
    dtype &= ~DSP_PREPASS_SMALL_TILES;
    if (!h || !code || (n > 0 && (!pts || !sdf_out)) || n < 0 || (dtype != DSP_PREPASS_F16 && dtype != DSP_PREPASS_BF16)) return DSP_E_ARG;
    return guarded(h, [&] { run_decoder_points(h, code, 1, pts, n, false, sdf_out, nullptr, dtype + (small ? 2 : 0)); });
}

int dsp_decode_sdf_multi(dsp_handle* h, const float* codes, int64_t n_codes, const float* pts, int64_t n, float* sdf_out) {
    if (!h || !codes || n_codes < 0 || n < 0 || (n > 0 && n_codes > 0 && (!pts || !sdf_out))) return DSP_E_ARG;
    return guarded(h, [&] { run_decoder_points(h, codes, n_codes, pts, n, false, sdf_out, nullptr); });
}

int dsp_sdf_jacobian_lp(dsp_handle* h, int dtype, const float* code, const float* pts, int64_t n, float* sdf_out, float* grad_out) {
    if (!h || !code || (n > 0 && !pts) || n < 0 || (dtype != DSP_COMPUTE_F16 && dtype != DSP_COMPUTE_BF16)) return DSP_E_ARG;
    return guarded(h, [&] {
        if (!h->lpj_ok) throw std::invalid_argument("this decoder's geometry has no 16-bit jacobian kernel (eight hidden layers, the latent_in layer fourth)");
        run_decoder_points(h, code, 1, pts, n, true, sdf_out, grad_out, 4 + dtype);
    });
}

int dsp_sdf_jacobian(dsp_handle* h, const float* code, const float* pts, int64_t n, float* sdf_out, float* grad_out) {
    if (!h || !code || (n > 0 && !pts) || n < 0) return DSP_E_ARG;
    return guarded(h, [&] { run_decoder_points(h, code, 1, pts, n, true, sdf_out, grad_out); });
}

int dsp_prepass_calibration(dsp_handle* h, int dtype, float* max_err, float* delta) {
    if (!h || (dtype != DSP_PREPASS_F16 && dtype != DSP_PREPASS_BF16)) return DSP_E_ARG;
    if (!h->lp_ok) return DSP_E_STATE;
    if (max_err) *max_err = h->lp_err[dtype == DSP_PREPASS_BF16 ? 1 : 0][0];
    if (delta) *delta = h->lp_tab[dtype == DSP_PREPASS_BF16 ? 1 : 0].delta[0];
    return DSP_OK;
}

int dsp_prepass_calibration_table(dsp_handle* h, int dtype, float* mags, float* max_err, float* delta, float* guard_err) {
    if (!h || (dtype != DSP_PREPASS_F16 && dtype != DSP_PREPASS_BF16)) return DSP_E_ARG;
    if (!h->lp_ok) return DSP_E_STATE;
    const int bf = dtype == DSP_PREPASS_BF16 ? 1 : 0;
    std::lock_guard<std::mutex> lock(h->mu);
    for (int m = 0; m < LP_NMAG; ++m) {
        if (mags) mags[m] = h->lp_tab[bf].mag[m];
        if (max_err) max_err[m] = h->lp_err[bf][m];
        if (delta) delta[m] = std::min(0.5f, std::max(h->lp_tab[bf].delta[m], 4.f * h->lp_guard_err[bf]));
    }
    if (guard_err) *guard_err = h->lp_guard_err[bf];
    return DSP_OK;
}

int dsp_prepass_reset_guard(dsp_handle* h) {
    if (!h) return DSP_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    h->lp_guard_err[0] = h->lp_guard_err[1] = 0.f;
    return DSP_OK;
}

}  // extern "C"
