// Host-only test hooks onto the decoder packers (decoder_pack.h): none of them needs a device.
#include "decoder_pack.h"
#include "host_common.h"

#include <cstring>

extern "C" {

/* Host-only: the per-object code bias (layer 0 and latent_in layer) exactly as the library computes it for single-shot
 * calls; out = 1024 floats. */
int dsp_debug_code_bias(const dsp_decoder_desc* decoder, const float* code, float* out) {
    if (!decoder || !code || !out) return DSP_E_ARG;
    return guarded(nullptr, [&] {
        PackedNet pn;
        pack_decoder_host(&pn, decoder);
        code_bias_host(pn.codew, pn.b0, pn.blat, code, out);
    });
}

/* Host-only: pack a decoder exactly as dsp_create does and copy the result out (tests emulate the kernel's
 * data flow on it without a GPU).  pass_out receives n_pass x 8 int32 {nog,nchunks,bias_row,relu,mask_slot,kind,chunk_base,0};
 * meta_out = {n_fwd, n_pass, chunks_fwd, chunks_all, n_bias_rows, wlast_row, w0_row, lat_tile, code_len}.  Call with NULL buffers to query sizes. */
int dsp_debug_pack(const dsp_decoder_desc* decoder, float* stream_out, int64_t* stream_len, float* bias_out,
                   int64_t* bias_len, int32_t* pass_out, int32_t* meta_out, float* b_last_out) {
    if (!decoder || !stream_len || !bias_len || !meta_out) return DSP_E_ARG;
    return guarded(nullptr, [&] {
        PackedNet pn;
        pack_decoder_host(&pn, decoder);
        *stream_len = (int64_t)pn.stream.size();
        *bias_len = (int64_t)pn.bias.size();
        meta_out[0] = pn.n_fwd; meta_out[1] = pn.n_pass_all; meta_out[2] = pn.chunks_fwd; meta_out[3] = pn.chunks_all; meta_out[4] = pn.n_bias_rows;
        if (b_last_out) *b_last_out = pn.b_last;
        meta_out[5] = pn.wlast_row; meta_out[6] = pn.w0_row; meta_out[7] = pn.lat_tile; meta_out[8] = pn.code_len;
        if (stream_out) memcpy(stream_out, pn.stream.data(), pn.stream.size() * 4);
        if (bias_out) memcpy(bias_out, pn.bias.data(), pn.bias.size() * 4);
        if (pass_out)
            for (int i = 0; i < pn.n_pass_all; ++i) {
                const PassDesc& p = pn.pass[i];
                int32_t* o = pass_out + 8 * i;
                o[0] = p.nog; o[1] = p.nchunks; o[2] = p.bias_row; o[3] = p.relu; o[4] = p.mask_slot; o[5] = p.kind; o[6] = p.chunk_base; o[7] = 0;
            }
    });
}

/* Host-only: pack the prepass weight stream exactly as dsp_create does (tests emulate the kernel's data flow on it without a GPU).
 * pass_out receives n_pass x 8 int32 {nog, nchunks, bias_row, kind, npad, last, chunk_base, 0}; meta_out = {n_pass, chunks}.
 * Call with NULL stream_out to query *stream_len (in 16-bit elements). */
int dsp_debug_pack_prepass(const dsp_decoder_desc* decoder, int dtype, uint16_t* stream_out, int64_t* stream_len, int32_t* pass_out,
                           int32_t* meta_out) {
    if (!decoder || !stream_len || !meta_out || (dtype != DSP_PREPASS_F16 && dtype != DSP_PREPASS_BF16)) return DSP_E_ARG;
    return guarded(nullptr, [&] {
        PackedLp pl;
        if (!pack_decoder_lp_host(&pl, decoder, dtype == DSP_PREPASS_BF16)) throw std::invalid_argument("decoder geometry not supported by the prepass kernel");
        *stream_len = (int64_t)pl.stream.size();
        meta_out[0] = pl.n_pass; meta_out[1] = pl.chunks;
        if (stream_out) memcpy(stream_out, pl.stream.data(), pl.stream.size() * 2);
        if (pass_out)
            for (int i = 0; i < pl.n_pass; ++i) {
                const LpPass& q = pl.pass[i];
                int32_t* o = pass_out + 8 * i;
                o[0] = q.nog; o[1] = q.nchunks; o[2] = q.bias_row; o[3] = q.kind; o[4] = q.npad; o[5] = q.last; o[6] = q.chunk_base; o[7] = 0;
            }
    });
}

/* Host-only: the transposed 16-bit stream of the low-precision compute mode's backward kernel, packed exactly as dsp_create does
 * (tests/lp_emulator.py replays mlp_lpj_kernel.hip's data flow on it without a GPU).  Same conventions as dsp_debug_pack_prepass; the passes
 * are those of layers hidden - 1 .. 0; meta_out = {n_pass, chunks, lat_tile}. */
int dsp_debug_pack_lpj(const dsp_decoder_desc* decoder, int dtype, uint16_t* stream_out, int64_t* stream_len, int32_t* pass_out, int32_t* meta_out) {
    if (!decoder || !stream_len || !meta_out || (dtype != DSP_COMPUTE_F16 && dtype != DSP_COMPUTE_BF16)) return DSP_E_ARG;
    return guarded(nullptr, [&] {
        PackedLp pl;
        if (!pack_decoder_lpj_host(&pl, decoder, dtype == DSP_COMPUTE_BF16)) throw std::invalid_argument("decoder geometry not supported by the 16-bit jacobian kernels");
        *stream_len = (int64_t)pl.stream.size();
        meta_out[0] = pl.n_pass; meta_out[1] = pl.chunks; meta_out[2] = (WIDTH - decoder->code_len - 3) / 16;
        if (stream_out) memcpy(stream_out, pl.stream.data(), pl.stream.size() * 2);
        if (pass_out)
            for (int i = 0; i < pl.n_pass; ++i) {
                const LpPass& p = pl.pass[i];
                int32_t* o = pass_out + 8 * i;
                o[0] = p.nog; o[1] = p.nchunks; o[2] = p.bias_row; o[3] = p.kind; o[4] = p.npad; o[5] = p.last; o[6] = p.chunk_base; o[7] = 0;
            }
    });
}

// host-only: the per-wave chunk order of the latency-form weight stream.  layout12 = off[4] | len[4] | len_fwd[4]; chunk_ids may be
// null (size query: *n_chunks is set), else it receives *n_chunks ids.
int dsp_debug_split_layout(const dsp_decoder_desc* decoder, int32_t* layout12, int32_t* chunk_ids, int64_t* n_chunks) {
    if (!decoder || !layout12 || !n_chunks) return DSP_E_ARG;
    return guarded(nullptr, [&] {
        PackedNet pn;
        pack_decoder_host(&pn, decoder);
        int off[4], len[4], lf[4];
        const std::vector<int> order = split_chunk_order(pn, off, len, lf);
        for (int w = 0; w < 4; ++w) { layout12[w] = off[w]; layout12[4 + w] = len[w]; layout12[8 + w] = lf[w]; }
        if (chunk_ids) {
            if (*n_chunks < (int64_t)order.size()) throw std::invalid_argument("chunk_ids too small");
            for (size_t i = 0; i < order.size(); ++i) chunk_ids[i] = order[i];
        }
        *n_chunks = (int64_t)order.size();
    });
}

// host-only: the cluster-form weight stream exactly as dsp_create uploads it (tests check its layout against the throughput stream on
// the CPU).  layout32 = off[16] | len[16] in 4 KiB mini-chunks; stream_out may be null (size query: *n_floats is set).
int dsp_debug_cluster_stream(const dsp_decoder_desc* decoder, int32_t* layout32, float* stream_out, int64_t* n_floats) {
    if (!decoder || !layout32 || !n_floats) return DSP_E_ARG;
    return guarded(nullptr, [&] {
        PackedNet pn;
        pack_decoder_host(&pn, decoder);
        int off[16], len[16];
        const std::vector<float> cs = cluster_stream(pn, off, len);
        for (int u = 0; u < 16; ++u) { layout32[u] = off[u]; layout32[16 + u] = len[u]; }
        if (stream_out) {
            if (*n_floats < (int64_t)cs.size()) throw std::invalid_argument("stream_out too small");
            memcpy(stream_out, cs.data(), cs.size() * 4);
        }
        *n_floats = (int64_t)cs.size();
    });
}

}  // extern "C"
