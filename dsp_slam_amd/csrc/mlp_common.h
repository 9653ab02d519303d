// Shared by the three fp32 decoder forms -- mlp_kernel.hip (throughput), mlp_split_kernel.hip (latency), mlp_cluster_kernel.hip (cluster):
// MFMA / LDS-DMA helpers, the LDS carve-up, every step of a tile that is not the form itself (all three keep the same lane layout:
// sin_[4t+r] = row 16t + 4g + r of point pl), and the per-wave weight ring of the latency and cluster forms.
#pragma once
#include "dsp_internal.h"

namespace dsp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NBUF = 6;                       // LDS ring depth (chunks)
constexpr int BIAS_ROWS_MAX = 11;             // 7 hidden biases, final-layer weights, 3 first-layer xyz columns
constexpr int BIAS_BYTES = BIAS_ROWS_MAX * WIDTH * 4;      // 22 KiB
constexpr int CODEBIAS_BYTES = 2 * WIDTH * 4;              // per-object code contribution of layer 0 and of the latent_in layer
constexpr int MASK_SLOTS = 8;
constexpr int MASK_BYTES = MASK_SLOTS * 8 * 256 * 2;       // [slot][og][tid] u16 = 32 KiB
// A operands are read from LDS in groups of PAIR_READS k-steps, one s_waitcnt per group, two groups ahead of their MFMAs: every instruction
// between two MFMAs costs matrix-pipe time even in the MFMA's shadow (measured: one read + one wait per k-step 0.885 of peak, groups of 2:
// 0.903, groups of 4: 0.898; profiles/r06_removed_experiments.md)
constexpr int PAIR_READS = 2;
constexpr int GLDS_PER_CHUNK = 4;             // per wave: 4 x 1 KiB pieces of a 16 KiB chunk

#define MFMA16(A, B, C) __builtin_amdgcn_mfma_f32_16x16x4f32((A), (B), (C), 0, 0, 0)

// LDS-DMA of one wave's quarter (4 KiB) of a weight chunk: four global_load_lds_dwordx4, each 64 lanes x 16 B from a
// global address to LDS at M0 + lane*16.  The instruction's immediate offset moves BOTH the global source and
// the LDS destination (measured: tools/probes/hw_probe.hip), so one address and one M0 value serve all four.
// Invisible to hipcc's s_waitcnt bookkeeping by design: completion is counted by hand (vmcnt) below.
// Addressing: the stream position is wave-uniform, so it travels as an SGPR pair (saddr) and the per-lane part is the constant
// 32-bit offset lane*16 -- half the address registers the 64-bit per-lane form sends through the address unit per instruction
// (measured: K1 0.862 -> 0.883 of peak against the per-lane form).
// M0 is written and NOT restored: hipcc treats M0 as reserved and sets it itself right before any instruction of its own that needs
// it; in these kernels it emits none (gfx9+ LDS instructions do not read M0), which tests/test_cabi_symbols.py checks on the built
// code objects (every M0 reference must be one of these writes).  Two SALU instructions fewer per piece, in the MFMA stream.
__device__ __forceinline__ void glds_quarter(const char* gsrc_uniform, unsigned lane_off, unsigned lds_dst) {
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %1\n\t"
        "global_load_lds_dwordx4 %0, %1 offset:1024\n\t"
        "global_load_lds_dwordx4 %0, %1 offset:2048\n\t"
        "global_load_lds_dwordx4 %0, %1 offset:3072"
        :
        : "v"(lane_off), "s"(gsrc_uniform), "s"(lds_dst)
        : "memory");
}

// The four pieces of a chunk share one LDS destination base: M0 is set once (glds_set_dst, at the barrier that frees the slot) and the
// pieces are bare loads whose immediate offset moves source and destination alike -- 5 instructions per chunk and wave in the MFMA stream
// (a form in which every piece writes M0 itself: 12; profiles/r06_removed_experiments.md).  M0 has to survive the k-steps in between;
// nothing else in these kernels writes it (tests/test_cabi_symbols.py checks the code objects).
__device__ __forceinline__ void glds_set_dst(unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" : : "s"(lds_dst) : "memory");
}
template <int PIECE>
__device__ __forceinline__ void glds_piece_m0(const char* gsrc_uniform, unsigned lane_off, unsigned lds_dst) {
    asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2" : : "v"(lane_off), "s"(gsrc_uniform), "n"(PIECE * 1024) : "memory");
}

__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)p;
}

// relu as ONE instruction: fmaxf() on an MFMA result makes hipcc emit a canonicalising v_max before the real one
__device__ __forceinline__ float relu1(float x) {
    float r;
    asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(x));
    return r;
}

// relu-mask bit of one pre-activation, two spellings of `x > 0` (same bit for every x, NaN included: 0).
// Throughput form: shifted into `bits` (bits = 2 * bits + (x > 0)): v_cmp + v_addc instead of the
// v_cmp / v_cndmask / v_lshl_or chain hipcc emits for `bits |= (x > 0) << k`.  Feed elements 15 down to 0 and element k ends at bit k.
__device__ __forceinline__ void push_mask_bit(unsigned& bits, float x) {
    asm volatile("v_cmp_lt_f32 vcc, 0, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(bits) : "v"(x) : "vcc");
}
// Latency and cluster forms: `bits |= mask_bit(x, k)`.  They keep the plain spelling because hipcc may schedule it and drop what is
// not stored (the latency form's layer 0 forms the bits of all eight groups and stores its wave's two); the volatile pair above
// stays where it is put.  Unifying the two was not measured, so each form keeps the code it was tuned with.
__device__ __forceinline__ unsigned mask_bit(float x, int k) { return (x > 0.f ? 1u : 0u) << k; }

// Always-on guard of the low-precision pre-classification (DESIGN.md "Prepass").  The prepass is exact as long as
// |sdf_lp - sdf_fp32| < lp_delta for every sample it classifies.  The fp32 kernels re-decode every sample the prepass left inside the
// widened band, plus a stratified sample of the ones it classified (k_band_*: guard samples), and each of those still holds its prepass value
// where the fp32 value is about to be stored: compare them.  A difference of half the object's margin or more is a TRIP (counted per
// wave, per object): the host then re-runs the batch with the prepass off (batch_run) -- results never depend on a margin that the
// workload itself has shown to be thin.  The largest difference seen is kept as well (dsp_stats.prepass_guard_max_err).
// `active`: this lane stores a sample's fp32 sdf; old_lp: what the slot held (1.0f = never decoded by the prepass: no comparison).
// tol: half the object's margin, 0.5f * float(guard word 0 of the object) -- passed in so that a caller can fetch it early
__device__ __forceinline__ void prepass_guard_tol(const MlpArgs& a, int obj, bool active, float old_lp, float y, float tol) {
    float err = 0.f;
    if (active && old_lp != 1.0f) {
        err = fabsf(old_lp - y);
        if (!(err < 1.0f)) err = 1.0f;                  // NaN / inf prepass value
    }
    float m = err;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if (m > 0.f && (threadIdx.x & 63) == 0) {
        unsigned* w = a.guard + (size_t)obj * a.guard_stride;
        atomicMax(w + 2, __float_as_uint(m));
        if (!(m < tol)) atomicAdd(w + 1, 1u);
    }
}

// the same with the tolerance read here (callers that have no early point to fetch it from)
__device__ __forceinline__ void prepass_guard(const MlpArgs& a, int obj, bool active, float old_lp, float y) {
    prepass_guard_tol(a, obj, active, old_lp, y, 0.5f * __uint_as_float(a.guard[(size_t)obj * a.guard_stride]));
}

// ---- tile steps of the fp32 forms ---------------------------------------------------------------------------------------------------
// Lane layout of all three: lane = 16 g + pl; sin_[4t+r] holds row 16t + 4g + r of point pl (g = MFMA k index of the lane group == 4-row
// block inside a 16-row tile).  "Same k order, same bias seeding, same masks per output element" across the forms holds because they
// call the code below, not because three files are kept in step.

// LDS-only barrier: __syncthreads() would also drain vmcnt, i.e. the weight prefetch in flight
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Head of every form's dynamic LDS: the bias table, the object's two code-bias vectors ([0..511] layer 0, [512..1023] latent_in layer),
// then the form's relu masks; what follows them (exchange slab, weight ring) is the form's own.
struct DecoderLds {
    float* bias;
    float* cb;
    unsigned short* mask;
};
__device__ __forceinline__ DecoderLds carve_lds(char* smem) {
    return DecoderLds{reinterpret_cast<float*>(smem), reinterpret_cast<float*>(smem + BIAS_BYTES),
                      reinterpret_cast<unsigned short*>(smem + BIAS_BYTES + CODEBIAS_BYTES)};
}
constexpr int LDS_HEAD_BYTES = BIAS_BYTES + CODEBIAS_BYTES;      // the form's masks start here

__device__ __forceinline__ void stage_bias_table(const MlpArgs& a, float* bias_l, int tid) {
    for (int i = tid; i < a.n_bias_rows * WIDTH; i += 256) bias_l[i] = a.bias_tab[i];
    __syncthreads();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The shape code is the same for every point of the tile, so its contribution to layer 0 and to the latent_in
// layer is a per-object bias vector (k_code_bias): stage both into LDS (the caller fences the readers on either side).
__device__ __forceinline__ void stage_code_bias(const MlpArgs& a, float* cb_l, int obj, int tid) {
    reinterpret_cast<float4*>(cb_l)[tid] = reinterpret_cast<const float4*>(a.code_bias + (size_t)obj * a.code_bias_stride)[tid];
}

// Layer 0, rows `row` + 4g .. + 3 (row = 16 x row tile) of this lane's point, before the relu.  What is left of layer 0 next to the code
// bias is three multiply-adds per row (W0[:, xyz] . p) -- done on the VALU instead of 16 mostly-empty MFMA chunks.
__device__ __forceinline__ f32x4 layer0_rows(const MlpArgs& a, const float* bias_l, const float* cb_l, int g, int row, const float4 pt) {
    const float* w0 = bias_l + a.w0_row * WIDTH + 4 * g;
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(cb_l + row + 4 * g);
    const f32x4 wx = *reinterpret_cast<const f32x4*>(w0 + row);
    const f32x4 wy = *reinterpret_cast<const f32x4*>(w0 + WIDTH + row);
    const f32x4 wz = *reinterpret_cast<const f32x4*>(w0 + 2 * WIDTH + row);
    f32x4 pre;
#pragma unroll
    for (int r = 0; r < 4; ++r) pre[r] = fmaf(wz[r], pt.z, fmaf(wy[r], pt.y, fmaf(wx[r], pt.x, c0[r])));
    return pre;
}

// latent_in layer: xyz re-enters at rows 445..447 (lane group 3); the code part is in the bias (cb_l + 512)
// (row 445 = tile 27, row 477 = tile 29 with 32-D codes; both are row 13 of their tile: lane group 3, registers 1..3)
__device__ __forceinline__ void reinject_xyz(float (&sin_)[128], int g, int lat_tile, const float4 pt) {
    // (element-wise selects: as a helper, two groups of stores under a branch on lat_tile came out of hipcc as one group at a run-time index
    // in mlp_split_kernel<2>, which put registers 109..120 of the slab into scratch memory)
    const bool lo = g == 3 && lat_tile != 29, hi = g == 3 && lat_tile == 29;
    sin_[109] = lo ? pt.x : sin_[109]; sin_[110] = lo ? pt.y : sin_[110]; sin_[111] = lo ? pt.z : sin_[111];
    sin_[117] = hi ? pt.x : sin_[117]; sin_[118] = hi ? pt.y : sin_[118]; sin_[119] = hi ? pt.z : sin_[119];
}

// first layer, backward: d y / d xyz = W0[:, xyz]^T ga0 on the VALU (ga0 = the input slab of this pass,
// which the pass epilogue overwrites); the MFMA pass itself only produces the 64 code rows.
// Returns d y / d (x|y|z by lane group) through the first layer.
__device__ __forceinline__ float first_layer_xyz_grad(const MlpArgs& a, const float* bias_l, int g, const float (&sin_)[128]) {
    const float* w0 = bias_l + a.w0_row * WIDTH + 4 * g;
    float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
    for (int t = 0; t < 32; ++t) {
        const f32x4 wx = *reinterpret_cast<const f32x4*>(w0 + 16 * t);
        const f32x4 wy = *reinterpret_cast<const f32x4*>(w0 + WIDTH + 16 * t);
        const f32x4 wz = *reinterpret_cast<const f32x4*>(w0 + 2 * WIDTH + 16 * t);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gx = fmaf(wx[r], sin_[4 * t + r], gx);
            gy = fmaf(wy[r], sin_[4 * t + r], gy);
            gz = fmaf(wz[r], sin_[4 * t + r], gz);
        }
    }
    gx += __shfl_xor(gx, 16); gx += __shfl_xor(gx, 32);
    gy += __shfl_xor(gy, 16); gy += __shfl_xor(gy, 32);
    gz += __shfl_xor(gz, 16); gz += __shfl_xor(gz, 32);
    return (g == 0) ? gx : (g == 1) ? gy : gz;
}

// final layer (512 -> 1) on the VALU + tanh  (deep_sdf_decoder.py:93,107-108)
__device__ __forceinline__ float final_layer_sdf(const MlpArgs& a, const float* bias_l, int g, const float (&sin_)[128]) {
    const float* wl = bias_l + a.wlast_row * WIDTH + 4 * g;
    float part = 0.f;
#pragma unroll
    for (int t = 0; t < 32; ++t) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wl + 16 * t);
        part = fmaf(sin_[4 * t + 0], w4.x, part);
        part = fmaf(sin_[4 * t + 1], w4.y, part);
        part = fmaf(sin_[4 * t + 2], w4.z, part);
        part = fmaf(sin_[4 * t + 3], w4.w, part);
    }
    part += __shfl_xor(part, 16);
    part += __shfl_xor(part, 32);
    return tanhf(part + a.b_last);
}

// seed of the backward sweep, rows 4g .. 4g + 3 of row tile t: d tanh * W_last (d = 1 - y^2), masked by the last hidden layer's relu
// (bits4: the row tile's four mask bits, row r at bit r)
__device__ __forceinline__ f32x4 backward_seed_rows(const MlpArgs& a, const float* bias_l, int g, int t, unsigned bits4, float d) {
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(bias_l + a.wlast_row * WIDTH + 4 * g + 16 * t);
    return (f32x4){(bits4 & 1u) ? d * w4.x : 0.f, (bits4 & 2u) ? d * w4.y : 0.f, (bits4 & 4u) ? d * w4.z : 0.f, (bits4 & 8u) ? d * w4.w : 0.f};
}

// bias seed of a pass: the accumulators start from the layer's bias vector (pd.bias_row: a row of the bias table, -2 = the object's
// latent_in code bias; -1 = none: the caller seeds zeros and does not call this).
// (Only the choice of the vector is shared.  A helper that also filled the caller's f32x4[N], by reference or returned by value, cost
// mlp_split_kernel<2> 100 more live registers and 1000 copy instructions at the pass seams; the loads stay in the kernels.)
__device__ __forceinline__ const float* pass_bias_vec(int bias_row, const float* bias_l, const float* cb_l) {
    return bias_row == -2 ? cb_l + WIDTH : bias_l + bias_row * WIDTH;
}

// latent_in layer, backward (pd.kind == 4), 64-row output group og of the throughput / latency forms: rows 445..447 / 448..511 of the
// layer's input are the re-injected xyz / code, not relu outputs -- keep their gradients (unmasked) for the final d/d[code,xyz] sum
__device__ __forceinline__ void capture_skip_rows(int lat_tile, int og, const float (&v)[16], float (&skipx)[3], float (&skipc)[16]) {
    if (lat_tile != 29) {          // 64-D codes: xyz at rows 445..447, code at 448..511
        if (og == 6) { skipx[0] = v[13]; skipx[1] = v[14]; skipx[2] = v[15]; }
        if (og == 7) {
#pragma unroll
            for (int k = 0; k < 16; ++k) skipc[k] = v[k];
        }
    } else if (og == 7) {            // 32-D codes: xyz at rows 477..479, code at 480..511 (code index 16 (j - 2) + 4 g + r)
        skipx[0] = v[5]; skipx[1] = v[6]; skipx[2] = v[7];
#pragma unroll
        for (int k = 0; k < 8; ++k) skipc[k] = v[8 + k];
    }
}

// One row of the jacobian: d y / d code = the first layer's code rows (sin_[0..15]: rows 16t + 4g + r) + the latent_in skip rows;
// d y / d xyz = gfirst (by lane group) + the skip xyz rows, which lane group 3 holds; then y.  Every lane of the wave calls this (shuffles).
__device__ __forceinline__ void write_jgrad_row(float* orow, bool valid, int g, int pl, const float (&sin_)[128], const float (&skipc)[16],
                                                float skipx0, float skipx1, float skipx2, float gfirst, float y) {
    if (valid) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float4 o4;
            o4.x = sin_[4 * t + 0] + skipc[4 * t + 0];
            o4.y = sin_[4 * t + 1] + skipc[4 * t + 1];
            o4.z = sin_[4 * t + 2] + skipc[4 * t + 2];
            o4.w = sin_[4 * t + 3] + skipc[4 * t + 3];
            *reinterpret_cast<float4*>(orow + 16 * t + 4 * g) = o4;
        }
    }
    const float s0 = __shfl(skipx0, pl + 48);
    const float s1 = __shfl(skipx1, pl + 48);
    const float s2 = __shfl(skipx2, pl + 48);
    const float sk = (g == 0) ? s0 : (g == 1) ? s1 : s2;
    if (valid) orow[64 + g] = (g < 3) ? (gfirst + sk) : y;
}

// speculative band rows: the jacobian launch's fp32 sdf goes back to the sample's slot (pt.w), past the prepass guard
__device__ __forceinline__ void scatter_sdf(const MlpArgs& a, int obj, bool sc, const float4 pt, float y) {
    if (a.guard) prepass_guard(a, obj, sc, sc ? a.sdf_scatter[__float_as_int(pt.w)] : 1.0f, y);
    if (sc) a.sdf_scatter[__float_as_int(pt.w)] = y;
}

// Exported relu masks (mask_buf): per sample and lane group 64 u16 words, [slot 8][output group 8]; as u32 words, word 4 slot + w holds
// groups 2w (low half) and 2w + 1.  A thread that keeps NG groups per slot in LDS (mask_l[(slot * NG + group) * 256 + tid]; the throughput
// form all 8, the latency form its wave's 2) moves NG / 2 words per slot, from `first` = its first group's word on.
__device__ __forceinline__ unsigned* mask_words(const MlpArgs& a, int sample, int g) {
    return reinterpret_cast<unsigned*>(a.mask_buf + ((size_t)sample * 4 + g) * 64);
}
template <int NG>
__device__ __forceinline__ void export_masks(unsigned* first, const unsigned short* mask_l, int tid) {
    typedef unsigned words_t __attribute__((ext_vector_type(NG / 2)));
#pragma unroll
    for (int sl = 0; sl < MASK_SLOTS; ++sl) {
        words_t w;
#pragma unroll
        for (int e = 0; e < NG / 2; ++e)
            w[e] = (unsigned)mask_l[(NG * sl + 2 * e + 0) * 256 + tid] | ((unsigned)mask_l[(NG * sl + 2 * e + 1) * 256 + tid] << 16);
        *reinterpret_cast<words_t*>(first + 4 * sl) = w;
    }
}
template <int NG>
__device__ __forceinline__ void import_masks(const unsigned* first, bool valid, unsigned short* mask_l, int tid) {
    typedef unsigned words_t __attribute__((ext_vector_type(NG / 2)));
#pragma unroll
    for (int sl = 0; sl < MASK_SLOTS; ++sl) {
        words_t w = (words_t)(0u);
        if (valid) w = *reinterpret_cast<const words_t*>(first + 4 * sl);
#pragma unroll
        for (int e = 0; e < NG / 2; ++e) {
            mask_l[(NG * sl + 2 * e + 0) * 256 + tid] = (unsigned short)(w[e] & 0xffffu);
            mask_l[(NG * sl + 2 * e + 1) * 256 + tid] = (unsigned short)(w[e] >> 16);
        }
    }
}

// ---- per-wave weight ring of the latency and cluster forms -------------------------------------------------------------------------
// Waves of these forms share no A operands, so each streams its own rows through a private LDS ring of DEPTH mini-chunks of MINI bytes
// (4 steps x 64 lanes x 16 B; a step is a k-step in the latency form, a pair of k-steps in the cluster form): one ds_read_b128 and one
// LDS-DMA piece per step, counted vmcnt, no barrier.  The stream is one wrapping pointer per wave (the host lays the wave's chunks out
// in consumption order).  Per step: ahead(s) before the step's MFMAs, behind_first(s) behind its first, behind_last(s) behind its last.
// All state is wave-uniform; a slot's address is formed once per mini-chunk and carried as state (every instruction between two MFMAs
// costs matrix-pipe time), and every index into abuf is a constant once the step loops are unrolled.
template <int DEPTH, int MINI>
struct WaveRing {
    const char* wbase;          // the wave's stream
    const char* rd0;            // ring + lane * 16: this lane's A element of step 0, slot 0
    unsigned ring0, lane_off;
    int total;                  // stream length in mini-chunks
    int wrap_to;                // where the stream restarts (the latency form's mixed launch moves it per tile)
    int issue_pos, issue_slot, rd_slot;
    int nx_slot;                // the slot after rd_slot and this lane's address in it: formed once per mini-chunk (at m == 0), read through at
    const char* nx_rd;          // m == 2 and carried into the next mini-chunk, whose own reads (m == 0) use the same address
    const char* cur_rd;
    const char* isrc;
    unsigned idst;
    f32x4 abuf[4];              // A operands, read one pair of steps ahead

    __device__ __forceinline__ void issue_next() {
        issue_pos = (issue_pos + 1 == total) ? wrap_to : issue_pos + 1;
        issue_slot = (issue_slot + 1 == DEPTH) ? 0 : issue_slot + 1;
        isrc = wbase + (size_t)issue_pos * MINI;
        idst = ring0 + issue_slot * MINI;
    }
    // fills DEPTH - 1 slots from mini-chunk `start` on and reads the first pair of A operands
    __device__ __forceinline__ void prime(const char* stream, char* ring, int lane, int total_minis, int start) {
        wbase = stream; rd0 = ring + lane * 16; ring0 = lds_addr(ring); lane_off = lane * 16;
        total = total_minis; wrap_to = start;
        issue_pos = start; issue_slot = 0; rd_slot = 0; cur_rd = rd0;
        isrc = wbase + (size_t)issue_pos * MINI;
        idst = ring0;
#pragma unroll
        for (int i = 0; i < DEPTH - 1; ++i) { glds_quarter(isrc, lane_off, idst); issue_next(); }
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (DEPTH - 2)) : "memory");     // mini-chunk 0 has landed
        abuf[0] = *reinterpret_cast<const f32x4*>(rd0);
        abuf[1] = *reinterpret_cast<const f32x4*>(rd0 + 1024);
    }
    // step s (counted from a mini-chunk boundary; s & 3 = step inside the mini-chunk); the step's A operand is abuf[s % 4] afterwards
    __device__ __forceinline__ void ahead(int s) {
        static_assert(PAIR_READS == 2, "pairs");
        const int m = s & 3;
        if (m == 2) {
            // the next mini-chunk is about to be read: it has landed once only the two mini-chunks
            // after it and the two pieces issued so far in this one are still in flight
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (DEPTH - 3) + 2) : "memory");
        }
        // A operands in pairs, one lgkmcnt wait per pair (PAIR_READS above): at m == 2 the pair belongs to the next
        // mini-chunk, which the vmcnt wait above has just proven landed
        if ((s & 1) == 0) {
            __builtin_amdgcn_s_waitcnt(0xC07F);     // lgkmcnt(0), vmcnt / expcnt untouched
            __builtin_amdgcn_sched_barrier(0);
            if (m == 0) {       // two steps ahead of the first read through it: the SALU -> VALU -> LDS chain of the address is off that read's path
                nx_slot = (rd_slot + 1 == DEPTH) ? 0 : rd_slot + 1;
                nx_rd = rd0 + nx_slot * MINI;
            }
            const char* p = (m == 0) ? cur_rd + 2048 : nx_rd;
            abuf[(s + 2) % 4] = *reinterpret_cast<const f32x4*>(p);
            abuf[(s + 3) % 4] = *reinterpret_cast<const f32x4*>(p + 1024);
        }
    }
    // refill of the slot behind the read pointer: one DMA piece per step, behind an MFMA
    __device__ __forceinline__ void behind_first(int s) {
        const int m = s & 3;
        if (m == 0) { glds_set_dst(idst); glds_piece_m0<0>(isrc, lane_off, idst); }
        if (m == 1) glds_piece_m0<1>(isrc, lane_off, idst);
        if (m == 2) glds_piece_m0<2>(isrc, lane_off, idst);
        if (m == 3) { glds_piece_m0<3>(isrc, lane_off, idst); issue_next(); }
    }
    __device__ __forceinline__ void behind_last(int s) {
        // pin "read for step s+2, then the MFMAs of step s": left alone, hipcc sinks every ds_read next to its use
        __builtin_amdgcn_sched_barrier(0);
        if ((s & 3) == 3) { rd_slot = nx_slot; cur_rd = nx_rd; }
    }
};

}  // namespace dsp
