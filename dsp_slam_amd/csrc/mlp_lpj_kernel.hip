// DeepSDF decoder forward + input gradient in f16 / bf16 MFMA for gfx950 (MI355X): the jacobian kernel of the LOW-PRECISION COMPUTE MODE
// (dsp_batch_set_compute(DSP_COMPUTE_F16), include/dsp_gn.h) -- an opt-in, non-parity fast path: BASELINE.json's north_star names "fp32/bf16
// GEMMs", SURVEY.md section 8(d) allows it "reported separately, never mixed into the fp32 fraction".  The default path (mlp_kernel.hip, fp32
// v_mfma_f32_16x16x4_f32) is untouched by it.
//
// Replaces get_batch_sdf_jacobian (reconstruct/loss_utils.py:82-103) with 16-bit matrix operands and fp32 accumulation -- the precision class
// the reference's authors ran in (PyTorch 1.10 on Ampere multiplies in TF32: 10-bit mantissas like f16's, fp32 accumulation).
//
// Structure: mlp_lp_kernel.hip's (one workgroup = 4 waves = one 128-point tile, a wave = 32 points as two 16-point column blocks, activation
// slabs X / Y in registers as packed 16-bit pairs, v_mfma_f32_16x16x32, weights through an 8-slot LDS ring by LDS-DMA), as TWO kernels over the
// same tile list (one kernel holding both sweeps wants more than the 512 registers a lane has: 197 spilled, measured):
//   mlp_lpj_fwd_kernel   the prepass kernel's eight passes, bit for bit: the same lp_setup / lp_tile_front / lp_pass of mlp_lp_common.h over the same
//                        stream, and the prepass kernel's own epilogue policies with a mask export plugged in (so the sdf equals
//                        mlp_lp_kernel's, which only clamps an exact 1.0f away).  Every pass
//                        also emits its relu mask: 128 bits per lane and column block (bit = accumulator > 0), 64 KiB per tile in global memory
//                        (the LDS is full: ring 128 KiB + tables).  Writes the sdf into the point's output row.
//   mlp_lpj_bwd_kernel   builds the backward sweep's input slab from the last hidden layer's mask -- S w_last where the accumulator was positive
//                        (S = 16: keeps small gradient entries out of f16's subnormals; d tanh = 1 - y^2 and 1 / S multiply the result at the end,
//                        in fp32) -- and runs eight passes over the TRANSPOSED weights (a stream of its own, packed by pack_decoder_lpj_host in the
//                        same slot order): the epilogue ANDs each accumulator with its mask bit instead of the relu, rounds and packs.  The
//                        latent_in layer's pass also yields the gradient of the re-injected [xyz | code] rows (unmasked; kept as packed pairs,
//                        20 registers), the first layer's pass leaves d sdf / d [code | xyz] in the accumulators: + the kept rows,
//                        x (1 - y^2) / S, stored as the fp32 kernel stores it (68 floats per point: d/dcode[64], d/dxyz[3], sdf).
// Masks travel through memory that the kernels also stream weights through by hand-counted vmcnt.  The forward kernel's mask stores are
// compiler-managed: they add to the counter, so a counted wait can only wait LONGER than needed (outstanding <= k still implies that at most k
// DMA pieces are in flight).  The backward kernel fetches a layer's masks by LDS-DMA a pass ahead of their use into the (otherwise unused) bias
// area and reads them back from the LDS: a compiler-managed global load would put an s_waitcnt vmcnt(0) in front of the first use and drain
// the weight ring once per pass (measured: profiles/r06_lp_compute.md).
#include "mlp_lp_common.h"

namespace dsp {

constexpr float LPJ_SEED_SCALE = 16.f;
constexpr int LPJ_SKIP_T0 = 27;            // first 16-row tile that may hold re-injected input rows of the latent_in layer (27: 64-D codes, 29: 32-D)
constexpr int LPJ_SKIP_TILES = 32 - LPJ_SKIP_T0;
constexpr int LPJ_MASK_TILE = 8 * 4 * 2 * 64;      // uint4 per 128-point tile: [layer 8][wave 4][column block 2][lane 64]

// relu-mask bit of one accumulator, shifted into `bits` (bits = 2 * bits + (x > 0)): v_cmp + v_addc (mlp_kernel.hip).  Element i of the 32
// pushed into a word ends at bit 31 - i.
__device__ __forceinline__ void lpj_push_bit(unsigned& bits, float x) {
    asm volatile("v_cmp_lt_f32 vcc, 0, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(bits) : "v"(x) : "vcc");
}
// x where bit (31 - i) of word is set, else +0: one v_bfe_i32 (0 / all ones) + one v_and
__device__ __forceinline__ float lpj_keep(float x, unsigned word, int i) {
    return __int_as_float(__float_as_int(x) & __builtin_amdgcn_sbfe((int)word, 31u - (unsigned)i, 1u));
}

// one layer's masks of one wave (two column blocks, 2 x 1 KiB) from global memory into its staging buffer by LDS-DMA.  Writes M0: only between
// a chunk's last DMA piece and the next chunk's glds_set_dst, i.e. outside lp_pass
__device__ __forceinline__ void lpj_mask_dma(const char* gsrc_uniform, unsigned lane_off, unsigned lds_dst) {
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %1\n\t"
        "global_load_lds_dwordx4 %0, %1 offset:1024"
        :
        : "v"(lane_off), "s"(gsrc_uniform), "s"(lds_dst)
        : "memory");
}

// The epilogue policies of the two kernels (mlp_lp_common.h: lp_pass), built at the call site around the kernel's own registers.
// Forward: the prepass kernel's own epilogues (LpEpiRelu / LpEpiDot), with every accumulator's relu-mask bit going out into mw on the way.
struct LpjMaskOut {
    unsigned (&mw)[2][4];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < 8; ++i) mw[i >> 2][i & 3] = 0u;
    }
    __device__ __forceinline__ void push(int T, int blk, float e0, float e1) {
        lpj_push_bit(mw[blk][T >> 3], e0);
        lpj_push_bit(mw[blk][T >> 3], e1);
    }
};
// Backward: the mask bits of mw applied instead of the relu.  With `cap` (wave-uniform: the latent_in layer's pass) the rows that are re-injected
// input are kept unmasked as well.  KEEP: the sweep's FIRST layer, whose accumulators are the result.
template <bool BF, bool KEEP>
struct LpjEpiMaskIn {
    static constexpr bool XYZ_PROLOGUE = false, KEEP_ACC = KEEP;
    unsigned (&mw)[2][4]; unsigned (&skip)[LPJ_SKIP_TILES][2][2]; bool cap;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void half(int T, int blk, int h, float e0, float e1, u32x4 (&out)[32]) {
        const int i0 = 4 * (T & 7) + 2 * h;                  // element index of e0 inside its mask word (T >> 3)
        if (T >= LPJ_SKIP_T0) {          // (compile-time)
            const unsigned raw = lp_pack<BF>(e0, e1);
            skip[T - LPJ_SKIP_T0][blk][h] = cap ? raw : skip[T - LPJ_SKIP_T0][blk][h];
        }
        out[2 * (T >> 1) + blk][2 * (T & 1) + h] = lp_pack<BF>(lpj_keep(e0, mw[blk][T >> 3], i0), lpj_keep(e1, mw[blk][T >> 3], i0 + 1));
    }
};

template <bool BF>
__device__ __forceinline__ f32x2 lpj_unpack(unsigned p) {
    if constexpr (BF) return __builtin_convertvector(__builtin_bit_cast(b2, p), f32x2);
    else return __builtin_convertvector(__builtin_bit_cast(h2, p), f32x2);
}

// ---- forward with mask export: tile t's masks at mask_buf[t * 4096 + ((slot * 4 + wave) * 2 + blk) * 64 + lane], slot = layer ----
template <bool BF>
__global__ __launch_bounds__(256, 1) void mlp_lpj_fwd_kernel(const LpjArgs a) {
    const LpCtx w = lp_ctx();
    const int n_tiles = *a.n_tiles;
    if ((int)blockIdx.x >= n_tiles) return;
    LpRing rg;
    u32x4 abuf[2][LP_RT], X[32], Y[32];
    f32x4 acc[2][LP_RT][2];
    lp_setup(a, w, rg, abuf, X, Y, acc, [](int) {});
    const float* wl = w.bias_l + a.wlast_row * WIDTH;
    unsigned mw[2][4];
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int4 td = a.tiles[tile];
        bool valid[2];
        int pidx[2], src[2];
        u32x4 xb[2];
        lp_tile_front<BF, 2>(a, nullptr, td, w, valid, pidx, src, xb);
        float part[2] = {0.f, 0.f};
        uint4* msc = a.mask_buf + (size_t)tile * LPJ_MASK_TILE + w.wave * 128 + w.lane;
        auto store_masks = [&](int slot) {
            msc[slot * 512] = make_uint4(mw[0][0], mw[0][1], mw[0][2], mw[0][3]);
            msc[slot * 512 + 64] = make_uint4(mw[1][0], mw[1][1], mw[1][2], mw[1][3]);
        };
        const LpEpiRelu<BF, LpjMaskOut> hidden{{mw}};
        // the prepass kernel's passes: first layer Y -> X, then X -> Y / Y -> X pairs, the last hidden layer reads X (eight hidden layers: the host
        // offers this kernel for that depth only)
        lp_pass<BF, 1, 2, LP_NOG>(a.pass[0], Y, X, acc, abuf, rg, xb, lp_bias_of(w, a.pass[0]), w.gq, hidden);
        store_masks(0);
        for (int ps = 1; ps < 7; ps += 2) {
            lp_pass<BF, LP_NCH, 2, LP_NOG>(a.pass[ps], X, Y, acc, abuf, rg, xb, lp_bias_of(w, a.pass[ps]), w.gq, hidden);
            store_masks(ps);
            lp_pass<BF, LP_NCH, 2, LP_NOG>(a.pass[ps + 1], Y, X, acc, abuf, rg, xb, lp_bias_of(w, a.pass[ps + 1]), w.gq, hidden);
            store_masks(ps + 1);
        }
        lp_pass<BF, LP_NCH, 2, LP_NOG>(a.pass[7], X, Y, acc, abuf, rg, xb, lp_bias_of(w, a.pass[7]), w.gq, LpEpiDot<LpjMaskOut>{wl, w.gq, part, {mw}, {}});
        store_masks(7);
        const float y = lp_finish(part[0], part[1], w.gq, a.b_last);        // as the prepass kernel's, without its clamp of an exact 1.0f
        const int sb = w.gq & 1;
        if (w.gq < 2 && (sb ? valid[1] : valid[0])) a.out_grad[(size_t)((sb ? pidx[1] : pidx[0]) + td.w) * GRAD_STRIDE + 67] = y;
        // stores and LDS-DMA share vmcnt and may retire out of order: drain before counting again
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lp_stamp(a.clk, 2, w.tid);
}

// ---- backward from the exported masks ----
template <bool BF>
__global__ __launch_bounds__(256, 1) void mlp_lpj_bwd_kernel(const LpjArgs a) {
    const LpCtx w = lp_ctx();
    const int n_tiles = *a.n_tiles;
    if ((int)blockIdx.x >= n_tiles) return;
    LpRing rg;
    u32x4 abuf[2][LP_RT], X[32], Y[32];
    f32x4 acc[2][LP_RT][2];
    // S x the final layer's weights live in the (otherwise unused) per-object code-bias area of the LDS carve-up
    lp_setup(a, w, rg, abuf, X, Y, acc, [&](int i) { w.cb_l[i] = LPJ_SEED_SCALE * a.bias_tab[a.wlast_row * WIDTH + i]; });
    unsigned mw[2][4];
    unsigned skip[LPJ_SKIP_TILES][2][2];
    u32x4 xb[2] = {(u32x4){0u, 0u, 0u, 0u}, (u32x4){0u, 0u, 0u, 0u}};
    // mask staging: two 8 KiB buffers in the bias area (the backward sweep adds no bias), [wave][column block][lane] uint4 each
    const unsigned stage0 = lds_addr(w.bias_l) + w.wave * 2048;
    const uint4* stage_l = reinterpret_cast<const uint4*>(w.bias_l) + w.wave * 128 + w.lane;
    const char* mbase = reinterpret_cast<const char*>(a.mask_buf) + w.wave * 2048;
    lpj_mask_dma(mbase + (size_t)blockIdx.x * (LPJ_MASK_TILE * 16) + 7 * 8192, rg.lane_off, stage0);
    lpj_mask_dma(mbase + (size_t)blockIdx.x * (LPJ_MASK_TILE * 16) + 6 * 8192, rg.lane_off, stage0 + 8192);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int4 td = a.tiles[tile];
        bool valid[2];
        int prow[2];
        float y[2];
        lp_tile_rows<2>(td, w, valid, prow);
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            prow[blk] += td.w;
            y[blk] = valid[blk] ? a.out_grad[(size_t)prow[blk] * GRAD_STRIDE + 67] : 0.f;      // the forward kernel's sdf
        }
        // next tile of this workgroup (the last one fetches its own masks again: no branch around the DMA)
        const int ntile = tile + (int)gridDim.x < n_tiles ? tile + (int)gridDim.x : tile;
        const char* msrc = mbase + (size_t)tile * (LPJ_MASK_TILE * 16), *nsrc = mbase + (size_t)ntile * (LPJ_MASK_TILE * 16);
        // masks of layer `slot`: staged by fetch_masks a pass earlier, read back by the lanes that the DMA wrote them for
        auto fetch_masks = [&](const char* src, int slot, int buf) { lpj_mask_dma(src + slot * 8192, rg.lane_off, stage0 + buf * 8192); };
        auto load_masks = [&](int buf) {
            const uint4 m0 = stage_l[buf * 512], m1 = stage_l[buf * 512 + 64];
            mw[0][0] = m0.x; mw[0][1] = m0.y; mw[0][2] = m0.z; mw[0][3] = m0.w;
            mw[1][0] = m1.x; mw[1][1] = m1.y; mw[1][2] = m1.z; mw[1][3] = m1.w;
        };
#pragma unroll
        for (int t = 0; t < LPJ_SKIP_TILES; ++t)
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2) { skip[t][b2][0] = 0u; skip[t][b2][1] = 0u; }
        // the sweep's input slab: S w_last where the last hidden layer's accumulator was positive (its mask, slot 7), in the slab's slot order --
        // registers 2 (T & 1), 2 (T & 1) + 1 of Y[2 (T >> 1) + blk] hold rows 16 T + 4 gq + {0, 1}, {2, 3}
        load_masks(0);
#pragma unroll
        for (int T = 0; T < 32; ++T) {
            const f32x4 ws = *reinterpret_cast<const f32x4*>(w.cb_l + 16 * T + 4 * w.gq);
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const unsigned word = mw[blk][T >> 3];
                const int i0 = 4 * (T & 7);
                Y[2 * (T >> 1) + blk][2 * (T & 1) + 0] = lp_pack<BF>(lpj_keep(ws.x, word, i0), lpj_keep(ws.y, word, i0 + 1));
                Y[2 * (T >> 1) + blk][2 * (T & 1) + 1] = lp_pack<BF>(lpj_keep(ws.z, word, i0 + 2), lpj_keep(ws.w, word, i0 + 3));
            }
        }
        // layers 7 .. 0, straight-line (pass 7 - L of the table, masks of layer L - 1): eight hidden layers with the latent_in layer fourth -- DeepSDF's
        // geometry, the only one the host offers this kernel for.  No loop and no branch: a join with both slabs live costs the compiler a hundred
        // spilled registers (mlp_lp_kernel.hip).
        // staging: buffer 0 holds layer 7's masks and buffer 1 layer 6's when the tile starts (fetched during the previous tile's pass 6 / 7, or
        // ahead of the loop); the pass that reads buffer b fetches the masks of the pass after it into the other buffer, whose last reader is a
        // pass behind.  A fetch is two LDS-DMA pieces older than the 32 (8) chunks the pass then issues: the ring's counted waits (at most 20
        // pieces outstanding) retire it within five chunks.
        // Passes 1 .. 6 are ONE loop body of two passes run three times (the latent_in layer's pass differs from its neighbours by a uniform flag):
        // four pass bodies of ~25 KB instead of eight (203 -> 100 KB of code per tile against a 64 KB instruction cache): 8 % faster, measured.
        using Masked = LpjEpiMaskIn<BF, false>;
        load_masks(1); fetch_masks(msrc, 5, 0);
        lp_pass<BF, LP_NCH, 2, LP_NOG>(a.pass[0], Y, X, acc, abuf, rg, xb, w.zero_l, w.gq, Masked{mw, skip, false});
        for (int it = 0; it < 3; ++it) {
            load_masks(0); fetch_masks(msrc, 4 - 2 * it, 1);
            lp_pass<BF, LP_NCH, 2, LP_NOG>(a.pass[2 * it + 1], X, Y, acc, abuf, rg, xb, w.zero_l, w.gq, Masked{mw, skip, it == 1});
            load_masks(1); fetch_masks(it < 2 ? msrc : nsrc, it < 2 ? 3 - 2 * it : 7, 0);
            lp_pass<BF, LP_NCH, 2, LP_NOG>(a.pass[2 * it + 2], Y, X, acc, abuf, rg, xb, w.zero_l, w.gq, Masked{mw, skip, false});
        }
        fetch_masks(nsrc, 6, 1);
        lp_pass<BF, LP_NCH, 2, 2>(a.pass[7], X, Y, acc, abuf, rg, xb, w.zero_l, w.gq, LpjEpiMaskIn<BF, true>{mw, skip, false});
        // acc[0][j][blk]: rows 16 j + 4 gq + r of d / d code through the first layer (j < 4); acc[1][0][blk]: lane group 3, registers 1..3 =
        // d / d xyz through the first layer (rows 77..79 of the pass).  + the rows the latent_in layer's pass kept; x (1 - y^2) / S.
        // 64-D codes: xyz in tile 27, code in 28..31; 32-D: xyz in 29, code in 30..31.  Chosen by mask arithmetic (a ternary on the register array
        // becomes a run-time index, which sends the array to scratch memory)
        const unsigned m64 = a.lat_tile == LPJ_SKIP_T0 ? 0xffffffffu : 0u, m32 = ~m64;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const float sc = (1.f - y[blk] * y[blk]) * (1.f / LPJ_SEED_SCALE);
            float* orow = a.out_grad + (size_t)prow[blk] * GRAD_STRIDE;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // code tile j of the kept rows: tile lat_tile + 1 + j while it exists
                const unsigned s0 = (skip[1 + j][blk][0] & m64) | (j < 2 ? skip[(3 + j) % LPJ_SKIP_TILES][blk][0] & m32 : 0u);
                const unsigned s1 = (skip[1 + j][blk][1] & m64) | (j < 2 ? skip[(3 + j) % LPJ_SKIP_TILES][blk][1] & m32 : 0u);
                const f32x2 k0 = lpj_unpack<BF>(s0), k1 = lpj_unpack<BF>(s1);
                const f32x4 g4 = acc[0][j][blk];
                if (valid[blk])
                    *reinterpret_cast<float4*>(orow + 16 * j + 4 * w.gq) = make_float4((g4.x + k0.x) * sc, (g4.y + k0.y) * sc, (g4.z + k1.x) * sc, (g4.w + k1.y) * sc);
            }
            const unsigned x0 = (skip[0][blk][0] & m64) | (skip[2][blk][0] & m32), x1 = (skip[0][blk][1] & m64) | (skip[2][blk][1] & m32);
            const f32x2 k0 = lpj_unpack<BF>(x0), k1 = lpj_unpack<BF>(x1);
            const f32x4 gx = acc[1][0][blk];
            if (valid[blk] && w.gq == 3) *reinterpret_cast<float4*>(orow + 64) = make_float4((gx.y + k0.y) * sc, (gx.z + k1.x) * sc, (gx.w + k1.y) * sc, y[blk]);
        }
        // stores and LDS-DMA share vmcnt and may retire out of order: drain before counting again
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lp_stamp(a.clk, 2, w.tid);
}

static void (*const LPJ_KERNELS[2][2])(const LpjArgs) = {{mlp_lpj_fwd_kernel<false>, mlp_lpj_fwd_kernel<true>}, {mlp_lpj_bwd_kernel<false>, mlp_lpj_bwd_kernel<true>}};     // [which][bf16]

hipError_t mlp_lpj_prepare_device() {
    for (int i = 0; i < 4; ++i) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(LPJ_KERNELS[i >> 1][i & 1]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LP_LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// which: 0 = forward with mask export (args: the prepass stream and pass table), 1 = backward from the masks (args: the transposed stream)
hipError_t launch_mlp_lpj(int which, bool bf16, const LpjArgs& args, int n_blocks, hipStream_t stream) {
    hipLaunchKernelGGL(LPJ_KERNELS[which != 0][bf16], dim3(n_blocks), dim3(256), LP_LDS_BYTES, stream, args);
    return hipGetLastError();
}

}  // namespace dsp
