// DeepSDF decoder forward in f16 / bf16 MFMA for gfx950 (MI355X): the PREPASS that classifies ray samples.
//
// Not a replacement for the fp32 decoder (mlp_kernel.hip) -- an exact filter in front of it.  The render term only looks at
// clamp(sdf, -th, th) (reconstruct/loss_utils.py:40-48, reconstruct/loss.py:84-96): occupancy is exactly 0 for sdf >= th
// and exactly 1 for sdf <= -th.  A sample whose low-precision sdf is farther than a calibrated margin delta from the band
// |sdf| < th is therefore classified for good, bit-exactly, and only the samples inside the widened band are decoded in
// fp32 (dsp_gn.hip, "prepass").
//
// Structure (DESIGN.md "K0"): one workgroup = 4 waves = one 128-point tile, one wave per SIMD.  A wave owns 32 points as TWO column
// blocks of 16 and keeps its [512 rows x 32 points] activation slab in registers as packed 16-bit pairs (128 registers; two slabs X, Y
// ping-pong between layers).  Round 5: the matrix instruction is v_mfma_f32_16x16x32_{f16,bf16} (rounds 2-4: 32x32x16).  A register-only
// probe with live (random) operand data holds 2.13 GHz on the 16x16x32 form and 1.78 GHz on the 32x32x16 form (same FLOP per cycle:
// tools/probes/mfma16_probe.hip, profiles/r05_k0_clock.md) -- the chip's clock under dense 16-bit MFMA follows the switching power, and the
// 16x16 form switches less per FLOP.  One A fragment (16 output rows x 32 k, one ds_read_b128 per lane) feeds both column blocks: the
// LDS duty is what it was (1 KiB per 32 matrix-pipe cycles and wave).
//
// Lane maps: A lane l = row l & 15, k slots 8 (l >> 4) + e; B lane l = point l & 15, the same k slots (the pairing of A and B slots is all
// that matters); D lane l = point l & 15, rows 4 (l >> 4) + r of the 16-row tile.  After v_cvt_pk the D registers of row tiles 2q, 2q + 1
// ARE the B operand of the next layer's 32-k step q if that layer's weights are packed with the slot order
// krow(q, gq, e) = 32 q + 16 (e >> 2) + 4 gq + (e & 3)  (pack_decoder_lp_host; tests/lp_emulator.py pins it on the CPU).
// Weights stream through an 8-slot LDS ring of 16 KiB chunks (4 steps of 32 k x 4 row tiles x 1 KiB A fragment) by LDS-DMA, one piece
// behind an MFMA, counted vmcnt + one s_barrier per chunk -- the protocol of mlp_kernel.hip at 4x the chunk rate.  The relu / v_cvt_pk
// epilogue of output group g-1 is interleaved with the MFMAs of group g (two accumulator sets).  xyz enters layer 0 and the latent_in
// layer through one 32-k step of split-precision products (LP_XYZ_TERMS), the code through the fp32 per-object bias (k_code_bias),
// biases are the fp32 C operand of each tile's first MFMA, and the final 512 -> 1 layer + tanh is an fp32 VALU dot product on the
// un-rounded accumulators of the last hidden layer.  The layer pass with its schedule, the kernel set-up and a tile's front live in
// mlp_lp_common.h, where the kernels of mlp_lpj_kernel.hip find them too: here are the tile loop and what is this kernel's alone.
#include "mlp_lp_common.h"

namespace dsp {

// Four waves, one per SIMD.  (Eight waves of one column block each -- two per SIMD, one wave's reads and epilogue in the slots the other's
// MFMAs leave -- were measured: duty 0.71 against 0.67, granted clock -150 MHz, slower; profiles/r05_k0_clock.md, r06_removed_experiments.md.)
template <bool BF, int NBLK>
__global__ __launch_bounds__(256, 1) void mlp_lp_kernel(const LpArgs a) {
    constexpr int TILE = 16 * NBLK * 4;     // LP_TILE_PTS for NBLK = 2
    const LpCtx w = lp_ctx();
    DirectList dl{0, 0, 0, 0};
    if (a.direct.kind) {
        dl = direct_list(a.direct, TILE);
        if (blockIdx.x == 0 && w.tid == 0) direct_commit(a.direct, dl);
    }
    const int n_tiles = a.direct.kind ? dl.n_tiles : *a.n_tiles;
    if ((int)blockIdx.x >= n_tiles) return;
    LpRing rg;
    u32x4 abuf[2][LP_RT], X[32], Y[32];
    f32x4 acc[2][LP_RT][2];
    lp_setup(a, w, rg, abuf, X, Y, acc, [](int) {});
    const float* wl = w.bias_l + a.wlast_row * WIDTH;

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int4 td = a.direct.kind ? direct_tile(a.direct, dl, tile, TILE) : a.tiles[tile];
        bool valid[2];
        int pidx[2], src[2];
        u32x4 xb[2];
        lp_tile_front<BF, NBLK>(a, a.index, td, w, valid, pidx, src, xb);
        float part[2] = {0.f, 0.f};
        const LpEpiRelu<BF, LpNoMask> hidden{};
        // Pass bodies: first layer (Y -> X: the slabs ping-pong), hidden layers X -> Y and Y -> X, and the LAST hidden layer, which reads X and
        // writes no slab.  The pass count is even (pack_decoder_lp_host refuses others: the prepass is then off), so the last layer's input is
        // always in X and the loop has no conditional half -- a join there costs ~120 spilled registers per tile.
        const int n_mid = a.n_pass - 2;      // hidden layers between the first and the last one
        lp_pass<BF, 1, NBLK, LP_NOG>(a.pass[0], Y, X, acc, abuf, rg, xb, lp_bias_of(w, a.pass[0]), w.gq, hidden);
        for (int ps = 1; ps < n_mid; ps += 2) {
            lp_pass<BF, LP_NCH, NBLK, LP_NOG>(a.pass[ps], X, Y, acc, abuf, rg, xb, lp_bias_of(w, a.pass[ps]), w.gq, hidden);
            lp_pass<BF, LP_NCH, NBLK, LP_NOG>(a.pass[ps + 1], Y, X, acc, abuf, rg, xb, lp_bias_of(w, a.pass[ps + 1]), w.gq, hidden);
        }
        lp_pass<BF, LP_NCH, NBLK, LP_NOG>(a.pass[a.n_pass - 1], X, Y, acc, abuf, rg, xb, lp_bias_of(w, a.pass[a.n_pass - 1]), w.gq, LpEpiDot<LpNoMask>{wl, w.gq, part, {}, {}});
        float y = lp_finish(part[0], part[1], w.gq, a.b_last);
        // exactly 1.0f is the optimiser's "never decoded" placeholder (gn_kernels.hip: sample_write_ray): a prepass value never takes it.
        // (tanh saturates to 1.0f above ~9 -- or after an f16 overflow upstream.)  NaN stays NaN: the band kernels send it to the fp32 kernel.
        if (y >= 1.0f) y = 0x1.fffffep-1f;
        const int sb = w.gq & 1;
        if (w.gq < NBLK && (sb ? valid[1] : valid[0])) a.out_sdf[a.index ? (sb ? src[1] : src[0]) : (sb ? pidx[1] : pidx[0]) + td.w] = y;
        // stores and LDS-DMA share vmcnt and may retire out of order: drain before counting again
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lp_stamp(a.clk, 2, w.tid);
}

static void (*const LP_KERNELS[2][2])(const LpArgs) = {{mlp_lp_kernel<false, 2>, mlp_lp_kernel<true, 2>}, {mlp_lp_kernel<false, 1>, mlp_lp_kernel<true, 1>}};     // [small tiles][bf16]

hipError_t mlp_lp_prepare_device() {
    for (int i = 0; i < 4; ++i) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(LP_KERNELS[i >> 1][i & 1]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LP_LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// tile_pts: LP_TILE_PTS (128: two column blocks per wave) or LP_TILE_PTS_SMALL (64: one); the tile list must have been built for it
hipError_t launch_mlp_lp(bool bf16, const LpArgs& args, int n_blocks, hipStream_t stream, int tile_pts) {
    hipLaunchKernelGGL(LP_KERNELS[tile_pts == LP_TILE_PTS_SMALL][bf16], dim3(n_blocks), dim3(256), LP_LDS_BYTES, stream, args);
    return hipGetLastError();
}

}  // namespace dsp
