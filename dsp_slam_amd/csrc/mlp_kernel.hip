// DeepSDF decoder forward / forward+input-gradient for gfx950 (MI355X), fp32 MFMA.
//
// Replaces, for batches of object-frame points:
//   decode_sdf              reconstruct/loss_utils.py:51-79   (mlp_kernel<0 / 1>)
//   get_batch_sdf_jacobian  reconstruct/loss_utils.py:82-103  (mlp_kernel<2>, <3>)
//   Decoder.forward         deep_sdf/deep_sdf_decoder.py:75-110
//
// Design (DESIGN.md "K1/K2"):  one workgroup = 4 waves = one 64-point tile, one wave per SIMD with the
// whole 512-entry register file.  Each wave owns 16 points and keeps its [512 rows x 16 points]
// activation slab IN REGISTERS for the whole network: v_mfma_f32_16x16x4_f32 produces D[row][pt] with
// lane (pt = l&15, g = l>>4) holding rows 4g..4g+3 of each 16-row tile -- which is exactly the B-operand
// layout (k = l>>4) of the next layer if that layer's weights are packed with the matching k
// permutation.  So activations never touch LDS or HBM; only the weights stream through a 6-deep LDS
// ring filled by LDS-DMA (global_load_lds_dwordx4) with counted vmcnt waits and one s_barrier per
// 16 KiB chunk (64 MFMAs per wave).  ReLU masks for the backward sweep live in LDS (32 KiB).
#include "dsp_internal.h"
#include "mlp_common.h"

namespace dsp {

constexpr int ZERO_VEC_BYTES = WIDTH * 4;     // behind the weight ring: see zero_l

#define FOR16(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15)

// MODE 0: forward only.  MODE 1: forward, relu masks kept and exported (with nothing else to do) for every sample whose
// |sdf| < th -- the candidates of the render term.  MODE 2: forward + backward (input gradient).  MODE 3: backward only,
// from the masks and sdf a MODE 1 launch exported for the same point and code (the render rows of the jacobian: their
// forward pass is not repeated).
template <int MODE>
__global__ __launch_bounds__(256, 1) void mlp_kernel(const MlpArgs a) {
    constexpr bool BWD = MODE >= 2;        // runs the backward sweep
    constexpr bool MASKS = MODE != 0;      // relu masks live in LDS
    constexpr bool DOFWD = MODE != 3;      // runs the forward sweep
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;    // MFMA k index of this lane group == 4-row block inside a 16-row tile
    const int pl = lane & 15;   // point of this lane inside the wave

    const DecoderLds lds = carve_lds(smem);
    float* const bias_l = lds.bias;
    float* const cb_l = lds.cb;
    unsigned short* const mask_l = lds.mask;
    char* ring_ptr = smem + LDS_HEAD_BYTES + (MASKS ? MASK_BYTES : 0);
    const unsigned ring0 = lds_addr(ring_ptr);
    // one all-zero 512-entry vector behind the ring: the "bias" of the passes that have none (pd.bias_row == -1), so that every
    // group's accumulators are seeded by the same four LDS reads, without a branch in the MFMA stream
    float* const zero_l = reinterpret_cast<float*>(ring_ptr + NBUF * CHUNK_BYTES);

    const int n_tiles = *a.n_tiles;
    const int tile0 = a.tile_begin ? *a.tile_begin : 0;
    if (tile0 + (int)blockIdx.x >= n_tiles) return;
    if (a.clk && blockIdx.x == 0 && tid == 0) { a.clk[0] = clock64(); a.clk[1] = wall_clock64(); }
    if (tid < ZERO_VEC_BYTES / 16) reinterpret_cast<float4*>(zero_l)[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    stage_bias_table(a, bias_l, tid);     // (its barrier publishes the zero vector as well)

    // ---- weight stream state (all wave-uniform) ---------------------------------------------------
    int issue_pos = 0, issue_slot = 0, rd_slot = 0;
    const char* wbase = reinterpret_cast<const char*>(a.wstream) + wave * 4096;   // wave-uniform; the lane part is lane_off
    const unsigned lane_off = lane * 16;
    const int total_chunks = a.total_chunks;
    // A chunk refill is four LDS-DMA instructions per wave.  Each costs ~30-60 issue cycles (64 lane addresses through
    // the address unit), so in the main loop they are spread over four k-steps, one behind an MFMA each, instead of
    // stalling the matrix pipe for a whole burst (measured: the burst form cost 5 % of the kernel).
    const char* isrc = wbase;
    unsigned idst = ring0 + wave * 4096;
    auto issue_next = [&]() {   // advance to the next chunk of the stream / next ring slot
        issue_pos = (issue_pos + 1 == total_chunks) ? 0 : issue_pos + 1;
        issue_slot = (issue_slot + 1 == NBUF) ? 0 : issue_slot + 1;
        isrc = wbase + (size_t)issue_pos * CHUNK_BYTES;
        idst = ring0 + issue_slot * CHUNK_BYTES + wave * 4096;
    };
    auto issue = [&]() {
        glds_quarter(isrc, lane_off, idst);
        issue_next();
    };
#pragma unroll
    for (int i = 0; i < NBUF - 1; ++i) issue();
    // chunk 0 visible to every wave; from here on the barrier for chunk q+1 sits in the middle of chunk q
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(GLDS_PER_CHUNK * (NBUF - 2)) : "memory");
    f32x4 abuf[2 * PAIR_READS];   // A operands run one group of PAIR_READS k-steps ahead of the MFMAs, across chunk / group / pass seams
    static_assert(PAIR_READS == 2, "the prologue below reads the first group");
    abuf[0] = *reinterpret_cast<const f32x4*>(ring_ptr + lane * 16);
    abuf[1] = *reinterpret_cast<const f32x4*>(ring_ptr + lane * 16 + 1024);

    float sin_[128];   // input slab of the current pass:  sin_[4t+r] = row 16t + 4g + r of point pl
    f32x4 acc[2][4];   // MFMA accumulators of the output group being produced ([og & 1]) and of the one before / after it
    f32x4 outv[32];    // output slab being produced: the finished groups' row tiles, outv[4 og + j][r] = row 64 og + 16 j + 4 g + r
#pragma unroll
    for (int i = 0; i < 128; ++i) sin_[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) outv[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i >> 2][i & 3] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int tile = tile0 + blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int4 td = a.tiles[tile];
        const int local = wave * WAVE_PTS + pl;
        const bool valid = local < td.y;
        const int pidx = td.x + (valid ? local : 0);
        const int src = (MODE <= 1 && a.index) ? a.index[pidx] : pidx;
        float4 pt = a.pts[src];
        // prepass guard (mlp_common.h): the value this tile's result will replace is fetched NOW, with the point, so that its latency
        // hides behind the tile instead of stalling its last instructions (one register per lane for the tile's lifetime)
        float old_lp = 1.0f, guard_tol = 0.f;
        if (MODE <= 1 && a.guard) {
            if (valid && g == 0) old_lp = a.out_sdf[a.index ? src : pidx + td.w];
            guard_tol = 0.5f * __uint_as_float(a.guard[(size_t)td.z * a.guard_stride]);     // tile-uniform: the object's margin / 2
        }
        if (!valid) pt = make_float4(0.f, 0.f, 0.f, 0.f);
        if (DOFWD) {
            stage_code_bias(a, cb_l, td.z, tid);
            __syncthreads();
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                float pre[16];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 p4 = layer0_rows(a, bias_l, cb_l, g, 16 * (4 * o + j), pt);
#pragma unroll
                    for (int r = 0; r < 4; ++r) pre[4 * j + r] = p4[r];
                }
                if (MASKS) {
                    unsigned bits = 0;
#pragma unroll
                    for (int k = 15; k >= 0; --k) push_mask_bit(bits, pre[k]);
                    mask_l[(0 * 8 + o) * 256 + tid] = (unsigned short)bits;
                }
#pragma unroll
                for (int k = 0; k < 16; ++k) sin_[16 * o + k] = relu1(pre[k]);
            }
        }
        float skipc[16];
        float skipx[3];
        float y = 0.f;
        float gfirst = 0.f;   // d y / d (x|y|z by lane group) through the first layer
#pragma unroll
        for (int i = 0; i < 16; ++i) skipc[i] = 0.f;
        skipx[0] = skipx[1] = skipx[2] = 0.f;

        // seed of the backward sweep, all rows, from the relu masks of slot `slot`
        auto seed_backward = [&](int slot) {
            const float d = 1.f - y * y;
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const unsigned bits = mask_l[(slot * 8 + o) * 256 + tid];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 s4 = backward_seed_rows(a, bias_l, g, 4 * o + j, bits >> (4 * j), d);
#pragma unroll
                    for (int r = 0; r < 4; ++r) sin_[16 * o + 4 * j + r] = s4[r];
                }
            }
        };
        if (MODE == 3) {
            // masks and sdf of this point as the forward (MODE 1) launch of the same iteration exported them; each lane
            // only ever touches its own 64 mask words, so no barrier is needed
            const int sidx = __float_as_int(pt.w);
            import_masks<8>(mask_words(a, sidx, g), valid, mask_l, tid);
            y = valid ? a.sdf_in[sidx] : 0.f;
            seed_backward(a.seed_slot);
        }

        for (int ps = 0; ps < a.n_pass; ++ps) {
            const PassDesc pd = a.pass[ps];
            // ---- pass prologue ------------------------------------------------------------------------------------
            if (pd.kind == 2) reinject_xyz(sin_, g, a.lat_tile, pt);
            else if (BWD && pd.kind == 5) gfirst = first_layer_xyz_grad(a, bias_l, g, sin_);

            // Output groups run one after the other on two ping-pong sets of four accumulator tiles (acc[og & 1][j], 32 AGPRs); a finished
            // group's 64 rows wait in outv for the layer epilogue.  Group / chunk / k-step loops are fully unrolled and skipped by uniform
            // branches, so no register is ever indexed dynamically.  The boundary og -> og + 1 holds the skip branches and the chunk's ring
            // addresses, nothing that waits: no drain, no accumulator moves, no LDS round trip between the last MFMA of one group and the
            // first of the next (profiles/group_boundaries.md has the generated sequence before and after, and what it was worth).
            // Its work rides in group og + 1's chunk 0 (every pass has one), tile j of four per step:
            //   * read-out of group og (accumulators -> outv): behind an MFMA of k-step 2 j + 1.  Only the pass's last group is read out
            //     in the layer epilogue.
            //   * seed of group og + 2 (its bias rows; the zero vector where the pass has no bias): read from LDS straight into the set
            //     group og has just left, with the A operands of k-steps 2, 4, 6 and 12, whose wait two k-steps on covers it too.  It stays
            //     the C operand of each tile's first MFMA.  A group past pd.nog is seeded as well: the reads stay inside the 512-entry
            //     vector and the values are dropped.  Group 1 is seeded from group 0's chunk 0, group 0 ahead of the pass.
            // pin_vgpr: empty asm that makes hipcc move the tile from accumulator to vector registers HERE, inside the k-step the
            // sched_barriers fence; left alone it hoists the read-out to the group's last MFMA, where the matrix pipe has to drain first.
            auto pin_vgpr = [](f32x4& t) __attribute__((always_inline)) { asm volatile("" : "=v"(t) : "0"(t)); };
            const float* const seed_src = (pd.bias_row == -1 ? zero_l : pass_bias_vec(pd.bias_row, bias_l, cb_l)) + 4 * g;
            auto seed_tile = [&](int og, int j) __attribute__((always_inline)) {       // seed of tile j of group og, into the group's set
                acc[og & 1][j] = *reinterpret_cast<const f32x4*>(seed_src + 64 * og + 16 * j);
            };
            auto read_out = [&](int og, int j) __attribute__((always_inline)) {                 // tile j of finished group og: accumulators -> outv
                f32x4 t = acc[og & 1][j];
                pin_vgpr(t);
                outv[4 * og + j] = t;
            };
#pragma unroll
            for (int j = 0; j < 4; ++j) seed_tile(0, j);
#pragma unroll
            for (int og = 0; og < 8; ++og) {
                if (og < pd.nog) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        if (c < pd.nchunks) {
                            const int nx_slot = (rd_slot + 1 == NBUF) ? 0 : rd_slot + 1;
                            const char* cb = ring_ptr + rd_slot * CHUNK_BYTES + lane * 16;
                            const char* nb = ring_ptr + nx_slot * CHUNK_BYTES + lane * 16;
#pragma unroll
                            for (int s = 0; s < KSTEPS_PER_CHUNK; ++s) {
                                if (s == KSTEPS_PER_CHUNK / 2) {
                                    // Chunk q+1 has landed for this wave once <= NBUF-3 younger chunks are in flight; the
                                    // barrier publishes every wave's quarter and proves all reads of chunk q-1 retired
                                    // (every wave is inside chunk q), so its slot can be refilled right away.
                                    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(GLDS_PER_CHUNK * (NBUF - 3)) : "memory");
                                }
                                // A operands in groups of RG k-steps: one wait (lgkmcnt(0): the group read RG k-steps ago) and RG reads
                                // (k-steps s+RG .. s+2RG-1) every RG-th k-step -- 1 + 1/RG non-MFMA instructions per k-step instead of 2
                                constexpr int RG = PAIR_READS;
                                if ((s % RG) == 0) {
                                    __builtin_amdgcn_s_waitcnt(0xC07F);     // lgkmcnt(0), vmcnt / expcnt untouched
                                    __builtin_amdgcn_sched_barrier(0);      // keep it ahead of the k-step's first MFMA
#pragma unroll
                                    for (int q = 0; q < RG; ++q) {
                                        const int sp = s + RG + q;
                                        abuf[sp % (2 * RG)] = (sp < KSTEPS_PER_CHUNK)
                                                           ? *reinterpret_cast<const f32x4*>(cb + sp * 1024)
                                                           : *reinterpret_cast<const f32x4*>(nb + (sp - KSTEPS_PER_CHUNK) * 1024);
                                    }
                                }
                                const f32x4 av = abuf[s % (2 * PAIR_READS)];
                                const float b = sin_[16 * c + s];
                                f32x4 (&ac)[4] = acc[og & 1];
                                ac[0] = MFMA16(av.x, b, ac[0]);
                                // refill of the slot freed by the barrier above: one DMA piece per k-step, behind an MFMA
                                if (s == KSTEPS_PER_CHUNK / 2 + 0) { glds_set_dst(idst); glds_piece_m0<0>(isrc, lane_off, idst); };
                                if (s == KSTEPS_PER_CHUNK / 2 + 1) glds_piece_m0<1>(isrc, lane_off, idst);
                                if (s == KSTEPS_PER_CHUNK / 2 + 2) glds_piece_m0<2>(isrc, lane_off, idst);
                                if (s == KSTEPS_PER_CHUNK / 2 + 3) { glds_piece_m0<3>(isrc, lane_off, idst); issue_next(); }
                                // the boundary work (above): read-out of the group before, then seed of the group after into the same set
                                constexpr int SSTEP[4] = {2, 4, 6, 12};
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    if (og > 0 && c == 0 && s == 2 * j + 1) read_out(og - 1, j);
                                    if (og < 7 && c == 0 && s == SSTEP[j]) seed_tile(og + 1, j);
                                }
                                ac[1] = MFMA16(av.y, b, ac[1]);
                                ac[2] = MFMA16(av.z, b, ac[2]);
                                ac[3] = MFMA16(av.w, b, ac[3]);
                                // pin "read for k-step s+2, then the four MFMAs of k-step s": left alone, hipcc sinks
                                // every ds_read next to its use (one A buffer, lgkmcnt(0) before each MFMA quad)
                                __builtin_amdgcn_sched_barrier(0);
                            }
                            rd_slot = nx_slot;
                        }
                    }
                }
            }

            // ---- layer epilogue: relu (+ mask store) or mask apply, finished rows -> next layer's input slab ------------------------
#pragma unroll
            for (int og = 0; og < 8; ++og) {
                if (og < pd.nog) {
                    if (og == pd.nog - 1) {       // the last group has no successor to hide its read-out behind
#pragma unroll
                        for (int j = 0; j < 4; ++j) read_out(og, j);
                    }
                    float v[16];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[4 * j + 0] = outv[4 * og + j].x; v[4 * j + 1] = outv[4 * og + j].y;
                        v[4 * j + 2] = outv[4 * og + j].z; v[4 * j + 3] = outv[4 * og + j].w;
                    }
                    if (pd.relu) {
                        if (MASKS) {
                            unsigned bits = 0;
#pragma unroll
                            for (int k = 15; k >= 0; --k) push_mask_bit(bits, v[k]);
                            mask_l[(pd.mask_slot * 8 + og) * 256 + tid] = (unsigned short)bits;
                        }
#pragma unroll
                        for (int k = 0; k < 16; ++k) v[k] = relu1(v[k]);
                    } else if (BWD && pd.mask_slot >= 0) {
                        if (pd.kind == 4) capture_skip_rows(a.lat_tile, og, v, skipx, skipc);
                        const unsigned bits = mask_l[(pd.mask_slot * 8 + og) * 256 + tid];
#pragma unroll
                        for (int k = 0; k < 16; ++k) v[k] = ((bits >> k) & 1u) ? v[k] : 0.f;
                    }
#pragma unroll
                    for (int k = 0; k < 16; ++k) sin_[16 * og + k] = v[k];
                }
            }

            if (DOFWD && ps == a.n_fwd - 1) {
                y = final_layer_sdf(a, bias_l, g, sin_);
                if (!BWD) {
                    if (a.guard) prepass_guard_tol(a, td.z, valid && g == 0, old_lp, y, guard_tol);
                    if (valid && g == 0) a.out_sdf[a.index ? src : pidx + td.w] = y;
                    if (MODE == 1 && valid && y > -a.th && y < a.th) {
                        // a candidate row of the render term (loss.py:88): export this lane's 64 mask words (8 layers x 8
                        // output groups) so that the jacobian launch can run the backward sweep without a second forward
                        export_masks<8>(mask_words(a, src, g), mask_l, tid);
                    }
                } else {
                    seed_backward(pd.mask_slot);
                }
            }
        }

        if (BWD) {
            // sin_[0..15] now holds d y / d code through the first layer (rows 16t + 4g + r); gfirst the xyz part
            write_jgrad_row(a.out_grad + (size_t)(pidx + td.w) * GRAD_STRIDE, valid, g, pl, sin_, skipc, skipx[0], skipx[1], skipx[2], gfirst, y);
            if (MODE == 2 && a.sdf_scatter && tile >= *a.scatter_tile_begin) scatter_sdf(a, td.z, valid && g == 3, pt, y);
        }
        // stores and LDS-DMA share vmcnt and may retire out of order: drain before counting again
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (a.clk && blockIdx.x == 0 && tid == 0) { a.clk[2] = clock64(); a.clk[3] = wall_clock64(); }
}

static void (*const MLP_KERNELS[4])(const MlpArgs) = {mlp_kernel<0>, mlp_kernel<1>, mlp_kernel<2>, mlp_kernel<3>};     // [MODE]

size_t mlp_lds_bytes(int mode) { return LDS_HEAD_BYTES + (mode != 0 ? MASK_BYTES : 0) + NBUF * CHUNK_BYTES + ZERO_VEC_BYTES; }

// Opt every kernel variant into > 64 KiB of dynamic LDS on the current device (called by dsp_create).
hipError_t mlp_prepare_device() {
    for (int i = 0; i < 4; ++i) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(MLP_KERNELS[i]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mlp_lds_bytes(i));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_mlp(int mode, const MlpArgs& args, int n_blocks, hipStream_t stream) {
    hipLaunchKernelGGL(MLP_KERNELS[mode], dim3(n_blocks), dim3(256), mlp_lds_bytes(mode), stream, args);
    return hipGetLastError();
}

}  // namespace dsp
