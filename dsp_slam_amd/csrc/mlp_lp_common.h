// Shared by mlp_lp_kernel.hip (the f16 / bf16 prepass: forward only) and mlp_lpj_kernel.hip (the 16-bit forward + input-gradient kernels of the
// low-precision compute mode): operand types, the v_mfma_f32_16x16x32 wrapper, packing, the weight-ring state, and everything the three kernels
// do alike -- the kernel set-up (lp_setup), a tile's front (lp_tile_front), the layer pass (lp_pass) and the final sum + tanh (lp_finish).  The
// kernels differ in their epilogue policies and in what they do with a tile's result, and in nothing else.
#pragma once
#include "dsp_internal.h"
#include "mlp_common.h"

namespace dsp {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef __bf16 b2 __attribute__((ext_vector_type(2)));

constexpr int LP_KQ = 4;               // 32-k steps per chunk (a chunk spans 128 slab rows)
constexpr int LP_RT = 4;               // 16-row tiles per 64-row output group
constexpr int LP_FRAG_BYTES = 1024;    // one A fragment: 16 rows x 32 k, 16 B per lane
constexpr int LP_NCH = 4;              // chunks per output group of a hidden layer: 16 steps of 32 k = 512 slab rows
constexpr int LP_NOG = 8;              // 64-row output groups per layer
constexpr int LP_ZERO_BYTES = WIDTH * 4;

template <bool BF>
__device__ __forceinline__ f32x4 lp_mfma(u32x4 a, u32x4 b, f32x4 c) {
    if constexpr (BF)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

// two fp32 -> one register holding two 16-bit values (element 0 in the low half), round to nearest even:
// v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32
template <bool BF>
__device__ __forceinline__ unsigned lp_pack(float lo, float hi) {
    const f32x2 v = {lo, hi};
    if constexpr (BF)
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, b2));
    else
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, h2));
}

// relu + round + pack of two accumulators.  f16: round first, then ONE v_pk_max_f16 on the pair -- max(round(x), 0) == round(max(x, 0)),
// rounding keeps the sign (a -0 that survives multiplies to a zero product).  bf16 has no packed max on gfx950: relu in fp32, then pack.
template <bool BF>
__device__ __forceinline__ unsigned lp_relu_pack(float lo, float hi) {
    if constexpr (BF) {
        return lp_pack<BF>(relu1(lo), relu1(hi));
    } else {
        unsigned r;
        asm("v_pk_max_f16 %0, %1, 0" : "=v"(r) : "v"(lp_pack<BF>(lo, hi)));
        return r;
    }
}

template <bool BF>
__device__ __forceinline__ float lp_round(float x) {
    if constexpr (BF)
        return (float)(__bf16)x;
    else
        return (float)(_Float16)x;
}

struct LpRing {            // weight-stream state, all wave-uniform
    int issue_pos, issue_slot, rd_slot, total_chunks;
    const char* wbase;     // this wave's source address inside chunk 0
    unsigned lane_off;     // lane * 16: the per-lane part of every source address
    const char* isrc;      // ... inside the chunk being issued
    unsigned ring0, idst;  // LDS byte addresses: ring start + this wave's quarter; destination of the chunk being issued
    char* ring_ptr;
    unsigned ring_lane;    // LDS byte address of the ring start + lane * 16: base of this lane's A-fragment reads
};

__device__ __forceinline__ void lp_issue_next(LpRing& rg) {
    rg.issue_pos = (rg.issue_pos + 1 == rg.total_chunks) ? 0 : rg.issue_pos + 1;
    rg.issue_slot = (rg.issue_slot + 1 == LP_NBUF) ? 0 : rg.issue_slot + 1;
    rg.isrc = rg.wbase + (size_t)rg.issue_pos * CHUNK_BYTES;
    rg.idst = rg.ring0 + rg.issue_slot * CHUNK_BYTES;
}

// rows 64 g + 16 rt + 4 gq + r of a fp32 table, in accumulator (D) order: dst[rt][r]
__device__ __forceinline__ void lp_load_rows(const float* tab, int g, int gq, f32x4 (&dst)[LP_RT]) {
#pragma unroll
    for (int rt = 0; rt < LP_RT; ++rt) dst[rt] = *reinterpret_cast<const f32x4*>(tab + 64 * g + 16 * rt + 4 * gq);
}

// ---- what every kernel sets up once ---------------------------------------------------------------------------------------------------
constexpr size_t LP_LDS_BYTES = BIAS_BYTES + CODEBIAS_BYTES + LP_ZERO_BYTES + LP_NBUF * CHUNK_BYTES;

struct LpCtx {             // thread coordinates and the LDS carve-up
    int tid, lane, wave;
    int gq;                // which 4-row block of each 16-row tile / which 8 of each step's 32 k slots this lane holds
    int pl;                // this lane's point inside each of the wave's two 16-point column blocks
    float *bias_l, *cb_l;  // the fp32 bias table; this tile's per-object code bias
    float* zero_l;         // a row of zeros: the bias of the backward sweep
    char* ring_ptr;
};

__device__ __forceinline__ LpCtx lp_ctx() {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    return LpCtx{tid, lane, __builtin_amdgcn_readfirstlane(tid >> 6), lane >> 4, lane & 15, reinterpret_cast<float*>(smem),
                 reinterpret_cast<float*>(smem + BIAS_BYTES), reinterpret_cast<float*>(smem + BIAS_BYTES + CODEBIAS_BYTES),
                 smem + BIAS_BYTES + CODEBIAS_BYTES + LP_ZERO_BYTES};
}

__device__ __forceinline__ void lp_stamp(unsigned long long* clk, int at, int tid) {
    if (clk && blockIdx.x == 0 && tid == 0) { clk[at] = clock64(); clk[at + 1] = wall_clock64(); }
}

// Start stamp, bias table and zero row into the LDS (`fill(i)`, i < WIDTH: what else a kernel keeps there), the weight ring primed with its first
// LP_NBUF - 1 chunks, the first A fragments, slabs and accumulators cleared.  Args: LpArgs / LpjArgs.
template <class Args, class Fill>
__device__ __forceinline__ void lp_setup(const Args& a, const LpCtx& w, LpRing& rg, u32x4 (&abuf)[2][LP_RT], u32x4 (&X)[32], u32x4 (&Y)[32],
                                         f32x4 (&acc)[2][LP_RT][2], Fill fill) {
    constexpr int NT = 256, WAVE_BYTES = CHUNK_BYTES / 4;       // four waves, one per SIMD
    lp_stamp(a.clk, 0, w.tid);
    for (int i = w.tid; i < a.n_bias_rows * WIDTH; i += NT) w.bias_l[i] = a.bias_tab[i];
    for (int i = w.tid; i < WIDTH; i += NT) { w.zero_l[i] = 0.f; fill(i); }
    __syncthreads();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    rg.issue_pos = 0; rg.issue_slot = 0; rg.rd_slot = 0; rg.total_chunks = a.total_chunks;
    rg.wbase = reinterpret_cast<const char*>(a.wstream) + w.wave * WAVE_BYTES;   // wave-uniform; the lane part is rg.lane_off
    rg.lane_off = w.lane * 16;
    rg.isrc = rg.wbase;
    rg.ring0 = lds_addr(w.ring_ptr) + w.wave * WAVE_BYTES;
    rg.idst = rg.ring0;
    rg.ring_ptr = w.ring_ptr;
    rg.ring_lane = lds_addr(w.ring_ptr) + w.lane * 16;
#pragma unroll
    for (int i = 0; i < LP_NBUF - 1; ++i) {
        glds_quarter(rg.isrc, rg.lane_off, rg.idst);
        lp_issue_next(rg);
    }
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(GLDS_PER_CHUNK * (LP_NBUF - 2)) : "memory");
    const u32x4 zero = (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
    for (int rt = 0; rt < LP_RT; ++rt) {       // A fragments of the current step and of the next one
        abuf[0][rt] = *reinterpret_cast<const u32x4*>(w.ring_ptr + w.lane * 16 + rt * LP_FRAG_BYTES);
        abuf[1][rt] = zero;
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) { X[i] = zero; Y[i] = zero; }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int rt = 0; rt < LP_RT; ++rt) acc[i][rt][0] = acc[i][rt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// ---- a tile's front ---------------------------------------------------------------------------------------------------------------------
// This lane's two rows of tile td = {first point, n points, object, output offset}, one per 16-point column block of the wave (NBLK = 1: block 0 only)
template <int NBLK>
__device__ __forceinline__ void lp_tile_rows(const int4 td, const LpCtx& w, bool (&valid)[2], int (&pidx)[2]) {
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        const int local = w.wave * 16 * NBLK + 16 * blk + w.pl;
        valid[blk] = blk < NBLK && local < td.y;
        pidx[blk] = td.x + (valid[blk] ? local : 0);
    }
}

// Split-precision xyz operand of one column block (LP_XYZ_TERMS): k slot 16 u + 3 t + c of the xyz step carries part xpart(u, t) of coordinate c
// (u = which of the table's two 16-slot halves); this lane holds slots 8 gq .. 8 gq + 7
template <bool BF>
__device__ __forceinline__ u32x4 lp_xyz_operand(float4 pt, int gq) {
    float xp[4][3];
    const float xyz[3] = {pt.x, pt.y, pt.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        xp[0][c] = 0.f;
        xp[1][c] = lp_round<BF>(xyz[c]);
        xp[2][c] = lp_round<BF>(xyz[c] - xp[1][c]);
        xp[3][c] = lp_round<BF>(xyz[c] - xp[1][c] - xp[2][c]);
    }
    float kv[32];
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
        const int u = kk >> 4, k16 = kk & 15, t = k16 / 3;
        const int ent = (t < 5) ? LP_XYZ_TERMS[BF ? 1 : 0][u][t] : 0;
        kv[kk] = ent ? xp[ent >> 2][k16 % 3] : 0.f;
    }
    u32x4 xb;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned v0 = lp_pack<BF>(kv[2 * q], kv[2 * q + 1]), v1 = lp_pack<BF>(kv[8 + 2 * q], kv[8 + 2 * q + 1]);
        const unsigned v2 = lp_pack<BF>(kv[16 + 2 * q], kv[16 + 2 * q + 1]), v3 = lp_pack<BF>(kv[24 + 2 * q], kv[24 + 2 * q + 1]);
        xb[q] = gq == 0 ? v0 : (gq == 1 ? v1 : (gq == 2 ? v2 : v3));
    }
    return xb;
}

// A forward tile's front: the lane's rows, their points (`index`: optional indirection, src = the point's place in `pts`; a row that is not valid
// decodes the origin) as xyz operands, and the tile's per-object code bias into the LDS
template <bool BF, int NBLK, class Args>
__device__ __forceinline__ void lp_tile_front(const Args& a, const int* index, const int4 td, const LpCtx& w, bool (&valid)[2], int (&pidx)[2], int (&src)[2],
                                              u32x4 (&xb)[2]) {
    lp_tile_rows<NBLK>(td, w, valid, pidx);
    float4 pt[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        src[blk] = index ? index[pidx[blk]] : pidx[blk];
        pt[blk] = a.pts[src[blk]];
        if (!valid[blk]) pt[blk] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    reinterpret_cast<float4*>(w.cb_l)[w.tid] = reinterpret_cast<const float4*>(a.code_bias + (size_t)td.z * a.code_bias_stride)[w.tid];
    __syncthreads();
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) xb[blk] = lp_xyz_operand<BF>(pt[blk], w.gq);
}

// the C operand of a pass's first MFMAs: a row of the bias table or one of the two per-object code-bias rows
__device__ __forceinline__ const float* lp_bias_of(const LpCtx& w, const LpPass& pd) {
    return pd.bias_row == -2 ? w.cb_l + WIDTH : (pd.bias_row == -3 ? w.cb_l : w.bias_l + pd.bias_row * WIDTH);
}

// The final layer's sum + tanh.  A point's 512 rows are spread over the four lane groups: lanes p, p + 16, p + 32, p + 48; lane group 0 returns
// (and stores) the point of column block 0, lane group 1 that of column block 1.  (The two sums by value: given the array they live in by
// reference, hipcc keeps that array in scratch memory through the whole last pass.)
__device__ __forceinline__ float lp_finish(float part0, float part1, int gq, float b_last) {
    part0 += __shfl_xor(part0, 16);
    part0 += __shfl_xor(part0, 32);
    part1 += __shfl_xor(part1, 16);
    part1 += __shfl_xor(part1, 32);
    return tanhf(((gq & 1) ? part1 : part0) + b_last);
}

// ---- the layer pass ---------------------------------------------------------------------------------------------------------------------
// One dense layer for this wave's points: NOG output groups of 64 rows x NCH chunks of straight-line code, the ONE schedule of all three kernels
// (which is why the forward jacobian kernel's sdf is the prepass kernel's, bit for bit: both instantiate this body over the same stream).
// `in` / `out` are the two register slabs, indexed [2 ks + blk]: 32-k step ks, column block blk.  Everything that differs between layers is data
// (bias pointer, prologue selects) -- hipcc answers run-time control flow inside this body with hundreds of register moves at every join.
// NCH = 1 for the first layer (its K is the xyz step only), LP_NCH for the others.  NBLK = 2: the wave's 32 points as two column blocks (128-point
// tiles, the throughput form); NBLK = 1: ONE column block of 16 points (64-point tiles: a detection-sized list -- ~117 tiles of 128 points on
// 256 CUs -- becomes ~235 tiles of half the length; the same arithmetic per point, so the same values).
// What becomes of a finished output group is the epilogue policy's business: a small struct built at the call site around the caller's registers
// and passed BY VALUE (through a reference hipcc extracts the backward kernel's mask bits another way: 1984 v_bfe_i32 for 1152, 1288 s_cselect_b32 for 872):
//   Epi::XYZ_PROLOGUE   forward passes: xyz enters at its fixed step
//   Epi::KEEP_ACC       no epilogue at all: the accumulators are the result (the backward sweep's first layer)
//   epi.begin()         once, ahead of the first MFMA
//   epi.half(T, blk, h, e0, e1, out)   two accumulators (rows 4 gq + 2 h + {0, 1}) of 16-row tile T = 4 g + rt and column block blk.  T, blk, h
//                       are compile-time constants after unrolling, so every register index folds.  Tile T is half (T & 1) of the next layer's
//                       32-k step T >> 1: a slab-writing policy fills register 2 (T & 1) + h of out[2 (T >> 1) + blk].
//                       Half 0 of a unit is always called before half 1 of the same unit, with no other unit between (LpEpiDot rests on it).
template <bool BF, int NCH, int NBLK, int NOG, class Epi>
__device__ __forceinline__ void lp_pass(const LpPass pd, u32x4 (&in)[32], u32x4 (&out)[32], f32x4 (&acc)[2][LP_RT][2], u32x4 (&abuf)[2][LP_RT], LpRing& rg,
                                        const u32x4 (&xb)[2], const float* bp, int gq, Epi epi) {
    // ---- prologue: place the xyz B operands at their fixed step -------------------------------------------------------
    // first layer: step 0 (the rest of its single chunk is padding); latent_in layer: the last step (15), behind the slab rows and
    // pd.npad padding 16-row tiles.  Padding meets zero A fragments: clear it so that no stale inf / nan of an earlier layer does.
    // (Selects, not branches: hipcc sinks the stores of two branches into one store through a pointer phi, which pins the whole slab
    // in scratch memory.)
    if constexpr (Epi::XYZ_PROLOGUE) {
        const u32x4 zero = (u32x4){0u, 0u, 0u, 0u};
        if (NCH == 1) {
#pragma unroll
            for (int ks = 0; ks < LP_KQ; ++ks)
#pragma unroll
                for (int blk = 0; blk < NBLK; ++blk) in[2 * ks + blk] = ks == 0 ? xb[blk] : zero;
        } else {
            const bool lat = pd.kind == 2;
            constexpr int KX = LP_KQ * NCH - 1;          // the xyz step of the latent_in layer
#pragma unroll
            for (int blk = 0; blk < NBLK; ++blk) in[2 * KX + blk] = lat ? xb[blk] : in[2 * KX + blk];
#pragma unroll
            for (int t = 1; t <= 3; ++t) {               // padding 16-row tile 2 KX - t = half (t & 1 ? 1 : 0) of step (2 KX - t) >> 1
                const int T = 2 * KX - t;
                const bool z = lat && pd.npad >= t;
#pragma unroll
                for (int blk = 0; blk < NBLK; ++blk) {
                    in[2 * (T >> 1) + blk][2 * (T & 1) + 0] = z ? 0u : in[2 * (T >> 1) + blk][2 * (T & 1) + 0];
                    in[2 * (T >> 1) + blk][2 * (T & 1) + 1] = z ? 0u : in[2 * (T >> 1) + blk][2 * (T & 1) + 1];
                }
            }
        }
    }
    epi.begin();
    f32x4 bias[LP_RT];
    lp_load_rows(bp, 0, gq, bias);

#pragma unroll
    for (int g = 0; g < NOG; ++g) {
        const int par = g & 1;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int nx_slot = (rg.rd_slot + 1 == LP_NBUF) ? 0 : rg.rd_slot + 1;
            // This lane's LDS byte address inside the chunk being read and inside the next one, each as ONE opaque 32-bit register: every
            // A-fragment read below is then `ds_read_b128 v, base offset:imm`.  Left to itself hipcc materialises a separate address for
            // every (slot, step, row tile), parks them in AGPRs and pays a v_accvgpr_read (often two) per ds_read.
            typedef const __attribute__((address_space(3))) char* lds_cptr;
            unsigned cb_a = rg.ring_lane + (unsigned)rg.rd_slot * CHUNK_BYTES, nb_a = rg.ring_lane + (unsigned)nx_slot * CHUNK_BYTES;
            asm volatile("" : "+v"(cb_a), "+v"(nb_a));
            const lds_cptr cbp = (lds_cptr)(size_t)cb_a, nbp = (lds_cptr)(size_t)nb_a;
#pragma unroll
            for (int kq = 0; kq < LP_KQ; ++kq) {
                const int ks = LP_KQ * c + kq;
                if (kq == LP_KQ / 2) {
                    // chunk q+1 has landed for this wave once <= LP_NBUF-3 younger chunks are in flight; the barrier
                    // publishes every wave's quarter and proves all reads of chunk q-1 retired (mlp_kernel.hip)
                    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(GLDS_PER_CHUNK * (LP_NBUF - 3)) : "memory");
                }
                // One step = eight MFMAs of 16 cycles (row tile m >> 1, column block m & 1).  A 16-cycle MFMA leaves this one wave THREE issue
                // slots, so everything else is dealt out over the eight gaps and pinned there (sched_barrier after every MFMA):
                //   gap 0: ONE lgkmcnt(0) -- the four A fragments of this step were read in gaps 0, 1 of the previous step, seven MFMAs ago --
                //          then the reads of fragments 0, 1 of the NEXT step;   gap 1: fragments 2, 3;
                //   gaps 1, 2 of steps 2, 3: the chunk's four LDS-DMA pieces;
                //   gaps 4 .. 7: one (row tile, column block) unit of the PREVIOUS output group's epilogue, its two halves two gaps each (fetch the
                //          accumulator pair, then epi.half; steps 1 .. 8 carry the eight units).  hipcc left alone sinks the reads behind the sixth
                //          MFMA and bunches the epilogue behind one step: measured 0.65 duty against 0.74 for the 32x32x16 form.
                constexpr int NM = NBLK * LP_RT;                          // MFMAs per step
                const bool epi_on = !Epi::KEEP_ACC && NCH > 1 && g > 0 && ks >= 1 && ks <= 4 * NBLK;
                const int ert = NBLK == 2 ? (ks - 1) >> 1 : ks - 1, eblk = NBLK == 2 ? (ks - 1) & 1 : 0;       // this step's epilogue unit
                constexpr int E0 = NM - 4;                                // the unit's four micro-steps sit in the step's last four gaps
                float e0 = 0.f, e1 = 0.f;
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    const int rt = NBLK == 2 ? m >> 1 : m, blk = NBLK == 2 ? m & 1 : 0;
                    if (m == 0) __builtin_amdgcn_s_waitcnt(0xC07F);     // lgkmcnt(0), vmcnt / expcnt untouched
                    if (m < 2) {
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const int f = 2 * m + q;        // fragment (= row tile) of step kq + 1
                            const lds_cptr src = (kq + 1 < LP_KQ) ? cbp + ((kq + 1) * LP_RT + f) * LP_FRAG_BYTES : nbp + f * LP_FRAG_BYTES;
                            abuf[(kq + 1) & 1][f] = *reinterpret_cast<const __attribute__((address_space(3))) u32x4*>(src);
                        }
                    }
                    acc[par][rt][blk] = lp_mfma<BF>(abuf[kq & 1][rt], in[2 * ks + blk], ks == 0 ? bias[rt] : acc[par][rt][blk]);
                    // refill of the slot freed by the barrier above: this wave's quarter of the chunk, four 1 KiB DMA pieces
                    if (kq == LP_KQ / 2 && m == 1) { glds_set_dst(rg.idst); glds_piece_m0<0>(rg.isrc, rg.lane_off, rg.idst); }
                    if (kq == LP_KQ / 2 && m == 2) glds_piece_m0<1>(rg.isrc, rg.lane_off, rg.idst);
                    if (kq == LP_KQ / 2 + 1 && m == 1) glds_piece_m0<2>(rg.isrc, rg.lane_off, rg.idst);
                    if (kq == LP_KQ / 2 + 1 && m == 2) { glds_piece_m0<3>(rg.isrc, rg.lane_off, rg.idst); lp_issue_next(rg); }
                    if (NCH == 1) {          // first layer (four steps in all): one row tile's units behind the last MFMA of that row tile in step 1
                        if (!Epi::KEEP_ACC && g > 0 && ks == 1 && blk == NBLK - 1) {
#pragma unroll
                            for (int b2 = 0; b2 < NBLK; ++b2) {
                                const f32x4 v = acc[par ^ 1][rt][b2];
                                epi.half(4 * (g - 1) + rt, b2, 0, v.x, v.y, out);
                                epi.half(4 * (g - 1) + rt, b2, 1, v.z, v.w, out);
                            }
                        }
                    } else if (epi_on) {
                        const int T = 4 * (g - 1) + ert;
                        if (m == E0 + 0) { e0 = acc[par ^ 1][ert][eblk].x; e1 = acc[par ^ 1][ert][eblk].y; asm volatile("" : "+v"(e0), "+v"(e1)); }
                        if (m == E0 + 1) epi.half(T, eblk, 0, e0, e1, out);
                        if (m == E0 + 2) { e0 = acc[par ^ 1][ert][eblk].z; e1 = acc[par ^ 1][ert][eblk].w; asm volatile("" : "+v"(e0), "+v"(e1)); }
                        if (m == E0 + 3) epi.half(T, eblk, 1, e0, e1, out);
                    }
                    // the next group's bias: behind the second MFMA of the group's last step, six MFMAs ahead of the lgkmcnt(0) that follows
                    if (ks == LP_KQ * NCH - 1 && m == 1 && g + 1 < NOG) lp_load_rows(bp, g + 1, gq, bias);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            rg.rd_slot = nx_slot;
        }
    }
    if constexpr (!Epi::KEEP_ACC) {        // the last group's epilogue has no MFMAs of its own pass to hide behind
#pragma unroll
        for (int rt = 0; rt < LP_RT; ++rt)
#pragma unroll
            for (int blk = 0; blk < NBLK; ++blk) {
                const f32x4 v = acc[(NOG - 1) & 1][rt][blk];
                epi.half(4 * (NOG - 1) + rt, blk, 0, v.x, v.y, out);
                epi.half(4 * (NOG - 1) + rt, blk, 1, v.z, v.w, out);
            }
    }
}

// The two forward epilogues.  Mask: what else sees every accumulator pair -- nothing in the prepass kernel (LpNoMask), the relu-mask export of the
// forward jacobian kernel (mlp_lpj_kernel.hip: LpjMaskOut); the arithmetic is this one copy either way.
struct LpNoMask {
    __device__ __forceinline__ void clear() {}
    __device__ __forceinline__ void push(int, int, float, float) {}
};
// Hidden layers: relu + round + pack into the next layer's input slab.
template <bool BF, class Mask>
struct LpEpiRelu {
    static constexpr bool XYZ_PROLOGUE = true, KEEP_ACC = false;
    Mask mask;
    __device__ __forceinline__ void begin() { mask.clear(); }
    __device__ __forceinline__ void half(int T, int blk, int h, float e0, float e1, u32x4 (&out)[32]) {
        mask.push(T, blk, e0, e1);
        out[2 * (T >> 1) + blk][2 * (T & 1) + h] = lp_relu_pack<BF>(e0, e1);
    }
};
// Last hidden layer: nothing reads its slab; only the final 512 -> 1 layer's dot product with the rows of `dp`, on the un-rounded values (fmaf
// order per part[blk]: x, y, z, w of a unit, units in the order of the schedule).  Half 0 reads the unit's four weights in one piece and
// leaves two to half 1 (lp_pass: half 1 of a unit follows its half 0 directly): one LDS read and one lgkmcnt wait a unit, not two.  The
// read stands AHEAD of the mask's instructions, which then cover part of its latency.
template <class Mask>
struct LpEpiDot {
    static constexpr bool XYZ_PROLOGUE = true, KEEP_ACC = false;
    const float* dp; int gq; float (&part)[2]; Mask mask; f32x4 w;
    __device__ __forceinline__ void begin() { mask.clear(); }
    __device__ __forceinline__ void half(int T, int blk, int h, float e0, float e1, u32x4 (&)[32]) {
        if (h == 0) w = *reinterpret_cast<const f32x4*>(dp + 16 * T + 4 * gq);
        mask.push(T, blk, e0, e1);
        part[blk] = fmaf(relu1(e0), h ? w.z : w.x, part[blk]);
        part[blk] = fmaf(relu1(e1), h ? w.w : w.y, part[blk]);
    }
};

}  // namespace dsp
