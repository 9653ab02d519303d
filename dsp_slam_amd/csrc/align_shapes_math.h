// Shape refinement (dsp_map_align_shapes, include/dsp_gn.h): the sensor is known, the map's objects change their SHAPE CODES, and with them,
// if asked, their poses.  One 70-dimensional Gauss-Newton system per map object against depth rays given in the world frame.  The
// arithmetic that is not align_objects_math.h's, written once for the device and for the host.  The kernels of align_shapes_kernels.hip
// call build_row / term_of from their lanes; dsp_debug_align_shapes_rows / _step run the same functions on the CPU, so the arithmetic is
// tested without a GPU (tests/align_shapes_ref.py restates THIS COMMENT in numpy) and the device is held to it bit for bit.
//
// The translation unit that includes this header must be compiled with floating-point contraction off (align_shapes_kernels.hip is): every
// fp32 and fp64 operation below is one correctly rounded operation.
//
// Unknowns.  DIM = 70 per object: x = [v(3), omega(3), dz(CODE = 64)].  The pose part is dsp_map_align_objects' left perturbation
//            C_k <- exp([v, omega]) C_k of the fp64 correction C_k; the code part is additive, z_k <- z_k + dz, on an fp64 code z_k that starts
//            as the fp32 input code converted exactly.
// State.     (C_k, z_k) per object.  At an evaluation object k stands at the pose compose(C_k, T_k0) (align_objects_math.h) with the code
//            z_k rounded ONCE to fp32; its code bias (the decoder's first-layer term of the code) is recomputed from that fp32 code.
// Residual.  Observation, cast, gradient, gap, d = fmaf(g_w . u, gap, dist_hit), the max_gap match and the owner rule are
//            align_objects_math.h's verbatim: ray i belongs to the object the cast names as its winner, matched or not.
// gcode.     The winner's jacobian row at the hit sample holds d sdf / d code[0 .. 63] (fp32).  gcode_c = that entry times the winner's
//            scale s: ONE fp32 multiply, as align_math::world_gradient scales g_w.  (d = sdf s, so this is d d / d code_c at a fixed hit
//            sample.)  The dependence of t_hit and g_w on the code is dropped: the first-order treatment the pose part already has.
// Row (fp64 from the fp32 p_w, d, g_w, gcode, w converted once).
//     valid = p_w finite and w > 0 and finite;   used = valid, obj_row >= 0, d finite, g_w finite, all 64 gcode finite, |d| <= max_dist
//     J = [ -g_w, -(p_w x g_w), gcode ]   (70 entries.  -g_w: the fp32 negation; the cross product c of align_math.h in fp64, then negated.
//         The object moves and the measured point stays: align_objects_math.h "sign".  A larger code value at a positive gcode raises the
//         signed distance d of the fixed point.)
//     wh = 1 for |d| <= huber, else huber / |d|;   ww = w wh
//     term[IDX_H + k] = (ww J_i) J_j for the k-th pair i <= j, row-major (0,0 0,1 .. 0,69 1,1 ..): 2485 entries
//     term[IDX_B + i] = -((ww J_i) d)        (the device multiplies (ww J_i) by the stored -d: the same bits)
//     term[IDX_COST] = w rho(d) for a used row, w rho(max_dist) for a valid row that is not used;  term[IDX_W] = w for a valid row;
//     term[IDX_N] = 1 for a used row.  A row that is not used has ww = 0, d = 0 and J = 0: its H and b terms are zeros.
// Summation.  The NSUM = 2558 sums of object k run over its winners in ascending ray order (the LIST of align_objects_math.h).  The order is
//     fixed by BLOCK below and by nothing else (not by passes, chunks, the grid or the number of threads): a block is BLOCK consecutive list
//     positions; a block's sum starts at +0 and adds the terms of its rows in ascending list order, one add at a time; the object's sum is
//     its first block's sum, then + the next block's, ascending; all zero for an empty list.  This is NOT align_math.h's butterfly: with 2558
//     sums one thread owns a few sums and walks the rows.  No float atomics, no matrix instructions.  block_sums below is that order on the host.
// Cost.      F = sum[IDX_COST] / W + code_reg |z|^2 + code_anchor |z - z0|^2, W = sum[IDX_W]; the first term is rho(max_dist) when W == 0.
//            |z|^2 = the squares of entries 0 .. code_len - 1 added in ascending order from +0, likewise |z - z0|^2 (z0: the input code,
//            converted to fp64), and F = (mean + code_reg |z|^2) + code_anchor |z - z0|^2.  z is the EVALUATED fp64 code, not its fp32 rounding.
// Step (host only).  The MEAN system: A_ij = H_ij / W, g_i = b_i / W (one division each; W > 0 and finite, otherwise SINGULAR).  Then, for
//     the code entries c (index 6 + c), kc = code_reg + code_anchor (formed first):  A_cc = A_cc + kc;
//     g_c = g_c - (code_reg z_c + code_anchor (z_c - z0_c)).  Then A_ii = A_ii + (damp + lambda) on all 70 (the sum formed first).  Then the
//     pins, last: entry i is pinned when it is a pose entry and unknowns lacks POSE, a code entry and unknowns lacks CODE, or a code entry
//     c >= code_len; a pinned entry's row and column are zeroed, A_ii = 1, g_i = 0.  Then align_math.h's Cholesky with forward and backward
//     substitution, in its written order, on 70 dimensions: + - * / sqrt only.  A pinned entry's dx is exactly 0.
//     Pose: C_trial = align_math::apply_step(dx[0 .. 5], C) when POSE is asked for, otherwise C's own bytes.
//     Code: z_trial_c = z_c + dx[6 + c] in fp64 for an entry that is not pinned; a pinned entry keeps z_c's own bytes.
// Loop.      align_objects_math.h's, the state being (C_k, z_k): statuses, min_points, the opt-in step rule (step_rule.h) on F, the best
//            evaluated state is returned.  An object converges when max |v| < trans_tol, max |omega| < rot_tol and max |dz| < code_tol
//            (strict: a tolerance of 0 stops nothing).  A trial code whose fp32 rounding or whose code bias is not finite, or a trial pose
//            the map's inversion refuses, ends the object with SINGULAR at its accepted state.
// LIMIT.     align_objects_math.h's: the winner set changes between evaluations.  Most code directions are not observed by a few views:
//            damp (on the mean system) and the opt-in code_reg / code_anchor are what keeps the 64 code entries conditioned.
//
// Out of scope: scale (Sim(3)); coupling between objects beyond occlusion; a prior from dsp_batch_posterior records; the 16-bit decoders.
#pragma once
#include "align_objects_math.h"

namespace align_shapes_math {

constexpr int BLOCK = 128;                                // the summation order
constexpr int CODE = 64, DIM = 6 + CODE;
constexpr int NPAIR = DIM * (DIM + 1) / 2;                // 2485
constexpr int IDX_H = 0, IDX_B = NPAIR, IDX_COST = NPAIR + DIM, IDX_W = IDX_COST + 1, IDX_N = IDX_COST + 2, NSUM = IDX_COST + 3;
constexpr int UNKNOWN_CODE = 1, UNKNOWN_POSE = 2;         // == DSP_SHAPES_* (include/dsp_gn.h)
// a built row: ROW_F floats {-g_w[3], gcode[64]} and ROW_D doubles {-(p_w x g_w)[3], -d, ww, cost, w, n}
constexpr int ROW_F = 3 + CODE, ROW_D = 8;
constexpr int COL_ND = DIM;                               // "column 70" of a row is -d: b_i = (ww J_i) J_70
constexpr int EXTRA = DIM + 1;                            // i == EXTRA: the sums without a J (j = 0 cost, 1 w, 2 n)
static_assert(NSUM == 2558 && NPAIR == 2485, "the sums of one object");

// sum index q -> (i, j): a pair i <= j of H, (i, COL_ND) for b_i, (EXTRA, 0 .. 2) for cost, w, n
DSP_QM_HD inline void pair_of(int q, int* i, int* j) {
    if (q >= IDX_COST) { *i = EXTRA; *j = q - IDX_COST; return; }
    if (q >= IDX_B) { *i = q - IDX_B; *j = COL_ND; return; }
    int r = 0, rem = q;
    while (rem >= DIM - r) { rem -= DIM - r; ++r; }
    *i = r;
    *j = r + rem;
}

// One row.  jf[3 .. 66] holds gcode on entry.  g is read only where obj_row >= 0.  -> jf, jd as described at ROW_F / ROW_D
DSP_QM_HD inline void build_row(const float* pw, int32_t obj_row, float dist, const float* g, float w32, double huber, double max_dist, float* jf,
                                double* jd) {
    for (int k = 0; k < ROW_D; ++k) jd[k] = 0.0;
    jf[0] = jf[1] = jf[2] = 0.f;
    const bool valid = align_math::finite32(pw[0]) && align_math::finite32(pw[1]) && align_math::finite32(pw[2]) && w32 > 0.f && align_math::finite32(w32);
    bool used = valid && obj_row >= 0 && align_math::finite32(dist);
    if (used) used = align_math::finite32(g[0]) && align_math::finite32(g[1]) && align_math::finite32(g[2]) && fabs((double)dist) <= max_dist;
    if (used)
        for (int c = 0; c < CODE; ++c) used = used && align_math::finite32(jf[3 + c]);
    if (!used)
        for (int c = 0; c < CODE; ++c) jf[3 + c] = 0.f;
    if (!valid) return;
    const double w = (double)w32;
    jd[6] = w;
    if (!used) {
        jd[5] = w * align_math::rho(max_dist, huber);
        return;
    }
    const double d = (double)dist, a = fabs(d);
    const double p0 = (double)pw[0], p1 = (double)pw[1], p2 = (double)pw[2];
    const double g0 = (double)g[0], g1 = (double)g[1], g2 = (double)g[2];
    jf[0] = -g[0]; jf[1] = -g[1]; jf[2] = -g[2];
    jd[0] = -(p1 * g2 - p2 * g1);
    jd[1] = -(p2 * g0 - p0 * g2);
    jd[2] = -(p0 * g1 - p1 * g0);
    jd[3] = -d;
    const double wh = a <= huber ? 1.0 : huber / a;
    jd[4] = w * wh;
    jd[5] = w * align_math::rho(d, huber);
    jd[7] = 1.0;
}

// entry idx of a built row: J_0 .. J_69, and -d at COL_ND
DSP_QM_HD inline double j_at(const float* jf, const double* jd, int idx) {
    return idx < 3 ? (double)jf[idx] : idx < 6 ? jd[idx - 3] : idx < DIM ? (double)jf[idx - 3] : jd[3];
}

// the term of sum (i, j) of a built row
DSP_QM_HD inline double term_of(const float* jf, const double* jd, int i, int j) {
    if (i == EXTRA) return jd[5 + j];
    return (jd[4] * j_at(jf, jd, i)) * j_at(jf, jd, j);
}

// host: the sums of one object over the n built rows of its list (jf: n x ROW_F, jd: n x ROW_D) -> sums[NSUM]
inline void block_sums(int64_t n, const float* jf, const double* jd, double* sums) {
    for (int q = 0; q < NSUM; ++q) {
        int i, j;
        pair_of(q, &i, &j);
        double total = 0.0;
        for (int64_t b0 = 0; b0 < n; b0 += BLOCK) {
            double blk = 0.0;
            for (int64_t r = b0; r < n && r < b0 + BLOCK; ++r) blk = blk + term_of(jf + r * ROW_F, jd + r * ROW_D, i, j);
            total = b0 == 0 ? blk : total + blk;
        }
        sums[q] = total;
    }
}

// host.  The first term of F from an object's sums
inline double mean_cost(const double* sums, double huber, double max_dist) {
    return sums[IDX_W] == 0.0 ? align_math::rho(max_dist, huber) : sums[IDX_COST] / sums[IDX_W];
}

// host.  F from the mean cost, the evaluated code z and the input code z0 (both CODE doubles)
inline double cost_of(double mean, const double* z, const double* z0, int code_len, double code_reg, double code_anchor) {
    double zz = 0.0, dd = 0.0;
    for (int c = 0; c < code_len; ++c) {
        zz = zz + z[c] * z[c];
        const double e = z[c] - z0[c];
        dd = dd + e * e;
    }
    return (mean + code_reg * zz) + code_anchor * dd;
}

DSP_QM_HD inline bool pinned(int i, int unknowns, int code_len) {
    if (i < 6) return !(unknowns & UNKNOWN_POSE);
    return !(unknowns & UNKNOWN_CODE) || i - 6 >= code_len;
}

// host.  H: DIM x DIM row-major raw sums (the upper triangle is read), b: DIM raw sums, W = sum of the valid weights.  false = SINGULAR
// (dx untouched)
inline bool solve(const double* H, const double* b, double W, const double* z, const double* z0, int code_len, int unknowns, double code_reg,
                  double code_anchor, double damp, double lambda, double* dx) {
    if (!(W > 0.0) || !align_math::finite64(W)) return false;
    static thread_local double A[DIM][DIM], L[DIM][DIM];
    double g[DIM], y[DIM], x[DIM];
    for (int i = 0; i < DIM; ++i) {
        for (int j = i; j < DIM; ++j) A[i][j] = A[j][i] = H[DIM * i + j] / W;
        g[i] = b[i] / W;
    }
    const double kc = code_reg + code_anchor;
    for (int c = 0; c < CODE; ++c) {
        A[6 + c][6 + c] = A[6 + c][6 + c] + kc;
        g[6 + c] = g[6 + c] - (code_reg * z[c] + code_anchor * (z[c] - z0[c]));
    }
    const double dl = damp + lambda;
    for (int i = 0; i < DIM; ++i) A[i][i] = A[i][i] + dl;
    for (int i = 0; i < DIM; ++i) {
        if (!pinned(i, unknowns, code_len)) continue;
        for (int j = 0; j < DIM; ++j) A[i][j] = A[j][i] = 0.0;
        A[i][i] = 1.0;
        g[i] = 0.0;
    }
    for (int i = 0; i < DIM; ++i)
        for (int j = 0; j < DIM; ++j) L[i][j] = 0.0;
    for (int j = 0; j < DIM; ++j) {
        double s = A[j][j];
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(s > 0.0) || !align_math::finite64(s)) return false;
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < DIM; ++i) {
            double q = A[i][j];
            for (int k = 0; k < j; ++k) q = q - L[i][k] * L[j][k];
            L[i][j] = q / L[j][j];
        }
    }
    for (int i = 0; i < DIM; ++i) {
        double s = g[i];
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    for (int i = DIM - 1; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < DIM; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    for (int i = 0; i < DIM; ++i)
        if (!align_math::finite64(x[i])) return false;
    for (int i = 0; i < DIM; ++i) dx[i] = x[i];
    return true;
}

// host.  (c_in, z_in) + dx -> (c_out, z_out): 16 and CODE doubles each; may not alias
inline void apply_step(const double* dx, int unknowns, int code_len, const double* c_in, const double* z_in, double* c_out, double* z_out) {
    if (unknowns & UNKNOWN_POSE) align_math::apply_step(dx, c_in, c_out);
    else memcpy(c_out, c_in, 16 * sizeof(double));
    for (int c = 0; c < CODE; ++c) z_out[c] = pinned(6 + c, unknowns, code_len) ? z_in[c] : z_in[c] + dx[6 + c];
}

}  // namespace align_shapes_math
