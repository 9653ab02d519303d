// Map alignment (dsp_map_align, include/dsp_gn.h): batched SE(3) Gauss-Newton of a sensor-frame point cloud against the map's decoded
// surfaces.  The arithmetic between the sensor points, the map query's answers and the 6 x 6 system, written once for the device and for
// the host.  The kernels of align_kernels.hip call it from their lanes; dsp_debug_align_rows / dsp_debug_align_step run the same functions
// on the CPU, so the arithmetic is tested without a GPU (tests/align_ref.py restates it in numpy) and the device is held to it bit for bit.
//
// The translation unit that includes this header must be compiled with floating-point contraction off (align_kernels.hip is): every fp32
// and fp64 operation below is one correctly rounded operation, fmaf where it says fmaf.
//
// State.  One fp64 sensor-to-world pose T_h per hypothesis, on the host.  check_pose refuses what query_math::invert refuses (an entry that
//   is not finite, a bottom row other than exactly 0 0 0 1, s2 <= 0, an A / s whose R^T R is off the identity by more than RIGID_TOL, an
//   entry that is not finite in fp32), restated in fp64 on the fp64 pose, and a scale s with |s - 1| > RIGID_TOL.
// Transform.  rt = the pose's 3 x 4 [R | t], every entry rounded ONCE to fp32;  p_w = query_math::to_object(rt, p_s)  (the nested fmaf).
// World gradient.  g = the winning row's d sdf / d xyz (object frame), rt / s the winner's table entry:
//     u_j = fmaf(rt[8+j], gz, fmaf(rt[4+j], gy, rt[j] gx))   (the u of query_math::normal);   g_w[j] = u_j s   (one multiply, NOT normalised:
//   DeepSDF's gradient is not unit length, so the unit normal is the wrong jacobian of d = sdf s).
// Row (fp64 from the fp32 p_w, d, g_w, w converted once).
//     valid = p_w finite and w > 0;   used = valid, obj >= 0, d and g_w finite, |d| <= max_dist
//     rho(d) = d d for |d| <= huber, else huber (2 |d| - huber)
//     J = [g_w, p_w x g_w]  (cross: c0 = p1 g2 - p2 g1, c1 = p2 g0 - p0 g2, c2 = p0 g1 - p1 g0): the left perturbation T <- exp(xi) T,
//         xi = [v, omega], the order of exp_se3 elsewhere in the project
//     wh = 1 for |d| <= huber, else huber / |d|;   t_j = (w wh) J_j
//     term[IDX_H + k] = t_i J_j for the k-th pair i <= j, row-major (00 01 .. 05 11 12 ..);   term[IDX_B + j] = -(t_j d)
//     term[IDX_COST] = w rho(d) for a used point, w rho(max_dist) for a valid point that is not used (its other terms are zero), so that
//         costs at different poses are comparable whatever set is used;   term[IDX_W] = w for a valid point;  term[IDX_N] = 1 for a used one
// Summation.  The NSUM sums of one hypothesis over its points i = 0 .. n_pts - 1 are ONE tree, fixed by BLOCK and WAVE below and by nothing
//   else (not by passes, chunks or the grid): a block is BLOCK consecutive points, padded with zero terms; inside a wave of WAVE points the
//   butterfly x[l] <- x[l] + x[l ^ m] for m = WAVE / 2, WAVE / 4 .. 1 (every lane ends with the same bits: + commutes); the block's sum is
//   its waves' sums added in ascending order from the first; the hypothesis' sum is its blocks' sums added in ascending order from the
//   first.  tree_sum below is that tree on the host.  No float atomics anywhere.
// Cost.  F = sum[IDX_COST] / sum[IDX_W];  rho(max_dist) when sum[IDX_W] == 0 (no valid point).
// Step (host only).  A = H, A_ii += (damp + lambda) (the sum formed first);  Cholesky A = L L^T column by column,
//     s = A_jj;  s = s - L_jk L_jk (k = 0 .. j-1);  not (s > 0) or s not finite: SINGULAR;  L_jj = sqrt(s)
//     s = A_ij;  s = s - L_ik L_jk (k = 0 .. j-1);  L_ij = s / L_jj      (i > j)
//   forward y_i = (b_i - L_ik y_k ...) / L_ii  (k ascending), backward x_i = (y_i - L_ki x_k ...) / L_ii (k = i+1 .. 5 ascending).  Only
//   + - * / sqrt, in this order.
// exp_se3 (host only, fp64, closed form).  th2 = (w0 w0 + w1 w1) + w2 w2, th = sqrt(th2);
//     th2 < SMALL_TH2:  A = 1 - th2 / 6,  B = 0.5 - th2 / 24,  C = 1 / 6 - th2 / 120;   else  A = sin th / th,  B = (1 - cos th) / th2,
//     C = (th - sin th) / (th2 th).   W = hat(omega), W2 = W W;   R = I + A W + B W2 (entry: (I_ij + A W_ij) + B W2_ij);   V = I + B W + C W2;
//     t = V v.   T_trial = exp(xi) T: R' = R R_T, t' = R t_T + t, dot products as (a0 b0 + a1 b1) + a2 b2.
#pragma once
#include <math.h>
#include <stdint.h>

#include "query_math.h"

namespace align_math {

constexpr int BLOCK = 256, WAVE = 64;                    // the summation tree
constexpr int IDX_H = 0, IDX_B = 21, IDX_COST = 27, IDX_W = 28, IDX_N = 29, NSUM = 30;
constexpr double SMALL_TH2 = 1e-8;
constexpr int OK = 0, CONVERGED = 1, NO_SUPPORT = 2, SINGULAR = 3;     // == DSP_ALIGN_* (include/dsp_gn.h)
static_assert(BLOCK % WAVE == 0 && (WAVE & (WAVE - 1)) == 0, "a block is whole waves, a wave a power of two");

DSP_QM_HD inline void world_gradient(const float* rt, float s, float gx, float gy, float gz, float* gw) {
    const float ux = fmaf(rt[8], gz, fmaf(rt[4], gy, DSP_QM_MUL(rt[0], gx)));
    const float uy = fmaf(rt[9], gz, fmaf(rt[5], gy, DSP_QM_MUL(rt[1], gx)));
    const float uz = fmaf(rt[10], gz, fmaf(rt[6], gy, DSP_QM_MUL(rt[2], gx)));
    gw[0] = DSP_QM_MUL(ux, s);
    gw[1] = DSP_QM_MUL(uy, s);
    gw[2] = DSP_QM_MUL(uz, s);
}

DSP_QM_HD inline bool finite32(float x) { return fabsf(x) <= 3.402823466e+38f; }
DSP_QM_HD inline bool finite64(double x) { return fabs(x) <= 1.7976931348623157e+308; }
DSP_QM_HD inline double rho(double d, double huber) {
    const double a = fabs(d);
    return a <= huber ? d * d : huber * (2.0 * a - huber);
}

// the NSUM terms of one point.  g is read only where obj >= 0 (a point without a winner has no gradient)
DSP_QM_HD inline void row_terms(const float* pw, int32_t obj, float dist, const float* g, float w32, double huber, double max_dist, double* term) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) term[k] = 0.0;
    const bool valid = finite32(pw[0]) && finite32(pw[1]) && finite32(pw[2]) && w32 > 0.f && finite32(w32);
    if (!valid) return;
    const double w = (double)w32;
    term[IDX_W] = w;
    bool used = obj >= 0 && finite32(dist);
    if (used) used = finite32(g[0]) && finite32(g[1]) && finite32(g[2]) && fabs((double)dist) <= max_dist;
    if (!used) {
        term[IDX_COST] = w * rho(max_dist, huber);
        return;
    }
    const double d = (double)dist, a = fabs(d);
    const double p0 = (double)pw[0], p1 = (double)pw[1], p2 = (double)pw[2];
    const double g0 = (double)g[0], g1 = (double)g[1], g2 = (double)g[2];
    const double J[6] = {g0, g1, g2, p1 * g2 - p2 * g1, p2 * g0 - p0 * g2, p0 * g1 - p1 * g0};
    const double wh = a <= huber ? 1.0 : huber / a;
    const double ww = w * wh;
    int k = IDX_H;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double t = ww * J[i];
#pragma unroll
        for (int j = i; j < 6; ++j) term[k++] = t * J[j];
        term[IDX_B + i] = -(t * d);
    }
    term[IDX_COST] = w * rho(d, huber);
    term[IDX_N] = 1.0;
}

inline double cost_of(const double* sums, double huber, double max_dist) {
    return sums[IDX_W] == 0.0 ? rho(max_dist, huber) : sums[IDX_COST] / sums[IDX_W];
}

// host: the tree over n points' terms (terms[i * NSUM + k]) -> sums[NSUM]
inline void tree_sum(int64_t n, const double* terms, double* sums) {
    for (int k = 0; k < NSUM; ++k) sums[k] = 0.0;
    double lane[WAVE];
    for (int64_t b0 = 0; b0 < n; b0 += BLOCK) {
        for (int k = 0; k < NSUM; ++k) {
            double blk = 0.0;
            for (int w0 = 0; w0 < BLOCK; w0 += WAVE) {
                for (int l = 0; l < WAVE; ++l) {
                    const int64_t i = b0 + w0 + l;
                    lane[l] = i < n ? terms[i * NSUM + k] : 0.0;
                }
                for (int m = WAVE / 2; m >= 1; m >>= 1)
                    for (int l = 0; l < m; ++l) lane[l] = lane[l] + lane[l + m];
                blk = w0 == 0 ? lane[0] : blk + lane[0];
            }
            sums[k] = b0 == 0 ? blk : sums[k] + blk;
        }
    }
}

// host.  t: 16 doubles row-major.  false = refused.  rt: the 12 floats of the point transform
inline bool check_pose(const double* t, float* rt) {
    for (int i = 0; i < 16; ++i)
        if (!finite64(t[i])) return false;
    if (t[12] != 0.0 || t[13] != 0.0 || t[14] != 0.0 || t[15] != 1.0) return false;
    double n[3];
    for (int c = 0; c < 3; ++c) n[c] = (t[c] * t[c] + t[4 + c] * t[4 + c]) + t[8 + c] * t[8 + c];
    const double s2 = ((n[0] + n[1]) + n[2]) / 3.0;
    if (!(s2 > 0.0)) return false;
    const double s = sqrt(s2);
    if (!(fabs(s - 1.0) <= (double)query_math::RIGID_TOL)) return false;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += (t[4 * k + r] / s) * (t[4 * k + c] / s);
            if (!(fabs(d - (r == c ? 1.0 : 0.0)) <= (double)query_math::RIGID_TOL)) return false;
        }
    float out[12];
    for (int i = 0; i < 12; ++i) {
        out[i] = (float)t[i];
        if (!finite32(out[i])) return false;
    }
    for (int i = 0; i < 12; ++i) rt[i] = out[i];
    return true;
}

// host.  H: 6 x 6 row-major, the upper triangle is read.  false = SINGULAR (xi untouched)
inline bool solve(const double* H, const double* b, double damp, double lambda, double* xi) {
    const double dl = damp + lambda;
    double A[6][6], L[6][6] = {}, y[6], x[6];
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = H[6 * i + j];
    for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] + dl;
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(s > 0.0) || !finite64(s)) return false;
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < 6; ++i) {
            double q = A[i][j];
            for (int k = 0; k < j; ++k) q = q - L[i][k] * L[j][k];
            L[i][j] = q / L[j][j];
        }
    }
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    for (int i = 0; i < 6; ++i)
        if (!finite64(x[i])) return false;
    for (int i = 0; i < 6; ++i) xi[i] = x[i];
    return true;
}

// host.  t_out = exp_se3(xi) t_in (16 doubles row-major each; may not alias)
inline void apply_step(const double* xi, const double* t_in, double* t_out) {
    const double w0 = xi[3], w1 = xi[4], w2 = xi[5];
    const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
    const double th = sqrt(th2);
    double a, b, c;
    if (th2 < SMALL_TH2) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
        c = 1.0 / 6.0 - th2 / 120.0;
    } else {
        const double sn = sin(th), cs = cos(th);
        a = sn / th;
        b = (1.0 - cs) / th2;
        c = (th - sn) / (th2 * th);
    }
    const double W[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    double W2[3][3], R[3][3], V[3][3], t[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[i][j] = (W[i][0] * W[0][j] + W[i][1] * W[1][j]) + W[i][2] * W[2][j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double e = i == j ? 1.0 : 0.0;
            R[i][j] = (e + a * W[i][j]) + b * W2[i][j];
            V[i][j] = (e + b * W[i][j]) + c * W2[i][j];
        }
    for (int i = 0; i < 3; ++i) t[i] = (V[i][0] * xi[0] + V[i][1] * xi[1]) + V[i][2] * xi[2];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) t_out[4 * i + j] = (R[i][0] * t_in[j] + R[i][1] * t_in[4 + j]) + R[i][2] * t_in[8 + j];
        t_out[4 * i + 3] = ((R[i][0] * t_in[3] + R[i][1] * t_in[7]) + R[i][2] * t_in[11]) + t[i];
    }
    t_out[12] = 0.0; t_out[13] = 0.0; t_out[14] = 0.0; t_out[15] = 1.0;
}

}  // namespace align_math
