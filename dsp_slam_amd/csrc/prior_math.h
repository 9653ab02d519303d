// Gaussian prior on pose and code (dsp_batch_prior, include/dsp_gn.h): the fp64 arithmetic of k_prior_terms, written once for the device
// and for the host (dsp_debug_prior_terms runs the very same functions on the CPU, so every branch is tested without a GPU).
//
// Unknowns as in H: [v(3), w(3), sigma | code(64)].  Prior residual at the state (T_oc, z):
//     e_p = Log(T_oc T0^-1)   -- the logarithm of the STANDARD Sim(3) exponential, hat(xi) = [[w^ + sigma I, v], [0, 0]]
//     e_c = z - z0
// linearised for the update T_oc <- exp(dx) T_oc with the BCH series of the inverse left jacobian,
//     J_p = I - 1/2 ad(e_p) + 1/12 ad(e_p)^2,   ad([v, w, s]) = [[w^ + s I, v^, -v], [0, w^, 0], [0, 0, 0]]
// Both 4 x 4 matrices are read as affine maps: their bottom rows are taken to be [0 0 0 1].
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSP_HD __host__ __device__
#else
#define DSP_HD
#endif

namespace prior_math {

constexpr int NS = 71;              // unknowns of a joint / multi-view batch (a pose-only batch: 6)
constexpr int RES_STRIDE = 72;      // doubles per object of the residual record: e (P + 64) | ... | chi2 at [71]
constexpr double HALF_TURN_MARGIN = 1e-3;

// V = A I + B W + C W^2 (W = w^, theta = |w|) is the matrix that multiplies v in the Sim(3) exponential:
//     V = int_0^1 exp(a (sigma I + W)) da,   A = int e^(sigma a) da,   B = int e^(sigma a) sin(theta a) da / theta,
//     C = int e^(sigma a) (1 - cos(theta a)) da / theta^2.
// theta >= 1/4: closed forms (sigma small: expm1).  theta < 1/4: the series in theta^2 of B and C over the moments
// I_n = int_0^1 e^(sigma a) a^n da, which come from a Taylor series of the highest one and the backward recurrence
// I_(n-1) = (e^sigma - sigma I_n) / n for |sigma| < 1, from I_0 and the forward recurrence I_n = (e^sigma - n I_(n-1)) / sigma otherwise
// (each is the stable direction in its range: the error a step passes on is scaled by |sigma| / n, respectively n / |sigma|, and moment
// n enters B and C divided by n!).
DSP_HD inline void v_coeffs(double sg, double th, double& A, double& B, double& C) {
    const double es = exp(sg);
    A = sg == 0.0 ? 1.0 : expm1(sg) / sg;
    if (th >= 0.25) {
        const double sn = sin(th), cs = cos(th), q = sg * sg + th * th;
        const double X = (es * (sg * cs + th * sn) - sg) / q;      // int e^(sigma a) cos(theta a) da
        const double Y = (es * (sg * sn - th * cs) + th) / q;      // int e^(sigma a) sin(theta a) da
        B = Y / th;
        C = (A - X) / (th * th);
        return;
    }
    constexpr int NM = 15;              // moments I_0 .. I_14: theta^12 / 14! < 1e-18 for theta < 1/4
    double I[NM + 1];
    if (fabs(sg) < 1.0) {
        double top = 0.0, term = 1.0;   // I_15 = sum_m sigma^m / (m! (16 + m))
        for (int m = 0; m < 22; ++m) { top += term / (double)(NM + 1 + m); term *= sg / (double)(m + 1); }
        I[NM] = top;
        for (int n = NM; n >= 1; --n) I[n - 1] = (es - sg * I[n]) / (double)n;
    } else {
        I[0] = A;
        for (int n = 1; n <= NM; ++n) I[n] = (es - (double)n * I[n - 1]) / sg;
    }
    const double t2 = th * th;
    double b = 0.0, c = 0.0, p = 1.0, f = 1.0;     // p = (-theta^2)^k, f = (2k + 1)!
    for (int k = 0; k < 7; ++k) {
        b += p * I[2 * k + 1] / f;
        c += p * I[2 * k + 2] / (f * (double)(2 * k + 2));
        p *= -t2;
        f *= (double)((2 * k + 2) * (2 * k + 3));
    }
    B = b;
    C = c;
}

DSP_HD inline double det3x3(const double* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
DSP_HD inline void adj3x3(const double* m, double* a) {      // adjugate: inverse times the determinant
    a[0] = m[4] * m[8] - m[5] * m[7]; a[1] = m[2] * m[7] - m[1] * m[8]; a[2] = m[1] * m[5] - m[2] * m[4];
    a[3] = m[5] * m[6] - m[3] * m[8]; a[4] = m[0] * m[8] - m[2] * m[6]; a[5] = m[2] * m[3] - m[0] * m[5];
    a[6] = m[3] * m[7] - m[4] * m[6]; a[7] = m[1] * m[6] - m[0] * m[7]; a[8] = m[0] * m[4] - m[1] * m[3];
}

// Log of the affine map [M | t] (M = s R): e = [v, w, sigma].  false: det M <= 0, or a rotation angle beyond pi - HALF_TURN_MARGIN (also NaN).
DSP_HD inline bool sim3_log(const double* M, const double* t, double* e) {
    const double det = det3x3(M);
    if (!(det > 0.0)) return false;
    const double s = cbrt(det), sg = log(s);
    double R[9];
    for (int i = 0; i < 9; ++i) R[i] = M[i] / s;
    const double a0 = 0.5 * (R[7] - R[5]), a1 = 0.5 * (R[2] - R[6]), a2 = 0.5 * (R[3] - R[1]);
    const double sn = sqrt(a0 * a0 + a1 * a1 + a2 * a2), cs = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    const double th = atan2(sn, cs);
    if (!(th <= 3.14159265358979323846 - HALF_TURN_MARGIN)) return false;
    const double k = th < 1e-4 ? 1.0 + th * th / 6.0 + 7.0 * th * th * th * th / 360.0 : th / sn;      // theta / sin(theta)
    const double w0 = k * a0, w1 = k * a1, w2 = k * a2;
    double A, B, C;
    v_coeffs(sg, th, A, B, C);
    const double W[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    double V[9], Va[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double w2rc = W[3 * r] * W[c] + W[3 * r + 1] * W[3 + c] + W[3 * r + 2] * W[6 + c];
            V[3 * r + c] = (r == c ? A : 0.0) + B * W[3 * r + c] + C * w2rc;
        }
    adj3x3(V, Va);
    const double dv = det3x3(V);
    for (int r = 0; r < 3; ++r) e[r] = (Va[3 * r] * t[0] + Va[3 * r + 1] * t[1] + Va[3 * r + 2] * t[2]) / dv;
    e[3] = w0; e[4] = w1; e[5] = w2; e[6] = sg;
    return true;
}

// D = T_oc T0^-1 from the two fp32 matrices, in fp64, and its logarithm.  P = 6 (pose-only batches: both matrices carry the same scale):
// the same logarithm with the sigma entry dropped.
DSP_HD inline bool pose_residual(const float* t_oc, const float* t0, double* e7) {
    double A0[9], Ai[9], Ac[9], t0v[3], tcv[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { A0[3 * r + c] = (double)t0[4 * r + c]; Ac[3 * r + c] = (double)t_oc[4 * r + c]; }
        t0v[r] = (double)t0[4 * r + 3];
        tcv[r] = (double)t_oc[4 * r + 3];
    }
    const double d0 = det3x3(A0);
    if (!(d0 > 0.0)) return false;
    adj3x3(A0, Ai);
    double M[9], t[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[3 * r + c] = (Ac[3 * r] * Ai[c] + Ac[3 * r + 1] * Ai[3 + c] + Ac[3 * r + 2] * Ai[6 + c]) / d0;
    for (int r = 0; r < 3; ++r) t[r] = tcv[r] - (M[3 * r] * t0v[0] + M[3 * r + 1] * t0v[1] + M[3 * r + 2] * t0v[2]);
    return sim3_log(M, t, e7);
}

// J_p (7 x 7, row-major; a pose-only batch reads its top-left 6 x 6, built with sigma = 0)
DSP_HD inline void jac_pose(const double* e, int P, double* J) {
    const double v0 = e[0], v1 = e[1], v2 = e[2], w0 = e[3], w1 = e[4], w2 = e[5], sg = P == 7 ? e[6] : 0.0;
    double ad[49];
    for (int i = 0; i < 49; ++i) ad[i] = 0.0;
    const double W[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0}, Vh[9] = {0.0, -v2, v1, v2, 0.0, -v0, -v1, v0, 0.0};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            ad[7 * r + c] = W[3 * r + c] + (r == c ? sg : 0.0);
            ad[7 * r + 3 + c] = Vh[3 * r + c];
            ad[7 * (3 + r) + 3 + c] = W[3 * r + c];
        }
        ad[7 * r + 6] = -e[r];
    }
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) {
            double a2 = 0.0;
            for (int k = 0; k < 7; ++k) a2 += ad[7 * i + k] * ad[7 * k + j];
            J[7 * i + j] = (i == j ? 1.0 : 0.0) - 0.5 * ad[7 * i + j] + a2 / 12.0;
        }
}

// Work area of one object (LDS on the device)
struct Work {
    double e[NS];       // e_p (P) | e_c (64)
    double J[49];       // J_p, stride 7
    double T[49];       // Lp_pp J_p, stride 7
    double y[NS];       // Lp e
    int ok;
};

// The three phases of one object's terms; thread tid of nt (the host: 0 of 1); a barrier between two phases.
// Lp: n x n (n = P + 64 = 71, pose-only n = 6), symmetric bit for bit -- rows are read as columns where that coalesces.
// phase 0: e and J_p
DSP_HD inline void phase0(Work& w, int tid, int nt, int P, bool pose_only, const float* t_oc, const float* code, const float* t0, const float* z0) {
    if (tid == 0) {
        double e7[7];
        w.ok = pose_residual(t_oc, t0, e7) ? 1 : 0;
        if (!w.ok) for (int i = 0; i < 7; ++i) e7[i] = 0.0;
        for (int i = 0; i < P; ++i) w.e[i] = e7[i];
        jac_pose(e7, P, w.J);
    }
    if (!pose_only)
        for (int i = tid; i < 64; i += nt) w.e[P + i] = (double)code[i] - (double)z0[i];
}
// phase 1: y = Lp e (k ascending) and T = Lp_pp J_p
DSP_HD inline void phase1(Work& w, int tid, int nt, int P, int n, const double* Lp) {
    for (int i = tid; i < n; i += nt) {
        double a = 0.0;
        for (int k = 0; k < n; ++k) a += Lp[(size_t)k * n + i] * w.e[k];
        w.y[i] = a;
    }
    for (int idx = tid; idx < P * P; idx += nt) {
        const int a = idx / P, j = idx % P;
        double acc = 0.0;
        for (int bb = 0; bb < P; ++bb) acc += Lp[(size_t)a * n + bb] * w.J[7 * bb + j];
        w.T[7 * a + j] = acc;
    }
}
// phase 2: entry (i, j) of [J^T Lp J | -J^T Lp e], j == n: the right-hand side.  live = P + the decoder's code length: zero beyond it.
DSP_HD inline double extra_entry(const Work& w, int i, int j, int P, int n, int live, const double* Lp) {
    if (i >= live || (j >= live && j != n)) return 0.0;
    if (j == n) {
        if (i >= P) return -w.y[i];
        double a = 0.0;
        for (int k = 0; k < P; ++k) a += w.J[7 * k + i] * w.y[k];
        return -a;
    }
    if (i >= P && j >= P) return Lp[(size_t)i * n + j];
    if (i < P && j < P) {            // the lower triangle's sum for both halves: symmetric bit for bit
        const int r = i > j ? i : j, c = i > j ? j : i;
        double a = 0.0;
        for (int k = 0; k < P; ++k) a += w.J[7 * k + r] * w.T[7 * k + c];
        return a;
    }
    const int p = i < P ? i : j, c = i < P ? j : i;      // pose row p, code column c (and its mirror image)
    double a = 0.0;
    for (int k = 0; k < P; ++k) a += w.J[7 * k + p] * Lp[(size_t)k * n + c];
    return a;
}
DSP_HD inline double chi2_of(const Work& w, int n) {
    double a = 0.0;
    for (int i = 0; i < n; ++i) a += w.e[i] * w.y[i];
    return a;
}

}  // namespace prior_math
