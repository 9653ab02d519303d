// Map query (dsp_map_query, include/dsp_gn.h): the arithmetic between world points, a map of posed objects and the decoder's rows, written
// once for the device and for the host.  The kernels of query_kernels.hip call it from their lanes; dsp_debug_query_invert / _candidates /
// _select run the same functions on the CPU, so the arithmetic is tested without a GPU and the device is held to it bit for bit.
//
// Every fp32 operation is a single correctly rounded operation: on the device the __f*_rn spellings and fmaf, on the host plain operators
// and fmaf -- the translation unit that includes this header must be compiled with floating-point contraction off (query_kernels.hip is).
//
// invert (host only, fp64, every output rounded ONCE to fp32).  T = [A t; 0 0 0 1] is the object-to-world Sim(3), a_rc = T[4 r + c]:
//     nx = (a00 a00 + a10 a10) + a20 a20   (|A e_x|^2; ny, nz alike from columns 1, 2)
//     s2 = ((nx + ny) + nz) / 3;   s = sqrt(s2);   R_ow[i][j] = a_ji / s2;   t_ow[i] = -((R_ow[i][0] t0 + R_ow[i][1] t1) + R_ow[i][2] t2)
//   with the UNROUNDED fp64 R_ow in t_ow.  Only + * / sqrt, in this order (numpy restates it bit for bit: tests/query_ref.py).  Refused: an
//   entry that is not finite, a bottom row other than exactly 0 0 0 1, s2 <= 0, an A / s whose R^T R is off the identity by more than 1e-4
//   in any entry (the rigidity test of dsp_reconstruct_multiview's view transforms), an output that is not finite in fp32.
//   The device gets 12 floats [R_ow | t_ow] per object, row-major 3 x 4 (rt[4 i + j], j < 3: R_ow[i][j]; rt[4 i + 3]: t_ow[i]), and s.
// to_object:    p_o[i] = fmaf(rt[4i+2], z, fmaf(rt[4i+1], y, fmaf(rt[4i], x, rt[4i+3])))
// norm2:        n2 = (x x + y y) + z z
// inside:       n2 < 1  (strict; false for NaN, like the optimiser's |p| < 1: a point with a NaN coordinate is inside nothing)
// sphere_bound: (sqrtf(n2) - 1) s, for an object that does NOT contain the point
// min_bound:    the per-point bound is the running minimum of sphere_bound over the objects in ascending order, started from +inf.  It is
//               fminf on numbers; a NaN candidate makes the bound NaN and it stays NaN (fminf alone would drop it): a NaN point reports NaN.
// distance:     d = sdf s, one multiply
// orderable:    float bits -> unsigned, monotone: negatives have all bits flipped, non-negatives the sign bit; NaN (either sign) -> 0xffffffff
// key:          (uint64) orderable(d) << 32 | (uint32) obj.  The smallest key wins: the smallest distance, and among equal distances the
//               lowest object index, whatever the order the rows are reduced in.  -0 orders below +0.  A key whose high word is 0xffffffff
//               (the all-ones start value, or a NaN distance) is no winner: obj = -1, dist = +inf.
// normal:       g = the row's d sdf / d xyz (object frame).  u_j = fmaf(rt[8+j], gz, fmaf(rt[4+j], gy, rt[j] gx)) = (R_ow^T g)_j, which is g
//               rotated into the world frame and divided by s;  u2 = norm2(u);  n_w = u / sqrtf(u2).  Zero when norm2(g) < TINY (the rule of
//               surface_math.h) or u2 == 0; a NaN gradient gives a NaN normal.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSP_QM_HD __host__ __device__
#else
#define DSP_QM_HD
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DSP_QM_ADD(a, b) __fadd_rn(a, b)
#define DSP_QM_SUB(a, b) __fsub_rn(a, b)
#define DSP_QM_MUL(a, b) __fmul_rn(a, b)
#define DSP_QM_DIV(a, b) __fdiv_rn(a, b)
#else
#define DSP_QM_ADD(a, b) ((a) + (b))
#define DSP_QM_SUB(a, b) ((a) - (b))
#define DSP_QM_MUL(a, b) ((a) * (b))
#define DSP_QM_DIV(a, b) ((a) / (b))
#endif
// sqrtf on both sides: the correctly rounded square root (surface_math.h)
#define DSP_QM_SQRT(a) sqrtf(a)

namespace query_math {

constexpr float TINY = 1e-20f;          // == surface_math::TINY
constexpr float RIGID_TOL = 1e-4f;      // the tolerance of make_groups (dsp_gn.hip) on R^T R
constexpr int OBJ_STRIDE = 16;          // floats per object of the device table: rt[12], s, s_sel, 0, 0 (s_sel: s, or NaN for an object that must never win)
constexpr uint64_t NO_KEY = ~(uint64_t)0;

// host only.  t: 16 floats row-major.  false = refused (rt / s untouched)
inline bool invert(const float* t, float* rt, float* s_out) {
    for (int i = 0; i < 16; ++i)
        if (!(fabsf(t[i]) <= 3.402823466e+38f)) return false;
    if (t[12] != 0.f || t[13] != 0.f || t[14] != 0.f || t[15] != 1.f) return false;
    double a[3][3], tr[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) a[r][c] = (double)t[4 * r + c];
        tr[r] = (double)t[4 * r + 3];
    }
    double n[3];
    for (int c = 0; c < 3; ++c) n[c] = (a[0][c] * a[0][c] + a[1][c] * a[1][c]) + a[2][c] * a[2][c];
    const double s2 = ((n[0] + n[1]) + n[2]) / 3.0;
    if (!(s2 > 0.0)) return false;
    const double s = sqrt(s2);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += (a[k][r] / s) * (a[k][c] / s);
            if (!(fabs(d - (r == c ? 1.0 : 0.0)) <= RIGID_TOL)) return false;
        }
    float out[12];
    for (int i = 0; i < 3; ++i) {
        double row[3];
        for (int j = 0; j < 3; ++j) row[j] = a[j][i] / s2;
        const double ti = -((row[0] * tr[0] + row[1] * tr[1]) + row[2] * tr[2]);
        for (int j = 0; j < 3; ++j) out[4 * i + j] = (float)row[j];
        out[4 * i + 3] = (float)ti;
    }
    const float sf = (float)s;
    for (int i = 0; i < 12; ++i)
        if (!(fabsf(out[i]) <= 3.402823466e+38f)) return false;
    if (!(fabsf(sf) <= 3.402823466e+38f) || !(sf > 0.f)) return false;
    memcpy(rt, out, sizeof out);
    *s_out = sf;
    return true;
}

DSP_QM_HD inline void to_object(const float* rt, float x, float y, float z, float* p) {
    p[0] = fmaf(rt[2], z, fmaf(rt[1], y, fmaf(rt[0], x, rt[3])));
    p[1] = fmaf(rt[6], z, fmaf(rt[5], y, fmaf(rt[4], x, rt[7])));
    p[2] = fmaf(rt[10], z, fmaf(rt[9], y, fmaf(rt[8], x, rt[11])));
}
DSP_QM_HD inline float norm2(float x, float y, float z) { return DSP_QM_ADD(DSP_QM_ADD(DSP_QM_MUL(x, x), DSP_QM_MUL(y, y)), DSP_QM_MUL(z, z)); }
DSP_QM_HD inline bool inside(float n2) { return n2 < 1.f; }
DSP_QM_HD inline float sphere_bound(float n2, float s) { return DSP_QM_MUL(DSP_QM_SUB(DSP_QM_SQRT(n2), 1.f), s); }
DSP_QM_HD inline float min_bound(float b, float v) { return v < b ? v : (v != v ? v : b); }
DSP_QM_HD inline float distance(float sdf, float s) { return DSP_QM_MUL(sdf, s); }

DSP_QM_HD inline uint32_t float_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
#endif
}
DSP_QM_HD inline float bits_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float x;
    memcpy(&x, &u, 4);
    return x;
#endif
}
DSP_QM_HD inline uint32_t orderable(float d) {
    if (d != d) return 0xffffffffu;
    const uint32_t u = float_bits(d);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}
DSP_QM_HD inline float from_orderable(uint32_t o) { return bits_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }
DSP_QM_HD inline uint64_t key(float d, int32_t obj) { return ((uint64_t)orderable(d) << 32) | (uint64_t)(uint32_t)obj; }
// key -> (obj, dist); a key whose high word is all ones is no winner
DSP_QM_HD inline void unpack(uint64_t k, int32_t* obj, float* dist) {
    const uint32_t hi = (uint32_t)(k >> 32);
    if (hi == 0xffffffffu) {
        *obj = -1;
        *dist = bits_float(0x7f800000u);
    } else {
        *obj = (int32_t)(uint32_t)(k & 0xffffffffu);
        *dist = from_orderable(hi);
    }
}

DSP_QM_HD inline void normal(const float* rt, float gx, float gy, float gz, float* n) {
    const float g2 = norm2(gx, gy, gz);
    const float ux = fmaf(rt[8], gz, fmaf(rt[4], gy, DSP_QM_MUL(rt[0], gx)));
    const float uy = fmaf(rt[9], gz, fmaf(rt[5], gy, DSP_QM_MUL(rt[1], gx)));
    const float uz = fmaf(rt[10], gz, fmaf(rt[6], gy, DSP_QM_MUL(rt[2], gx)));
    const float u2 = norm2(ux, uy, uz);
    const float un = DSP_QM_SQRT(u2);
    const bool flat = g2 < TINY || u2 == 0.f;
    n[0] = flat ? 0.f : DSP_QM_DIV(ux, un);
    n[1] = flat ? 0.f : DSP_QM_DIV(uy, un);
    n[2] = flat ? 0.f : DSP_QM_DIV(uz, un);
}

}  // namespace query_math
