// Surface projection (dsp_surface_points / dsp_meshes_refine, include/dsp_gn.h): the per-point arithmetic behind the decoder's row
// {d sdf / d code [64], d sdf / d xyz [3], sdf}, written once for the device and for the host.  k_surface_step and k_surface_attributes
// (surface_kernels.hip) call it from their lanes; dsp_debug_surface_step / dsp_debug_surface_attributes run the same functions on the
// CPU, so the arithmetic is tested without a GPU and the device is held to it bit for bit.
//
// Every operation is a single correctly rounded fp32 operation: on the device the __f*_rn spellings, on the host plain operators -- the
// translation unit that includes this header must be compiled with floating-point contraction off (surface_kernels.hip is).
//
// Constants:
//   TINY      = 1e-20   a squared gradient norm below it means "no direction": step() leaves the point where it is, attributes() returns a
//                       zero normal and a zero sigma
//   MAX_STEPS = 8       the most Newton steps one call runs (n_steps 0 .. 8)
//   max_step            (argument, > 0) the longest move of one step; a longer Newton step is scaled to exactly this length.  The mesh path's
//                       default is one voxel of the extraction, 2 / (vol_dim - 1).
//
// step:        g2 = (gx gx + gy gy) + gz gz;  k = sdf / g2;  d = k g;  d2 = (dx dx + dy dy) + dz dz;
//              d2 > max_step max_step:  d = (max_step / sqrt(d2)) d;      p' = p - d
//              g2 < TINY, or g2 / any entry of d not finite:  p' = p      (a NaN point stays NaN)
// attributes:  gn = sqrt(g2);  normal = g / gn (g2 < TINY: 0; a NaN gradient gives a NaN normal);  grad_norm = gn;  sdf = row[67];
//              sigma = sqrt(S) / gn (g2 < TINY: 0),  S = sum_k (gc_k gc_k) var_k in the fixed order below -- the first-order standard deviation
//              of the surface's displacement along the normal under the code's variance.
// bad points: a point with a coordinate that is not finite has NaN in all its outputs (coordinates included) and takes no step -- the
//              decoder's ReLUs would turn a NaN input into a finite value, so the kernels test the point itself (point_ok, nan_attr).
// The sum S:   lane l of 16 holds entries 4l .. 4l+3 and adds their terms left to right, ((t0 + t1) + t2) + t3; then an xor butterfly over the
//              16 lanes with the masks 1, 2, 4, 8 in that order, v_l <- v_l + v_{l ^ mask}.  fp32 addition commutes, so every lane ends with the
//              same value; lane 0's is S.  lane_sum / butterfly_host below are that tree; the kernel runs the butterfly with __shfl_xor.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSP_SURF_HD __host__ __device__
#else
#define DSP_SURF_HD
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DSP_SM_ADD(a, b) __fadd_rn(a, b)
#define DSP_SM_SUB(a, b) __fsub_rn(a, b)
#define DSP_SM_MUL(a, b) __fmul_rn(a, b)
#define DSP_SM_DIV(a, b) __fdiv_rn(a, b)
#else
#define DSP_SM_ADD(a, b) ((a) + (b))
#define DSP_SM_SUB(a, b) ((a) - (b))
#define DSP_SM_MUL(a, b) ((a) * (b))
#define DSP_SM_DIV(a, b) ((a) / (b))
#endif
// sqrtf on both sides: the HIP headers' __fsqrt_rn is the native (1 ulp) square root, sqrtf the correctly rounded one
#define DSP_SM_SQRT(a) sqrtf(a)

namespace surface_math {

constexpr float TINY = 1e-20f;
constexpr int MAX_STEPS = 8;
constexpr int CODE = 64;        // == CODE_LEN (dsp_internal.h)
constexpr int ROW = 68;         // == GRAD_STRIDE: d/dcode[64], d/dxyz[3], sdf
constexpr int LANES = 16;       // lanes per point of the 64-term sum, 4 entries each
constexpr int N_MASKS = 4;
DSP_SURF_HD constexpr int mask(int m) { return 1 << m; }       // 1, 2, 4, 8

DSP_SURF_HD inline bool finite(float x) { return fabsf(x) <= 3.402823466e+38f; }      // false for NaN and +-inf
DSP_SURF_HD inline float norm2(float x, float y, float z) { return DSP_SM_ADD(DSP_SM_ADD(DSP_SM_MUL(x, x), DSP_SM_MUL(y, y)), DSP_SM_MUL(z, z)); }

// one capped Newton step along the gradient; p, g, out: 3 floats (out may alias p)
DSP_SURF_HD inline void step(const float* p, float sdf, const float* g, float max_step, float* out) {
    const float px = p[0], py = p[1], pz = p[2];
    const float g2 = norm2(g[0], g[1], g[2]);
    bool move = g2 >= TINY && finite(g2);
    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (move) {
        const float k = DSP_SM_DIV(sdf, g2);
        dx = DSP_SM_MUL(k, g[0]); dy = DSP_SM_MUL(k, g[1]); dz = DSP_SM_MUL(k, g[2]);
        const float d2 = norm2(dx, dy, dz);
        if (d2 > DSP_SM_MUL(max_step, max_step)) {
            const float s = DSP_SM_DIV(max_step, DSP_SM_SQRT(d2));
            dx = DSP_SM_MUL(s, dx); dy = DSP_SM_MUL(s, dy); dz = DSP_SM_MUL(s, dz);
        }
        move = finite(dx) && finite(dy) && finite(dz);
    }
    out[0] = move ? DSP_SM_SUB(px, dx) : px;
    out[1] = move ? DSP_SM_SUB(py, dy) : py;
    out[2] = move ? DSP_SM_SUB(pz, dz) : pz;
}

// lane l's share of S: its four terms, left to right.  gc4 / var4: entries 4l .. 4l+3 of the row's code gradient / of the variance
DSP_SURF_HD inline float lane_sum(const float* gc4, const float* var4) {
    float s = DSP_SM_MUL(DSP_SM_MUL(gc4[0], gc4[0]), var4[0]);
    s = DSP_SM_ADD(s, DSP_SM_MUL(DSP_SM_MUL(gc4[1], gc4[1]), var4[1]));
    s = DSP_SM_ADD(s, DSP_SM_MUL(DSP_SM_MUL(gc4[2], gc4[2]), var4[2]));
    s = DSP_SM_ADD(s, DSP_SM_MUL(DSP_SM_MUL(gc4[3], gc4[3]), var4[3]));
    return s;
}
// the butterfly over the 16 lane sums as a loop; v is overwritten, every entry ends as S
DSP_SURF_HD inline void butterfly_host(float* v) {
    for (int m = 0; m < N_MASKS; ++m) {
        float w[LANES];
        for (int l = 0; l < LANES; ++l) w[l] = DSP_SM_ADD(v[l], v[l ^ mask(m)]);
        for (int l = 0; l < LANES; ++l) v[l] = w[l];
    }
}

// what one point's outputs are once S is known (S is ignored when has_var is false: sigma is not written then)
struct Attr { float nx, ny, nz, grad_norm, sdf, sigma; };
DSP_SURF_HD inline Attr finish(float gx, float gy, float gz, float sdf, float S, bool has_var) {
    Attr a;
    const float g2 = norm2(gx, gy, gz);
    const float gn = DSP_SM_SQRT(g2);
    const bool flat = g2 < TINY;
    a.nx = flat ? 0.f : DSP_SM_DIV(gx, gn);
    a.ny = flat ? 0.f : DSP_SM_DIV(gy, gn);
    a.nz = flat ? 0.f : DSP_SM_DIV(gz, gn);
    a.grad_norm = gn;
    a.sdf = sdf;
    a.sigma = (!has_var || flat) ? 0.f : DSP_SM_DIV(DSP_SM_SQRT(S), gn);
    return a;
}

// a point the projection refuses (see "bad points" above) and what it returns
DSP_SURF_HD inline bool point_ok(float x, float y, float z) { return finite(x) && finite(y) && finite(z); }
DSP_SURF_HD inline Attr nan_attr() {
    const float q = nanf("");
    return Attr{q, q, q, q, q, q};
}

// one row on the host: row68 as mlp_kernel<2> writes it, var = 64 floats or null
DSP_SURF_HD inline Attr attributes(const float* row68, const float* var) {
    float v[LANES];
    if (var) {
        for (int l = 0; l < LANES; ++l) v[l] = lane_sum(row68 + 4 * l, var + 4 * l);
        butterfly_host(v);
    }
    return finish(row68[64], row68[65], row68[66], row68[67], var ? v[0] : 0.f, var != nullptr);
}

}  // namespace surface_math
