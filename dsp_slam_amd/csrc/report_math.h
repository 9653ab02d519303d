// Observation report (dsp_batch_report, include/dsp_gn.h): the per-ray arithmetic of the render term (loss.py:84-141), written once for the
// device and for the host.  k_render_scan and k_report_rays (gn_kernels.hip) call the per-sample steps below from their lanes and walk the
// three sequential chains with the wave helpers next to them; report_math::ray is the same ray as ONE scalar function, the chains written
// as plain loops in the same order -- dsp_debug_report_ray runs it on the CPU, so the arithmetic is tested without a GPU and the device is
// held to it bit for bit.
//
// Every operation is a single correctly rounded fp32 operation: on the device the __f*_rn spellings, on the host plain operators -- the
// translation unit that includes this header must be compiled with floating-point contraction off (gn_kernels.hip is).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSP_REPORT_HD __host__ __device__
#else
#define DSP_REPORT_HD
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DSP_RM_ADD(a, b) __fadd_rn(a, b)
#define DSP_RM_SUB(a, b) __fsub_rn(a, b)
#define DSP_RM_MUL(a, b) __fmul_rn(a, b)
#define DSP_RM_DIV(a, b) __fdiv_rn(a, b)
#define DSP_RM_SQRT(a) __fsqrt_rn(a)
#else
#define DSP_RM_ADD(a, b) ((a) + (b))
#define DSP_RM_SUB(a, b) ((a) - (b))
#define DSP_RM_MUL(a, b) ((a) * (b))
#define DSP_RM_DIV(a, b) ((a) / (b))
#define DSP_RM_SQRT(a) sqrtf(a)
#endif

namespace report_math {

constexpr int MAX_DEPTH = 64;       // == MAX_DEPTH_SAMPLES (dsp_internal.h)
constexpr float KEEP_MIN = 1e-2f;   // a band sample becomes a row when de_do > 1e-2 (loss.py:124)
constexpr float RES_CLIP = 0.30f;   // loss.py:139-140

// ---- per-sample steps: one lane of the wave kernels, one loop index of the scalar function -------------------------------------------
// sdf_to_occupancy (loss_utils.py:40-48): 0.5 - clamp(sdf, -th, th) / (2 th)
DSP_REPORT_HD inline float occupancy(float sd, float th) {
    const float cl = fminf(fmaxf(sd, -th), th);
    return DSP_RM_SUB(0.5f, DSP_RM_DIV(cl, DSP_RM_MUL(2.f, th)));
}
// with_grad: -th < sdf < th (loss.py:88)
DSP_REPORT_HD inline bool in_band(float sd, float th) { return sd > -th && sd < th; }
// 1 - o: the factor of the termination chain (1 exactly where there is no sample)
DSP_REPORT_HD inline float pass_through(float o) { return DSP_RM_SUB(1.f, o); }
// the background term's depth: 1.1 d_max (optimizer.py:126)
DSP_REPORT_HD inline float background_depth(float d_last) { return DSP_RM_MUL(1.1f, d_last); }
// d_l o_l T_{l-1}: one term of the rendered depth (loss.py:100-114); t_prev = 1 in front of the first sample
DSP_REPORT_HD inline float depth_term(float d, float o, float t_prev) { return DSP_RM_MUL(d, DSP_RM_MUL(o, t_prev)); }
// loss.py:139-140 as written there -- two masked assignments, NOT fminf / fmaxf: a NaN residual stays NaN
DSP_REPORT_HD inline float clip_residual(float res) {
    res = res > RES_CLIP ? RES_CLIP : res;
    res = res < -RES_CLIP ? -RES_CLIP : res;
    return res;
}
// de_do_k = (sum_{l >= k} T_l) / (1 - o_k) of a band sample; kept when > 1e-2 (loss.py:118-124)
DSP_REPORT_HD inline bool keep_sample(float suffix, float o, float& dedo) {
    dedo = DSP_RM_DIV(suffix, DSP_RM_SUB(1.f, o));
    return dedo > KEEP_MIN;
}
// de_ds = de_do * delta_d * (-1 / (2 th))  (loss.py:125-130)
DSP_REPORT_HD inline float depth_step(float d_first, float d_last, int n_depth) { return DSP_RM_DIV(DSP_RM_SUB(d_last, d_first), (float)(n_depth - 1)); }
DSP_REPORT_HD inline float occupancy_slope(float th) { return DSP_RM_DIV(-1.f, DSP_RM_MUL(2.f, th)); }
DSP_REPORT_HD inline float de_ds(float dedo, float delta_d, float do_ds) { return DSP_RM_MUL(DSP_RM_MUL(dedo, delta_d), do_ds); }

// ---- one ray, scalar -------------------------------------------------------------------------------------------------------------------
// depths[n_depth]: the ray's depth samples; sdf[n_depth]: the value the occupancy scan reads at each, NaN = the sample is not in the unit
// sphere; depth_obs is read for a foreground ray only (a background ray is observed at 1.1 d_max).
// out4 = {d_u, 1 - T_{D-1}, obs - d_u (unclipped), the clipped residual of the render rows};
// counts3 = {in-sphere samples, band samples, kept samples}.  The three chains run in k_render_scan's order: T and d_u front to back, the
// suffix sums of T back to front.
DSP_REPORT_HD inline void ray(int n_depth, const float* depths, const float* sdf, float th, float depth_obs, int is_fg, float* out4, int* counts3) {
    float o[MAX_DEPTH], T[MAX_DEPTH];
    bool wg[MAX_DEPTH];
    int n_in = 0, n_band = 0, n_kept = 0;
    float acc = 1.f;
    for (int j = 0; j < n_depth; ++j) {
        const bool in = !(sdf[j] != sdf[j]);
        o[j] = in ? occupancy(sdf[j], th) : 0.f;
        wg[j] = in && in_band(sdf[j], th);
        n_in += in ? 1 : 0;
        n_band += wg[j] ? 1 : 0;
        acc = DSP_RM_MUL(acc, pass_through(o[j]));
        T[j] = acc;
    }
    const float d_bg = background_depth(depths[n_depth - 1]);
    float du = 0.f;
    for (int j = 0; j < n_depth; ++j) du = DSP_RM_ADD(du, depth_term(depths[j], o[j], j == 0 ? 1.f : T[j - 1]));
    du = DSP_RM_ADD(du, DSP_RM_MUL(d_bg, T[n_depth - 1]));
    const float obs = is_fg ? depth_obs : d_bg;
    const float res = DSP_RM_SUB(obs, du);
    float sacc = 0.f;
    for (int j = n_depth - 1; j >= 0; --j) {
        sacc = DSP_RM_ADD(sacc, T[j]);
        float dedo;
        if (wg[j] && keep_sample(sacc, o[j], dedo)) ++n_kept;
    }
    out4[0] = du;
    out4[1] = DSP_RM_SUB(1.f, T[n_depth - 1]);
    out4[2] = res;
    out4[3] = clip_residual(res);
    counts3[0] = n_in; counts3[1] = n_band; counts3[2] = n_kept;
}

// huber_norm_weights applied to a residual (loss_utils.py:236-265): w r with w = sqrt(rho) / |r| -- the last column of a jacobian row
// (k_gram, build_row), whose squares k_report_members sums
DSP_REPORT_HD inline float robust_residual(float r, float huber_b) {
    const float a = fabsf(r);
    const float rho = (a <= huber_b) ? DSP_RM_MUL(a, a) : DSP_RM_SUB(DSP_RM_MUL(DSP_RM_MUL(2.f, huber_b), a), DSP_RM_MUL(huber_b, huber_b));
    const float w = (a == 0.f) ? 0.f : DSP_RM_DIV(DSP_RM_SQRT(rho), a);
    return DSP_RM_MUL(w, r);
}

}  // namespace report_math
