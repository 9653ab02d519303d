// Ray alignment (dsp_map_align_rays, include/dsp_gn.h): projective Gauss-Newton of measured depth rays against the ray-cast map.  The
// arithmetic between the sensor-frame rays, the ray caster's answers and the rows of align_math.h, written once for the device and for the
// host.  The kernels of align_kernels.hip call it from their lanes; dsp_debug_align_ray_rows runs the same functions on the CPU, so the
// arithmetic is tested without a GPU (tests/align_rays_ref.py restates THIS COMMENT in numpy) and the device is held to it bit for bit.
//
// The translation unit that includes this header must be compiled with floating-point contraction off (align_kernels.hip is): every fp32
// operation below is one correctly rounded operation, fmaf where it says fmaf.
//
// Observation i: the measured end point p_s and the ray's origin o_s in the sensor frame (o_s = (0, 0, 0) when the call gives no origins).
// One evaluation of a hypothesis at the pose T:
//   build.     rt = T's [R | t], every entry rounded ONCE to fp32 (align_math.h "Transform");
//              p_w = query_math::to_object(rt, p_s);   o_w = query_math::to_object(rt, o_s).  An ended hypothesis gets NaN p_w and o_w.
//              dir_j = p_w_j - o_w_j  (three subtractions).  raycast_math::ray(o_w, dir, u) decides void and gives the unit direction u;
//              len = sqrtf(norm2(dir)) -- the operations ray itself uses -- is the observed depth along u.
//   cast.      The rows (o_w, dir) of all live hypotheses go through the ray caster (raycast_math.h) in one cast: per row the winner obj,
//              its hit parameter t_hit, dist_hit = sdf s at the hit sample, and the status.
//   gradient.  g_w = align_math::world_gradient(the winner's table entry rt, s, the decoder's d sdf / d xyz at the hit sample): NOT
//              normalised, for the reason align_math.h gives.
//   residual.  gap = len - t_hit;   gu = (g_w0 u0 + g_w1 u1) + g_w2 u2;   d = fmaf(gu, gap, dist_hit): the first-order signed distance from
//              the measured point to the surface patch its ray sees.  It removes the marcher's eps staircase to first order; what is left
//              of it is second order in gap and in eps.
//              A void ray, or a row without a winner (obj < 0), is unmatched with d = +inf; g_w is not read for it.
//   match.     The row is matched when status == HIT (UNDECIDED is not), obj >= 0, gap is finite and |gap| <= max_gap, compared in fp64.
//              obj_row = obj when matched, otherwise -1.  max_gap >= max_dist; +inf = no gate.
//   rows.      align_math::row_terms(p_w, obj_row, d, g_w, w, huber, max_dist) verbatim: the measured point moves with the sensor and the
//              patch stays, so J = [g_w, p_w x g_w] holds.  An unmatched valid ray contributes w rho(max_dist): seeing through a map
//              object costs something.  The sums are align_math.h's tree.
#pragma once
#include "align_math.h"
#include "raycast_math.h"

namespace align_rays_math {

// dir <- p_w - o_w
DSP_QM_HD inline void direction(const float* ow, const float* pw, float* dir) {
    dir[0] = DSP_QM_SUB(pw[0], ow[0]);
    dir[1] = DSP_QM_SUB(pw[1], ow[1]);
    dir[2] = DSP_QM_SUB(pw[2], ow[2]);
}

// u <- the unit direction of dir, *len <- its length.  false = a void ray (u and *len untouched)
DSP_QM_HD inline bool ray(const float* ow, const float* dir, float* u, float* len) {
    if (!raycast_math::ray(ow, dir, u)) return false;
    *len = DSP_QM_SQRT(query_math::norm2(dir[0], dir[1], dir[2]));
    return true;
}

// One row behind the cast.  ok: the ray is not void (u, len from ray()).  g is read only where ok and obj >= 0.  -> obj_row; *d
DSP_QM_HD inline int32_t residual(bool ok, const float* u, float len, int32_t obj, float t_hit, float dist_hit, int32_t status, const float* g,
                                  double max_gap, float* d) {
    if (!ok || obj < 0) {
        *d = query_math::bits_float(0x7f800000u);
        return -1;
    }
    const float gap = DSP_QM_SUB(len, t_hit);
    const float gu = DSP_QM_ADD(DSP_QM_ADD(DSP_QM_MUL(g[0], u[0]), DSP_QM_MUL(g[1], u[1])), DSP_QM_MUL(g[2], u[2]));
    *d = fmaf(gu, gap, dist_hit);
    const bool matched = status == raycast_math::STATUS_HIT && raycast_math::finite32(gap) && fabs((double)gap) <= max_gap;
    return matched ? obj : -1;
}

// nullptr, or what is wrong with the gate (host only)
inline const char* check_gap(double max_gap, double max_dist) {
    return max_gap >= max_dist ? nullptr : "align_rays: max_gap must be >= max_dist and not NaN (+inf: no gate)";
}

}  // namespace align_rays_math
