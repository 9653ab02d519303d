// Object refinement (dsp_map_align_objects, include/dsp_gn.h): the sensor is known, the OBJECTS move.  One rigid correction per map object
// is solved for against depth rays given in the world frame.  The arithmetic that is not align_math.h's or align_rays_math.h's, written once
// for the device and for the host.  The kernels of align_objects_kernels.hip call row_terms from their lanes; dsp_debug_align_objects_rows /
// _compose run the same functions on the CPU, so the arithmetic is tested without a GPU (tests/align_objects_ref.py restates THIS COMMENT in
// numpy) and the device is held to it bit for bit.
//
// The translation unit that includes this header must be compiled with floating-point contraction off (align_objects_kernels.hip is).
//
// Observation i: the measured end point p_w and the ray's origin o_w, both in the WORLD frame (the caller applies the known sensor poses;
// rays of several frames or sensors are simply concatenated).  dir = p_w - o_w (align_rays_math::direction), made once.
// State.     One fp64 rigid correction C_k per object, identity at the start; object k's pose at an evaluation is T_k = C_k T_k0.
// compose.   T_k0 is the fp32 input pose, converted exactly to fp64.  R' = C_R A, t' = C_R t0 + C_t in fp64, dot products written
//            (a0 b0 + a1 b1) + a2 b2, the translation ((..) + ..) + C_t[i]; every entry rounded ONCE to fp32; bottom row 0 0 0 1.  A C that
//            is exactly the identity (all 16 entries) gives T_k0's own bytes: an object that never moved keeps its input pose, -0 included.
// table.     The object table of an evaluation comes from the composed fp32 poses through the map's own inversion (query_math::invert).
//            If the inversion refuses a composed pose, that object ends with SINGULAR at its accepted state.
// cast.      All rays (o_w, dir) go through ONE cast of the map (raycast_math.h) at the poses T_k: an object that has ended, or that is
//            not refined, stays in the map at its accepted pose -- it still occludes -- and an evaluated object stands at its trial pose.
// gradient, residual, match.  align_rays_math.h verbatim (ray, residual, align_math::world_gradient), the max_gap gate included.
// owner.     Ray i belongs to the object the cast names as its winner (obj >= 0), matched or not: an unmatched ray contributes
//            w rho(max_dist) to that object's cost through align_math::row_terms(p_w, obj_row, d, g_w, w, ..), unchanged.  A ray without a
//            winner belongs to no object.  No ray is ever charged to an object that it does not see.
// sums.      The align_math::NSUM sums of object k run over its winners in ascending ray order through align_math's tree: blocks of BLOCK
//            consecutive LIST positions padded with zero terms, the butterfly inside a wave, waves ascending, blocks ascending.  The tree is
//            a function of the list alone: not of the cast's passes, the winners' chunks or the grid.  An empty list sums to zero.  No
//            float atomics.
// sign.      The measured point is fixed and the object moves by C <- exp(xi) C, so d(p; exp(xi) C) ~ d - g_w . v - omega . (p_w x g_w): the
//            jacobian is -[g_w, p_w x g_w].  H is row_terms's; b is its negation.  The host negates the six b sums after the read-back
//            (exact; a zero sum becomes -0): the only difference to the sensor's system.
// loop.      align_loop (map_host.hip) with "hypothesis" = object and T = C_k: statuses, min_points, damping, the opt-in step rule,
//            tolerances, align_math::solve and apply_step.  Objects are coupled only through occlusion; each decides on its own cost
//            F_k = sum cost / sum w over that evaluation's winners.
// LIMIT.     The winner set changes between evaluations, so F_k compares means over different sets of rays (a trial that loses its worst
//            rays to a neighbour, or to the void, looks better than it is).  The step rule and cost0 / cost are to be read with that in mind.
// Jacobian rows of objects that are not evaluated (not refined, or ended) are still decoded by the cast's winner pass and ignored: the
// chunk plan is shared with dsp_map_raycast and cutting objects out of it would change it.
//
// Code refinement is dsp_map_align_shapes (align_shapes_math.h).  Out of scope: scale; a world-axis mask on the six degrees of freedom (yaw
// only); a prior on the correction; the conversion of H into an edge of dsp_pg_edge_information.
#pragma once
#include "align_math.h"
#include "align_rays_math.h"

namespace align_objects_math {

// host.  c: 16 doubles row-major (rigid), t0: 16 floats row-major -> out: 16 floats
inline void compose(const double* c, const float* t0, float* out) {
    bool identity = true;
    for (int i = 0; i < 16; ++i) identity = identity && c[i] == ((i % 5 == 0) ? 1.0 : 0.0);
    if (identity) {
        memcpy(out, t0, 16 * sizeof(float));
        return;
    }
    double t[16];
    for (int i = 0; i < 16; ++i) t[i] = (double)t0[i];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out[4 * i + j] = (float)((c[4 * i] * t[j] + c[4 * i + 1] * t[4 + j]) + c[4 * i + 2] * t[8 + j]);
        out[4 * i + 3] = (float)(((c[4 * i] * t[3] + c[4 * i + 1] * t[7]) + c[4 * i + 2] * t[11]) + c[4 * i + 3]);
    }
    out[12] = 0.f; out[13] = 0.f; out[14] = 0.f; out[15] = 1.f;
}

}  // namespace align_objects_math
