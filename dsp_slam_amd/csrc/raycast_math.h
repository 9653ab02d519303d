// Ray casting against the object map (dsp_map_raycast, include/dsp_gn.h): the arithmetic between world rays, the map's object table and the
// decoder's rows, written once for the device and for the host in the manner of query_math.h, whose to_object, norm2, orderable, key, unpack
// and normal it reuses.  The kernels of raycast_kernels.hip call it from their lanes; dsp_debug_raycast_segments / _step run the same
// functions on the CPU.  Every fp32 operation is a single correctly rounded operation (the including translation unit is compiled with
// contraction off); fmaf where written.  tests/raycast_ref.py restates THIS COMMENT in numpy.
//
// ray (origin o, direction d, fp32, world frame):
//     n2 = norm2(d) = (dx dx + dy dy) + dz dz;   len = sqrtf(n2);   u = (dx / len, dy / len, dz / len)
//   void: any of the six numbers is not finite, or n2 is 0 or not finite.  A void ray has no pair with any object.
// segment (ray, object with table entry rt[12] = [R_ow | t_ow], s, s_sel):
//     o_o   = to_object(rt, o)
//     d_o_i = fmaf(rt[4i+2], uz, fmaf(rt[4i+1], uy, rt[4i] ux))        (R_ow u; R_ow carries 1 / s, so the world parameter t is the object-frame one)
//     a = norm2(d_o);   b = (o_ox d_ox + o_oy d_oy) + o_oz d_oz;   c = norm2(o_o) - 1
//     disc = fmaf(b, b, -(a c));   q = sqrtf(disc);   t_in = ((-b) - q) / a;   t_out = (q - b) / a        (|o_o + t d_o|^2 = 1)
//   the pair exists when disc > 0 and t_out > t_min and t_in < t_max and s_sel is not NaN (every comparison false for NaN).  Its march
//   runs over [t0, t1]:  t0 = t_in > t_min ? t_in : t_min;   t1 = t_out < t_max ? t_out : t_max.  It starts at t = t0.
// sample at parameter t:   p_i = fmaf(t, d_o_i, o_o_i)
// step rule, with sdf the decoder's value at the sample and dist = sdf s (one multiply):
//     dist is NaN        -> MISS   (the pair ends)
//     dist <= eps        -> HIT    (the pair ends with hit parameter t and that dist)
//     t' = fmaf(relax, dist, t);   t' > t1 -> EXIT (the pair ends as a miss);   otherwise ADVANCE: the pair's next sample is at t'
//   A pair that has taken max_steps samples without ending is EXHAUSTED; its parameter is the t' it would have sampled next.
// winner per ray: the smallest key(t_hit, obj) = orderable(t_hit) << 32 | obj over the ray's hits: the nearest hit, the lowest object index
//   among equal parameters, whatever the order of reduction.  obj, t from unpack(key); dist is the winning pair's; no hit: -1, +inf, +inf.
// status per ray: UNDECIDED if some pair of the ray was exhausted at a parameter strictly below the winner's t_hit, or was exhausted and
//   the ray has no winner; otherwise HIT with a winner, MISS without.  An UNDECIDED ray still reports the winner it has.
// occlusion retirement: at the start of a round (one sample of every live pair of a pass), a live pair whose parameter t is strictly
//   greater than its ray's best t_hit AS IT STOOD WHEN THE PREVIOUS ROUND ENDED (for the first round of a pass: when the previous pass ended)
//   ends as a miss.  It could only have hit behind the winner, so no output changes; the rows of every round are a function of the inputs and
//   of the pass cut alone.
// normal of a winner: the decoder's gradient g at the winner's hit sample, through query_math::normal.
//
// params: t_min >= 0, t_max > t_min (t_max may be +inf), eps > 0 and finite, 0 < relax <= 1, 1 <= max_steps <= 4096.
// Defaults (dsp_raycast_params_default): t_min 0, t_max +inf, eps 1e-3, relax 1, max_steps 64.
#pragma once
#include "query_math.h"

namespace raycast_math {

constexpr int STATUS_MISS = 0, STATUS_HIT = 1, STATUS_UNDECIDED = 2;         // == DSP_RAYCAST_MISS / _HIT / _UNDECIDED
constexpr int STEP_HIT = 0, STEP_MISS = 1, STEP_ADVANCE = 2, STEP_EXIT = 3;  // decisions of the step rule
constexpr int MAX_STEPS_CAP = 4096;
constexpr float DEFAULT_T_MIN = 0.f, DEFAULT_EPS = 1e-3f, DEFAULT_RELAX = 1.f;
constexpr int DEFAULT_MAX_STEPS = 64;

struct Params {
    float t_min, t_max, eps, relax;
    int max_steps;
};

DSP_QM_HD inline bool finite32(float x) { return (query_math::float_bits(x) & 0x7f800000u) != 0x7f800000u; }

// nullptr, or what is wrong (host only)
inline const char* check(const Params& p) {
    if (!(p.t_min >= 0.f) || !finite32(p.t_min)) return "raycast: t_min must be finite and >= 0";
    if (!(p.t_max > p.t_min)) return "raycast: t_max must be > t_min";
    if (!(p.eps > 0.f) || !finite32(p.eps)) return "raycast: eps must be finite and > 0";
    if (!(p.relax > 0.f) || !(p.relax <= 1.f)) return "raycast: 0 < relax <= 1";
    if (p.max_steps < 1 || p.max_steps > MAX_STEPS_CAP) return "raycast: 1 <= max_steps <= 4096";
    return nullptr;
}

// u <- the unit direction; false = a void ray (u untouched)
DSP_QM_HD inline bool ray(const float* o, const float* d, float* u) {
    const float n2 = query_math::norm2(d[0], d[1], d[2]);
    if (!finite32(o[0]) || !finite32(o[1]) || !finite32(o[2]) || !finite32(d[0]) || !finite32(d[1]) || !finite32(d[2])) return false;
    if (!(n2 > 0.f) || !finite32(n2)) return false;
    const float len = DSP_QM_SQRT(n2);
    u[0] = DSP_QM_DIV(d[0], len);
    u[1] = DSP_QM_DIV(d[1], len);
    u[2] = DSP_QM_DIV(d[2], len);
    return true;
}

struct Segment {
    float o_o[3], d_o[3], t0, t1;
    bool exists;
};

// tab16: the object's entry of the device table (query_math::OBJ_STRIDE floats: rt[12], s, s_sel, 0, 0)
DSP_QM_HD inline Segment segment(const float* tab16, const float* o, const float* u, float t_min, float t_max) {
    Segment g;
    query_math::to_object(tab16, o[0], o[1], o[2], g.o_o);
#pragma unroll
    for (int i = 0; i < 3; ++i) g.d_o[i] = fmaf(tab16[4 * i + 2], u[2], fmaf(tab16[4 * i + 1], u[1], DSP_QM_MUL(tab16[4 * i], u[0])));
    const float a = query_math::norm2(g.d_o[0], g.d_o[1], g.d_o[2]);
    const float b = DSP_QM_ADD(DSP_QM_ADD(DSP_QM_MUL(g.o_o[0], g.d_o[0]), DSP_QM_MUL(g.o_o[1], g.d_o[1])), DSP_QM_MUL(g.o_o[2], g.d_o[2]));
    const float c = DSP_QM_SUB(query_math::norm2(g.o_o[0], g.o_o[1], g.o_o[2]), 1.f);
    const float disc = fmaf(b, b, -DSP_QM_MUL(a, c));
    const float q = DSP_QM_SQRT(disc);
    const float t_in = DSP_QM_DIV(DSP_QM_SUB(-b, q), a), t_out = DSP_QM_DIV(DSP_QM_SUB(q, b), a);
    const float s_sel = tab16[13];
    g.exists = disc > 0.f && t_out > t_min && t_in < t_max && s_sel == s_sel;
    g.t0 = t_in > t_min ? t_in : t_min;
    g.t1 = t_out < t_max ? t_out : t_max;
    return g;
}

DSP_QM_HD inline void sample(const float* o_o, const float* d_o, float t, float* p) {
    p[0] = fmaf(t, d_o[0], o_o[0]);
    p[1] = fmaf(t, d_o[1], o_o[1]);
    p[2] = fmaf(t, d_o[2], o_o[2]);
}

// -> STEP_*; *dist = sdf s; *t_next = t' (ADVANCE, EXIT), otherwise t
DSP_QM_HD inline int step(float t, float t1, float sdf, float s, float eps, float relax, float* dist, float* t_next) {
    const float d = query_math::distance(sdf, s);
    *dist = d;
    *t_next = t;
    if (d != d) return STEP_MISS;
    if (d <= eps) return STEP_HIT;
    const float tn = fmaf(relax, d, t);
    *t_next = tn;
    return tn > t1 ? STEP_EXIT : STEP_ADVANCE;
}

// a ray's status from its best key and the smallest orderable(t) of its exhausted pairs (0xffffffff: none)
DSP_QM_HD inline int status(uint64_t best, uint32_t exhausted) {
    const uint32_t hi = (uint32_t)(best >> 32);
    if (hi == 0xffffffffu) return exhausted != 0xffffffffu ? STATUS_UNDECIDED : STATUS_MISS;
    return exhausted < hi ? STATUS_UNDECIDED : STATUS_HIT;
}

}  // namespace raycast_math
