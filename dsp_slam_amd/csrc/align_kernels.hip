// Map alignment kernels (dsp_map_align): what stands around the map query's pipeline (query_kernels.hip) in one evaluation of every
// hypothesis -- sensor points to world points in front of it, the winner's world gradient behind each chunk's reduce, and the fixed-tree
// fp64 sums of the 6 x 6 system behind its finish.  The arithmetic is align_math.h.  Compiled with contraction off (build.py), like every
// file that restates a formula operation by operation.
//
// No float atomics: a hypothesis' sums are one written tree (align_math.h "Summation") -- a butterfly inside each wave, the block's waves
// added in ascending order through LDS, the blocks' slabs added in ascending order by k_align_gram_reduce.  The slabs are combined in a
// second kernel and not by the last block to arrive: the combine would need a counter and a fence per hypothesis, and the kernel behind it
// exists anyway as the producer of the one array the host reads back.
//
// Ray alignment (dsp_map_align_rays; the arithmetic: align_rays_math.h) puts the ray caster's pipeline (raycast_kernels.hip) where the map
// query stands: k_align_rays_build makes the world rays of every hypothesis in front of the cast, k_align_rays_gradient writes the winners'
// world gradients behind each chunk of their jacobian rows, and k_align_rays_residual turns the cast's answers into the (obj, dist) that
// k_align_gram reads.  Plain per-row kernels, no atomics.
#include "dsp_internal.h"
#include "align_math.h"
#include "align_rays_math.h"

#include <vector>

namespace dsp {

namespace {

constexpr int ALIGN_BLOCK = align_math::BLOCK;
constexpr int ALIGN_WAVE = align_math::WAVE;
constexpr int ALIGN_WAVES = ALIGN_BLOCK / ALIGN_WAVE;
constexpr int NSUM = align_math::NSUM;
static_assert(ALIGN_WAVE == 64, "a wave of the summation tree is a hardware wave");

// One thread per row r = h n_pts + i of [r0, r0 + n): world point of sensor point i under hypothesis h.  hyp: ALIGN_HYP_STRIDE floats per
// hypothesis {rt[12], live, 0, 0, 0}; a hypothesis that has ended (live == 0) gets NaN points, which are inside no sphere.
__global__ __launch_bounds__(ALIGN_BLOCK) void k_align_transform(const float* __restrict__ pts_s, long long n_pts, const float4* __restrict__ hyp,
                                                                 long long r0, long long n, float* __restrict__ pts_w) {
    const long long k = (long long)blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    if (k >= n) return;
    const long long r = r0 + k;
    const long long h = r / n_pts, i = r - h * n_pts;
    const float4 a0 = hyp[4 * h], a1 = hyp[4 * h + 1], a2 = hyp[4 * h + 2], m = hyp[4 * h + 3];
    float p[3];
    if (m.x != 0.f) {
        const float rt[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
        query_math::to_object(rt, pts_s[3 * i], pts_s[3 * i + 1], pts_s[3 * i + 2], p);
    } else {
        p[0] = p[1] = p[2] = __uint_as_float(0x7fc00000u);
    }
    pts_w[3 * r] = p[0]; pts_w[3 * r + 1] = p[1]; pts_w[3 * r + 2] = p[2];
}

// The sibling of k_query_winner, behind the chunk's reduce: the row whose key is its point's best so far writes the world gradient of
// d = sdf s.  Keys are unique per (point, object), so one row writes; a later chunk's smaller key writes over it.
__global__ __launch_bounds__(ALIGN_BLOCK) void k_align_winner(const float* __restrict__ rows, const int2* __restrict__ row_meta, int n_rows,
                                                              const float4* __restrict__ tab, int n_obj, long long n_pts,
                                                              const unsigned long long* __restrict__ best, float* __restrict__ grad_w) {
    const int r = blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int2 m = row_meta[r];
    if (m.x < 0 || m.x >= n_pts || m.y < 0 || m.y >= n_obj) return;
    const float4 t = *reinterpret_cast<const float4*>(rows + (size_t)r * GRAD_STRIDE + CODE_LEN);     // {gx, gy, gz, sdf}
    const float4 r0 = tab[4 * (size_t)m.y], r1 = tab[4 * (size_t)m.y + 1], r2 = tab[4 * (size_t)m.y + 2], q = tab[4 * (size_t)m.y + 3];
    if ((unsigned long long)query_math::key(query_math::distance(t.w, q.y), m.y) != best[m.x]) return;
    const float rt[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
    float gw[3];
    align_math::world_gradient(rt, q.x, t.x, t.y, t.z, gw);
    grad_w[3 * (size_t)m.x] = gw[0]; grad_w[3 * (size_t)m.x + 1] = gw[1]; grad_w[3 * (size_t)m.x + 2] = gw[2];
}

// Block (b, h): the terms of points [b BLOCK, (b + 1) BLOCK) of hypothesis h, summed by the tree's first two levels into slab[h][b][NSUM].
// An ended hypothesis is skipped.  weights null = ones.
__global__ __launch_bounds__(ALIGN_BLOCK) void k_align_gram(const float* __restrict__ pts_w, const int* __restrict__ obj, const float* __restrict__ dist,
                                                            const float* __restrict__ grad_w, const float* __restrict__ weights, long long n_pts,
                                                            const float4* __restrict__ hyp, double huber, double max_dist, int n_blocks,
                                                            double* __restrict__ slab) {
    __shared__ double sh[ALIGN_WAVES][NSUM];
    const int h = blockIdx.y;
    if (hyp[4 * (size_t)h + 3].x == 0.f) return;                      // uniform over the block
    const long long i = (long long)blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    const int wave = threadIdx.x / ALIGN_WAVE, lane = threadIdx.x & (ALIGN_WAVE - 1);
    double term[NSUM];
    if (i < n_pts) {
        const size_t r = (size_t)h * (size_t)n_pts + (size_t)i;
        const float pw[3] = {pts_w[3 * r], pts_w[3 * r + 1], pts_w[3 * r + 2]};
        const int o = obj[r];
        float g[3] = {0.f, 0.f, 0.f};
        if (o >= 0) { g[0] = grad_w[3 * r]; g[1] = grad_w[3 * r + 1]; g[2] = grad_w[3 * r + 2]; }
        align_math::row_terms(pw, o, dist[r], g, weights ? weights[i] : 1.f, huber, max_dist, term);
    } else {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) term[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < NSUM; ++k) {
        double v = term[k];
#pragma unroll
        for (int m = ALIGN_WAVE / 2; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, ALIGN_WAVE);
        if (lane == 0) sh[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NSUM) {
        double s = sh[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < ALIGN_WAVES; ++w) s = s + sh[w][threadIdx.x];
        slab[((size_t)h * n_blocks + blockIdx.x) * NSUM + threadIdx.x] = s;
    }
}

// Block h: sums[h][k] = slab[h][0][k] + slab[h][1][k] + ... in ascending order (thread k).  An ended hypothesis is skipped.
__global__ __launch_bounds__(ALIGN_WAVE) void k_align_gram_reduce(const double* __restrict__ slab, int n_blocks, const float4* __restrict__ hyp,
                                                                  double* __restrict__ sums) {
    const int h = blockIdx.x;
    if (hyp[4 * (size_t)h + 3].x == 0.f || (int)threadIdx.x >= NSUM) return;
    const double* p = slab + (size_t)h * n_blocks * NSUM + threadIdx.x;
    double s = p[0];
    for (int b = 1; b < n_blocks; ++b) s = s + p[(size_t)b * NSUM];
    sums[(size_t)h * NSUM + threadIdx.x] = s;
}

// Ray alignment.  One thread per row r = h n_rays + i of [0, n): the world end point, origin and direction of observation i under hypothesis
// h.  org_s null = the sensor origin.  An ended hypothesis gets NaN: its rays are void and pair with nothing.
__global__ __launch_bounds__(ALIGN_BLOCK) void k_align_rays_build(const float* __restrict__ pts_s, const float* __restrict__ org_s, long long n_rays,
                                                                  const float4* __restrict__ hyp, long long n, float* __restrict__ pts_w,
                                                                  float* __restrict__ org_w, float* __restrict__ dir_w) {
    const long long r = (long long)blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    if (r >= n) return;
    const long long h = r / n_rays, i = r - h * n_rays;
    const float4 a0 = hyp[4 * h], a1 = hyp[4 * h + 1], a2 = hyp[4 * h + 2], m = hyp[4 * h + 3];
    float p[3], o[3], d[3];
    if (m.x != 0.f) {
        const float rt[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
        query_math::to_object(rt, pts_s[3 * i], pts_s[3 * i + 1], pts_s[3 * i + 2], p);
        if (org_s) query_math::to_object(rt, org_s[3 * i], org_s[3 * i + 1], org_s[3 * i + 2], o);
        else query_math::to_object(rt, 0.f, 0.f, 0.f, o);
    } else {
        p[0] = p[1] = p[2] = o[0] = o[1] = o[2] = __uint_as_float(0x7fc00000u);
    }
    align_rays_math::direction(o, p, d);
    pts_w[3 * r] = p[0]; pts_w[3 * r + 1] = p[1]; pts_w[3 * r + 2] = p[2];
    org_w[3 * r] = o[0]; org_w[3 * r + 1] = o[1]; org_w[3 * r + 2] = o[2];
    dir_w[3 * r] = d[0]; dir_w[3 * r + 1] = d[1]; dir_w[3 * r + 2] = d[2];
}

// The sibling of k_raycast_normal: one thread per jacobian row of a winner {ray, object}, its world gradient (not normalised)
__global__ __launch_bounds__(ALIGN_BLOCK) void k_align_rays_gradient(const float* __restrict__ rows, const int2* __restrict__ row_meta, int n_rows,
                                                                     const float4* __restrict__ tab, int n_obj, long long n_rays,
                                                                     float* __restrict__ grad_w) {
    const int r = blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int2 m = row_meta[r];
    if (m.x < 0 || m.x >= n_rays || m.y < 0 || m.y >= n_obj) return;
    const float4 t = *reinterpret_cast<const float4*>(rows + (size_t)r * GRAD_STRIDE + CODE_LEN);     // {gx, gy, gz, sdf}
    const float4 r0 = tab[4 * (size_t)m.y], r1 = tab[4 * (size_t)m.y + 1], r2 = tab[4 * (size_t)m.y + 2], q = tab[4 * (size_t)m.y + 3];
    const float rt[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
    float gw[3];
    align_math::world_gradient(rt, q.x, t.x, t.y, t.z, gw);
    grad_w[3 * (size_t)m.x] = gw[0]; grad_w[3 * (size_t)m.x + 1] = gw[1]; grad_w[3 * (size_t)m.x + 2] = gw[2];
}

// One thread per row of [0, n): the cast's answers -> the row's first-order signed distance and the object it is matched to (-1: unmatched)
__global__ __launch_bounds__(ALIGN_BLOCK) void k_align_rays_residual(const float* __restrict__ org_w, const float* __restrict__ dir_w,
                                                                     const int* __restrict__ obj, const float* __restrict__ t_hit,
                                                                     const float* __restrict__ dist_hit, const int* __restrict__ status,
                                                                     const float* __restrict__ grad_w, long long n, double max_gap,
                                                                     int* __restrict__ obj_row, float* __restrict__ d_row) {
    const long long r = (long long)blockIdx.x * ALIGN_BLOCK + threadIdx.x;
    if (r >= n) return;
    const float o[3] = {org_w[3 * r], org_w[3 * r + 1], org_w[3 * r + 2]}, dir[3] = {dir_w[3 * r], dir_w[3 * r + 1], dir_w[3 * r + 2]};
    float u[3] = {0.f, 0.f, 0.f}, len = 0.f, g[3] = {0.f, 0.f, 0.f}, d;
    const bool ok = align_rays_math::ray(o, dir, u, &len);
    const int w = obj[r];
    if (ok && w >= 0) { g[0] = grad_w[3 * r]; g[1] = grad_w[3 * r + 1]; g[2] = grad_w[3 * r + 2]; }
    obj_row[r] = align_rays_math::residual(ok, u, len, w, t_hit[r], dist_hit[r], status[r], g, max_gap, &d);
    d_row[r] = d;
}

inline int blocks_for(long long n) { return (int)((n + ALIGN_BLOCK - 1) / ALIGN_BLOCK); }

}  // namespace

hipError_t launch_align_transform(const float* pts_s, int64_t n_pts, const float* hyp, int64_t r0, int64_t n, float* pts_w, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_align_transform, dim3(blocks_for(n)), dim3(ALIGN_BLOCK), 0, s, pts_s, (long long)n_pts, reinterpret_cast<const float4*>(hyp),
                       (long long)r0, (long long)n, pts_w);
    return hipGetLastError();
}

hipError_t launch_align_winner(const float* rows, const int2* row_meta, int n_rows, const float* tab, int n_obj, int64_t n_pts,
                               const unsigned long long* best, float* grad_w, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_align_winner, dim3(blocks_for(n_rows)), dim3(ALIGN_BLOCK), 0, s, rows, row_meta, n_rows, reinterpret_cast<const float4*>(tab), n_obj,
                       (long long)n_pts, best, grad_w);
    return hipGetLastError();
}

hipError_t launch_align_gram(const float* pts_w, const int* obj, const float* dist, const float* grad_w, const float* weights, int64_t n_pts, int n_hyp,
                             const float* hyp, double huber, double max_dist, double* slab, double* sums, hipStream_t s) {
    if (n_pts <= 0 || n_hyp <= 0) return hipSuccess;
    const int nb = blocks_for(n_pts);
    const float4* h4 = reinterpret_cast<const float4*>(hyp);
    for (int h0 = 0; h0 < n_hyp; h0 += 65535) {                      // gridDim.y
        const int nh = n_hyp - h0 < 65535 ? n_hyp - h0 : 65535;
        hipLaunchKernelGGL(k_align_gram, dim3(nb, nh), dim3(ALIGN_BLOCK), 0, s, pts_w + 3 * (size_t)h0 * n_pts, obj + (size_t)h0 * n_pts,
                           dist + (size_t)h0 * n_pts, grad_w + 3 * (size_t)h0 * n_pts, weights, (long long)n_pts, h4 + 4 * (size_t)h0, huber, max_dist, nb,
                           slab + (size_t)h0 * nb * NSUM);
    }
    hipLaunchKernelGGL(k_align_gram_reduce, dim3(n_hyp), dim3(ALIGN_WAVE), 0, s, slab, nb, h4, sums);
    return hipGetLastError();
}

hipError_t launch_align_rays_build(const float* pts_s, const float* org_s, int64_t n_rays, const float* hyp, int64_t n, float* pts_w, float* org_w,
                                   float* dir_w, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_align_rays_build, dim3(blocks_for(n)), dim3(ALIGN_BLOCK), 0, s, pts_s, org_s, (long long)n_rays,
                       reinterpret_cast<const float4*>(hyp), (long long)n, pts_w, org_w, dir_w);
    return hipGetLastError();
}

hipError_t launch_align_rays_gradient(const float* rows, const int2* row_meta, int n_rows, const float* tab, int n_obj, int64_t n_rays, float* grad_w,
                                      hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_align_rays_gradient, dim3(blocks_for(n_rows)), dim3(ALIGN_BLOCK), 0, s, rows, row_meta, n_rows,
                       reinterpret_cast<const float4*>(tab), n_obj, (long long)n_rays, grad_w);
    return hipGetLastError();
}

hipError_t launch_align_rays_residual(const float* org_w, const float* dir_w, const int* obj, const float* t_hit, const float* dist_hit, const int* status,
                                      const float* grad_w, int64_t n, double max_gap, int* obj_row, float* d_row, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_align_rays_residual, dim3(blocks_for(n)), dim3(ALIGN_BLOCK), 0, s, org_w, dir_w, obj, t_hit, dist_hit, status, grad_w,
                       (long long)n, max_gap, obj_row, d_row);
    return hipGetLastError();
}

int64_t align_gram_blocks(int64_t n_pts) { return blocks_for(n_pts); }

// align_math.h compiled for the host in this translation unit, which has contraction off (dsp_map_align's step and dsp_debug_align_*)
bool align_check_pose_host(const double* t16, float* rt12) { return align_math::check_pose(t16, rt12); }

void align_rows_host(int64_t n, const float* pts_w, const int32_t* obj, const float* dist, const float* grad_w, const float* weights, double huber,
                     double max_dist, double* sums) {
    std::vector<double> terms((size_t)n * NSUM);
    for (int64_t i = 0; i < n; ++i)
        align_math::row_terms(pts_w + 3 * i, obj[i], dist[i], grad_w + 3 * i, weights ? weights[i] : 1.f, huber, max_dist, terms.data() + (size_t)i * NSUM);
    align_math::tree_sum(n, terms.data(), sums);
}

// align_rays_math.h compiled for the host here as well (dsp_debug_align_ray_rows)
void align_ray_rows_host(int64_t n, const float* org_w, const float* pts_w, const int32_t* obj, const float* t_hit, const float* dist_hit,
                         const int32_t* status, const float* grad_w, const float* weights, double huber, double max_dist, double max_gap,
                         int32_t* obj_row, float* d_row, double* sums) {
    std::vector<double> terms((size_t)n * NSUM);
    for (int64_t i = 0; i < n; ++i) {
        float dir[3], u[3] = {0.f, 0.f, 0.f}, len = 0.f;
        align_rays_math::direction(org_w + 3 * i, pts_w + 3 * i, dir);
        const bool ok = align_rays_math::ray(org_w + 3 * i, dir, u, &len);
        obj_row[i] = align_rays_math::residual(ok, u, len, obj[i], t_hit[i], dist_hit[i], status[i], grad_w + 3 * i, max_gap, d_row + i);
        align_math::row_terms(pts_w + 3 * i, obj_row[i], d_row[i], grad_w + 3 * i, weights ? weights[i] : 1.f, huber, max_dist,
                              terms.data() + (size_t)i * NSUM);
    }
    align_math::tree_sum(n, terms.data(), sums);
}

const char* align_rays_check_gap_host(double max_gap, double max_dist) { return align_rays_math::check_gap(max_gap, max_dist); }

double align_cost_host(const double* sums, double huber, double max_dist) { return align_math::cost_of(sums, huber, max_dist); }

bool align_solve_host(const double* H36, const double* b6, double damp, double lambda, double* xi6) { return align_math::solve(H36, b6, damp, lambda, xi6); }

void align_apply_step_host(const double* xi6, const double* t_in, double* t_out) { align_math::apply_step(xi6, t_in, t_out); }

}  // namespace dsp
