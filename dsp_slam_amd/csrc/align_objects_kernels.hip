// Object refinement kernels (dsp_map_align_objects): the Gauss-Newton sums of the map alignment SEGMENTED by the object a ray sees.  The
// arithmetic is align_objects_math.h (rows and tree: align_math.h).  Compiled with contraction off (build.py).
//
// Behind the cast's winner count (raycast_core), wave_base[obj][wave] is the exclusive scan of the winners per (object, wave of rays) and
// the host holds the objects' totals, so a ray's position in its object's list is wave_base[obj][wave] + its rank among the wave's lanes
// that see the same object: nothing is sorted.  k_align_objects_list writes the lists; k_align_objects_gram sums one block of BLOCK list
// positions of one object by the tree's first two levels; k_align_objects_reduce adds an object's blocks in ascending order.  The block
// table comes from the host (from the totals), so the tree is a function of the lists alone.  No float atomics.
#include "dsp_internal.h"
#include "align_objects_math.h"

#include <vector>

namespace dsp {

namespace {

constexpr int AO_BLOCK = align_math::BLOCK;
constexpr int AO_WAVE = align_math::WAVE;
constexpr int AO_WAVES = AO_BLOCK / AO_WAVE;
constexpr int NSUM = align_math::NSUM;
static_assert(AO_WAVE == 64, "a wave of the summation tree is a hardware wave");

// One thread per ray i of [0, n): win_ray[off[k] + j] = i for the j-th winner (ascending ray order) of object k = obj[i].  The wave loops
// over the distinct objects its lanes see.  off: the exclusive scan of the objects' winner totals; n_list: their sum (the list's length).
__global__ __launch_bounds__(AO_BLOCK) void k_align_objects_list(const int* __restrict__ obj, int n, int n_obj, int n_waves,
                                                                 const int* __restrict__ wave_base, const int* __restrict__ off, int n_list,
                                                                 int* __restrict__ win_ray) {
    const int i = blockIdx.x * AO_BLOCK + threadIdx.x;
    const int wave = i / AO_WAVE, lane = threadIdx.x & (AO_WAVE - 1);
    int mine = i < n ? obj[i] : -1;
    if (mine >= n_obj) mine = -1;
    unsigned long long todo = __ballot(mine >= 0);      // uniform over the wave
    while (todo) {
        const int k = __shfl(mine, __ffsll(todo) - 1, AO_WAVE);
        const unsigned long long m = __ballot(mine == k);
        if (mine == k) {
            const long long pos = (long long)off[k] + wave_base[(size_t)k * n_waves + wave] + __popcll(m & ((1ull << lane) - 1ull));
            if (pos >= 0 && pos < n_list) win_ray[pos] = i;
        }
        todo &= ~m;
    }
}

// Block q of the table {object, first list position, positions (1 .. BLOCK), 0}: the terms of these winners, summed by the tree's first two
// levels into slab[q][NSUM].  obj_row / d_row / grad_w per RAY (k_align_rays_residual, k_align_rays_gradient); weights null = ones.
__global__ __launch_bounds__(AO_BLOCK) void k_align_objects_gram(const int4* __restrict__ blocks, const int* __restrict__ win_ray, int n_list, int n_rays,
                                                                 const float* __restrict__ pts_w, const int* __restrict__ obj_row,
                                                                 const float* __restrict__ d_row, const float* __restrict__ grad_w,
                                                                 const float* __restrict__ weights, double huber, double max_dist,
                                                                 double* __restrict__ slab) {
    __shared__ double sh[AO_WAVES][NSUM];
    const int4 blk = blocks[blockIdx.x];
    const int wave = threadIdx.x / AO_WAVE, lane = threadIdx.x & (AO_WAVE - 1);
    double term[NSUM];
    const long long pos = (long long)blk.y + threadIdx.x;
    int ray = -1;
    if ((int)threadIdx.x < blk.z && pos >= 0 && pos < n_list) ray = win_ray[pos];
    if (ray >= 0 && ray < n_rays) {
        const size_t r = (size_t)ray;
        const float pw[3] = {pts_w[3 * r], pts_w[3 * r + 1], pts_w[3 * r + 2]};
        const int o = obj_row[r];
        float g[3] = {0.f, 0.f, 0.f};
        if (o >= 0) { g[0] = grad_w[3 * r]; g[1] = grad_w[3 * r + 1]; g[2] = grad_w[3 * r + 2]; }
        align_math::row_terms(pw, o, d_row[r], g, weights ? weights[r] : 1.f, huber, max_dist, term);
    } else {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) term[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < NSUM; ++k) {
        double v = term[k];
#pragma unroll
        for (int m = AO_WAVE / 2; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, AO_WAVE);
        if (lane == 0) sh[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NSUM) {
        double s = sh[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < AO_WAVES; ++w) s = s + sh[w][threadIdx.x];
        slab[(size_t)blockIdx.x * NSUM + threadIdx.x] = s;
    }
}

// One wave per object k: sums[k][.] = its blocks' slabs [first[k], first[k + 1]) added in ascending order (thread = sum index); zero for an
// object without a block (no winner, or not evaluated).
__global__ __launch_bounds__(AO_WAVE) void k_align_objects_reduce(const double* __restrict__ slab, const int* __restrict__ first, int n_blocks,
                                                                  double* __restrict__ sums) {
    const int k = blockIdx.x;
    if ((int)threadIdx.x >= NSUM) return;
    const int b0 = first[k], b1 = first[k + 1];
    double s = 0.0;
    if (b0 < b1 && b0 >= 0 && b1 <= n_blocks) {
        s = slab[(size_t)b0 * NSUM + threadIdx.x];
        for (int b = b0 + 1; b < b1; ++b) s = s + slab[(size_t)b * NSUM + threadIdx.x];
    }
    sums[(size_t)k * NSUM + threadIdx.x] = s;
}

inline int ao_blocks_for(long long n) { return (int)((n + AO_BLOCK - 1) / AO_BLOCK); }

}  // namespace

hipError_t launch_align_objects_list(const int* obj, int n_rays, int n_obj, int n_waves, const int* wave_base, const int* off, int n_list, int* win_ray,
                                     hipStream_t s) {
    if (n_rays <= 0 || n_obj <= 0 || n_list <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_align_objects_list, dim3(ao_blocks_for(n_rays)), dim3(AO_BLOCK), 0, s, obj, n_rays, n_obj, n_waves, wave_base, off, n_list, win_ray);
    return hipGetLastError();
}

hipError_t launch_align_objects_gram(const int4* blocks, int n_blocks, const int* first, int n_obj, const int* win_ray, int n_list, int n_rays,
                                     const float* pts_w, const int* obj_row, const float* d_row, const float* grad_w, const float* weights, double huber,
                                     double max_dist, double* slab, double* sums, hipStream_t s) {
    if (n_obj <= 0) return hipSuccess;
    if (n_blocks > 0)
        hipLaunchKernelGGL(k_align_objects_gram, dim3(n_blocks), dim3(AO_BLOCK), 0, s, blocks, win_ray, n_list, n_rays, pts_w, obj_row, d_row, grad_w, weights,
                           huber, max_dist, slab);
    hipLaunchKernelGGL(k_align_objects_reduce, dim3(n_obj), dim3(AO_WAVE), 0, s, slab, first, n_blocks, sums);
    return hipGetLastError();
}

// align_objects_math.h compiled for the host in this translation unit, which has contraction off (dsp_map_align_objects' poses and
// directions, dsp_debug_align_objects_*)
void align_objects_compose_host(const double* c16, const float* t16, float* out16) { align_objects_math::compose(c16, t16, out16); }

void align_objects_directions_host(int64_t n, const float* org_w, const float* pts_w, float* dir_w) {
    for (int64_t i = 0; i < n; ++i) align_rays_math::direction(org_w + 3 * i, pts_w + 3 * i, dir_w + 3 * i);
}

void align_objects_rows_host(int64_t n, const float* pts_w, const int32_t* winner, const int32_t* obj_row, const float* d_row, const float* grad_w,
                             const float* weights, int64_t n_obj, double huber, double max_dist, double* sums) {
    std::vector<int64_t> first((size_t)n_obj + 1, 0), list;
    for (int64_t i = 0; i < n; ++i)
        if (winner[i] >= 0 && winner[i] < n_obj) first[(size_t)winner[i] + 1] += 1;
    for (int64_t k = 0; k < n_obj; ++k) first[(size_t)k + 1] += first[(size_t)k];
    list.resize((size_t)first[(size_t)n_obj]);
    std::vector<int64_t> fill(first.begin(), first.end() - 1);
    for (int64_t i = 0; i < n; ++i)
        if (winner[i] >= 0 && winner[i] < n_obj) list[(size_t)fill[(size_t)winner[i]]++] = i;
    std::vector<double> terms;
    for (int64_t k = 0; k < n_obj; ++k) {
        const int64_t m = first[(size_t)k + 1] - first[(size_t)k];
        terms.resize((size_t)m * NSUM);
        for (int64_t j = 0; j < m; ++j) {
            const int64_t i = list[(size_t)(first[(size_t)k] + j)];
            align_math::row_terms(pts_w + 3 * i, obj_row[i], d_row[i], grad_w + 3 * i, weights ? weights[i] : 1.f, huber, max_dist,
                                  terms.data() + (size_t)j * NSUM);
        }
        double* s = sums + (size_t)k * NSUM;
        align_math::tree_sum(m, terms.data(), s);
        for (int q = 0; q < 6; ++q) s[align_math::IDX_B + q] = -s[align_math::IDX_B + q];
    }
}

}  // namespace dsp
