// Shape refinement kernels (dsp_map_align_shapes): the 70-dimensional Gauss-Newton sums of the map's objects against depth rays, SEGMENTED
// by the object a ray sees.  The arithmetic is align_shapes_math.h.  Compiled with contraction off (build.py).
//
// k_align_shapes_rows stands behind every chunk of the cast's winner rows (next to k_align_rays_gradient) and keeps what that kernel drops:
// the 64 code derivatives of the jacobian row, times the winner's scale, in a per-RAY buffer gcode[n_rays][64].  The chunks end there: the
// kernels below read per-ray arrays only.  k_align_shapes_gram takes one block of BLOCK positions of one object's list (the list and the
// block table are dsp_map_align_objects': k_align_objects_list, the host's totals): it builds the block's rows in LDS, then every thread
// owns a few of the 2558 sums and walks the rows in ascending order with fp64 adds.  k_align_shapes_reduce adds an object's blocks in
// ascending order.  No float atomics, no matrix instructions: the order of every sum is the header's.
#include "dsp_internal.h"
#include "align_shapes_math.h"

#include <vector>

namespace dsp {

namespace {

namespace sm = align_shapes_math;
constexpr int AS_BLOCK = sm::BLOCK;         // rows of a block
constexpr int AS_THREADS = 256;             // threads of the gram kernel: more than rows, so that a thread owns fewer sums
constexpr int AS_OWN = (sm::NSUM + AS_THREADS - 1) / AS_THREADS;
constexpr int AS_VEC = sm::CODE / 4;        // float4 per row of gcode
constexpr int NSUM = sm::NSUM;
static_assert(AS_THREADS >= AS_BLOCK && sm::CODE % 4 == 0 && (sm::ROW_F & 1) == 1, "one thread per row in the staging; an odd row stride in LDS");
static_assert((GRAD_STRIDE * 4) % 16 == 0 && CODE_LEN == sm::CODE, "a jacobian row starts 16-byte aligned with the code derivatives first");

// One thread per float4 of the code derivatives of a winner's jacobian row {ray, object}: gcode[ray][.] <- row[0 .. 63] s  (s: the winner's
// scale, one fp32 multiply).  16 consecutive threads move one row: 256 B in, 256 B out, both contiguous.
__global__ __launch_bounds__(256) void k_align_shapes_rows(const float* __restrict__ rows, const int2* __restrict__ row_meta, int n_rows,
                                                           const float4* __restrict__ tab, int n_obj, long long n_rays, float* __restrict__ gcode) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long r = t / AS_VEC;
    const int q = (int)(t % AS_VEC);
    if (r >= n_rows) return;
    const int2 m = row_meta[r];
    if (m.x < 0 || m.x >= n_rays || m.y < 0 || m.y >= n_obj) return;
    const float s = tab[4 * (size_t)m.y + 3].x;
    float4 v = *reinterpret_cast<const float4*>(rows + (size_t)r * GRAD_STRIDE + 4 * q);
    v.x = DSP_QM_MUL(v.x, s); v.y = DSP_QM_MUL(v.y, s); v.z = DSP_QM_MUL(v.z, s); v.w = DSP_QM_MUL(v.w, s);
    *reinterpret_cast<float4*>(gcode + (size_t)m.x * sm::CODE + 4 * q) = v;
}

// Block q of the table {object, first list position, positions (1 .. BLOCK), 0}: slab[q][NSUM] <- the block's sums.  obj_row / d_row /
// grad_w / gcode per RAY; weights null = ones.
__global__ __launch_bounds__(AS_THREADS) void k_align_shapes_gram(const int4* __restrict__ blocks, const int* __restrict__ win_ray, int n_list, int n_rays,
                                                                  const float* __restrict__ pts_w, const int* __restrict__ obj_row,
                                                                  const float* __restrict__ d_row, const float* __restrict__ grad_w,
                                                                  const float* __restrict__ gcode, const float* __restrict__ weights, double huber,
                                                                  double max_dist, double* __restrict__ slab) {
    __shared__ float jf[AS_BLOCK * sm::ROW_F];
    __shared__ double jd[AS_BLOCK * sm::ROW_D];
    __shared__ int sray[AS_BLOCK];
    const int4 blk = blocks[blockIdx.x];
    const int tid = threadIdx.x;
    const int n_rows = blk.z < AS_BLOCK ? (blk.z > 0 ? blk.z : 0) : AS_BLOCK;
    // the rays of the block's rows
    if (tid < AS_BLOCK) {
        const long long pos = (long long)blk.y + tid;
        int ray = -1;
        if (tid < n_rows && pos >= 0 && pos < n_list) ray = win_ray[pos];
        sray[tid] = (ray >= 0 && ray < n_rays) ? ray : -1;
    }
    __syncthreads();
    // gcode of every row into its place of the row, 16 threads per row
    for (int k = tid; k < n_rows * AS_VEC; k += AS_THREADS) {
        const int row = k / AS_VEC, q = k % AS_VEC;
        const int ray = sray[row];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ray >= 0) v = *reinterpret_cast<const float4*>(gcode + (size_t)ray * sm::CODE + 4 * q);
        float* dst = jf + row * sm::ROW_F + 3 + 4 * q;
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
    __syncthreads();
    // one thread per row: the rest of the row
    if (tid < n_rows) {
        const int ray = sray[tid];
        float pw[3] = {0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f}, dist = 0.f, w = 0.f;      // w = 0: a position without a ray is not valid
        int o = -1;
        if (ray >= 0) {
            const size_t r = (size_t)ray;
            pw[0] = pts_w[3 * r]; pw[1] = pts_w[3 * r + 1]; pw[2] = pts_w[3 * r + 2];
            o = obj_row[r];
            if (o >= 0) { g[0] = grad_w[3 * r]; g[1] = grad_w[3 * r + 1]; g[2] = grad_w[3 * r + 2]; }
            dist = d_row[r];
            w = weights ? weights[r] : 1.f;
        }
        sm::build_row(pw, o, dist, g, w, huber, max_dist, jf + tid * sm::ROW_F, jd + tid * sm::ROW_D);
    }
    __syncthreads();
    // every thread owns the sums tid, tid + AS_THREADS, ..: the rows in ascending order, one add at a time
    int pi[AS_OWN], pj[AS_OWN];
    double acc[AS_OWN];
#pragma unroll
    for (int m = 0; m < AS_OWN; ++m) {
        const int q = tid + m * AS_THREADS;
        pi[m] = sm::EXTRA; pj[m] = 0;
        if (q < NSUM) sm::pair_of(q, &pi[m], &pj[m]);
        acc[m] = 0.0;
    }
    for (int r = 0; r < n_rows; ++r) {
        const float* f = jf + r * sm::ROW_F;
        const double* d = jd + r * sm::ROW_D;
#pragma unroll
        for (int m = 0; m < AS_OWN; ++m) acc[m] = acc[m] + sm::term_of(f, d, pi[m], pj[m]);
    }
#pragma unroll
    for (int m = 0; m < AS_OWN; ++m) {
        const int q = tid + m * AS_THREADS;
        if (q < NSUM) slab[(size_t)blockIdx.x * NSUM + q] = acc[m];
    }
}

// One workgroup per object k, a thread per sum: sums[k][.] = its blocks' slabs [first[k], first[k + 1]) added in ascending order; zero
// for an object without a block (no winner, or not evaluated).
__global__ __launch_bounds__(AS_THREADS) void k_align_shapes_reduce(const double* __restrict__ slab, const int* __restrict__ first, int n_blocks,
                                                                    double* __restrict__ sums) {
    const int k = blockIdx.x;
    const int b0 = first[k], b1 = first[k + 1];
    const bool any = b0 < b1 && b0 >= 0 && b1 <= n_blocks;
    for (int q = threadIdx.x; q < NSUM; q += AS_THREADS) {
        double s = 0.0;
        if (any) {
            s = slab[(size_t)b0 * NSUM + q];
            for (int b = b0 + 1; b < b1; ++b) s = s + slab[(size_t)b * NSUM + q];
        }
        sums[(size_t)k * NSUM + q] = s;
    }
}

}  // namespace

hipError_t launch_align_shapes_rows(const float* rows, const int2* row_meta, int n_rows, const float* tab, int n_obj, int64_t n_rays, float* gcode,
                                    hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    const long long threads = (long long)n_rows * AS_VEC;
    hipLaunchKernelGGL(k_align_shapes_rows, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, rows, row_meta, n_rows,
                       reinterpret_cast<const float4*>(tab), n_obj, (long long)n_rays, gcode);
    return hipGetLastError();
}

hipError_t launch_align_shapes_gram(const int4* blocks, int n_blocks, const int* first, int n_obj, const int* win_ray, int n_list, int n_rays,
                                    const float* pts_w, const int* obj_row, const float* d_row, const float* grad_w, const float* gcode,
                                    const float* weights, double huber, double max_dist, double* slab, double* sums, hipStream_t s) {
    if (n_obj <= 0) return hipSuccess;
    if (n_blocks > 0)
        hipLaunchKernelGGL(k_align_shapes_gram, dim3(n_blocks), dim3(AS_THREADS), 0, s, blocks, win_ray, n_list, n_rays, pts_w, obj_row, d_row, grad_w, gcode,
                           weights, huber, max_dist, slab);
    hipLaunchKernelGGL(k_align_shapes_reduce, dim3(n_obj), dim3(AS_THREADS), 0, s, slab, first, n_blocks, sums);
    return hipGetLastError();
}

// align_shapes_math.h compiled for the host in this translation unit, which has contraction off (dsp_map_align_shapes' step and cost,
// dsp_debug_align_shapes_*)
void align_shapes_rows_host(int64_t n, const float* pts_w, const int32_t* winner, const int32_t* obj_row, const float* d_row, const float* grad_w,
                            const float* gcode, const float* weights, int64_t n_obj, double huber, double max_dist, double* sums) {
    std::vector<std::vector<int64_t>> lists((size_t)n_obj);
    for (int64_t i = 0; i < n; ++i)
        if (winner[i] >= 0 && winner[i] < n_obj) lists[(size_t)winner[i]].push_back(i);
    std::vector<float> jf;
    std::vector<double> jd;
    const float zero3[3] = {0.f, 0.f, 0.f};
    for (int64_t k = 0; k < n_obj; ++k) {
        const std::vector<int64_t>& list = lists[(size_t)k];
        jf.assign(list.size() * sm::ROW_F, 0.f);
        jd.assign(list.size() * sm::ROW_D, 0.0);
        for (size_t j = 0; j < list.size(); ++j) {
            const int64_t i = list[j];
            float* f = jf.data() + j * sm::ROW_F;
            memcpy(f + 3, gcode + (size_t)i * sm::CODE, sm::CODE * sizeof(float));
            sm::build_row(pts_w + 3 * i, obj_row[i], d_row[i], obj_row[i] >= 0 ? grad_w + 3 * i : zero3, weights ? weights[i] : 1.f, huber, max_dist, f,
                          jd.data() + j * sm::ROW_D);
        }
        sm::block_sums((int64_t)list.size(), jf.data(), jd.data(), sums + (size_t)k * NSUM);
    }
}

double align_shapes_mean_cost_host(const double* sums, double huber, double max_dist) { return sm::mean_cost(sums, huber, max_dist); }

double align_shapes_cost_host(double mean, const double* z, const double* z0, int code_len, double code_reg, double code_anchor) {
    return sm::cost_of(mean, z, z0, code_len, code_reg, code_anchor);
}

bool align_shapes_solve_host(const double* H, const double* b, double W, const double* z, const double* z0, int code_len, int unknowns, double code_reg,
                             double code_anchor, double damp, double lambda, double* dx) {
    return sm::solve(H, b, W, z, z0, code_len, unknowns, code_reg, code_anchor, damp, lambda, dx);
}

void align_shapes_apply_step_host(const double* dx, int unknowns, int code_len, const double* c_in, const double* z_in, double* c_out, double* z_out) {
    sm::apply_step(dx, unknowns, code_len, c_in, z_in, c_out, z_out);
}

}  // namespace dsp
