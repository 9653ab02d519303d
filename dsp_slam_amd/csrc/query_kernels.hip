// Map query kernels (dsp_map_query): the front that turns (world points x posed objects) into the decoder's ragged per-object point lists,
// and the back that reduces the decoder's rows to one answer per point.  The decoder work itself is mlp_kernel<0> / mlp_kernel<2>
// (mlp_kernel.hip) as surface_run launches them; the arithmetic is query_math.h.  Compiled with contraction off (build.py), like every file
// that restates a formula operation by operation.
//
// No float atomics: an object's candidates are listed in ascending point order (ballot rank inside a wave + the scanned wave counts), and the
// only atomic is the 64-bit integer minimum on the selection key, whose result does not depend on the order of its operands.
#include "dsp_internal.h"
#include "query_math.h"

#include <vector>

namespace dsp {

namespace {

constexpr int QUERY_BLOCK = 256;
constexpr int QUERY_WAVE = 64;
constexpr int QUERY_LDS_OBJ = 256;      // objects staged in LDS at a time: 256 x 16 floats = 16 KiB
static_assert(query_math::OBJ_STRIDE == 16 && QUERY_LDS_OBJ == QUERY_BLOCK, "one thread stages one object: four float4 loads");
static_assert(QUERY_BLOCK % QUERY_WAVE == 0, "a block is whole waves");

// the block's threads stage objects [o0, o0 + n) of the table (n <= QUERY_LDS_OBJ) in LDS
__device__ __forceinline__ void stage_objects(float4* lds, const float4* __restrict__ tab, int o0, int n) {
    if ((int)threadIdx.x < n) {
#pragma unroll
        for (int q = 0; q < 4; ++q) lds[4 * threadIdx.x + q] = tab[4 * ((size_t)o0 + threadIdx.x) + q];
    }
}

// what both the count and the fill kernel compute for (point, staged object k): p_o, |p_o|^2 -- the same calls, so both decide containment alike
struct Cand { float p[3]; float n2; };
__device__ __forceinline__ Cand candidate(const float4* lds, int k, float x, float y, float z, float* s) {
    const float4 r0 = lds[4 * k], r1 = lds[4 * k + 1], r2 = lds[4 * k + 2], m = lds[4 * k + 3];
    const float rt[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
    Cand c;
    query_math::to_object(rt, x, y, z, c.p);
    c.n2 = query_math::norm2(c.p[0], c.p[1], c.p[2]);
    *s = m.x;
    return c;
}

// One thread per point of the pass (points p0 .. p0 + n of pts3), the wave loops over all objects.  wave_cnt[obj][wave] = contained points of
// the wave; bound[pt] = the running sphere bound; best[pt] = the all-ones key.  n_waves = ceil(n / 64).
__global__ __launch_bounds__(QUERY_BLOCK) void k_query_count(const float* __restrict__ pts3, long long p0, int n, const float4* __restrict__ tab,
                                                             int n_obj, int n_waves, int* __restrict__ wave_cnt, float* __restrict__ bound,
                                                             unsigned long long* __restrict__ best) {
    __shared__ float4 lds[4 * QUERY_LDS_OBJ];
    const int i = blockIdx.x * QUERY_BLOCK + threadIdx.x;
    const bool valid = i < n;
    const int wave = i / QUERY_WAVE, lane = threadIdx.x & (QUERY_WAVE - 1);
    float x = 0.f, y = 0.f, z = 0.f;
    if (valid) {
        const size_t q = 3 * ((size_t)p0 + i);
        x = pts3[q]; y = pts3[q + 1]; z = pts3[q + 2];
    }
    float b = __uint_as_float(0x7f800000u);
    for (int o0 = 0; o0 < n_obj; o0 += QUERY_LDS_OBJ) {
        const int nk = min(QUERY_LDS_OBJ, n_obj - o0);
        __syncthreads();
        stage_objects(lds, tab, o0, nk);
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
            float s;
            const Cand c = candidate(lds, k, x, y, z, &s);
            const bool in = valid && query_math::inside(c.n2);
            if (valid && !in) b = query_math::min_bound(b, query_math::sphere_bound(c.n2, s));
            const unsigned long long m = __ballot(in);
            if (lane == 0 && wave < n_waves) wave_cnt[(size_t)(o0 + k) * n_waves + wave] = __popcll(m);
        }
    }
    if (valid) {
        bound[(size_t)p0 + i] = b;
        best[(size_t)p0 + i] = query_math::NO_KEY;
    }
}

// One block per object: wave_cnt[obj][.] -> its exclusive scan in place (each wave's first row among the object's candidates), cnt[obj] = the total
__global__ __launch_bounds__(QUERY_BLOCK) void k_query_scan(int* __restrict__ wave_cnt, int n_waves, int* __restrict__ cnt) {
    __shared__ int sh[QUERY_BLOCK];
    int* w = wave_cnt + (size_t)blockIdx.x * n_waves;
    int carry = 0;
    for (int base = 0; base < n_waves; base += QUERY_BLOCK) {
        const int j = base + threadIdx.x;
        const int v = j < n_waves ? w[j] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < QUERY_BLOCK; d <<= 1) {
            const int t = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (j < n_waves) w[j] = carry + sh[threadIdx.x] - v;
        carry += sh[QUERY_BLOCK - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt[blockIdx.x] = carry;
}

// The chunk's objects [o0, o0 + nc): candidate j of object o0 + k (ascending point order) has chunk row base[k] + j; the rows inside
// [0, n_rows) are written -- p_o to the decoder's list, {point, object} to row_meta.  base[k] may be negative (the chunk starts inside the object).
__global__ __launch_bounds__(QUERY_BLOCK) void k_query_fill(const float* __restrict__ pts3, long long p0, int n, const float4* __restrict__ tab,
                                                            int o0, int nc, const int* __restrict__ base, int n_waves,
                                                            const int* __restrict__ wave_base, int n_rows, float4* __restrict__ pts4,
                                                            int2* __restrict__ row_meta) {
    __shared__ float4 lds[4 * QUERY_LDS_OBJ];
    __shared__ int lbase[QUERY_LDS_OBJ];
    const int i = blockIdx.x * QUERY_BLOCK + threadIdx.x;
    const bool valid = i < n;
    const int wave = i / QUERY_WAVE, lane = threadIdx.x & (QUERY_WAVE - 1);
    float x = 0.f, y = 0.f, z = 0.f;
    if (valid) {
        const size_t q = 3 * ((size_t)p0 + i);
        x = pts3[q]; y = pts3[q + 1]; z = pts3[q + 2];
    }
    for (int c0 = 0; c0 < nc; c0 += QUERY_LDS_OBJ) {
        const int nk = min(QUERY_LDS_OBJ, nc - c0);
        __syncthreads();
        stage_objects(lds, tab, o0 + c0, nk);
        if ((int)threadIdx.x < nk) lbase[threadIdx.x] = base[c0 + threadIdx.x];
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
            float s;
            const Cand c = candidate(lds, k, x, y, z, &s);
            const bool in = valid && query_math::inside(c.n2);
            const unsigned long long m = __ballot(in);
            if (in) {
                const int rank = __popcll(m & ((1ull << lane) - 1ull));
                const long long row = (long long)lbase[k] + wave_base[(size_t)(o0 + c0 + k) * n_waves + wave] + rank;
                if (row >= 0 && row < n_rows) {
                    pts4[row] = make_float4(c.p[0], c.p[1], c.p[2], 0.f);
                    row_meta[row] = make_int2((int)(p0 + i), o0 + c0 + k);      // point index relative to the call's first point
                }
            }
        }
    }
}

// One thread per row: best[point] = min(best[point], key(sdf s_sel, object)).  sdf of row r = out[r * stride + off] (forward form: 1, 0; the
// jacobian form: GRAD_STRIDE, 67)
__global__ __launch_bounds__(QUERY_BLOCK) void k_query_reduce(const float* __restrict__ out, int stride, int off, const int2* __restrict__ row_meta,
                                                              int n_rows, const float4* __restrict__ tab, int n_obj, long long n_pts,
                                                              unsigned long long* __restrict__ best) {
    const int r = blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int2 m = row_meta[r];
    if (m.x < 0 || m.x >= n_pts || m.y < 0 || m.y >= n_obj) return;      // never taken: every row of a chunk is written by k_query_fill
    const float s_sel = tab[4 * (size_t)m.y + 3].y;
    const float d = query_math::distance(out[(size_t)r * stride + off], s_sel);
    atomicMin(&best[m.x], (unsigned long long)query_math::key(d, m.y));
}

// Normals only, behind the chunk's reduce: the row whose key is its point's best so far writes its world normal.  Keys are unique per
// (point, object), so one row writes; a later chunk's smaller key writes over it.
__global__ __launch_bounds__(QUERY_BLOCK) void k_query_winner(const float* __restrict__ rows, const int2* __restrict__ row_meta, int n_rows,
                                                              const float4* __restrict__ tab, int n_obj, long long n_pts,
                                                              const unsigned long long* __restrict__ best, float* __restrict__ normal) {
    const int r = blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int2 m = row_meta[r];
    if (m.x < 0 || m.x >= n_pts || m.y < 0 || m.y >= n_obj) return;
    const float4 t = *reinterpret_cast<const float4*>(rows + (size_t)r * GRAD_STRIDE + CODE_LEN);     // {gx, gy, gz, sdf}
    const float4 r0 = tab[4 * (size_t)m.y], r1 = tab[4 * (size_t)m.y + 1], r2 = tab[4 * (size_t)m.y + 2], q = tab[4 * (size_t)m.y + 3];
    if ((unsigned long long)query_math::key(query_math::distance(t.w, q.y), m.y) != best[m.x]) return;
    const float rt[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
    float nw[3];
    query_math::normal(rt, t.x, t.y, t.z, nw);
    normal[3 * (size_t)m.x] = nw[0]; normal[3 * (size_t)m.x + 1] = nw[1]; normal[3 * (size_t)m.x + 2] = nw[2];
}

// One thread per point: best -> obj, dist; a point without a winner gets a zero normal
__global__ __launch_bounds__(QUERY_BLOCK) void k_query_finish(const unsigned long long* __restrict__ best, long long n, int* __restrict__ obj,
                                                              float* __restrict__ dist, float* __restrict__ normal) {
    const long long i = (long long)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (i >= n) return;
    int32_t o;
    float d;
    query_math::unpack(best[i], &o, &d);
    obj[i] = o;
    dist[i] = d;
    if (normal && o < 0) { normal[3 * i] = 0.f; normal[3 * i + 1] = 0.f; normal[3 * i + 2] = 0.f; }
}

inline int blocks_for(long long n) { return (int)((n + QUERY_BLOCK - 1) / QUERY_BLOCK); }

}  // namespace

hipError_t launch_query_count(const float* pts3, int64_t p0, int n, const float* tab, int n_obj, int n_waves, int* wave_cnt, int* cnt, float* bound,
                              unsigned long long* best, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_query_count, dim3(blocks_for(n)), dim3(QUERY_BLOCK), 0, s, pts3, (long long)p0, n, reinterpret_cast<const float4*>(tab), n_obj,
                       n_waves, wave_cnt, bound, best);
    if (n_obj > 0) hipLaunchKernelGGL(k_query_scan, dim3(n_obj), dim3(QUERY_BLOCK), 0, s, wave_cnt, n_waves, cnt);
    return hipGetLastError();
}

hipError_t launch_query_fill(const float* pts3, int64_t p0, int n, const float* tab, int o0, int nc, const int* base, int n_waves, const int* wave_base,
                             int n_rows, float4* pts4, int2* row_meta, hipStream_t s) {
    if (n <= 0 || nc <= 0 || n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_query_fill, dim3(blocks_for(n)), dim3(QUERY_BLOCK), 0, s, pts3, (long long)p0, n, reinterpret_cast<const float4*>(tab), o0, nc,
                       base, n_waves, wave_base, n_rows, pts4, row_meta);
    return hipGetLastError();
}

hipError_t launch_query_reduce(const float* out, bool jacobian_rows, const int2* row_meta, int n_rows, const float* tab, int n_obj, int64_t n_pts,
                               unsigned long long* best, float* normal, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    const float4* t4 = reinterpret_cast<const float4*>(tab);
    hipLaunchKernelGGL(k_query_reduce, dim3(blocks_for(n_rows)), dim3(QUERY_BLOCK), 0, s, out, jacobian_rows ? GRAD_STRIDE : 1, jacobian_rows ? GRAD_STRIDE - 1 : 0,
                       row_meta, n_rows, t4, n_obj, (long long)n_pts, best);
    if (normal) hipLaunchKernelGGL(k_query_winner, dim3(blocks_for(n_rows)), dim3(QUERY_BLOCK), 0, s, out, row_meta, n_rows, t4, n_obj,
                                   (long long)n_pts, best, normal);
    return hipGetLastError();
}

hipError_t launch_query_finish(const unsigned long long* best, int64_t n, int* obj, float* dist, float* normal, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_query_finish, dim3(blocks_for(n)), dim3(QUERY_BLOCK), 0, s, best, (long long)n, obj, dist, normal);
    return hipGetLastError();
}

// query_math.h compiled for the host in this translation unit, which has contraction off (dsp_map_query's pose inversion and the
// dsp_debug_query_* functions)
bool query_invert_host(const float* t16, float* rt12, float* scale) { return query_math::invert(t16, rt12, scale); }

void query_candidates_host(int64_t n_obj, const float* rt, const float* scale, int64_t n_pts, const float* pts, float* p_obj, unsigned char* inside,
                           float* bound) {
    for (int64_t i = 0; i < n_pts; ++i) {
        float b = INFINITY;
        for (int64_t o = 0; o < n_obj; ++o) {
            float p[3];
            query_math::to_object(rt + 12 * o, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], p);
            const float n2 = query_math::norm2(p[0], p[1], p[2]);
            const bool in = query_math::inside(n2);
            if (!in) b = query_math::min_bound(b, query_math::sphere_bound(n2, scale[o]));
            const size_t k = (size_t)o * n_pts + i;
            if (p_obj) { p_obj[3 * k] = p[0]; p_obj[3 * k + 1] = p[1]; p_obj[3 * k + 2] = p[2]; }
            if (inside) inside[k] = in ? 1 : 0;
        }
        if (bound) bound[i] = b;
    }
}

void query_select_host(int64_t n_rows, const float* sdf, const float* scale_of_row, const int32_t* obj_of_row, const int32_t* pt_of_row, int64_t n_pts,
                       int32_t* obj, float* dist) {
    std::vector<uint64_t> best((size_t)n_pts, query_math::NO_KEY);
    for (int64_t r = 0; r < n_rows; ++r) {
        const uint64_t k = query_math::key(query_math::distance(sdf[r], scale_of_row[r]), obj_of_row[r]);
        if (k < best[pt_of_row[r]]) best[pt_of_row[r]] = k;
    }
    for (int64_t i = 0; i < n_pts; ++i) query_math::unpack(best[i], obj + i, dist + i);
}

}  // namespace dsp
