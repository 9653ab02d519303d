// Surface projection kernels (dsp_surface_points / dsp_meshes_refine): the steps between the decoder launches.  The decoder work itself is
// mlp_kernel<2> (mlp_kernel.hip) as decode_resident_points launches it; these kernels only move points in and out of its float4 list and
// apply surface_math.h to the 68-float rows it writes.  Compiled with contraction off (build.py), like every file that restates a
// formula operation by operation.
#include "dsp_internal.h"
#include "surface_math.h"

namespace dsp {

namespace {

constexpr int SURF_BLOCK = 256;
static_assert(GRAD_STRIDE == surface_math::ROW && CODE_LEN == surface_math::CODE, "row layout");
static_assert((GRAD_STRIDE * 4) % 16 == 0 && ((GRAD_STRIDE - 4) * 4) % 16 == 0, "the row's tail {gx, gy, gz, sdf} is one aligned 16-byte load");
static_assert(TILE_PTS % (SURF_BLOCK / surface_math::LANES) == 0, "a tile is a whole number of 16-point rounds of a block");

// packed float3 points -> the decoder's float4 list (unpack = 0), or back (unpack = 1); n points.  A point with a coordinate that is not
// finite enters the list as NaN in every coordinate and stays that way (k_surface_step does not move it, k_surface_attributes returns NaN)
__global__ __launch_bounds__(SURF_BLOCK) void k_surface_pack(const float* __restrict__ p3, float4* __restrict__ p4, float* __restrict__ out3,
                                                             int n, int unpack) {
    const int i = blockIdx.x * SURF_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (!unpack) {
        const float x = p3[3 * (size_t)i], y = p3[3 * (size_t)i + 1], z = p3[3 * (size_t)i + 2];
        const float q = nanf("");
        p4[i] = surface_math::point_ok(x, y, z) ? make_float4(x, y, z, 0.f) : make_float4(q, q, q, 0.f);
    } else {
        const float4 p = p4[i];
        out3[3 * (size_t)i] = p.x; out3[3 * (size_t)i + 1] = p.y; out3[3 * (size_t)i + 2] = p.z;
    }
}

// one lane per point: p <- surface_math::step(p, row tail).  rows: [n][GRAD_STRIDE], row i belongs to point i
__global__ __launch_bounds__(SURF_BLOCK) void k_surface_step(float4* __restrict__ pts, const float* __restrict__ rows, int n, float max_step) {
    const int i = blockIdx.x * SURF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 t = *reinterpret_cast<const float4*>(rows + (size_t)i * GRAD_STRIDE + CODE_LEN);     // {gx, gy, gz, sdf}
    const float4 p = pts[i];
    if (!surface_math::point_ok(p.x, p.y, p.z)) return;
    const float pin[3] = {p.x, p.y, p.z}, g[3] = {t.x, t.y, t.z};
    float o[3];
    surface_math::step(pin, t.w, g, max_step, o);
    pts[i] = make_float4(o[0], o[1], o[2], 0.f);
}

// 16 lanes per point, one workgroup per tile of the decoder's list ({first point, count <= TILE_PTS, object, output base}): the tile's
// object is uniform, so each lane keeps its four variance entries in registers for the whole tile.  var: [object][64] floats or null -- then
// the 256 B of code gradient per point are never read and sigma is not written.  Outputs are indexed by point (first + i), any may be null.
__global__ __launch_bounds__(SURF_BLOCK) void k_surface_attributes(const int4* __restrict__ tiles, const float4* __restrict__ pts,
                                                                   const float* __restrict__ rows,
                                                                   const float* __restrict__ var, float* __restrict__ normals,
                                                                   float* __restrict__ grad_norm, float* __restrict__ sdf,
                                                                   float* __restrict__ sigma) {
    constexpr int L = surface_math::LANES, PER_ROUND = SURF_BLOCK / L;
    const int4 td = tiles[blockIdx.x];
    const int lane = threadIdx.x & (L - 1), slot = threadIdx.x / L;
    float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (var) v4 = *reinterpret_cast<const float4*>(var + (size_t)td.z * CODE_LEN + 4 * lane);
    const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
    for (int r = 0; r < TILE_PTS / PER_ROUND; ++r) {
        const int local = r * PER_ROUND + slot;         // uniform over the 16 lanes of a point: they leave together
        if (local >= td.y) break;
        const size_t i = (size_t)td.x + local;
        const float* row = rows + (i + td.w) * GRAD_STRIDE;
        float S = 0.f;
        if (var) {
            const float4 c4 = *reinterpret_cast<const float4*>(row + 4 * lane);
            const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
            S = surface_math::lane_sum(cc, vv);
#pragma unroll
            for (int m = 0; m < surface_math::N_MASKS; ++m) S = __fadd_rn(S, __shfl_xor(S, surface_math::mask(m), L));
        }
        if (lane == 0) {
            const float4 t = *reinterpret_cast<const float4*>(row + CODE_LEN);
            const float4 p = pts[i];
            const surface_math::Attr a = surface_math::point_ok(p.x, p.y, p.z) ? surface_math::finish(t.x, t.y, t.z, t.w, S, var != nullptr)
                                                                               : surface_math::nan_attr();
            if (normals) { normals[3 * i] = a.nx; normals[3 * i + 1] = a.ny; normals[3 * i + 2] = a.nz; }
            if (grad_norm) grad_norm[i] = a.grad_norm;
            if (sdf) sdf[i] = a.sdf;
            if (sigma && var) sigma[i] = a.sigma;
        }
    }
}

}  // namespace

hipError_t launch_surface_pack(const float* p3, float4* p4, float* out3, int n, int unpack, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_surface_pack, dim3((n + SURF_BLOCK - 1) / SURF_BLOCK), dim3(SURF_BLOCK), 0, s, p3, p4, out3, n, unpack);
    return hipGetLastError();
}

hipError_t launch_surface_step(float4* pts, const float* rows, int n, float max_step, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_surface_step, dim3((n + SURF_BLOCK - 1) / SURF_BLOCK), dim3(SURF_BLOCK), 0, s, pts, rows, n, max_step);
    return hipGetLastError();
}

hipError_t launch_surface_attributes(const int4* tiles, int n_tiles, const float4* pts, const float* rows, const float* var, float* normals, float* grad_norm,
                                     float* sdf, float* sigma, hipStream_t s) {
    if (n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_surface_attributes, dim3(n_tiles), dim3(SURF_BLOCK), 0, s, tiles, pts, rows, var, normals, grad_norm, sdf, sigma);
    return hipGetLastError();
}

// surface_math.h compiled for the host in this translation unit, which has contraction off (dsp_debug_surface_step / _attributes)
void surface_step_host(int64_t n, const float* pts, const float* sdf, const float* grad_xyz, float max_step, float* pts_out) {
    for (int64_t i = 0; i < n; ++i) surface_math::step(pts + 3 * i, sdf[i], grad_xyz + 3 * i, max_step, pts_out + 3 * i);
}

void surface_attributes_host(int64_t n, const float* rows68, const float* var64, float* normals, float* grad_norm, float* sdf, float* sigma) {
    for (int64_t i = 0; i < n; ++i) {
        const surface_math::Attr a = surface_math::attributes(rows68 + i * surface_math::ROW, var64);
        if (normals) { normals[3 * i] = a.nx; normals[3 * i + 1] = a.ny; normals[3 * i + 2] = a.nz; }
        if (grad_norm) grad_norm[i] = a.grad_norm;
        if (sdf) sdf[i] = a.sdf;
        if (sigma && var64) sigma[i] = a.sigma;
    }
}

}  // namespace dsp
