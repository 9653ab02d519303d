// Mesh extraction on the device: voxel grid -> decoder forward (mlp_kernel) -> marching cubes, without the SDF volume ever
// leaving HBM.  Replaces MeshExtractor.extract_mesh_from_code's grid decode + scikit-image call
// (reference reconstruct/optimizer.py:206-223, reconstruct/utils.py:97-140).
//
// Marching cubes here is HBM/latency-bound byte work (4 B read per grid point and a few neighbours from L2, 12 B written
// per vertex and per face): one thread per grid point, three small kernels around one block-sum scan:
//   k_mc_count   per block: number of vertices (sign-changing owned edges) and triangles (cell case table)
//   k_mc_scan    exclusive scan of the block sums (one block)
//   k_mc_verts   vertex positions + the (grid point, axis) -> vertex id map
//   k_mc_faces   triangles as vertex ids through that map
// Output order is fixed (vertices by (grid point, axis), faces by (cell, table order)) so it can be compared bit for bit
// with oracle/mc_oracle.py.  The 256-case table is generated on the host at first use (mc_build_tables) by the same
// published construction the oracle restates: per cube face, join each entering edge to the next leaving edge counter-
// clockwise; chain the segments into loops; triangulate each loop avoiding diagonals that lie inside a cube face.
#include "dsp_internal.h"

#include <algorithm>
#include <array>
#include <map>
#include <vector>

namespace dsp {

// ------------------------------------------------------------------------------------------------
// host: case table
// ------------------------------------------------------------------------------------------------
namespace {

struct Off3 { int o[3]; };

inline Off3 corner_offset(int c) { return Off3{{c & 1, (c >> 1) & 1, (c >> 2) & 1}}; }
inline int corner_index(const Off3& o) { return o.o[0] | (o.o[1] << 1) | (o.o[2] << 2); }

// cube edge between adjacent corners: 4 * axis + u + 2 v, (u, v) = its offsets along the two other axes (increasing order)
int edge_id(int c0, int c1) {
    const Off3 a = corner_offset(c0), b = corner_offset(c1);
    int axis = -1;
    for (int i = 0; i < 3; ++i) if (a.o[i] != b.o[i]) axis = i;
    int rest[2], n = 0;
    for (int i = 0; i < 3; ++i) if (i != axis) rest[n++] = i;
    return 4 * axis + a.o[rest[0]] + 2 * a.o[rest[1]];
}

void edge_owner(int e, Off3& off, int& axis) {
    axis = e / 4;
    const int uv = e % 4;
    int rest[2], n = 0;
    for (int i = 0; i < 3; ++i) if (i != axis) rest[n++] = i;
    off = Off3{{0, 0, 0}};
    off.o[rest[0]] = uv & 1;
    off.o[rest[1]] = uv >> 1;
}

bool edges_share_face(int e0, int e1) {
    Off3 o0, o1;
    int a0, a1;
    edge_owner(e0, o0, a0);
    edge_owner(e1, o1, a1);
    for (int a = 0; a < 3; ++a)
        if (a != a0 && a != a1 && o0.o[a] == o1.o[a]) return true;
    return false;
}

std::vector<std::array<int, 4>> cube_faces() {   // corners counter-clockwise seen from outside
    static const int other[3][2] = {{1, 2}, {2, 0}, {0, 1}};   // (b, c) with e_a = e_b x e_c
    std::vector<std::array<int, 4>> faces;
    for (int a = 0; a < 3; ++a)
        for (int side = 0; side < 2; ++side) {
            int ring[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
            if (side == 0) { std::swap(ring[0][0], ring[3][0]); std::swap(ring[0][1], ring[3][1]); std::swap(ring[1][0], ring[2][0]); std::swap(ring[1][1], ring[2][1]); }
            std::array<int, 4> f;
            for (int i = 0; i < 4; ++i) {
                Off3 o{{0, 0, 0}};
                o.o[a] = side; o.o[other[a][0]] = ring[i][0]; o.o[other[a][1]] = ring[i][1];
                f[i] = corner_index(o);
            }
            faces.push_back(f);
        }
    return faces;
}

std::vector<std::vector<int>> case_loops(int cfg, bool flip) {
    std::map<int, int> nxt;
    for (const auto& ring : cube_faces()) {
        int ins[4];
        for (int i = 0; i < 4; ++i) ins[i] = (cfg >> ring[i]) & 1;
        for (int i = 0; i < 4; ++i) {
            if (!ins[i] && ins[(i + 1) % 4]) {                                   // entering edge
                int j = (i + 1) % 4;
                while (!(ins[j] && !ins[(j + 1) % 4])) j = (j + 1) % 4;         // next leaving edge counter-clockwise
                const int e_in = edge_id(ring[i], ring[(i + 1) % 4]), e_out = edge_id(ring[j], ring[(j + 1) % 4]);
                if (flip) nxt[e_out] = e_in; else nxt[e_in] = e_out;
            }
        }
    }
    std::vector<std::vector<int>> loops;
    bool seen[12] = {false};
    for (const auto& kv : nxt) {
        const int e = kv.first;
        if (seen[e]) continue;
        std::vector<int> loop{e};
        seen[e] = true;
        while (nxt[loop.back()] != e) { loop.push_back(nxt[loop.back()]); seen[loop.back()] = true; }
        loops.push_back(loop);
    }
    return loops;
}

typedef std::vector<std::array<int, 3>> TriList;

std::vector<TriList> triangulations(const std::vector<int>& loop) {
    const int n = (int)loop.size();
    if (n < 3) return {TriList()};
    std::vector<TriList> out;
    for (int k = 1; k < n - 1; ++k) {   // the polygon edge (first, last) belongs to exactly one triangle (first, k, last)
        const std::vector<int> l(loop.begin(), loop.begin() + k + 1), r(loop.begin() + k, loop.end());
        for (const auto& left : triangulations(l))
            for (const auto& right : triangulations(r)) {
                TriList t = left;
                t.push_back({loop[0], loop[k], loop[n - 1]});
                t.insert(t.end(), right.begin(), right.end());
                out.push_back(t);
            }
    }
    return out;
}

TriList triangulate(const std::vector<int>& loop) {
    const int n = (int)loop.size();
    auto pos = [&](int e) { return (int)(std::find(loop.begin(), loop.end(), e) - loop.begin()); };
    bool have = false;
    int best_bad = 0;
    TriList best;
    for (const auto& tri : triangulations(loop)) {
        int bad = 0;
        for (const auto& t : tri)
            for (int s = 0; s < 3; ++s) {
                const int a = t[s], b = t[(s + 1) % 3];
                const int d = ((pos(a) - pos(b)) % n + n) % n;
                if (d != 1 && d != n - 1 && edges_share_face(a, b)) ++bad;
            }
        if (!have || bad < best_bad || (bad == best_bad && tri < best)) { have = true; best_bad = bad; best = tri; }
    }
    return best;
}

}  // namespace

void mc_build_tables(McTables& t) {
    memset(&t, 0xff, sizeof t);
    // winding: a lone inside corner 0 must give a triangle whose normal points away from it (towards +gradient)
    bool flip = false;
    {
        const std::vector<int> l = case_loops(1, false)[0];
        double p[3][3];
        for (int i = 0; i < 3; ++i) {
            Off3 o; int ax;
            edge_owner(l[i], o, ax);
            for (int c = 0; c < 3; ++c) p[i][c] = o.o[c];
            p[i][ax] = 0.5;
        }
        double u[3], v[3];
        for (int c = 0; c < 3; ++c) { u[c] = p[1][c] - p[0][c]; v[c] = p[2][c] - p[0][c]; }
        const double nsum = (u[1] * v[2] - u[2] * v[1]) + (u[2] * v[0] - u[0] * v[2]) + (u[0] * v[1] - u[1] * v[0]);
        flip = nsum < 0;
    }
    for (int cfg = 0; cfg < 256; ++cfg) {
        int n = 0;
        for (const auto& loop : case_loops(cfg, flip))
            for (const auto& tri : triangulate(loop)) {
                if (n >= MC_MAX_TRI) throw std::logic_error("marching-cubes case table overflow");
                for (int s = 0; s < 3; ++s) t.tri[cfg][3 * n + s] = (unsigned char)tri[s];
                ++n;
            }
        t.n_tri[cfg] = (unsigned char)n;
    }
    for (int e = 0; e < 12; ++e) {
        Off3 o; int ax;
        edge_owner(e, o, ax);
        t.edge_off[e][0] = (unsigned char)o.o[0]; t.edge_off[e][1] = (unsigned char)o.o[1]; t.edge_off[e][2] = (unsigned char)o.o[2];
        t.edge_off[e][3] = (unsigned char)ax;
    }
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int MC_BLOCK = 256;

struct Dims { int n0, n1, n2; };

__device__ __forceinline__ void unravel(int g, Dims d, int& i, int& j, int& k) {
    k = g % d.n2;
    j = (g / d.n2) % d.n1;
    i = g / (d.n2 * d.n1);
}

// vertices owned by grid point g (sign changes along +axis) and triangles of the cell whose lowest corner is g
__device__ __forceinline__ void mc_classify(const float* __restrict__ vol, Dims d, float level, int g, int n_pts,
                                            const McTables* __restrict__ tab, int& nv, int& cfg, int& nt, bool cross[3]) {
    nv = 0; cfg = 0; nt = 0;
    cross[0] = cross[1] = cross[2] = false;
    if (g >= n_pts) return;
    int i, j, k;
    unravel(g, d, i, j, k);
    const int s1 = d.n2, s0 = d.n1 * d.n2;
    const bool in0 = vol[g] < level;
    const bool h0 = i + 1 < d.n0, h1 = j + 1 < d.n1, h2 = k + 1 < d.n2;
    if (h0) cross[0] = in0 != (vol[g + s0] < level);
    if (h1) cross[1] = in0 != (vol[g + s1] < level);
    if (h2) cross[2] = in0 != (vol[g + 1] < level);
    nv = (int)cross[0] + (int)cross[1] + (int)cross[2];
    if (h0 && h1 && h2) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int gi = g + (c & 1) * s0 + ((c >> 1) & 1) * s1 + ((c >> 2) & 1);
            cfg |= (vol[gi] < level ? 1 : 0) << c;
        }
        nt = tab->n_tri[cfg];
    }
}

// exclusive scan of one int2 per thread over the block; returns this thread's offsets, block totals in `total`
__device__ __forceinline__ int2 block_scan(int2 v, int2* sh, int2& total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < MC_BLOCK; d <<= 1) {
        int2 add = make_int2(0, 0);
        if (t >= d) add = sh[t - d];
        __syncthreads();
        sh[t].x += add.x; sh[t].y += add.y;
        __syncthreads();
    }
    total = sh[MC_BLOCK - 1];
    return make_int2(sh[t].x - v.x, sh[t].y - v.y);
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_count(const float* vol, Dims d, float level, int n_pts, const McTables* tab, int2* block_sums) {
    __shared__ int2 sh[MC_BLOCK];
    const int g = blockIdx.x * MC_BLOCK + threadIdx.x;
    int nv, cfg, nt;
    bool cross[3];
    mc_classify(vol, d, level, g, n_pts, tab, nv, cfg, nt, cross);
    int2 total;
    block_scan(make_int2(nv, nt), sh, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void k_mc_scan(int2* block_sums, int n_blocks, long long* totals) {
    __shared__ long long shx[1024], shy[1024];
    const int t = threadIdx.x;
    const int per = (n_blocks + 1023) / 1024;
    const int b0 = t * per, b1 = min(n_blocks, b0 + per);
    long long sx = 0, sy = 0;
    for (int b = b0; b < b1; ++b) { sx += block_sums[b].x; sy += block_sums[b].y; }
    shx[t] = sx; shy[t] = sy;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        long long ax = 0, ay = 0;
        if (t >= d) { ax = shx[t - d]; ay = shy[t - d]; }
        __syncthreads();
        shx[t] += ax; shy[t] += ay;
        __syncthreads();
    }
    long long ox = shx[t] - sx, oy = shy[t] - sy;
    if (t == 1023) { totals[0] = shx[t]; totals[1] = shy[t]; }
    for (int b = b0; b < b1; ++b) {     // totals stay below 2^31 (checked on the host before the emit kernels run)
        const int2 v = block_sums[b];
        block_sums[b] = make_int2((int)ox, (int)oy);
        ox += v.x; oy += v.y;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_verts(const float* vol, Dims d, float level, int n_pts, const McTables* tab,
                                                       const int2* block_off, float spacing, float origin, float* verts, int* vidmap) {
    __shared__ int2 sh[MC_BLOCK];
    const int g = blockIdx.x * MC_BLOCK + threadIdx.x;
    int nv, cfg, nt;
    bool cross[3];
    mc_classify(vol, d, level, g, n_pts, tab, nv, cfg, nt, cross);
    int2 total;
    const int2 off = block_scan(make_int2(nv, nt), sh, total);
    if (nv == 0) return;
    int i, j, k;
    unravel(g, d, i, j, k);
    const int stride[3] = {d.n1 * d.n2, d.n2, 1};
    const float s0 = vol[g];
    int vid = block_off[blockIdx.x].x + off.x;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!cross[a]) continue;
        const float s1 = vol[g + stride[a]];
        const float t = __fdiv_rn(__fsub_rn(level, s0), __fsub_rn(s1, s0));
        float p[3] = {(float)i, (float)j, (float)k};
        p[a] = __fadd_rn(p[a], t);
#pragma unroll
        for (int c = 0; c < 3; ++c) verts[3 * (size_t)vid + c] = __fadd_rn(__fmul_rn(p[c], spacing), origin);
        vidmap[3 * (size_t)g + a] = vid;
        ++vid;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_faces(const float* vol, Dims d, float level, int n_pts, const McTables* tab,
                                                       const int2* block_off, const int* vidmap, int* faces) {
    __shared__ int2 sh[MC_BLOCK];
    const int g = blockIdx.x * MC_BLOCK + threadIdx.x;
    int nv, cfg, nt;
    bool cross[3];
    mc_classify(vol, d, level, g, n_pts, tab, nv, cfg, nt, cross);
    int2 total;
    const int2 off = block_scan(make_int2(nv, nt), sh, total);
    if (nt == 0) return;
    const int s1 = d.n2, s0 = d.n1 * d.n2;
    const size_t f0 = (size_t)block_off[blockIdx.x].y + off.y;
    for (int t = 0; t < nt; ++t)
        for (int c = 0; c < 3; ++c) {
            const int e = tab->tri[cfg][3 * t + c];
            const int go = g + tab->edge_off[e][0] * s0 + tab->edge_off[e][1] * s1 + tab->edge_off[e][2];
            faces[3 * (f0 + t) + c] = vidmap[3 * (size_t)go + tab->edge_off[e][3]];
        }
}

// voxel grid of MeshExtractor (reference utils.py:97-116), x slowest.  regular: point g = (i, j, k) * voxel_size + (-1).
// Otherwise the grid the reference really samples: `overall_index.long() / vol_dim` is true division under torch >= 1.6, so in
// float32 q1 = g / n, y index = fmod(q1, n), x index = fmod(q1 / n, n) (sheared by up to one voxel; golden_voxel_grid.npz).
__global__ void k_grid_points(float4* pts, int n, float voxel_size, int regular) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * n * n) return;
    float fi, fj;
    const float fk = (float)(g % n);
    if (regular) {
        fj = (float)((g / n) % n);
        fi = (float)(g / (n * n));
    } else {
        const float fn = (float)n;
        const float q1 = __fdiv_rn((float)g, fn);
        fj = fmodf(q1, fn);
        fi = fmodf(__fdiv_rn(q1, fn), fn);
    }
    pts[g] = make_float4(__fadd_rn(__fmul_rn(fi, voxel_size), -1.f), __fadd_rn(__fmul_rn(fj, voxel_size), -1.f),
                         __fadd_rn(__fmul_rn(fk, voxel_size), -1.f), 0.f);
}

// ---- batched extraction (extract_meshes_impl, mesh_host.hip) ----------------------------------------------------------------
// n_obj volumes of the same grid, back to back.  The marching-cubes kernels below are the ones above with the object taken from
// blockIdx.y; their block sums form ONE list (object-major) that k_mc_scan scans across the whole chunk, so every object's vertices
// and faces land in their own contiguous range in the order dsp_extract_mesh produces.  Vertex ids in vidmap are chunk-global; faces
// subtract the object's first vertex id, so face indices stay local to their mesh.

__global__ __launch_bounds__(MC_BLOCK) void k_mc_count_b(const float* vol, Dims d, float level, int n_pts, const McTables* tab, int2* block_sums) {
    __shared__ int2 sh[MC_BLOCK];
    const int g = blockIdx.x * MC_BLOCK + threadIdx.x, obj = blockIdx.y;
    int nv, cfg, nt;
    bool cross[3];
    mc_classify(vol + (size_t)obj * n_pts, d, level, g, n_pts, tab, nv, cfg, nt, cross);
    int2 total;
    block_scan(make_int2(nv, nt), sh, total);
    if (threadIdx.x == 0) block_sums[(size_t)obj * gridDim.x + blockIdx.x] = total;
}

// first (vertex, face) of every object: the scanned sum of its first block
__global__ void k_mc_obj_base(const int2* block_off, int nb, int n_obj, int2* base) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o < n_obj) base[o] = block_off[(size_t)o * nb];
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_verts_b(const float* vol, Dims d, float level, int n_pts, const McTables* tab,
                                                         const int2* block_off, float spacing, float origin, float* verts, int* vidmap) {
    __shared__ int2 sh[MC_BLOCK];
    const int g = blockIdx.x * MC_BLOCK + threadIdx.x, obj = blockIdx.y;
    const float* v = vol + (size_t)obj * n_pts;
    int nv, cfg, nt;
    bool cross[3];
    mc_classify(v, d, level, g, n_pts, tab, nv, cfg, nt, cross);
    int2 total;
    const int2 off = block_scan(make_int2(nv, nt), sh, total);
    if (nv == 0) return;
    int i, j, k;
    unravel(g, d, i, j, k);
    const int stride[3] = {d.n1 * d.n2, d.n2, 1};
    const float s0 = v[g];
    int vid = block_off[(size_t)obj * gridDim.x + blockIdx.x].x + off.x;
    int* vm = vidmap + (size_t)obj * 3 * n_pts;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!cross[a]) continue;
        const float s1 = v[g + stride[a]];
        const float t = __fdiv_rn(__fsub_rn(level, s0), __fsub_rn(s1, s0));
        float p[3] = {(float)i, (float)j, (float)k};
        p[a] = __fadd_rn(p[a], t);
#pragma unroll
        for (int c = 0; c < 3; ++c) verts[3 * (size_t)vid + c] = __fadd_rn(__fmul_rn(p[c], spacing), origin);
        vm[3 * (size_t)g + a] = vid;
        ++vid;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_faces_b(const float* vol, Dims d, float level, int n_pts, const McTables* tab,
                                                         const int2* block_off, const int* vidmap, int* faces) {
    __shared__ int2 sh[MC_BLOCK];
    const int g = blockIdx.x * MC_BLOCK + threadIdx.x, obj = blockIdx.y;
    int nv, cfg, nt;
    bool cross[3];
    mc_classify(vol + (size_t)obj * n_pts, d, level, g, n_pts, tab, nv, cfg, nt, cross);
    int2 total;
    const int2 off = block_scan(make_int2(nv, nt), sh, total);
    if (nt == 0) return;
    const int s1 = d.n2, s0 = d.n1 * d.n2;
    const int v0 = block_off[(size_t)obj * gridDim.x].x;          // the object's first vertex
    const int* vm = vidmap + (size_t)obj * 3 * n_pts;
    const size_t f0 = (size_t)block_off[(size_t)obj * gridDim.x + blockIdx.x].y + off.y;
    for (int t = 0; t < nt; ++t)
        for (int c = 0; c < 3; ++c) {
            const int e = tab->tri[cfg][3 * t + c];
            const int go = g + tab->edge_off[e][0] * s0 + tab->edge_off[e][1] * s1 + tab->edge_off[e][2];
            faces[3 * (f0 + t) + c] = vm[3 * (size_t)go + tab->edge_off[e][3]] - v0;
        }
}

// ---- surface band of a prepass volume (DESIGN.md "Mesh extraction") ---------------------------------------------------------
// Class of a prepass value against the object's margin: +1 (lp >= delta), -1 (lp <= -delta), 0 = uncertain (|lp| < delta, NaN, inf).
__device__ __forceinline__ int band_class(float x, float delta) {
    if (!isfinite(x)) return 0;
    return x >= delta ? 1 : (x <= -delta ? -1 : 0);
}

// fixed hash of (object, grid point): the stratified audit's choice (the same points every call)
__device__ __forceinline__ unsigned band_hash(unsigned c, unsigned g) {
    unsigned x = g * 0x9E3779B1u ^ (c + 0x7F4A7C15u) * 0x85EBCA77u;
    x ^= x >> 15; x *= 0x2C1B3C6Du;
    x ^= x >> 12; x *= 0x297A2D39u;
    return x ^ (x >> 15);
}

// One thread per grid point g of volume c (blockIdx.y).  A point needs its fp32 value when it is uncertain, or when one of its <= 6
// axis neighbours inside the grid is uncertain or certain of the opposite sign: then every sign marching cubes reads is certified
// and every value it interpolates is fp32.  Audit: 1/8 of the certain points with |lp| < 2 delta and 1/512 of the rest go to the fp32
// kernel too, so that its guard also looks at classified points.  Selected points are compacted per object (one atomic per wave,
// ballot order inside it) into [c * n, c * n + cnt[c]) of the point / value / index lists; the value list holds lp, which the fp32
// kernel's guard compares with what it stores there.  cnt = [n_obj] selected, [n_obj] audited; guard = per object {delta, trips, max err}.
__global__ __launch_bounds__(256) void k_mesh_band(const float* __restrict__ lp, const float4* __restrict__ grid, int n, int n_pts,
                                                   const unsigned* __restrict__ guard, float4* band_pts, float* band_val,
                                                   long long* band_idx, int* cnt, int n_obj) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const float delta = __uint_as_float(guard[3 * c]);
    const float* v = lp + (size_t)c * n_pts;
    bool need = false, audit = false;
    float x = 0.f;
    if (g < n_pts) {
        x = v[g];
        const int own = band_class(x, delta);
        need = own == 0;
        if (!need) {
            const int k = g % n, j = (g / n) % n, i = g / (n * n);
            const int s1 = n, s0 = n * n;
            int nb[6], m = 0;
            if (i > 0) nb[m++] = g - s0;
            if (i + 1 < n) nb[m++] = g + s0;
            if (j > 0) nb[m++] = g - s1;
            if (j + 1 < n) nb[m++] = g + s1;
            if (k > 0) nb[m++] = g - 1;
            if (k + 1 < n) nb[m++] = g + 1;
            for (int q = 0; q < m; ++q) {
                const int o = band_class(v[nb[q]], delta);
                if (o != own) { need = true; break; }       // uncertain (0) or the opposite sign
            }
        }
        if (!need) audit = (band_hash((unsigned)c, (unsigned)g) & (fabsf(x) < 2.f * delta ? 7u : 511u)) == 0u;
    }
    const bool sel = need || audit;
    const unsigned long long m = __ballot(sel), ma = __ballot(audit);
    if (m == 0ull) return;
    int base = 0;
    if (lane == 0) {
        base = atomicAdd(cnt + c, __popcll(m));
        if (ma) atomicAdd(cnt + n_obj + c, __popcll(ma));
    }
    base = __shfl(base, 0);
    if (!sel) return;
    const size_t o = (size_t)c * n_pts + base + __popcll(m & ((1ull << lane) - 1ull));
    band_pts[o] = grid[g];
    band_val[o] = x;
    band_idx[o] = (long long)c * n_pts + g;
}

// tile list of the fp32 kernel over the band lists: object c's tiles {c * n + 64 i, points, c, 0} follow those of objects < c.
// One block: per-object tile counts scanned (n_obj <= 1024), first tile of every object into tile0[c], the total into *n_tiles.
__global__ __launch_bounds__(1024) void k_mesh_tile_scan(const int* cnt, int n_obj, int* tile0, int* n_tiles) {
    __shared__ int sh[1024];
    const int t = threadIdx.x;
    const int nt = t < n_obj ? (cnt[t] + MESH_TILE_PTS - 1) / MESH_TILE_PTS : 0;
    sh[t] = nt;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    if (t < n_obj) tile0[t] = sh[t] - nt;
    if (t == 1023) *n_tiles = sh[t];
}

__global__ void k_mesh_tiles(const int* cnt, const int* tile0, int n_pts, int4* tiles) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
    const int first = i * MESH_TILE_PTS;
    if (first >= cnt[c]) return;
    tiles[tile0[c] + i] = make_int4(c * n_pts + first, min(MESH_TILE_PTS, cnt[c] - first), c, 0);
}

// the band's fp32 values into the volumes at their flat index (every other entry keeps its prepass value of certified sign)
__global__ void k_mesh_scatter(const float* band_val, const long long* band_idx, const int* cnt, int n_pts, float* vol) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
    if (i >= cnt[c]) return;
    const size_t o = (size_t)c * n_pts + i;
    vol[band_idx[o]] = band_val[o];
}

}  // namespace

int mc_num_blocks(int n_pts) { return (n_pts + MC_BLOCK - 1) / MC_BLOCK; }

hipError_t launch_grid_points(float4* pts, int n, float voxel_size, int regular, hipStream_t s) {
    const int total = n * n * n;
    hipLaunchKernelGGL(k_grid_points, dim3((total + 255) / 256), dim3(256), 0, s, pts, n, voxel_size, regular);
    return hipGetLastError();
}

hipError_t launch_mc_count(const float* vol, int n0, int n1, int n2, float level, const McTables* tab, int2* block_sums, long long* totals,
                           hipStream_t s) {
    const int n_pts = n0 * n1 * n2, nb = mc_num_blocks(n_pts);
    const Dims d{n0, n1, n2};
    hipLaunchKernelGGL(k_mc_count, dim3(nb), dim3(MC_BLOCK), 0, s, vol, d, level, n_pts, tab, block_sums);
    hipLaunchKernelGGL(k_mc_scan, dim3(1), dim3(1024), 0, s, block_sums, nb, totals);
    return hipGetLastError();
}

hipError_t launch_mc_emit(const float* vol, int n0, int n1, int n2, float level, const McTables* tab, const int2* block_off, float spacing,
                          float origin, float* verts, int* vidmap, int* faces, hipStream_t s) {
    const int n_pts = n0 * n1 * n2, nb = mc_num_blocks(n_pts);
    const Dims d{n0, n1, n2};
    hipLaunchKernelGGL(k_mc_verts, dim3(nb), dim3(MC_BLOCK), 0, s, vol, d, level, n_pts, tab, block_off, spacing, origin, verts, vidmap);
    hipLaunchKernelGGL(k_mc_faces, dim3(nb), dim3(MC_BLOCK), 0, s, vol, d, level, n_pts, tab, block_off, vidmap, faces);
    return hipGetLastError();
}

hipError_t launch_mc_count_batched(const float* vol, int n, int n_obj, float level, const McTables* tab, int2* block_sums, long long* totals,
                                   int2* obj_base, hipStream_t s) {
    const int n_pts = n * n * n, nb = mc_num_blocks(n_pts);
    const Dims d{n, n, n};
    hipLaunchKernelGGL(k_mc_count_b, dim3(nb, n_obj), dim3(MC_BLOCK), 0, s, vol, d, level, n_pts, tab, block_sums);
    hipLaunchKernelGGL(k_mc_scan, dim3(1), dim3(1024), 0, s, block_sums, nb * n_obj, totals);
    hipLaunchKernelGGL(k_mc_obj_base, dim3((n_obj + 255) / 256), dim3(256), 0, s, block_sums, nb, n_obj, obj_base);
    return hipGetLastError();
}

hipError_t launch_mc_emit_batched(const float* vol, int n, int n_obj, float level, const McTables* tab, const int2* block_off, float spacing,
                                  float origin, float* verts, int* vidmap, int* faces, hipStream_t s) {
    const int n_pts = n * n * n, nb = mc_num_blocks(n_pts);
    const Dims d{n, n, n};
    hipLaunchKernelGGL(k_mc_verts_b, dim3(nb, n_obj), dim3(MC_BLOCK), 0, s, vol, d, level, n_pts, tab, block_off, spacing, origin, verts, vidmap);
    hipLaunchKernelGGL(k_mc_faces_b, dim3(nb, n_obj), dim3(MC_BLOCK), 0, s, vol, d, level, n_pts, tab, block_off, vidmap, faces);
    return hipGetLastError();
}

hipError_t launch_mesh_band(const float* lp, const float4* grid, int n, int n_obj, const unsigned* guard, float4* band_pts, float* band_val,
                            long long* band_idx, int* cnt, int* tile0, int* n_tiles, int4* tiles, hipStream_t s) {
    const int n_pts = n * n * n;
    hipLaunchKernelGGL(k_mesh_band, dim3((n_pts + 255) / 256, n_obj), dim3(256), 0, s, lp, grid, n, n_pts, guard, band_pts, band_val, band_idx,
                       cnt, n_obj);
    hipLaunchKernelGGL(k_mesh_tile_scan, dim3(1), dim3(1024), 0, s, cnt, n_obj, tile0, n_tiles);
    const int max_tiles = (n_pts + MESH_TILE_PTS - 1) / MESH_TILE_PTS;
    hipLaunchKernelGGL(k_mesh_tiles, dim3((max_tiles + 255) / 256, n_obj), dim3(256), 0, s, cnt, tile0, n_pts, tiles);
    return hipGetLastError();
}

hipError_t launch_mesh_scatter(const float* band_val, const long long* band_idx, const int* cnt, int n, int n_obj, float* vol, hipStream_t s) {
    const int n_pts = n * n * n;
    hipLaunchKernelGGL(k_mesh_scatter, dim3((n_pts + 255) / 256, n_obj), dim3(256), 0, s, band_val, band_idx, cnt, n_pts, vol);
    return hipGetLastError();
}

}  // namespace dsp
