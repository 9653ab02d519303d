// Ray casting kernels (dsp_map_raycast): the listing of (ray, object) pairs, the rounds of the march -- compaction with device-built tile
// lists, the step rule -- and the winners' normals.  The decoder work itself is mlp_kernel<0> / mlp_kernel<2> (mlp_kernel.hip); the
// arithmetic is raycast_math.h.  Compiled with contraction off (build.py), like every file that restates a formula operation by operation.
//
// No float atomics: pairs are listed per object in ascending ray order (ballot rank inside a wave + scanned wave counts), a round's live
// pairs are compacted in that same order, and the only atomics are integer minima (the 64-bit hit key, the 32-bit exhausted parameter) and
// one integer count, whose results do not depend on the order of their operands.
//
// A pass holds the pairs [lo, hi) of each of its objects in SLOTS: object k's pairs start at a multiple of 64, so a wave of slots belongs to
// one object.  Slot state: 0 live, 1 hit, 2 ended as a miss, anything else padding.
#include "dsp_internal.h"
#include "raycast_math.h"

namespace dsp {

namespace {

constexpr int RC_BLOCK = 256;
constexpr int RC_WAVE = 64;
constexpr int RC_LDS_OBJ = 256;         // objects staged in LDS at a time: 256 x 16 floats = 16 KiB
constexpr int RC_PLAN_BLOCK = 1024;     // k_raycast_plan is ONE block
static_assert(query_math::OBJ_STRIDE == 16 && RC_LDS_OBJ == RC_BLOCK, "one thread stages one object: four float4 loads");

__device__ __forceinline__ void rc_stage(float4* lds, const float4* __restrict__ tab, int o0, int n) {
    if ((int)threadIdx.x < n) {
#pragma unroll
        for (int q = 0; q < 4; ++q) lds[4 * threadIdx.x + q] = tab[4 * ((size_t)o0 + threadIdx.x) + q];
    }
}

__device__ __forceinline__ void rc_entry(const float4* e, float* t16) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = e[q];
        t16[4 * q] = v.x; t16[4 * q + 1] = v.y; t16[4 * q + 2] = v.z; t16[4 * q + 3] = v.w;
    }
}

// ray i of the call: origin, unit direction; false = void or past the end
__device__ __forceinline__ bool rc_load_ray(const float* __restrict__ org, const float* __restrict__ dir, int i, int n, float* o, float* u) {
    if (i >= n) return false;
    const size_t q = 3 * (size_t)i;
    o[0] = org[q]; o[1] = org[q + 1]; o[2] = org[q + 2];
    const float d[3] = {dir[q], dir[q + 1], dir[q + 2]};
    return raycast_math::ray(o, d, u);
}

// One thread per ray, the wave loops over all objects.  wave_cnt[obj][wave] = pairs of the wave that exist; per ray best = the all-ones key,
// exh = none, dist = +inf.  n_waves = ceil(n / 64).
__global__ __launch_bounds__(RC_BLOCK) void k_raycast_count(const float* __restrict__ org, const float* __restrict__ dir, int n,
                                                            const float4* __restrict__ tab, int n_obj, int n_waves, raycast_math::Params prm,
                                                            int* __restrict__ wave_cnt, unsigned long long* __restrict__ best,
                                                            unsigned* __restrict__ exh, float* __restrict__ dist) {
    __shared__ float4 lds[4 * RC_LDS_OBJ];
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    const int wave = i / RC_WAVE, lane = threadIdx.x & (RC_WAVE - 1);
    float o[3] = {0.f, 0.f, 0.f}, u[3] = {0.f, 0.f, 0.f};
    const bool ok = rc_load_ray(org, dir, i, n, o, u);
    for (int o0 = 0; o0 < n_obj; o0 += RC_LDS_OBJ) {
        const int nk = min(RC_LDS_OBJ, n_obj - o0);
        __syncthreads();
        rc_stage(lds, tab, o0, nk);
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
            float e[16];
            rc_entry(lds + 4 * k, e);
            const raycast_math::Segment g = raycast_math::segment(e, o, u, prm.t_min, prm.t_max);
            const unsigned long long m = __ballot(ok && g.exists);
            if (lane == 0 && wave < n_waves) wave_cnt[(size_t)(o0 + k) * n_waves + wave] = __popcll(m);
        }
    }
    if (i < n) {
        best[i] = query_math::NO_KEY;
        exh[i] = 0xffffffffu;
        dist[i] = __uint_as_float(0x7f800000u);
    }
}

// One block per object: wave_cnt[obj][.] -> its exclusive scan in place, cnt[obj] = the total
__global__ __launch_bounds__(RC_BLOCK) void k_raycast_scan(int* __restrict__ wave_cnt, int n_waves, int* __restrict__ cnt) {
    __shared__ int sh[RC_BLOCK];
    int* w = wave_cnt + (size_t)blockIdx.x * n_waves;
    int carry = 0;
    for (int base = 0; base < n_waves; base += RC_BLOCK) {
        const int j = base + threadIdx.x;
        const int v = j < n_waves ? w[j] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < RC_BLOCK; d <<= 1) {
            const int t = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (j < n_waves) w[j] = carry + sh[threadIdx.x] - v;
        carry += sh[RC_BLOCK - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt[blockIdx.x] = carry;
}

// The pass's objects [o0, o0 + nc): pair j of object o0 + k (ascending ray order) with lo <= j < hi goes to slot pobj[k].x + j
// (pobj[k] = {slot offset, lo, hi, 0}).
__global__ __launch_bounds__(RC_BLOCK) void k_raycast_fill(const float* __restrict__ org, const float* __restrict__ dir, int n,
                                                           const float4* __restrict__ tab, int o0, int nc, const int4* __restrict__ pobj,
                                                           int n_waves, const int* __restrict__ wave_base, raycast_math::Params prm, int n_slots,
                                                           int2* __restrict__ pr_meta, int* __restrict__ pr_state, float* __restrict__ pr_t,
                                                           float* __restrict__ pr_t1, float4* __restrict__ pr_oo, float4* __restrict__ pr_do) {
    __shared__ float4 lds[4 * RC_LDS_OBJ];
    __shared__ int4 lobj[RC_LDS_OBJ];
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    const int wave = i / RC_WAVE, lane = threadIdx.x & (RC_WAVE - 1);
    float o[3] = {0.f, 0.f, 0.f}, u[3] = {0.f, 0.f, 0.f};
    const bool ok = rc_load_ray(org, dir, i, n, o, u);
    for (int c0 = 0; c0 < nc; c0 += RC_LDS_OBJ) {
        const int nk = min(RC_LDS_OBJ, nc - c0);
        __syncthreads();
        rc_stage(lds, tab, o0 + c0, nk);
        if ((int)threadIdx.x < nk) lobj[threadIdx.x] = pobj[c0 + threadIdx.x];
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
            float e[16];
            rc_entry(lds + 4 * k, e);
            const raycast_math::Segment g = raycast_math::segment(e, o, u, prm.t_min, prm.t_max);
            const bool in = ok && g.exists;
            const unsigned long long m = __ballot(in);
            if (in) {
                const int4 po = lobj[k];
                const long long j = (long long)wave_base[(size_t)(o0 + c0 + k) * n_waves + wave] + __popcll(m & ((1ull << lane) - 1ull));
                const long long slot = (long long)po.x + j;
                if (j >= po.y && j < po.z && slot >= 0 && slot < n_slots) {
                    pr_meta[slot] = make_int2(i, o0 + c0 + k);
                    pr_state[slot] = 0;
                    pr_t[slot] = g.t0;
                    pr_t1[slot] = g.t1;
                    pr_oo[slot] = make_float4(g.o_o[0], g.o_o[1], g.o_o[2], 0.f);
                    pr_do[slot] = make_float4(g.d_o[0], g.d_o[1], g.d_o[2], 0.f);
                }
            }
        }
    }
}

__device__ __forceinline__ bool rc_slot_live(const int* pr_state, int slot, int n_slots) { return slot < n_slots && pr_state[slot] == 0; }

// Start of a round, one thread per slot: occlusion retirement against the keys of the previous round, then live_cnt[wave] = live slots
__global__ __launch_bounds__(RC_BLOCK) void k_raycast_live(int n_slots, const int2* __restrict__ pr_meta, int* __restrict__ pr_state,
                                                           const float* __restrict__ pr_t, int n_rays,
                                                           const unsigned long long* __restrict__ best, int* __restrict__ live_cnt) {
    const int slot = blockIdx.x * RC_BLOCK + threadIdx.x;
    const int wave = slot / RC_WAVE, lane = threadIdx.x & (RC_WAVE - 1);
    bool live = rc_slot_live(pr_state, slot, n_slots);
    if (live) {
        const int ray = pr_meta[slot].x;
        if (ray < 0 || ray >= n_rays) live = false;         // never taken: every live slot was written by k_raycast_fill
        else {
            const unsigned hi = (unsigned)(best[ray] >> 32);
            if (hi != 0xffffffffu && pr_t[slot] > query_math::from_orderable(hi)) {
                pr_state[slot] = 2;
                live = false;
            }
        }
    }
    const unsigned long long m = __ballot(live);
    if (lane == 0 && slot < n_slots) live_cnt[wave] = __popcll(m);
}

// block-wide exclusive scan of one value per thread; returns the exclusive prefix, *total = the block's sum.  sh: RC_PLAN_BLOCK ints
__device__ __forceinline__ int rc_block_scan(int* sh, int v, int* total) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < RC_PLAN_BLOCK; d <<= 1) {
        const int t = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    const int incl = sh[threadIdx.x];
    *total = sh[RC_PLAN_BLOCK - 1];
    __syncthreads();
    return incl - v;
}

// ONE block.  live_cnt[n_slot_waves] -> wave_row (exclusive scan: the compacted row of each wave's first live slot); per object k of the pass
// (ob[k] = {first wave, waves, object index, 0}) oinfo[k] = {first row, live rows, first tile, object index}; ctrl = {tiles, live rows};
// dstats += {rows, tiles, rounds that decoded a row}
__global__ __launch_bounds__(RC_PLAN_BLOCK) void k_raycast_plan(const int* __restrict__ live_cnt, int n_slot_waves, const int4* __restrict__ ob, int nc,
                                                                int* __restrict__ wave_row, int4* __restrict__ oinfo, int* __restrict__ ctrl,
                                                                unsigned long long* __restrict__ dstats) {
    __shared__ int sh[RC_PLAN_BLOCK];
    int carry = 0;
    for (int base = 0; base < n_slot_waves; base += RC_PLAN_BLOCK) {
        const int j = base + threadIdx.x;
        const int v = j < n_slot_waves ? live_cnt[j] : 0;
        int total;
        const int ex = rc_block_scan(sh, v, &total);
        if (j < n_slot_waves) wave_row[j] = carry + ex;
        carry += total;
    }
    const int n_live = carry;
    __syncthreads();                    // wave_row is read below by other threads of this block
    int tcarry = 0;
    for (int base = 0; base < nc; base += RC_PLAN_BLOCK) {
        const int k = base + threadIdx.x;
        int first = 0, live = 0, obj = 0;
        if (k < nc) {
            const int4 e = ob[k];
            obj = e.z;
            if (e.y > 0) {
                first = wave_row[e.x];
                const int end = e.x + e.y < n_slot_waves ? wave_row[e.x + e.y] : n_live;
                live = end - first;
            }
        }
        const int nt = (live + TILE_PTS - 1) / TILE_PTS;
        int total;
        const int ex = rc_block_scan(sh, nt, &total);
        if (k < nc) oinfo[k] = make_int4(first, live, tcarry + ex, obj);
        tcarry += total;
    }
    if (threadIdx.x == 0) {
        ctrl[0] = tcarry;
        ctrl[1] = n_live;
        dstats[0] += (unsigned long long)n_live;
        dstats[1] += (unsigned long long)tcarry;
        dstats[2] += n_live > 0 ? 1ull : 0ull;
    }
}

// One thread per slot: the live slots' samples in slot order (grouped by object, ascending ray) and row -> slot; the first lane of the j-th
// wave of an object writes the object's j-th tile.  wtab[wave] = {object of the pass, the object's first wave}
__global__ __launch_bounds__(RC_BLOCK) void k_raycast_emit(int n_slots, const int* __restrict__ pr_state, const float* __restrict__ pr_t,
                                                           const float4* __restrict__ pr_oo, const float4* __restrict__ pr_do,
                                                           const int2* __restrict__ wtab, const int* __restrict__ wave_row,
                                                           const int4* __restrict__ oinfo, int nc, int n_slot_waves, float4* __restrict__ pts4,
                                                           int* __restrict__ row_slot, int4* __restrict__ tiles) {
    const int slot = blockIdx.x * RC_BLOCK + threadIdx.x;
    const int wave = slot / RC_WAVE, lane = threadIdx.x & (RC_WAVE - 1);
    const bool live = rc_slot_live(pr_state, slot, n_slots);
    const unsigned long long m = __ballot(live);
    if (slot >= n_slots) return;
    if (live) {
        const int row = wave_row[wave] + __popcll(m & ((1ull << lane) - 1ull));
        if (row >= 0 && row < n_slots) {
            const float4 oo = pr_oo[slot], dd = pr_do[slot];
            const float a[3] = {oo.x, oo.y, oo.z}, b[3] = {dd.x, dd.y, dd.z};
            float p[3];
            raycast_math::sample(a, b, pr_t[slot], p);
            pts4[row] = make_float4(p[0], p[1], p[2], 0.f);
            row_slot[row] = slot;
        }
    }
    if (lane == 0) {
        const int2 w = wtab[wave];
        if (w.x >= 0 && w.x < nc) {
            const int4 oi = oinfo[w.x];
            const int j = wave - w.y;
            if (j >= 0 && j * TILE_PTS < oi.y && oi.z + j < n_slot_waves)
                tiles[oi.z + j] = make_int4(oi.x + j * TILE_PTS, min(TILE_PTS, oi.y - j * TILE_PTS), oi.w, 0);
        }
    }
}

// One thread per compacted row: the step rule on the decoder's value
__global__ __launch_bounds__(RC_BLOCK) void k_raycast_step(const float* __restrict__ sdf, const int* __restrict__ row_slot, const int* __restrict__ ctrl,
                                                           int n_slots, const int2* __restrict__ pr_meta, int* __restrict__ pr_state,
                                                           float* __restrict__ pr_t, const float* __restrict__ pr_t1, float* __restrict__ pr_dist,
                                                           const float4* __restrict__ tab, int n_obj, int n_rays, raycast_math::Params prm,
                                                           unsigned long long* __restrict__ best) {
    const int r = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (r >= ctrl[1] || r >= n_slots) return;
    const int slot = row_slot[r];
    if (slot < 0 || slot >= n_slots) return;                // never taken: every row below ctrl[1] was written by k_raycast_emit
    const int2 m = pr_meta[slot];
    if (m.x < 0 || m.x >= n_rays || m.y < 0 || m.y >= n_obj) return;
    const float s = tab[4 * (size_t)m.y + 3].y;             // s_sel == s: the pair exists
    const float t = pr_t[slot];
    float d, tn;
    const int dec = raycast_math::step(t, pr_t1[slot], sdf[r], s, prm.eps, prm.relax, &d, &tn);
    if (dec == raycast_math::STEP_HIT) {
        pr_dist[slot] = d;
        pr_state[slot] = 1;
        atomicMin(&best[m.x], (unsigned long long)query_math::key(t, m.y));
    } else if (dec == raycast_math::STEP_ADVANCE) {
        pr_t[slot] = tn;
    } else {
        pr_state[slot] = 2;
    }
}

// End of a pass, one thread per slot: a slot still live is exhausted (its parameter joins the ray's minimum; counted); the hit that holds
// its ray's key writes the ray's dist (keys are unique per ray and object; a later pass's smaller key writes over it)
__global__ __launch_bounds__(RC_BLOCK) void k_raycast_end(int n_slots, const int2* __restrict__ pr_meta, const int* __restrict__ pr_state,
                                                          const float* __restrict__ pr_t, const float* __restrict__ pr_dist, int n_rays,
                                                          const unsigned long long* __restrict__ best, unsigned* __restrict__ exh,
                                                          float* __restrict__ dist, unsigned long long* __restrict__ dstats) {
    const int slot = blockIdx.x * RC_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (RC_WAVE - 1);
    int st = slot < n_slots ? pr_state[slot] : 2;
    int2 m = make_int2(-1, -1);
    if (st == 0 || st == 1) {
        m = pr_meta[slot];
        if (m.x < 0 || m.x >= n_rays) st = 2;
    }
    if (st == 0) atomicMin(&exh[m.x], query_math::orderable(pr_t[slot]));
    if (st == 1 && (unsigned long long)query_math::key(pr_t[slot], m.y) == best[m.x]) dist[m.x] = pr_dist[slot];
    const unsigned long long b = __ballot(st == 0);
    if (lane == 0 && b) atomicAdd(&dstats[3], (unsigned long long)__popcll(b));
}

// One thread per ray: best, exh -> obj, t, status; a ray without a winner gets a zero normal
__global__ __launch_bounds__(RC_BLOCK) void k_raycast_finish(const unsigned long long* __restrict__ best, const unsigned* __restrict__ exh, int n,
                                                             int* __restrict__ obj, float* __restrict__ t, int* __restrict__ status,
                                                             float* __restrict__ normal) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n) return;
    int32_t o;
    float th;
    const unsigned long long k = best[i];
    query_math::unpack(k, &o, &th);
    obj[i] = o;
    t[i] = th;
    status[i] = raycast_math::status(k, exh[i]);
    if (normal && o < 0) { normal[3 * (size_t)i] = 0.f; normal[3 * (size_t)i + 1] = 0.f; normal[3 * (size_t)i + 2] = 0.f; }
}

// Normals.  One thread per ray, the wave loops over all objects: wave_cnt[obj][wave] = rays of the wave whose winner is obj
__global__ __launch_bounds__(RC_BLOCK) void k_raycast_wincount(const int* __restrict__ obj, int n, int n_obj, int n_waves, int* __restrict__ wave_cnt) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    const int wave = i / RC_WAVE, lane = threadIdx.x & (RC_WAVE - 1);
    const int mine = i < n ? obj[i] : -1;
    for (int k = 0; k < n_obj; ++k) {
        const unsigned long long m = __ballot(mine == k);
        if (lane == 0 && wave < n_waves) wave_cnt[(size_t)k * n_waves + wave] = __popcll(m);
    }
}

// The chunk's objects [o0, o0 + nc): winner j of object o0 + k (ascending ray order) has chunk row base[k] + j; rows inside [0, n_rows) are
// written: the hit sample to the decoder's list, {ray, object} to row_meta
__global__ __launch_bounds__(RC_BLOCK) void k_raycast_winfill(const float* __restrict__ org, const float* __restrict__ dir, const int* __restrict__ obj,
                                                              const float* __restrict__ t_hit, int n, const float4* __restrict__ tab, int n_obj,
                                                              int o0, int nc, const int* __restrict__ base, int n_waves,
                                                              const int* __restrict__ wave_base, raycast_math::Params prm, int n_rows,
                                                              float4* __restrict__ pts4, int2* __restrict__ row_meta) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    const int wave = i / RC_WAVE, lane = threadIdx.x & (RC_WAVE - 1);
    const int mine = i < n ? obj[i] : -1;
    float o[3] = {0.f, 0.f, 0.f}, u[3] = {0.f, 0.f, 0.f};
    const bool ok = rc_load_ray(org, dir, i, n, o, u) && mine >= 0 && mine < n_obj;
    for (int k = 0; k < nc; ++k) {
        const bool in = ok && mine == o0 + k;
        const unsigned long long m = __ballot(in);
        if (in) {
            const long long row = (long long)base[k] + wave_base[(size_t)(o0 + k) * n_waves + wave] + __popcll(m & ((1ull << lane) - 1ull));
            if (row >= 0 && row < n_rows) {
                float e[16];
                rc_entry(tab + 4 * (size_t)mine, e);
                const raycast_math::Segment g = raycast_math::segment(e, o, u, prm.t_min, prm.t_max);
                float p[3];
                raycast_math::sample(g.o_o, g.d_o, t_hit[i], p);
                pts4[row] = make_float4(p[0], p[1], p[2], 0.f);
                row_meta[row] = make_int2(i, mine);
            }
        }
    }
}

// One thread per jacobian row of a winner: its world normal
__global__ __launch_bounds__(RC_BLOCK) void k_raycast_normal(const float* __restrict__ rows, const int2* __restrict__ row_meta, int n_rows,
                                                             const float4* __restrict__ tab, int n_obj, int n_rays, float* __restrict__ normal) {
    const int r = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const int2 m = row_meta[r];
    if (m.x < 0 || m.x >= n_rays || m.y < 0 || m.y >= n_obj) return;
    const float4 g = *reinterpret_cast<const float4*>(rows + (size_t)r * GRAD_STRIDE + CODE_LEN);      // {gx, gy, gz, sdf}
    float e[16], nw[3];
    rc_entry(tab + 4 * (size_t)m.y, e);
    query_math::normal(e, g.x, g.y, g.z, nw);
    normal[3 * (size_t)m.x] = nw[0]; normal[3 * (size_t)m.x + 1] = nw[1]; normal[3 * (size_t)m.x + 2] = nw[2];
}

inline int rc_blocks(long long n) { return (int)((n + RC_BLOCK - 1) / RC_BLOCK); }

}  // namespace

hipError_t launch_raycast_count(const RaycastDev& d, int* wave_cnt, int* cnt, hipStream_t s) {
    if (d.n_rays <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_raycast_count, dim3(rc_blocks(d.n_rays)), dim3(RC_BLOCK), 0, s, d.org, d.dir, d.n_rays, reinterpret_cast<const float4*>(d.tab),
                       d.n_obj, d.n_waves, d.prm, wave_cnt, d.best, d.exh, d.dist);
    if (d.n_obj > 0) hipLaunchKernelGGL(k_raycast_scan, dim3(d.n_obj), dim3(RC_BLOCK), 0, s, wave_cnt, d.n_waves, cnt);
    return hipGetLastError();
}

hipError_t launch_raycast_fill(const RaycastDev& d, const RaycastPass& p, const int* wave_base, hipStream_t s) {
    if (d.n_rays <= 0 || p.nc <= 0 || p.n_slots <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_raycast_fill, dim3(rc_blocks(d.n_rays)), dim3(RC_BLOCK), 0, s, d.org, d.dir, d.n_rays, reinterpret_cast<const float4*>(d.tab), p.o0,
                       p.nc, p.pobj, d.n_waves, wave_base, d.prm, p.n_slots, p.pr_meta, p.pr_state, p.pr_t, p.pr_t1, p.pr_oo, p.pr_do);
    return hipGetLastError();
}

hipError_t launch_raycast_round_front(const RaycastDev& d, const RaycastPass& p, hipStream_t s) {
    if (p.n_slots <= 0) return hipSuccess;
    const int nw = p.n_slots / RC_WAVE;
    hipLaunchKernelGGL(k_raycast_live, dim3(rc_blocks(p.n_slots)), dim3(RC_BLOCK), 0, s, p.n_slots, p.pr_meta, p.pr_state, p.pr_t, d.n_rays, d.best,
                       p.live_cnt);
    hipLaunchKernelGGL(k_raycast_plan, dim3(1), dim3(RC_PLAN_BLOCK), 0, s, p.live_cnt, nw, p.ob, p.nc, p.wave_row, p.oinfo, p.ctrl, d.dstats);
    hipLaunchKernelGGL(k_raycast_emit, dim3(rc_blocks(p.n_slots)), dim3(RC_BLOCK), 0, s, p.n_slots, p.pr_state, p.pr_t, p.pr_oo, p.pr_do, p.wtab,
                       p.wave_row, p.oinfo, p.nc, nw, p.pts4, p.row_slot, p.tiles);
    return hipGetLastError();
}

hipError_t launch_raycast_step(const RaycastDev& d, const RaycastPass& p, const float* sdf, hipStream_t s) {
    if (p.n_slots <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_raycast_step, dim3(rc_blocks(p.n_slots)), dim3(RC_BLOCK), 0, s, sdf, p.row_slot, p.ctrl, p.n_slots, p.pr_meta, p.pr_state, p.pr_t,
                       p.pr_t1, p.pr_dist, reinterpret_cast<const float4*>(d.tab), d.n_obj, d.n_rays, d.prm, d.best);
    return hipGetLastError();
}

hipError_t launch_raycast_end(const RaycastDev& d, const RaycastPass& p, hipStream_t s) {
    if (p.n_slots <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_raycast_end, dim3(rc_blocks(p.n_slots)), dim3(RC_BLOCK), 0, s, p.n_slots, p.pr_meta, p.pr_state, p.pr_t, p.pr_dist, d.n_rays, d.best,
                       d.exh, d.dist, d.dstats);
    return hipGetLastError();
}

hipError_t launch_raycast_finish(const RaycastDev& d, hipStream_t s) {
    if (d.n_rays <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_raycast_finish, dim3(rc_blocks(d.n_rays)), dim3(RC_BLOCK), 0, s, d.best, d.exh, d.n_rays, d.obj, d.t, d.status, d.normal);
    return hipGetLastError();
}

hipError_t launch_raycast_wincount(const RaycastDev& d, int* wave_cnt, int* cnt, hipStream_t s) {
    if (d.n_rays <= 0 || d.n_obj <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_raycast_wincount, dim3(rc_blocks(d.n_rays)), dim3(RC_BLOCK), 0, s, d.obj, d.n_rays, d.n_obj, d.n_waves, wave_cnt);
    hipLaunchKernelGGL(k_raycast_scan, dim3(d.n_obj), dim3(RC_BLOCK), 0, s, wave_cnt, d.n_waves, cnt);
    return hipGetLastError();
}

hipError_t launch_raycast_winfill(const RaycastDev& d, int o0, int nc, const int* base, const int* wave_base, int n_rows, float4* pts4, int2* row_meta,
                                  hipStream_t s) {
    if (d.n_rays <= 0 || nc <= 0 || n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_raycast_winfill, dim3(rc_blocks(d.n_rays)), dim3(RC_BLOCK), 0, s, d.org, d.dir, d.obj, d.t, d.n_rays,
                       reinterpret_cast<const float4*>(d.tab), d.n_obj, o0, nc, base, d.n_waves, wave_base, d.prm, n_rows, pts4, row_meta);
    return hipGetLastError();
}

hipError_t launch_raycast_normal(const RaycastDev& d, const float* rows, const int2* row_meta, int n_rows, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_raycast_normal, dim3(rc_blocks(n_rows)), dim3(RC_BLOCK), 0, s, rows, row_meta, n_rows, reinterpret_cast<const float4*>(d.tab), d.n_obj,
                       d.n_rays, d.normal);
    return hipGetLastError();
}

// raycast_math.h compiled for the host in this translation unit, which has contraction off (the dsp_debug_raycast_* functions)
void raycast_segments_host(int64_t n_obj, const float* rt, const float* scale, int64_t n_rays, const float* org, const float* dir, float t_min, float t_max,
                           unsigned char* is_void, unsigned char* exists, float* t0, float* t1, float* o_o, float* d_o) {
    for (int64_t i = 0; i < n_rays; ++i) {
        float u[3] = {0.f, 0.f, 0.f};
        const bool ok = raycast_math::ray(org + 3 * i, dir + 3 * i, u);
        if (is_void) is_void[i] = ok ? 0 : 1;
        for (int64_t o = 0; o < n_obj; ++o) {
            float e[16] = {};
            memcpy(e, rt + 12 * o, 12 * sizeof(float));
            e[12] = e[13] = scale[o];
            const size_t k = (size_t)o * n_rays + i;
            raycast_math::Segment g{};
            if (ok) g = raycast_math::segment(e, org + 3 * i, u, t_min, t_max);
            if (exists) exists[k] = ok && g.exists ? 1 : 0;
            if (t0) t0[k] = ok ? g.t0 : 0.f;
            if (t1) t1[k] = ok ? g.t1 : 0.f;
            for (int c = 0; c < 3; ++c) {
                if (o_o) o_o[3 * k + c] = ok ? g.o_o[c] : 0.f;
                if (d_o) d_o[3 * k + c] = ok ? g.d_o[c] : 0.f;
            }
        }
    }
}

void raycast_step_host(int64_t n, const float* t, const float* t1, const float* sdf, const float* s, float eps, float relax, int32_t* decision,
                       float* dist, float* t_next) {
    for (int64_t i = 0; i < n; ++i) decision[i] = raycast_math::step(t[i], t1[i], sdf[i], s[i], eps, relax, dist + i, t_next + i);
}

const char* raycast_check_host(float t_min, float t_max, float eps, float relax, int max_steps) {
    return raycast_math::check(raycast_math::Params{t_min, t_max, eps, relax, max_steps});
}

}  // namespace dsp
