// The object map on the host: signed distance and normal of world points (dsp_map_query) and the alignment of a point cloud to the map
// (dsp_map_align), which runs the query's core; ray casting (dsp_map_raycast) and the alignment of depth rays to the map
// (dsp_map_align_rays), which runs the cast's core inside the alignment's hypothesis loop; the refinement of the objects' own poses against
// world-frame depth rays (dsp_map_align_objects), which runs the same loop with one correction per object; the refinement of the objects'
// shape codes against the same rays (dsp_map_align_shapes), a sibling loop whose state carries a code; with their C ABI.
#include "decoder_calls.h"
#include "decoder_pack.h"
#include "query_math.h"     // constants only: the arithmetic is compiled in query_kernels.hip (contraction off)
#include "align_math.h"     // constants only, likewise (align_kernels.hip; the ray alignment's arithmetic, align_rays_math.h, is compiled there too)
#include "align_shapes_math.h"      // constants only, likewise (align_shapes_kernels.hip)

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <stdexcept>
#include <vector>

namespace {

// ------------------------------------------------------------------------------------------------
// map query (dsp_map_query; arithmetic: query_math.h, kernels: query_kernels.hip)
// ------------------------------------------------------------------------------------------------

// Both budgets are fixed, whatever the device has free.  A chunk holds at most QUERY_CHUNK_BYTES of decoder output rows, counted as
// GRAD_STRIDE floats each in either decoder form (246 723 rows); a pass holds at most QUERY_PASS_PTS points, and fewer when the map is so
// large that n_obj x ceil(points / 64) wave counts would exceed QUERY_WAVECNT_BYTES (above 8192 objects).  QUERY_MAX_OBJ keeps a pass at
// 64 waves of points or more.
constexpr size_t QUERY_CHUNK_BYTES = (size_t)64 << 20;
constexpr size_t QUERY_WAVECNT_BYTES = (size_t)64 << 20;
constexpr int64_t QUERY_PASS_PTS = (int64_t)1 << 17;
constexpr int64_t QUERY_MAX_OBJ = (int64_t)1 << 18;
static_assert(QUERY_WAVECNT_BYTES / sizeof(int) / QUERY_MAX_OBJ >= 1, "a pass has at least one wave of points");

// what one chunk uploads; kept until the stream has been synchronised behind the chunk's launches
struct QueryChunk {
    int o0 = 0, nc = 0, n_rows = 0, nt = 0;     // objects [o0, o0 + nc) of the map, rows and tiles of the chunk
    std::vector<int> base;                      // per object of the chunk: chunk row of its first candidate (negative: the chunk starts inside it)
    std::vector<int4> tiles;                    // {first row, count, code-bias slot, 0}
    std::vector<int> slot_obj;                  // the object of each code-bias slot: the chunk's objects that have rows in it, ascending
    std::vector<float> cb;                      // code biases of the objects that have rows in the chunk, in slot order
};

// points of one pass: QUERY_PASS_PTS, and fewer (whole waves) where n_obj x waves counts would exceed QUERY_WAVECNT_BYTES.  1 <= n_obj <= QUERY_MAX_OBJ
int64_t query_pass_pts(int64_t n_obj) {
    return std::min<int64_t>(QUERY_PASS_PTS, (int64_t)(QUERY_WAVECNT_BYTES / sizeof(int) / (size_t)n_obj) * 64);
}

int64_t query_default_budget() { return (int64_t)(QUERY_CHUNK_BYTES / (GRAD_STRIDE * sizeof(float))); }

// The chunks of one pass from the objects' candidate counts: consecutive objects, or a range of one object's candidates, of at most `budget`
// rows.  Geometry only -- a function of (cnt, budget), no handle and no device (dsp_debug_query_plan); query_plan_codes fills cb.
std::vector<QueryChunk> query_plan_geometry(const int* cnt, int64_t n_obj, int64_t budget) {
    std::vector<QueryChunk> plan;
    int64_t o = 0, used = 0;                    // the next candidate without a chunk: candidate `used` of object o
    for (;;) {
        while (o < n_obj && used >= cnt[o]) { ++o; used = 0; }
        if (o == n_obj) break;
        plan.emplace_back();
        QueryChunk& c = plan.back();
        c.o0 = (int)o;
        int64_t rows = 0;
        int slot = 0;
        while (o < n_obj && rows < budget) {
            const int64_t take = std::min<int64_t>(cnt[o] - used, budget - rows);
            c.base.push_back((int)(rows - used));
            if (take > 0) {
                for (int64_t i = 0; i < take; i += TILE_PTS) c.tiles.push_back(make_int4((int)(rows + i), (int)std::min<int64_t>(TILE_PTS, take - i), slot, 0));
                c.slot_obj.push_back((int)o);
                ++slot;
            }
            rows += take;
            used += take;
            if (used < cnt[o]) break;           // the budget ends inside this object: the next chunk goes on from `used`
            ++o;
            used = 0;
        }
        c.nc = (int)c.base.size();
        c.n_rows = (int)rows;
        c.nt = (int)c.tiles.size();
    }
    return plan;
}

// the code biases of every chunk's slots
void query_plan_codes(const dsp_handle* h, const float* codes, std::vector<QueryChunk>& plan) {
    for (QueryChunk& c : plan) {
        c.cb.resize(c.slot_obj.size() * 2 * WIDTH);
        for (size_t slot = 0; slot < c.slot_obj.size(); ++slot)
            code_bias_host(h->h_codew, h->h_b0, h->h_blat, codes + (size_t)c.slot_obj[slot] * CODE_LEN, c.cb.data() + slot * 2 * WIDTH);
    }
}

std::vector<QueryChunk> query_plan(const dsp_handle* h, const float* codes, const std::vector<int>& cnt, int64_t budget) {
    std::vector<QueryChunk> plan = query_plan_geometry(cnt.data(), (int64_t)cnt.size(), budget);
    query_plan_codes(h, codes, plan);
    return plan;
}

// dsp_debug_query_timing: HIP events on the handle's stream around a whole call (first and last mark) and around every decoder launch (the
// pairs in between)
struct QueryTimer {
    bool on;
    hipStream_t s;
    std::vector<hipEvent_t> ev;
    ~QueryTimer() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    void mark() {
        if (!on) return;
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        ev.push_back(e);
        HIP_TRY(hipEventRecord(e, s));
    }
    // after the stream has been synchronised behind the last mark: ms2 = {decoder launches, whole call}
    void read(double* ms2) {
        ms2[0] = ms2[1] = 0.0;
        if (!on || ev.size() < 2) return;
        float ms = 0.f;
        for (size_t k = 1; k + 1 < ev.size(); k += 2) {
            HIP_TRY(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
            ms2[0] += ms;
        }
        HIP_TRY(hipEventElapsedTime(&ms, ev.front(), ev.back()));
        ms2[1] = ms;
    }
};

// the device arrays of one query: n_pts world points (packed float3) and the object table in, per-point results out
struct QueryDev {
    const float* pts;
    const float* tab;
    float* bound;
    unsigned long long* best;
    int* obj;
    float* dist;
    float* normal;              // null: no unit normals
};

// The device-resident query: passes, chunks, decoder launches, reduce and finish on the handle's stream, device arrays in and out.
// jacobian: the decoder's jacobian form (required by d.normal and by a hook that reads the rows' gradients).  behind_reduce (may be empty)
// is called behind every chunk's launch_query_reduce, while the chunk's rows (h->s_out) and row_meta are in place.  Synchronises once per
// pass (the counts' read-back); the caller synchronises behind it before `plan` (the last pass's uploads) dies.  stats4 += {rows, tiles,
// chunks, passes}.  n_pts > 0, n_obj > 0.
void query_core(dsp_handle* h, const float* codes, int64_t n_obj, int64_t n_pts, const QueryDev& d, bool jacobian, std::vector<QueryChunk>& plan,
                QueryTimer& timer, int64_t* stats4, const std::function<void(const QueryChunk&)>& behind_reduce) {
    const int64_t budget = h->q_chunk_rows > 0 ? h->q_chunk_rows : query_default_budget();
    const int64_t pass_pts = query_pass_pts(n_obj);
    std::vector<int> cnt((size_t)n_obj);
    h->q_cnt.ensure((size_t)n_obj);
    h->s_ntiles.ensure(1);
    h->s_clk.ensure(4);
    for (int64_t p0 = 0; p0 < n_pts; p0 += pass_pts) {
        const int n = (int)std::min(pass_pts, n_pts - p0);
        const int n_waves = (n + 63) / 64;
        h->q_wave_cnt.ensure((size_t)n_obj * n_waves);
        HIP_TRY(launch_query_count(d.pts, p0, n, d.tab, (int)n_obj, n_waves, h->q_wave_cnt.p, h->q_cnt.p, d.bound, d.best, h->stream));
        HIP_TRY(hipMemcpyAsync(cnt.data(), h->q_cnt.p, (size_t)n_obj * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));       // the counts; everything the previous pass uploaded has been consumed
        plan = query_plan(h, codes, cnt, budget);
        stats4[3] += 1;
        size_t max_rows = 0, max_nt = 0, max_nc = 0, max_cb = 0;
        for (const QueryChunk& c : plan) {
            max_rows = std::max<size_t>(max_rows, c.n_rows); max_nt = std::max<size_t>(max_nt, c.nt);
            max_nc = std::max<size_t>(max_nc, c.nc); max_cb = std::max(max_cb, c.cb.size());
        }
        if (plan.empty()) continue;
        h->s_pts.ensure(max_rows);
        h->s_out.ensure(max_rows * (jacobian ? GRAD_STRIDE : 1));
        h->q_row_meta.ensure(max_rows);
        h->s_tiles.ensure(max_nt);
        h->s_cbias.ensure(max_cb);
        h->q_base.ensure(max_nc);
        for (const QueryChunk& c : plan) {
            HIP_TRY(hipMemcpyAsync(h->s_cbias.p, c.cb.data(), c.cb.size() * 4, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->s_tiles.p, c.tiles.data(), c.nt * sizeof(int4), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->s_ntiles.p, &c.nt, 4, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->q_base.p, c.base.data(), c.nc * sizeof(int), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(launch_query_fill(d.pts, p0, n, d.tab, c.o0, c.nc, h->q_base.p, n_waves, h->q_wave_cnt.p, c.n_rows, h->s_pts.p,
                                      h->q_row_meta.p, h->stream));
            MlpArgs a = make_mlp_args(h, jacobian ? 2 : 0);
            a.n_tiles = h->s_ntiles.p;
            a.tiles = h->s_tiles.p;
            a.pts = h->s_pts.p;
            a.code_bias = h->s_cbias.p;
            a.code_bias_stride = 2 * WIDTH;
            a.out_sdf = h->s_out.p;
            a.out_grad = h->s_out.p;
            a.clk = h->s_clk.p;
            timer.mark();
            HIP_TRY(launch_mlp(jacobian ? 2 : 0, a, std::min(c.nt, h->n_cu), h->stream));
            timer.mark();
            HIP_TRY(launch_query_reduce(h->s_out.p, jacobian, h->q_row_meta.p, c.n_rows, d.tab, (int)n_obj, n_pts, d.best, d.normal, h->stream));
            if (behind_reduce) behind_reduce(c);
            stats4[0] += c.n_rows;
            stats4[1] += c.nt;
            stats4[2] += 1;
        }
    }
    HIP_TRY(launch_query_finish(d.best, n_pts, d.obj, d.dist, d.normal, h->stream));
}

// synchronises the stream when it goes: declared behind the call's device blocks and host uploads, so that it is destroyed before them,
// also when an allocation further down throws
struct SyncOnExit {
    hipStream_t s;
    ~SyncOnExit() { (void)hipStreamSynchronize(s); }
};

// tab: n_obj x query_math::OBJ_STRIDE floats (host).  Outputs are host arrays; normal null = the forward decoder form.  Upload, query_core,
// download; synchronises once per pass (the counts' read-back) and once at the end.
void query_run(dsp_handle* h, const std::vector<float>& tab, const float* codes, int64_t n_obj, const float* pts_world, int64_t n_pts, int32_t* obj,
               float* dist, float* bound, float* normal) {
    for (auto& c : h->q_stats) c = 0;
    if (n_pts == 0) return;
    if (n_obj == 0) {
        for (int64_t i = 0; i < n_pts; ++i) {
            obj[i] = -1;
            dist[i] = bound[i] = INFINITY;
            if (normal) normal[3 * i] = normal[3 * i + 1] = normal[3 * i + 2] = 0.f;
        }
        return;
    }
    HIP_TRY(hipSetDevice(h->device));
    DevBuf<float> q_pts, q_tab, q_bound, q_dist, q_normal;
    DevBuf<unsigned long long> q_best;
    DevBuf<int> q_obj;
    std::vector<QueryChunk> plan;   // the uploads of the pass in flight are copied from here
    SyncOnExit sync_on_exit{h->stream};
    QueryTimer timer{h->q_timing, h->stream, {}};
    h->q_ms[0] = h->q_ms[1] = 0.0;
    timer.mark();
    q_pts.alloc((size_t)n_pts * 3);
    q_tab.alloc(tab.size());
    q_bound.alloc((size_t)n_pts);
    q_dist.alloc((size_t)n_pts);
    q_obj.alloc((size_t)n_pts);
    q_best.alloc((size_t)n_pts);
    if (normal) q_normal.alloc((size_t)n_pts * 3);
    HIP_TRY(hipMemcpyAsync(q_pts.p, pts_world, (size_t)n_pts * 12, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(q_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->stream));
    const QueryDev d{q_pts.p, q_tab.p, q_bound.p, q_best.p, q_obj.p, q_dist.p, normal ? q_normal.p : nullptr};
    query_core(h, codes, n_obj, n_pts, d, normal != nullptr, plan, timer, h->q_stats, {});
    HIP_TRY(hipMemcpyAsync(obj, q_obj.p, (size_t)n_pts * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(dist, q_dist.p, (size_t)n_pts * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(bound, q_bound.p, (size_t)n_pts * 4, hipMemcpyDeviceToHost, h->stream));
    if (normal) HIP_TRY(hipMemcpyAsync(normal, q_normal.p, (size_t)n_pts * 12, hipMemcpyDeviceToHost, h->stream));
    timer.mark();
    HIP_TRY(hipStreamSynchronize(h->stream));           // `plan` (the last pass's uploads) lives until here
    HIP_TRY(hipGetLastError());
    timer.read(h->q_ms);
}

// the map's host table (query_math::OBJ_STRIDE floats per object) as dsp_map_query and dsp_map_align check and build it
std::vector<float> query_table(const dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj) {
    if (n_obj > QUERY_MAX_OBJ) throw std::invalid_argument("map query too large (split the request)");
    std::vector<float> tab((size_t)n_obj * query_math::OBJ_STRIDE, 0.f);
    for (int64_t o = 0; o < n_obj; ++o) {
        float* e = tab.data() + o * query_math::OBJ_STRIDE;
        if (!query_invert_host(t_world_obj + 16 * o, e, e + 12))
            throw std::invalid_argument("t_world_obj: a pose is not a finite Sim(3) (rotation times a positive scale, bottom row 0 0 0 1)");
        // an object whose code is not finite never wins: the decoder's ReLUs may turn it into finite values, so its distances are made NaN
        bool code_ok = true;
        for (int k = 0; k < h->code_len; ++k) code_ok = code_ok && std::isfinite(codes[o * CODE_LEN + k]);
        e[13] = code_ok ? e[12] : std::nanf("");
    }
    return tab;
}

// ------------------------------------------------------------------------------------------------
// ray casting (dsp_map_raycast; arithmetic: raycast_math.h, kernels: raycast_kernels.hip)
// ------------------------------------------------------------------------------------------------

// The code biases of ALL objects of a call live in one device table (4 KiB per object) of at most RAYCAST_CBIAS_BYTES: 16 384 objects.  The
// pair counts per (object, wave of rays) share the query's budget QUERY_WAVECNT_BYTES.  Both fixed, whatever the device has free.
constexpr size_t RAYCAST_CBIAS_BYTES = (size_t)64 << 20;
constexpr int RAYCAST_POLL_ROUNDS = 8;      // the host reads the live count back every so many rounds to stop enqueueing early

// what one pass uploads (RaycastPass, dsp_internal.h); kept until the stream has been synchronised behind the pass's launches
struct RaycastPassHost {
    int o0 = 0, nc = 0, n_slots = 0;
    std::vector<int4> pobj, ob;
    std::vector<int2> wtab;
};

// The passes of a call from the objects' pair counts: the chunks of query_plan_geometry -- consecutive objects, or a range of one object's
// pairs, of at most `budget` pairs -- with every object's pairs padded to whole waves of slots.
std::vector<RaycastPassHost> raycast_passes(const int* cnt, int64_t n_obj, int64_t budget) {
    std::vector<RaycastPassHost> passes;
    for (const QueryChunk& c : query_plan_geometry(cnt, n_obj, budget)) {
        passes.emplace_back();
        RaycastPassHost& p = passes.back();
        p.o0 = c.o0;
        p.nc = c.nc;
        int slots = 0;
        for (int k = 0; k < c.nc; ++k) {
            const int lo = std::max(0, -c.base[k]);
            const int hi = std::max(lo, (int)std::min<int64_t>(cnt[c.o0 + k], (int64_t)c.n_rows - c.base[k]));
            const int waves = (hi - lo + 63) / 64;
            p.pobj.push_back(make_int4(slots - lo, lo, hi, 0));
            p.ob.push_back(make_int4(slots / 64, waves, c.o0 + k, 0));
            for (int w = 0; w < waves; ++w) p.wtab.push_back(make_int2(k, slots / 64));
            slots += waves * 64;
        }
        p.n_slots = slots;
    }
    return passes;
}

// nullptr, or why a cast of n_rays rays against n_obj objects is refused: its tables would exceed the fixed budgets above
const char* raycast_check_size(int64_t n_obj, int64_t n_rays) {
    const int64_t n_waves = (n_rays + 63) / 64;
    if (n_obj > 0 && n_rays > 0 &&
        ((size_t)n_obj * 2 * WIDTH * sizeof(float) > RAYCAST_CBIAS_BYTES || (size_t)n_obj * (size_t)n_waves * sizeof(int) > QUERY_WAVECNT_BYTES))
        return "raycast: objects x rays too large (split the request)";
    return nullptr;
}

// The device blocks and the host uploads of a cast.  They belong to the caller and live until the stream has been synchronised behind the
// cast; a caller that casts again (dsp_map_align_rays, once per evaluation) reuses them.  The answers stay on the device: r_obj, r_t,
// r_dist, r_status per ray.
struct RaycastWork {
    DevBuf<float> r_t, r_dist, p_t, p_t1, p_dist, p_out, n_out;
    DevBuf<unsigned long long> r_best, r_dstats;
    DevBuf<unsigned> r_exh;
    DevBuf<int> r_obj, r_status, r_wave_cnt, r_cnt, p_state, p_live, p_wrow, p_ctrl, p_rslot, n_base, n_ntiles;
    DevBuf<int2> p_wtab, p_meta, n_meta;
    DevBuf<int4> p_pobj, p_ob, p_oinfo, p_tiles, n_tiles;
    DevBuf<float4> p_oo, p_do, p_pts, n_pts;
    std::vector<int> cnt;
    std::vector<RaycastPassHost> passes;        // the uploads of the passes in flight are copied from here ...
    std::vector<QueryChunk> plan;               // ... and those of the winners' chunks from here
    unsigned long long dstats[4] = {0, 0, 0, 0};
};

using RaycastRows = std::function<void(const RaycastDev&, const float* rows, const int2* row_meta, int n_rows)>;

// The device-resident cast: n_rays world rays (org, dir: packed float3), the object table and the code biases of all objects (2 * WIDTH floats
// each) on the device in; the answers in w.r_* on the device.  behind_rows (may be empty: no winner rows are decoded) is called behind every
// chunk of the winners' jacobian rows -- the hit samples grouped by object in ascending ray order -- with row_meta = {ray, object}.  normal
// (may be null) is only zeroed here where a ray has no winner.  Synchronises for the pair counts, the live polls and the winners' counts; the
// caller synchronises behind it before w's uploads die, then calls raycast_core_stats.  stats6[0], [4] += pairs, passes.  n_rays, n_obj > 0.
void raycast_core(dsp_handle* h, RaycastWork& w, const float* org, const float* dir, const float* tab, const float* cbias, int64_t n_obj, int64_t n_rays,
                  const raycast_math::Params& prm, float* normal, QueryTimer& timer, int64_t* stats6, const RaycastRows& behind_rows) {
    const int64_t n_waves = (n_rays + 63) / 64;
    const int64_t budget = h->q_chunk_rows > 0 ? h->q_chunk_rows : query_default_budget();
    w.cnt.resize((size_t)n_obj);
    w.r_best.ensure((size_t)n_rays);
    w.r_exh.ensure((size_t)n_rays);
    w.r_obj.ensure((size_t)n_rays);
    w.r_t.ensure((size_t)n_rays);
    w.r_dist.ensure((size_t)n_rays);
    w.r_status.ensure((size_t)n_rays);
    w.r_dstats.ensure(4);
    w.r_wave_cnt.ensure((size_t)n_obj * n_waves);
    w.r_cnt.ensure((size_t)n_obj);
    h->s_clk.ensure(4);
    HIP_TRY(hipMemsetAsync(w.r_dstats.p, 0, sizeof w.dstats, h->stream));
    const RaycastDev d{org, dir, tab, (int)n_rays, (int)n_obj, (int)n_waves, prm, w.r_best.p, w.r_exh.p, w.r_obj.p, w.r_t.p, w.r_dist.p, w.r_status.p,
                       normal, w.r_dstats.p};
    HIP_TRY(launch_raycast_count(d, w.r_wave_cnt.p, w.r_cnt.p, h->stream));
    HIP_TRY(hipMemcpyAsync(w.cnt.data(), w.r_cnt.p, (size_t)n_obj * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));           // the pair counts, once per cast
    w.passes = raycast_passes(w.cnt.data(), n_obj, budget);
    for (int c : w.cnt) stats6[0] += c;
    stats6[4] += (int64_t)w.passes.size();
    size_t max_slots = 0, max_nc = 0;
    for (const RaycastPassHost& p : w.passes) { max_slots = std::max<size_t>(max_slots, p.n_slots); max_nc = std::max<size_t>(max_nc, p.nc); }
    if (!w.passes.empty()) {
        w.p_pobj.ensure(max_nc); w.p_ob.ensure(max_nc); w.p_oinfo.ensure(max_nc);
        w.p_wtab.ensure(max_slots / 64); w.p_live.ensure(max_slots / 64); w.p_wrow.ensure(max_slots / 64); w.p_tiles.ensure(max_slots / 64);
        w.p_meta.ensure(max_slots); w.p_state.ensure(max_slots); w.p_t.ensure(max_slots); w.p_t1.ensure(max_slots); w.p_dist.ensure(max_slots);
        w.p_oo.ensure(max_slots); w.p_do.ensure(max_slots); w.p_pts.ensure(max_slots); w.p_rslot.ensure(max_slots); w.p_out.ensure(max_slots);
        w.p_ctrl.ensure(2);
    }
    for (const RaycastPassHost& ph : w.passes) {
        if (ph.n_slots <= 0) continue;
        const RaycastPass p{ph.o0, ph.nc, ph.n_slots, w.p_pobj.p, w.p_ob.p, w.p_wtab.p, w.p_meta.p, w.p_state.p, w.p_t.p, w.p_t1.p, w.p_dist.p, w.p_oo.p,
                            w.p_do.p, w.p_live.p, w.p_wrow.p, w.p_oinfo.p, w.p_ctrl.p, w.p_pts.p, w.p_rslot.p, w.p_tiles.p};
        HIP_TRY(hipMemcpyAsync(w.p_pobj.p, ph.pobj.data(), ph.pobj.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(w.p_ob.p, ph.ob.data(), ph.ob.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(w.p_wtab.p, ph.wtab.data(), ph.wtab.size() * sizeof(int2), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemsetAsync(w.p_state.p, 0xff, (size_t)ph.n_slots * sizeof(int), h->stream));       // padding: neither live nor hit
        HIP_TRY(hipMemsetAsync(w.p_meta.p, 0xff, (size_t)ph.n_slots * sizeof(int2), h->stream));
        HIP_TRY(launch_raycast_fill(d, p, w.r_wave_cnt.p, h->stream));
        MlpArgs a = make_mlp_args(h, 0);
        a.n_tiles = w.p_ctrl.p;
        a.tiles = w.p_tiles.p;
        a.pts = w.p_pts.p;
        a.code_bias = cbias;
        a.code_bias_stride = 2 * WIDTH;
        a.out_sdf = w.p_out.p;
        a.out_grad = w.p_out.p;
        a.clk = h->s_clk.p;
        const int grid = std::min(ph.n_slots / 64, h->n_cu);
        for (int round = 0; round < prm.max_steps; ++round) {
            HIP_TRY(launch_raycast_round_front(d, p, h->stream));
            timer.mark();
            HIP_TRY(launch_mlp(0, a, grid, h->stream));
            timer.mark();
            HIP_TRY(launch_raycast_step(d, p, w.p_out.p, h->stream));
            if ((round + 1) % RAYCAST_POLL_ROUNDS == 0 && round + 1 < prm.max_steps) {
                int live = 0;
                HIP_TRY(hipMemcpyAsync(&live, w.p_ctrl.p + 1, sizeof live, hipMemcpyDeviceToHost, h->stream));
                HIP_TRY(hipStreamSynchronize(h->stream));
                if (live == 0) break;           // the round just run decoded nothing: no later one would
            }
        }
        HIP_TRY(launch_raycast_end(d, p, h->stream));
    }
    HIP_TRY(launch_raycast_finish(d, h->stream));
    if (behind_rows) {  // the winners' hit samples through the jacobian form, grouped by object in ascending ray order
        HIP_TRY(launch_raycast_wincount(d, w.r_wave_cnt.p, w.r_cnt.p, h->stream));
        HIP_TRY(hipMemcpyAsync(w.cnt.data(), w.r_cnt.p, (size_t)n_obj * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        w.plan = query_plan_geometry(w.cnt.data(), n_obj, budget);
        size_t max_rows = 0, max_nt = 0, max_base = 0;
        for (QueryChunk& c : w.plan) {
            for (int4& tile : c.tiles) tile.z = c.slot_obj[tile.z];        // the slot of the call's code-bias table: the object itself
            max_rows = std::max<size_t>(max_rows, c.n_rows); max_nt = std::max<size_t>(max_nt, c.nt); max_base = std::max<size_t>(max_base, c.nc);
        }
        if (!w.plan.empty()) {
            w.n_pts.ensure(max_rows); w.n_out.ensure(max_rows * GRAD_STRIDE); w.n_meta.ensure(max_rows); w.n_tiles.ensure(max_nt); w.n_base.ensure(max_base);
            w.n_ntiles.ensure(1);
        }
        for (const QueryChunk& c : w.plan) {
            HIP_TRY(hipMemcpyAsync(w.n_tiles.p, c.tiles.data(), c.nt * sizeof(int4), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(w.n_ntiles.p, &c.nt, 4, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(w.n_base.p, c.base.data(), c.nc * sizeof(int), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(launch_raycast_winfill(d, c.o0, c.nc, w.n_base.p, w.r_wave_cnt.p, c.n_rows, w.n_pts.p, w.n_meta.p, h->stream));
            MlpArgs a = make_mlp_args(h, 2);
            a.n_tiles = w.n_ntiles.p;
            a.tiles = w.n_tiles.p;
            a.pts = w.n_pts.p;
            a.code_bias = cbias;
            a.code_bias_stride = 2 * WIDTH;
            a.out_sdf = w.n_out.p;
            a.out_grad = w.n_out.p;
            a.clk = h->s_clk.p;
            timer.mark();
            HIP_TRY(launch_mlp(2, a, std::min(c.nt, h->n_cu), h->stream));
            timer.mark();
            behind_rows(d, w.n_out.p, w.n_meta.p, c.n_rows);
        }
    }
    HIP_TRY(hipMemcpyAsync(w.dstats, w.r_dstats.p, sizeof w.dstats, hipMemcpyDeviceToHost, h->stream));
}

// behind the synchronisation that follows raycast_core: stats6[1], [2], [3], [5] += decoder rows, tiles, rounds, exhausted pairs
void raycast_core_stats(const RaycastWork& w, int64_t* stats6) {
    stats6[1] += (int64_t)w.dstats[0];
    stats6[2] += (int64_t)w.dstats[1];
    stats6[3] += (int64_t)w.dstats[2];
    stats6[5] += (int64_t)w.dstats[3];
}

// the code biases of all objects of a call: 2 * WIDTH floats each
std::vector<float> raycast_code_biases(const dsp_handle* h, const float* codes, int64_t n_obj) {
    std::vector<float> cb((size_t)n_obj * 2 * WIDTH);
    for (int64_t o = 0; o < n_obj; ++o) code_bias_host(h->h_codew, h->h_b0, h->h_blat, codes + (size_t)o * CODE_LEN, cb.data() + (size_t)o * 2 * WIDTH);
    return cb;
}

// dsp_map_raycast: host rays up, raycast_core, host answers down
void raycast_run(dsp_handle* h, const std::vector<float>& tab, const float* codes, int64_t n_obj, const float* org, const float* dir, int64_t n_rays,
                 const raycast_math::Params& prm, int32_t* obj, float* t, float* dist, int32_t* status, float* normal) {
    for (auto& c : h->r_stats) c = 0;
    if (n_rays == 0) return;
    if (n_obj == 0) {
        for (int64_t i = 0; i < n_rays; ++i) {
            obj[i] = -1;
            t[i] = dist[i] = INFINITY;
            status[i] = raycast_math::STATUS_MISS;
            if (normal) normal[3 * i] = normal[3 * i + 1] = normal[3 * i + 2] = 0.f;
        }
        return;
    }
    if (const char* why = raycast_check_size(n_obj, n_rays)) throw std::invalid_argument(why);
    HIP_TRY(hipSetDevice(h->device));
    DevBuf<float> r_org, r_dir, r_tab, r_normal, r_cb;
    RaycastWork w;
    std::vector<float> cb;
    SyncOnExit sync_on_exit{h->stream};
    QueryTimer timer{h->q_timing, h->stream, {}};
    h->q_ms[0] = h->q_ms[1] = 0.0;
    timer.mark();
    cb = raycast_code_biases(h, codes, n_obj);
    r_org.alloc((size_t)n_rays * 3);
    r_dir.alloc((size_t)n_rays * 3);
    r_tab.alloc(tab.size());
    r_cb.alloc(cb.size());
    if (normal) r_normal.alloc((size_t)n_rays * 3);
    HIP_TRY(hipMemcpyAsync(r_org.p, org, (size_t)n_rays * 12, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(r_dir.p, dir, (size_t)n_rays * 12, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(r_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(r_cb.p, cb.data(), cb.size() * 4, hipMemcpyHostToDevice, h->stream));
    RaycastRows normals;
    if (normal)
        normals = [&](const RaycastDev& d, const float* rows, const int2* row_meta, int n_rows) {
            HIP_TRY(launch_raycast_normal(d, rows, row_meta, n_rows, h->stream));
        };
    raycast_core(h, w, r_org.p, r_dir.p, r_tab.p, r_cb.p, n_obj, n_rays, prm, normal ? r_normal.p : nullptr, timer, h->r_stats, normals);
    HIP_TRY(hipMemcpyAsync(obj, w.r_obj.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(t, w.r_t.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(dist, w.r_dist.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(status, w.r_status.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
    if (normal) HIP_TRY(hipMemcpyAsync(normal, r_normal.p, (size_t)n_rays * 12, hipMemcpyDeviceToHost, h->stream));
    timer.mark();
    HIP_TRY(hipStreamSynchronize(h->stream));           // w's uploads live until here
    HIP_TRY(hipGetLastError());
    timer.read(h->q_ms);
    raycast_core_stats(w, h->r_stats);
}

raycast_math::Params raycast_params(const dsp_raycast_params& p) { return raycast_math::Params{p.t_min, p.t_max, p.eps, p.relax, p.max_steps}; }

// ------------------------------------------------------------------------------------------------
// map alignment (dsp_map_align; arithmetic: align_math.h, kernels: align_kernels.hip)
// ------------------------------------------------------------------------------------------------

const char* align_check_params(const dsp_align_params& p) {
    if (p.iterations < 1) return "align: iterations must be >= 1";
    if (p.min_points < 6) return "align: min_points must be >= 6";
    if (!std::isfinite(p.max_dist) || !std::isfinite(p.huber) || !(p.huber > 0.0) || !(p.huber <= p.max_dist)) return "align: 0 < huber <= max_dist, both finite";
    if (!std::isfinite(p.damp) || p.damp < 0.0) return "align: damp must be finite and >= 0";
    if (!(p.trans_tol >= 0.0) || !(p.rot_tol >= 0.0)) return "align: the tolerances must be >= 0";
    const step_rule::Params sp{p.lambda0, p.up, p.down, p.lambda_min, p.lambda_max};
    return step_rule::is_off(sp) ? nullptr : step_rule::check(sp);
}

// what dsp_map_align refuses before it touches the device, besides the map: nullptr, or what is wrong
const char* align_check_inputs(const dsp_align_params& p, const double* T0, int64_t n_hyp, const float* weights, int64_t n_pts) {
    if (const char* why = align_check_params(p)) return why;
    if (n_hyp > 0 && n_pts > (int64_t)0x7fffffff / n_hyp) return "align: n_hyp x n_pts exceeds 2^31 - 1 (split the request)";
    float rt[12];
    for (int64_t k = 0; k < n_hyp; ++k)
        if (!align_check_pose_host(T0 + 16 * k, rt)) return "t_world_sensor0: a pose is not a finite rigid transform (rotation, unit scale, bottom row 0 0 0 1)";
    if (weights)
        for (int64_t i = 0; i < n_pts; ++i)
            if (!(weights[i] >= 0.f) || !std::isfinite(weights[i])) return "align: weights must be finite and >= 0";
    return nullptr;
}

// one hypothesis on the host: the accepted state with its sums, and the pose to evaluate next
struct AlignHyp {
    double T_acc[16], T_eval[16];
    double S[align_math::NSUM];         // the sums at T_acc
    double F_acc = 0.0, F0 = 0.0, lam = 0.0;
    bool live = true, has_acc = false;
    int status = DSP_ALIGN_OK, evals = 0, steps = 0;
};

void align_write(const AlignHyp& a, double* T_out, double* rec) {
    memcpy(T_out, a.T_acc, sizeof a.T_acc);
    rec[0] = a.status; rec[1] = a.evals; rec[2] = a.steps; rec[3] = a.F0; rec[4] = a.F_acc;
    rec[5] = a.S[align_math::IDX_N]; rec[6] = a.S[align_math::IDX_W]; rec[7] = a.lam;
    int k = align_math::IDX_H;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) rec[8 + 6 * i + j] = rec[8 + 6 * j + i] = a.S[k++];
    for (int i = 0; i < 6; ++i) rec[44 + i] = a.S[align_math::IDX_B + i];
}

std::vector<AlignHyp> align_start(const double* T0, int64_t n_hyp) {
    std::vector<AlignHyp> hyp((size_t)n_hyp);
    for (int64_t k = 0; k < n_hyp; ++k) {
        memcpy(hyp[k].T_acc, T0 + 16 * k, sizeof hyp[k].T_acc);
        memcpy(hyp[k].T_eval, T0 + 16 * k, sizeof hyp[k].T_eval);
        for (double& s : hyp[k].S) s = 0.0;
    }
    return hyp;
}

// nothing to evaluate: no support at the input pose
void align_write_no_support(std::vector<AlignHyp>& hyp, const dsp_align_params& prm, double* T_out, double* record) {
    double zero[align_math::NSUM] = {};
    for (size_t k = 0; k < hyp.size(); ++k) {
        hyp[k].status = DSP_ALIGN_NO_SUPPORT;
        hyp[k].F0 = hyp[k].F_acc = align_cost_host(zero, prm.huber, prm.max_dist);
        align_write(hyp[k], T_out + 16 * k, record + (size_t)DSP_ALIGN_RECORD * k);
    }
}

// The hypothesis loop of dsp_map_align and dsp_map_align_rays: statuses, step control, convergence rule, Cholesky and exp_se3; the step lives
// on the host.  evaluate(hyp_tab, sums) runs one evaluation of every live hypothesis at the fp32 poses of hyp_tab (ALIGN_HYP_STRIDE floats
// per hypothesis; it uploads them) and returns with align_math::NSUM sums per hypothesis on the host and the stream idle; it may end a
// hypothesis itself (live = false and a status: dsp_map_align_objects, whose trial pose the map may refuse), which is then skipped.
// accepted(k) (may be empty) is called when hypothesis k's evaluation becomes its returned state.  *n_evals += 1 per evaluation.
void align_loop(std::vector<AlignHyp>& hyp, const dsp_align_params& prm, double* trace, int64_t* n_evals,
                const std::function<void(const std::vector<float>&, std::vector<double>&)>& evaluate, const std::function<void(int64_t)>& accepted) {
    constexpr int NS = align_math::NSUM;
    const int64_t n_hyp = (int64_t)hyp.size();
    const step_rule::Params sp{prm.lambda0, prm.up, prm.down, prm.lambda_min, prm.lambda_max};
    const bool step_on = !step_rule::is_off(sp);
    const int iters = prm.iterations;
    std::vector<float> hyp_tab((size_t)n_hyp * ALIGN_HYP_STRIDE, 0.f);
    std::vector<double> sums((size_t)n_hyp * NS, 0.0);
    auto end = [](AlignHyp& a, int status) { a.live = false; a.status = status; };
    for (int e = 0; e < iters; ++e) {
        bool any = false;
        for (int64_t k = 0; k < n_hyp; ++k) {   // the stream is idle here: the previous evaluation's read-back has been waited for
            float* t = hyp_tab.data() + k * ALIGN_HYP_STRIDE;
            for (int i = 0; i < 12; ++i) t[i] = (float)hyp[k].T_eval[i];
            t[12] = hyp[k].live ? 1.f : 0.f;
            any = any || hyp[k].live;
        }
        if (!any) break;
        evaluate(hyp_tab, sums);
        *n_evals += 1;
        for (int64_t k = 0; k < n_hyp; ++k) {
            AlignHyp& a = hyp[k];
            if (!a.live) continue;
            const double* S = sums.data() + k * NS;
            const double F = align_cost_host(S, prm.huber, prm.max_dist);
            const bool support = S[align_math::IDX_N] >= (double)prm.min_points;
            double* tr = trace ? trace + ((size_t)k * iters + e) * DSP_ALIGN_TRACE : nullptr;
            a.evals += 1;
            if (e == 0) a.F0 = F;
            int dec = step_rule::ACCEPTED;
            if (step_on)
                dec = !a.has_acc ? step_rule::decide(true, F, 0.0, sp, a.lam)
                                 : step_rule::decide(false, support ? F : (double)INFINITY, a.F_acc, sp, a.lam);
            if (dec == step_rule::ACCEPTED) {
                if (a.has_acc) a.steps += 1;
                memcpy(a.T_acc, a.T_eval, sizeof a.T_acc);
                memcpy(a.S, S, sizeof a.S);
                a.F_acc = F;
                a.has_acc = true;
                if (accepted) accepted(k);      // the per-observation outputs belong to the returned state
            }
            if (tr) {
                memcpy(tr, a.T_eval, sizeof a.T_eval);
                tr[16] = dec; tr[17] = F; tr[18] = a.lam; tr[19] = S[align_math::IDX_N];
                memcpy(tr + 20, S, 27 * sizeof(double));
            }
            // the step from the accepted state
            if (a.S[align_math::IDX_N] < (double)prm.min_points) { end(a, DSP_ALIGN_NO_SUPPORT); continue; }
            double H[36], xi[6];
            int q = align_math::IDX_H;
            for (int i = 0; i < 6; ++i)
                for (int j = i; j < 6; ++j) H[6 * i + j] = H[6 * j + i] = a.S[q++];
            bool solved = false;
            for (int tries = 0; !solved; ++tries) {
                solved = align_solve_host(H, a.S + align_math::IDX_B, prm.damp, a.lam, xi);
                if (solved || !step_on || tries >= 64 || !(a.lam < sp.lambda_max)) break;
                a.lam = fmin(fmax(a.lam, sp.lambda_min) * sp.up, sp.lambda_max);        // a failed factorisation: lambda grows like after a rejection
            }
            if (tr) tr[18] = a.lam;
            if (!solved) { end(a, DSP_ALIGN_SINGULAR); continue; }
            if (tr) memcpy(tr + 47, xi, sizeof xi);
            const double mv = fmax(fmax(fabs(xi[0]), fabs(xi[1])), fabs(xi[2])), mw = fmax(fmax(fabs(xi[3]), fabs(xi[4])), fabs(xi[5]));
            if (mv < prm.trans_tol && mw < prm.rot_tol) { end(a, DSP_ALIGN_CONVERGED); continue; }
            if (e == iters - 1) { end(a, DSP_ALIGN_OK); continue; }
            align_apply_step_host(xi, a.T_acc, a.T_eval);
        }
    }
}

// Points and weights are uploaded once; per evaluation the host sends the hypotheses' fp32 poses and reads the query's candidate counts
// (once per pass) and align_math::NSUM doubles per hypothesis.
void align_run(dsp_handle* h, const std::vector<float>& tab, const float* codes, int64_t n_obj, const float* pts, const float* weights, int64_t n_pts,
               const double* T0, int64_t n_hyp, const dsp_align_params& prm, double* T_out, double* record, int32_t* obj, float* dist, double* trace) {
    constexpr int NS = align_math::NSUM;
    for (auto& c : h->a_stats) c = 0;
    std::vector<AlignHyp> hyp = align_start(T0, n_hyp);
    if (trace) std::fill(trace, trace + (size_t)n_hyp * prm.iterations * DSP_ALIGN_TRACE, 0.0);
    if (n_hyp == 0) return;
    if (n_pts == 0 || n_obj == 0) {
        align_write_no_support(hyp, prm, T_out, record);
        if (obj)
            for (int64_t r = 0; r < n_hyp * n_pts; ++r) { obj[r] = -1; dist[r] = INFINITY; }
        return;
    }
    HIP_TRY(hipSetDevice(h->device));
    const int64_t n_rows = n_hyp * n_pts, nb = align_gram_blocks(n_pts);
    DevBuf<float> a_pts, a_w, a_hyp, a_grad, q_tab, q_pw, q_bound, q_dist, r_dist;
    DevBuf<unsigned long long> q_best;
    DevBuf<int> q_obj, r_obj;
    DevBuf<double> a_slab, a_sums;
    std::vector<QueryChunk> plan;               // the uploads of the pass in flight are copied from here
    SyncOnExit sync_on_exit{h->stream};
    QueryTimer timer{h->q_timing, h->stream, {}};
    h->q_ms[0] = h->q_ms[1] = 0.0;
    timer.mark();
    a_pts.alloc((size_t)n_pts * 3);
    if (weights) a_w.alloc((size_t)n_pts);
    a_hyp.alloc((size_t)n_hyp * ALIGN_HYP_STRIDE);
    a_grad.alloc((size_t)n_rows * 3);
    q_tab.alloc(tab.size());
    q_pw.alloc((size_t)n_rows * 3);
    q_bound.alloc((size_t)n_rows);
    q_dist.alloc((size_t)n_rows);
    q_obj.alloc((size_t)n_rows);
    q_best.alloc((size_t)n_rows);
    if (obj) { r_obj.alloc((size_t)n_rows); r_dist.alloc((size_t)n_rows); }
    a_slab.alloc((size_t)n_hyp * nb * NS);
    a_sums.alloc((size_t)n_hyp * NS);
    HIP_TRY(hipMemcpyAsync(a_pts.p, pts, (size_t)n_pts * 12, hipMemcpyHostToDevice, h->stream));
    if (weights) HIP_TRY(hipMemcpyAsync(a_w.p, weights, (size_t)n_pts * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(q_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->stream));
    const QueryDev d{q_pw.p, q_tab.p, q_bound.p, q_best.p, q_obj.p, q_dist.p, nullptr};
    const std::function<void(const QueryChunk&)> winner = [&](const QueryChunk& c) {
        HIP_TRY(launch_align_winner(h->s_out.p, h->q_row_meta.p, c.n_rows, q_tab.p, (int)n_obj, n_rows, q_best.p, a_grad.p, h->stream));
    };
    align_loop(hyp, prm, trace, &h->a_stats[4],
               [&](const std::vector<float>& hyp_tab, std::vector<double>& sums) {
                   HIP_TRY(hipMemcpyAsync(a_hyp.p, hyp_tab.data(), hyp_tab.size() * 4, hipMemcpyHostToDevice, h->stream));
                   HIP_TRY(launch_align_transform(a_pts.p, n_pts, a_hyp.p, 0, n_rows, q_pw.p, h->stream));
                   query_core(h, codes, n_obj, n_rows, d, true, plan, timer, h->a_stats, winner);
                   HIP_TRY(launch_align_gram(q_pw.p, q_obj.p, q_dist.p, a_grad.p, weights ? a_w.p : nullptr, n_pts, (int)n_hyp, a_hyp.p, prm.huber,
                                             prm.max_dist, a_slab.p, a_sums.p, h->stream));
                   HIP_TRY(hipMemcpyAsync(sums.data(), a_sums.p, sums.size() * 8, hipMemcpyDeviceToHost, h->stream));
                   HIP_TRY(hipStreamSynchronize(h->stream));    // the sums; `plan` and hyp_tab have been consumed
               },
               [&](int64_t k) {
                   if (!obj) return;
                   HIP_TRY(hipMemcpyAsync(r_obj.p + k * n_pts, q_obj.p + k * n_pts, (size_t)n_pts * 4, hipMemcpyDeviceToDevice, h->stream));
                   HIP_TRY(hipMemcpyAsync(r_dist.p + k * n_pts, q_dist.p + k * n_pts, (size_t)n_pts * 4, hipMemcpyDeviceToDevice, h->stream));
               });
    if (obj) {
        HIP_TRY(hipMemcpyAsync(obj, r_obj.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(dist, r_dist.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, h->stream));
    }
    timer.mark();
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    timer.read(h->q_ms);
    for (int64_t k = 0; k < n_hyp; ++k) align_write(hyp[k], T_out + 16 * k, record + (size_t)DSP_ALIGN_RECORD * k);
}

// ------------------------------------------------------------------------------------------------
// ray alignment (dsp_map_align_rays; arithmetic: align_rays_math.h, kernels: align_kernels.hip)
// ------------------------------------------------------------------------------------------------

// the default gate on the along-ray gap in units of max_dist (profiles/map_align_rays.md: the sweep behind it)
constexpr double ALIGN_RAYS_GAP_FACTOR = 2.0;

// what dsp_map_align_rays refuses before it touches the device, besides the map: nullptr, or what is wrong
const char* align_rays_check_inputs(const dsp_align_params& p, const dsp_raycast_params& rp, double max_gap, const double* T0, int64_t n_hyp,
                                    const float* weights, int64_t n_rays, int64_t n_obj) {
    if (const char* why = align_check_inputs(p, T0, n_hyp, weights, n_rays)) return why;
    if (const char* why = raycast_check_host(rp.t_min, rp.t_max, rp.eps, rp.relax, rp.max_steps)) return why;
    if (const char* why = align_rays_check_gap_host(max_gap, p.max_dist)) return why;
    return raycast_check_size(n_obj, n_hyp * n_rays);
}

// Rays and weights are uploaded once; per evaluation the host sends the hypotheses' fp32 poses and reads the cast's pair counts, live polls
// and winner counts and align_math::NSUM doubles per hypothesis.  The rows r = h n_rays + i of all hypotheses are ONE cast.
void align_rays_run(dsp_handle* h, const std::vector<float>& tab, const float* codes, int64_t n_obj, const float* pts, const float* origins,
                    const float* weights, int64_t n_rays, const double* T0, int64_t n_hyp, const dsp_align_params& prm, const raycast_math::Params& rprm,
                    double max_gap, double* T_out, double* record, int32_t* obj, float* dist, float* t_hit, int32_t* status, double* trace) {
    constexpr int NS = align_math::NSUM;
    for (auto& c : h->ar_stats) c = 0;
    std::vector<AlignHyp> hyp = align_start(T0, n_hyp);
    if (trace) std::fill(trace, trace + (size_t)n_hyp * prm.iterations * DSP_ALIGN_TRACE, 0.0);
    if (n_hyp == 0) return;
    if (n_rays == 0 || n_obj == 0) {
        align_write_no_support(hyp, prm, T_out, record);
        if (obj)
            for (int64_t r = 0; r < n_hyp * n_rays; ++r) { obj[r] = -1; dist[r] = t_hit[r] = INFINITY; status[r] = raycast_math::STATUS_MISS; }
        return;
    }
    HIP_TRY(hipSetDevice(h->device));
    const int64_t n_rows = n_hyp * n_rays, nb = align_gram_blocks(n_rays);
    DevBuf<float> a_pts, a_org, a_w, a_hyp, a_grad, c_tab, c_cb, c_pw, c_ow, c_dir, m_dist, r_dist, r_t;
    DevBuf<int> m_obj, r_obj, r_status;
    DevBuf<double> a_slab, a_sums;
    RaycastWork w;
    std::vector<float> cb;
    SyncOnExit sync_on_exit{h->stream};
    QueryTimer timer{h->q_timing, h->stream, {}};
    h->q_ms[0] = h->q_ms[1] = 0.0;
    timer.mark();
    cb = raycast_code_biases(h, codes, n_obj);
    a_pts.alloc((size_t)n_rays * 3);
    if (origins) a_org.alloc((size_t)n_rays * 3);
    if (weights) a_w.alloc((size_t)n_rays);
    a_hyp.alloc((size_t)n_hyp * ALIGN_HYP_STRIDE);
    a_grad.alloc((size_t)n_rows * 3);
    c_tab.alloc(tab.size());
    c_cb.alloc(cb.size());
    c_pw.alloc((size_t)n_rows * 3);
    c_ow.alloc((size_t)n_rows * 3);
    c_dir.alloc((size_t)n_rows * 3);
    m_obj.alloc((size_t)n_rows);
    m_dist.alloc((size_t)n_rows);
    if (obj) { r_obj.alloc((size_t)n_rows); r_dist.alloc((size_t)n_rows); r_t.alloc((size_t)n_rows); r_status.alloc((size_t)n_rows); }
    a_slab.alloc((size_t)n_hyp * nb * NS);
    a_sums.alloc((size_t)n_hyp * NS);
    HIP_TRY(hipMemcpyAsync(a_pts.p, pts, (size_t)n_rays * 12, hipMemcpyHostToDevice, h->stream));
    if (origins) HIP_TRY(hipMemcpyAsync(a_org.p, origins, (size_t)n_rays * 12, hipMemcpyHostToDevice, h->stream));
    if (weights) HIP_TRY(hipMemcpyAsync(a_w.p, weights, (size_t)n_rays * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(c_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(c_cb.p, cb.data(), cb.size() * 4, hipMemcpyHostToDevice, h->stream));
    const RaycastRows gradient = [&](const RaycastDev&, const float* rows, const int2* row_meta, int n) {
        HIP_TRY(launch_align_rays_gradient(rows, row_meta, n, c_tab.p, (int)n_obj, n_rows, a_grad.p, h->stream));
    };
    align_loop(hyp, prm, trace, &h->ar_stats[6],
               [&](const std::vector<float>& hyp_tab, std::vector<double>& sums) {
                   HIP_TRY(hipMemcpyAsync(a_hyp.p, hyp_tab.data(), hyp_tab.size() * 4, hipMemcpyHostToDevice, h->stream));
                   HIP_TRY(launch_align_rays_build(a_pts.p, origins ? a_org.p : nullptr, n_rays, a_hyp.p, n_rows, c_pw.p, c_ow.p, c_dir.p, h->stream));
                   raycast_core(h, w, c_ow.p, c_dir.p, c_tab.p, c_cb.p, n_obj, n_rows, rprm, nullptr, timer, h->ar_stats, gradient);
                   HIP_TRY(launch_align_rays_residual(c_ow.p, c_dir.p, w.r_obj.p, w.r_t.p, w.r_dist.p, w.r_status.p, a_grad.p, n_rows, max_gap, m_obj.p,
                                                      m_dist.p, h->stream));
                   HIP_TRY(launch_align_gram(c_pw.p, m_obj.p, m_dist.p, a_grad.p, weights ? a_w.p : nullptr, n_rays, (int)n_hyp, a_hyp.p, prm.huber,
                                             prm.max_dist, a_slab.p, a_sums.p, h->stream));
                   HIP_TRY(hipMemcpyAsync(sums.data(), a_sums.p, sums.size() * 8, hipMemcpyDeviceToHost, h->stream));
                   HIP_TRY(hipStreamSynchronize(h->stream));    // the sums; w's uploads and hyp_tab have been consumed
                   raycast_core_stats(w, h->ar_stats);
               },
               [&](int64_t k) {
                   if (!obj) return;
                   const size_t o = (size_t)k * n_rays, nbytes = (size_t)n_rays * 4;
                   HIP_TRY(hipMemcpyAsync(r_obj.p + o, m_obj.p + o, nbytes, hipMemcpyDeviceToDevice, h->stream));
                   HIP_TRY(hipMemcpyAsync(r_dist.p + o, m_dist.p + o, nbytes, hipMemcpyDeviceToDevice, h->stream));
                   HIP_TRY(hipMemcpyAsync(r_t.p + o, w.r_t.p + o, nbytes, hipMemcpyDeviceToDevice, h->stream));
                   HIP_TRY(hipMemcpyAsync(r_status.p + o, w.r_status.p + o, nbytes, hipMemcpyDeviceToDevice, h->stream));
               });
    if (obj) {
        HIP_TRY(hipMemcpyAsync(obj, r_obj.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(dist, r_dist.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(t_hit, r_t.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(status, r_status.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, h->stream));
    }
    timer.mark();
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    timer.read(h->q_ms);
    for (int64_t k = 0; k < n_hyp; ++k) align_write(hyp[k], T_out + 16 * k, record + (size_t)DSP_ALIGN_RECORD * k);
}

// ------------------------------------------------------------------------------------------------
// object refinement (dsp_map_align_objects; arithmetic: align_objects_math.h, kernels: align_objects_kernels.hip)
// ------------------------------------------------------------------------------------------------

// what dsp_map_align_objects refuses before it touches the device, besides the map: nullptr, or what is wrong
const char* align_objects_check_inputs(const dsp_align_params& p, const dsp_raycast_params& rp, double max_gap, const float* origins, const float* weights,
                                       int64_t n_rays, int64_t n_obj) {
    if (const char* why = align_check_params(p)) return why;
    if (n_rays > (int64_t)0x7fffffff) return "align_objects: n_rays exceeds 2^31 - 1 (split the request)";
    if (n_rays > 0 && !origins) return "align_objects: origins_world is required (one ray origin per measured point)";
    if (weights)
        for (int64_t i = 0; i < n_rays; ++i)
            if (!(weights[i] >= 0.f) || !std::isfinite(weights[i])) return "align: weights must be finite and >= 0";
    if (const char* why = raycast_check_host(rp.t_min, rp.t_max, rp.eps, rp.relax, rp.max_steps)) return why;
    if (const char* why = align_rays_check_gap_host(max_gap, p.max_dist)) return why;
    return raycast_check_size(n_obj, n_rays);
}

// Rays, directions and weights are uploaded once; per evaluation the host sends the object table of the composed poses and reads the cast's
// pair counts, live polls and winner counts -- from which it makes the lists' offsets and the block table -- and align_math::NSUM doubles
// per object.  The "hypotheses" of align_loop are the objects and their poses the corrections C_k.
void align_objects_run(dsp_handle* h, const std::vector<float>& tab0, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts,
                       const float* origins, const float* weights, int64_t n_rays, const unsigned char* refine, const dsp_align_params& prm,
                       const raycast_math::Params& rprm, double max_gap, float* t_out, double* correction, double* record, int32_t* obj, float* dist,
                       float* t_hit, int32_t* status, double* trace) {
    constexpr int NS = align_math::NSUM;
    for (auto& c : h->ao_stats) c = 0;
    if (trace) std::fill(trace, trace + (size_t)n_obj * prm.iterations * DSP_ALIGN_TRACE, 0.0);
    auto no_rays = [&] {
        if (obj)
            for (int64_t r = 0; r < n_rays; ++r) { obj[r] = -1; dist[r] = t_hit[r] = INFINITY; status[r] = raycast_math::STATUS_MISS; }
    };
    if (n_obj == 0) { no_rays(); return; }
    std::vector<double> ident((size_t)n_obj * 16, 0.0);
    for (int64_t k = 0; k < n_obj; ++k) ident[16 * k] = ident[16 * k + 5] = ident[16 * k + 10] = ident[16 * k + 15] = 1.0;
    std::vector<AlignHyp> hyp = align_start(ident.data(), n_obj);
    const double zero[NS] = {};
    for (int64_t k = 0; k < n_obj; ++k) {
        hyp[k].F0 = hyp[k].F_acc = align_cost_host(zero, prm.huber, prm.max_dist);
        if (refine && !refine[k]) hyp[k].live = false;                  // never evaluated: status OK, 0 evaluations
        else if (n_rays == 0) { hyp[k].live = false; hyp[k].status = DSP_ALIGN_NO_SUPPORT; }
    }
    auto write_out = [&] {
        for (int64_t k = 0; k < n_obj; ++k) {
            align_write(hyp[k], correction + 16 * k, record + (size_t)DSP_ALIGN_RECORD * k);
            align_objects_compose_host(hyp[k].T_acc, t_world_obj + 16 * k, t_out + 16 * k);
        }
    };
    bool any = false;
    for (const AlignHyp& a : hyp) any = any || a.live;
    if (n_rays == 0 || (!any && !obj)) { no_rays(); write_out(); return; }
    HIP_TRY(hipSetDevice(h->device));
    DevBuf<float> a_pts, a_org, a_dir, a_w, a_grad, c_tab, c_cb, m_dist;
    DevBuf<int> m_obj, a_off, a_first, a_win;
    DevBuf<int4> a_blocks;
    DevBuf<double> a_slab, a_sums;
    RaycastWork w;
    std::vector<float> cb, dirs((size_t)n_rays * 3), tab((size_t)n_obj * query_math::OBJ_STRIDE, 0.f);
    std::vector<int> off((size_t)n_obj), first((size_t)n_obj + 1);
    std::vector<int4> blocks;
    SyncOnExit sync_on_exit{h->stream};
    QueryTimer timer{h->q_timing, h->stream, {}};
    h->q_ms[0] = h->q_ms[1] = 0.0;
    timer.mark();
    cb = raycast_code_biases(h, codes, n_obj);
    align_objects_directions_host(n_rays, origins, pts, dirs.data());
    a_pts.alloc((size_t)n_rays * 3);
    a_org.alloc((size_t)n_rays * 3);
    a_dir.alloc((size_t)n_rays * 3);
    if (weights) a_w.alloc((size_t)n_rays);
    a_grad.alloc((size_t)n_rays * 3);
    c_tab.alloc(tab.size());
    c_cb.alloc(cb.size());
    m_obj.alloc((size_t)n_rays);
    m_dist.alloc((size_t)n_rays);
    a_off.alloc((size_t)n_obj);
    a_first.alloc((size_t)n_obj + 1);
    a_win.alloc((size_t)n_rays);
    a_sums.alloc((size_t)n_obj * NS);
    HIP_TRY(hipMemcpyAsync(a_pts.p, pts, (size_t)n_rays * 12, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(a_org.p, origins, (size_t)n_rays * 12, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(a_dir.p, dirs.data(), (size_t)n_rays * 12, hipMemcpyHostToDevice, h->stream));
    if (weights) HIP_TRY(hipMemcpyAsync(a_w.p, weights, (size_t)n_rays * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(c_cb.p, cb.data(), cb.size() * 4, hipMemcpyHostToDevice, h->stream));
    const RaycastRows gradient = [&](const RaycastDev&, const float* rows, const int2* row_meta, int n) {
        HIP_TRY(launch_align_rays_gradient(rows, row_meta, n, c_tab.p, (int)n_obj, n_rays, a_grad.p, h->stream));
    };
    // the object table at the trial poses of the evaluated objects (trial) or at every object's accepted pose; a trial pose the map's
    // inversion refuses ends its object with SINGULAR at its accepted state
    auto table = [&](bool trial) {
        for (int64_t k = 0; k < n_obj; ++k) {
            float pose[16];
            float* e = tab.data() + k * query_math::OBJ_STRIDE;
            bool ok = false;
            if (trial && hyp[k].live) {
                align_objects_compose_host(hyp[k].T_eval, t_world_obj + 16 * k, pose);
                ok = query_invert_host(pose, e, e + 12);
                if (!ok) { hyp[k].live = false; hyp[k].status = DSP_ALIGN_SINGULAR; }
            }
            if (!ok) {
                align_objects_compose_host(hyp[k].T_acc, t_world_obj + 16 * k, pose);
                if (!query_invert_host(pose, e, e + 12)) throw std::runtime_error("align_objects: an accepted pose is not invertible");
            }
            e[13] = std::isnan(tab0[(size_t)k * query_math::OBJ_STRIDE + 13]) ? std::nanf("") : e[12];     // a code that is not finite never wins
        }
    };
    // table up, the cast with the winners' gradients behind it, the rows' (obj, d): the stream is NOT synchronised behind it
    auto cast = [&](bool trial) {
        table(trial);
        HIP_TRY(hipMemcpyAsync(c_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->stream));
        raycast_core(h, w, a_org.p, a_dir.p, c_tab.p, c_cb.p, n_obj, n_rays, rprm, nullptr, timer, h->ao_stats, gradient);
        HIP_TRY(launch_align_rays_residual(a_org.p, a_dir.p, w.r_obj.p, w.r_t.p, w.r_dist.p, w.r_status.p, a_grad.p, n_rays, max_gap, m_obj.p, m_dist.p,
                                           h->stream));
    };
    align_loop(hyp, prm, trace, &h->ao_stats[6],
               [&](const std::vector<float>&, std::vector<double>& sums) {
                   cast(true);
                   // w.cnt: the winners per object, read back by the cast.  The lists of ALL objects, blocks for the evaluated ones
                   int64_t n_list = 0;
                   blocks.clear();
                   for (int64_t k = 0; k < n_obj; ++k) {
                       off[k] = (int)n_list;
                       first[k] = (int)blocks.size();
                       if (hyp[k].live)
                           for (int j = 0; j < w.cnt[k]; j += align_math::BLOCK)
                               blocks.push_back(make_int4((int)k, (int)n_list + j, std::min(align_math::BLOCK, w.cnt[k] - j), 0));
                       n_list += w.cnt[k];
                   }
                   first[n_obj] = (int)blocks.size();
                   if (n_list > n_rays) throw std::runtime_error("align_objects: more winners than rays");
                   a_blocks.ensure(blocks.size());
                   a_slab.ensure(blocks.size() * NS);
                   HIP_TRY(hipMemcpyAsync(a_off.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
                   HIP_TRY(hipMemcpyAsync(a_first.p, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
                   if (!blocks.empty())
                       HIP_TRY(hipMemcpyAsync(a_blocks.p, blocks.data(), blocks.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
                   HIP_TRY(launch_align_objects_list(w.r_obj.p, (int)n_rays, (int)n_obj, (int)((n_rays + 63) / 64), w.r_wave_cnt.p, a_off.p, (int)n_list,
                                                     a_win.p, h->stream));
                   HIP_TRY(launch_align_objects_gram(a_blocks.p, (int)blocks.size(), a_first.p, (int)n_obj, a_win.p, (int)n_list, (int)n_rays, a_pts.p,
                                                     m_obj.p, m_dist.p, a_grad.p, weights ? a_w.p : nullptr, prm.huber, prm.max_dist, a_slab.p, a_sums.p,
                                                     h->stream));
                   HIP_TRY(hipMemcpyAsync(sums.data(), a_sums.p, sums.size() * 8, hipMemcpyDeviceToHost, h->stream));
                   HIP_TRY(hipStreamSynchronize(h->stream));    // the sums; w's uploads, the table and the block table have been consumed
                   raycast_core_stats(w, h->ao_stats);
                   for (int64_t k = 0; k < n_obj; ++k)          // the object moves, not the measured point: b is row_terms's negated
                       for (int q = 0; q < 6; ++q) sums[k * NS + align_math::IDX_B + q] = -sums[k * NS + align_math::IDX_B + q];
               },
               {});
    if (obj) {      // one more evaluation of the returned map, every object at its returned pose
        cast(false);
        h->ao_stats[6] += 1;
        HIP_TRY(hipMemcpyAsync(obj, m_obj.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(dist, m_dist.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(t_hit, w.r_t.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(status, w.r_status.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
    }
    timer.mark();
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    timer.read(h->q_ms);
    if (obj) raycast_core_stats(w, h->ao_stats);
    write_out();
}

// ------------------------------------------------------------------------------------------------
// shape refinement (dsp_map_align_shapes; arithmetic: align_shapes_math.h, kernels: align_shapes_kernels.hip)
// ------------------------------------------------------------------------------------------------

const char* align_shapes_check_params(const dsp_shapes_params& sp) {
    if (sp.unknowns == 0 || (sp.unknowns & ~(DSP_SHAPES_CODE | DSP_SHAPES_POSE))) return "align_shapes: unknowns must be DSP_SHAPES_CODE, DSP_SHAPES_POSE or both";
    if (!std::isfinite(sp.code_reg) || sp.code_reg < 0.0 || !std::isfinite(sp.code_anchor) || sp.code_anchor < 0.0)
        return "align_shapes: code_reg and code_anchor must be finite and >= 0";
    if (!std::isfinite(sp.code_tol) || sp.code_tol < 0.0) return "align_shapes: code_tol must be finite and >= 0";
    return nullptr;
}

// one object on the host: the accepted state (C, z) with its sums, and the state to evaluate next
struct ShapeHyp {
    double C_acc[16], C_eval[16], z_acc[CODE_LEN], z_eval[CODE_LEN], z0[CODE_LEN];
    std::vector<double> S;              // the sums at the accepted state
    double F_acc = 0.0, F0 = 0.0, lam = 0.0;
    bool live = true, has_acc = false;
    int status = DSP_ALIGN_OK, evals = 0, steps = 0;
};

// The sibling of align_objects_run whose state carries a code: the same uploads, cast, lists and block table (blocks of
// align_shapes_math::BLOCK positions); per evaluation the host also sends the code biases of the objects' evaluated codes and reads
// align_shapes_math::NSUM doubles per object.  The loop is align_loop's with the 70-dimensional step.
void align_shapes_run(dsp_handle* h, const std::vector<float>& tab0, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts,
                      const float* origins, const float* weights, int64_t n_rays, const unsigned char* refine, const dsp_align_params& prm,
                      const dsp_shapes_params& sprm, const raycast_math::Params& rprm, double max_gap, float* t_out, float* codes_out, double* correction,
                      double* record, int32_t* obj, float* dist, float* t_hit, int32_t* status, double* trace) {
    namespace sm = align_shapes_math;
    constexpr int NS = sm::NSUM, DIM = sm::DIM;
    const int iters = prm.iterations, code_len = h->code_len, unknowns = sprm.unknowns;
    for (auto& c : h->as_stats) c = 0;
    if (trace) std::fill(trace, trace + (size_t)n_obj * iters * DSP_SHAPES_TRACE, 0.0);
    auto no_rays = [&] {
        if (obj)
            for (int64_t r = 0; r < n_rays; ++r) { obj[r] = -1; dist[r] = t_hit[r] = INFINITY; status[r] = raycast_math::STATUS_MISS; }
    };
    if (n_obj == 0) { no_rays(); return; }
    const std::vector<double> zero((size_t)NS, 0.0);
    std::vector<ShapeHyp> hyp((size_t)n_obj);
    for (int64_t k = 0; k < n_obj; ++k) {
        ShapeHyp& a = hyp[k];
        for (int i = 0; i < 16; ++i) a.C_acc[i] = a.C_eval[i] = (i % 5 == 0) ? 1.0 : 0.0;
        for (int c = 0; c < CODE_LEN; ++c) a.z0[c] = a.z_acc[c] = a.z_eval[c] = (double)codes[k * CODE_LEN + c];
        a.S = zero;
        a.F0 = a.F_acc = align_shapes_cost_host(align_shapes_mean_cost_host(zero.data(), prm.huber, prm.max_dist), a.z0, a.z0, code_len, sprm.code_reg,
                                                sprm.code_anchor);
        if (refine && !refine[k]) a.live = false;                       // never evaluated: status OK, 0 evaluations
        else if (n_rays == 0) { a.live = false; a.status = DSP_ALIGN_NO_SUPPORT; }
    }
    // the fp32 code an object is decoded with: the input's own bytes as long as the fp64 code is the input's
    auto code32 = [&](int64_t k, const double* z, float* out) {
        for (int c = 0; c < CODE_LEN; ++c)
            out[c] = (z[c] == hyp[k].z0[c] || memcmp(z + c, hyp[k].z0 + c, sizeof(double)) == 0) ? codes[k * CODE_LEN + c] : (float)z[c];
        if (!(unknowns & DSP_SHAPES_CODE)) memcpy(out, codes + k * CODE_LEN, CODE_LEN * sizeof(float));
    };
    auto write_out = [&] {
        for (int64_t k = 0; k < n_obj; ++k) {
            const ShapeHyp& a = hyp[k];
            memcpy(correction + 16 * k, a.C_acc, sizeof a.C_acc);
            align_objects_compose_host(a.C_acc, t_world_obj + 16 * k, t_out + 16 * k);
            code32(k, a.z_acc, codes_out + k * CODE_LEN);
            double* rec = record + (size_t)DSP_SHAPES_RECORD * k;
            rec[0] = a.status; rec[1] = a.evals; rec[2] = a.steps; rec[3] = a.F0; rec[4] = a.F_acc;
            rec[5] = a.S[sm::IDX_N]; rec[6] = a.S[sm::IDX_W]; rec[7] = a.lam;
            int q = sm::IDX_H;
            for (int i = 0; i < DIM; ++i)
                for (int j = i; j < DIM; ++j) rec[8 + DIM * i + j] = rec[8 + DIM * j + i] = a.S[q++];
            for (int i = 0; i < DIM; ++i) rec[8 + DIM * DIM + i] = a.S[sm::IDX_B + i];
        }
    };
    bool any = false;
    for (const ShapeHyp& a : hyp) any = any || a.live;
    if (n_rays == 0 || (!any && !obj)) { no_rays(); write_out(); return; }
    HIP_TRY(hipSetDevice(h->device));
    DevBuf<float> a_pts, a_org, a_dir, a_w, a_grad, a_gcode, c_tab, c_cb, m_dist;
    DevBuf<int> m_obj, a_off, a_first, a_win;
    DevBuf<int4> a_blocks;
    DevBuf<double> a_slab, a_sums;
    RaycastWork w;
    std::vector<float> cb((size_t)n_obj * 2 * WIDTH), dirs((size_t)n_rays * 3), tab((size_t)n_obj * query_math::OBJ_STRIDE, 0.f);
    std::vector<int> off((size_t)n_obj), first((size_t)n_obj + 1);
    std::vector<int4> blocks;
    std::vector<double> sums((size_t)n_obj * NS, 0.0);
    SyncOnExit sync_on_exit{h->stream};
    QueryTimer timer{h->q_timing, h->stream, {}};
    h->q_ms[0] = h->q_ms[1] = 0.0;
    timer.mark();
    align_objects_directions_host(n_rays, origins, pts, dirs.data());
    a_pts.alloc((size_t)n_rays * 3);
    a_org.alloc((size_t)n_rays * 3);
    a_dir.alloc((size_t)n_rays * 3);
    if (weights) a_w.alloc((size_t)n_rays);
    a_grad.alloc((size_t)n_rays * 3);
    a_gcode.alloc((size_t)n_rays * CODE_LEN);
    c_tab.alloc(tab.size());
    c_cb.alloc(cb.size());
    m_obj.alloc((size_t)n_rays);
    m_dist.alloc((size_t)n_rays);
    a_off.alloc((size_t)n_obj);
    a_first.alloc((size_t)n_obj + 1);
    a_win.alloc((size_t)n_rays);
    a_sums.alloc((size_t)n_obj * NS);
    HIP_TRY(hipMemcpyAsync(a_pts.p, pts, (size_t)n_rays * 12, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(a_org.p, origins, (size_t)n_rays * 12, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(a_dir.p, dirs.data(), (size_t)n_rays * 12, hipMemcpyHostToDevice, h->stream));
    if (weights) HIP_TRY(hipMemcpyAsync(a_w.p, weights, (size_t)n_rays * 4, hipMemcpyHostToDevice, h->stream));
    const RaycastRows gradient = [&](const RaycastDev&, const float* rows, const int2* row_meta, int n) {
        HIP_TRY(launch_align_rays_gradient(rows, row_meta, n, c_tab.p, (int)n_obj, n_rays, a_grad.p, h->stream));
        HIP_TRY(launch_align_shapes_rows(rows, row_meta, n, c_tab.p, (int)n_obj, n_rays, a_gcode.p, h->stream));
    };
    // The object table and the code biases at the trial states of the evaluated objects (trial) or at every object's accepted state.  A trial
    // code or bias that is not finite, or a trial pose the map's inversion refuses, ends its object with SINGULAR at its accepted state.
    auto table = [&](bool trial) {
        for (int64_t k = 0; k < n_obj; ++k) {
            ShapeHyp& a = hyp[k];
            float pose[16], z32[CODE_LEN];
            float* e = tab.data() + k * query_math::OBJ_STRIDE;
            float* bias = cb.data() + (size_t)k * 2 * WIDTH;
            bool ok = false;
            if (trial && a.live) {
                align_objects_compose_host(a.C_eval, t_world_obj + 16 * k, pose);
                ok = query_invert_host(pose, e, e + 12);
                code32(k, a.z_eval, z32);
                code_bias_host(h->h_codew, h->h_b0, h->h_blat, z32, bias);
                if (ok && a.has_acc) {          // the first evaluation is the input's: the map's own rule for a code that is not finite holds
                    for (int c = 0; c < CODE_LEN; ++c) ok = ok && std::isfinite(z32[c]);
                    for (int c = 0; c < 2 * WIDTH; ++c) ok = ok && std::isfinite(bias[c]);
                }
                if (!ok) { a.live = false; a.status = DSP_ALIGN_SINGULAR; }
            }
            if (!ok) {
                align_objects_compose_host(a.C_acc, t_world_obj + 16 * k, pose);
                if (!query_invert_host(pose, e, e + 12)) throw std::runtime_error("align_shapes: an accepted pose is not invertible");
                code32(k, a.z_acc, z32);
                code_bias_host(h->h_codew, h->h_b0, h->h_blat, z32, bias);
            }
            e[13] = std::isnan(tab0[(size_t)k * query_math::OBJ_STRIDE + 13]) ? std::nanf("") : e[12];     // a code that is not finite never wins
        }
    };
    // table and biases up, the cast with the winners' gradients behind it, the rows' (obj, d): the stream is NOT synchronised behind it
    auto cast = [&](bool trial) {
        table(trial);
        HIP_TRY(hipMemcpyAsync(c_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(c_cb.p, cb.data(), cb.size() * 4, hipMemcpyHostToDevice, h->stream));
        raycast_core(h, w, a_org.p, a_dir.p, c_tab.p, c_cb.p, n_obj, n_rays, rprm, nullptr, timer, h->as_stats, gradient);
        HIP_TRY(launch_align_rays_residual(a_org.p, a_dir.p, w.r_obj.p, w.r_t.p, w.r_dist.p, w.r_status.p, a_grad.p, n_rays, max_gap, m_obj.p, m_dist.p,
                                           h->stream));
    };
    auto evaluate = [&] {
        cast(true);
        // w.cnt: the winners per object, read back by the cast.  The lists of ALL objects, blocks for the evaluated ones
        int64_t n_list = 0;
        blocks.clear();
        for (int64_t k = 0; k < n_obj; ++k) {
            off[k] = (int)n_list;
            first[k] = (int)blocks.size();
            if (hyp[k].live)
                for (int j = 0; j < w.cnt[k]; j += sm::BLOCK) blocks.push_back(make_int4((int)k, (int)n_list + j, std::min(sm::BLOCK, w.cnt[k] - j), 0));
            n_list += w.cnt[k];
        }
        first[n_obj] = (int)blocks.size();
        if (n_list > n_rays) throw std::runtime_error("align_shapes: more winners than rays");
        a_blocks.ensure(blocks.size());
        a_slab.ensure(blocks.size() * NS);
        HIP_TRY(hipMemcpyAsync(a_off.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(a_first.p, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (!blocks.empty()) HIP_TRY(hipMemcpyAsync(a_blocks.p, blocks.data(), blocks.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(launch_align_objects_list(w.r_obj.p, (int)n_rays, (int)n_obj, (int)((n_rays + 63) / 64), w.r_wave_cnt.p, a_off.p, (int)n_list, a_win.p,
                                          h->stream));
        HIP_TRY(launch_align_shapes_gram(a_blocks.p, (int)blocks.size(), a_first.p, (int)n_obj, a_win.p, (int)n_list, (int)n_rays, a_pts.p, m_obj.p, m_dist.p,
                                         a_grad.p, a_gcode.p, weights ? a_w.p : nullptr, prm.huber, prm.max_dist, a_slab.p, a_sums.p, h->stream));
        HIP_TRY(hipMemcpyAsync(sums.data(), a_sums.p, sums.size() * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));    // the sums; w's uploads, the table, the biases and the block table have been consumed
        raycast_core_stats(w, h->as_stats);
    };
    const step_rule::Params sp{prm.lambda0, prm.up, prm.down, prm.lambda_min, prm.lambda_max};
    const bool step_on = !step_rule::is_off(sp);
    auto end = [](ShapeHyp& a, int st) { a.live = false; a.status = st; };
    std::vector<double> H((size_t)DIM * DIM);
    for (int e = 0; e < iters; ++e) {
        any = false;
        for (const ShapeHyp& a : hyp) any = any || a.live;
        if (!any) break;
        evaluate();
        h->as_stats[6] += 1;
        for (int64_t k = 0; k < n_obj; ++k) {
            ShapeHyp& a = hyp[k];
            if (!a.live) continue;          // also an object whose trial state the table refused
            const double* S = sums.data() + k * NS;
            const double F = align_shapes_cost_host(align_shapes_mean_cost_host(S, prm.huber, prm.max_dist), a.z_eval, a.z0, code_len, sprm.code_reg,
                                                    sprm.code_anchor);
            const bool support = S[sm::IDX_N] >= (double)prm.min_points;
            double* tr = trace ? trace + ((size_t)k * iters + e) * DSP_SHAPES_TRACE : nullptr;
            a.evals += 1;
            if (e == 0) a.F0 = F;
            int dec = step_rule::ACCEPTED;
            if (step_on)
                dec = !a.has_acc ? step_rule::decide(true, F, 0.0, sp, a.lam)
                                 : step_rule::decide(false, support ? F : (double)INFINITY, a.F_acc, sp, a.lam);
            if (dec == step_rule::ACCEPTED) {
                if (a.has_acc) a.steps += 1;
                memcpy(a.C_acc, a.C_eval, sizeof a.C_acc);
                memcpy(a.z_acc, a.z_eval, sizeof a.z_acc);
                a.S.assign(S, S + NS);
                a.F_acc = F;
                a.has_acc = true;
            }
            if (tr) {
                memcpy(tr, a.C_eval, sizeof a.C_eval);
                memcpy(tr + 16, a.z_eval, sizeof a.z_eval);
                tr[80] = dec; tr[81] = F; tr[82] = a.lam; tr[83] = S[sm::IDX_N];
            }
            // the step from the accepted state
            if (a.S[sm::IDX_N] < (double)prm.min_points) { end(a, DSP_ALIGN_NO_SUPPORT); continue; }
            double dx[DIM];
            int q = sm::IDX_H;
            for (int i = 0; i < DIM; ++i)
                for (int j = i; j < DIM; ++j) H[(size_t)DIM * i + j] = H[(size_t)DIM * j + i] = a.S[q++];
            bool solved = false;
            for (int tries = 0; !solved; ++tries) {
                solved = align_shapes_solve_host(H.data(), a.S.data() + sm::IDX_B, a.S[sm::IDX_W], a.z_acc, a.z0, code_len, unknowns, sprm.code_reg,
                                                 sprm.code_anchor, prm.damp, a.lam, dx);
                if (solved || !step_on || tries >= 64 || !(a.lam < sp.lambda_max)) break;
                a.lam = fmin(fmax(a.lam, sp.lambda_min) * sp.up, sp.lambda_max);        // a failed factorisation: lambda grows like after a rejection
            }
            if (tr) tr[82] = a.lam;
            if (!solved) { end(a, DSP_ALIGN_SINGULAR); continue; }
            if (tr) memcpy(tr + 84, dx, sizeof dx);
            double mv = 0.0, mw = 0.0, mz = 0.0;
            for (int i = 0; i < 3; ++i) { mv = fmax(mv, fabs(dx[i])); mw = fmax(mw, fabs(dx[3 + i])); }
            for (int c = 0; c < CODE_LEN; ++c) mz = fmax(mz, fabs(dx[6 + c]));
            if (mv < prm.trans_tol && mw < prm.rot_tol && mz < sprm.code_tol) { end(a, DSP_ALIGN_CONVERGED); continue; }
            if (e == iters - 1) { end(a, DSP_ALIGN_OK); continue; }
            align_shapes_apply_step_host(dx, unknowns, code_len, a.C_acc, a.z_acc, a.C_eval, a.z_eval);
        }
    }
    if (obj) {      // one more evaluation of the returned map, every object at its returned state
        cast(false);
        h->as_stats[6] += 1;
        HIP_TRY(hipMemcpyAsync(obj, m_obj.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(dist, m_dist.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(t_hit, w.r_t.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(status, w.r_status.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, h->stream));
    }
    timer.mark();
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipGetLastError());
    timer.read(h->q_ms);
    if (obj) raycast_core_stats(w, h->as_stats);
    write_out();
}

}  // namespace

extern "C" {

int dsp_map_query(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts_world, int64_t n_pts, int32_t flags,
                  int32_t* obj, float* dist, float* bound, float* normal) {
    if (!h || n_obj < 0 || n_pts < 0 || (flags & ~DSP_QUERY_NORMALS)) return DSP_E_ARG;
    const bool normals = (flags & DSP_QUERY_NORMALS) != 0;
    if ((n_obj > 0 && (!t_world_obj || !codes)) || (!normals && normal)) return DSP_E_ARG;
    if (n_pts > 0 && (!pts_world || !obj || !dist || !bound || (normals && !normal))) return DSP_E_ARG;
    return guarded(h, [&] {
        if (n_pts > (int64_t)0x7fffffff) throw std::invalid_argument("map query too large (split the request)");
        const std::vector<float> tab = query_table(h, t_world_obj, codes, n_obj);
        query_run(h, tab, codes, n_obj, pts_world, n_pts, obj, dist, bound, normal);
    });
}

void dsp_raycast_params_default(dsp_raycast_params* p) {
    if (!p) return;
    *p = dsp_raycast_params{raycast_math::DEFAULT_T_MIN, INFINITY, raycast_math::DEFAULT_EPS, raycast_math::DEFAULT_RELAX, raycast_math::DEFAULT_MAX_STEPS};
}

int dsp_map_raycast(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* origins, const float* dirs, int64_t n_rays,
                    const dsp_raycast_params* params, int32_t flags, int32_t* obj, float* t, float* dist, int32_t* status, float* normal) {
    if (!h || !params || n_obj < 0 || n_rays < 0 || (flags & ~DSP_RAYCAST_NORMALS)) return DSP_E_ARG;
    const bool normals = (flags & DSP_RAYCAST_NORMALS) != 0;
    if ((n_obj > 0 && (!t_world_obj || !codes)) || (!normals && normal)) return DSP_E_ARG;
    if (n_rays > 0 && (!origins || !dirs || !obj || !t || !dist || !status || (normals && !normal))) return DSP_E_ARG;
    return guarded(h, [&] {
        const raycast_math::Params prm = raycast_params(*params);
        if (const char* why = raycast_check_host(prm.t_min, prm.t_max, prm.eps, prm.relax, prm.max_steps)) throw std::invalid_argument(why);
        if (n_rays > (int64_t)0x7fffffff) throw std::invalid_argument("raycast too large (split the request)");
        const std::vector<float> tab = query_table(h, t_world_obj, codes, n_obj);
        raycast_run(h, tab, codes, n_obj, origins, dirs, n_rays, prm, obj, t, dist, status, normal);
    });
}

int dsp_map_raycast_last_stats(dsp_handle* h, int64_t* counts6) {
    if (!h || !counts6) return DSP_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    memcpy(counts6, h->r_stats, sizeof h->r_stats);
    return DSP_OK;
}

int dsp_debug_raycast_check(const dsp_raycast_params* params) {
    if (!params) return DSP_E_ARG;
    return raycast_check_host(params->t_min, params->t_max, params->eps, params->relax, params->max_steps) ? DSP_E_ARG : DSP_OK;
}

int dsp_debug_raycast_segments(int64_t n_obj, const float* rt_ow, const float* scale, int64_t n_rays, const float* origins, const float* dirs, float t_min,
                               float t_max, unsigned char* is_void, unsigned char* exists, float* t0, float* t1, float* o_o, float* d_o) {
    if (n_obj < 0 || n_rays < 0 || (n_obj > 0 && (!rt_ow || !scale)) || (n_rays > 0 && (!origins || !dirs))) return DSP_E_ARG;
    raycast_segments_host(n_obj, rt_ow, scale, n_rays, origins, dirs, t_min, t_max, is_void, exists, t0, t1, o_o, d_o);
    return DSP_OK;
}

int dsp_debug_raycast_step(int64_t n, const float* t, const float* t1, const float* sdf, const float* s, const dsp_raycast_params* params,
                           int32_t* decision, float* dist, float* t_next) {
    if (n < 0 || !params || (n > 0 && (!t || !t1 || !sdf || !s || !decision || !dist || !t_next))) return DSP_E_ARG;
    if (raycast_check_host(params->t_min, params->t_max, params->eps, params->relax, params->max_steps)) return DSP_E_ARG;
    raycast_step_host(n, t, t1, sdf, s, params->eps, params->relax, decision, dist, t_next);
    return DSP_OK;
}

void dsp_align_params_default(dsp_align_params* p) {
    if (!p) return;
    *p = dsp_align_params{10, 6, 0.3, 0.05, 0.0, 1e-6, 1e-6, 0.0, 0.0, 0.0, 0.0, 0.0};
}

int dsp_map_align(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts_sensor, const float* weights,
                  int64_t n_pts, const double* t_world_sensor0, int64_t n_hyp, const dsp_align_params* params, double* t_world_sensor,
                  double* record, int32_t* obj, float* dist, double* trace) {
    if (!h || !params || n_obj < 0 || n_pts < 0 || n_hyp < 0 || (obj == nullptr) != (dist == nullptr)) return DSP_E_ARG;
    if ((n_obj > 0 && (!t_world_obj || !codes)) || (n_pts > 0 && !pts_sensor) || (n_hyp > 0 && (!t_world_sensor0 || !t_world_sensor || !record)))
        return DSP_E_ARG;
    return guarded(h, [&] {
        if (const char* why = align_check_inputs(*params, t_world_sensor0, n_hyp, weights, n_pts)) throw std::invalid_argument(why);
        const std::vector<float> tab = query_table(h, t_world_obj, codes, n_obj);
        align_run(h, tab, codes, n_obj, pts_sensor, weights, n_pts, t_world_sensor0, n_hyp, *params, t_world_sensor, record, obj, dist, trace);
    });
}

double dsp_align_rays_default_max_gap(const dsp_align_params* params) { return params ? ALIGN_RAYS_GAP_FACTOR * params->max_dist : 0.0; }

int dsp_map_align_rays(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts_sensor, const float* origins_sensor,
                       const float* weights, int64_t n_rays, const double* t_world_sensor0, int64_t n_hyp, const dsp_align_params* params,
                       const dsp_raycast_params* raycast, double max_gap, double* t_world_sensor, double* record, int32_t* obj, float* dist, float* t_hit,
                       int32_t* status, double* trace) {
    if (!h || !params || !raycast || n_obj < 0 || n_rays < 0 || n_hyp < 0) return DSP_E_ARG;
    const int n_out = (obj != nullptr) + (dist != nullptr) + (t_hit != nullptr) + (status != nullptr);
    if (n_out != 0 && n_out != 4) return DSP_E_ARG;
    if ((n_obj > 0 && (!t_world_obj || !codes)) || (n_rays > 0 && !pts_sensor) || (n_hyp > 0 && (!t_world_sensor0 || !t_world_sensor || !record)))
        return DSP_E_ARG;
    return guarded(h, [&] {
        if (const char* why = align_rays_check_inputs(*params, *raycast, max_gap, t_world_sensor0, n_hyp, weights, n_rays, n_obj))
            throw std::invalid_argument(why);
        const std::vector<float> tab = query_table(h, t_world_obj, codes, n_obj);
        align_rays_run(h, tab, codes, n_obj, pts_sensor, origins_sensor, weights, n_rays, t_world_sensor0, n_hyp, *params, raycast_params(*raycast), max_gap,
                       t_world_sensor, record, obj, dist, t_hit, status, trace);
    });
}

int dsp_map_align_rays_last_stats(dsp_handle* h, int64_t* counts7) {
    if (!h || !counts7) return DSP_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    memcpy(counts7, h->ar_stats, sizeof h->ar_stats);
    return DSP_OK;
}

int dsp_debug_align_rays_check(const dsp_align_params* params, const dsp_raycast_params* raycast, double max_gap, const double* t_world_sensor0,
                               int64_t n_hyp, const float* weights, int64_t n_rays, int64_t n_obj) {
    if (!params || !raycast || n_hyp < 0 || n_rays < 0 || n_obj < 0 || (n_hyp > 0 && !t_world_sensor0)) return DSP_E_ARG;
    if (n_obj > QUERY_MAX_OBJ) return DSP_E_ARG;
    return align_rays_check_inputs(*params, *raycast, max_gap, t_world_sensor0, n_hyp, weights, n_rays, n_obj) ? DSP_E_ARG : DSP_OK;
}

int dsp_debug_align_ray_rows(int64_t n, const float* origins_world, const float* pts_world, const int32_t* obj, const float* t_hit, const float* dist_hit,
                             const int32_t* status, const float* grad_world, const float* weights, double huber, double max_dist, double max_gap,
                             int32_t* obj_row, float* d, double* sums30) {
    if (n < 0 || !sums30 || (n > 0 && (!origins_world || !pts_world || !obj || !t_hit || !dist_hit || !status || !grad_world || !obj_row || !d)))
        return DSP_E_ARG;
    if (!std::isfinite(max_dist) || !std::isfinite(huber) || !(huber > 0.0) || !(huber <= max_dist)) return DSP_E_ARG;
    if (align_rays_check_gap_host(max_gap, max_dist)) return DSP_E_ARG;
    try {
        align_ray_rows_host(n, origins_world, pts_world, obj, t_hit, dist_hit, status, grad_world, weights, huber, max_dist, max_gap, obj_row, d, sums30);
    } catch (const std::bad_alloc&) {
        return DSP_E_NOMEM;
    }
    return DSP_OK;
}

int dsp_map_align_objects(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts_world, const float* origins_world,
                          const float* weights, int64_t n_rays, const unsigned char* refine, const dsp_align_params* params,
                          const dsp_raycast_params* raycast, double max_gap, float* t_world_obj_out, double* correction, double* record, int32_t* obj,
                          float* dist, float* t_hit, int32_t* status, double* trace) {
    if (!h || !params || !raycast || n_obj < 0 || n_rays < 0) return DSP_E_ARG;
    const int n_out = (obj != nullptr) + (dist != nullptr) + (t_hit != nullptr) + (status != nullptr);
    if (n_out != 0 && n_out != 4) return DSP_E_ARG;
    if ((n_obj > 0 && (!t_world_obj || !codes || !t_world_obj_out || !correction || !record)) || (n_rays > 0 && !pts_world)) return DSP_E_ARG;
    return guarded(h, [&] {
        if (const char* why = align_objects_check_inputs(*params, *raycast, max_gap, origins_world, weights, n_rays, n_obj)) throw std::invalid_argument(why);
        const std::vector<float> tab = query_table(h, t_world_obj, codes, n_obj);
        align_objects_run(h, tab, t_world_obj, codes, n_obj, pts_world, origins_world, weights, n_rays, refine, *params, raycast_params(*raycast), max_gap,
                          t_world_obj_out, correction, record, obj, dist, t_hit, status, trace);
    });
}

int dsp_map_align_objects_last_stats(dsp_handle* h, int64_t* counts7) {
    if (!h || !counts7) return DSP_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    memcpy(counts7, h->ao_stats, sizeof h->ao_stats);
    return DSP_OK;
}

int dsp_debug_align_objects_check(const dsp_align_params* params, const dsp_raycast_params* raycast, double max_gap, const float* origins_world,
                                  const float* weights, int64_t n_rays, int64_t n_obj) {
    if (!params || !raycast || n_rays < 0 || n_obj < 0 || n_obj > QUERY_MAX_OBJ) return DSP_E_ARG;
    return align_objects_check_inputs(*params, *raycast, max_gap, origins_world, weights, n_rays, n_obj) ? DSP_E_ARG : DSP_OK;
}

int dsp_debug_align_objects_rows(int64_t n, const float* pts_world, const int32_t* winner, const int32_t* obj_row, const float* d, const float* grad_world,
                                 const float* weights, int64_t n_obj, double huber, double max_dist, double* sums) {
    if (n < 0 || n_obj < 0 || (n_obj > 0 && !sums) || (n > 0 && (!pts_world || !winner || !obj_row || !d || !grad_world))) return DSP_E_ARG;
    if (!std::isfinite(max_dist) || !std::isfinite(huber) || !(huber > 0.0) || !(huber <= max_dist)) return DSP_E_ARG;
    try {
        align_objects_rows_host(n, pts_world, winner, obj_row, d, grad_world, weights, n_obj, huber, max_dist, sums);
    } catch (const std::bad_alloc&) {
        return DSP_E_NOMEM;
    }
    return DSP_OK;
}

int dsp_debug_align_objects_compose(int64_t n, const double* correction, const float* t_world_obj, float* t_world_obj_out) {
    if (n < 0 || (n > 0 && (!correction || !t_world_obj || !t_world_obj_out))) return DSP_E_ARG;
    for (int64_t k = 0; k < n; ++k) align_objects_compose_host(correction + 16 * k, t_world_obj + 16 * k, t_world_obj_out + 16 * k);
    return DSP_OK;
}

void dsp_shapes_params_default(dsp_align_params* params, dsp_shapes_params* shapes) {
    if (params) {
        dsp_align_params_default(params);
        params->damp = 1e-4;
    }
    if (shapes) *shapes = dsp_shapes_params{DSP_SHAPES_CODE, 0.0, 0.0, 1e-6};
}

int dsp_map_align_shapes(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts_world, const float* origins_world,
                         const float* weights, int64_t n_rays, const unsigned char* refine, const dsp_align_params* params,
                         const dsp_shapes_params* shapes, const dsp_raycast_params* raycast, double max_gap, float* t_world_obj_out, float* codes_out,
                         double* correction, double* record, int32_t* obj, float* dist, float* t_hit, int32_t* status, double* trace) {
    if (!h || !params || !shapes || !raycast || n_obj < 0 || n_rays < 0) return DSP_E_ARG;
    const int n_out = (obj != nullptr) + (dist != nullptr) + (t_hit != nullptr) + (status != nullptr);
    if (n_out != 0 && n_out != 4) return DSP_E_ARG;
    if ((n_obj > 0 && (!t_world_obj || !codes || !t_world_obj_out || !codes_out || !correction || !record)) || (n_rays > 0 && !pts_world)) return DSP_E_ARG;
    return guarded(h, [&] {
        if (const char* why = align_objects_check_inputs(*params, *raycast, max_gap, origins_world, weights, n_rays, n_obj)) throw std::invalid_argument(why);
        if (const char* why = align_shapes_check_params(*shapes)) throw std::invalid_argument(why);
        const std::vector<float> tab = query_table(h, t_world_obj, codes, n_obj);
        align_shapes_run(h, tab, t_world_obj, codes, n_obj, pts_world, origins_world, weights, n_rays, refine, *params, *shapes, raycast_params(*raycast),
                         max_gap, t_world_obj_out, codes_out, correction, record, obj, dist, t_hit, status, trace);
    });
}

int dsp_map_align_shapes_last_stats(dsp_handle* h, int64_t* counts7) {
    if (!h || !counts7) return DSP_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    memcpy(counts7, h->as_stats, sizeof h->as_stats);
    return DSP_OK;
}

int dsp_debug_align_shapes_check(const dsp_align_params* params, const dsp_shapes_params* shapes, const dsp_raycast_params* raycast, double max_gap,
                                 const float* origins_world, const float* weights, int64_t n_rays, int64_t n_obj) {
    if (!params || !shapes || !raycast || n_rays < 0 || n_obj < 0 || n_obj > QUERY_MAX_OBJ) return DSP_E_ARG;
    if (align_shapes_check_params(*shapes)) return DSP_E_ARG;
    return align_objects_check_inputs(*params, *raycast, max_gap, origins_world, weights, n_rays, n_obj) ? DSP_E_ARG : DSP_OK;
}

int dsp_debug_align_shapes_rows(int64_t n, const float* pts_world, const int32_t* winner, const int32_t* obj_row, const float* d, const float* grad_world,
                                const float* gcode, const float* weights, int64_t n_obj, double huber, double max_dist, double* sums) {
    if (n < 0 || n_obj < 0 || (n_obj > 0 && !sums) || (n > 0 && (!pts_world || !winner || !obj_row || !d || !grad_world || !gcode))) return DSP_E_ARG;
    if (!std::isfinite(max_dist) || !std::isfinite(huber) || !(huber > 0.0) || !(huber <= max_dist)) return DSP_E_ARG;
    try {
        align_shapes_rows_host(n, pts_world, winner, obj_row, d, grad_world, gcode, weights, n_obj, huber, max_dist, sums);
    } catch (const std::bad_alloc&) {
        return DSP_E_NOMEM;
    }
    return DSP_OK;
}

int dsp_debug_align_shapes_step(const double* H4900, const double* b70, double W, const double* code, const float* code0, int32_t code_len,
                                const dsp_shapes_params* shapes, double damp, double lambda, const double* c16, int32_t* status, double* dx70,
                                double* c_trial16, double* code_trial64) {
    if (!H4900 || !b70 || !code || !code0 || !shapes || !c16 || !status || !dx70 || !c_trial16 || !code_trial64) return DSP_E_ARG;
    if (code_len < 1 || code_len > CODE_LEN || align_shapes_check_params(*shapes)) return DSP_E_ARG;
    double z0[CODE_LEN], dx[DSP_SHAPES_DIM];
    for (int c = 0; c < CODE_LEN; ++c) z0[c] = (double)code0[c];
    if (!align_shapes_solve_host(H4900, b70, W, code, z0, code_len, shapes->unknowns, shapes->code_reg, shapes->code_anchor, damp, lambda, dx)) {
        *status = DSP_ALIGN_SINGULAR;
        return DSP_OK;
    }
    *status = DSP_ALIGN_OK;
    memcpy(dx70, dx, sizeof dx);
    align_shapes_apply_step_host(dx, shapes->unknowns, code_len, c16, code, c_trial16, code_trial64);
    return DSP_OK;
}

int dsp_map_align_last_stats(dsp_handle* h, int64_t* counts5) {
    if (!h || !counts5) return DSP_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    memcpy(counts5, h->a_stats, sizeof h->a_stats);
    return DSP_OK;
}

int dsp_debug_align_check(const dsp_align_params* params, const double* t_world_sensor0, int64_t n_hyp, const float* weights, int64_t n_pts) {
    if (!params || n_hyp < 0 || n_pts < 0 || (n_hyp > 0 && !t_world_sensor0)) return DSP_E_ARG;
    return align_check_inputs(*params, t_world_sensor0, n_hyp, weights, n_pts) ? DSP_E_ARG : DSP_OK;
}

int dsp_debug_align_rows(int64_t n, const float* pts_world, const int32_t* obj, const float* dist, const float* grad_world, const float* weights,
                         double huber, double max_dist, double* sums30) {
    if (n < 0 || !sums30 || (n > 0 && (!pts_world || !obj || !dist || !grad_world))) return DSP_E_ARG;
    if (!std::isfinite(max_dist) || !std::isfinite(huber) || !(huber > 0.0) || !(huber <= max_dist)) return DSP_E_ARG;
    align_rows_host(n, pts_world, obj, dist, grad_world, weights, huber, max_dist, sums30);
    return DSP_OK;
}

int dsp_debug_align_step(const double* H36, const double* b6, double damp, double lambda, const double* t16, int32_t* status, double* xi6,
                         double* t_trial16) {
    if (!H36 || !b6 || !t16 || !status || !xi6 || !t_trial16) return DSP_E_ARG;
    if (!align_solve_host(H36, b6, damp, lambda, xi6)) {
        *status = DSP_ALIGN_SINGULAR;
        return DSP_OK;
    }
    *status = DSP_ALIGN_OK;
    align_apply_step_host(xi6, t16, t_trial16);
    return DSP_OK;
}

int dsp_map_query_last_stats(dsp_handle* h, int64_t* counts4) {
    if (!h || !counts4) return DSP_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    memcpy(counts4, h->q_stats, sizeof h->q_stats);
    return DSP_OK;
}

int dsp_debug_query_invert(int64_t n_obj, const float* t_world_obj, float* rt_ow, float* scale) {
    if (n_obj < 0 || (n_obj > 0 && (!t_world_obj || !rt_ow || !scale))) return DSP_E_ARG;
    for (int64_t o = 0; o < n_obj; ++o)
        if (!query_invert_host(t_world_obj + 16 * o, rt_ow + 12 * o, scale + o)) return DSP_E_ARG;
    return DSP_OK;
}

int dsp_debug_query_candidates(int64_t n_obj, const float* rt_ow, const float* scale, int64_t n_pts, const float* pts_world, float* p_obj,
                               unsigned char* inside, float* bound) {
    if (n_obj < 0 || n_pts < 0 || (n_obj > 0 && (!rt_ow || !scale)) || (n_pts > 0 && !pts_world)) return DSP_E_ARG;
    query_candidates_host(n_obj, rt_ow, scale, n_pts, pts_world, p_obj, inside, bound);
    return DSP_OK;
}

int dsp_debug_query_select(int64_t n_rows, const float* sdf, const float* scale_of_row, const int32_t* obj_of_row, const int32_t* pt_of_row,
                           int64_t n_pts, int32_t* obj, float* dist) {
    if (n_rows < 0 || n_pts < 0 || (n_rows > 0 && (!sdf || !scale_of_row || !obj_of_row || !pt_of_row)) || (n_pts > 0 && (!obj || !dist))) return DSP_E_ARG;
    for (int64_t r = 0; r < n_rows; ++r)
        if (pt_of_row[r] < 0 || pt_of_row[r] >= n_pts || obj_of_row[r] < 0) return DSP_E_ARG;
    query_select_host(n_rows, sdf, scale_of_row, obj_of_row, pt_of_row, n_pts, obj, dist);
    return DSP_OK;
}

int dsp_debug_query_plan(int64_t n_obj, const int32_t* cnt, int64_t budget, int64_t pass_n_obj, int64_t* sizes3, int32_t* chunks4, int32_t* base,
                         int32_t* tiles4, int64_t* pass_pts) {
    if (n_obj < 0 || n_obj > QUERY_MAX_OBJ || (n_obj > 0 && !cnt) || budget < 0 || budget > ((int64_t)1 << 24)) return DSP_E_ARG;
    if (pass_pts && (pass_n_obj < 1 || pass_n_obj > QUERY_MAX_OBJ)) return DSP_E_ARG;
    for (int64_t o = 0; o < n_obj; ++o)
        if (cnt[o] < 0) return DSP_E_ARG;
    if (pass_pts) *pass_pts = query_pass_pts(pass_n_obj);
    if (!sizes3 && !chunks4 && !base && !tiles4) return DSP_OK;
    std::vector<QueryChunk> plan;
    try {
        plan = query_plan_geometry(cnt, n_obj, budget > 0 ? budget : query_default_budget());
    } catch (const std::bad_alloc&) {
        return DSP_E_NOMEM;
    }
    int64_t nb = 0, nt = 0;
    for (const QueryChunk& c : plan) {
        if (chunks4) { chunks4[0] = c.o0; chunks4[1] = c.nc; chunks4[2] = c.n_rows; chunks4[3] = c.nt; chunks4 += 4; }
        if (base) memcpy(base + nb, c.base.data(), c.base.size() * sizeof(int));
        if (tiles4) memcpy(tiles4 + 4 * nt, c.tiles.data(), c.tiles.size() * sizeof(int4));
        nb += (int64_t)c.base.size();
        nt += (int64_t)c.tiles.size();
    }
    if (sizes3) { sizes3[0] = (int64_t)plan.size(); sizes3[1] = nb; sizes3[2] = nt; }
    return DSP_OK;
}

int dsp_debug_query_timing(dsp_handle* h, int on, double* ms2) {
    if (!h) return DSP_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    h->q_timing = on != 0;
    if (ms2) memcpy(ms2, h->q_ms, sizeof h->q_ms);
    return DSP_OK;
}

int dsp_debug_query_chunk_rows(dsp_handle* h, int64_t rows) {
    if (!h || rows < 0 || rows > ((int64_t)1 << 24)) return DSP_E_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    h->q_chunk_rows = rows;
    return DSP_OK;
}

}  // extern "C"
