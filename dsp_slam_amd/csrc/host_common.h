// Shared by the host files of libdspgn (no kernel file includes it): error plumbing, the device-block pool, the handle and guarded().
// What more than one host file uses lives in namespace dsp_host; what a single file needs stays in its anonymous namespace.
#pragma once
#include "dsp_gn.h"
#include "dsp_internal.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

using namespace dsp;

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) {                                                                             \
            char buf_[512];                                                                                 \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            throw std::runtime_error(buf_);                                                                 \
        }                                                                                                   \
    } while (0)

namespace dsp_host __attribute__((visibility("hidden"))) {

struct state_error : std::runtime_error {      // mapped to DSP_E_STATE by guarded()
    using std::runtime_error::runtime_error;
};
struct device_oom : std::bad_alloc {            // mapped to DSP_E_NOMEM by guarded(): hipMalloc failed twice (the second time with the handle's cache drained)
    const char* what() const noexcept override { return "out of device memory"; }
};

// Per-handle cache of device blocks.  The one-shot entry points (dsp_reconstruct_batch, dsp_estimate_pose_batch, the stand-alone
// residual terms: what SLAM calls once per detection, LocalMapping_util.cc:109-110,179-180) build a batch, run it and drop it; with
// ~45 arrays per batch that was ~45 hipMalloc + hipFree per call (0.8-1.1 ms, round-1 probe).  Blocks are rounded up to a size class
// and go back to the handle's pool instead; a later call of similar shape allocates nothing.  A block is only ever returned after the
// handle's stream has been synchronised (every entry point ends with a sync), so reuse cannot race with the device.
struct DevPool {
    std::mutex mu;
    std::unordered_map<size_t, std::vector<void*>> free_blocks;
    size_t cached_bytes = 0;
    int fail_after = -1;      // test hook (dsp_debug_fail_alloc): >= 0 = the (fail_after + 1)-th fresh device allocation from now on fails like an exhausted HBM
    static constexpr size_t MAX_BLOCK = (size_t)256 << 20, MAX_CACHED = (size_t)1 << 30;     // (dsp_trim hands everything back; destroying a LARGE resident batch trims to 64 MiB)
    static size_t size_class(size_t bytes) {       // powers of two x {1, 1.25, 1.5, 1.75}, at least 512 B: <= 25 % slack
        size_t c = 512;
        while (c < bytes) c <<= 1;
        if (c > 512) {
            const size_t q = c >> 3;                // c/2 .. c in steps of c/8
            for (size_t k = 5; k <= 7; ++k) if ((q * k) >= bytes) return q * k;
        }
        return c;
    }
    void* take(size_t bytes, size_t* got) {
        const size_t c = bytes > MAX_BLOCK ? bytes : size_class(bytes);
        *got = c;
        if (bytes <= MAX_BLOCK) {
            std::lock_guard<std::mutex> l(mu);
            auto it = free_blocks.find(c);
            if (it != free_blocks.end() && !it->second.empty()) {
                void* p = it->second.back();
                it->second.pop_back();
                cached_bytes -= c;
                return p;
            }
        }
        void* p = nullptr;
        bool injected = false;
        {
            std::lock_guard<std::mutex> l(mu);
            if (fail_after >= 0 && fail_after-- == 0) injected = true;
        }
        if (injected || hipMalloc(&p, c) != hipSuccess) {       // out of HBM with blocks parked here: release them and try once more
            (void)hipGetLastError();
            drain();
            if (injected || hipMalloc(&p, c) != hipSuccess) {
                (void)hipGetLastError();
                throw device_oom();                 // -> DSP_E_NOMEM; nothing of the half-built batch stays allocated (DevBuf destructors)
            }
        }
        return p;
    }
    void drain() {
        std::lock_guard<std::mutex> l(mu);
        for (auto& kv : free_blocks)
            for (void* q : kv.second) (void)hipFree(q);
        free_blocks.clear();
        cached_bytes = 0;
    }
    void trim_to(size_t keep) {          // largest blocks first, until at most `keep` bytes stay parked
        std::lock_guard<std::mutex> l(mu);
        std::vector<size_t> classes;
        for (auto& kv : free_blocks) classes.push_back(kv.first);
        std::sort(classes.rbegin(), classes.rend());
        for (size_t c : classes) {
            auto& v = free_blocks[c];
            while (cached_bytes > keep && !v.empty()) { (void)hipFree(v.back()); v.pop_back(); cached_bytes -= c; }
        }
    }
    void give(void* p, size_t c) {
        if (c <= MAX_BLOCK) {
            std::lock_guard<std::mutex> l(mu);
            if (cached_bytes + c <= MAX_CACHED) {
                free_blocks[c].push_back(p);
                cached_bytes += c;
                return;
            }
        }
        (void)hipFree(p);
    }
    ~DevPool() { drain(); }
};
inline thread_local DevPool* t_pool = nullptr;       // the pool allocations of the current call go through (set by guarded(): the handle's)
struct PoolScope {
    DevPool* saved;
    explicit PoolScope(DevPool* p) : saved(t_pool) { t_pool = p; }
    ~PoolScope() { t_pool = saved; }
};

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevPool* pool = nullptr;      // where the block came from (nullptr: hipMalloc)
    size_t bytes = 0;
    void alloc(size_t count) {
        free();
        if (count == 0) count = 1;
        if (t_pool) {
            p = static_cast<T*>(t_pool->take(count * sizeof(T), &bytes));
            pool = t_pool;
        } else {
            if (hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); p = nullptr; throw device_oom(); }
            bytes = count * sizeof(T);
        }
        n = count;
    }
    void ensure(size_t count) { if (count > n) alloc(count + count / 4); }
    void free() {
        if (!p) return;
        if (pool) pool->give(p, bytes); else (void)hipFree(p);
        p = nullptr; n = 0; pool = nullptr; bytes = 0;
    }
    ~DevBuf() { free(); }
};

// pinned host staging: uploads of a batch go through it as asynchronous copies on the handle's stream (one synchronisation instead of
// one blocking pageable copy per array), and a run's results come back through it in the copy that precedes the run's final sync
struct HostStage {
    char* p = nullptr;
    size_t n = 0;
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
    void ensure(size_t bytes) {
        if (bytes <= n) return;
        if (p) (void)hipHostFree(p);
        p = nullptr; n = 0;
        const size_t want = std::max<size_t>(bytes + bytes / 2, (size_t)1 << 20);
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p), want, hipHostMallocDefault));
        n = want;
    }
    ~HostStage() { if (p) (void)hipHostFree(p); }
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace dsp_host
using namespace dsp_host;

struct dsp_handle {
    DevPool pool;              // FIRST member: destroyed last, after every DevBuf below has handed its block back
    std::mutex mu;             // every entry point that touches the handle's stream / scratch holds it (see guarded())
    std::atomic<int> pins{0};  // calls in flight that reached this handle through one of its batch tokens (BatchRef): dsp_destroy waits for them
    int device = 0;
    hipStream_t stream = nullptr;
    HostStage stage_in, stage_out;        // pinned: uploads of a batch / the results + counters of a run
    bool stage_in_busy = false;           // asynchronous uploads from stage_in may still be in flight (cleared by the next stream sync)
    std::vector<hipEvent_t> event_pool;   // timing events of dropped batches, reused by the next one
    ~dsp_handle() { for (auto e : event_pool) (void)hipEventDestroy(e); }
    std::string err;
    int n_cu = 256;
    // packed decoder
    DevBuf<float> wstream, wsplit, wcluster, bias_tab, codew, b0, blat;
    int cl_off[16] = {}, cl_len[16] = {};                     // per-wave-slot layout of wcluster (cluster-form kernel), in 4 KiB mini-chunks
    DevBuf<float> cl_xbuf;                                    // cluster form: exchange buffers, [n_clusters][2][CL_XCH_UNITS][64] tagged 16-byte units
    unsigned cl_epoch = 0;                                    //   counter base of the next launch (advanced by CL_EPOCH_STRIDE per launch)
    unsigned cl_spin_ticks = CL_SPIN_TICKS_DEFAULT;           //   bound of the cluster kernel's spins, 100 MHz ticks (dsp_debug_cluster_timeout)
    int cl_cooldown = 0;                                      //   runs for which the cluster form stays off after a lost hand-off (the GPU is shared and busy: try again later)
    int cl_fallbacks_total = 0;                               //   launches on this handle that fell back to the latency form on the device
    int n_clusters = 0;                                       //   clusters of 4 workgroups the chip holds at once (multiple of 8)
    int split_off[4] = {0, 0, 0, 0}, split_len[4] = {0, 0, 0, 0}, split_len_fwd[4] = {0, 0, 0, 0};   // per-wave layout of wsplit (latency-form kernels)
    std::vector<float> h_codew, h_b0, h_blat;   // host copies for the single-shot decoder calls
    float b_last = 0.f;
    int wlast_row = 0, w0_row = 0;
    int n_bias_rows = 0, n_fwd = 0, n_pass_all = 0, chunks_fwd = 0, chunks_all = 0;
    int lat_tile = 27, code_len = CODE_LEN;
    PassDesc pass[MAX_PASSES];
    // low-precision prepass (mlp_lp_kernel.hip): packed 16-bit weight streams [0] = f16, [1] = bf16 and their pass table
    DevBuf<uint16_t> wlp[2];
    LpPass lp_pass[LP_MAX_PASSES];
    int lp_n_pass = 0, lp_chunks = 0;
    bool lp_ok = false;        // decoder geometry supported by the prepass kernel (hidden width 512)
    // low-precision compute mode (mlp_lpj_kernel.hip): the transposed 16-bit stream of the backward kernel and its pass table
    DevBuf<uint16_t> wlpj[2];
    LpPass lpj_pass[LPJ_MAX_PASSES];
    int lpj_chunks = 0;
    bool lpj_ok = false;       // ... and by the 16-bit jacobian kernels (eight hidden layers, the latent_in layer fourth: DeepSDF)
    DevBuf<uint4> s_lpj_masks; // scratch of the single-shot dsp_sdf_jacobian_lp
    // calibration at dsp_create (calibrate_prepass), per dtype: largest |sdf_lp - sdf_fp32| with codes drawn at each magnitude of
    // LP_MAGS, and the margin table derived from it (delta = 6 x error, monotone in the magnitude, floor, cap 0.5)
    float lp_err[2][LP_NMAG] = {};
    LpDeltaTab lp_tab[2] = {};
    float lp_guard_err[2] = {0.f, 0.f};   // largest error any guard trip on this handle has reported: the tables are raised to 4 x that
    double guard_trips_total = 0.0, guard_reruns_total = 0.0;
    // scratch of the single-shot decoder calls
    DevBuf<float4> s_pts;
    DevBuf<float> s_code, s_out, s_cbias;
    DevBuf<int4> s_tiles;
    DevBuf<int> s_ntiles;
    DevBuf<unsigned long long> s_clk;
    // mesh extraction: case table, scan scratch and the last extracted mesh (device resident until fetched)
    DevBuf<McTables> mc_tab;
    DevBuf<int2> mc_blocks;
    DevBuf<long long> mc_totals;
    DevBuf<float> mc_vol, mc_verts;
    DevBuf<int> mc_vidmap, mc_faces;
    int64_t mesh_nv = -1, mesh_nf = -1;
    // batched extraction (extract_meshes_impl): chunk volumes, surface-band lists, tile list, per-object counters and guard words
    DevBuf<float> mb_vol, mb_val;
    DevBuf<float4> mb_pts;
    DevBuf<long long> mb_idx;
    DevBuf<int4> mb_tiles;
    DevBuf<int> mb_cnt;           // [n] selected, [n] audited, [n] first tile, [1] tiles
    DevBuf<unsigned> mb_guard;    // [n][3] {delta, trips, max err}
    DevBuf<int2> mb_base;         // first (vertex, face) of every object of the chunk
    // ... the concatenated meshes of the last dsp_extract_meshes (device resident until dsp_meshes_fetch) and their counts
    DevBuf<float> mm_verts;
    DevBuf<int> mm_faces;
    std::vector<int64_t> mm_nv, mm_nf;
    bool mm_valid = false;
    // ... what dsp_meshes_refine needs of that call (the codes, one voxel of its grid) and what it leaves until dsp_meshes_fetch_attributes:
    // refined vertices, normals, sdf and -- with a variance -- sigma of every vertex, in the order of mm_verts
    std::vector<float> mm_codes;
    float mm_voxel = 0.f;
    DevBuf<float> mr_verts, mr_normals, mr_sdf, mr_sigma;
    bool mr_valid = false, mr_has_var = false;
    // surface projection (surface_run): per-object variances of a call, and the chunk budget in rows (0 = SURFACE_CHUNK_BYTES; dsp_debug_surface_chunk_rows)
    DevBuf<float> sf_var;
    int64_t sf_chunk_rows = 0;
    // map query (query_run): a pass's wave counts and object counts; a chunk's row bases and row -> {point, object}; the chunk budget in
    // rows (0 = QUERY_CHUNK_BYTES; dsp_debug_query_chunk_rows) and the last call's stats.  (The call's own arrays -- points, object table,
    // per-point results -- are blocks of the pool for the length of the call.)
    DevBuf<int> q_wave_cnt, q_cnt, q_base;
    DevBuf<int2> q_row_meta;
    int64_t q_chunk_rows = 0;
    int64_t q_stats[4] = {0, 0, 0, 0};      // candidate rows, decoder tiles, chunks, point passes
    bool q_timing = false;                  // dsp_debug_query_timing: bracket the decoder launches with events ...
    double q_ms[2] = {0.0, 0.0};            // ... {decoder launches, whole call} of the last call, ms on the handle's stream
    // map alignment (align_run) runs the query's core on the scratch above; the last call's stats
    int64_t a_stats[5] = {0, 0, 0, 0, 0};   // candidate rows, decoder tiles, chunks, point passes, evaluations
    // ray casting (raycast_run) holds its arrays as blocks of the pool for the length of the call and shares q_chunk_rows; the last call's stats
    int64_t r_stats[6] = {0, 0, 0, 0, 0, 0};    // pairs, decoder rows, tiles, rounds run, passes, exhausted pairs
    int64_t ar_stats[7] = {0, 0, 0, 0, 0, 0, 0};    // ray alignment (align_rays_run): the six above summed over the evaluations, evaluations
    int64_t ao_stats[7] = {0, 0, 0, 0, 0, 0, 0};    // object refinement (align_objects_run): likewise, the extra evaluation behind the per-ray outputs included
    int64_t as_stats[7] = {0, 0, 0, 0, 0, 0, 0};    // shape refinement (align_shapes_run): likewise
    // dsp_mesh_last_stats: prepass points, fp32 band points, fp32 audit points, points decoded densely in fp32, objects re-run dense;
    // largest guard error
    int64_t ms_counts[5] = {0, 0, 0, 0, 0};
    float ms_max_err = 0.f;
};

namespace dsp_host __attribute__((visibility("hidden"))) {

std::string& create_error();      // what dsp_last_error(NULL) reports: thread local, owned by dsp_gn.hip

// The exception in flight -> (code, message).  Call it inside a catch block.
inline int translate_error(std::string& msg) {
    try {
        throw;
    } catch (const std::invalid_argument& e) {
        msg = e.what();
        return DSP_E_ARG;
    } catch (const device_oom& e) {
        msg = e.what();
        return DSP_E_NOMEM;
    } catch (const std::bad_alloc&) {
        msg = "out of host memory";
        return DSP_E_NOMEM;
    } catch (const state_error& e) {
        msg = e.what();
        return DSP_E_STATE;
    } catch (const std::exception& e) {
        msg = e.what();
        return DSP_E_HIP;
    }
}

template <class F>
int guarded(dsp_handle* h, F f) {
    // one call at a time per handle: its HIP stream, scratch buffers and last mesh are shared state, and ctypes / pybind11
    // callers release the GIL around these calls, so two Python threads can arrive here together
    std::unique_lock<std::mutex> lock;
    if (h) lock = std::unique_lock<std::mutex>(h->mu);
    PoolScope pool_scope(h ? &h->pool : nullptr);      // device blocks allocated inside f come from / go back to the handle's pool
    try {
        f();
        return DSP_OK;
    } catch (const std::exception&) {
        return translate_error(h ? h->err : create_error());
    }
}

}  // namespace dsp_host
