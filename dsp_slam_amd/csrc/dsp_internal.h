// Internal definitions shared by the HIP kernels and the host side of libdspgn.
// (The public C-ABI is include/dsp_gn.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdexcept>

#include "prior_math.h"
#include "raycast_math.h"
#include "step_rule.h"

namespace dsp {

// ---- decoder geometry the MLP kernel is built for (DeepSDF as used by DSP-SLAM) -------------
// hidden width 512, code length 64, one latent_in layer; see DESIGN.md "MLP kernel".
constexpr int WIDTH = 512;          // hidden width == slab rows
constexpr int CODE_LEN = 64;
constexpr int IN_DIM = CODE_LEN + 3;
constexpr int TILE_PTS = 64;        // points per workgroup tile (4 waves x 16)
constexpr int SPLIT_TILE_PTS = 16;  // points per workgroup tile of the latency form (4 waves share them, mlp_split_kernel.hip)
constexpr int WAVE_PTS = 16;
constexpr int KSTEPS_PER_CHUNK = 16;            // 16 MFMA k-steps (64 slab rows) per weight chunk
constexpr int CHUNK_BYTES = KSTEPS_PER_CHUNK * 64 * 16;   // 16 KiB: [kstep][lane] float4
constexpr int MAX_PASSES = 32;
constexpr int GRAD_STRIDE = 68;     // per-point output row: d/dcode[64], d/dxyz[3], sdf

// One "pass" = one dense layer traversal (forward layer or backward layer) of the weight stream.
struct PassDesc {
    int16_t nog;        // number of 64-row output groups
    int16_t nchunks;    // number of 64-row K chunks per output group
    int16_t bias_row;   // row of the LDS bias table to start the accumulators from, -1 = zero, -2 = per-object code bias
    int16_t relu;       // 1: relu + store mask (forward hidden layer)
    int16_t mask_slot;  // forward: slot the relu mask is stored to; backward: slot applied; -1 none
    int16_t kind;       // 1 fwd hidden, 2 fwd latent_in layer, 3 bwd, 4 bwd latent_in, 5 bwd first layer (code rows only)
    int32_t chunk_base; // first chunk of this pass in the packed stream
};

// Tile list of a ONE-object batch without a list: the decoder kernels derive their tiles from the object's counters themselves (the
// k_build_tiles launch in front of them goes: 4.6 us + a kernel boundary, twice per iteration of a detection).  kind 0 = off (tiles /
// n_tiles are read); 1 = forward list over the V in-sphere samples (with the "< 10 samples" rule of loss.py:73-74 and the work
// counters k_build_tiles mode 0 keeps); 3 = jacobian list, n0 surface points then the P band rows (k_build_tiles mode 3).
struct ObjState;
struct DirectTiles {
    int kind;
    int off0, n0, off1;         // first point of segment 0 / its length where the host knows it (surface points) / first point of segment 1
    ObjState* st;               // the object's state: status, V, P
    double* counters;           // dsp_batch::counters()
};
struct DirectList { int n_tiles, nt0, n0, n1; };

struct MlpArgs {
    const float* wstream;       // packed weight stream (fwd passes then bwd passes), chunk-major
    const float* bias_tab;      // [n_bias_rows][512]: hidden biases, last row = final layer weights
    float b_last;               // final layer bias
    int n_bias_rows;            // hidden biases b1.., final-layer weights (row wlast_row), first-layer xyz columns (rows w0_row..+2)
    int wlast_row, w0_row;
    int n_fwd;                  // number of forward passes (hidden layers)
    int n_pass;                 // fwd (+ bwd when BWD)
    int total_chunks;           // chunks consumed per tile
    PassDesc pass[MAX_PASSES];
    // work list (device memory, produced on device)
    const int* n_tiles;         // [1] one past the last tile
    const int* tile_begin;      // optional [1]: first tile (0 when null)
    const int4* tiles;          // [n_tiles] {first point, n points, object (code index), output offset added to the point index}
    const float4* pts;          // object-frame points (xyz, w unused)
    const int* index;           // forward kernel, optional: point i of a tile is pts[index[first + i]] and its sdf goes to
                                // out_sdf[index[first + i]] (front-to-back ray passes evaluate a subset of the sample list)
    const float* code_bias;     // per object: [0..511] = W0[:, :64] code + b0, [512..1023] = W_lat[:, code cols] code + b_lat
    int code_bias_stride;       // in floats (multiple of 4)
    unsigned short* mask_buf;   // MODE 1 writes / MODE 3 reads: [sample][lane group 4][layer 8][output group 8] relu bits (16 per word)
    const float* sdf_in;        // MODE 3: sdf of the samples, as written by the forward launches
    float th;                   // MODE 1: export masks of samples with |sdf| < th
    int seed_slot;              // MODE 3: mask slot of the last hidden layer
    int lat_tile;               // 16-row slab tile of the latent_in layer's re-injected xyz: 27 (rows 445..447, 64-D codes) or 29 (477..479, 32-D)
    float* out_sdf;             // FWD: [n_points]
    float* out_grad;            // BWD: [n_points][GRAD_STRIDE]
    // always-on guard of the low-precision pre-classification (prepass_guard, mlp_common.h): the fp32 kernels compare every sample they
    // re-decode with the prepass value it replaces.  guard = per-object words {lp_delta (float), trips, max error (float bits)} of object 0,
    // guard_stride words apart (inside ObjState); nullptr = off
    unsigned* guard;
    int guard_stride;
    float* sdf_scatter;         // BWD, optional: tiles from *scatter_tile_begin on also store their sdf at sdf_scatter[int(pt.w)] (speculative band rows)
    const int* scatter_tile_begin;
    const int* bwd_only_tile_begin;   // latency form, mixed launch: tiles from *this on run the backward sweep only, from exported masks (mlp_split_kernel<2>); nullptr = none
    const float* wsplit;        // latency form (mlp_split_kernel): the same chunks laid out per wave (see pack_decoder)
    int split_off[4];           //   first chunk of wave w's stream inside wsplit
    int split_len[4];           //   chunks wave w consumes per tile (forward + backward)
    int split_len_fwd[4];       //   ... of which the forward passes (a prefix of the wave's stream)
    unsigned long long* clk;    // optional: block 0 writes {clock64, wall_clock64} at entry and exit (effective shader clock)
    // cluster form (mlp_cluster_kernel.hip): four workgroups per 16-point tile, layer rows split over their 16 waves
    const float* wcluster;      //   the same chunks laid out per wave slot (two row tiles, two k-steps per 16-byte element; pack_decoder)
    int cl_off[16];             //   first 4 KiB mini-chunk of wave slot u inside wcluster
    int cl_len[16];             //   mini-chunks slot u consumes per tile (forward + backward)
    float* cl_xbuf;             //   exchange buffers: [cluster][2 parities][16 wave slots x 3 units][64 lanes] x 16 B (3 floats + counter tag)
    unsigned* cl_err;           //   raised when a bounded spin ran out: the latency-form kernel behind the cluster kernel then takes the list (device-side fallback)
    unsigned cl_spin_ticks;     //   bound of every spin in ticks of the 100 MHz wall clock (CL_SPIN_TICKS_DEFAULT = 2 ms)
    double* cl_tiles_done;      //   optional: + the list's tile count when the cluster kernel takes it (dsp_stats.n_cluster_tiles)
    unsigned cl_epoch_base;     //   counter value this launch starts from (the host advances it by CL_EPOCH_STRIDE per launch)
    int cl_fault;               //   fault injection (tests): workgroup 3 of every cluster never publishes -> its siblings' bounded spins run out
    int cluster_max_tiles;      //   the cluster kernel runs lists of up to this many tiles ...
    int split_min_tiles;        //   ... and the latency form (mlp_split_kernel<2>) lists of at least this many (0 = always)
    DirectTiles direct;         // one-object batches: no tile list (kind != 0)
};
constexpr unsigned CL_SPIN_TICKS_DEFAULT = 200000;   // 2 ms: ~500 healthy hand-offs of ~3.5 us
constexpr int CL_EPOCH_STRIDE = 4096;      // exchanges a launch may count: 15 per tile and cluster
constexpr int CL_XCH_UNITS = 16 * 3;         // tagged 16-byte units per lane in one parity of a cluster's global exchange buffer (mlp_cluster_kernel.hip)


// ---- low-precision prepass (mlp_lp_kernel.hip): f16 / bf16 MFMA forward used ONLY to classify ray samples ------------
// Occupancy is exactly 0 for sdf >= th and exactly 1 for sdf <= -th (loss_utils.py:40-48), so a sample whose low-precision
// sdf is farther than a calibrated margin from the band needs no fp32 decode at all (DESIGN.md "Prepass").
constexpr int LP_TILE_PTS = 128;    // points per workgroup tile (4 waves x 32)
constexpr int LP_TILE_PTS_SMALL = 64;   // ... of the latency form (4 waves x 16: one column block per wave), for lists that fill less than half the chip
constexpr int LP_WAVE_PTS = 32;
constexpr int LP_NBUF = 8;          // LDS ring depth in 16 KiB chunks
constexpr int LP_KSTEPS_PER_CHUNK = 8;   // chunk = 8 k-steps (of 16 slab rows) x 2 row tiles (of 32 output rows) x 1 KiB
constexpr int LP_MAX_PASSES = 12;
constexpr int LP_XYZ_KSTEPS = 2;    // k-steps reserved for the split-precision xyz products (f16 uses one, bf16 two)

// xyz enters layer 0 and the latent_in layer as sums of low-precision parts: x = x1 + x2 (+ x3), w = w1 + w2 (+ w3),
// x.w ~ sum of the listed (x part, w part) products -- 22-24 significant bits, so the prepass error is set by the hidden
// layers' activation rounding only.  Entry [kstep][term] = 4 * xpart + wpart (parts 1-based), 0 = unused; MFMA k index
// of (term t, coordinate c) = 3 t + c.
constexpr unsigned char LP_XYZ_TERMS[2][LP_XYZ_KSTEPS][5] = {
    {{4 * 1 + 1, 4 * 2 + 1, 4 * 1 + 2, 4 * 2 + 2, 0}, {0, 0, 0, 0, 0}},                                   // f16
    {{4 * 1 + 1, 4 * 2 + 1, 4 * 3 + 1, 4 * 1 + 2, 4 * 2 + 2}, {4 * 1 + 3, 4 * 3 + 2, 4 * 2 + 3, 0, 0}},   // bf16
};

struct LpPass {
    int16_t nog;        // 64-row output groups (2 MFMA row tiles each)
    int16_t nchunks;    // chunks per group = ceil(k-steps / 8)
    int16_t bias_row;   // row of the fp32 bias table; -2 = per-object latent_in code bias, -3 = per-object layer-0 code bias
    int16_t kind;       // 0 first layer (xyz k-steps only), 1 hidden, 2 latent_in (slab k-steps, then xyz k-steps)
    int16_t npad;       // latent_in layer: padding k-steps between the slab rows and the xyz k-steps (the xyz B operands sit at
                        // fixed k-steps: 0, 1 of the first layer; the last two of the latent_in layer's groups)
    int16_t last;       // 1: final 512->1 layer + tanh follow in the epilogue
    int32_t chunk_base;
};

struct LpArgs {
    const void* wstream;        // packed 16-bit weight stream, chunk-major (pack_decoder_lp)
    const float* bias_tab;      // the fp32 kernel's table: hidden biases, final-layer weights (row wlast_row)
    float b_last;
    int n_bias_rows, wlast_row;
    int n_pass, total_chunks;
    LpPass pass[LP_MAX_PASSES];
    const int* n_tiles;
    const int4* tiles;          // {first point, n points (<= 128), object, output offset}
    const float4* pts;
    const int* index;           // optional indirection, as MlpArgs::index
    const float* code_bias;     // per object [2][512] fp32 (k_code_bias)
    int code_bias_stride;
    float* out_sdf;
    unsigned long long* clk;
    DirectTiles direct;         // one-object batches: no tile list (kind != 0)
};

// ---- low-precision compute mode (mlp_lpj_kernel.hip): forward + input gradient on 16-bit MFMA operands ------------------------------
constexpr int LPJ_MAX_PASSES = 8;   // eight forward passes (the prepass stream: mlp_lpj_fwd_kernel) or eight backward passes (mlp_lpj_bwd_kernel)
struct LpjArgs {
    const void* wstream;        // the prepass stream (forward kernel) or the transposed stream (backward kernel: pack_decoder_lpj_host), chunk-major
    const float* bias_tab;
    float b_last;
    int n_bias_rows, wlast_row;
    int total_chunks;
    LpPass pass[LPJ_MAX_PASSES];   // backward passes, last hidden layer first: kind 3 hidden, 4 latent_in (also yields the re-injected rows' gradient), 5 first layer (two output groups)
    const int* n_tiles;
    const int4* tiles;          // {first point, n points (<= 128), object, output offset}
    const float4* pts;
    const float* code_bias;     // per object [2][512] fp32 (k_code_bias)
    int code_bias_stride;
    float* out_grad;            // [point + offset][GRAD_STRIDE]: d/dcode[64], d/dxyz[3], sdf -- what mlp_kernel<2> writes
    uint4* mask_buf;            // [tile][8 layers][4 waves][2 column blocks][64 lanes] x 16 B: the relu masks (forward kernel writes, backward kernel reads)
    int lat_tile;               // 27 (64-D codes) / 29 (32-D)
    unsigned long long* clk;
};

// ---- Gauss-Newton batch state ------------------------------------------------------------------
constexpr int DSP_STATUS_GOOD = 0;
constexpr int DSP_STATUS_FEW = 1;    // < 10 in-sphere samples (loss.py:73-74)
constexpr int DSP_STATUS_NAN = 2;    // NaN loss / singular system (optimizer.py:135-136,149-150)
constexpr int DSP_STATUS_SKIP = 3;   // internal: not part of this (partial re-)run; never leaves the library (k_init_state run_mask, k_finalize)
// internal: converged under the batch's convergence rule (dsp_batch_convergence) and FROZEN for the rest of the run: like SKIP it is
// "not GOOD" to every kernel -- no tiles, rows, guard samples, no write to the state -- but k_finalize writes its row and reports DSP_OBJ_GOOD
constexpr int DSP_STATUS_DONE = 4;
constexpr int MAX_DEPTH_SAMPLES = 64;
// the run summary, ONE device block of 32-bit words: [8 fp64 work counters | 4 audit words | B x {margin, trips, max error} | B words: updates applied]
constexpr int SUM_COUNTERS = 0, SUM_AUDIT = 16, SUM_GUARD = 20, SUM_GUARD_WORDS = 3;
constexpr int SUM_HEAD_WORDS = SUM_GUARD;       // what a run zeroes at its start: the counters and the audit words
constexpr size_t sum_iters(int B) { return SUM_GUARD + (size_t)B * SUM_GUARD_WORDS; }
constexpr int TRACE_STRIDE = 5344;   // 71*71 H | 71 b | 71 dx | 16 t_oc | 64 code | V m K | vsum lo,hi | ksum lo,hi | pad | 64 depths

struct ObjConst {           // static layout of one object inside the batch arrays
    int pts_off, n_pts;     // surface points (camera frame)
    int ray_off, n_rays, n_fg;
    int depth_off;          // foreground depths
    int samp_off;           // segment of the in-sphere sample list (capacity roundup64(n_rays * D))
    int jsdf_off;           // jacobian-point segment, surface term (capacity roundup64(n_pts))
    int jren_off;           // jacobian-point segment, render term (capacity = sample capacity)
    int view_member;        // 1: one view of a multi-view group (GroupEnt): with < 10 in-sphere samples (loss.py:73-74) the view contributes no render
                            // rows in that iteration -- the OBJECT's status is decided over the whole group (k_group_reduce); 0: an object of its own
};

// Multi-view batches (dsp_batch_create_multiview): one entry per batch member.  A group = the views of one object, consecutive members; its
// first member (view 0, the reference camera) is the leader and carries the object's pose and code; member v samples at T_oc_v = T_oc * t_ref.
struct GroupEnt {
    int leader;             // member index of the group's first view
    int n_members;          // views of the group (read at the leader)
    int object;             // index of the object = row of the packed results
    int pad;
    float t_ref[16];        // view camera -> reference camera, rigid (identity for the leader)
};

struct ObjState {           // per-object optimiser state, lives on the device for the whole run
    float t_oc[16];         // camera -> object Sim(3)/SE(3)   (t_obj_cam)
    float t_co[16];
    float code[CODE_LEN];
    float depths[MAX_DEPTH_SAMPLES];
    float scale, dmin, dmax, loss;
    int status, V, m, K;
    int n_alive;
    int P;                  // samples selected for the current front-to-back pass
    unsigned vsum, ksum;    // order-independent checksums of the in-sphere set and of the kept (jacobian) sample set
    // prepass: this object's margin (from the magnitude of its CURRENT code, lp_delta_of), and what the guard saw
    float lp_delta;
    unsigned guard_trips;   // waves that re-decoded a sample whose prepass value was off by >= lp_delta / 2
    unsigned guard_err;     // largest |sdf_lp - sdf_fp32| over the re-decoded samples (float bits)
    int n_iter;             // Gauss-Newton updates applied so far in this run (k_solve; dsp_batch_iterations_used)
};

#ifdef __HIPCC__
// (wave-uniform: kernel arguments and scalar loads only; no side effects -- every workgroup of every kernel that may take the list calls it)
__device__ __forceinline__ DirectList direct_list(const DirectTiles& d, int tile_pts) {
    DirectList l{0, 0, 0, 0};
    const int status = d.st->status;
    if (d.kind == 1) {
        const int V = d.st->V;
        l.n0 = (status == DSP_STATUS_GOOD && V >= 10) ? V : 0;          // "< 10 in-sphere samples": the object fails (direct_commit records it)
    } else {
        const bool good = status == DSP_STATUS_GOOD;
        l.n0 = good ? d.n0 : 0;
        l.n1 = good ? d.st->P : 0;
    }
    l.nt0 = (l.n0 + tile_pts - 1) / tile_pts;
    l.n_tiles = l.nt0 + (l.n1 + tile_pts - 1) / tile_pts;
    return l;
}
// ONE thread of the ONE kernel that takes the list: what k_build_tiles records besides the list
__device__ __forceinline__ void direct_commit(const DirectTiles& d, const DirectList& l) {
    if (d.kind == 1) {
        if (d.st->status == DSP_STATUS_GOOD && d.st->V < 10) d.st->status = DSP_STATUS_FEW;
        d.counters[4] += (double)l.n0;
        d.counters[2] += (double)l.n0;
    } else {
        d.counters[1] += (double)l.n0;
        d.counters[3] += (double)l.n1;
    }
}
__device__ __forceinline__ int4 direct_tile(const DirectTiles& d, const DirectList& l, int tile, int tile_pts) {
    if (tile < l.nt0) return make_int4(d.off0 + tile * tile_pts, min(tile_pts, l.n0 - tile * tile_pts), 0, 0);
    const int t = tile - l.nt0;
    return make_int4(d.off1 + t * tile_pts, min(tile_pts, l.n1 - t * tile_pts), 0, 0);
}
#endif
static_assert(sizeof(ObjState) % 16 == 0, "ObjState is addressed as float4-aligned rows");

// Prepass margin as a function of the code's largest entry: calibrate_prepass (decoder_calls.hip) measures the largest |sdf_lp - sdf_fp32|
// with codes drawn at each of these magnitudes; delta is interpolated between them (linear extrapolation above, capped at 0.5).
constexpr int LP_NMAG = 5;
struct LpDeltaTab {
    float mag[LP_NMAG];
    float delta[LP_NMAG];
};

struct GnParamsDev {
    float k1, k2, k3, k4, b1, b2, lr, s_damp, cut_off;
    int n_depth, pose_only;
    int code_len;       // of the decoder (32 or 64); the state always carries CODE_LEN entries
    LpDeltaTab lp;      // prepass margin table of the dtype in use (all entries equal when the caller fixed delta)
};

// Convergence rule of a run (dsp_batch_convergence), evaluated by k_solve<., true> in fp64 on the step it has just applied: the object is
// frozen (DSP_STATUS_DONE) when iter + 1 >= min_iterations, every |lr dx_pose| < pose_tol and every |lr dx_code| < code_tol (strict: a
// tolerance of 0 stops nothing, +inf switches its half off, a NaN step never passes)
struct StopRule {
    double pose_tol, code_tol;
    int min_iterations;
};

// Gaussian prior on pose and code (dsp_batch_prior; arithmetic in prior_math.h), per OBJECT (multi-view: per object, not per view):
// k_prior_terms reads the state, t0, z0 and Lp and leaves [H_extra | b_extra] in `extra` for k_solve<.., PRIOR = true> / k_posterior<., true>;
// its final pass leaves e and chi2 in `res` (prior_math::RES_STRIDE doubles per object) for the run's read-back.
struct PriorDev {
    const float* t0 = nullptr;          // 16 per object: the prior's t_obj_cam
    const float* z0 = nullptr;          // CODE_LEN per object
    const double* Lp = nullptr;         // n x n per object, symmetric bit for bit
    const unsigned char* on = nullptr;  // per object: 0 = Lambda is all zero, the object has no prior
    double* extra = nullptr;            // n x (n + 1) per object
    double* res = nullptr;
    int n = 0;                          // 71, pose-only batches 6
};

// Levenberg-Marquardt step control (dsp_batch_step_control; the rule: step_rule.h), joint batches only.  k_solve<.., STEP = true> keeps one
// StepObj and one saved system [H | b] (STEP_SYS doubles: 71 rows of 72) per object and writes one log entry per iteration and object.
constexpr int STEP_SYS = 71 * 72;
struct StepObj {
    double F_acc, lambda;       // cost of the accepted state; the damping the next step is solved with
    float loss_acc;             // ObjState::loss at the accepted state
    int pad;
    float t_oc[16];             // the accepted state x_acc
    float code[CODE_LEN];
};
struct StepLogEnt {
    double cost, lambda;        // F_e; lambda after the decision
    int decision, pad;          // step_rule::NOT_EVALUATED / ACCEPTED / REJECTED
};
struct StepDev {
    step_rule::Params p{0.0, 0.0, 0.0, 0.0, 0.0};
    double* sys = nullptr;      // [object][STEP_SYS]
    StepObj* obj = nullptr;     // [object]
    StepLogEnt* log = nullptr;  // [iteration][object]
    int last = 0;               // the run's last iteration: evaluate and decide, apply no step
};

// Per-observation weights (dsp_batch_observation_weights), all null = off: the run's launches are those of a batch without them.  A weight
// multiplies the observation's squared residual: H gets sum w J^T J, b gets -sum w J^T r~, and the means divide by the sums of the weights
// (fp64, fixed order: k_weight_sums) instead of the counts.  A ray of weight 0 is absent: never sampled.
struct ObsWeightsDev {
    const float* pt_w = nullptr;    // per surface point, in the order of the inputs (ObjConst::pts_off)
    const float* ray_w = nullptr;   // per ray (ObjConst::ray_off)
    float* jw = nullptr;            // per jacobian row, render rows only (from ObjConst::jren_off): the weight of the row's ray, written by the row writers
    double* sums = nullptr;         // 2 per member: sum of w over the (alive) surface points, over the kept render rows
    double* gsums = nullptr;        // multi-view batches, 2 per member, written at the leaders: the group's pooled sums (k_group_reduce)
};

// Observation report (dsp_batch_report): the device arrays of one batch, in the order of the inputs -- points by pts_off, rays by ray_off,
// 8 doubles per member.
struct ReportDev {
    float* pt_sdf = nullptr;
    unsigned char* pt_flags = nullptr;
    float* ray_depth = nullptr;
    float* ray_hit = nullptr;
    float* ray_residual = nullptr;
    int* ray_counts = nullptr;      // 3 per ray: in-sphere, band, kept
    double* member = nullptr;       // 8 per member: M, V, m, K, sum_s, sum_r, status, 0
};

// One run's view of a batch for the Gauss-Newton launchers below: the stream, the sizes, the settings and every device array they address.
// The host fills it ONCE per run (dsp_gn.hip: fill_view, behind plan_run and size_run_buffers, so every pointer holds for the whole run) and
// applies there the rules whose answer is fixed for a run; a launcher's body is the one place that says which arrays its kernel reads.
struct GnView {
    hipStream_t s = nullptr;
    int B = 0, D = 0, maxR = 0, maxM = 0, n_slices = 1;
    GnParamsDev prm{};
    const ObjConst* oc = nullptr;
    ObjState* st = nullptr;
    const float *pts = nullptr, *rays = nullptr, *depth = nullptr;      // the inputs; depth: the observed foreground depths
    // start of a run (k_init_state): t_start holds object->camera estimates (the reference's argument) or -- init_flags bit 1 -- camera->object
    // matrices taken as they are (bit 0: pose-only); codes_start optional; depths_start: optional B x 64 override of the first depth samples
    const float *t_start = nullptr, *codes_start = nullptr, *scale = nullptr, *depths_start = nullptr;
    int init_flags = 0;
    const unsigned char* run_mask = nullptr;    // optional, B bytes: objects with a zero byte are left out of the run (DSP_STATUS_SKIP, state and result row untouched)
    unsigned* summary = nullptr;                // the run summary (SUM_*); k_init_state zeroes its head
    // per-ray bookkeeping and the sample list
    unsigned long long* raymask = nullptr;
    int *raycnt = nullptr, *rayoff = nullptr, *kcnt = nullptr, *koff = nullptr, *mcnt = nullptr, *pcnt = nullptr, *poff = nullptr, *plist = nullptr;
    unsigned char* ray_alive = nullptr;
    float *ray_res = nullptr, *ssdf = nullptr, *sdeds = nullptr;
    const float* saudit = nullptr;              // prepass audit: the fp32 value of every in-sphere sample
    float4* spts = nullptr;
    // jacobian rows: surface points, then kept render rows
    float4* jpts = nullptr;
    float2* jaux = nullptr;
    float* jgrad = nullptr;
    int *srow = nullptr, *jrow = nullptr;       // speculative band rows, null unless the plan is speculative: jgrad row of a sample / of kept render row i
    unsigned char* alive = nullptr;             // inlier flags of the surface points; null unless the batch is pose-only
    int4 *tiles_f = nullptr, *tiles_j = nullptr;    // tile lists of the decoder launches ...
    int* n_tiles = nullptr;                         // ... and their counts, slot LIST_*
    float* partials = nullptr;
    double* gsum = nullptr;
    float* trace = nullptr;                     // optional: TRACE_STRIDE floats per iteration and member
    const float *codew = nullptr, *b0 = nullptr, *blat = nullptr;   // the decoder's code columns: k_solve writes the next iteration's code bias ...
    float* cbias = nullptr;                                         // ... here
    const float* depth_sched = nullptr;         // optional [iteration][member][64]: row e + 1 overrides the depth samples k_solve derives in iteration e
    int sched_iters = 0;
    // multi-view groups (both set, or both null = every member is an object of its own): the members' Gram sums are pooled at the leader
    // (k_group_reduce), only leaders solve, and the new pose and code go back to the members (k_group_broadcast); gmk = 2 ints per member
    const GroupEnt* grp = nullptr;
    int* gmk = nullptr;
    // optional features, all null = off: the launches and kernel instantiations are those of a batch without the feature
    ObsWeightsDev obs;              // on: the weighted k_gram with k_weight_sums behind it, and the means divide by the weight sums
    PriorDev prior;                 // on: k_prior_terms in front of k_solve / k_posterior, Lambda and g include the prior's block
    StopRule stop{0.0, 0.0, 1};     // the convergence rule; off = a pose tolerance of 0, which can stop nothing
    StepDev step;                   // Levenberg-Marquardt step control (StepDev::last is set per launch)
    ReportDev report;
    const unsigned char* live = nullptr;    // mask of unknowns (dsp_batch_unknowns): 71 bytes per OBJECT (pose-only 6), 1 = live; on: the masked k_solve / k_posterior
    bool masked() const { return live != nullptr; }
    bool weighted() const { return obs.sums != nullptr; }
    bool has_prior() const { return prior.extra != nullptr; }
    bool stops() const { return stop.pose_tol > 0.0; }
    bool step_control() const { return step.sys != nullptr; }
    // the pass at the returned state: every member's status word is parked in park[] in front of it (frozen objects, DSP_STATUS_DONE, take part
    // as good ones).  Posterior (post_level 0 = off): one record of post_stride doubles per OBJECT (POSTERIOR_REC_L1, or _L2 with Lambda, g and
    // the state); post_weights: DSP_POSTERIOR_MEAN / _SUM
    int post_level = 0, post_weights = 0, post_stride = 0;
    int* park = nullptr;
    double* post_rec = nullptr;
    // results (k_finalize): one row per OBJECT, a group's written by its leader
    float* packed = nullptr;
    int guard_on = 0;               // the prepass guard is on: what it saw goes to the summary's guard words
};
enum { LIST_FWD = 0, LIST_JAC = 1, LIST_AUDIT = 3 };     // the lists k_build_tiles fills: tiles_f; tiles_j; tiles_j again (free while the audit runs)

// kernels_mlp / kernels_gn launchers
size_t mlp_lds_bytes(int mode);
void launch_code_bias(const float* codew, const float* b0, const float* blat, const float* codes, int code_stride, float* out, int n_obj, hipStream_t s);
hipError_t mlp_prepare_device();
hipError_t launch_mlp(int mode, const MlpArgs& args, int n_blocks, hipStream_t stream);   // mode: see mlp_kernel
hipError_t mlp_split_prepare_device();
hipError_t launch_mlp_split(int mode, const MlpArgs& args, int n_blocks, hipStream_t stream);   // 16-point tiles; mode 0 forward, 1 forward + mask export, 2 forward + backward (+ backward-only tiles)
hipError_t mlp_cluster_prepare_device();
hipError_t launch_mlp_cluster(const MlpArgs& args, int n_clusters, hipStream_t stream);   // 16-point tiles, four workgroups each; grid = 4 x n_clusters (n_clusters a multiple of 8), all resident
hipError_t mlp_lp_prepare_device();
hipError_t launch_mlp_lp(bool bf16, const LpArgs& args, int n_blocks, hipStream_t stream, int tile_pts = LP_TILE_PTS);   // 128- or 64-point tiles, forward only
hipError_t mlp_lpj_prepare_device();
hipError_t launch_mlp_lpj(int which, bool bf16, const LpjArgs& args, int n_blocks, hipStream_t stream);   // 128-point tiles; which: 0 forward + mask export, 1 backward from the masks
void launch_tail_tiles(const int4* tiles, int* n_tiles, int4* tiles16, int* n_tiles16, int n_cu, hipStream_t s);   // see k_tail_tiles

// ---- Gauss-Newton launchers: the view, plus what varies from call to call ----
void launch_init_state(const GnView& v);
// throughput forms of the per-ray bookkeeping (one thread block per 256 rays + a scan launch per list): front = sample_count + scan +
// sample_write (with observation weights a ray of weight 0 gets an empty mask), pass_list = pass_select + scan + pass_write, band_select =
// count + scan + write, render_tail = scan + sum_m + render_write (behind k_render_scan; every kept row's weight goes to ObsWeightsDev::jw)
void launch_front(const GnView& v);
void launch_surface(const GnView& v);
// mode 3 = mode 1 with the band samples (P) in place of the kept render rows (K); cnt_slot: counter the point count of a mode 0 / 2 list is added to
void launch_build_tiles(const GnView& v, int mode, int list, int add_v, int tile_pts, int cnt_slot, int apply_few);
// the band of object b is |sdf_lp| < cut_off + st[b].lp_delta.  guard_salt: samples OUTSIDE the band whose id hash (xor salt) selects them (1/8 of
// the ring just beyond the band, 1/512 farther out) are listed too, so that the fp32 kernel re-decodes them and prepass_guard compares (0 = no
// guard samples)
void launch_band_select(const GnView& v, unsigned guard_salt);
// wave-per-ray forms (latency path; one wave per ray, 16 rays per workgroup, whole chip) of front (+ surface), band and render tail: list
// segments from running counters (ObjState::V / ::P) instead of scans; kept rows stay in ray-major order.  See gn_kernels.hip.
void launch_front_wave(const GnView& v);
void launch_band_wave(const GnView& v, unsigned guard_salt);
void launch_render_tail_wave(const GnView& v);
void launch_prepass_audit(const GnView& v);
void launch_render_scan(const GnView& v);
void launch_render_tail(const GnView& v);
// one front-to-back forward pass: fixed depth-index range [j0, j1) (hint == nullptr), or per-ray adaptive ranges where
// j0 = margin added to the hint in pass 0 and j1 = step of the middle passes
struct PassSpec {
    int j0, j1, n_depth, pass, last;
    unsigned char* hint;   // per ray: depth index of the first solid sample in the previous GN iteration
    unsigned char* plo;    // per ray: end of the range decoded so far in this iteration
};
void launch_pass_list(const GnView& v, const PassSpec& ps);
void launch_pass_update(const GnView& v, int use_lp_delta, const PassSpec& ps);   // use_lp_delta: a ray stops at sdf <= -(cut_off + st[b].lp_delta)
void launch_gram(const GnView& v);
void launch_jrows(const GnView& v, int term, float* rows, int cap);
// one update: the reductions, the prior's terms, k_solve and -- groups -- the broadcast; last: the run's last iteration (StepDev::last)
void launch_solve(const GnView& v, int iter, int last);
// the members of every group take the leader's state: t_oc = T_oc * t_ref, the derived state (depths: optional B x 64 override), code, margin and
// -- cbias given -- the code-bias row; a failed leader's status goes to its members.  start: once behind k_init_state (no code-bias row,
// depths_start); otherwise the leader's LAST state in front of the pass at the returned state
void launch_group_broadcast(const GnView& v, bool start);
void launch_inlier_filter(const GnView& v);
// posterior pass (dsp_batch_posterior).  launch_posterior: launch_solve's reductions (no trace), then k_posterior, and the parked status words go back.
constexpr int POSTERIOR_REC_L1 = 168;
constexpr int POSTERIOR_REC_L2 = POSTERIOR_REC_L1 + 71 * 71 + 71 + (16 + CODE_LEN + MAX_DEPTH_SAMPLES) / 2;
void launch_posterior_park(const GnView& v);
void launch_posterior(const GnView& v);
// launch_report runs k_report_rays / k_report_points / k_report_members behind the front of the pass at the returned state; with observation
// weights sum_s / sum_r are the weighted sums and a ray of weight 0 reads as absent.
// report_ray_host: report_math::ray compiled for the host in the translation unit that has contraction off (dsp_debug_report_ray).
void launch_report(const GnView& v);
void report_ray_host(int n_depth, const float* depths, const float* sdf, float th, float depth_obs, int is_fg, float* out4, int* counts3);
// the prior's terms at the current state (launch_solve launches it itself, in front of k_solve); final_pass 1: e and chi2 at the returned
// state instead; 2 (launch_solve with step control): the terms, and chi2 at the current state in the record's chi2 slot
void launch_prior_terms(const GnView& v, int final_pass);
constexpr int DSP_RESULT_WIDTH_DEV = 82;   // == DSP_RESULT_WIDTH (dsp_gn.h): t_cam_obj 16 | code 64 | loss | status
void launch_finalize(const GnView& v);

hipError_t launch_debug_lie(int kind, const float* x_dev, float* out_dev, int n_depth, hipStream_t s);   // testing: exp_sim3 / exp_se3 / rotation prior as k_solve evaluates them

// ---- mesh extraction (mesh_kernels.hip) ---------------------------------------------------------
constexpr int MC_MAX_TRI = 5;
struct McTables {                        // marching-cubes case table, generated on the host (mc_build_tables)
    unsigned char n_tri[256];            // triangles of a cell whose corner-inside bits are the index
    unsigned char tri[256][16];          // 3 cube-edge ids per triangle, 0xff padded
    unsigned char edge_off[12][4];       // cube edge -> (offset of the owning grid point along axes 0, 1, 2; axis)
};
void mc_build_tables(McTables& t);
int mc_num_blocks(int n_pts);
hipError_t launch_grid_points(float4* pts, int n, float voxel_size, int regular, hipStream_t s);
hipError_t launch_mc_count(const float* vol, int n0, int n1, int n2, float level, const McTables* tab, int2* block_sums, long long* totals,
                           hipStream_t s);
hipError_t launch_mc_emit(const float* vol, int n0, int n1, int n2, float level, const McTables* tab, const int2* block_off, float spacing,
                          float origin, float* verts, int* vidmap, int* faces, hipStream_t s);
// batched extraction: n_obj volumes of n^3 back to back (object-major); block sums [n_obj][mc_num_blocks(n^3)] scanned as one list,
// obj_base[o] = first (vertex, face) of object o inside the chunk's output
hipError_t launch_mc_count_batched(const float* vol, int n, int n_obj, float level, const McTables* tab, int2* block_sums, long long* totals,
                                   int2* obj_base, hipStream_t s);
hipError_t launch_mc_emit_batched(const float* vol, int n, int n_obj, float level, const McTables* tab, const int2* block_off, float spacing,
                                  float origin, float* verts, int* vidmap, int* faces, hipStream_t s);
// surface band of n_obj prepass volumes (k_mesh_band): selected points compacted per object into the band lists (capacity n^3 each),
// cnt = [n_obj] selected + [n_obj] of them audited (zeroed by the caller), and the fp32 kernel's tile list over them (tiles: capacity
// n_obj x ceil(n^3 / MESH_TILE_PTS); *n_tiles on the device).  guard: per object {delta, trips, max err}, delta read here
constexpr int MESH_TILE_PTS = TILE_PTS;
hipError_t launch_mesh_band(const float* lp, const float4* grid, int n, int n_obj, const unsigned* guard, float4* band_pts, float* band_val,
                            long long* band_idx, int* cnt, int* tile0, int* n_tiles, int4* tiles, hipStream_t s);
hipError_t launch_mesh_scatter(const float* band_val, const long long* band_idx, const int* cnt, int n, int n_obj, float* vol, hipStream_t s);

// ---- surface projection (surface_kernels.hip; the arithmetic: surface_math.h) --------------------
// pack: n packed float3 points -> the decoder's float4 list (unpack = 0) or the list -> out3 (unpack = 1).  step: point i moves by the tail
// of row i.  attributes: one workgroup per tile {first point, count, object, row offset} of the decoder's list; var = [object][CODE_LEN]
// floats or null (sigma is then not written); outputs indexed by point, any may be null.  A point that is not finite is NaN in every output.
hipError_t launch_surface_pack(const float* p3, float4* p4, float* out3, int n, int unpack, hipStream_t s);
hipError_t launch_surface_step(float4* pts, const float* rows, int n, float max_step, hipStream_t s);
hipError_t launch_surface_attributes(const int4* tiles, int n_tiles, const float4* pts, const float* rows, const float* var, float* normals, float* grad_norm,
                                     float* sdf, float* sigma, hipStream_t s);
// surface_math.h compiled for the host in the translation unit that has contraction off (dsp_debug_surface_step / _attributes)
void surface_step_host(int64_t n, const float* pts, const float* sdf, const float* grad_xyz, float max_step, float* pts_out);
void surface_attributes_host(int64_t n, const float* rows68, const float* var64, float* normals, float* grad_norm, float* sdf, float* sigma);

// ---- map query (query_kernels.hip; the arithmetic: query_math.h) ---------------------------------
// tab: the objects of the call, query_math::OBJ_STRIDE floats each {[R_ow | t_ow] 12, s, s_sel, 0, 0}: s scales the sphere bound, s_sel the
// decoder's sdf (NaN for an object that must never win).  A pass = points [p0, p0 + n) of pts3 (packed float3, world frame), n_waves = ceil(n / 64).
// count: wave_cnt[n_obj][n_waves] <- contained points per (object, wave), then its exclusive scan over the waves in place and cnt[obj] = the
//   object's candidates; bound[p0 + i] and best[p0 + i] (the all-ones key) for every point of the pass.
// fill: for the chunk's objects [o0, o0 + nc), candidate j of object o0 + k gets chunk row base[k] + j; rows inside [0, n_rows) are written:
//   p_o to pts4 (the decoder's list), {point, object} to row_meta.
// reduce: best[point] = min(., key) over the chunk's rows, sdf from out[row] (forward form) or out[row][67] (jacobian_rows); with normal != null
//   the row that holds its point's best key then writes its world normal.
// finish: best -> obj, dist; normal (optional) zeroed where there is no winner.
hipError_t launch_query_count(const float* pts3, int64_t p0, int n, const float* tab, int n_obj, int n_waves, int* wave_cnt, int* cnt, float* bound,
                              unsigned long long* best, hipStream_t s);
hipError_t launch_query_fill(const float* pts3, int64_t p0, int n, const float* tab, int o0, int nc, const int* base, int n_waves, const int* wave_base,
                             int n_rows, float4* pts4, int2* row_meta, hipStream_t s);
hipError_t launch_query_reduce(const float* out, bool jacobian_rows, const int2* row_meta, int n_rows, const float* tab, int n_obj, int64_t n_pts,
                               unsigned long long* best, float* normal, hipStream_t s);
hipError_t launch_query_finish(const unsigned long long* best, int64_t n, int* obj, float* dist, float* normal, hipStream_t s);
// query_math.h compiled for the host in the translation unit that has contraction off (dsp_map_query's pose inversion, dsp_debug_query_*)
bool query_invert_host(const float* t16, float* rt12, float* scale);
void query_candidates_host(int64_t n_obj, const float* rt, const float* scale, int64_t n_pts, const float* pts, float* p_obj, unsigned char* inside,
                           float* bound);
void query_select_host(int64_t n_rows, const float* sdf, const float* scale_of_row, const int32_t* obj_of_row, const int32_t* pt_of_row, int64_t n_pts,
                       int32_t* obj, float* dist);

// ---- ray casting against the map (raycast_kernels.hip; the arithmetic: raycast_math.h) ------------
// The device arrays of one call: n_rays world rays (packed float3 origins and directions) and the object table in; per ray the hit key
// (orderable(t_hit) << 32 | obj), the smallest parameter of its exhausted pairs (orderable bits, all ones = none) and the outputs.
// dstats = {decoder rows, tiles, rounds that decoded a row, exhausted pairs} of the march, kept on the device.
struct RaycastDev {
    const float *org, *dir, *tab;
    int n_rays, n_obj, n_waves;         // n_waves = ceil(n_rays / 64)
    raycast_math::Params prm;
    unsigned long long* best;
    unsigned* exh;
    int* obj;
    float *t, *dist;
    int* status;
    float* normal;                      // null: no normals
    unsigned long long* dstats;
};
// One pass: the pairs [lo, hi) of each of the objects [o0, o0 + nc), held in n_slots slots (a multiple of 64; every object's pairs start at
// a multiple of 64).  The host uploads, once per pass: pobj[k] = {slot offset added to the pair index, lo, hi, 0}; ob[k] = {first wave of
// slots, waves, object index, 0}; wtab[wave] = {object of the pass, the object's first wave}.  Everything else is written on the device:
// the pair state (pr_*), and per round live_cnt / wave_row per wave of slots, oinfo per object, ctrl = {tiles, live rows}, the compacted
// samples pts4 with row_slot, and the tile list.
struct RaycastPass {
    int o0, nc, n_slots;
    const int4* pobj;
    const int4* ob;
    const int2* wtab;
    int2* pr_meta;                      // {ray, object}
    int* pr_state;                      // 0 live, 1 hit, 2 ended as a miss, anything else padding
    float *pr_t, *pr_t1, *pr_dist;
    float4 *pr_oo, *pr_do;
    int *live_cnt, *wave_row;
    int4* oinfo;
    int* ctrl;
    float4* pts4;
    int* row_slot;
    int4* tiles;
};
// count: wave_cnt[n_obj][n_waves] <- existing pairs per (object, wave) and its scan, cnt[obj]; best / exh / dist initialised for every ray.
// fill: the pass's pair state.  round_front: retirement and live counts, the scan (ONE block), the compacted samples and the tile list.
// step: the step rule on the decoder's values sdf[row].  end: the pass's exhausted pairs and the winners' dist.  finish: obj, t, status.
// wincount / winfill / normal: the winners grouped by object in ascending ray order, their hit samples, their world normals.
hipError_t launch_raycast_count(const RaycastDev& d, int* wave_cnt, int* cnt, hipStream_t s);
hipError_t launch_raycast_fill(const RaycastDev& d, const RaycastPass& p, const int* wave_base, hipStream_t s);
hipError_t launch_raycast_round_front(const RaycastDev& d, const RaycastPass& p, hipStream_t s);
hipError_t launch_raycast_step(const RaycastDev& d, const RaycastPass& p, const float* sdf, hipStream_t s);
hipError_t launch_raycast_end(const RaycastDev& d, const RaycastPass& p, hipStream_t s);
hipError_t launch_raycast_finish(const RaycastDev& d, hipStream_t s);
hipError_t launch_raycast_wincount(const RaycastDev& d, int* wave_cnt, int* cnt, hipStream_t s);
hipError_t launch_raycast_winfill(const RaycastDev& d, int o0, int nc, const int* base, const int* wave_base, int n_rows, float4* pts4, int2* row_meta,
                                  hipStream_t s);
hipError_t launch_raycast_normal(const RaycastDev& d, const float* rows, const int2* row_meta, int n_rows, hipStream_t s);
// raycast_math.h compiled for the host in the translation unit that has contraction off (dsp_debug_raycast_*)
void raycast_segments_host(int64_t n_obj, const float* rt, const float* scale, int64_t n_rays, const float* org, const float* dir, float t_min, float t_max,
                           unsigned char* is_void, unsigned char* exists, float* t0, float* t1, float* o_o, float* d_o);
void raycast_step_host(int64_t n, const float* t, const float* t1, const float* sdf, const float* s, float eps, float relax, int32_t* decision,
                       float* dist, float* t_next);
const char* raycast_check_host(float t_min, float t_max, float eps, float relax, int max_steps);

// ---- map alignment (align_kernels.hip; the arithmetic: align_math.h) ----------------------------
// hyp: ALIGN_HYP_STRIDE floats per hypothesis {[R | t] of the sensor-to-world pose in fp32, 12; live (1 / 0); 0, 0, 0}.  Rows are
// r = h n_pts + i.  transform: rows [r0, r0 + n) of pts_w <- to_object(rt_h, pts_s[i]), NaN for an ended hypothesis.  winner: behind a
// chunk's launch_query_reduce (jacobian rows), the row that holds its point's best key writes the world gradient of d.  gram: the
// align_math::NSUM sums of every live hypothesis through the written tree: slab[n_hyp][align_gram_blocks(n_pts)][NSUM] -> sums[n_hyp][NSUM].
constexpr int ALIGN_HYP_STRIDE = 16;
hipError_t launch_align_transform(const float* pts_s, int64_t n_pts, const float* hyp, int64_t r0, int64_t n, float* pts_w, hipStream_t s);
hipError_t launch_align_winner(const float* rows, const int2* row_meta, int n_rows, const float* tab, int n_obj, int64_t n_pts,
                               const unsigned long long* best, float* grad_w, hipStream_t s);
hipError_t launch_align_gram(const float* pts_w, const int* obj, const float* dist, const float* grad_w, const float* weights, int64_t n_pts, int n_hyp,
                             const float* hyp, double huber, double max_dist, double* slab, double* sums, hipStream_t s);
int64_t align_gram_blocks(int64_t n_pts);
// Ray alignment (the arithmetic: align_rays_math.h).  build: rows [0, n) of pts_w / org_w / dir_w <- the world end point, origin and
// direction of observation i under hypothesis h (org_s null: the sensor origin), NaN for an ended hypothesis.  gradient: behind a chunk of
// the winners' jacobian rows (row_meta = {row of the cast, object}), the world gradient of d.  residual: the cast's answers -> obj_row, d_row,
// which launch_align_gram reads as obj and dist.
hipError_t launch_align_rays_build(const float* pts_s, const float* org_s, int64_t n_rays, const float* hyp, int64_t n, float* pts_w, float* org_w,
                                   float* dir_w, hipStream_t s);
hipError_t launch_align_rays_gradient(const float* rows, const int2* row_meta, int n_rows, const float* tab, int n_obj, int64_t n_rays, float* grad_w,
                                      hipStream_t s);
hipError_t launch_align_rays_residual(const float* org_w, const float* dir_w, const int* obj, const float* t_hit, const float* dist_hit, const int* status,
                                      const float* grad_w, int64_t n, double max_gap, int* obj_row, float* d_row, hipStream_t s);
// align_math.h compiled for the host in the translation unit that has contraction off (dsp_map_align's step, dsp_debug_align_*)
bool align_check_pose_host(const double* t16, float* rt12);
void align_rows_host(int64_t n, const float* pts_w, const int32_t* obj, const float* dist, const float* grad_w, const float* weights, double huber,
                     double max_dist, double* sums);
void align_ray_rows_host(int64_t n, const float* org_w, const float* pts_w, const int32_t* obj, const float* t_hit, const float* dist_hit,
                         const int32_t* status, const float* grad_w, const float* weights, double huber, double max_dist, double max_gap,
                         int32_t* obj_row, float* d_row, double* sums);
const char* align_rays_check_gap_host(double max_gap, double max_dist);
double align_cost_host(const double* sums, double huber, double max_dist);
bool align_solve_host(const double* H36, const double* b6, double damp, double lambda, double* xi6);
void align_apply_step_host(const double* xi6, const double* t_in, double* t_out);

// ---- object refinement (align_objects_kernels.hip; the arithmetic: align_objects_math.h) ---------
// Behind a cast's winner count (launch_raycast_wincount: wave_base = the scan per (object, wave), totals on the host).  list: win_ray[off[k] + j]
// <- the j-th winner of object k in ascending ray order; off = the exclusive scan of the totals (n_obj ints), n_list their sum.  gram: blocks[q] =
// {object, first list position, positions <= align_math::BLOCK, 0} -> slab[q][NSUM]; then sums[k][NSUM] <- the slabs [first[k], first[k + 1]) in
// ascending order, zero where there is none (first: n_obj + 1 ints).  obj_row / d_row / grad_w are per ray (launch_align_rays_residual / _gradient).
hipError_t launch_align_objects_list(const int* obj, int n_rays, int n_obj, int n_waves, const int* wave_base, const int* off, int n_list, int* win_ray,
                                     hipStream_t s);
hipError_t launch_align_objects_gram(const int4* blocks, int n_blocks, const int* first, int n_obj, const int* win_ray, int n_list, int n_rays,
                                     const float* pts_w, const int* obj_row, const float* d_row, const float* grad_w, const float* weights, double huber,
                                     double max_dist, double* slab, double* sums, hipStream_t s);
// align_objects_math.h compiled for the host in the translation unit that has contraction off (dsp_map_align_objects, dsp_debug_align_objects_*)
void align_objects_compose_host(const double* c16, const float* t16, float* out16);
void align_objects_directions_host(int64_t n, const float* org_w, const float* pts_w, float* dir_w);
void align_objects_rows_host(int64_t n, const float* pts_w, const int32_t* winner, const int32_t* obj_row, const float* d_row, const float* grad_w,
                             const float* weights, int64_t n_obj, double huber, double max_dist, double* sums);

// ---- shape refinement (align_shapes_kernels.hip; the arithmetic: align_shapes_math.h) ------------
// rows: behind a chunk of the winners' jacobian rows (next to launch_align_rays_gradient), gcode[ray][64] <- the row's code derivatives times
// the winner's scale.  gram: the lists and the block table of launch_align_objects_list / _gram with blocks of align_shapes_math::BLOCK
// positions -> slab[q][align_shapes_math::NSUM], then sums[k][NSUM] <- the slabs [first[k], first[k + 1]) in ascending order.
hipError_t launch_align_shapes_rows(const float* rows, const int2* row_meta, int n_rows, const float* tab, int n_obj, int64_t n_rays, float* gcode,
                                    hipStream_t s);
hipError_t launch_align_shapes_gram(const int4* blocks, int n_blocks, const int* first, int n_obj, const int* win_ray, int n_list, int n_rays,
                                    const float* pts_w, const int* obj_row, const float* d_row, const float* grad_w, const float* gcode,
                                    const float* weights, double huber, double max_dist, double* slab, double* sums, hipStream_t s);
// align_shapes_math.h compiled for the host in the translation unit that has contraction off (dsp_map_align_shapes, dsp_debug_align_shapes_*)
void align_shapes_rows_host(int64_t n, const float* pts_w, const int32_t* winner, const int32_t* obj_row, const float* d_row, const float* grad_w,
                            const float* gcode, const float* weights, int64_t n_obj, double huber, double max_dist, double* sums);
double align_shapes_mean_cost_host(const double* sums, double huber, double max_dist);
double align_shapes_cost_host(double mean, const double* z, const double* z0, int code_len, double code_reg, double code_anchor);
bool align_shapes_solve_host(const double* H, const double* b, double W, const double* z, const double* z0, int code_len, int unknowns, double code_reg,
                             double code_anchor, double damp, double lambda, double* dx);
void align_shapes_apply_step_host(const double* dx, int unknowns, int code_len, const double* c_in, const double* z_in, double* c_out, double* z_out);

}  // namespace dsp
