// A batch on the host: struct dsp_batch and its tokens, for the files that reach into a batch (dsp_gn.hip builds and runs it, gather.hip reads its results).
#pragma once
#include "batch_tokens.h"
#include "host_common.h"
#include "launch_plan.h"

#include <atomic>
#include <cstdint>
#include <mutex>
#include <vector>

using launch_plan::LaunchPlan;
using launch_plan::PlanInputs;
using launch_plan::make_launch_plan;
static_assert(launch_plan::TILE == TILE_PTS && launch_plan::SPLIT_TILE == SPLIT_TILE_PTS && launch_plan::LP_TILE == LP_TILE_PTS && launch_plan::LP_TILE_SMALL == LP_TILE_PTS_SMALL, "tile sizes");
struct dsp_batch {
    dsp_handle* h = nullptr;
    std::atomic<int> pins{0};  // calls in flight on THIS batch (BatchRef): dsp_batch_destroy from another thread waits for them
    dsp_gn_params prm;
    int B = 0, D = 0, maxR = 0, maxM = 0, n_slices = 1;
    // multi-view batches (dsp_batch_create_multiview): the B members are the VIEWS, grouped by object (GroupEnt); results, run masks and
    // failures are per object.  Every other batch: n_obj == B, no table.
    int n_obj = 0;
    std::vector<GroupEnt> grp_host;
    DevBuf<GroupEnt> grp;
    DevBuf<int> gmk;          // per member, read at the leaders: the group's M and K of the current iteration (k_group_reduce)
    bool grouped() const { return !grp_host.empty(); }
    bool pose_only = false, trace_on = false;
    int64_t sum_pts = 0, sum_rays = 0, sum_depth = 0, cap_s = 0, cap_j = 0;
    std::vector<ObjConst> oc_host;
    DevBuf<ObjConst> oc;
    DevBuf<ObjState> st;
    DevBuf<float> pts, rays, depth, t_in, codes_in, scale_in;
    bool have_codes = false;
    DevBuf<unsigned long long> raymask;
    DevBuf<int> raycnt, rayoff, kcnt, koff, mcnt, pcnt, poff, plist;
    DevBuf<unsigned char> ray_alive, ray_hint, ray_plo;
    DevBuf<unsigned short> maskbuf;   // relu masks of band samples, 512 B per sample (written by the forward passes)
    // settings: what launch_plan.h decides from (PlanInputs); the tri-states are pinned through dsp_batch_set_debug (DSP_DBG_*)
    int split_rows = -1;      // jacobian launch in the latency form (16-point tiles, rows split over waves): -1 auto, 0 off, 1 on (DSP_DBG_SPLIT_ROWS)
    int mask_reuse = -1;      // render rows backward-only from exported relu masks: -1 auto, 0 off, 1 on (DSP_DBG_MASK_REUSE)
    int n_ray_passes = 0;     // front-to-back forward passes per iteration (0 = pick from the batch size)
    std::vector<int> pass_bounds;   // optional explicit depth-index boundaries (n_passes + 1 entries, 0 .. D)
    int hint_margin = 2, hint_step = 8;   // adaptive passes: pass 0 = [0, hint + margin), middle pass = next `step` indices
    int speculative = -1;         // band samples straight into the jacobian launch (latency path): -1 auto, 0 off, 1 on
    DevBuf<int> srow, jrow;       // speculative band rows: jgrad row of a sample / of a kept render row
    int fused_bookkeeping = -1;   // per-ray bookkeeping: -1 auto (wave form for latency-sized batches), 0 throughput form, 2 wave-per-ray form
    int tail_split = -1;          // last partial round of the fp32 forward launch as 16-point latency-form tiles: -1 auto, 0 off, 1 on
    DevBuf<int4> tiles16;
    int compute = 0;          // DSP_COMPUTE_F32 (default) / _F16 / _BF16: the opt-in low-precision compute mode (dsp_batch_set_compute)
    int lp_small = -1;        // ... on detection-sized batches too (DSP_DBG_LP_SMALL_BATCHES; -1 / 0: they keep the fp32 latency path, which is faster there)
    DevBuf<uint4> lpj_masks;  // ... its relu masks: 64 KiB per 128-point jacobian tile
    int prepass = -1;         // low-precision classification pass in front of the fp32 forward decoder: -1 auto, 0 off, 1 f16, 2 bf16
    int lp_tile = -1;         // points per prepass tile: -1 auto, LP_TILE_PTS (128) or LP_TILE_PTS_SMALL (64) (DSP_DBG_PREPASS_TILE)
    float prepass_delta = -1.f;   // margin added to cut_off on both sides (< 0: the dtype's default)
    bool prepass_audit = false;   // also decode every sample in fp32 and compare (tests / calibration)
    int prepass_guard = 1;        // always-on guard (prepass_guard, mlp_common.h): 1 on, 0 off (tests: what an unguarded run returns)
    unsigned guard_salt = 0;      // which of the classified samples the guard re-decodes: advances with every launch
    // optional start state (dsp_batch_set_start_state): camera->object matrices and codes the next runs start from, as they are
    DevBuf<float> start_t_oc, start_depths;
    bool have_start_t_oc = false, have_start_depths = false;
    DevBuf<float> depth_sched;    // forensics (dsp_batch_set_depth_schedule): [iteration][object][64] depth samples, sched_iters rows
    int sched_iters = 0;
    DevBuf<float> saudit;
    DevBuf<unsigned> summary;     // the run summary (layout: SUM_*, dsp_internal.h), the head of the run's ONE read-back (ReadBack below)
    size_t summary_words() const { return sum_iters(B) + (size_t)B; }
    double* counters() const { return reinterpret_cast<double*>(summary.p + SUM_COUNTERS); }
    unsigned* audit_out() const { return summary.p + SUM_AUDIT; }
    // convergence rule (dsp_batch_convergence); (0, 0, 1) = off: the run's launches are those of a batch without it
    float stop_pose_tol = 0.f, stop_code_tol = 0.f;
    int stop_min_iterations = 1;
    bool stop_on() const { return stop_pose_tol > 0.f && (pose_only || stop_code_tol > 0.f); }     // a tolerance of 0 can stop nothing
    std::vector<int32_t> iters_used;  // per object: updates applied in the run that produced its row (dsp_batch_iterations_used)
    // posterior (dsp_batch_posterior): level 0 = off -- the run's launches are those of a batch without it.  One record per OBJECT
    // (k_posterior: POSTERIOR_REC_L1 doubles, level 2 POSTERIOR_REC_L2), read back with the results; post_host is the last run's.
    int post_level = 0, post_weights = DSP_POSTERIOR_MEAN;
    DevBuf<int> post_park;
    DevBuf<double> post_rec;
    int post_rec_level = 0;           // the level post_rec was sized for
    std::vector<double> post_host;
    int post_host_level = 0;          // the level of the LAST run, whose records post_host holds (0: it ran with the posterior off, or nothing ran yet)
    size_t post_stride(int level) const { return level >= 2 ? POSTERIOR_REC_L2 : POSTERIOR_REC_L1; }
    // Gaussian prior on pose and code (dsp_batch_prior), per OBJECT; off (initial) = the run's launches are those of a batch without it.
    // prior_res: e and chi2 at the returned state (k_prior_terms' final pass), read back with the results; prior_host is the last run's.
    bool prior_on = false;
    DevBuf<float> prior_t0, prior_z0;
    DevBuf<double> prior_L, prior_extra, prior_res;
    DevBuf<unsigned char> prior_flag;
    std::vector<double> prior_host;
    bool prior_host_valid = false;    // the LAST run was made with a prior
    int prior_n() const { return pose_only ? 6 : 71; }
    // Levenberg-Marquardt step control (dsp_batch_step_control; step_rule.h), joint batches only; all zero (initial) = off: the run's
    // launches are those of a batch without it.  The saved systems and the rule's state come from the handle's pool the first time the
    // feature is enabled; the log ([iteration][object]) rides in the run's read-back, step_host is the last run's.
    step_rule::Params step_prm{0.0, 0.0, 0.0, 0.0, 0.0};
    bool step_on() const { return !step_rule::is_off(step_prm); }
    DevBuf<double> step_sys;
    DevBuf<StepObj> step_obj;
    DevBuf<StepLogEnt> step_log;
    std::vector<StepLogEnt> step_host;
    int step_host_iters = 0;          // iterations of the LAST run if it was made with step control, else 0
    // observation report (dsp_batch_report): off (initial) = the run's launches are those of a batch without it.  The arrays come from the
    // handle's pool the first time the report is enabled and stay on the device until dsp_batch_report_fetch copies them (no read-back in a run).
    bool report_on = false;
    bool report_valid = false;        // the LAST run was made with the report on
    DevBuf<float> rep_pt_sdf, rep_ray_depth, rep_ray_hit, rep_ray_res;
    DevBuf<unsigned char> rep_pt_flags;
    DevBuf<int> rep_ray_counts;
    DevBuf<double> rep_member;
    // per-observation weights (dsp_batch_observation_weights): off (initial) = the run's launches are those of a batch without them.  The
    // arrays come from the handle's pool the first time weights are set and stay set for every following run (partial re-runs included).
    bool obs_on = false;
    DevBuf<float> obs_pt_w, obs_ray_w, obs_jw;
    DevBuf<double> obs_sums;          // [B][2] the members' sums, then [B][2] the groups' pooled sums
    // mask of unknowns (dsp_batch_unknowns), per OBJECT: off (initial, and for an all-live mask) = the run's launches are those of a batch
    // without one.  The array (71 bytes per object, pose-only 6) comes from the handle's pool the first time a mask is set and stays set for
    // every following run (partial re-runs included: they address the same members).
    bool unk_on = false;
    DevBuf<unsigned char> unk_live;
    int unk_width() const { return pose_only ? 6 : 71; }
    DevBuf<unsigned char> run_mask;   // partial re-run after a guard trip: 1 = object takes part
    std::vector<float> h_packed;      // host copy of out_packed of the last run (dsp_batch_results unpacks it: no device access)
    int kernel_timing = -1;           // HIP events around every decoder launch: -1 auto (throughput-sized batches), 0 off, 1 on
    int direct_tiles = -1;            // one-object batches: the decoder kernels derive their tile lists themselves (-1 / 1 on, 0 off)
    int mixed_reuse = -1;             // latency path: kept render rows backward-only inside the jacobian launch (DSP_DBG_MIXED_REUSE): -1 auto, 0 off, 1 on
    int cluster_tiles = -1;           // jacobian launch of a detection-sized list as 4-workgroup clusters (mlp_cluster_kernel): -1 auto, 0 off, 1 on
    bool cluster_failed = false;      // the last run's cluster kernel gave up on a spin: from that launch on the latency-form kernel took the lists (on the device)
    int cluster_fault = 0;            // fault injection (tests, DSP_DBG_CLUSTER_FAULT): the next run's cluster launches lose a workgroup's counters
    int cluster_fallbacks = 0;        // runs of this batch in which the cluster kernel reported a lost hand-off and the latency form took over
    DevBuf<float> ray_res, ssdf, sdeds, jgrad, partials, trace, out_packed, rows;
    DevBuf<float4> spts, jpts;
    DevBuf<float2> jaux;
    DevBuf<unsigned char> alive;
    DevBuf<int4> tiles_f, tiles_j;
    DevBuf<int> n_tiles;
    DevBuf<double> gsum;
    DevBuf<float> cbias;
    std::vector<hipEvent_t> ev;   // [run start, run end] + (kernel timing on) pairs around every decoder launch
    std::vector<int> ev_kind;
    int n_launch[3] = {0, 0, 0};  // decoder launches of the run by kind (0 fp32 forward, 1 jacobian, 2 prepass): counted on the host
    dsp_stats stats;
    int iters_run = 0;
    LaunchPlan plan{}; std::vector<PassSpec> passes;     // the forms the current / last run uses and its ray passes per iteration (plan_run)
    GnView view;                  // ... and what its GN launchers address (fill_view)
    // The current / last run's ONE read-back into the handle's pinned block, in front of its ONE synchronisation: element counts and byte offsets of
    // [summary words | result rows (fp32) | posterior records | prior records (fp64) | step log]; a section the run does not have is empty.
    struct ReadBack {
        const char* base;                 // the pinned block (valid until the handle's next run)
        size_t n_sum, n_res, n_post, n_prior, n_step;
        size_t res_off() const { return n_sum * 4; }
        size_t post_off() const { return (res_off() + n_res * 4 + 7) / 8 * 8; }      // the fp64 sections start on 8 bytes
        size_t prior_off() const { return post_off() + n_post * 8; }
        size_t step_off() const { return prior_off() + n_prior * 8; }
        size_t bytes() const { return step_off() + n_step * sizeof(StepLogEnt); }
        template <class T> const T* at(size_t off) const { return reinterpret_cast<const T*>(base + off); }
        const unsigned* summary(size_t word) const { return at<unsigned>(word * 4); }
    } rb{};
    std::vector<unsigned char> guard_tripped;     // per member, the last guarded run's: the prepass guard tripped on it (a group: on any of its views)
    ~dsp_batch() {                // events go back to the handle's pool (the handle outlives its batches)
        if (h) { std::lock_guard<std::mutex> l(h->pool.mu); for (auto e : ev) h->event_pool.push_back(e); }
        else for (auto e : ev) (void)hipEventDestroy(e);
    }
};

// batch tokens: what dsp_batch_create hands out, and how the two destroy calls retire them (batch_tokens.h)
using Tokens = batch_tokens::Table<dsp_batch>;
using BatchRef = Tokens::BatchRef;
