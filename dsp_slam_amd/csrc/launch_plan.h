// The launch plan: which of the bit-identical forms of each computation one run of a batch uses.  Host-only (no HIP include): plain
// integer and floating-point arithmetic on the values in PlanInputs, decided ONCE per run (batch_run_once / each attempt of run_terms,
// dsp_gn.hip) and read everywhere else as b->plan.x.  The inputs only change between runs: setters, the handle's cluster cool-down
// (note_cluster_outcome), `prepass` for the guard's re-run.  tests/test_launch_plan.py replays a recorded table of (inputs, plan) rows.
#pragma once
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>

namespace launch_plan {
constexpr int TILE = 64, SPLIT_TILE = 16, LP_TILE = 128, LP_TILE_SMALL = 64;   // = TILE_PTS, SPLIT_TILE_PTS, LP_TILE_PTS(_SMALL) of dsp_internal.h (static_assert in batch.h)

// tri-state settings: -1 automatic, 0 off, 1 on (fused_bookkeeping: 2 = the wave form), pinned through dsp_batch_set_debug (DSP_DBG_*)
struct PlanInputs {
    int pose_only, B, D;                    // the batch ...
    int64_t sum_pts, sum_rays, cap_s;       // surface points, rays, ray-sample slots (rays x D, rounded up to 64 per object)
    int split_rows, mask_reuse, mixed_reuse, speculative, fused_bookkeeping, tail_split, cluster_tiles, direct_tiles, kernel_timing;
    int compute, lp_small;                  // DSP_COMPUTE_*; the low-precision compute mode on detection-sized batches too (1)
    int prepass, lp_tile, prepass_guard;    // -1 / DSP_PREPASS_*; -1 / 128 / 64; 0 / 1
    int n_ray_passes, n_pass_bounds, n_bound_ranges;   // 0 = automatic; entries of the explicit depth-index bounds (0 = none) and how many of their ranges are not empty
    int n_cu, n_clusters, lp_ok, lpj_ok, cl_cooldown;   // ... and its handle (lpj_ok implies lp_ok: dsp_create)
};

struct LaunchPlan {          // all int: the test hook hands the struct out as a row of integers
    int kernel_timing;       // HIP events around every decoder launch
    int lp_compute;          // 0, or DSP_COMPUTE_F16 / _BF16: the low-precision compute mode is in force
    int reuse_throughput;    // throughput form of mask reuse: the kept render rows backward-only in a launch of 64-point tiles of their own
    int bookkeeping_form;    // 0 = one thread block per 256 rays + scan launches, 2 = one wave per ray
    int prepass_mode;        // 0 off, 1 f16, 2 bf16: the kernel the forward ray samples go through first (compute mode: the only one)
    int guard_on;            // fp32 launches that overwrite prepass values compare them on the way; a trip re-runs the object with the prepass off
    int speculative_band;    // the samples the prepass could not classify go straight into the jacobian launch
    int split_rows;          // jacobian launch in the latency form (16-point tiles, each layer's rows split over the four waves)
    int mixed_reuse, mask_reuse;       // mixed form of mask reuse; either form (dsp_stats: n_jac_points counts the surface points only, n_render_rows the rest)
    int cluster, cluster_max_tiles;    // the cluster-form kernel in front of the latency-form jacobian kernel, for lists of up to this many tiles
    int split_fwd, tail_split;         // fp32 forward launches in the latency form / their last partial round of 64-point tiles as 16-point tiles
    int lp_tile_pts, fwd_tile_pts, jac_tile_pts;    // points per tile: prepass / fp32 forward / jacobian list
    int direct_tiles;        // one-object batch in the wave form: the decoder kernels derive their tile lists themselves
    int fixed_passes, hint_passes;     // ray passes per iteration: fixed depth-index ranges, or (fixed_passes == 0) per-ray ranges steered by the last iteration's hints
    int whole, explicit_bounds;        // the one pass covers every in-sphere sample in place (no selection list); the fixed ranges are the caller's, not uniform
};

inline LaunchPlan make_launch_plan(const PlanInputs& in) {
    LaunchPlan p{};
    assert(in.lp_ok || !in.lpj_ok);
    const bool render = !in.pose_only;
    const double n_cu = in.n_cu, sum_pts = (double)in.sum_pts, cap_s = (double)in.cap_s;
    auto tri = [](int setting, bool automatic) { return setting >= 0 ? setting != 0 : automatic; };
    // HIP events around every decoder launch (dsp_stats.ms_mlp_*): what the bench's roofline is computed from.  An event record between two
    // kernels is a marker packet of its own on the queue, so latency-sized batches (SLAM's per-detection calls) skip them unless asked.
    p.kernel_timing = tri(in.kernel_timing, in.B > 16);
    // Low-precision compute mode: ray samples by the 16-bit forward kernel ONLY (no fp32 re-decode of the band), jacobian rows by the 16-bit
    // forward + backward kernels (mlp_lpj_kernel.hip), 128-point tiles throughout; every fp32-path form below is off.  Detection-sized batches
    // (surface points + band samples fit one round of 16-point tiles) keep the fp32 latency path even when the mode is set: one KITTI-size
    // detection 2.89 ms on it (cluster jacobian, exact) against 3.40 ms on 128-point 16-bit tiles that fill 6 of 256 CUs; one cfg2-size object: 14.0 -> 6.0 ms in the mode (profiles/r06_latency_ab.md).
    const bool one_round16 = (sum_pts + 0.16 * cap_s) / SPLIT_TILE <= 1.0 * n_cu;
    const bool detection_sized = in.B <= 16 && one_round16;
    p.lp_compute = (render && in.lpj_ok && in.compute && (in.lp_small == 1 || !detection_sized)) ? in.compute : 0;
    const bool fp32 = !p.lp_compute, fp32_render = render && fp32;
    // Render rows backward-only from the relu masks the forward launches exported, THROUGHPUT form (a launch of 64-point tiles of its own
    // behind the surface points' forward + backward launch).  Not for latency-sized batches: with one or two objects every jacobian tile fits
    // a single round over the CUs, so a second launch adds a round instead of saving a forward sweep (tools/probes/gpu_reuse_probe.py, cfg2
    // objects: 1 object 38.1 ms on vs 32.3 off; 4 objects 42.1 obj/s vs 40.1; 8: 49.6 vs 45.5; 32: 49.4 vs 44.9)
    p.reuse_throughput = fp32_render && tri(in.mask_reuse, in.sum_pts / TILE >= in.n_cu / 4);
    const bool latency_ok = fp32 && !p.reuse_throughput;      // (the throughput form's backward-only launch runs 64-point tiles)
    // Small batches run the per-ray bookkeeping (sampling + compaction, band selection, row compaction) in one launch per stage: form 2 = one
    // WAVE per ray over the whole chip (k_front_wave / k_band_wave / k_render_tail_wave), form 0 = one thread block per 256 rays + scan launches.
    // Same device arithmetic, same sets, same bits.  Real-KITTI-size detection, per iteration: 11 launches / ~60 us in form 0; large batches keep
    // form 0 (their scans are amortised over many objects and the lists stay in ray order, which the 128-point prepass tiles like)
    p.bookkeeping_form = !render ? 0 : in.fused_bookkeeping >= 0 ? in.fused_bookkeeping : (in.B <= 16 ? 2 : 0);
    const bool wave = p.bookkeeping_form == 2;
    p.prepass_mode = (!render || !in.lp_ok) ? 0 : p.lp_compute ? p.lp_compute : in.prepass >= 0 ? in.prepass : 1 /* DSP_PREPASS_F16 */;
    p.guard_on = p.prepass_mode && in.prepass_guard && fp32;
    // Latency path, prepass on: the unclassified samples go STRAIGHT into the jacobian launch (forward + backward, their sdf scattered back for
    // the occupancy scan) instead of a forward launch of their own followed by forward + backward of the kept ones.  One decoder launch less per
    // iteration; the backward sweep of the ~25 % band samples that are not kept is wasted, so only while surface points + band samples fit one
    // round of 16-point tiles.  The Gram kernel reads each kept row's gradient where that launch left it (jrow), in the same row order: same bits.
    p.speculative_band = wave && p.prepass_mode && latency_ok && tri(in.speculative, one_round16);
    // Jacobian launch in the latency form (mlp_split_kernel: a tile takes ~1/3 of a 64-point tile's time)?  Worth it only while the 16-point
    // tiles still fit a round or two over the CUs.
    const double rows = sum_pts + (render ? (p.speculative_band ? 0.16 : 0.045) * (double)in.sum_rays * in.D : 0.0);   // M + typical K (or band)
    p.split_rows = latency_ok && tri(in.split_rows, 0.34 * std::ceil(rows / SPLIT_TILE / n_cu) <= 0.8 * std::ceil(rows / TILE / n_cu));
    // Mixed form of mask reuse (latency path, lists too long for the speculative band rows -- e.g. ONE cfg2-size object: 125 surface tiles + ~550
    // render-row tiles of 16 points): the forward launch exports the relu masks of its band samples, and the kept render rows run the backward
    // sweep only, as tiles of the same launch as the surface points' forward + backward tiles -- 1/3 less MFMA work for them, and the two kinds
    // share the rounds over the CUs.  DSP_DBG_MASK_REUSE = 0 turns every form of mask reuse off.  A list short enough for the cluster form (a
    // detection with the prepass off: ~16 surface + ~60 render-row tiles) is faster there, forward sweep repeated (one round of ~120 us), than mixed on one workgroup per tile (241 us)
    p.cluster_max_tiles = 2 * in.n_clusters;
    const double exp_tiles = (sum_pts + 0.045 * (double)in.sum_rays * in.D) / SPLIT_TILE;
    const bool cluster_instead = in.mixed_reuse < 0 && in.cluster_tiles != 0 && in.n_clusters >= 8 && exp_tiles <= p.cluster_max_tiles;
    p.mixed_reuse = render && p.split_rows && !p.speculative_band && in.mask_reuse != 0 && in.mixed_reuse != 0 && !cluster_instead;
    p.mask_reuse = p.reuse_throughput || p.mixed_reuse;
    // Latency form, lists of at most two rounds of clusters (detections of SLAM's real size: 40-60 tiles of 16 points): four workgroups per tile,
    // the layer rows split over their 16 waves, hand-off through L2 after every pass (mlp_cluster_kernel.hip; it has no backward-only tiles).  The
    // tile count is known on the device only, so the cluster kernel AND the latency-form kernel are launched; each looks at the count and one
    // returns at once.  A pin (DSP_DBG_CLUSTER_TILES) beats the cool-down (a hand-off was lost on this handle a few runs ago: a co-tenant kept a member off its CU).
    p.cluster = p.split_rows && in.n_clusters >= 8 && !p.mixed_reuse && tri(in.cluster_tiles, in.cl_cooldown <= 0);
    // The latency form for the forward launches over ray samples (per pass roughly a third of the in-sphere samples).
    // tools/probes/gpu_split_probe.py: 4 real-size objects 14.8 vs 17.3 ms forward; 1-2 cfg2 objects: 64-point tiles win
    p.split_fwd = render && latency_ok && tri(in.split_rows, 0.30 * std::ceil(0.2 * cap_s / SPLIT_TILE / n_cu) <= 0.8 * std::ceil(0.2 * cap_s / TILE / n_cu));
    // Forward launches of 64-point tiles that end in a mostly empty last round hand that remainder to the latency-form kernel (k_tail_tiles).
    // Small batches only (the throughput form of mask reuse keeps whole 64-point launches), and not where the whole launch is in the latency
    // form already.  With the mixed form of mask reuse on, the tail tiles export their masks too (mlp_split_kernel<1>).
    p.tail_split = render && latency_ok && !p.split_fwd && tri(in.tail_split, true);
    // Prepass tile: 128 points (two 16-point column blocks per wave), or 64 (one) where the 128-point tiles of an iteration would leave more
    // than ~40 % of the CUs without one -- a detection of SLAM's real size has ~117 of them on 256 CUs: twice as many tiles of half the length
    // (the same arithmetic per point: the same values)
    p.lp_tile_pts = p.lp_compute ? LP_TILE : (in.lp_tile == LP_TILE || in.lp_tile == LP_TILE_SMALL) ? in.lp_tile
                  : 0.75 * cap_s / LP_TILE <= 0.6 * n_cu ? LP_TILE_SMALL : LP_TILE;
    p.fwd_tile_pts = p.split_fwd ? SPLIT_TILE : TILE;
    p.jac_tile_pts = p.lp_compute ? LP_TILE : p.split_rows ? SPLIT_TILE : TILE;
    p.direct_tiles = wave && in.B == 1 && in.direct_tiles != 0 && fp32;
    // Forward decoder, front to back with exact early ray termination (gn_kernels.hip, "front-to-back ray passes").
    //  * explicit pass count / boundaries (dsp_batch_set_ray_passes / dsp_batch_debug_ray_pass_bounds): fixed depth-index ranges for all rays;
    //  * automatic (default): per-ray ranges steered by where each ray terminated in the previous GN iteration -- pass 0 decodes [0, hint + 2), a
    //    middle pass the next 8 indices (only with enough tiles to fill the chip), the last pass the rest: fewer launches, less overshoot.
    // With the prepass on, these passes run the LOW-PRECISION kernel (a ray stops behind its first certainly-solid sample), and one fp32 launch
    // follows over the samples the prepass could not classify (k_band_count).
    if (render) {
        const double tiles = 0.75 * cap_s / (p.prepass_mode ? LP_TILE : TILE);     // expected forward tiles per iteration
        int fixed = in.n_ray_passes;
        if (fixed <= 0 && tiles >= 100.0 * n_cu) fixed = 10;   // large batches: ten uniform ranges measured best
        // a prepass over every sample that fits a round and a half of 128-point tiles is one launch with no pass bookkeeping at all
        if (fixed <= 0 && p.prepass_mode && cap_s / LP_TILE <= 1.5 * n_cu) fixed = 1;
        if (fixed > 0) {
            p.fixed_passes = std::max(1, std::min(fixed, in.D));
            p.explicit_bounds = in.n_pass_bounds == p.fixed_passes + 1;
            p.whole = p.prepass_mode && (p.explicit_bounds ? in.n_bound_ranges : p.fixed_passes) == 1;
        } else {
            // small and medium batches: few launches matter more than the last few % of skipped samples
            // (tools/probes/gpu_auto_probe.py: 1 object 32.3 ms vs 32.9 fixed-2; 8 objects 45.4 obj/s vs 43.1 fixed-10)
            p.hint_passes = tiles >= 12.0 * n_cu ? 3 : 2;
        }
    }


    // what ties the forms together
    assert(p.bookkeeping_form == 0 || p.bookkeeping_form == 2);
    assert(!p.speculative_band || (p.bookkeeping_form == 2 && p.prepass_mode && !p.reuse_throughput && !p.lp_compute));
    assert(!p.cluster || (p.split_rows && !p.mixed_reuse));
    assert(!p.mixed_reuse || (p.split_rows && !p.speculative_band));
    assert(p.mask_reuse == (p.reuse_throughput || p.mixed_reuse));
    assert(!p.reuse_throughput || !(p.split_rows || p.split_fwd || p.tail_split || p.cluster || p.mixed_reuse || p.speculative_band));
    assert(!p.lp_compute || (p.prepass_mode == p.lp_compute && !p.guard_on && !p.mask_reuse && !p.split_rows && !p.cluster && !p.split_fwd &&
                             !p.tail_split && !p.speculative_band && !p.direct_tiles && p.lp_tile_pts == LP_TILE && p.jac_tile_pts == LP_TILE));
    assert(!(p.split_fwd && p.tail_split) && (!p.direct_tiles || wave) && (!p.whole || (p.prepass_mode && p.fixed_passes >= 1)));
    assert(render ? (p.fixed_passes > 0) != (p.hint_passes > 0)
                  : !(p.lp_compute || p.prepass_mode || p.mask_reuse || p.bookkeeping_form || p.speculative_band || p.split_fwd || p.tail_split || p.fixed_passes || p.hint_passes));
    return p;
}
}  // namespace launch_plan
