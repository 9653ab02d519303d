/* dsp_gn.h -- C ABI of libdspgn: MI355X (gfx950) DeepSDF shape-code + pose Gauss-Newton optimiser.
 *
 * Drop-in boundary for ONE hot path of DSP-SLAM (reference: JingwenWang95/DSP-SLAM).  The reference has
 * no FFI of its own for this path: C++ reaches it through an embedded CPython interpreter
 * (src/LocalMapping.cc:38-40, src/LocalMapping_util.cc:109-110,179-196,391-426) calling the Python
 * functions listed below.  Each entry point here cites the reference interface it replaces; the Python
 * mirror package (dsp_slam_amd/reconstruct, dsp_slam_amd/deep_sdf) binds these through ctypes and keeps
 * the reference's Python names, so the C++ caller is unchanged.
 *
 * Conventions: plain C types; all pointers are HOST pointers unless a name ends in _dev; row-major
 * float32; every function returns 0 on success or a negative DSP_E_* code (dsp_last_error() gives
 * text).  A handle owns one device, one HIP stream and its device memory; calls on one handle (and on
 * batches created from it) are serialised INSIDE the library (a per-handle mutex), so they may come from
 * any thread; different handles are independent.  Nothing here depends on Python or PyTorch.
 */
#ifndef DSP_GN_H
#define DSP_GN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSP_OK 0
#define DSP_E_ARG (-1)      /* bad argument / unsupported decoder geometry */
#define DSP_E_HIP (-2)      /* HIP runtime error */
#define DSP_E_NOMEM (-3)
#define DSP_E_STATE (-4)

#define DSP_CODE_LEN 64
#define DSP_GRAD_DIM 67     /* d sdf / d [code(64), x, y, z] */

typedef struct dsp_handle dsp_handle;
typedef struct dsp_batch dsp_batch;

/* Folded decoder weights, layer k: weights[k] is (out_dims[k] x in_dims[k]) row-major, biases[k] (out_dims[k]).
 * Replaces deep_sdf/workspace.py:202-223 (config_decoder) + Decoder.__init__ (deep_sdf/deep_sdf_decoder.py:10-73):
 * weight-norm is folded by the caller, W = g * v / ||v||_row.  Supported geometry (checked by dsp_create, DSP_E_ARG otherwise): code_len
 * 64 or 32; ONE hidden width, a multiple of 16 and at most 512 (narrower decoders run embedded in the 512-row slabs); 2..8 hidden layers;
 * exactly one latent_in layer >= 2 whose input is [h | code | xyz] (the layer in front of it emits width - code_len - 3 rows); final layer
 * width -> 1 + tanh.  The optimiser state always carries 64 code entries (the unused ones of a 32-D decoder stay zero).  The low-precision
 * prepass additionally needs an even number of hidden layers (DeepSDF's 8); other decoders run with the prepass off. */
typedef struct dsp_decoder_desc {
    int32_t n_layers;            /* number of Linear layers (9 for DSP-SLAM) */
    int32_t code_len;            /* 64 or 32 */
    int32_t latent_in;           /* index of the layer whose input is [h | code | xyz] (4), or -1 */
    const int32_t* out_dims;     /* [n_layers] */
    const int32_t* in_dims;      /* [n_layers] */
    const float* const* weights; /* [n_layers] */
    const float* const* biases;  /* [n_layers] */
} dsp_decoder_desc;

/* Hyper-parameters read by Optimizer.__init__ (reconstruct/optimizer.py:27-43). */
typedef struct dsp_gn_params {
    float k1, k2, k3, k4;        /* render / sdf / code-prior / rotation-prior weights */
    float b1, b2;                /* Huber thresholds: render, sdf */
    float lr;                    /* learning_rate */
    float s_damp;                /* scale_damping */
    int32_t num_iterations;      /* joint_optim.num_iterations */
    int32_t num_depth_samples;   /* optimizer.num_depth_samples (2 .. 64; DSP_E_ARG otherwise) */
    float cut_off;               /* optimizer.cut_off_threshold (positive and finite; DSP_E_ARG otherwise) */
    int32_t pose_only_iterations;/* pose_only_optim.num_iterations */
} dsp_gn_params;

/* Per-object status of a batch run (ragged failures do not poison the batch). */
#define DSP_OBJ_GOOD 0
#define DSP_OBJ_FEW_SAMPLES 1   /* < 10 in-sphere ray samples: compute_render_loss returned None (loss.py:73-74) */
#define DSP_OBJ_NAN 2           /* NaN loss, e.g. K == 0 (optimizer.py:135-136,149-150) */

/* Counters and device timings of the last run of a batch. */
typedef struct dsp_stats {
    double n_fwd_points;         /* forward-only decoder points actually evaluated (<= sum of V: samples behind a solid sample are skipped) */
    double n_jac_points;         /* points decoded forward + backward: sum of M (surface), plus K (render rows) without mask reuse */
    double ms_total;             /* HIP-event time of the whole run on the handle's stream */
    double ms_mlp_fwd;           /* summed time of the forward-only decoder kernel launches (0 with kernel timing off: dsp_batch_set_kernel_timing) */
    double ms_mlp_jac;           /* summed time of the forward+gradient decoder kernel launches (likewise) */
    int32_t n_mlp_fwd_launches;
    int32_t n_mlp_jac_launches;
    double n_insphere_points;    /* sum over iterations and objects of V, the in-sphere sample count the reference decodes */
    double n_render_rows;        /* render rows that ran the backward sweep only (mask reuse on): sum of K, else 0 */
    /* prepass (ABI version 2): with it on, n_fwd_points counts only the samples that still needed the fp32 kernel */
    double n_prepass_points;     /* samples decoded by the low-precision prepass kernel */
    double ms_mlp_prepass;       /* summed time of the prepass kernel launches */
    int32_t n_mlp_prepass_launches;
    int32_t prepass_mode;        /* DSP_PREPASS_* the run used */
    float prepass_delta;         /* margin the run used: samples with |sdf_lp| < cut_off + delta went to the fp32 kernel */
    float prepass_max_err;       /* audit only: max |sdf_lp - sdf_fp32| over the audited samples */
    double prepass_misclassified;/* audit only: samples classified against their fp32 value (must be 0) */
    double prepass_audited;      /* audit only: samples compared */
    /* always-on prepass guard (ABI version 3): every sample the fp32 kernel re-decodes -- the widened band plus a stratified sample of
     * the classified ones -- is compared with the prepass value it replaces */
    double prepass_guard_trips;  /* waves that saw |sdf_lp - sdf_fp32| >= half the object's margin (0 in a healthy run) */
    double prepass_guard_objects;/* objects with at least one trip */
    float prepass_guard_max_err; /* largest |sdf_lp - sdf_fp32| over the compared samples */
    int32_t prepass_guard_rerun; /* 1: the guard tripped; the objects it tripped on were run again with the prepass off (their results come from that run) */
    double n_cluster_tiles;      /* (ABI version 4) 16-point jacobian tiles that ran in the cluster form: four workgroups per tile (dsp_batch_set_cluster_tiles) */
    int32_t cluster_fallback;    /* (ABI version 5) 1: a cluster-form launch of this run lost a hand-off within its time bound (2 ms: a busy shared GPU kept one of the
                                  * four workgroups off its CU); the latency-form kernel recomputed that launch and took the run's remaining lists on the device --
                                  * same results, a few ms later; the handle keeps the cluster form off for its next 64 runs */
    int32_t cluster_cooldown;    /* (ABI version 6) runs for which the handle still keeps the cluster form off after a lost hand-off (0 = it is in use again) */
} dsp_stats;

/* ---- lifetime --------------------------------------------------------------------------------- */
/* Thread safety: calls on ONE handle (and on batches created from it) are serialised inside the library (one call at a time per handle);
 * different handles are independent.  Callers that release the GIL around these calls (ctypes, pybind11) may therefore call from any thread. */
int dsp_create(const dsp_decoder_desc* decoder, int device, dsp_handle** out);
/* Destroys the handle AND every resident batch still alive on it.  A dsp_batch* is an opaque, generation-tagged TOKEN, not an address: once its
 * batch is gone -- destroyed, or taken by dsp_destroy of its handle -- every call that is handed the token returns DSP_E_ARG (dsp_batch_destroy:
 * does nothing), also after the memory has been reused for another batch.  So the two destroy calls are safe in either order and from any
 * thread (finalisers at interpreter exit run in no particular order); dsp_destroy waits for calls in flight on the handle's batches, and
 * dsp_batch_destroy for calls in flight on that batch (a call that starts after it sees a stale token). */
void dsp_destroy(dsp_handle* h);
/* A handle keeps device blocks (up to 1 GiB, size-classed) and pinned host staging of dropped one-shot batches for its next call.  dsp_trim
 * hands all of it back to the runtime: for a process that shares the GPU with another allocator (torch, RCCL, a second handle).  Destroying
 * a LARGE resident batch (more than 512 MiB left parked behind it) trims the cache to the footprint of one KITTI-size detection (64 MiB) on
 * its own; detection-sized batches created and destroyed per frame keep their blocks. */
int dsp_trim(dsp_handle* h);
/* Priority of the handle's HIP stream among the queues of the device: 1 = highest, 0 = default, -1 = lowest the device offers.  Where the GPU
 * is shared -- DSP-SLAM runs its detectors on it from the Tracking thread (src/Tracking_util.cc:31-57) while this path runs in the
 * LocalMapping thread (src/LocalMapping_util.cc:165-203) -- the integrator decides who yields: -1 lets the detectors' kernels go first,
 * 1 shortens a detection's ~110 dependent kernels beside them.  The stream is re-created (after a synchronisation); batches of the handle
 * pick the new one up at their next run.  Results do not depend on it. */
int dsp_set_stream_priority(dsp_handle* h, int priority);
const char* dsp_last_error(const dsp_handle* h);   /* h may be NULL: error of the last failed dsp_create */
int dsp_abi_version(void);
/* Which compiler produced this library (hipcc --version at build time, clang version, HIP header version) -- the decoder kernels rely on
 * properties of the generated code that the build checks by disassembly (dsp_slam_amd/build.py: check_isa); and the HIP runtime / driver
 * versions of the box it is running on (hipRuntimeGetVersion / hipDriverGetVersion encodings). */
const char* dsp_build_info(void);
int dsp_runtime_versions(int* hip_runtime, int* hip_driver);
int dsp_device_count(void);   /* number of gfx950 devices dsp_create accepts (ordinals 0 .. n-1); 0 without a HIP device */

/* ---- decoder ---------------------------------------------------------------------------------- */
/* decode_sdf(decoder, lat_vec, x)  -- reconstruct/loss_utils.py:51-79.  pts (n,3) object frame -> sdf (n). */
int dsp_decode_sdf(dsp_handle* h, const float* code, const float* pts, int64_t n, float* sdf_out);
/* The same decoder evaluated by the low-precision PREPASS kernel (v_mfma_f32_16x16x32_f16 / _bf16, fp32 accumulation; xyz, code
 * and biases enter at fp32 accuracy, hidden activations are rounded to 16 bits per layer).  Never used for results: the optimiser
 * uses it only to classify ray samples whose occupancy is exactly 0 or 1 (sdf outside the cut-off band by more than a calibrated
 * margin, reconstruct/loss_utils.py:40-48); exposed for calibration and tests. */
#define DSP_PREPASS_OFF 0
#define DSP_PREPASS_F16 1
#define DSP_PREPASS_BF16 2
#define DSP_PREPASS_SMALL_TILES 0x100   /* or-ed into dtype: run the kernel's 64-point-tile form (one 16-point column block per wave) */
int dsp_decode_sdf_prepass(dsp_handle* h, int dtype, const float* code, const float* pts, int64_t n, float* sdf_out);
/* The same point set decoded for n_codes shape codes in ONE launch: sdf_out[c * n + i].  Batched form of the
 * MeshExtractor grid decode (reconstruct/optimizer.py:217-218) / the per-object loop of extract_map_objects.py:46-63. */
int dsp_decode_sdf_multi(dsp_handle* h, const float* codes, int64_t n_codes, const float* pts, int64_t n, float* sdf_out);
/* get_batch_sdf_jacobian through the 16-bit kernels of the LOW-PRECISION COMPUTE MODE (dsp_batch_set_compute below): f16 / bf16 matrix operands,
 * fp32 accumulation, forward and backward.  NOT the parity path -- exposed so that its accuracy can be measured point by point. */
#define DSP_COMPUTE_F32 0
#define DSP_COMPUTE_F16 1
#define DSP_COMPUTE_BF16 2
int dsp_sdf_jacobian_lp(dsp_handle* h, int dtype, const float* code, const float* pts, int64_t n, float* sdf_out, float* grad_out);
/* get_batch_sdf_jacobian(decoder, lat_vec, x, 1) -- reconstruct/loss_utils.py:82-103.
 * sdf_out (n), grad_out (n, 67) = d sdf / d [code, xyz]. */
int dsp_sdf_jacobian(dsp_handle* h, const float* code, const float* pts, int64_t n, float* sdf_out, float* grad_out);

/* ---- residual terms --------------------------------------------------------------------------- */
/* compute_sdf_loss(decoder, pts_surface_cam, t_obj_cam, latent_vector) -- reconstruct/loss.py:22-43.
 * Outputs: jac_pose (n,7), jac_code (n,64), res (n). */
int dsp_compute_sdf_loss(dsp_handle* h, const float* pts_cam, int64_t n, const float* t_obj_cam, const float* code,
                         float* jac_pose, float* jac_code, float* res);
/* compute_render_loss(decoder, ray_directions, depth_obs, t_obj_cam, sampled_ray_depth, latent_vector, th)
 * -- reconstruct/loss.py:46-152.  *k_out = number of rows K, or -1 when the reference returns None
 * (< 10 in-sphere samples).  Outputs need capacity n_rays * n_depths rows; row order = the reference's
 * (ray-major, depth-minor).  v_out / m_out (optional) receive the ragged set sizes V and m.  m (samples with |sdf| < th) is
 * INFORMATIONAL: with early ray termination or the prepass on, samples behind a ray's first solid sample are not decoded (their
 * transmittance is exactly 0, so they cannot reach K, the rows or the results), and they are not counted in m either -- it can be smaller
 * than the reference's m.  V and K are the reference's. */
int dsp_compute_render_loss(dsp_handle* h, const float* rays, int64_t n_rays, const float* depth_obs,
                            const float* t_obj_cam, const float* sampled_depth, int32_t n_depths, const float* code,
                            float th, int64_t* k_out, float* jac_pose, float* jac_code, float* res, int64_t* v_out,
                            int64_t* m_out);

/* ---- optimiser -------------------------------------------------------------------------------- */
/* Optimizer.reconstruct_object for a ragged batch of independent objects -- reconstruct/optimizer.py:88-203.
 * Object i uses pts[pts_off[i]..pts_off[i+1]) (camera frame, (M_i,3)), rays[ray_off[i]..ray_off[i+1]) ((R_i,3);
 * the first n_fg[i] rows are foreground and pair with depth[depth_off[i] + r]), t_cam_obj[i] (4x4 Sim(3)
 * object->camera initial estimate) and codes_in[i] (64; NULL => zero start, optimizer.py:96-99).
 * Outputs per object: t_cam_obj (16), code (64), loss (k1*L_render + k2*L_sdf at the last linearisation
 * point, :155), status (DSP_OBJ_*).  For a failed object t_cam_obj/code hold the last state. */
int dsp_reconstruct_batch(dsp_handle* h, const dsp_gn_params* prm, int32_t n_objects, const int64_t* pts_off,
                          const float* pts, const int64_t* ray_off, const float* rays, const int64_t* depth_off,
                          const float* depth, const float* t_cam_obj_in, const float* codes_in,
                          float* t_cam_obj_out, float* codes_out, float* loss_out, int32_t* status_out);

/* MULTI-VIEW reconstruction (an addition; the reference optimises an object from ONE observation, optimizer.py:88-203, although its map holds
 * one per key frame, src/Optimizer_util.cc:196-217): object i has one Sim(3) pose and one code, observed by the views
 * view_off[i] .. view_off[i+1]-1 (at least one).  View v has t_ref_view[v] (4x4 rigid: view-v camera -> the object's reference camera; the
 * object's first view IS the reference camera: identity) and its own pts / rays / depth in ITS camera frame -- pts_off, ray_off, depth_off
 * have n_views + 1 entries, laid out as dsp_reconstruct_batch lays them out per object; any of a view's counts may be 0.  t_cam_obj_in /
 * codes_in and the outputs are per OBJECT (t_cam_obj in the reference camera's frame).  Per iteration, with T_oc_v = T_oc * t_ref_view[v]:
 *   - per view exactly the reference's two terms at T_oc_v: compute_sdf_loss (loss.py:22-43) and compute_render_loss (loss.py:46-152) with the
 *     depth samples and the background depth derived from T_oc_v as optimizer.py:120-126 derives them from T_oc; a view whose render term is
 *     None (< 10 in-sphere samples, loss.py:73-74) contributes no render rows in that iteration (it may in a later one);
 *   - the rows of all views are ONE row set: H = k2 sum J^T J / sum M_v + k1 sum J^T J / sum K_v, b and the loss likewise (optimizer.py:134-168);
 *     code prior, rotation prior (from T_oc), damping, solve and the update T_oc <- exp_sim3(dx) T_oc as optimizer.py:170-192 -- the update is
 *     a left perturbation in the object frame, so it moves every T_oc_v alike.
 * Status: DSP_OBJ_FEW_SAMPLES when no view reached 10 in-sphere samples; DSP_OBJ_NAN when sum M_v == 0, sum K_v == 0 or a loss is NaN.
 * With one view per object the result is dsp_reconstruct_batch's, bit for bit.  DSP_E_ARG: view_off not increasing from 0 (an object
 * without views), a t_ref_view that is not rigid (R^T R - I or the bottom row off by more than 1e-4), a first view that is not the identity. */
int dsp_reconstruct_multiview(dsp_handle* h, const dsp_gn_params* prm, int32_t n_objects, const int64_t* view_off, const float* t_ref_view,
                              const int64_t* pts_off, const float* pts, const int64_t* ray_off, const float* rays, const int64_t* depth_off,
                              const float* depth, const float* t_cam_obj_in, const float* codes_in, float* t_cam_obj_out, float* codes_out,
                              float* loss_out, int32_t* status_out);

/* Optimizer.estimate_pose_cam_obj for a ragged batch -- reconstruct/optimizer.py:45-86.
 * t_co_se3_in[i] (4x4 SE(3)), scale[i], pts as above, codes[i] (64).  Output t_co_se3_out[i] (4x4 SE(3)).
 * The inputs are not modified (the reference scales the caller's matrix in place, :53-54).
 * After the update of iteration 4 the points with |sdf| > 0.05 at that iteration's start are dropped, and the following iterations
 * divide by the number left (:76-78).  An object left with no points -- or given none -- has H = J^T J / 0 in the reference, which
 * returns NaN: such an object's t_co_se3_out is NaN in all 16 entries here too (its status, with dsp_batch_create_pose, is DSP_OBJ_NAN). */
int dsp_estimate_pose_batch(dsp_handle* h, const dsp_gn_params* prm, int32_t n_objects, const int64_t* pts_off,
                            const float* pts, const float* t_co_se3_in, const float* scale, const float* codes,
                            float* t_co_se3_out);

/* ---- mesh extraction (reference MeshExtractor.extract_mesh_from_code, reconstruct/optimizer.py:206-223 ->
 *      create_voxel_grid / decode_sdf / convert_sdf_voxels_to_mesh, reconstruct/utils.py:97-140) -----------------------------------
 * dsp_extract_mesh decodes the vol_dim^3 grid over [-1,1]^3 and runs marching cubes (level 0) on the device; the SDF volume
 * never leaves HBM.  The sample points are the ones the reference's create_voxel_grid really produces: under torch >= 1.6 its
 * `overall_index.long() / vol_dim` is true division, so the grid is sheared by up to one voxel (y index + z / N, x index + y / N + z / N^2);
 * DSP_MESH_REGULAR_GRID samples the regular lattice instead.  Vertices are placed on the regular lattice either way, as in the reference.  It returns the mesh size; dsp_mesh_fetch then copies the last mesh extracted on this handle:
 * vertices (n_vertices x 3 float32, object frame: index * voxel_size - 1, voxel_size = 2 / (vol_dim - 1)) and faces
 * (n_faces x 3 int32 vertex ids, normals by the right-hand rule along +grad sdf, i.e. outward).  One vertex per sign-changing grid
 * edge (shared between faces, like scikit-image's output); order: vertices by (grid point, axis), faces by (cell, case-table order).
 * An empty mesh (no sign change) is n_vertices = n_faces = 0 and not an error here (the Python mirror raises scikit-image's
 * ValueError for it).  The case table is a generated classic table, not Lewiner's: see oracle/mc_oracle.py. */
#define DSP_MESH_REGULAR_GRID 1   /* flags: sample the regular lattice instead of the reference's sheared grid (see below) */
#define DSP_MESH_PREPASS_F16 2    /* flags: decode the grid with the f16 prepass kernel and only the surface band in fp32 (see dsp_extract_meshes) */
#define DSP_MESH_PREPASS_BF16 4   /* flags: the same with the bf16 prepass kernel (at most one of the two) */
int dsp_extract_mesh(dsp_handle* h, const float* code, int32_t vol_dim, int32_t flags, int64_t* n_vertices, int64_t* n_faces);
/* Batched extraction: the meshes of n_codes objects (codes: n_codes x 64) on one vol_dim^3 grid, in chunks that fit a fixed device
 * budget.  n_vertices[i] / n_faces[i] receive object i's mesh size (0 / 0 when its surface does not cross the grid: not an error);
 * dsp_meshes_fetch copies them.  Each object's mesh is, bit for bit and in the same order, what dsp_extract_mesh returns for it.
 * Without a DSP_MESH_PREPASS_* flag every grid point is decoded in fp32.  With one, the low-precision prepass decodes every grid
 * point; a point gets its fp32 value when its prepass value lies within the object's margin delta of 0 (or is not finite), or when one
 * of its axis neighbours does or is certain of the other sign -- so every sign marching cubes reads is certified and every value it
 * interpolates is fp32 -- plus a fixed stratified audit sample of the rest.  The fp32 kernel's guard compares both values; an object
 * with a difference of delta / 2 or more is decoded densely in fp32 again.  delta <= 0: the margin calibrated at dsp_create for the
 * object's code magnitude (the table is read, never changed by a mesh call); delta > 0: that margin for every object.  A decoder
 * without a prepass kernel refuses the flags (DSP_E_ARG). */
int dsp_extract_meshes(dsp_handle* h, const float* codes, int64_t n_codes, int32_t vol_dim, int32_t flags, float delta, int64_t* n_vertices,
                       int64_t* n_faces);
/* Copies the meshes of the last dsp_extract_meshes on this handle, concatenated in object order: vertices (sum n_vertices) x 3 float32,
 * faces (sum n_faces) x 3 int32, face indices local to their own mesh.  n_codes / n_vertices / n_faces must be what that call returned,
 * else nothing is copied and DSP_E_STATE is returned. */
int dsp_meshes_fetch(dsp_handle* h, int64_t n_codes, const int64_t* n_vertices, const int64_t* n_faces, float* vertices, int32_t* faces);
/* Counts of the last mesh extraction on this handle (dsp_extract_mesh or dsp_extract_meshes): counts5 = {grid points decoded by the
 * prepass, fp32 points of the surface band, fp32 points of the audit, grid points decoded densely in fp32 (no prepass, or objects
 * re-run), objects re-run densely after a guard trip}; max_guard_err (optional) = largest |prepass - fp32| the guard saw. */
int dsp_mesh_last_stats(dsp_handle* h, int64_t* counts5, float* max_guard_err);
/* The marching-cubes step alone on a host volume (n0 x n1 x n2, axis 0 slowest): vertices = index * spacing + origin
 * (replaces convert_sdf_voxels_to_mesh, utils.py:119-140, with spacing = 2 / (n - 1), origin = -1, level = 0). */
int dsp_marching_cubes(dsp_handle* h, const float* volume, int32_t n0, int32_t n1, int32_t n2, float level, float spacing, float origin,
                       int64_t* n_vertices, int64_t* n_faces);
/* Copies the last mesh extracted on this handle.  n_vertices / n_faces are the counts the caller sized its buffers for (as returned by
 * its dsp_extract_mesh / dsp_marching_cubes call); if the handle's last mesh has other counts -- another thread extracted in between --
 * nothing is copied and DSP_E_STATE is returned. */
int dsp_mesh_fetch(dsp_handle* h, float* vertices, int64_t n_vertices, int32_t* faces, int64_t n_faces);

/* ---- surface projection: points onto the decoded zero set, with the decoder's own normals ------------------------------------------
 * The decoder's forward + input-gradient launch (the one behind dsp_sdf_jacobian) gives sdf and g = d sdf / d xyz at a point; one step is
 * p <- p - sdf g / |g|^2, capped at max_step in length (a longer step is scaled to max_step; a point whose |g|^2 is below 1e-20 or whose
 * step is not finite stays where it is).  After n_steps steps one more launch gives, at the final points: normal = g / |g| (zero where
 * |g|^2 < 1e-20), sdf, grad_norm = |g| and -- with a code variance -- sigma = sqrt(sum_k (d sdf / d code_k)^2 var_k) / |g|, the
 * first-order standard deviation of the surface's displacement along the normal.  The arithmetic is csrc/surface_math.h, one correctly
 * rounded fp32 operation at a time, the same on the device and in the dsp_debug_surface_* host functions.
 *
 * dsp_surface_points: n_codes objects (codes: n_codes x 64), object c owns pts[pts_off[c] .. pts_off[c+1]) (x 3 floats, object frame);
 * pts_off has n_codes + 1 entries, non-decreasing from 0.  n_steps 0 .. 8 (0: attributes at the points as given).  max_step > 0.
 * var_code: NULL or n_codes x 64 doubles as dsp_batch_posterior_fetch writes them (finite, >= 0, else DSP_E_ARG; entries at or beyond the
 * decoder's code length are ignored).  Any output may be NULL; sigma requires var_code (DSP_E_ARG).  pts_out / normals: 3 floats per
 * point; sdf / grad_norm / sigma: one.  Objects without points and a total of zero points are not errors.  A non-finite input point has
 * NaN in its own outputs and disturbs no other point.  The work runs in chunks under a fixed device budget; a batched, ragged or
 * chunked call computes each point exactly as a call with that point alone. */
int dsp_surface_points(dsp_handle* h, const float* codes, int64_t n_codes, const int64_t* pts_off, const float* pts, int32_t n_steps, float max_step,
                       const double* var_code, float* pts_out, float* normals, float* sdf, float* grad_norm, float* sigma);
/* The same on the vertices of the last dsp_extract_meshes of this handle, device resident, with the codes that call was given (the handle
 * keeps a host copy).  n_codes / n_vertices must be what that call returned (else DSP_E_STATE).  max_step <= 0: one voxel of that
 * extraction, 2 / (vol_dim - 1).  The marching-cubes vertices stay what they are: dsp_meshes_fetch is unchanged.  The results stay on
 * the device until the next dsp_extract_meshes on the handle. */
int dsp_meshes_refine(dsp_handle* h, int64_t n_codes, const int64_t* n_vertices, int32_t n_steps, float max_step, const double* var_code);
/* Copies what the last dsp_meshes_refine left, concatenated in object order like dsp_meshes_fetch: refined vertices and normals
 * (sum n_vertices x 3), sdf and sigma (sum n_vertices); any may be NULL.  DSP_E_STATE: no refine since the last extraction, other
 * counts, or sigma requested when the refine had no var_code. */
int dsp_meshes_fetch_attributes(dsp_handle* h, int64_t n_codes, const int64_t* n_vertices, float* vertices, float* normals, float* sdf, float* sigma);
/* Host only, no handle: csrc/surface_math.h's two functions on arrays.  dsp_debug_surface_step: n points, their sdf (n) and gradient
 * (n x 3) -> pts_out (n x 3).  dsp_debug_surface_attributes: n rows of 68 floats {d sdf / d code [64], d sdf / d xyz [3], sdf} and ONE
 * variance of 64 doubles (or NULL) for all of them; any output may be NULL, sigma requires var_code. */
int dsp_debug_surface_step(int64_t n, const float* pts, const float* sdf, const float* grad_xyz, float max_step, float* pts_out);
int dsp_debug_surface_attributes(int64_t n, const float* rows68, const double* var_code, float* normals, float* grad_norm, float* sdf, float* sigma);
/* Testing: this handle's chunk budget of the surface projection in decoder rows (0 = the default, 64 MiB of rows), so that a small call
 * crosses chunk borders. */
int dsp_debug_surface_chunk_rows(dsp_handle* h, int64_t rows);

/* ---- map query: signed distance and normal of world points to a map of posed objects ------------------------------------------------
 * A map is n_obj objects, each an object-to-world Sim(3) pose (4x4 row-major, as MapObjects.txt carries it) and a code.  For every world
 * point the call answers: which object, how far from its surface, and -- with DSP_QUERY_NORMALS -- in which direction the surface lies.
 *   obj    index of the object with the smallest world-scaled signed distance among the objects whose unit sphere (object frame) contains
 *          the point; -1 if no sphere contains it.  Equal distances go to the lower index.
 *   dist   that object's sdf * s, s its object-to-world scale: negative inside the shape; +inf when obj == -1.
 *   bound  the minimum over the objects whose sphere does NOT contain the point of (|p_o| - 1) * s, the distance to that sphere; +inf if
 *          there is none.  The decoder says nothing beyond its sphere, so dist <= bound certifies that obj really is the nearest object,
 *          and min(dist, bound) is the clearance a planner would use.
 *   normal the unit outward normal of the winning object's surface in the WORLD frame: the decoder's own d sdf / d xyz, rotated and
 *          normalised; zeros when obj == -1 or when |g|^2 < 1e-20 (the rule of dsp_surface_points).
 * DeepSDF's output is a clamped (tanh) distance: metric near the surface, saturating away from it.  So dist is exact in sign, exact near
 * the surface, and an under-estimate in magnitude far from it.
 * A point with a NaN coordinate is inside nothing: obj -1, dist +inf, bound NaN; it disturbs no other point.  An object whose decoded
 * distance is NaN, or whose code is not finite, never wins (its sphere still counts in bound).  The arithmetic is csrc/query_math.h, one
 * correctly rounded fp32 operation at a time (the pose inversion: fp64 on the host, rounded once); the decoder rows are those of
 * dsp_decode_sdf / dsp_sdf_jacobian at the object-frame points, bit for bit, and the result does not depend on chunking or on the order
 * in which rows are reduced: two calls return the same bytes.
 *
 * dsp_map_query: t_world_obj n_obj x 16, codes n_obj x 64 (a 32-D decoder reads the first 32 of each row), pts_world n_pts x 3.  flags: 0
 * or DSP_QUERY_NORMALS; normal (n_pts x 3) is required with the flag and must be NULL without it.  n_obj == 0 is valid (-1, +inf, +inf
 * for every point), so is n_pts == 0.  DSP_E_ARG: a NULL output other than normal, a negative count, an unknown flag, or a pose that is
 * not finite, has a bottom row other than 0 0 0 1, has no positive scale, or whose linear part over its scale is not a rotation (R^T R
 * off the identity by more than 1e-4, the test of dsp_reconstruct_multiview's view transforms).  The work runs in passes of at most
 * 131 072 points and chunks of at most 64 MiB of decoder rows, both fixed, whatever the device has free. */
#define DSP_QUERY_NORMALS 1   /* flags: also return the winning object's world-frame unit normal (the decoder's forward + gradient form) */
int dsp_map_query(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts_world, int64_t n_pts, int32_t flags,
                  int32_t* obj, float* dist, float* bound, float* normal);
/* Counts of the last dsp_map_query on this handle: counts4 = {candidate rows (point-in-sphere pairs, each decoded once), decoder tiles of
 * up to 64 rows, chunks, point passes}. */
int dsp_map_query_last_stats(dsp_handle* h, int64_t* counts4);
/* Host only, no handle: csrc/query_math.h on arrays.  dsp_debug_query_invert: n_obj poses -> rt_ow (n_obj x 12: [R_ow | t_ow], row-major
 * 3 x 4) and scale (n_obj); DSP_E_ARG for a pose dsp_map_query refuses.  dsp_debug_query_candidates: p_obj (n_obj x n_pts x 3, object
 * major), inside (n_obj x n_pts bytes) and bound (n_pts); any output may be NULL.  dsp_debug_query_select: n_rows decoder values with
 * their object's scale, object index and point index -> obj / dist per point, the selection of dsp_map_query. */
int dsp_debug_query_invert(int64_t n_obj, const float* t_world_obj, float* rt_ow, float* scale);
int dsp_debug_query_candidates(int64_t n_obj, const float* rt_ow, const float* scale, int64_t n_pts, const float* pts_world, float* p_obj,
                               unsigned char* inside, float* bound);
int dsp_debug_query_select(int64_t n_rows, const float* sdf, const float* scale_of_row, const int32_t* obj_of_row, const int32_t* pt_of_row,
                           int64_t n_pts, int32_t* obj, float* dist);
/* Testing: this handle's chunk budget of the map query in decoder rows (0 = the default, 64 MiB of rows), so that a small call crosses
 * chunk borders. */
int dsp_debug_query_chunk_rows(dsp_handle* h, int64_t rows);
/* Host only, no handle: how dsp_map_query cuts one pass into chunks, as a function of the objects' candidate counts (cnt, n_obj entries
 * >= 0, in object order) and the chunk budget in rows (0 = the default; at most 2^24).  A chunk holds consecutive rows of the list of all
 * (object, candidate) pairs in order: chunks4 receives {o0, nc, n_rows, nt} per chunk (objects [o0, o0 + nc), rows, tiles); base, nc
 * entries per chunk concatenated: chunk row base[k] + j holds candidate j of object o0 + k (negative: the chunk starts inside the object;
 * only rows inside [0, n_rows) belong to the chunk); tiles4, nt x 4 per chunk concatenated: {first row, rows (1 .. 64, of one object),
 * code-bias slot, 0}, slots counting the chunk's objects that have rows in it.  sizes3 = {chunks, entries of base, tiles}; a call with the
 * three arrays NULL only sizes.  pass_pts (optional) receives the points of one pass of a map of pass_n_obj objects (1 .. 2^18): 131 072,
 * fewer from 8193 objects on.  DSP_E_ARG: a negative count, a budget or object count out of range. */
int dsp_debug_query_plan(int64_t n_obj, const int32_t* cnt, int64_t budget, int64_t pass_n_obj, int64_t* sizes3, int32_t* chunks4, int32_t* base,
                         int32_t* tiles4, int64_t* pass_pts);
/* Measurement: on != 0 brackets the following dsp_map_query, dsp_map_align and dsp_map_raycast calls on this handle, and every decoder
 * launch inside them, with HIP events on the handle's stream; ms2 (optional) receives {decoder launches, whole call} of the last such
 * call in milliseconds (0, 0 before one).  The results of a call do not depend on it. */
int dsp_debug_query_timing(dsp_handle* h, int on, double* ms2);

/* ---- ray casting: what does the map look like from here?  First surface hit per world ray ----------------------------------------------
 * For every ray (origin, direction; the direction need not be a unit vector, the parameter t is in world units along the unit direction)
 * the call answers: the depth t of the first object surface, which object it belongs to, the signed distance dist (sdf * s) at the hit
 * sample and -- with DSP_RAYCAST_NORMALS -- the surface's world-frame unit normal there.  Rays are marched by sphere tracing inside every
 * object's unit sphere, with occlusion between objects: the smallest hit parameter wins, the lower object index among equal ones.
 *   obj     the winning object, -1 for none        t     its hit parameter, +inf for none        dist   sdf * s at the hit, +inf for none
 *   status  DSP_RAYCAST_HIT, DSP_RAYCAST_MISS, or DSP_RAYCAST_UNDECIDED: some (ray, object) pair took max_steps samples without ending,
 *           at a parameter below the winner's t or with no winner at all; an UNDECIDED ray still reports the winner it has.
 *   normal  zeros without a winner, and under the rule of dsp_map_query.
 * A ray with a number that is not finite, or a zero direction, is void: -1, +inf, +inf, MISS; it disturbs no other ray.  An object whose
 * code is not finite is never hit.  The arithmetic, the step rule and the occlusion retirement are written out in csrc/raycast_math.h, one
 * correctly rounded fp32 operation at a time; the decoder rows are those of dsp_decode_sdf / dsp_sdf_jacobian at the object-frame
 * samples, bit for bit, and the outputs do not depend on grid sizes, on the pass cut or on the order of reduction: two calls return the
 * same bytes.  The march keeps its state, its compaction and its tile lists on the device; the host reads the pair counts once per call.
 *
 * params: t_min >= 0; t_max > t_min (+inf allowed); eps > 0, finite: a sample with dist <= eps is a hit; 0 < relax <= 1: the step is
 * relax * dist; 1 <= max_steps <= 4096 samples per (ray, object) pair.  dsp_raycast_params_default: 0, +inf, 1e-3, 1, 64.
 * The map is taken and checked as by dsp_map_query.  n_rays == 0 and n_obj == 0 are valid and touch no device.  DSP_E_ARG: a NULL
 * argument (normal excepted), normal without the flag or the flag without normal, an unknown flag, params out of range, n_rays > 2^31 - 1,
 * or a request too large for the fixed budgets -- 64 MiB of code biases (16 384 objects), 64 MiB of pair counts (objects x rays / 64):
 * "split the request".  Pairs are marched in passes of at most the map query's chunk budget (dsp_debug_query_chunk_rows overrides it). */
#define DSP_RAYCAST_NORMALS 1
#define DSP_RAYCAST_MISS 0
#define DSP_RAYCAST_HIT 1
#define DSP_RAYCAST_UNDECIDED 2
typedef struct dsp_raycast_params {
    float t_min, t_max;     /* the parameter range of a hit */
    float eps;              /* hit threshold on sdf * s, world units */
    float relax;            /* step = relax * dist */
    int32_t max_steps;      /* samples per (ray, object) pair */
} dsp_raycast_params;
void dsp_raycast_params_default(dsp_raycast_params* p);
int dsp_map_raycast(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* origins, const float* dirs, int64_t n_rays,
                    const dsp_raycast_params* params, int32_t flags, int32_t* obj, float* t, float* dist, int32_t* status, float* normal);
/* Counts of the last dsp_map_raycast on this handle: counts6 = {(ray, object) pairs, decoder rows of the march, its tiles, rounds that
 * decoded a row (summed over the passes), passes, exhausted pairs}.  The normals' rows are not counted.  Rows, tiles, rounds and exhausted
 * pairs are a function of the inputs and of the pass cut (a pass retires pairs behind the hits of the passes before it); the outputs are not. */
int dsp_map_raycast_last_stats(dsp_handle* h, int64_t* counts6);
/* Host only, no handle: csrc/raycast_math.h on arrays.  dsp_debug_raycast_check: DSP_E_ARG for params dsp_map_raycast refuses.
 * dsp_debug_raycast_segments: the map as dsp_debug_query_invert returns it (rt_ow, scale; a NaN scale stands for an object that is never
 * hit) and n_rays rays -> is_void (n_rays bytes) and per pair, object major (n_obj x n_rays): exists (bytes), t0, t1, o_o and d_o (x 3);
 * any output may be NULL; the pairs of a void ray read 0.  dsp_debug_raycast_step: n samples (t, t1, sdf, s) -> decision (0 hit, 1 miss
 * on a NaN, 2 advance, 3 exit), dist and the next parameter (t itself for a hit or a NaN). */
int dsp_debug_raycast_check(const dsp_raycast_params* params);
int dsp_debug_raycast_segments(int64_t n_obj, const float* rt_ow, const float* scale, int64_t n_rays, const float* origins, const float* dirs, float t_min,
                               float t_max, unsigned char* is_void, unsigned char* exists, float* t0, float* t1, float* o_o, float* d_o);
int dsp_debug_raycast_step(int64_t n, const float* t, const float* t1, const float* sdf, const float* s, const dsp_raycast_params* params,
                           int32_t* decision, float* dist, float* t_next);

/* ---- map alignment: where is the sensor, given points in its frame and the map?  Batched SE(3) Gauss-Newton ---------------------------
 * n_hyp initial sensor-to-world poses (hypotheses: a relocaliser's seeds, the yaw alternatives of the mono path) are refined against the
 * map's decoded surfaces.  All hypotheses share the n_pts sensor-frame points and their optional weights (NULL = ones) and are
 * independent of each other: a call with n_hyp hypotheses returns what n_hyp calls with one would, byte for byte.
 * One evaluation of a hypothesis at pose T: p_w = T p_s (T's [R | t] rounded once to fp32, nested fmaf); the map query of p_w gives the
 * winning object and d = sdf s; the winner's gradient rotated to the world and multiplied by s gives g_w (NOT normalised: it is the
 * jacobian of d).  A point is valid if p_w is finite and its weight > 0; used if it is valid, has a winner, d and g_w are finite and
 * |d| <= max_dist.  Cost: the truncated Huber F = sum w rho~ / sum_valid w, rho(d) = d^2 for |d| <= huber, else huber (2 |d| - huber);
 * a valid point that is not used contributes the constant rho(max_dist), so costs at different poses are comparable.  System, fp64:
 * J = [g_w, p_w x g_w] for the left perturbation T <- exp(xi) T, xi = [v, omega]; H = sum w wh J J^T, b = -sum w wh J d with the IRLS
 * weight wh = 1 for |d| <= huber, else huber / |d|.  The sums are one written tree (csrc/align_math.h), the same bits whatever the
 * passes, chunks or grid; no float atomics.  Step, host fp64: Cholesky of H + (damp + lambda) I, T_trial = exp_se3(xi) T.
 * Loop, by the conventions of dsp_batch_step_control: `iterations` is the number of evaluations (1 = evaluate only); at most
 * iterations - 1 steps are made and the state returned is the best EVALUATED one, with the record of that state.  Step control all zero
 * = off: every trial is accepted (plain damped Gauss-Newton, lambda = 0), and a trial with fewer than min_points used points or a failed
 * factorisation ends the hypothesis with that status at that state.  With step control on, the rule of dsp_debug_step_rule decides on F;
 * a rejected trial solves the saved system again with the larger lambda; a trial without support is a rejection; a factorisation that
 * fails raises lambda like a rejection and is repeated (DSP_ALIGN_SINGULAR once lambda_max fails too); a FIRST evaluation without
 * support ends the hypothesis.  Convergence is tested on the solved step: max |v| < trans_tol and max |omega| < rot_tol (strict: 0
 * stops nothing) gives DSP_ALIGN_CONVERGED and no step.  A hypothesis that has ended is never evaluated again and costs no decoder rows.
 *
 * dsp_map_align: the map as dsp_map_query takes and checks it; pts_sensor n_pts x 3; weights NULL or n_pts (finite, >= 0);
 * t_world_sensor0 n_hyp x 16 doubles, row-major 4 x 4, rigid.  Outputs: t_world_sensor n_hyp x 16 doubles; record n_hyp x
 * DSP_ALIGN_RECORD doubles {status, evaluations, accepted steps, cost at the first state, cost at the returned state, used points, sum of
 * valid weights, lambda, H 6 x 6 (undamped: the information matrix of xi at the returned state), b 6}; obj / dist (optional, both or
 * neither, n_hyp x n_pts): the query's answer per point at the returned state; trace (optional, n_hyp x iterations x DSP_ALIGN_TRACE
 * doubles, zero where nothing was evaluated) per evaluation {pose evaluated 16, decision (1 accepted, 2 rejected), cost, lambda behind
 * the decision, used points, H 21 (upper triangle, row-major), b 6, xi solved 6}.  n_hyp, n_pts and n_obj may be 0; with no points or
 * no objects every hypothesis returns DSP_ALIGN_NO_SUPPORT with its input pose.  DSP_E_ARG: a map dsp_map_query refuses; an initial pose
 * that is not finite, has a bottom row other than 0 0 0 1, whose linear part is off a rotation by more than 1e-4 or whose scale is off 1
 * by more than 1e-4; a negative or non-finite weight; n_hyp x n_pts > 2^31 - 1; params that dsp_align_params_default's comment refuses. */
#define DSP_ALIGN_OK 0           /* the iterations ran out */
#define DSP_ALIGN_CONVERGED 1
#define DSP_ALIGN_NO_SUPPORT 2   /* fewer than min_points used points */
#define DSP_ALIGN_SINGULAR 3     /* a pivot of the Cholesky factorisation was not positive or not finite */
#define DSP_ALIGN_RECORD 50
#define DSP_ALIGN_TRACE 53
typedef struct dsp_align_params {
    int32_t iterations;          /* evaluations, >= 1 */
    int32_t min_points;          /* >= 6 */
    double max_dist;             /* the gate on |d|, world units; finite */
    double huber;                /* 0 < huber <= max_dist */
    double damp;                 /* >= 0, finite: added to H's diagonal in every solve */
    double trans_tol, rot_tol;   /* >= 0, not NaN */
    double lambda0, up, down, lambda_min, lambda_max;   /* all zero = off; otherwise dsp_batch_step_control's checks */
} dsp_align_params;
/* 10 evaluations, min_points 6, max_dist 0.3, huber 0.05, damp 0, both tolerances 1e-6, step control off */
void dsp_align_params_default(dsp_align_params* p);
int dsp_map_align(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts_sensor, const float* weights,
                  int64_t n_pts, const double* t_world_sensor0, int64_t n_hyp, const dsp_align_params* params, double* t_world_sensor,
                  double* record, int32_t* obj, float* dist, double* trace);
/* Counts of the last dsp_map_align on this handle: counts5 = {candidate rows, decoder tiles, chunks, point passes (all summed over its
 * evaluations), device evaluations (one per iteration in which any hypothesis was live)}. */
int dsp_map_align_last_stats(dsp_handle* h, int64_t* counts5);
/* Host only, no handle: csrc/align_math.h on arrays.  dsp_debug_align_rows: n points' p_w (n x 3), obj, d, g_w (n x 3) and w (NULL =
 * ones) -> sums30 = {H 21, b 6, sum w rho~, sum_valid w, used points} through the written tree.  dsp_debug_align_step: H (6 x 6, the
 * upper triangle is read), b, damp, lambda, T (16) -> status (DSP_ALIGN_OK or DSP_ALIGN_SINGULAR), xi (6) and T_trial = exp_se3(xi) T
 * (16; both untouched when singular).  dsp_debug_align_check: DSP_E_ARG for params, initial poses or weights (NULL = none) that
 * dsp_map_align refuses, by the very checks it makes before it touches the device. */
int dsp_debug_align_check(const dsp_align_params* params, const double* t_world_sensor0, int64_t n_hyp, const float* weights, int64_t n_pts);
int dsp_debug_align_rows(int64_t n, const float* pts_world, const int32_t* obj, const float* dist, const float* grad_world, const float* weights,
                         double huber, double max_dist, double* sums30);
int dsp_debug_align_step(const double* H36, const double* b6, double damp, double lambda, const double* t16, int32_t* status, double* xi6,
                         double* t_trial16);

/* ---- ray alignment: where is the sensor, given the depths it measured along its rays?  Projective Gauss-Newton against the cast map ----
 * dsp_map_align answers for a cloud already cut down to object points, and pairs a point with the nearest surface among the unit spheres
 * that contain it: a point outside every sphere has no residual, occlusion between objects is ignored, and a pose that puts a map object
 * between the sensor and what it measured costs nothing.  dsp_map_align_rays pairs every observation with the surface its RAY sees.
 * Observation i is the measured end point pts_sensor[i] of the ray that runs from origins_sensor[i] (NULL: the sensor origin 0 0 0)
 * through it, both in the sensor frame.  The map, the hypotheses, weights, record, trace, statuses, loop, step control, convergence rule
 * and step are dsp_map_align's; hypotheses are independent, byte for byte, and one that has ended costs no decoder rows.
 * One evaluation of a hypothesis at pose T (csrc/align_rays_math.h, one correctly rounded fp32 operation at a time):
 *   p_w = T p_s, o_w = T o_s as dsp_map_align transforms points; dir = p_w - o_w; u = dir / |dir|, len = |dir| is the observed depth.  A
 *   ray with a number that is not finite or with p_s == o_s is void.
 *   The rays (o_w, dir) of ALL live hypotheses go through dsp_map_raycast's pipeline in one cast with `raycast`: obj, t_hit, the hit
 *   sample's dist_hit = sdf s and the status per ray; the winners' hit samples go through the decoder's jacobian form, and g_w is the
 *   gradient rotated to the world and multiplied by s (NOT normalised).
 *   gap = len - t_hit;  d = fmaf(g_w . u, gap, dist_hit): the first-order signed distance from the measured point to the surface patch its
 *   ray sees.  It removes the marcher's eps staircase to first order; a residual pose error of second order in eps and gap remains (about
 *   half of eps in translation on the project's test scene: profiles/map_align_rays.md), so cast with a smaller eps for a finer pose.
 *   The observation is matched when status == DSP_RAYCAST_HIT (UNDECIDED is not), gap is finite and |gap| <= max_gap (compared in fp64).
 *   A matched observation enters dsp_map_align's rows with (p_w, obj, d, g_w): J = [g_w, p_w x g_w], because the measured point moves with
 *   the sensor and the patch stays.  An unmatched one whose p_w is finite and whose weight is > 0 contributes w rho(max_dist), like a
 *   valid point that is not used: seeing through a map object, or at a surface far from the measured depth, costs something.
 * max_gap >= max_dist, not NaN; +inf = no gate.  Without the gate, background rays reach the system through grazing hits, where
 * g_w . u -> 0 makes d small whatever the depth mismatch.  dsp_align_rays_default_max_gap: 2 max_dist (the sweep in the profile).
 * Outputs as dsp_map_align's, and per observation at the RETURNED state (optional, all four or none, n_hyp x n_rays): obj (the matched
 * object, -1 for unmatched), dist (d; +inf without a winner), t_hit and status of the cast.  With no rays or no objects every hypothesis
 * returns DSP_ALIGN_NO_SUPPORT with its input pose (-1, +inf, +inf, MISS).  DSP_E_ARG, before the device is touched: everything
 * dsp_map_align and dsp_map_raycast refuse; max_gap < max_dist or NaN; n_hyp x n_rays > 2^31 - 1; n_obj x ceil(n_hyp n_rays / 64) pair
 * counts or the objects' code biases beyond dsp_map_raycast's budgets ("split the request": hypotheses are not grouped). */
double dsp_align_rays_default_max_gap(const dsp_align_params* params);
int dsp_map_align_rays(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts_sensor, const float* origins_sensor,
                       const float* weights, int64_t n_rays, const double* t_world_sensor0, int64_t n_hyp, const dsp_align_params* params,
                       const dsp_raycast_params* raycast, double max_gap, double* t_world_sensor, double* record, int32_t* obj, float* dist, float* t_hit,
                       int32_t* status, double* trace);
/* Counts of the last dsp_map_align_rays on this handle: counts7 = dsp_map_raycast_last_stats' six summed over its evaluations (pairs,
 * decoder rows of the march, tiles, rounds, passes, exhausted pairs), device evaluations. */
int dsp_map_align_rays_last_stats(dsp_handle* h, int64_t* counts7);
/* Host only, no handle: csrc/align_rays_math.h on arrays.  dsp_debug_align_ray_rows: n rays' o_w and p_w (n x 3 each), the cast's answers
 * (obj, t_hit, dist_hit, status), g_w (n x 3, read where obj >= 0), w (NULL = ones) and the three gates -> obj_row, d (n each) and sums30
 * as dsp_debug_align_rows.  dsp_debug_align_rays_check: DSP_E_ARG for what dsp_map_align_rays refuses before it touches the device, the
 * map's poses and codes excepted (n_obj objects are assumed valid). */
int dsp_debug_align_ray_rows(int64_t n, const float* origins_world, const float* pts_world, const int32_t* obj, const float* t_hit, const float* dist_hit,
                             const int32_t* status, const float* grad_world, const float* weights, double huber, double max_dist, double max_gap,
                             int32_t* obj_row, float* d, double* sums30);
int dsp_debug_align_rays_check(const dsp_align_params* params, const dsp_raycast_params* raycast, double max_gap, const double* t_world_sensor0,
                               int64_t n_hyp, const float* weights, int64_t n_rays, int64_t n_obj);

/* ---- object refinement: where are the OBJECTS, given depth rays from known sensor poses?  One SE(3) correction per map object ----------
 * The calls above treat the map as fixed and solve for the sensor.  dsp_map_align_objects takes the sensor as known (tracking, bundle
 * adjustment) and moves the objects to where the depth says they are.  Observation i is the measured end point pts_world[i] of the ray
 * that runs from origins_world[i] through it, both in the WORLD frame: the caller applies the known sensor poses (map_objects.pixel_rays'
 * convention), origins are required, and the rays of several frames or sensors are simply concatenated.  weights NULL = ones, finite and
 * >= 0.  refine: NULL = all ones, or n_obj bytes; an object with 0 is never moved and never evaluated -- it still occludes.
 * State: one fp64 rigid correction C_k per object, identity at the start; object k stands at T_k = C_k T_k0 (composed in fp64 from the fp32
 * input, every entry rounded ONCE to fp32; csrc/align_objects_math.h).  One evaluation: the object table comes from the composed poses
 * through dsp_map_query's inversion; ALL rays go through ONE cast of the map, evaluated objects at their trial pose, every other object at
 * its accepted pose; gradient, residual, the max_gap gate and the match are dsp_map_align_rays' verbatim.  Ray i belongs to the object
 * the cast names as its winner, matched or not (an unmatched ray costs that object w rho(max_dist)); a ray without a winner belongs to no
 * object.  The sums of object k run over its winners in ascending ray order through dsp_map_align's written tree over the LIST (the same
 * bits whatever the passes, chunks or grid; no float atomics).  The object moves and the measured point stays, C <- exp(xi) C, so the
 * jacobian is -[g_w, p_w x g_w]: H is dsp_map_align's, b its negation.  Loop, statuses, min_points, damping, step control, tolerances and
 * step are dsp_map_align's with "hypothesis" = object and pose = C_k.  Objects are coupled only through occlusion; each decides on its own
 * cost F_k = sum cost / sum w over that evaluation's winners.  LIMIT: the winner set changes between evaluations, so F_k compares means
 * over different sets of rays.  No ray is ever charged to an object that it does not see.  A composed pose that the map's inversion
 * refuses ends its object with DSP_ALIGN_SINGULAR at its accepted state.  The jacobian rows of winners of objects that are not evaluated
 * are decoded and ignored (the winners' chunk plan is the cast's).
 * Outputs: t_world_obj_out n_obj x 16 floats, the composed poses at the returned states (an object whose correction is still the identity
 * -- not refined, without support, or never stepped -- returns its input bytes); correction n_obj x 16 doubles; record n_obj x
 * DSP_ALIGN_RECORD as dsp_map_align's, H being the information of the left perturbation of C_k (an object that is not refined: status
 * DSP_ALIGN_OK, 0 evaluations); per ray, optional, all four or none (n_rays each): obj, dist, t_hit, status as dsp_map_align_rays reports
 * them, from ONE extra evaluation of the returned map with every object at its returned pose (run only when asked for, and counted in
 * the stats); trace optional, n_obj x iterations x DSP_ALIGN_TRACE, the pose traced being C_k.  n_obj and n_rays may be 0: no device is
 * touched and every refined object returns DSP_ALIGN_NO_SUPPORT with its input pose.  DSP_E_ARG, before the device is touched: a map
 * dsp_map_query refuses; params dsp_map_align refuses; a raycast dsp_map_raycast refuses; max_gap < max_dist or NaN; NULL origins with
 * n_rays > 0; a negative or non-finite weight; n_rays > 2^31 - 1; n_obj x ceil(n_rays / 64) pair counts or the objects' code biases beyond
 * dsp_map_raycast's budgets.
 * Code refinement is dsp_map_align_shapes, below.  Out of scope: scale; a world-axis mask on the degrees of freedom (yaw only); a prior on
 * the correction; the conversion of H into an edge of dsp_pg_edge_information. */
int dsp_map_align_objects(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts_world, const float* origins_world,
                          const float* weights, int64_t n_rays, const unsigned char* refine, const dsp_align_params* params,
                          const dsp_raycast_params* raycast, double max_gap, float* t_world_obj_out, double* correction, double* record, int32_t* obj,
                          float* dist, float* t_hit, int32_t* status, double* trace);
/* Counts of the last dsp_map_align_objects on this handle, laid out as dsp_map_align_rays_last_stats'; the evaluation behind the per-ray
 * outputs is included. */
int dsp_map_align_objects_last_stats(dsp_handle* h, int64_t* counts7);
/* Host only, no handle: csrc/align_objects_math.h on arrays.  dsp_debug_align_objects_rows: n rays' p_w (n x 3), the cast's winner, the
 * matched object (-1: unmatched), d, g_w (n x 3, read where matched) and w (NULL = ones) -> sums, n_obj x 30 as dsp_debug_align_rows',
 * per object over its winners through the written tree, b already negated.  dsp_debug_align_objects_compose: n corrections (16 doubles)
 * and n fp32 poses -> the composed fp32 poses.  dsp_debug_align_objects_check: DSP_E_ARG for what dsp_map_align_objects refuses before it
 * touches the device, the map's poses and codes excepted; origins_world is only tested against NULL. */
int dsp_debug_align_objects_rows(int64_t n, const float* pts_world, const int32_t* winner, const int32_t* obj_row, const float* d, const float* grad_world,
                                 const float* weights, int64_t n_obj, double huber, double max_dist, double* sums);
int dsp_debug_align_objects_compose(int64_t n, const double* correction, const float* t_world_obj, float* t_world_obj_out);
int dsp_debug_align_objects_check(const dsp_align_params* params, const dsp_raycast_params* raycast, double max_gap, const float* origins_world,
                                  const float* weights, int64_t n_rays, int64_t n_obj);

/* ---- shape refinement: what SHAPE do the objects have, given depth rays from known sensor poses?  One 70-dim system per map object ----
 * dsp_map_align_objects moves the map's objects; dsp_map_align_shapes refits their shape codes -- and, if asked, their poses with them --
 * against the same world-frame depth rays, inside the map: one cast with occlusion between the objects, a ray charged only to the object
 * it sees.  Observations, weights, refine, the cast, gradient, residual d, the max_gap match and the owner rule are
 * dsp_map_align_objects' verbatim.  Unknowns per object: x = [v 3, omega 3, dz 64] (DSP_SHAPES_DIM); the pose part is
 * dsp_map_align_objects' C_k <- exp(xi) C_k, the code part is additive on an fp64 code z_k that starts at the input code and is rounded
 * ONCE to fp32 for every evaluation, where the object's code bias is recomputed from it.  Jacobian row of a used ray:
 * J = [-g_w, -(p_w x g_w), s dsdf/dcode] with the code derivatives of the winner's jacobian row at the hit sample and the winner's scale
 * s (one fp32 multiply): the dependence of t_hit and g_w on the code is dropped, the first-order treatment the pose part has too.
 * H = sum w wh J J^T (70 x 70), b = -sum w wh J d, cost, sum of valid weights W and used count as dsp_map_align's.  The sums of an object
 * run over its winners in ascending ray order, in blocks of 128 list positions, rows added one at a time in ascending order, blocks in
 * ascending order (csrc/align_shapes_math.h): the same bits whatever the passes, chunks or grid; no float atomics.
 * Step, host fp64, on the MEAN system A = H / W, g = b / W:  A_cc += code_reg + code_anchor and g_c -= code_reg z_c + code_anchor (z_c -
 * z0_c) on the code entries (z0: the input code), A_ii += damp + lambda on all 70, then the entries that are not asked for (`unknowns`)
 * and the code entries beyond a 32-D decoder's length are pinned (dx exactly 0), then a 70-dim Cholesky.  The cost that step control
 * decides on, and that the record reports, is F = sum cost / W + code_reg |z|^2 + code_anchor |z - z0|^2.  code_reg is the reference
 * optimiser's code regulariser; with few views most code directions are unobserved and damp (default 1e-4 here, on the mean system) is
 * what conditions them.  Loop, statuses, min_points, step control: dsp_map_align_objects'; an object converges when max |v| < trans_tol,
 * max |omega| < rot_tol and max |dz| < code_tol (strict).  A trial code or code bias that is not finite, or a trial pose the map's
 * inversion refuses, ends the object with DSP_ALIGN_SINGULAR at its accepted state.
 * Outputs: t_world_obj_out and correction as dsp_map_align_objects'; codes_out n_obj x 64 floats; record n_obj x DSP_SHAPES_RECORD doubles
 * {dsp_map_align's first 8, H 70 x 70 (raw sums, undamped, full), b 70}; the per-ray four from one extra evaluation of the returned map;
 * trace optional, n_obj x iterations x DSP_SHAPES_TRACE doubles {C_k evaluated 16, code evaluated 64 (fp64), decision, cost, lambda, used
 * rays, dx solved 70}.  An object that is not refined or never stepped returns its input pose and code bytes; with unknowns ==
 * DSP_SHAPES_POSE every code returns its input bytes; with unknowns == DSP_SHAPES_CODE every pose returns its input bytes and every
 * correction is the identity.  DSP_E_ARG: everything dsp_map_align_objects refuses; unknowns 0 or with unknown bits; code_reg,
 * code_anchor or code_tol negative or not finite.
 * Out of scope: scale (Sim(3)); coupling between objects beyond occlusion; a prior from dsp_batch_posterior records; the 16-bit decoders. */
#define DSP_SHAPES_CODE 1
#define DSP_SHAPES_POSE 2
#define DSP_SHAPES_DIM 70
#define DSP_SHAPES_RECORD (8 + 70 * 70 + 70)
#define DSP_SHAPES_TRACE (16 + 64 + 4 + 70)
typedef struct dsp_shapes_params {
    int32_t unknowns;                        /* DSP_SHAPES_CODE, DSP_SHAPES_POSE or both */
    double code_reg, code_anchor, code_tol;  /* >= 0, finite */
} dsp_shapes_params;
/* dsp_align_params_default's values but damp 1e-4 (on the mean system); code only, code_reg 0, code_anchor 0, code_tol 1e-6.  Either may
 * be NULL. */
void dsp_shapes_params_default(dsp_align_params* params, dsp_shapes_params* shapes);
int dsp_map_align_shapes(dsp_handle* h, const float* t_world_obj, const float* codes, int64_t n_obj, const float* pts_world, const float* origins_world,
                         const float* weights, int64_t n_rays, const unsigned char* refine, const dsp_align_params* params,
                         const dsp_shapes_params* shapes, const dsp_raycast_params* raycast, double max_gap, float* t_world_obj_out, float* codes_out,
                         double* correction, double* record, int32_t* obj, float* dist, float* t_hit, int32_t* status, double* trace);
/* Counts of the last dsp_map_align_shapes on this handle, laid out as dsp_map_align_objects_last_stats'. */
int dsp_map_align_shapes_last_stats(dsp_handle* h, int64_t* counts7);
/* Host only, no handle: csrc/align_shapes_math.h on arrays.  dsp_debug_align_shapes_rows: dsp_debug_align_objects_rows' inputs and gcode
 * (n x 64: s dsdf/dcode per ray) -> sums, n_obj x 2558 {H 2485 (pairs i <= j, row-major), b 70, cost, sum of valid weights, used rays}.
 * dsp_debug_align_shapes_step: H (70 x 70 raw sums, the upper triangle is read), b, W, the fp64 code z (64), the fp32 input code z0 (64),
 * the decoder's code length (1 .. 64), shapes, damp, lambda and C (16) -> status (DSP_ALIGN_OK or DSP_ALIGN_SINGULAR), dx (70), C_trial
 * (16) and z_trial (64 doubles); all three untouched when singular.  dsp_debug_align_shapes_check: DSP_E_ARG for what
 * dsp_map_align_shapes refuses before it touches the device, the map's poses and codes excepted. */
int dsp_debug_align_shapes_rows(int64_t n, const float* pts_world, const int32_t* winner, const int32_t* obj_row, const float* d, const float* grad_world,
                                const float* gcode, const float* weights, int64_t n_obj, double huber, double max_dist, double* sums);
int dsp_debug_align_shapes_step(const double* H4900, const double* b70, double W, const double* code, const float* code0, int32_t code_len,
                                const dsp_shapes_params* shapes, double damp, double lambda, const double* c16, int32_t* status, double* dx70,
                                double* c_trial16, double* code_trial64);
int dsp_debug_align_shapes_check(const dsp_align_params* params, const dsp_shapes_params* shapes, const dsp_raycast_params* raycast, double max_gap,
                                 const float* origins_world, const float* weights, int64_t n_rays, int64_t n_obj);

/* ---- device-resident batches (bench / steady-state serving: inputs stay in HBM between runs) --- */
int dsp_batch_create(dsp_handle* h, const dsp_gn_params* prm, int32_t n_objects, const int64_t* pts_off,
                     const float* pts, const int64_t* ray_off, const float* rays, const int64_t* depth_off,
                     const float* depth, const float* t_cam_obj_in, const float* codes_in, dsp_batch** out);
/* The pose-only batch of dsp_estimate_pose_batch (same inputs), device-resident: dsp_batch_run / _results / _set_iterations (the
 * pose-only iteration count) / _enable_trace / _trace / _debug_start_state / _destroy work on it; dsp_batch_results' t_cam_obj_out is
 * dsp_estimate_pose_batch's t_co_se3_out, bit for bit; its codes are the input codes and its loss is 0. */
int dsp_batch_create_pose(dsp_handle* h, const dsp_gn_params* prm, int32_t n_objects, const int64_t* pts_off, const float* pts,
                          const float* t_co_se3_in, const float* scale, const float* codes, dsp_batch** out);
/* The batch of dsp_reconstruct_multiview (same inputs), device-resident.  dsp_batch_run / _results (per object) / _stats / the setters /
 * _enable_trace / _trace / _destroy and both gathers work on it; dsp_batch_set_compute refuses the low-precision mode (DSP_E_ARG).
 * dsp_batch_debug_start_state takes t_obj_cam and codes per OBJECT and depths per VIEW (n_views x 64); dsp_batch_debug_depth_schedule and
 * dsp_batch_debug_samples count VIEWS where they say objects.  A prepass-guard trip on any view re-runs the whole object. */
int dsp_batch_create_multiview(dsp_handle* h, const dsp_gn_params* prm, int32_t n_objects, const int64_t* view_off, const float* t_ref_view,
                               const int64_t* pts_off, const float* pts, const int64_t* ray_off, const float* rays, const int64_t* depth_off,
                               const float* depth, const float* t_cam_obj_in, const float* codes_in, dsp_batch** out);
int dsp_batch_run(dsp_batch* b);        /* resets the state to the uploaded initial estimate, runs, synchronises */
int dsp_batch_results(dsp_batch* b, float* t_cam_obj_out, float* codes_out, float* loss_out, int32_t* status_out);
int dsp_batch_stats(dsp_batch* b, dsp_stats* out);
/* ---- settings (all optional; results are identical, bit for bit, for every value) ------------------------------------------------------ */
/* Number of front-to-back depth ranges the forward decoder is run in per iteration (exact early ray termination: a ray
 * stops being sampled behind its first solid sample, where the transmittance is exactly 0).  0 = automatic (ten uniform
 * ranges for large batches; otherwise 2-3 per-ray ranges steered by where each ray stopped in the previous iteration); 1 = decode every in-sphere sample like the reference does.
 * With the prepass on these are the ranges of the low-precision kernel; the fp32 kernel then runs once per iteration over the samples the
 * prepass could not classify. */
int dsp_batch_set_ray_passes(dsp_batch* b, int n_passes);
/* Exact low-precision pre-classification of the forward ray samples.  The render term only sees clamp(sdf, -cut_off, cut_off)
 * (reconstruct/loss_utils.py:40-48): occupancy is exactly 0 for sdf >= cut_off and exactly 1 for sdf <= -cut_off.  With the
 * prepass on, every candidate sample is first decoded by an f16 (or bf16) MFMA kernel at 16x the fp32 matrix rate; samples with
 * |sdf_lp| >= cut_off + delta are classified by that value alone, rays stop behind their first certainly-solid sample, and only the
 * samples inside the widened band are decoded by the fp32 kernel (one launch per iteration).  delta must exceed the largest
 * |sdf_lp - sdf_fp32| of the decoder.  The default is calibrated PER DECODER at dsp_create: 6x the largest difference over 32 768 seeded
 * unit-ball points x 2 codes per code magnitude (dsp_prepass_calibration_table), not below 5e-4 (f16) / 3e-3 (bf16); the margin of every
 * object follows the largest entry of its CURRENT code.
 * mode: -1 automatic (f16 when the decoder geometry is supported), DSP_PREPASS_OFF / _F16 / _BF16; delta < 0 = default. */
int dsp_batch_set_prepass(dsp_batch* b, int mode, float delta);
/* The guard is ON by default and costs ~0.3 % more fp32 points: with the prepass on, the fp32 kernel also re-decodes a sample of the
 * samples the prepass classified -- 1/8 of the ring th + delta <= |sdf_lp| < th + 2 delta, where an error between delta and 2 delta would
 * misclassify, 1/512 of everything farther out; a different sample every launch -- and compares EVERY sample it decodes (the whole
 * widened band included) with the prepass value it replaces.  A difference of half the object's margin or more trips the guard:
 * dsp_batch_run then runs the OBJECTS IT TRIPPED ON again with the prepass off and returns those results for them (the healthy objects
 * keep theirs: dsp_stats.prepass_guard_rerun = 1, prepass_guard_objects = how many were re-run); the stand-alone dsp_compute_render_loss
 * re-evaluates the term the same way.  Where the run used the calibrated margins, the handle's margins are raised to 4 x the error seen
 * (at most 0.125; dsp_prepass_reset_guard undoes it); a margin forced through dsp_batch_set_prepass leaves them alone.
 * on = 0 turns the guard off (tests: what an unguarded run would have returned). */
int dsp_batch_set_prepass_guard(dsp_batch* b, int on);
/* HIP events around every decoder launch, i.e. the dsp_stats.ms_mlp_* fields: -1 = automatic (on for batches of more than 16 objects --
 * the bench's roofline needs them; off for latency-sized batches, where an event record between two kernels is a queue packet of its own),
 * 0 = off, 1 = on.  Launch COUNTS and ms_total are filled either way. */
int dsp_batch_set_kernel_timing(dsp_batch* b, int mode);
/* OPT-IN, NON-PARITY fast path (BASELINE.json north_star: "fp32/bf16 GEMMs"; SURVEY.md 8(d): "optional non-parity fast path, reported
 * separately").  DSP_COMPUTE_F32 (default): everything that reaches a result is decoded in fp32 -- the mode every parity statement is about.
 * DSP_COMPUTE_F16 / _BF16: the decoder runs on 16-bit matrix operands with fp32 accumulation everywhere -- the ray samples' sdf come from the
 * 16-bit forward kernel alone (no fp32 re-decode of the band, no guard), the jacobian rows from 16-bit forward + backward kernels
 * (mlp_lpj_kernel.hip); thresholds, scans, the Gram matrices and the fp64 solve are unchanged.  The precision class of the reference's own
 * published runs (PyTorch 1.10 on Ampere multiplied in TF32: 10-bit mantissas, as f16).  How far H, b and the results move:
 * profiles/r06_lp_compute.md, tests/test_gpu_lp_compute.py.  DSP_E_ARG for a decoder geometry other than DeepSDF's (eight hidden layers, the
 * latent_in layer fourth) and for pose-only batches.  A DETECTION-SIZED batch (<= 16 objects whose surface points + band samples fit one round of
 * 16-point tiles over the CUs: SLAM's own per-detection calls) keeps the fp32 latency path with the mode set -- it is faster there (2.89 against
 * 3.40 ms) and exact; one cfg2-size object: 14.0 -> 6.0 ms in the mode (profiles/r06_latency_ab.md). */
int dsp_batch_set_compute(dsp_batch* b, int mode);
/* The iteration count of the following runs (instead of dsp_gn_params.num_iterations / pose_only_iterations given at creation). */
int dsp_batch_set_iterations(dsp_batch* b, int32_t n);
/* The calibration dsp_create made for this decoder at a ZERO code: largest |sdf_lp - sdf_fp32| it measured and the margin it derived
 * (DSP_E_STATE when the decoder's geometry has no prepass kernel); the full table follows. */
int dsp_prepass_calibration(dsp_handle* h, int dtype, float* max_err, float* delta);
/* The whole calibration: the prepass error grows with the hidden activations, hence with the code, so dsp_create measures it with codes
 * drawn uniformly in +-mag on every entry for mag in {0, 0.15, 0.5, 1, 2} (5 entries each: mags, largest error, margin = max(floor,
 * 6 x largest error up to that magnitude), capped at 0.5).  Every object's margin follows the largest entry of its CURRENT code,
 * piecewise linearly through this table, re-evaluated after every Gauss-Newton step.  guard_err: largest error a guard trip on this
 * handle has reported (the margins returned are already raised to 4 x that).  Any pointer may be NULL. */
int dsp_prepass_calibration_table(dsp_handle* h, int dtype, float* mags, float* max_err, float* delta, float* guard_err);
/* Forget what earlier guard trips on this handle have left behind (dsp_prepass_calibration_table: guard_err): the margins return to the
 * decoder's calibration. */
int dsp_prepass_reset_guard(dsp_handle* h);

/* ---- convergence rule (optional; NOT one of the settings above: a run with it returns, per object, the result of a SHORTER run) ------------
 * By default every object runs the batch's iteration count, as the reference does.  With a rule set, the solve step of iteration e (0-based)
 * evaluates in fp64, on the update it has just applied,
 *     sp = max_i |lr dx[i]| over the pose entries (7 for Sim(3); a pose-only batch: 6, and lr = 1 there, optimizer.py:73-74),
 *     sc = max_i |lr dx[P + i]| over the code entries (absent for pose-only batches: code_tol is ignored),
 * and the object has CONVERGED when e + 1 >= min_iterations, sp < pose_tol and sc < code_tol.  Both comparisons are strict: a tolerance of 0
 * stops nothing, a NaN step never passes, +inf switches that half of the rule off.  A converged object keeps the update just applied and is
 * frozen for the rest of the run: the remaining iterations decode, scan and solve nothing for it.  Objects are independent, so an object
 * stopped after n updates returns BIT FOR BIT what a run of n iterations returns for it -- pose, code, status (DSP_OBJ_GOOD) and loss (that of
 * its last linearisation); trace rows of iterations it did not run are zeros.  A multi-view object converges as one, decided on its pooled
 * system.  A pose-only object frozen before the update of iteration 4 keeps all its points (the inlier filter never sees it, as in a run of
 * <= 5 iterations).  (0, 0, 1) is the initial state and means off.  DSP_E_ARG (the previous rule stays): a negative or NaN tolerance,
 * min_iterations < 1.  Works on joint, pose-only and multi-view batches, in fp32 and in the low-precision compute mode; the partial re-run
 * after a prepass-guard trip uses the same rule.  The one-shot calls (dsp_reconstruct_batch, ...) always run every iteration.
 * (Not named dsp_batch_set_*: that family is the settings above, and ABI 6 fixes its members.) */
int dsp_batch_convergence(dsp_batch* b, float pose_tol, float code_tol, int32_t min_iterations);
/* out[i] (n_objects entries; a multi-view batch: per object, not per view) = Gauss-Newton updates applied to object i in the last run: the
 * iteration count without a rule; for an object that ended DSP_OBJ_FEW_SAMPLES / DSP_OBJ_NAN the updates applied before it failed; for an object
 * left out of the partial re-run after a guard trip, the value of the run that produced its row.  Host data of the run's one read-back: no device
 * access.  DSP_E_STATE before the first run. */
int dsp_batch_iterations_used(dsp_batch* b, int32_t* out);

/* ---- posterior (optional): how well the data determined each object's returned pose and code ----------------------------------------------
 * With level > 0, the run is followed by ONE more linearisation at each object's final state x* = (T_oc, z), done exactly as an iteration of
 * the run linearises there (same sampling, depth samples derived from the pose, selection rules, Huber weights, prepass, guard and launch
 * forms; in the low-precision compute mode, in that mode).  Unknowns are ordered as in H: [v(3), w(3), sigma | code(64)].
 *     Lambda = w_s G_s + w_r G_r + k3 I_code + k4 J_rot J_rot^T     (fp64, assembled as the solve step assembles H, WITHOUT the damping:
 *                                                                    no + I_7, no + s_damp -- damping is step control, not information)
 *     g      = the solve step's right-hand side b
 *     DSP_POSTERIOR_MEAN: w_s = k2 / M, w_r = k1 / K (the reference's objective);  DSP_POSTERIOR_SUM: w_s = k2, w_r = k1 (sums of squares:
 *     information grows with the number of observations -- what a pose graph wants).  The priors are the same in both.
 * Code slots beyond the decoder's code length are not unknowns (outputs 0).  Pose-only batches: Lambda = J6^T J6 w over the points alive at
 * the end of the run (after the inlier filter if it ran), w = 1 / n_alive or 1; no 1e-2 I.  Multi-view objects: the pooled system.
 * Per OBJECT (multi-view: per object, not per view), float64, row-major, symmetric bit for bit:
 *     status     DSP_POSTERIOR_OK; _NONE: the object did not end the run good, or the linearisation at x* failed by the reference's rules
 *                (< 10 in-sphere samples, K == 0, NaN); _SINGULAR: a pivot of the pivot-free fp64 elimination was not greater than
 *                16 FLT_EPSILON times its own original diagonal entry (round-off of the fp32 Gram chains)
 *     info_pose  P x P (P = 7, pose-only 6): the pose's marginal information, Lambda_pp - Lambda_pc Lambda_cc^-1 Lambda_cp (pose-only: Lambda,
 *                filled also when singular)
 *     cov_pose   P x P: its inverse, (Lambda^-1)_pp;  var_code 64: diag((Lambda^-1)_cc).  Zeros when singular, for pose-only (var_code) and unused slots
 *     loss       k1 L_render + k2 L_sdf AT x*, in the solve step's float32 arithmetic (dsp_batch_results' loss is one update older)
 *     M, V, K    the counts the linearisation used (pose-only: M = points alive)
 *     level 2:   Lambda 71 x 71, g 71, and the state: t_obj_cam 16, code 64, depths 64 (float32; multi-view: the reference view's)
 * dsp_batch_results, _iterations_used, _trace and the packed rows are bit for bit what they are with the posterior off: the pass parks and
 * restores every status word (objects frozen by the convergence rule take part as good ones), writes no loss, iteration count or trace row,
 * and a failure inside it is DSP_POSTERIOR_NONE, not a changed result status.  The prepass guard works in the pass as in any iteration.
 * Level 1 costs ~1.3 KB per object in the run's one read-back, level 2 ~42 KB.  level 0 (initial) = off.  DSP_E_ARG: another level or
 * weights value (the previous setting stays).  The one-shot calls have no posterior.  (Not named dsp_batch_set_*: see dsp_batch_convergence.) */
#define DSP_POSTERIOR_MEAN 0
#define DSP_POSTERIOR_SUM 1
#define DSP_POSTERIOR_OK 0
#define DSP_POSTERIOR_NONE 1
#define DSP_POSTERIOR_SINGULAR 2
int dsp_batch_posterior(dsp_batch* b, int level /* 0 off (initial), 1, 2 */, int weights);
/* The records of the last run (host data of its read-back: no device access); an object left out of the partial re-run after a guard trip
 *  keeps its record like its result row.  Any pointer may be NULL.  DSP_E_STATE when the LAST run was not made with the posterior on (no run yet, or
 * level 0: records of an earlier run are not handed out beside newer result rows), and for a non-NULL level-2 pointer when it was at level 1. */
int dsp_batch_posterior_fetch(dsp_batch* b, int32_t* status, double* info_pose, double* cov_pose, double* var_code, float* loss, int64_t* M,
                              int64_t* V, int64_t* K, double* Lambda, double* g, float* t_obj_cam, float* code, float* depths);

/* ---- Gaussian prior on pose and code (optional): fuse an earlier estimate into a run -------------------------------------------------------
 * Information form.  Unknowns are ordered as in H: [v(3), w(3), sigma | code(64)]; P = 7 for joint and multi-view batches, P = 6 (no code
 * block) for pose-only batches.  Per OBJECT (multi-view: per object, not per view) the caller gives
 *     t_obj_cam0  T0, 4 x 4 camera -> object -- the posterior record's t_obj_cam field (a pose-only batch: with the scale in it, as
 *                 dsp_batch_debug_start_state takes it).  Both T0 and the state are read as affine maps: bottom rows taken as [0 0 0 1]
 *     code0       z0, 64 floats (ignored, may be NULL, for pose-only batches)
 *     Lambda      Lp, n x n float64, row-major, symmetric bit for bit; n = 71 (slots beyond the decoder's code length all zero), pose-only n = 6
 * At the state (T_oc, z) of an iteration the prior's residual is
 *     e_p = Log(T_oc T0^-1)    in fp64 from the two fp32 matrices: the logarithm of the STANDARD Sim(3) exponential,
 *                              hat(xi) = [[w^ + sigma I, v], [0, 0]], translation solved from V v = t with V = int_0^1 exp(a (sigma I + w^)) da.
 *                              NOT the inverse of the reference's exp_sim3 (loss_utils.py:188-233), whose `c = 0. if s <= eps` quirk has none.
 *                              Closed forms for theta >= 1/4, series in theta^2 and sigma below (csrc/prior_math.h).  Pose-only: the same
 *                              logarithm with the sigma entry dropped (both matrices carry the same scale).
 *     e_c = z - z0
 * linearised for the update T_oc <- exp(dx) T_oc by the BCH series of the inverse left jacobian,
 *     J_p = I - 1/2 ad(e_p) + 1/12 ad(e_p)^2,   ad([v, w, s]) = [[w^ + s I, v^, -v], [0, w^, 0], [0, 0, 0]]   (pose-only: top-left 6 x 6, s = 0)
 *     J   = blkdiag(J_p, I_code)
 * -- signs confirmed by finite differences of Log(Exp(d) Exp(e)) in fp64 (tests/test_prior_host.py); the truncation error is fourth order in
 * |e|.  Every iteration adds, in fp64 and in a fixed summation order, before the solve
 *     H += J^T Lp J        behind the k4 term and in FRONT of the damping, so that H = Lambda + damping with the Lambda the posterior reports
 *     b -= J^T Lp e        as the last addition
 * Damping, k3 and k4 are unchanged.  WARNING: a posterior record (dsp_batch_posterior, level 2) already CONTAINS k3 I_code and the k4 rotation
 * term; feeding it back as Lambda while the batch keeps k3 and k4 counts both twice -- subtract them, or run with k3 = k4 = 0.
 * Entries with a row or column beyond P + the decoder's code length are never added (the pinned rows of 32-D codes stay as they are).  An object
 * whose Lambda is all zero has NO prior: it returns the bits of a batch without one, as do its neighbours.  An object whose T_oc T0^-1 has a
 * rotation angle beyond pi - 1e-3 ends DSP_OBJ_NAN: a prior half a turn from the state is a contradiction, not an estimate (the mono flip
 * hypothesis is exactly this case).  The loss of the result row stays k1 L_render + k2 L_sdf.  With the posterior on, Lambda and g of the
 * record include the prior's terms (the relation to a traced H and b holds with the same prior set); a frozen object (dsp_batch_convergence)
 * gets no further prior terms; the partial re-run after a prepass-guard trip keeps the prior; every launch form and the low-precision
 * compute mode take it.  All NULL = off, the initial state: such a run launches exactly the kernels of a batch that never had a prior.
 * DSP_E_ARG (the previous setting stays): some but not all pointers NULL, a non-finite input, det(T0[:3,:3]) <= 0, Lambda not bit-symmetric,
 * a negative diagonal entry, a non-zero entry in a slot beyond the code length (T0 and code0 of an object without a prior are not looked at).
 * The one-shot calls have no prior.  (Not named dsp_batch_set_*: see dsp_batch_convergence.) */
int dsp_batch_prior(dsp_batch* b, const float* t_obj_cam0, const float* code0, const double* Lambda);
/* e (n_objects x (P + 64): e_p | e_c, pose-only: e_c = 0) and chi2 = e^T Lp e (n_objects) at the RETURNED state of the last run -- the
 * Mahalanobis gate "does the new data contradict the old estimate?".  Host data of the run's one read-back.  NaN for an object that did not
 * end good, 0 for an object without a prior; an object left out of the partial re-run after a guard trip keeps its values.  Either pointer
 * may be NULL.  DSP_E_STATE if the last run had no prior. */
int dsp_batch_prior_fetch(dsp_batch* b, double* e, double* chi2);
/* Testing (host only, no device): dsp_batch_prior's argument checks for n_objects objects of a batch kind, and ONE object's prior terms
 * computed on the CPU by the functions the device kernel runs: extra n x (n + 1) = [J^T Lp J | -J^T Lp e], e (P + 64), chi2.  Any output
 * may be NULL.  dsp_debug_prior_terms returns DSP_E_STATE where the device ends the object DSP_OBJ_NAN. */
int dsp_debug_prior_check(int pose_only, int code_len, int n_objects, const float* t_obj_cam0, const float* code0, const double* Lambda);
int dsp_debug_prior_terms(int pose_only, int code_len, const float* t_obj_cam, const float* code, const float* t_obj_cam0, const float* code0,
                          const double* Lambda, double* extra, double* e, double* chi2);

/* ---- Levenberg-Marquardt step control (opt-in, joint batches) ---------------------------------------------------------------------------
 * The reference's iteration has FIXED damping and does not settle: it passes through states several times better than the one it
 * returns (profiles/early_stop.md: the step "wanders").  With step control every iteration's state is a TRIAL that is kept only if it
 * lowers the cost; the rule lives in csrc/step_rule.h, on the device inside the solve step, with no host round trip.  Per object:
 *     cost       F_e = (double) loss_e (float32 k1 L_render + k2 L_sdf, the result row's `loss`), + the prior's chi2 at x_e with a prior on.
 *                The k3 and k4 terms are NOT part of it: the k4 term (1e7) has a zero jacobian on the reference's exact-upright branch, so
 *                the first step tilts freely and a cost with k4 in it rejects the steps that lower the loss.
 *     e == 0     accept; lambda = lambda0
 *     F_e < F_acc (strict, false for NaN): accept; lambda <- lambda * down
 *     otherwise  reject; lambda <- min(max(lambda, lambda_min) * up, lambda_max)
 *     accept     x_acc <- x_e, F_acc <- F_e, and [H | b] as assembled (the reference's damping and a prior's block included) is saved
 *     reject     [H | b] is reloaded from the saved copy, the trial and its linearisation are discarded
 *     step       (S + lambda I) dx = b, lambda added in fp64 to the diagonal of the live unknowns behind everything else (lambda = 0 leaves
 *                the bits of the system alone); the update exp(lr dx) x_acc and everything derived from it follow as without the rule
 * NO step is applied on the run's last iteration, nor on an iteration whose solved step meets the convergence rule (dsp_batch_convergence,
 * evaluated on that step): the object is put back to (frozen at) x_acc.  So a run of N iterations makes N linearisations and at most
 * N - 1 steps, the returned state is the best EVALUATED state, and the returned loss is the loss AT that state (without step control it is
 * one update older).  dsp_batch_iterations_used counts the iterations the object evaluated.  Trace rows record the linearisation at the
 * state the iteration evaluated and the dx it solved (zeros when no step was applied).  A trial state at which the object fails by the
 * reference's rules (< 10 in-sphere samples, K == 0, NaN, singular solve, underivable pose) fails the object as in a run without step
 * control; turning that into a rejection is not built.  The partial re-run after a prepass-guard trip starts the rule afresh for the
 * objects it re-runs.  Works with the convergence rule, the posterior (it linearises at the returned state), the prior and either compute
 * mode.  All five arguments zero = off, the initial state: such a run launches the kernels of a batch that never had it and returns the
 * same bits.  The saved systems (~41 KB per object) are allocated the first time the feature is enabled.
 * DSP_E_ARG (the previous setting stays): a non-finite value (lambda_max may be +inf), lambda0 < 0, up <= 1, down <= 0 or > 1,
 * lambda_min <= 0, lambda_max < lambda_min, a pose-only batch (the inlier filter changes the point set at iteration 4: costs are not
 * comparable across it), a multi-view batch.  The one-shot calls have no step control.  (Not named dsp_batch_set_*: see dsp_batch_convergence.) */
int dsp_batch_step_control(dsp_batch* b, double lambda0, double up, double down, double lambda_min, double lambda_max);
/* The last run's decisions: decision 0 not evaluated (failed / frozen / left out), 1 accepted, 2 rejected; cost = F_e; lambda = the value
 * after the decision.  n_iterations x n_objects each (iteration-major), host data of the run's one read-back; any pointer may be NULL.
 * An object left out of the partial re-run after a guard trip keeps its rows.  DSP_E_STATE if the last run had no step control. */
int dsp_batch_step_log(dsp_batch* b, int32_t* decision, double* cost, double* lambda);
/* Testing (host only, no device): the rule of csrc/step_rule.h applied to a cost sequence of n entries (the function the device runs),
 * and dsp_batch_step_control's argument checks (DSP_E_ARG; the all-zero "off" setting is no rule: DSP_E_ARG too).  Outputs may be NULL. */
int dsp_debug_step_rule(int32_t n, const double* cost, double lambda0, double up, double down, double lambda_min, double lambda_max,
                        int32_t* decision, double* lambda);

/* ---- observation report (optional): which observations disagree with the returned state ---------------------------------------------------
 * With the report on, a run evaluates every observation once more at the state it RETURNS (x_acc with step control, the frozen state under
 * the convergence rule) and keeps the values on the device until dsp_batch_report_fetch copies them: a run adds launches, no read-back.
 * The evaluation is the front of the posterior's pass -- shared with it when the posterior is on, run by the report itself otherwise
 * (without the Gram launch, which feeds the posterior alone): same sampling, selection rules, prepass, guard and launch forms as an
 * iteration; status words parked and put back.  dsp_batch_results, _iterations_used, _trace, the step log, posterior records and the
 * prior's residual are bit for bit what they are with the report off.  Off (initial): the run launches the kernels of a batch that never
 * had it.  A MEMBER is what the batch iterates over: an object of a joint or pose-only batch, a VIEW of a multi-view batch (in view_off
 * order, evaluated at T_oc_v).  Arrays are concatenated in member order, exactly as the inputs were given (pts_off / ray_off).
 *   per surface point   pt_sdf     the decoder value at the transformed point: the residual of compute_sdf_loss (loss.py:22-43)
 *                       pt_flags   bit 0: the point is alive -- always set in joint and multi-view batches; a pose-only batch: the inlier
 *                                  filter's mask as the pass (the last evaluation) used it
 *   per ray (foreground rays first, as uploaded; a pose-only batch has none)
 *                       ray_depth     d_u of loss.py:100-114, with 1.1 d_max as the background term
 *                       ray_hit       1 - T_{D-1}: the silhouette probability
 *                       ray_residual  obs - d_u, UNCLIPPED; obs = the uploaded depth of a foreground ray, 1.1 d_max behind them (optimizer.py:126)
 *                       ray_counts    3 per ray: in-sphere samples, band samples (-th < sdf < th), kept samples (de_do > 1e-2: the rows this
 *                                     ray contributed).  The band count is INFORMATIONAL, like dsp_compute_render_loss' m: samples behind a
 *                                     ray's first solid sample are not decoded where early ray termination or the prepass is on (their
 *                                     transmittance is exactly 0: they reach neither d_u, the hit probability nor a kept row), and are not
 *                                     counted in it; with dsp_batch_set_ray_passes(1) and the prepass off it is the reference's.
 *   per member, 8 doubles   M, V, m, K (pose-only: M = points alive, the others 0) | sum_s = sum (w r)^2 over the member's surface rows with the
 *                       weights of get_robust_res(., b2) (a pose-only batch: r^2 over its alive points, as optimizer.py:69-72 has no weights) |
 *                       sum_r = the same over its kept render rows with b1 -- each w r the float32 last column of the row, squared and summed
 *                       in fp64 | the member's status at the pass (DSP_OBJ_*) | 0 (reserved).  A single-view object's
 *                       k2 sum_s / M + k1 sum_r / K is the loss at the returned state; any pooling over views is the caller's.
 * A member that did not end good has NaN in its float rows and sums, zero counts and flags, and its status says why.  A view with fewer
 * than 10 in-sphere samples at that state has no render term (loss.py:73-74): its ray rows are NaN, its ray counts, K, m and sum_r
 * are 0 and its status is DSP_OBJ_FEW_SAMPLES; its surface points, which the pooled system does use, are reported (pt_sdf, flags, M, sum_s).
 * A member left out of the partial re-run after a prepass-guard trip keeps the rows it had, as posterior records do.
 * Works on joint, pose-only and multi-view batches, with the convergence rule, step control, prior and posterior, in either compute mode
 * (the low-precision mode's values are that mode's: no accuracy is claimed for them).  The report arrays (5 B per point, 24 B per ray) come
 * from the handle's pool the first time the report is enabled: DSP_E_NOMEM leaves the report off and the batch usable.  DSP_E_ARG: on
 * outside {0, 1}.  dsp_batch_report_fetch: any pointer may be NULL; DSP_E_STATE if the last run had no report.  The one-shot calls have
 * no report.  (Not named dsp_batch_set_*: see dsp_batch_convergence.) */
int dsp_batch_report(dsp_batch* b, int on);                    /* 0 = off (initial) */
int dsp_batch_report_sizes(dsp_batch* b, int64_t* n_points, int64_t* n_rays, int64_t* n_members);
int dsp_batch_report_fetch(dsp_batch* b, float* pt_sdf, uint8_t* pt_flags, float* ray_depth, float* ray_hit, float* ray_residual,
                           int32_t* ray_counts /* n_rays x 3 */, double* member /* n_members x 8 */);
/* Testing (host only, no device): ONE ray in the scalar statement of the arithmetic (csrc/report_math.h) that the device kernels are built
 * from.  depths, sdf: n_depth entries (2..64); sdf = the value the occupancy scan reads, NaN = the sample is not in the unit sphere.
 * out4 = {d_u, 1 - T_{D-1}, obs - d_u unclipped, the clipped residual of the render rows}; counts3 as ray_counts.  depth_obs is read for a
 * foreground ray only. */
int dsp_debug_report_ray(int32_t n_depth, const float* depths, const float* sdf /* NaN = not in the sphere */, float th, float depth_obs,
                         int is_fg, float* out4, int32_t* counts3);

/* ---- per-observation weights (optional): the input the report's answer can be fed back through ---------------------------------------------
 * pt_w: one float per surface point; ray_w: one float per ray (foreground rays first, as uploaded); both concatenated in MEMBER order, exactly
 * as dsp_batch_report_fetch lays its rows out (dsp_batch_report_sizes gives the lengths).  Either may be NULL = all ones for that kind; both
 * NULL = off (initial): the run launches the kernels of a batch that never had weights and returns the same bits.  A pose-only batch ignores
 * ray_w.  The values are copied to the device (arrays from the handle's pool the first time: DSP_E_NOMEM leaves weights off and the batch
 * usable) and stay set for every following run, a partial re-run after a prepass-guard trip included, until changed.
 * The objective (priors and damping unchanged):
 *   E = k2 sum_p w_p (rho_b2 r_p)^2 / sum_p w_p  +  k1 sum_k w_ray(k) (rho_b1 r_k)^2 / sum_k w_ray(k)
 * p over the surface points (a pose-only batch: the points alive, raw residual), k over the KEPT render rows, each with the weight of its
 * ray: H gets sum w J^T J, b gets -sum w J^T r~, and the divisors M / K (pose-only: the points alive) are replaced by the fp64 sums of the
 * weights, taken in a fixed order; a multi-view object pools both sums over its views.  The device multiplies every row by the correctly
 * rounded float32 square root of its weight.
 * A RAY OF WEIGHT 0 IS ABSENT: not sampled -- nothing in V, m, K, the "< 10 in-sphere samples" rule or the decoder's work -- and its report
 * rows are those of a member without a render term (NaN floats, zero counts).  A point of weight 0 is decoded and contributes a zero row.
 * sum_p w_p == 0 ends the object DSP_OBJ_NAN (as M == 0 does); every ray at 0 is V == 0: DSP_OBJ_FEW_SAMPLES; a view whose weights are all
 * 0 behaves as a view given no observations.  The integer counts of traces, posterior records and report members stay counts.
 * With all weights 1 every result bit equals a run without weights.  Composes with the convergence rule, step control (the cost is the
 * weighted loss), the prior, the posterior (MEAN divides by the weight sums; SUM applies k2 / k1 to the weighted Grams: the weights act as
 * inverse-variance factors) and the report (pt_sdf and ray_* stay raw; sum_s / sum_r become the weighted sums, and the loss identity holds
 * with the weight sums, which the caller forms from its weights, the alive bits and ray_counts[:, 2]), in both compute modes and every
 * launch form.  DSP_E_ARG (previous setting kept): a negative or non-finite weight, a stale token.  The one-shot calls have no weights.
 * (Not named dsp_batch_set_*: see dsp_batch_convergence.) */
int dsp_batch_observation_weights(dsp_batch* b, const float* pt_w, const float* ray_w);
/* Testing (host only, no device): dsp_batch_observation_weights' checks on n_points / n_rays values (NULL = all ones: nothing to check). */
int dsp_debug_observation_weights_check(int64_t n_points, int64_t n_rays, const float* pt_w, const float* ray_w);

/* ---- mask of unknowns (optional): which of an object's pose, scale and code entries a run estimates ------------------------------------------
 * live: n_objects x 71 bytes in H's order [v(3), w(3), sigma | code(64)] (a pose-only batch: n_objects x 6), 1 = live, 0 = frozen; a
 * multi-view batch takes it per OBJECT, not per view.  NULL = every entry live = off (initial): the run launches the kernels of a batch that
 * never had a mask and returns the same bits, and so does a mask of ones.  Entries at or beyond 7 + code_len of a 32-D decoder are not looked
 * at (those slots stay pinned as they are).  The mask is copied to the device (the array comes from the handle's pool the first time:
 * DSP_E_NOMEM leaves the mask off and the batch usable) and stays set for every following run, the partial re-run after a prepass-guard trip
 * included, until changed.
 * Frozen entries are NOT unknowns: the system is conditioned on their current value.  Behind everything else the solve step adds to its
 * system -- data terms, k3, k4, a prior's block, the damping -- row and column i of H of a frozen index i are set to zero, H_ii = 1 and
 * b_i = 0; that is the system the trace records and step control saves, and step control's lambda is not added to a frozen diagonal.  The
 * pivot-free elimination then returns dx_i == 0.0 exactly and gives the live block the arithmetic of the reduced system in the same pivot
 * order ("Mask of unknowns").  A frozen code entry keeps its bits; with every pose entry frozen (7; pose-only 6) the pose update is
 * skipped, so t_obj_cam, the depth samples and everything else derived from the pose keep their bits across iterations.  The update is a
 * left perturbation in the object frame: with w_x and w_z frozen the rotation is a pure yaw and the object's up axis keeps its direction in
 * the camera frame -- the hard form of the k4 prior, which can then be 0.  An object with no live unknown is allowed: its run evaluates and
 * moves nothing, `loss` is the loss at the start state.
 *   convergence rule   a frozen entry's step is 0 and blocks no stop; an object with no live unknown converges at min_iterations
 *   prior              entries of J^T Lp J and -J^T Lp e in a frozen row or column are not added (conditioning); e and chi2 of
 *                      dsp_batch_prior_fetch stay the full residual
 *   posterior          Lambda and g (level 2) have zeros in frozen rows and columns; info_pose is the Schur complement over the LIVE code
 *                      entries on the live pose entries, cov_pose its inverse on that sub-block, zeros elsewhere (no live pose entry: both all
 *                      zero, status DSP_POSTERIOR_OK); var_code is 0 at frozen entries; the singularity rule looks at live pivots only
 * The report, observation weights, the low-precision compute mode, step control and every launch form work as without a mask.  NO decoder or
 * Gram work is skipped for frozen entries: a masked run costs what the plain run costs (skipping the code columns of a code-frozen batch is
 * a possible follow-up).  DSP_E_ARG (the previous mask stays): a value other than 0 or 1, a stale token.  The one-shot calls have no mask.
 * (Not named dsp_batch_set_*: see dsp_batch_convergence.) */
int dsp_batch_unknowns(dsp_batch* b, const uint8_t* live);
/* Testing (host only, no device): dsp_batch_unknowns' argument checks for n_objects objects of a batch kind. */
int dsp_debug_unknowns_check(int pose_only, int code_len, int n_objects, const uint8_t* live);

/* ---- testing: ONE door for the forms the library chooses between by itself-----------------------------------------------------------
 * The launch sequence has several bit-identical forms per stage, chosen from the batch's size.  Tests pin a form to
 * compare it with the one it replaces; an integrator has no reason to.  value: -1 automatic, 0 off, 1 on where applicable, unless noted. */
#define DSP_DBG_MASK_REUSE 1        /* render rows run the backward sweep only, from relu masks the forward launches exported (throughput form: a launch of their own) */
#define DSP_DBG_SPLIT_ROWS 2        /* latency form of the decoder launches: 16-point tiles, a layer's rows split over the four waves */
#define DSP_DBG_TAIL_SPLIT 3        /* the last, at most half-empty round of a 64-point forward launch as 16-point tiles in a launch of its own */
#define DSP_DBG_WAVE_BOOKKEEPING 4  /* per-ray bookkeeping as one wave per ray with running counters (1) instead of count / scan / write launches (0) */
#define DSP_DBG_SPECULATIVE_BAND 5  /* prepass on: unclassified samples go straight into the jacobian launch (no forward launch of their own) */
#define DSP_DBG_MIXED_REUSE 6       /* mask reuse inside the latency form: backward-only tiles in the same launch as the surface points' tiles */
#define DSP_DBG_CLUSTER_TILES 7     /* cluster form of the jacobian launch: four workgroups per 16-point tile (lists of <= 128 tiles); 1 also bypasses the handle's cool-down */
#define DSP_DBG_DIRECT_TILES 8      /* one-object batches: the decoder kernels derive their tile lists themselves */
#define DSP_DBG_PREPASS_TILE 9      /* value = 128 or 64 points per prepass tile, -1 / 0 automatic */
#define DSP_DBG_PREPASS_AUDIT 10    /* value != 0: every run also decodes all in-sphere samples in fp32 and fills dsp_stats.prepass_max_err / _misclassified / _audited */
#define DSP_DBG_LP_SMALL_BATCHES 12 /* 1: the low-precision compute mode also on detection-sized batches (automatic: they keep the fp32 latency path, which is faster there) */
#define DSP_DBG_CLUSTER_FAULT 11    /* value != 0: the following runs' cluster launches lose one workgroup's hand-off (the device-side fallback takes over); 0 also ends the cool-down */
int dsp_batch_set_debug(dsp_batch* b, int key, int value);
/* Forensics: front-to-back ranges with explicit depth-index boundaries: bounds[0] = 0 <= ... <= bounds[n_passes] = num_depth_samples,
 * 1 <= n_passes <= num_depth_samples (DSP_E_ARG otherwise); empty ranges are skipped. */
int dsp_batch_debug_ray_pass_bounds(dsp_batch* b, const int32_t* bounds, int n_passes);
/* Forensics: start the following runs from the given camera->object matrices (n_objects x 16, used as they are -- no
 * inversion, so a recorded state of the reference can be injected bit for bit) and / or codes (n_objects x 64); NULL t_obj_cam returns
 * to the uploaded object->camera estimates.  depths (optional, n_objects x 64, needs t_obj_cam): the FIRST iteration samples the rays at
 * exactly these num_depth_samples depths instead of deriving them from the pose (optimizer.py:120-125) -- the reference derives them in
 * fp32 LAPACK / powf arithmetic that can differ from this library's by 1-2 ulp, which is enough to move samples across the render term's
 * thresholds.  A pose-only batch (dsp_batch_create_pose) takes t_obj_cam only: the camera->object Sim(3) matrix the reference's
 * iteration starts from, scale included (optimizer.py:53-55). */
int dsp_batch_debug_start_state(dsp_batch* b, const float* t_obj_cam, const float* codes, const float* depths);
/* Forensics: iteration e < n_iterations of the following runs samples the rays at depths[(e * n_objects + i) * 64 ..] instead of
 * the depths derived from the pose (n_iterations = 0 turns the schedule off). */
int dsp_batch_debug_depth_schedule(dsp_batch* b, const float* depths, int32_t n_iterations);
/* Forensics: the per-sample arrays the LAST iteration of the last run left behind for object obj (with the posterior or the
 * observation report on, that is their pass: it is then the last linearisation of the last run, at the returned state), expanded to
 * (n_rays x num_depth_samples) grids: raymask (n_rays; bit j = sample j lies inside the unit sphere), ssdf (the sdf the occupancy
 * scan read: fp32 inside the band, the prepass value or the placeholder 1.0 elsewhere; NaN = not in the sphere), sdeds (de_ds of a kept
 * sample, 0 = not kept, NaN = not in the sphere).  cap = floats available in ssdf / sdeds (>= n_rays * num_depth_samples). */
int dsp_batch_debug_samples(dsp_batch* b, int32_t obj, uint64_t* raymask, float* ssdf, float* sdeds, int64_t cap);
/* Testing: the Lie-group maps and the rotation prior evaluated ON THE DEVICE by the very functions the solve kernel calls (one thread, same
 * fp32 / fp64 arithmetic), so that every branch can be compared with vectors recorded from the reference:
 *   kind 0: x[7]  -> out[16] = exp_sim3(x)   -- reconstruct/loss_utils.py:188-233 (theta <= 1e-8 / s == 0 branch :211-218, the
 *                                               `c = 0. if s <= eps` quirk :223)
 *   kind 1: x[6]  -> out[16] = exp_se3(x)    -- reconstruct/loss_utils.py:129-163
 *   kind 2: x[16] = t_obj_cam -> out[0..6] = J_rot, out[7] = res_rot (compute_rotation_loss_sim3, reconstruct/loss.py:155-178, zero branch
 *           :172-173), out[8] = scale = det(R_co)^(1/3), out[9], out[10] = the depth range t_z -+ scale (reconstruct/optimizer.py:120-125),
 *           out[11] = status (DSP_OBJ_NAN for a singular matrix: the other entries are then zero)
 *   kind 3: x[0..15] = t_obj_cam, x[16..22] = dx -> out[16] = exp_sim3(dx) @ t_obj_cam  (the update of reconstruct/optimizer.py:187-188)
 * n_depth = num_depth_samples (2..64; only kind 2 reads it). */
int dsp_debug_lie(dsp_handle* h, int kind, const float* x, int32_t n_depth, float* out16);
/* Testing: the (n + 1)-th fresh device allocation the handle's pool makes from now on fails as if HBM were exhausted (n < 0: off).  The call
 * that hits it returns DSP_E_NOMEM with nothing of its half-built batch left allocated; the handle stays usable. */
int dsp_debug_fail_alloc(dsp_handle* h, int n);
/* Record per-iteration traces during the following runs (testing; costs ~21 KB per object-iteration). */
int dsp_batch_enable_trace(dsp_batch* b, int on);
/* Per-iteration trace of the last run (testing): for iteration e < num_iterations and object i,
 * H (71x71), b (71), dx (71), V, m, K, the state the iteration started from, and set_sums[2*i + {0,1}] = order-
 * independent checksums of the in-sphere sample set and of the kept (jacobian) sample set: sum over members of
 * hash(ray << 6 | depth_index), hash(x) = (x * 2654435761) ^ (x >> 7), mod 2^32.  Any pointer may be NULL.
 * A pose-only batch (dsp_batch_create_pose) fills H as 6x6 (n_objects x 36), b and dx as 6 per object; its K is the number of points
 * the iteration's system was built from (M, or those the inlier filter kept after iteration 4), V = m = 0; of an iteration that finds
 * no point only K (= 0) is written.  What an iteration does not write -- the rows of an object that has failed, or that the convergence
 * rule has frozen -- reads as zeros. */
int dsp_batch_trace(dsp_batch* b, int32_t iteration, float* H, float* bvec, float* dx, int64_t* V, int64_t* m,
                    int64_t* K, float* t_obj_cam, float* code, uint32_t* set_sums, float* depths /* 64 per object */);
/* A multi-view batch (dsp_batch_create_multiview): dsp_batch_trace returns, per OBJECT, the pooled H, b, dx, the object's state, the
 * reference view's depths, and V, m, K summed over its views (set_sums is zero there: a checksum belongs to one view's sample set, whose
 * ray indices are the view's own); this call returns them per VIEW:
 * V, m, K (n_views), t_obj_cam (n_views x 16: T_oc_v), set_sums (n_views x 2), depths (n_views x 64).  A view with V < 10 has K = 0.  Any
 * pointer may be NULL; DSP_E_ARG for any other kind of batch. */
int dsp_batch_trace_views(dsp_batch* b, int32_t iteration, int64_t* V, int64_t* m, int64_t* K, float* t_obj_cam, uint32_t* set_sums,
                          float* depths /* 64 per view */);
void dsp_batch_destroy(dsp_batch* b);

/* ---- multi-GPU: objects are independent, so GPUs take disjoint blocks of the object list (one handle per GPU, one host
 *      thread per handle) and the ONLY exchange is one gather of the per-object results.  The Python mirror does this across processes with
 *      torch.distributed (dsp_slam_amd/distributed.py); these two calls are the same for a single C / C++ process that owns several GPUs. */
#define DSP_RESULT_WIDTH 82   /* t_cam_obj 16 | code 64 | loss | status (as float) */
/* Pack the outputs of dsp_reconstruct_batch / dsp_batch_results into n x DSP_RESULT_WIDTH rows (host only). */
void dsp_pack_results(int32_t n, const float* t_cam_obj, const float* codes, const float* loss, const int32_t* status, float* packed);
/* results[i]: n_objects[i] x DSP_RESULT_WIDTH host floats produced on handles[i] (distinct GPUs).  The blocks are uploaded, gathered
 * device-to-device to handles[0]'s GPU by ONE RCCL ncclGather (xGMI; uneven blocks padded to the largest), and returned in `out`
 * concatenated in handle order (sum(n_objects) x DSP_RESULT_WIDTH).  librccl is loaded on first use (dlopen), not linked. */
int dsp_gather_results(dsp_handle* const* handles, int32_t n_handles, const float* const* results, const int32_t* n_objects, float* out);
/* The same gather straight from device-resident batches (one per GPU, each run before): every batch keeps its results as packed rows in
 * HBM, so the data goes device -> ncclGather -> host ONCE (no host bounce in front of the collective).  out: sum of the batches' object
 * counts x DSP_RESULT_WIDTH, in batch order.  Both gathers hold the mutex of EVERY handle involved (taken in a fixed order) for the whole
 * call: a dsp_batch_run issued on one of the handles by its own host thread waits, it cannot interleave with the collective. */
int dsp_gather_batch_results(dsp_batch* const* batches, int32_t n_batches, float* out);
/* Copy a batch's packed result rows (n_objects x DSP_RESULT_WIDTH) to a DEVICE buffer on the batch's GPU -- e.g. a PyTorch-ROCm tensor's
 * data_ptr() that a torch.distributed collective then sends (dsp_slam_amd/distributed.py: gather_results_device). */
int dsp_batch_results_packed_dev(dsp_batch* b, float* dst_dev);

#ifdef __cplusplus
}
#endif
#endif /* DSP_GN_H */
