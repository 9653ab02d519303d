"""Python face of libdspgn: one Engine per (decoder, GPU).  Thin: marshals numpy arrays into the C ABI.

Everything numeric happens in the HIP library; there is no CPU or PyTorch fallback.
"""
import atexit
import ctypes as C
import weakref

import numpy as np

from . import _lib as L


def gn_params(k1=1.0, k2=100.0, k3=0.25, k4=1e7, b1=0.2, b2=0.025, lr=1.0, s_damp=1.0, num_iterations=10,
              num_depth_samples=50, cut_off=0.01, pose_only_iterations=5):
    return L.GnParams(k1, k2, k3, k4, b1, b2, lr, s_damp, int(num_iterations), int(num_depth_samples), cut_off,
                      int(pose_only_iterations))


def params_from_configs(configs):
    """Hyper-parameters as Optimizer.__init__ reads them (reference reconstruct/optimizer.py:27-43)."""
    o = configs["optimizer"] if isinstance(configs, dict) else configs.optimizer
    get = (lambda d, k: d[k]) if isinstance(o, dict) else getattr
    j = get(o, "joint_optim")
    try:
        pose_it = get(get(o, "pose_only_optim"), "num_iterations")
    except (KeyError, AttributeError):
        pose_it = 5
    return gn_params(get(j, "k1"), get(j, "k2"), get(j, "k3"), get(j, "k4"), get(j, "b1"), get(j, "b2"),
                     get(j, "learning_rate"), get(j, "scale_damping"), get(j, "num_iterations"),
                     get(o, "num_depth_samples"), get(o, "cut_off_threshold"), pose_it)


# ---- mask of unknowns (dsp_batch_unknowns, include/dsp_gn.h): named groups of H's order [v(3), w(3), sigma | code(64)] ---------------------
UNKNOWN_GROUPS = {"translation": (0, 1, 2), "rotation": (3, 4, 5), "yaw": (4,), "scale": (6,), "pose": tuple(range(7)), "code": tuple(range(7, 71)),
                  "all": tuple(range(71))}


def unknowns_mask(groups, pose_only=False):
    """The LIVE groups -> a uint8 mask (71,), pose-only (6,): 1 = live, 0 = frozen.  groups: one name or a list of names out of "translation"
    (entries 0-2), "rotation" (3-5), "yaw" (4 only: the rotation about the object's up axis), "scale" (6), "pose" (0-6), "code" (7-70), "all".
    An empty list freezes everything.  A pose-only batch has the six SE(3) entries: "scale" and "code" name nothing there, "pose" and "all" are
    its six.  An unknown name raises ValueError."""
    if isinstance(groups, str):
        groups = [groups]
    n = 6 if pose_only else 71
    m = np.zeros(n, np.uint8)
    for g in groups:
        if g not in UNKNOWN_GROUPS:
            raise ValueError("unknowns: no group %r (known: %s)" % (g, ", ".join(sorted(UNKNOWN_GROUPS))))
        idx = [i for i in UNKNOWN_GROUPS[g] if i < n]
        m[idx] = 1
    return m


def _ragged(arrays, width):
    """list of (n_i, width) arrays -> (offsets int64 (B+1), flat float32 (sum n_i, width))."""
    arrays = [L.f32(a).reshape(-1, width) if width else L.f32(a).reshape(-1) for a in arrays]
    off = np.zeros(len(arrays) + 1, np.int64)
    off[1:] = np.cumsum([a.shape[0] for a in arrays])
    flat = np.concatenate(arrays, 0) if arrays else np.zeros((0, width), np.float32)
    if flat.size == 0:
        flat = np.zeros((1, width) if width else (1,), np.float32)
    return off, np.ascontiguousarray(flat, np.float32)


class Batch(object):
    """Device-resident batch of objects (dsp_batch_*): upload once, run many times."""

    def __init__(self, engine, prm, t_cam_obj, pts, rays, depth, codes=None, trace=False, scale=None):
        self.engine = engine
        self.n = len(pts)
        self.pose_only = scale is not None
        if self.pose_only:       # Engine.pose_batch: t_cam_obj holds the SE(3) estimates, rays / depth are unused
            self._create_pose(prm, t_cam_obj, pts, scale, codes)
            if trace:
                L.check(L.load().dsp_batch_enable_trace(self._h, 1), engine._h, "dsp_batch_enable_trace")
            return
        self._keep = (
            _ragged(pts, 3), _ragged(rays, 3), _ragged(depth, 0),
            L.f32(np.stack([np.asarray(t, np.float32).reshape(4, 4) for t in t_cam_obj])),
            None if codes is None else L.f32(np.stack([L.code64(c) for c in codes])),
        )
        (po, p), (ro, r), (do, d), t, c = self._keep
        self._h = C.c_void_p()
        lib = L.load()
        L.check(lib.dsp_batch_create(engine._h, C.byref(prm), self.n, L.ptr(po, L.c_i64p), L.ptr(p), L.ptr(ro, L.c_i64p),
                                     L.ptr(r), L.ptr(do, L.c_i64p), L.ptr(d), L.ptr(t), L.ptr(c), C.byref(self._h)),
                engine._h, "dsp_batch_create")
        self.iters = prm.num_iterations
        engine._batches.add(self)          # Engine.close() closes its live batches first: a batch must not outlive its handle
        if trace:
            L.check(lib.dsp_batch_enable_trace(self._h, 1), engine._h, "dsp_batch_enable_trace")

    def _create_pose(self, prm, t_co_se3, pts, scale, codes):
        n = self.n
        po, p = _ragged(pts, 3)
        t = L.f32(np.stack([np.asarray(x, np.float32).reshape(4, 4) for x in t_co_se3]))
        sc = L.f32(np.asarray(scale, np.float32).reshape(n))
        cd = L.f32(np.stack([L.code64(c) for c in codes]))
        self._keep = (po, p, t, sc, cd)
        self._h = C.c_void_p()
        L.check(L.load().dsp_batch_create_pose(self.engine._h, C.byref(prm), n, L.ptr(po, L.c_i64p), L.ptr(p), L.ptr(t), L.ptr(sc), L.ptr(cd),
                                               C.byref(self._h)), self.engine._h, "dsp_batch_create_pose")
        self.iters = prm.pose_only_iterations
        self.engine._batches.add(self)

    # ---- the five settings of the C ABI (include/dsp_gn.h) ------------------------------------------------------------------------------
    def set_ray_passes(self, n):
        """0 = automatic, 1 = decode every in-sphere sample (reference behaviour), n = n front-to-back depth ranges."""
        L.check(L.load().dsp_batch_set_ray_passes(self._h, int(n)), self.engine._h, "dsp_batch_set_ray_passes")

    def set_prepass(self, mode=-1, delta=-1.0):
        """Low-precision pre-classification of the forward ray samples: -1 automatic, 0 off, 1 f16, 2 bf16; delta < 0 = default margin.
        Results are bit-identical for every setting whose delta exceeds the decoder's prepass error."""
        L.check(L.load().dsp_batch_set_prepass(self._h, int(mode), float(delta)), self.engine._h, "dsp_batch_set_prepass")

    def set_prepass_guard(self, on=True):
        """The always-on guard of the prepass (include/dsp_gn.h): off only to see what an unguarded run would return."""
        L.check(L.load().dsp_batch_set_prepass_guard(self._h, int(bool(on))), self.engine._h, "dsp_batch_set_prepass_guard")

    def set_kernel_timing(self, mode):
        """HIP events around every decoder launch (stats ms_mlp_*): -1 = automatic (batches of more than 16 objects), 0 = off, 1 = on."""
        L.check(L.load().dsp_batch_set_kernel_timing(self._h, int(mode)), self.engine._h, "dsp_batch_set_kernel_timing")

    def set_compute(self, mode):
        """0 = fp32 (default: the parity path), 1 = f16, 2 = bf16: the opt-in low-precision compute mode (dsp_batch_set_compute) -- NOT bit- or
        1e-4-comparable with the reference; see include/dsp_gn.h."""
        L.check(L.load().dsp_batch_set_compute(self._h, int(mode)), self.engine._h, "dsp_batch_set_compute")

    def set_iterations(self, n):
        L.check(L.load().dsp_batch_set_iterations(self._h, int(n)), self.engine._h, "dsp_batch_set_iterations")
        self.iters = int(n)

    # ---- convergence rule (NOT one of the "identical results" settings: an object stopped after n updates returns a run of n iterations) ------
    def set_convergence(self, pose_tol, code_tol, min_iterations=1):
        """Freeze each object once its Gauss-Newton step is small (dsp_batch_convergence): after the update of iteration e, converged when
        e + 1 >= min_iterations, max |lr dx_pose| < pose_tol and max |lr dx_code| < code_tol (strict; inf switches a half off; code_tol is
        ignored by pose-only batches).  (0, 0, 1) = off, the initial state."""
        L.check(L.load().dsp_batch_convergence(self._h, float(pose_tol), float(code_tol), int(min_iterations)), self.engine._h,
                "dsp_batch_convergence")

    def iterations_used(self):
        """Updates applied to each object in the last run (dsp_batch_iterations_used): int32 (n,), per object also for multi-view batches."""
        out = np.zeros(self.n, np.int32)
        L.check(L.load().dsp_batch_iterations_used(self._h, L.ptr(out, L.c_i32p)), self.engine._h, "dsp_batch_iterations_used")
        return out

    # ---- Levenberg-Marquardt step control (dsp_batch_step_control, include/dsp_gn.h; the rule: csrc/step_rule.h) ---------------------------
    def set_step_control(self, lambda0=0.0, up=10.0, down=0.1, lambda_min=1.0, lambda_max=float("inf")):
        """Keep an iteration's state only if it lowers the cost (loss, + the prior's chi2): a rejected trial is discarded and the accepted
        state's system is solved again with lambda <- min(max(lambda, lambda_min) * up, lambda_max) on its diagonal; an acceptance multiplies
        lambda by down.  The run's last iteration only evaluates, so the returned state is the best evaluated one and `loss` is the loss at it.
        The defaults are NOT measurements: 10 and 0.1 are Marquardt's conventional factors, lambda_min = 1 is the size of the reference's
        own pose damping (+ I), and lambda0 = 0 makes the first step the reference's.  set_step_control(0, 0, 0, 0, 0) = off, the initial
        state.  Joint batches only."""
        L.check(L.load().dsp_batch_step_control(self._h, float(lambda0), float(up), float(down), float(lambda_min), float(lambda_max)),
                self.engine._h, "dsp_batch_step_control")

    def step_log(self):
        """The last run's decisions (dsp_batch_step_log): dict(decision int32 (iterations, n) -- 0 not evaluated (failed / frozen / left out),
        1 accepted, 2 rejected; cost float64 (iterations, n) = F_e; lambda float64 (iterations, n) = the value after the decision)."""
        shape = (self.iters, self.n)
        out = {"decision": np.zeros(shape, np.int32), "cost": np.zeros(shape), "lambda": np.zeros(shape)}
        L.check(L.load().dsp_batch_step_log(self._h, L.ptr(out["decision"], L.c_i32p), L.ptr(out["cost"], L.c_f64p), L.ptr(out["lambda"], L.c_f64p)),
                self.engine._h, "dsp_batch_step_log")
        return out

    # ---- posterior (changes no result: one more linearisation at the returned state, include/dsp_gn.h) ------------------------------------
    def set_posterior(self, level=1, weights="mean"):
        """level 0 = off (initial), 1 = pose information / covariance, code variance, loss and counts per object, 2 = also Lambda, g and the
        state they were taken at.  weights "mean" (the reference's objective: k2 / M, k1 / K) or "sum" (k2, k1: information grows with the
        number of observations -- what pose_graph.edge_information wants)."""
        L.check(L.load().dsp_batch_posterior(self._h, int(level), _posterior_weights(weights)), self.engine._h, "dsp_batch_posterior")
        self._posterior_level = int(level)

    def posterior(self):
        """The records of the last run (dsp_batch_posterior_fetch), per object: dict(status int32 (n,) -- L.POSTERIOR_OK / _NONE / _SINGULAR,
        info_pose / cov_pose float64 (n, P, P) with P = 7 (pose-only: 6) in the order [v, w, sigma], var_code float64 (n, code_len),
        loss float32, M / V / K int64; after a level-2 run also Lambda (n, 71, 71), g (n, 71), t_obj_cam (n, 4, 4), code (n, code_len),
        depths (n, 64))."""
        n, P = self.n, 6 if self.pose_only else 7
        lib, h = L.load(), self.engine._h
        out = dict(status=np.zeros(n, np.int32), info_pose=np.zeros((n, P, P)), cov_pose=np.zeros((n, P, P)), var_code=np.zeros((n, L.CODE_LEN)),
                   loss=np.zeros(n, np.float32), M=np.zeros(n, np.int64), V=np.zeros(n, np.int64), K=np.zeros(n, np.int64))
        l1 = (L.ptr(out["status"], L.c_i32p), L.ptr(out["info_pose"], L.c_f64p), L.ptr(out["cov_pose"], L.c_f64p), L.ptr(out["var_code"], L.c_f64p),
              L.ptr(out["loss"]), L.ptr(out["M"], L.c_i64p), L.ptr(out["V"], L.c_i64p), L.ptr(out["K"], L.c_i64p))
        if getattr(self, "_posterior_run_level", 0) < 2:            # a level-1 run keeps no Lambda (level 0 / no run: the call says so)
            L.check(lib.dsp_batch_posterior_fetch(self._h, *l1, None, None, None, None, None), h, "dsp_batch_posterior_fetch")
        else:
            l2 = dict(Lambda=np.zeros((n, 71, 71)), g=np.zeros((n, 71)), t_obj_cam=np.zeros((n, 4, 4), np.float32), code=np.zeros((n, L.CODE_LEN), np.float32),
                      depths=np.zeros((n, 64), np.float32))
            L.check(lib.dsp_batch_posterior_fetch(self._h, *l1, L.ptr(l2["Lambda"], L.c_f64p), L.ptr(l2["g"], L.c_f64p), L.ptr(l2["t_obj_cam"]), L.ptr(l2["code"]),
                                                  L.ptr(l2["depths"])), h, "dsp_batch_posterior_fetch")
            out.update(l2)
            out["code"] = np.ascontiguousarray(out["code"][:, :self.engine.code_len])
        out["var_code"] = np.ascontiguousarray(out["var_code"][:, :self.engine.code_len])
        return out

    # ---- observation report (dsp_batch_report, include/dsp_gn.h): every observation once more at the returned state; changes no result ------
    def set_report(self, on=True):
        """on: the following runs evaluate every surface point and every ray once more at the state they return and keep the values on the
        device for report().  False = off, the initial state."""
        L.check(L.load().dsp_batch_report(self._h, int(bool(on))), self.engine._h, "dsp_batch_report")

    def report(self):
        """The last run's observation report (dsp_batch_report_fetch), concatenated in MEMBER order -- a member is an object, or a view of a
        multi-view batch: dict(pt_sdf float32 (n_points,), pt_alive bool (n_points,) -- bit 0 of the flags, pt_flags uint8, ray_depth /
        ray_hit / ray_residual float32 (n_rays,), ray_counts int32 (n_rays, 3) = in-sphere, band, kept samples, and per member M, V, m, K
        int64, sum_s / sum_r float64, status int32; pts_off / ray_off / depth_off int64 (n_members + 1) cut the rows per member
        (depth_off: its foreground rays come first, depth_off[i + 1] - depth_off[i] of them) and view_off int64 (n_objects + 1) the
        members per object."""
        lib, h = L.load(), self.engine._h
        n_p, n_r, n_m = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        L.check(lib.dsp_batch_report_sizes(self._h, C.byref(n_p), C.byref(n_r), C.byref(n_m)), h, "dsp_batch_report_sizes")
        n_p, n_r, n_m = n_p.value, n_r.value, n_m.value
        out = dict(pt_sdf=np.zeros(n_p, np.float32), pt_flags=np.zeros(n_p, np.uint8), ray_depth=np.zeros(n_r, np.float32),
                   ray_hit=np.zeros(n_r, np.float32), ray_residual=np.zeros(n_r, np.float32), ray_counts=np.zeros((n_r, 3), np.int32))
        member = np.zeros((n_m, 8))
        L.check(lib.dsp_batch_report_fetch(self._h, L.ptr(out["pt_sdf"]), L.ptr(out["pt_flags"], C.POINTER(C.c_uint8)), L.ptr(out["ray_depth"]),
                                           L.ptr(out["ray_hit"]), L.ptr(out["ray_residual"]), L.ptr(out["ray_counts"], L.c_i32p),
                                           L.ptr(member, L.c_f64p)), h, "dsp_batch_report_fetch")
        out["pt_alive"] = (out["pt_flags"] & 1).astype(bool)
        for i, k in enumerate(("M", "V", "m", "K")):
            out[k] = member[:, i].astype(np.int64)
        out["sum_s"], out["sum_r"] = member[:, 4].copy(), member[:, 5].copy()
        out["status"] = member[:, 6].astype(np.int32)
        out.update(self._member_offsets(n_m))
        return out

    # ---- per-observation weights (dsp_batch_observation_weights, include/dsp_gn.h): the input the report's answer is fed back through -------
    def set_observation_weights(self, pt_w=None, ray_w=None):
        """pt_w: one weight per surface point, ray_w: one per ray (foreground rays first), each a concatenated array in MEMBER order -- the
        layout of report() -- or a list of per-member arrays.  None = all ones for that kind; both None = off, the initial state.  A
        weight multiplies the observation's squared residual and the means divide by the weight sums; a ray of weight 0 is absent.  The
        weights stay set for the following runs.  A pose-only batch ignores ray_w."""
        lib, h = L.load(), self.engine._h
        n_p, n_r, n_m = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        L.check(lib.dsp_batch_report_sizes(self._h, C.byref(n_p), C.byref(n_r), C.byref(n_m)), h, "dsp_batch_report_sizes")

        def flat(w, n, what):
            if w is None:
                return None
            if isinstance(w, (list, tuple)):
                w = np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in w]) if len(w) else np.zeros(0, np.float32)
            w = L.f32(np.asarray(w, np.float32).reshape(-1))
            if w.size != n:
                raise ValueError("set_observation_weights: %s has %d entries, the batch has %d" % (what, w.size, n))
            return w
        pw = flat(pt_w, n_p.value, "pt_w")
        rw = None if self.pose_only else flat(ray_w, n_r.value, "ray_w")
        L.check(lib.dsp_batch_observation_weights(self._h, L.ptr(pw), L.ptr(rw)), h, "dsp_batch_observation_weights")

    # ---- mask of unknowns (dsp_batch_unknowns, include/dsp_gn.h): which pose, scale and code entries the following runs estimate -------------
    def set_unknowns(self, live=None):
        """live: None = every entry live = off (the initial state); an (n, 71) array (pose-only batch: (n, 6)) of 1 = live / 0 = frozen in H's
        order [v(3), w(3), sigma | code(64)], or one (71,) / (6,) row for every object; or group names (unknowns_mask): a list of names for the
        whole batch, or a list of n lists, one per object.  Frozen entries keep their value: the run solves the system conditioned on them.
        The mask stays set for the following runs.  Multi-view batches take it per object."""
        lib, h = L.load(), self.engine._h
        if live is None:
            L.check(lib.dsp_batch_unknowns(self._h, None), h, "dsp_batch_unknowns")
            return
        w = 6 if self.pose_only else 71
        if isinstance(live, str):
            live = [live]
        if isinstance(live, (list, tuple)) and (len(live) == 0 or all(isinstance(x, str) for x in live)):
            m = unknowns_mask(live, self.pose_only)
        elif isinstance(live, (list, tuple)) and all(isinstance(x, (list, tuple, str)) and (isinstance(x, str) or all(isinstance(y, str) for y in x))
                                                     for x in live):
            m = np.stack([unknowns_mask(x, self.pose_only) for x in live])
        else:
            m = np.asarray(live)
            m = np.where((m == 0) | (m == 1), m, 2).astype(np.uint8)         # anything else reaches the library as 2, which it refuses
        if m.ndim == 1 and m.shape[0] == w:
            m = np.broadcast_to(m, (self.n, w))
        if m.shape != (self.n, w):
            raise ValueError("set_unknowns: the mask must be (%d, %d) or (%d,), not %r" % (self.n, w, w, tuple(m.shape)))
        m = np.ascontiguousarray(m, np.uint8)
        L.check(lib.dsp_batch_unknowns(self._h, L.ptr(m, C.POINTER(C.c_uint8))), h, "dsp_batch_unknowns")

    def _member_offsets(self, n_members):
        """pts_off / ray_off / depth_off per member as they were uploaded, and view_off (every object one member)."""
        if self.pose_only:
            zeros = np.zeros(n_members + 1, np.int64)
            offs = dict(pts_off=np.asarray(self._keep[0], np.int64).copy(), ray_off=zeros, depth_off=zeros.copy())
        else:
            (po, _), (ro, _), (do, _) = self._keep[0], self._keep[1], self._keep[2]
            offs = dict(pts_off=po.copy(), ray_off=ro.copy(), depth_off=do.copy())
        offs["view_off"] = np.arange(n_members + 1, dtype=np.int64)
        return offs

    # ---- Gaussian prior on pose and code (dsp_batch_prior, include/dsp_gn.h): fuse an earlier estimate into the run -------------------------
    def set_prior(self, t_obj_cam0=None, code0=None, Lambda=None):
        """Per object: t_obj_cam0 (4, 4) camera -> object, code0 (code_len or 64; ignored by pose-only batches), Lambda (71, 71) float64
        (pose-only: (6, 6)) in the order [v, w, sigma | code] -- the t_obj_cam, code and Lambda of a level-2 Batch.posterior() can be passed as
        they are (mind that such a Lambda already contains the k3 and k4 terms).  An object whose Lambda is all zero has no prior.  All None =
        off, the initial state."""
        lib, h = L.load(), self.engine._h
        if t_obj_cam0 is None and code0 is None and Lambda is None:
            L.check(lib.dsp_batch_prior(self._h, None, None, None), h, "dsp_batch_prior")
            return
        n, N = self.n, 6 if self.pose_only else 71
        if t_obj_cam0 is None or Lambda is None or (code0 is None and not self.pose_only):
            raise ValueError("set_prior takes t_obj_cam0, code0 and Lambda together (code0 may be None for pose-only batches), or all None")
        t = L.f32(np.stack([np.asarray(x, np.float32).reshape(4, 4) for x in t_obj_cam0]))
        lam = np.ascontiguousarray(np.stack([_prior_lambda(x, N) for x in Lambda]))
        c = None if self.pose_only or code0 is None else L.f32(np.stack([L.code64(x) for x in code0]))
        if t.shape[0] != n or lam.shape[0] != n or (c is not None and c.shape[0] != n):
            raise ValueError("set_prior: one t_obj_cam0, code0 and Lambda per object (%d)" % n)
        L.check(lib.dsp_batch_prior(self._h, L.ptr(t), L.ptr(c), L.ptr(lam, L.c_f64p)), h, "dsp_batch_prior")

    def prior_residual(self):
        """dict(e float64 (n, P + code_len) = [Log(T_oc T0^-1) | z - z0] (pose-only: (n, 6)), chi2 float64 (n,) = e^T Lambda e) at the state
        the last run RETURNED (dsp_batch_prior_fetch): NaN for an object that did not end good, 0 for an object without a prior."""
        n, P = self.n, 6 if self.pose_only else 7
        e = np.zeros((n, P + L.CODE_LEN))
        chi2 = np.zeros(n)
        L.check(L.load().dsp_batch_prior_fetch(self._h, L.ptr(e, L.c_f64p), L.ptr(chi2, L.c_f64p)), self.engine._h, "dsp_batch_prior_fetch")
        return dict(e=np.ascontiguousarray(e[:, :P] if self.pose_only else e[:, :P + self.engine.code_len]), chi2=chi2)

    # ---- testing: pin one of the bit-identical forms the library chooses between by itself (dsp_batch_set_debug) --------------------------
    def set_debug(self, key, value):
        L.check(L.load().dsp_batch_set_debug(self._h, int(key), int(value)), self.engine._h, "dsp_batch_set_debug(%d, %d)" % (key, value))

    def set_mask_reuse(self, mode):
        """-1 = automatic, 0 = render rows share the surface points' forward+backward launch, 1 = backward-only from exported masks."""
        self.set_debug(L.DBG_MASK_REUSE, mode)

    def set_split_rows(self, mode):
        """-1 = automatic, 0 = 64-point throughput tiles, 1 = 16-point latency tiles for the jacobian launch (when mask reuse is off)."""
        self.set_debug(L.DBG_SPLIT_ROWS, mode)

    def set_tail_split(self, mode):
        """-1 = automatic, 0 = off, 1 = the last partial round of the fp32 forward launch runs as 16-point latency-form tiles."""
        self.set_debug(L.DBG_TAIL_SPLIT, mode)

    def set_wave_bookkeeping(self, mode):
        """-1 = automatic, 0 = per-ray bookkeeping as count / scan / write launches (throughput form), 1 = one wave per ray over the whole chip."""
        self.set_debug(L.DBG_WAVE_BOOKKEEPING, mode)

    def set_speculative_band(self, mode):
        """-1 = automatic, 0 = band samples get a forward launch of their own, 1 = they go straight into the jacobian launch (latency path)."""
        self.set_debug(L.DBG_SPECULATIVE_BAND, mode)

    def set_mixed_reuse(self, mode):
        """-1 = automatic, 0 = off, 1 = kept render rows backward-only from exported masks INSIDE the latency-form jacobian launch."""
        self.set_debug(L.DBG_MIXED_REUSE, mode)

    def set_cluster_tiles(self, mode):
        """-1 = automatic, 0 = one workgroup per 16-point jacobian tile, 1 = four (cluster form) for lists of up to 128 tiles."""
        self.set_debug(L.DBG_CLUSTER_TILES, mode)

    def set_direct_tiles(self, mode):
        """-1 automatic / 1: a one-object batch's decoder kernels derive their tile lists themselves; 0: k_build_tiles launches."""
        self.set_debug(L.DBG_DIRECT_TILES, mode)

    def set_prepass_tile(self, points=-1):
        """-1 = automatic, 128 or 64 points per prepass tile.  Results are identical for either."""
        self.set_debug(L.DBG_PREPASS_TILE, points)

    def set_prepass_audit(self, on=True):
        self.set_debug(L.DBG_PREPASS_AUDIT, int(bool(on)))

    def set_lp_small_batches(self, mode):
        """-1 / 0 = a detection-sized batch keeps the fp32 latency path when the low-precision compute mode is set (faster there), 1 = the mode applies to it too."""
        self.set_debug(L.DBG_LP_SMALL_BATCHES, mode)

    def set_cluster_fault(self, on):
        """Fault injection: the following runs' cluster launches lose one workgroup's hand-off; False also ends the handle's cool-down."""
        self.set_debug(L.DBG_CLUSTER_FAULT, int(bool(on)))

    # ---- forensics ------------------------------------------------------------------------------------------------------------------------
    def set_ray_pass_bounds(self, bounds):
        bounds = np.ascontiguousarray(bounds, np.int32)
        L.check(L.load().dsp_batch_debug_ray_pass_bounds(self._h, L.ptr(bounds, L.c_i32p), bounds.shape[0] - 1), self.engine._h,
                "dsp_batch_debug_ray_pass_bounds")

    def set_start_state(self, t_obj_cam=None, codes=None, depths=None):
        """Testing / forensics: start the following runs from these camera->object matrices (taken bit for bit) and / or codes; depths
        (per object, num_depth_samples values): the first iteration samples the rays at exactly these depths."""
        t = None if t_obj_cam is None else L.f32(np.stack([np.asarray(x, np.float32).reshape(4, 4) for x in t_obj_cam]))
        c = None if codes is None else L.f32(np.stack([L.code64(x) for x in codes]))
        d = None
        if depths is not None:
            d = np.zeros((self.n, 64), np.float32)
            for i, row in enumerate(depths):
                row = np.asarray(row, np.float32).reshape(-1)
                d[i, :row.shape[0]] = row
        L.check(L.load().dsp_batch_debug_start_state(self._h, L.ptr(t), L.ptr(c), L.ptr(d)), self.engine._h, "dsp_batch_debug_start_state")

    def set_depth_schedule(self, depths=None):
        """Testing / forensics: depths[e][i] = the depth samples object i uses in iteration e (None = derive them from the pose again)."""
        if depths is None:
            L.check(L.load().dsp_batch_debug_depth_schedule(self._h, None, 0), self.engine._h, "dsp_batch_debug_depth_schedule")
            return
        n_it = len(depths)
        d = np.zeros((n_it, self.n, 64), np.float32)
        for e in range(n_it):
            for i in range(self.n):
                row = np.asarray(depths[e][i], np.float32).reshape(-1)
                d[e, i, :row.shape[0]] = row
        L.check(L.load().dsp_batch_debug_depth_schedule(self._h, L.ptr(d), n_it), self.engine._h, "dsp_batch_debug_depth_schedule")

    def debug_samples(self, obj, n_rays, n_depth, raw_masks=False):
        """(in-sphere mask (n_rays, n_depth) bool, sdf grid, de_ds grid) the last iteration of the last run left for object obj
        (NaN outside the sphere; de_ds != 0 marks a kept sample).  raw_masks: a fourth item, the rays' 64-bit masks as the device holds
        them (uint64 (n_rays,); bit j = depth index j)."""
        rm = np.zeros(n_rays, np.uint64)
        sdf = np.zeros((n_rays, n_depth), np.float32)
        deds = np.zeros((n_rays, n_depth), np.float32)
        L.check(L.load().dsp_batch_debug_samples(self._h, int(obj), L.ptr(rm, C.POINTER(C.c_uint64)), L.ptr(sdf), L.ptr(deds), sdf.size),
                self.engine._h, "dsp_batch_debug_samples")
        mask = ((rm[:, None] >> np.arange(n_depth, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
        return (mask, sdf, deds, rm) if raw_masks else (mask, sdf, deds)

    def run(self):
        L.check(L.load().dsp_batch_run(self._h), self.engine._h, "dsp_batch_run")
        self._posterior_run_level = getattr(self, "_posterior_level", 0)      # what posterior() may ask dsp_batch_posterior_fetch for

    def results(self):
        n = self.n
        t = np.zeros((n, 4, 4), np.float32)
        code = np.zeros((n, L.CODE_LEN), np.float32)
        loss = np.zeros(n, np.float32)
        status = np.zeros(n, np.int32)
        L.check(L.load().dsp_batch_results(self._h, L.ptr(t), L.ptr(code), L.ptr(loss), L.ptr(status, L.c_i32p)),
                self.engine._h, "dsp_batch_results")
        return t, np.ascontiguousarray(code[:, :self.engine.code_len]), loss, status

    def results_packed_to_device(self, dst_ptr):
        """Copy the packed result rows (n x 82 float32, distributed.RESULT_WIDTH) device-to-device to dst_ptr (e.g. a torch tensor's data_ptr() on
        this batch's GPU): the results never touch the host in front of the multi-GPU gather."""
        L.check(L.load().dsp_batch_results_packed_dev(self._h, C.c_void_p(int(dst_ptr))), self.engine._h, "dsp_batch_results_packed_dev")

    def stats(self):
        s = L.Stats()
        L.check(L.load().dsp_batch_stats(self._h, C.byref(s)), self.engine._h, "dsp_batch_stats")
        return {k: getattr(s, k) for k, _ in L.Stats._fields_}

    def trace(self, iteration):
        """One iteration of the last run.  Pose-only batches: H (n, 6, 6), b / dx (n, 6), K = the points the system was built from."""
        n = self.n
        u = 6 if self.pose_only else 71
        out = dict(H=np.zeros((n, u, u), np.float32), b=np.zeros((n, u), np.float32), dx=np.zeros((n, u), np.float32),
                   V=np.zeros(n, np.int64), m=np.zeros(n, np.int64), K=np.zeros(n, np.int64),
                   t_obj_cam=np.zeros((n, 4, 4), np.float32), code=np.zeros((n, L.CODE_LEN), np.float32),
                   set_sums=np.zeros((n, 2), np.uint32), depths=np.zeros((n, 64), np.float32))
        L.check(L.load().dsp_batch_trace(self._h, int(iteration), L.ptr(out["H"]), L.ptr(out["b"]), L.ptr(out["dx"]),
                                         L.ptr(out["V"], L.c_i64p), L.ptr(out["m"], L.c_i64p), L.ptr(out["K"], L.c_i64p),
                                         L.ptr(out["t_obj_cam"]), L.ptr(out["code"]), L.ptr(out["set_sums"], C.POINTER(C.c_uint32)), L.ptr(out["depths"])),
                self.engine._h, "dsp_batch_trace")
        return out

    def close(self):
        if self._h:
            L.load().dsp_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _posterior_weights(weights):
    w = {"mean": L.POSTERIOR_MEAN, "sum": L.POSTERIOR_SUM, L.POSTERIOR_MEAN: L.POSTERIOR_MEAN, L.POSTERIOR_SUM: L.POSTERIOR_SUM}.get(weights)
    if w is None:
        raise ValueError("posterior weights must be 'mean' or 'sum', not %r" % (weights,))
    return w


def _posterior_args(posterior):
    """posterior= of the Engine calls: "mean" / "sum" (level 1) or (level, weights)."""
    if isinstance(posterior, (tuple, list)):
        return int(posterior[0]), posterior[1]
    return 1, posterior


def _step_control_args(step_control):
    """step_control= of the Engine calls and of the Optimizer's config: True (Batch.set_step_control's defaults), a dict of its keyword
    arguments, or a (lambda0, up, down, lambda_min, lambda_max) tuple -> keyword arguments."""
    if step_control is True:
        return {}
    if isinstance(step_control, dict):
        return dict(step_control)
    return dict(zip(("lambda0", "up", "down", "lambda_min", "lambda_max"), step_control))


def _run_resident(b, convergence, posterior, prior, step_control=None, report=None, obs_weights=None):
    """The optional rules of the Engine's one-call forms on a resident batch: -> results() [+ (posterior(),)] [+ (report(),)] [+ (prior_residual(),)]."""
    if convergence is not None:
        b.set_convergence(*convergence)
    if step_control is not None and step_control is not False:
        b.set_step_control(**_step_control_args(step_control))
    if posterior is not None:
        b.set_posterior(*_posterior_args(posterior))
    if prior is not None:
        b.set_prior(*_prior_args(prior))
    if report:
        b.set_report(True)
    if obs_weights is not None:
        b.set_observation_weights(*obs_weights)
    b.run()
    return (b.results() + (() if posterior is None else (b.posterior(),)) + ((b.report(),) if report else ()) +
            (() if prior is None else (b.prior_residual(),)))


def _prior_lambda(lam, n):
    """One object's Lambda as (n, n) float64; a pose-only batch (n = 6) also takes the (71, 71) a level-2 posterior record holds: its 6 x 6 block."""
    lam = np.asarray(lam, np.float64)
    if n == 6 and lam.shape == (71, 71):
        lam = lam[:6, :6]
    return lam.reshape(n, n)


def _prior_args(prior):
    """prior= of the Engine calls: dict(t_obj_cam, code, Lambda) of per-object arrays (a level-2 Batch.posterior() as it is) or a
    (t_obj_cam0, code0, Lambda) tuple -> the arguments of Batch.set_prior."""
    if isinstance(prior, dict):
        return prior["t_obj_cam"], prior.get("code"), prior["Lambda"]
    t0, c0, lam = prior
    return t0, c0, lam


def _flatten_views(views_per_object):
    """[[dict(t_ref_cam, pts, rays, depth), ...] per object] -> (view_off int64 (n + 1), t_ref (n_views, 4, 4), pts / rays / depth lists per view)."""
    off = np.zeros(len(views_per_object) + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in views_per_object])
    flat = [v for views in views_per_object for v in views]
    t_ref = L.f32(np.stack([np.asarray(v["t_ref_cam"], np.float32).reshape(4, 4) for v in flat])) if flat else np.zeros((1, 4, 4), np.float32)
    return (off, t_ref, [L.f32(v["pts"]).reshape(-1, 3) for v in flat], [L.f32(v["rays"]).reshape(-1, 3) for v in flat],
            [L.f32(v["depth"]).reshape(-1) for v in flat])


class MultiviewBatch(Batch):
    """Device-resident multi-view batch (dsp_batch_create_multiview): every object has ONE pose and ONE code and a list of views
    dict(t_ref_cam (4, 4) rigid view camera -> reference camera, pts, rays, depth) -- the first view is the reference camera (identity).
    run / results / stats / the setters / trace work as on a Batch, per object; set_start_state takes t_obj_cam and codes per object and
    depths per view; trace_views gives the per-view counts."""

    def __init__(self, engine, prm, t_cam_obj, views, codes=None, trace=False):
        self.engine = engine
        self.n = len(views)
        self.pose_only = False
        vo, t_ref, pts, rays, depth = _flatten_views(views)
        self.n_views = int(vo[-1])
        self.view_off = vo
        self._keep = (
            vo, t_ref, _ragged(pts, 3), _ragged(rays, 3), _ragged(depth, 0),
            L.f32(np.stack([np.asarray(t, np.float32).reshape(4, 4) for t in t_cam_obj])),
            None if codes is None else L.f32(np.stack([L.code64(c) for c in codes])),
        )
        _, _, (po, p), (ro, r), (do, d), t, c = self._keep
        self._h = C.c_void_p()
        lib = L.load()
        L.check(lib.dsp_batch_create_multiview(engine._h, C.byref(prm), self.n, L.ptr(vo, L.c_i64p), L.ptr(t_ref), L.ptr(po, L.c_i64p), L.ptr(p),
                                               L.ptr(ro, L.c_i64p), L.ptr(r), L.ptr(do, L.c_i64p), L.ptr(d), L.ptr(t), L.ptr(c), C.byref(self._h)),
                engine._h, "dsp_batch_create_multiview")
        self.iters = prm.num_iterations
        engine._batches.add(self)
        if trace:
            L.check(lib.dsp_batch_enable_trace(self._h, 1), engine._h, "dsp_batch_enable_trace")

    def _member_offsets(self, n_members):
        """The members are the views: offsets per view, view_off per object (Batch.report)."""
        vo, _, (po, _), (ro, _), (do, _) = self._keep[:5]
        return dict(pts_off=po.copy(), ray_off=ro.copy(), depth_off=do.copy(), view_off=np.asarray(vo, np.int64).copy())

    def set_start_state(self, t_obj_cam=None, codes=None, depths=None):
        """t_obj_cam / codes: one per object; depths: one row per VIEW (all objects' views in order)."""
        t = None if t_obj_cam is None else L.f32(np.stack([np.asarray(x, np.float32).reshape(4, 4) for x in t_obj_cam]))
        c = None if codes is None else L.f32(np.stack([L.code64(x) for x in codes]))
        d = None
        if depths is not None:
            d = np.zeros((self.n_views, 64), np.float32)
            for i, row in enumerate(depths):
                row = np.asarray(row, np.float32).reshape(-1)
                d[i, :row.shape[0]] = row
        L.check(L.load().dsp_batch_debug_start_state(self._h, L.ptr(t), L.ptr(c), L.ptr(d)), self.engine._h, "dsp_batch_debug_start_state")

    def set_depth_schedule(self, depths=None):
        """depths[e][v] = the depth samples VIEW v uses in iteration e."""
        if depths is None:
            return Batch.set_depth_schedule(self, None)
        n_it = len(depths)
        d = np.zeros((n_it, self.n_views, 64), np.float32)
        for e in range(n_it):
            for i in range(self.n_views):
                row = np.asarray(depths[e][i], np.float32).reshape(-1)
                d[e, i, :row.shape[0]] = row
        L.check(L.load().dsp_batch_debug_depth_schedule(self._h, L.ptr(d), n_it), self.engine._h, "dsp_batch_debug_depth_schedule")

    def trace_views(self, iteration):
        """Per view of one iteration of the last run: V, m, K, t_obj_cam (T_oc_v), set_sums, depths."""
        n = self.n_views
        out = dict(V=np.zeros(n, np.int64), m=np.zeros(n, np.int64), K=np.zeros(n, np.int64), t_obj_cam=np.zeros((n, 4, 4), np.float32),
                   set_sums=np.zeros((n, 2), np.uint32), depths=np.zeros((n, 64), np.float32))
        L.check(L.load().dsp_batch_trace_views(self._h, int(iteration), L.ptr(out["V"], L.c_i64p), L.ptr(out["m"], L.c_i64p), L.ptr(out["K"], L.c_i64p),
                                               L.ptr(out["t_obj_cam"]), L.ptr(out["set_sums"], C.POINTER(C.c_uint32)), L.ptr(out["depths"])),
                self.engine._h, "dsp_batch_trace_views")
        return out


def gather_results_c(engines, packed):
    """dsp_gather_results: one RCCL gather, inside ONE process, of the (n_i, 82) result blocks of several engines (one per GPU)
    to the first engine's GPU; returns them concatenated in engine order.  (Across processes use dsp_slam_amd.distributed.)"""
    n = len(engines)
    blocks = [L.f32(np.asarray(p, np.float32).reshape(-1, 82)) for p in packed]
    hs = (C.c_void_p * n)(*[e._h for e in engines])
    ptrs = (L.c_f32p * n)(*[L.ptr(b) for b in blocks])
    cnt = np.array([b.shape[0] for b in blocks], np.int32)
    out = np.zeros((int(cnt.sum()), 82), np.float32)
    L.check(L.load().dsp_gather_results(hs, n, ptrs, L.ptr(cnt, L.c_i32p), L.ptr(out)), engines[0]._h, "dsp_gather_results")
    return out


def gather_batches_c(batches):
    """dsp_gather_batch_results: the same gather straight from device-resident batches (one per GPU, each run before): device ->
    ncclGather -> host once."""
    n = len(batches)
    hs = (C.c_void_p * n)(*[b._h for b in batches])
    out = np.zeros((sum(b.n for b in batches), 82), np.float32)
    L.check(L.load().dsp_gather_batch_results(hs, n, L.ptr(out)), batches[0].engine._h, "dsp_gather_batch_results")
    return out


def pack_results_c(t_cam_obj, codes, loss, status):
    n = len(loss)
    out = np.zeros((n, 82), np.float32)
    codes = np.stack([L.code64(c) for c in codes]) if n else np.zeros((0, L.CODE_LEN), np.float32)
    L.load().dsp_pack_results(n, L.ptr(L.f32(t_cam_obj)), L.ptr(L.f32(codes)), L.ptr(L.f32(loss)), L.ptr(np.ascontiguousarray(status, np.int32), L.c_i32p),
                              L.ptr(out))
    return out


_last_engine = None
_live_engines = weakref.WeakSet()


@atexit.register
def _close_engines_at_exit():
    """Engines (and their batches) that are still alive when the interpreter exits -- a test that failed half way, a script that never called
    close() -- are closed HERE, while the interpreter and the HIP runtime are intact and in the right order (batches first), instead of by
    finalisers in no particular order."""
    for e in list(_live_engines):
        try:
            e.close()
        except Exception:
            pass


def last_engine():
    """The engine created last that is still alive (for module-level helpers of the reference API that take no decoder
    argument, such as reconstruct.utils.convert_sdf_voxels_to_mesh)."""
    e = _last_engine() if _last_engine is not None else None
    if e is None or not e._h:
        raise RuntimeError("no decoder is loaded on a GPU (get_decoder / config_decoder first)")
    return e


class Engine(object):
    """Owns a dsp_handle: packed decoder weights on one MI355X + a HIP stream."""

    def __init__(self, layers, latent_in, code_len=64, device=0):
        """layers: list of (W (out,in), b (out,)) float32 with weight-norm already folded."""
        lib = L.load()
        self._desc = L.DecoderDescHolder(layers, latent_in, code_len)
        self._batches = weakref.WeakSet()
        _live_engines.add(self)
        self._h = C.c_void_p()
        rc = lib.dsp_create(C.byref(self._desc.desc), int(device), C.byref(self._h))
        if rc != 0:
            msg = lib.dsp_last_error(None)
            raise L.DspError("dsp_create failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        self.device = int(device)
        self.code_len = int(code_len)
        global _last_engine
        _last_engine = weakref.ref(self)

    # -- decoder ------------------------------------------------------------------------------------
    def decode_sdf(self, code, pts):
        pts = L.f32(pts).reshape(-1, 3)
        code = L.code64(code)
        out = np.zeros(pts.shape[0], np.float32)
        L.check(L.load().dsp_decode_sdf(self._h, L.ptr(code), L.ptr(pts), pts.shape[0], L.ptr(out)), self._h, "dsp_decode_sdf")
        return out

    def decode_sdf_prepass(self, code, pts, dtype=L.PREPASS_F16):
        """The decoder through the low-precision prepass kernel (f16 / bf16 MFMA).  Calibration and tests only: the optimiser
        uses these values to classify samples, never as results."""
        pts = L.f32(pts).reshape(-1, 3)
        code = L.code64(code)
        out = np.zeros(pts.shape[0], np.float32)
        L.check(L.load().dsp_decode_sdf_prepass(self._h, int(dtype), L.ptr(code), L.ptr(pts), pts.shape[0], L.ptr(out)), self._h,
                "dsp_decode_sdf_prepass")
        return out

    def prepass_calibration(self, dtype=L.PREPASS_F16):
        """(largest |sdf_lp - sdf_fp32| measured at creation, margin derived from it) for this decoder."""
        err, delta = C.c_float(0), C.c_float(0)
        L.check(L.load().dsp_prepass_calibration(self._h, int(dtype), C.byref(err), C.byref(delta)), self._h, "dsp_prepass_calibration")
        return err.value, delta.value

    def prepass_calibration_table(self, dtype=L.PREPASS_F16):
        """dict(mags, max_err, delta: 5 entries each; guard_err): the margin as a function of the code's largest entry."""
        m, e, d = (np.zeros(5, np.float32) for _ in range(3))
        g = C.c_float(0)
        L.check(L.load().dsp_prepass_calibration_table(self._h, int(dtype), L.ptr(m), L.ptr(e), L.ptr(d), C.byref(g)), self._h,
                "dsp_prepass_calibration_table")
        return dict(mags=m, max_err=e, delta=d, guard_err=g.value)

    def prepass_reset_guard(self):
        """Forget what earlier guard trips on this engine left behind: the margins return to the decoder's calibration."""
        L.check(L.load().dsp_prepass_reset_guard(self._h), self._h, "dsp_prepass_reset_guard")

    def decode_sdf_multi(self, codes, pts):
        """(n_codes, 64) codes x one shared (n, 3) point set -> (n_codes, n) sdf, one kernel launch."""
        pts = L.f32(pts).reshape(-1, 3)
        codes = np.asarray(codes, np.float32)
        codes = L.f32(np.stack([L.code64(c) for c in codes.reshape(-1, codes.shape[-1])]))
        out = np.zeros((codes.shape[0], pts.shape[0]), np.float32)
        L.check(L.load().dsp_decode_sdf_multi(self._h, L.ptr(codes), codes.shape[0], L.ptr(pts), pts.shape[0], L.ptr(out)),
                self._h, "dsp_decode_sdf_multi")
        return out

    # -- mesh extraction ---------------------------------------------------------------------------
    def _fetch_mesh(self, nv, nf):
        verts = np.zeros((nv.value, 3), np.float32)
        faces = np.zeros((nf.value, 3), np.int32)
        L.check(L.load().dsp_mesh_fetch(self._h, L.ptr(verts), nv.value, L.ptr(faces, L.c_i32p), nf.value), self._h, "dsp_mesh_fetch")
        return verts, faces

    @staticmethod
    def _mesh_flags(regular_grid, prepass):
        """flags word of dsp_extract_mesh(es): prepass None / "off" / PREPASS_OFF, "f16" / PREPASS_F16 or "bf16" / PREPASS_BF16."""
        lp = {None: 0, "off": 0, L.PREPASS_OFF: 0, "f16": L.MESH_PREPASS_F16, L.PREPASS_F16: L.MESH_PREPASS_F16,
              "bf16": L.MESH_PREPASS_BF16, L.PREPASS_BF16: L.MESH_PREPASS_BF16}.get(prepass)
        if lp is None:
            raise ValueError("prepass must be None, 'off', 'f16' or 'bf16', not %r" % (prepass,))
        return (L.MESH_REGULAR_GRID if regular_grid else 0) | lp

    def extract_mesh(self, code, vol_dim, regular_grid=False, prepass=None):
        """Grid decode + marching cubes on the device (the SDF volume never leaves HBM): vertices (V,3) float32 in the
        decoder's [-1,1]^3 frame, faces (F,3) int32.  Empty when the surface does not cross the grid.  regular_grid=False
        samples the reference's (sheared) grid, see reconstruct.utils.create_voxel_grid.  prepass="f16" / "bf16": the grid goes
        through the low-precision prepass and only its surface band through the fp32 kernel -- the same mesh, bit for bit
        (dsp_extract_meshes)."""
        code = L.code64(code)
        nv, nf = C.c_int64(0), C.c_int64(0)
        L.check(L.load().dsp_extract_mesh(self._h, L.ptr(code), int(vol_dim), self._mesh_flags(regular_grid, prepass), C.byref(nv), C.byref(nf)),
                self._h, "dsp_extract_mesh")
        return self._fetch_mesh(nv, nf)

    def extract_meshes(self, codes, vol_dim, regular_grid=False, prepass=None, delta=0.0):
        """The meshes of n objects on one grid in a few launches (dsp_extract_meshes): a list of (vertices, faces), each equal to
        extract_mesh of that code; an object whose surface misses the grid gets empty arrays.  delta > 0 forces the prepass margin
        of every object (tests)."""
        codes = np.stack([L.code64(c) for c in codes]) if len(codes) else np.zeros((0, L.CODE_LEN), np.float32)
        n = codes.shape[0]
        if n == 0:
            return []
        nv, nf = np.zeros(n, np.int64), np.zeros(n, np.int64)
        lib = L.load()
        L.check(lib.dsp_extract_meshes(self._h, L.ptr(codes), n, int(vol_dim), self._mesh_flags(regular_grid, prepass), float(delta),
                                       L.ptr(nv, L.c_i64p), L.ptr(nf, L.c_i64p)), self._h, "dsp_extract_meshes")
        verts = np.zeros((int(nv.sum()), 3), np.float32)
        faces = np.zeros((int(nf.sum()), 3), np.int32)
        L.check(lib.dsp_meshes_fetch(self._h, n, L.ptr(nv, L.c_i64p), L.ptr(nf, L.c_i64p), L.ptr(verts), L.ptr(faces, L.c_i32p)), self._h,
                "dsp_meshes_fetch")
        ov, of = np.concatenate([[0], np.cumsum(nv)]), np.concatenate([[0], np.cumsum(nf)])
        return [(verts[ov[i]:ov[i + 1]], faces[of[i]:of[i + 1]]) for i in range(n)]

    # -- surface projection ------------------------------------------------------------------------
    def _var_codes(self, var_code, n):
        """(n, 64) float64 as the C ABI carries a code variance; shorter rows (a 32-D decoder's) are zero-padded."""
        if var_code is None:
            return None
        v = np.asarray(var_code, np.float64).reshape(n, -1)
        out = np.zeros((n, L.CODE_LEN), np.float64)
        k = min(v.shape[1], L.CODE_LEN)
        out[:, :k] = v[:, :k]
        return out

    def surface_points(self, codes, pts_list, steps=6, max_step=0.1, var_code=None):
        """Projects object i's points pts_list[i] ((n_i, 3), object frame) onto the zero set of codes[i] with `steps` capped Newton steps
        along the decoder's gradient (dsp_surface_points), all objects in one call.  A list of dicts with the keys of
        extract_meshes_refined: `vertices` (the foot points), `faces` (empty: points have none), `normals` (unit, d sdf / d xyz at the
        foot point), `sdf` there, `vertices_mc` (the points as given), and `grad_norm`, plus `sigma` (standard deviation of the surface
        along the normal) when var_code ((n, code_len), e.g. a posterior's code variance) is given.  steps=0 evaluates at the points as
        given.  max_step: the longest move of one step."""
        codes = np.stack([L.code64(c) for c in codes]) if len(codes) else np.zeros((0, L.CODE_LEN), np.float32)
        n = codes.shape[0]
        if n == 0:
            return []
        if len(pts_list) != n:
            raise ValueError("one point array per code")
        pts = [L.f32(p).reshape(-1, 3) for p in pts_list]
        off = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])]).astype(np.int64)
        flat = L.f32(np.concatenate(pts, 0)) if off[-1] else np.zeros((0, 3), np.float32)
        total = int(off[-1])
        var = self._var_codes(var_code, n)
        out_p, out_n = np.zeros((total, 3), np.float32), np.zeros((total, 3), np.float32)
        sdf, gn = np.zeros(total, np.float32), np.zeros(total, np.float32)
        sigma = np.zeros(total, np.float32) if var is not None else None
        L.check(L.load().dsp_surface_points(self._h, L.ptr(codes), n, L.ptr(off, L.c_i64p), L.ptr(flat), int(steps), float(max_step),
                                            L.ptr(var, L.c_f64p), L.ptr(out_p), L.ptr(out_n), L.ptr(sdf), L.ptr(gn), L.ptr(sigma)),
                self._h, "dsp_surface_points")
        res = []
        for i in range(n):
            s = slice(off[i], off[i + 1])
            d = {"vertices": out_p[s], "faces": np.zeros((0, 3), np.int32), "normals": out_n[s], "sdf": sdf[s], "vertices_mc": flat[s],
                 "grad_norm": gn[s]}
            if sigma is not None:
                d["sigma"] = sigma[s]
            res.append(d)
        return res

    def extract_meshes_refined(self, codes, vol_dim, steps=6, regular_grid=False, prepass=None, delta=0.0, max_step=None, var_code=None):
        """extract_meshes, then every vertex projected onto the decoder's zero set on the device (dsp_meshes_refine).  A list of dicts:
        `vertices` (refined), `faces`, `normals` (analytic, unit), `sdf` (at the refined vertices), `vertices_mc` (the marching-cubes
        vertices, what extract_meshes returns), plus `sigma` when var_code is given.  max_step None: one voxel per step."""
        codes = np.stack([L.code64(c) for c in codes]) if len(codes) else np.zeros((0, L.CODE_LEN), np.float32)
        n = codes.shape[0]
        if n == 0:
            return []
        nv, nf = np.zeros(n, np.int64), np.zeros(n, np.int64)
        lib = L.load()
        L.check(lib.dsp_extract_meshes(self._h, L.ptr(codes), n, int(vol_dim), self._mesh_flags(regular_grid, prepass), float(delta),
                                       L.ptr(nv, L.c_i64p), L.ptr(nf, L.c_i64p)), self._h, "dsp_extract_meshes")
        tv = int(nv.sum())
        verts_mc = np.zeros((tv, 3), np.float32)
        faces = np.zeros((int(nf.sum()), 3), np.int32)
        L.check(lib.dsp_meshes_fetch(self._h, n, L.ptr(nv, L.c_i64p), L.ptr(nf, L.c_i64p), L.ptr(verts_mc), L.ptr(faces, L.c_i32p)), self._h,
                "dsp_meshes_fetch")
        var = self._var_codes(var_code, n)
        L.check(lib.dsp_meshes_refine(self._h, n, L.ptr(nv, L.c_i64p), int(steps), 0.0 if max_step is None else float(max_step),
                                      L.ptr(var, L.c_f64p)), self._h, "dsp_meshes_refine")
        verts, normals, sdf = np.zeros((tv, 3), np.float32), np.zeros((tv, 3), np.float32), np.zeros(tv, np.float32)
        sigma = np.zeros(tv, np.float32) if var is not None else None
        L.check(lib.dsp_meshes_fetch_attributes(self._h, n, L.ptr(nv, L.c_i64p), L.ptr(verts), L.ptr(normals), L.ptr(sdf), L.ptr(sigma)),
                self._h, "dsp_meshes_fetch_attributes")
        ov, of = np.concatenate([[0], np.cumsum(nv)]), np.concatenate([[0], np.cumsum(nf)])
        res = []
        for i in range(n):
            s = slice(ov[i], ov[i + 1])
            d = {"vertices": verts[s], "faces": faces[of[i]:of[i + 1]], "normals": normals[s], "sdf": sdf[s], "vertices_mc": verts_mc[s]}
            if sigma is not None:
                d["sigma"] = sigma[s]
            res.append(d)
        return res

    # -- map query ---------------------------------------------------------------------------------
    def query_map(self, t_world_obj, codes, pts_world, normals=False):
        """Signed distance of world points to a map of posed objects (dsp_map_query).  t_world_obj: (n_obj, 4, 4) object-to-world Sim(3);
        codes: n_obj codes; pts_world: (n_pts, 3).  A dict: `obj` (int32, index of the object with the smallest world-scaled signed distance
        among those whose unit sphere contains the point, -1 for none), `dist` (sdf * scale of that object, +inf for none), `bound`
        (distance to the nearest unit sphere the point is outside of: dist <= bound certifies obj) and, with normals=True, `normal`
        ((n_pts, 3), the winning surface's unit outward normal in the world frame, zeros for none)."""
        t = L.f32(np.asarray(t_world_obj, np.float32).reshape(-1, 4, 4))
        n_obj = t.shape[0]
        codes = np.stack([L.code64(c) for c in codes]) if len(codes) else np.zeros((0, L.CODE_LEN), np.float32)
        if codes.shape[0] != n_obj:
            raise ValueError("one code per pose")
        pts = L.f32(np.asarray(pts_world, np.float32).reshape(-1, 3))
        n = pts.shape[0]
        out = {"obj": np.zeros(n, np.int32), "dist": np.zeros(n, np.float32), "bound": np.zeros(n, np.float32)}
        if normals:
            out["normal"] = np.zeros((n, 3), np.float32)
        L.check(L.load().dsp_map_query(self._h, L.ptr(t), L.ptr(codes), n_obj, L.ptr(pts), n, L.QUERY_NORMALS if normals else 0,
                                       L.ptr(out["obj"], L.c_i32p), L.ptr(out["dist"]), L.ptr(out["bound"]), L.ptr(out.get("normal"))),
                self._h, "dsp_map_query")
        return out

    def query_stats(self):
        """Counts of the last query_map on this engine (dsp_map_query_last_stats)."""
        c = np.zeros(4, np.int64)
        L.check(L.load().dsp_map_query_last_stats(self._h, L.ptr(c, L.c_i64p)), self._h, "dsp_map_query_last_stats")
        return {"rows": int(c[0]), "tiles": int(c[1]), "chunks": int(c[2]), "passes": int(c[3])}

    # -- ray casting -------------------------------------------------------------------------------
    @staticmethod
    def raycast_params(**params):
        """dsp_raycast_params: the library's defaults with `params` written over them.  Fields: t_min, t_max, eps, relax, max_steps."""
        prm = L.RaycastParams()
        L.load().dsp_raycast_params_default(C.byref(prm))
        names = {n for n, _ in L.RaycastParams._fields_}
        for k, v in params.items():
            if k not in names:
                raise TypeError("cast_rays: unknown parameter %r" % k)
            setattr(prm, k, int(v) if k == "max_steps" else float(v))
        return prm

    def cast_rays(self, t_world_obj, codes, origins, dirs, normals=False, **params):
        """What does the map look like from here?  The first object surface along every world ray (dsp_map_raycast).  The map as query_map
        takes it; origins, dirs: (n_rays, 3), dirs of any non-zero length; params: see raycast_params.  A dict: `obj` (int32, -1 for no
        hit), `t` (the hit's parameter in world units along the unit direction, +inf for none), `dist` (sdf * scale at the hit sample, +inf
        for none), `status` (L.RAYCAST_MISS / _HIT / _UNDECIDED) and `normal` ((n_rays, 3) world unit normals with normals=True, else
        None)."""
        t = L.f32(np.asarray(t_world_obj, np.float32).reshape(-1, 4, 4))
        n_obj = t.shape[0]
        codes = np.stack([L.code64(c) for c in codes]) if len(codes) else np.zeros((0, L.CODE_LEN), np.float32)
        if codes.shape[0] != n_obj:
            raise ValueError("one code per pose")
        org = L.f32(np.asarray(origins, np.float32).reshape(-1, 3))
        dr = L.f32(np.asarray(dirs, np.float32).reshape(-1, 3))
        n = org.shape[0]
        if dr.shape[0] != n:
            raise ValueError("one direction per origin")
        prm = self.raycast_params(**params)
        out = {"obj": np.zeros(n, np.int32), "t": np.zeros(n, np.float32), "dist": np.zeros(n, np.float32), "status": np.zeros(n, np.int32),
               "normal": np.zeros((n, 3), np.float32) if normals else None}
        L.check(L.load().dsp_map_raycast(self._h, L.ptr(t), L.ptr(codes), n_obj, L.ptr(org), L.ptr(dr), n, C.byref(prm),
                                         L.RAYCAST_NORMALS if normals else 0, L.ptr(out["obj"], L.c_i32p), L.ptr(out["t"]), L.ptr(out["dist"]),
                                         L.ptr(out["status"], L.c_i32p), L.ptr(out["normal"])), self._h, "dsp_map_raycast")
        return out

    def raycast_stats(self):
        """Counts of the last cast_rays on this engine (dsp_map_raycast_last_stats)."""
        c = np.zeros(6, np.int64)
        L.check(L.load().dsp_map_raycast_last_stats(self._h, L.ptr(c, L.c_i64p)), self._h, "dsp_map_raycast_last_stats")
        return {"pairs": int(c[0]), "rows": int(c[1]), "tiles": int(c[2]), "rounds": int(c[3]), "passes": int(c[4]), "exhausted": int(c[5])}

    # -- map alignment -----------------------------------------------------------------------------
    @staticmethod
    def align_params(**params):
        """dsp_align_params: the library's defaults with `params` written over them.  Fields: iterations, min_points, max_dist, huber, damp,
        trans_tol, rot_tol, and step_control=(lambda0, up, down, lambda_min, lambda_max) (or the five by name)."""
        prm = L.AlignParams()
        L.load().dsp_align_params_default(C.byref(prm))
        sc = params.pop("step_control", None)
        if sc is not None:
            prm.lambda0, prm.up, prm.down, prm.lambda_min, prm.lambda_max = [float(x) for x in sc]
        names = {n for n, _ in L.AlignParams._fields_}
        for k, v in params.items():
            if k not in names:
                raise TypeError("align_to_map: unknown parameter %r" % k)
            setattr(prm, k, int(v) if k in ("iterations", "min_points") else float(v))
        return prm

    def align_to_map(self, t_world_obj, codes, pts_sensor, t_world_sensor0, weights=None, trace=False, per_point=False, **params):
        """Where is the sensor?  Batched SE(3) Gauss-Newton of sensor-frame points against the map's decoded surfaces (dsp_map_align), one run
        per initial pose of t_world_sensor0 ((n_hyp, 4, 4) or (4, 4), sensor-to-world, rigid), all on the device in one call.  The map as
        query_map takes it; weights: None or (n_pts,) >= 0; params: see align_params.  A dict: `pose` (n_hyp, 4, 4) float64, `status`
        (L.ALIGN_*), `cost`, `cost0` (truncated Huber cost at the returned / the first state), `n_used`, `sum_w`, `evaluations`, `steps`,
        `lambda`, `information` (n_hyp, 6, 6: H of xi = [v, omega] at the returned state, undamped), `b` (n_hyp, 6), `best` (index of the
        lowest cost among the hypotheses with support, -1 if none has any); with per_point=True `obj` / `dist` (n_hyp, n_pts) at the returned
        state; with trace=True `trace`: a dict of per-evaluation arrays (n_hyp, iterations, ...): pose, decision, cost, lambda, n_used,
        H (6, 6), b, xi."""
        t = L.f32(np.asarray(t_world_obj, np.float32).reshape(-1, 4, 4))
        n_obj = t.shape[0]
        codes = np.stack([L.code64(c) for c in codes]) if len(codes) else np.zeros((0, L.CODE_LEN), np.float32)
        if codes.shape[0] != n_obj:
            raise ValueError("one code per pose")
        pts = L.f32(np.asarray(pts_sensor, np.float32).reshape(-1, 3))
        n = pts.shape[0]
        w = None
        if weights is not None:
            w = L.f32(np.asarray(weights, np.float32).reshape(-1))
            if w.shape[0] != n:
                raise ValueError("one weight per point")
        t0 = np.ascontiguousarray(np.asarray(t_world_sensor0, np.float64).reshape(-1, 4, 4))
        n_hyp = t0.shape[0]
        prm = self.align_params(**params)
        iters = max(int(prm.iterations), 0)
        pose, rec = np.zeros((n_hyp, 4, 4), np.float64), np.zeros((n_hyp, L.ALIGN_RECORD), np.float64)
        obj = np.zeros((n_hyp, n), np.int32) if per_point else None
        dist = np.zeros((n_hyp, n), np.float32) if per_point else None
        tr = np.zeros((n_hyp, iters, L.ALIGN_TRACE), np.float64) if trace else None
        L.check(L.load().dsp_map_align(self._h, L.ptr(t), L.ptr(codes), n_obj, L.ptr(pts), L.ptr(w), n, L.ptr(t0, L.c_f64p), n_hyp, C.byref(prm),
                                       L.ptr(pose, L.c_f64p), L.ptr(rec, L.c_f64p), L.ptr(obj, L.c_i32p), L.ptr(dist), L.ptr(tr, L.c_f64p)),
                self._h, "dsp_map_align")
        out = self._align_result(pose, rec, tr, prm, n_hyp, iters)
        if per_point:
            out["obj"], out["dist"] = obj, dist
        return out

    @staticmethod
    def _align_result(pose, rec, tr, prm, n_hyp, iters):
        """the result dict of align_to_map / align_rays_to_map from the call's record and trace arrays"""
        out = {"pose": pose, "status": rec[:, 0].astype(np.int32), "evaluations": rec[:, 1].astype(np.int32), "steps": rec[:, 2].astype(np.int32),
               "cost0": rec[:, 3].copy(), "cost": rec[:, 4].copy(), "n_used": rec[:, 5].astype(np.int64), "sum_w": rec[:, 6].copy(),
               "lambda": rec[:, 7].copy(), "information": rec[:, 8:44].reshape(n_hyp, 6, 6).copy(), "b": rec[:, 44:50].copy()}
        ok = np.flatnonzero(out["n_used"] >= prm.min_points)
        out["best"] = int(ok[np.argmin(out["cost"][ok])]) if ok.size else -1
        if tr is not None:
            iu = np.triu_indices(6)
            hh = np.zeros((n_hyp, iters, 6, 6), np.float64)
            hh[:, :, iu[0], iu[1]] = tr[:, :, 20:41]
            hh[:, :, iu[1], iu[0]] = tr[:, :, 20:41]
            out["trace"] = {"pose": tr[:, :, :16].reshape(n_hyp, iters, 4, 4).copy(), "decision": tr[:, :, 16].astype(np.int32), "cost": tr[:, :, 17].copy(),
                            "lambda": tr[:, :, 18].copy(), "n_used": tr[:, :, 19].astype(np.int64), "H": hh, "b": tr[:, :, 41:47].copy(),
                            "xi": tr[:, :, 47:53].copy()}
        return out

    def align_stats(self):
        """Counts of the last align_to_map on this engine (dsp_map_align_last_stats), summed over its evaluations."""
        c = np.zeros(5, np.int64)
        L.check(L.load().dsp_map_align_last_stats(self._h, L.ptr(c, L.c_i64p)), self._h, "dsp_map_align_last_stats")
        return {"rows": int(c[0]), "tiles": int(c[1]), "chunks": int(c[2]), "passes": int(c[3]), "evaluations": int(c[4])}

    # -- ray alignment ------------------------------------------------------------------------------
    def align_rays_to_map(self, t_world_obj, codes, pts_sensor, t_world_sensor0, origins=None, weights=None, trace=False, per_ray=False,
                          max_gap=None, raycast=None, **params):
        """Where is the sensor, given the depths it measured along its rays?  Projective SE(3) Gauss-Newton against the ray-cast map
        (dsp_map_align_rays).  pts_sensor: (n_rays, 3) measured end points in the sensor frame; origins: None (the sensor origin) or
        (n_rays, 3); the ray of an observation runs from its origin through its end point.  max_gap: the gate on |observed depth - cast
        depth| (None: the library's default, 2 max_dist; inf: no gate); raycast: a dict of raycast_params fields; everything else as
        align_to_map.  The dict of align_to_map; with per_ray=True `obj` (the matched object, -1 for unmatched), `dist` (the first-order
        signed distance), `t` and `status_ray` (the cast's hit parameter and L.RAYCAST_* status), (n_hyp, n_rays) each, at the returned state."""
        t = L.f32(np.asarray(t_world_obj, np.float32).reshape(-1, 4, 4))
        n_obj = t.shape[0]
        codes = np.stack([L.code64(c) for c in codes]) if len(codes) else np.zeros((0, L.CODE_LEN), np.float32)
        if codes.shape[0] != n_obj:
            raise ValueError("one code per pose")
        pts = L.f32(np.asarray(pts_sensor, np.float32).reshape(-1, 3))
        n = pts.shape[0]
        org = None
        if origins is not None:
            org = L.f32(np.asarray(origins, np.float32).reshape(-1, 3))
            if org.shape[0] != n:
                raise ValueError("one origin per point")
        w = None
        if weights is not None:
            w = L.f32(np.asarray(weights, np.float32).reshape(-1))
            if w.shape[0] != n:
                raise ValueError("one weight per ray")
        t0 = np.ascontiguousarray(np.asarray(t_world_sensor0, np.float64).reshape(-1, 4, 4))
        n_hyp = t0.shape[0]
        prm = self.align_params(**params)
        rprm = self.raycast_params(**(raycast or {}))
        lib = L.load()
        gap = float(lib.dsp_align_rays_default_max_gap(C.byref(prm))) if max_gap is None else float(max_gap)
        iters = max(int(prm.iterations), 0)
        pose, rec = np.zeros((n_hyp, 4, 4), np.float64), np.zeros((n_hyp, L.ALIGN_RECORD), np.float64)
        obj = np.zeros((n_hyp, n), np.int32) if per_ray else None
        dist = np.zeros((n_hyp, n), np.float32) if per_ray else None
        th = np.zeros((n_hyp, n), np.float32) if per_ray else None
        st = np.zeros((n_hyp, n), np.int32) if per_ray else None
        tr = np.zeros((n_hyp, iters, L.ALIGN_TRACE), np.float64) if trace else None
        L.check(lib.dsp_map_align_rays(self._h, L.ptr(t), L.ptr(codes), n_obj, L.ptr(pts), L.ptr(org), L.ptr(w), n, L.ptr(t0, L.c_f64p), n_hyp,
                                       C.byref(prm), C.byref(rprm), gap, L.ptr(pose, L.c_f64p), L.ptr(rec, L.c_f64p), L.ptr(obj, L.c_i32p), L.ptr(dist),
                                       L.ptr(th), L.ptr(st, L.c_i32p), L.ptr(tr, L.c_f64p)), self._h, "dsp_map_align_rays")
        out = self._align_result(pose, rec, tr, prm, n_hyp, iters)
        out["max_gap"] = gap
        if per_ray:
            out["obj"], out["dist"], out["t"], out["status_ray"] = obj, dist, th, st
        return out

    def align_rays_stats(self):
        """Counts of the last align_rays_to_map on this engine (dsp_map_align_rays_last_stats): the cast's, summed over its evaluations."""
        c = np.zeros(7, np.int64)
        L.check(L.load().dsp_map_align_rays_last_stats(self._h, L.ptr(c, L.c_i64p)), self._h, "dsp_map_align_rays_last_stats")
        return {"pairs": int(c[0]), "rows": int(c[1]), "tiles": int(c[2]), "rounds": int(c[3]), "passes": int(c[4]), "exhausted": int(c[5]),
                "evaluations": int(c[6])}

    # -- object refinement --------------------------------------------------------------------------
    def align_objects_to_rays(self, t_world_obj, codes, pts_world, origins_world, weights=None, refine=None, trace=False, per_ray=False,
                              max_gap=None, raycast=None, **params):
        """Where are the objects, given depth rays from known sensor poses?  One SE(3) correction per map object, projective Gauss-Newton
        against the ray-cast map (dsp_map_align_objects).  pts_world / origins_world: (n_rays, 3) measured end points and ray origins in
        the WORLD frame (several frames are concatenated); refine: None (all) or (n_obj,) of 0 / 1, an object with 0 is never moved but
        still occludes; max_gap, raycast, weights and params as align_rays_to_map.  The dict of align_to_map indexed by OBJECT (`pose` is
        the correction C_k, `information` the 6 x 6 information of its left perturbation), plus `t_world_obj` (n_obj, 4, 4) float32, the
        corrected poses C_k T_k0 (the input bytes where C_k is the identity), `correction` (n_obj, 4, 4) float64 and `max_gap`; with
        per_ray=True `obj`, `dist`, `t`, `status_ray` (n_rays,) from one more evaluation of the returned map."""
        t = L.f32(np.asarray(t_world_obj, np.float32).reshape(-1, 4, 4))
        n_obj = t.shape[0]
        codes = np.stack([L.code64(c) for c in codes]) if len(codes) else np.zeros((0, L.CODE_LEN), np.float32)
        if codes.shape[0] != n_obj:
            raise ValueError("one code per pose")
        pts = L.f32(np.asarray(pts_world, np.float32).reshape(-1, 3))
        n = pts.shape[0]
        org = None
        if origins_world is not None:
            org = L.f32(np.asarray(origins_world, np.float32).reshape(-1, 3))
            if org.shape[0] != n:
                raise ValueError("one origin per point")
        w = None
        if weights is not None:
            w = L.f32(np.asarray(weights, np.float32).reshape(-1))
            if w.shape[0] != n:
                raise ValueError("one weight per ray")
        ref = None
        if refine is not None:
            ref = np.ascontiguousarray(np.asarray(refine).reshape(-1) != 0, np.uint8)
            if ref.shape[0] != n_obj:
                raise ValueError("one refine flag per object")
        prm = self.align_params(**params)
        rprm = self.raycast_params(**(raycast or {}))
        lib = L.load()
        gap = float(lib.dsp_align_rays_default_max_gap(C.byref(prm))) if max_gap is None else float(max_gap)
        iters = max(int(prm.iterations), 0)
        t_out, corr = np.zeros((n_obj, 4, 4), np.float32), np.zeros((n_obj, 4, 4), np.float64)
        rec = np.zeros((n_obj, L.ALIGN_RECORD), np.float64)
        obj = np.zeros(n, np.int32) if per_ray else None
        dist = np.zeros(n, np.float32) if per_ray else None
        th = np.zeros(n, np.float32) if per_ray else None
        st = np.zeros(n, np.int32) if per_ray else None
        tr = np.zeros((n_obj, iters, L.ALIGN_TRACE), np.float64) if trace else None
        L.check(lib.dsp_map_align_objects(self._h, L.ptr(t), L.ptr(codes), n_obj, L.ptr(pts), L.ptr(org), L.ptr(w), n, L.ptr(ref, C.POINTER(C.c_uint8)),
                                          C.byref(prm), C.byref(rprm), gap, L.ptr(t_out), L.ptr(corr, L.c_f64p), L.ptr(rec, L.c_f64p),
                                          L.ptr(obj, L.c_i32p), L.ptr(dist), L.ptr(th), L.ptr(st, L.c_i32p), L.ptr(tr, L.c_f64p)),
                self._h, "dsp_map_align_objects")
        out = self._align_result(corr, rec, tr, prm, n_obj, iters)
        out["t_world_obj"], out["correction"], out["max_gap"] = t_out, corr, gap
        if per_ray:
            out["obj"], out["dist"], out["t"], out["status_ray"] = obj, dist, th, st
        return out

    def align_objects_stats(self):
        """Counts of the last align_objects_to_rays on this engine (dsp_map_align_objects_last_stats): the cast's, summed over its
        evaluations, the one behind the per-ray outputs included."""
        c = np.zeros(7, np.int64)
        L.check(L.load().dsp_map_align_objects_last_stats(self._h, L.ptr(c, L.c_i64p)), self._h, "dsp_map_align_objects_last_stats")
        return {"pairs": int(c[0]), "rows": int(c[1]), "tiles": int(c[2]), "rounds": int(c[3]), "passes": int(c[4]), "exhausted": int(c[5]),
                "evaluations": int(c[6])}

    # -- shape refinement ---------------------------------------------------------------------------
    UNKNOWNS = {"code": L.SHAPES_CODE, "pose": L.SHAPES_POSE, "pose+code": L.SHAPES_CODE | L.SHAPES_POSE, "code+pose": L.SHAPES_CODE | L.SHAPES_POSE}

    @classmethod
    def shapes_params(cls, unknowns="code", code_reg=None, code_anchor=None, code_tol=None, **params):
        """(dsp_align_params, dsp_shapes_params) of align_shapes_to_rays: dsp_shapes_params_default's values (align_params' but damp 1e-4;
        code only, no regulariser, code_tol 1e-6) with the arguments written over them."""
        sp = L.ShapesParams()
        dflt = L.AlignParams()
        L.load().dsp_shapes_params_default(C.byref(dflt), C.byref(sp))
        params.setdefault("damp", dflt.damp)
        prm = cls.align_params(**params)
        if unknowns not in cls.UNKNOWNS:
            raise ValueError("unknowns must be 'code', 'pose' or 'pose+code'")
        sp.unknowns = cls.UNKNOWNS[unknowns]
        for name, v in (("code_reg", code_reg), ("code_anchor", code_anchor), ("code_tol", code_tol)):
            if v is not None:
                setattr(sp, name, float(v))
        return prm, sp

    def align_shapes_to_rays(self, t_world_obj, codes, pts_world, origins_world, weights=None, refine=None, trace=False, per_ray=False,
                             max_gap=None, raycast=None, unknowns="code", code_reg=None, code_anchor=None, code_tol=None, **params):
        """What shape do the objects have, given depth rays from known sensor poses?  One 70-dimensional Gauss-Newton system per map object
        -- 6 pose and 64 code unknowns -- against the ray-cast map (dsp_map_align_shapes).  Rays, weights, refine, max_gap, raycast and
        params as align_objects_to_rays (damp defaults to 1e-4, on the mean system); unknowns: "code", "pose" or "pose+code"; code_reg:
        weight of |z|^2, code_anchor: weight of |z - z_input|^2 (both 0 by default); code_tol: the code's convergence tolerance.  The dict of
        align_objects_to_rays plus `codes` (n_obj, 64) float32, with `information` (n_obj, 70, 70) and `b` (n_obj, 70) the raw sums of
        x = [v, omega, dz]; the trace holds pose, code, decision, cost, lambda, n_used and dx (70)."""
        t = L.f32(np.asarray(t_world_obj, np.float32).reshape(-1, 4, 4))
        n_obj = t.shape[0]
        codes = np.stack([L.code64(c) for c in codes]) if len(codes) else np.zeros((0, L.CODE_LEN), np.float32)
        if codes.shape[0] != n_obj:
            raise ValueError("one code per pose")
        pts = L.f32(np.asarray(pts_world, np.float32).reshape(-1, 3))
        n = pts.shape[0]
        org = None
        if origins_world is not None:
            org = L.f32(np.asarray(origins_world, np.float32).reshape(-1, 3))
            if org.shape[0] != n:
                raise ValueError("one origin per point")
        w = None
        if weights is not None:
            w = L.f32(np.asarray(weights, np.float32).reshape(-1))
            if w.shape[0] != n:
                raise ValueError("one weight per ray")
        ref = None
        if refine is not None:
            ref = np.ascontiguousarray(np.asarray(refine).reshape(-1) != 0, np.uint8)
            if ref.shape[0] != n_obj:
                raise ValueError("one refine flag per object")
        prm, sp = self.shapes_params(unknowns, code_reg, code_anchor, code_tol, **params)
        rprm = self.raycast_params(**(raycast or {}))
        lib = L.load()
        gap = float(lib.dsp_align_rays_default_max_gap(C.byref(prm))) if max_gap is None else float(max_gap)
        iters = max(int(prm.iterations), 0)
        D = L.SHAPES_DIM
        t_out, corr = np.zeros((n_obj, 4, 4), np.float32), np.zeros((n_obj, 4, 4), np.float64)
        c_out = np.zeros((n_obj, L.CODE_LEN), np.float32)
        rec = np.zeros((n_obj, L.SHAPES_RECORD), np.float64)
        obj = np.zeros(n, np.int32) if per_ray else None
        dist = np.zeros(n, np.float32) if per_ray else None
        th = np.zeros(n, np.float32) if per_ray else None
        st = np.zeros(n, np.int32) if per_ray else None
        tr = np.zeros((n_obj, iters, L.SHAPES_TRACE), np.float64) if trace else None
        L.check(lib.dsp_map_align_shapes(self._h, L.ptr(t), L.ptr(codes), n_obj, L.ptr(pts), L.ptr(org), L.ptr(w), n, L.ptr(ref, C.POINTER(C.c_uint8)),
                                         C.byref(prm), C.byref(sp), C.byref(rprm), gap, L.ptr(t_out), L.ptr(c_out), L.ptr(corr, L.c_f64p),
                                         L.ptr(rec, L.c_f64p), L.ptr(obj, L.c_i32p), L.ptr(dist), L.ptr(th), L.ptr(st, L.c_i32p), L.ptr(tr, L.c_f64p)),
                self._h, "dsp_map_align_shapes")
        out = {"pose": corr, "status": rec[:, 0].astype(np.int32), "evaluations": rec[:, 1].astype(np.int32), "steps": rec[:, 2].astype(np.int32),
               "cost0": rec[:, 3].copy(), "cost": rec[:, 4].copy(), "n_used": rec[:, 5].astype(np.int64), "sum_w": rec[:, 6].copy(),
               "lambda": rec[:, 7].copy(), "information": rec[:, 8:8 + D * D].reshape(n_obj, D, D).copy(), "b": rec[:, 8 + D * D:].copy()}
        ok = np.flatnonzero(out["n_used"] >= prm.min_points)
        out["best"] = int(ok[np.argmin(out["cost"][ok])]) if ok.size else -1
        if tr is not None:
            out["trace"] = {"pose": tr[:, :, :16].reshape(n_obj, iters, 4, 4).copy(), "code": tr[:, :, 16:80].copy(), "decision": tr[:, :, 80].astype(np.int32),
                            "cost": tr[:, :, 81].copy(), "lambda": tr[:, :, 82].copy(), "n_used": tr[:, :, 83].astype(np.int64), "dx": tr[:, :, 84:].copy()}
        out["t_world_obj"], out["correction"], out["codes"], out["max_gap"] = t_out, corr, c_out, gap
        if per_ray:
            out["obj"], out["dist"], out["t"], out["status_ray"] = obj, dist, th, st
        return out

    def align_shapes_stats(self):
        """Counts of the last align_shapes_to_rays on this engine (dsp_map_align_shapes_last_stats), laid out as align_objects_stats'."""
        c = np.zeros(7, np.int64)
        L.check(L.load().dsp_map_align_shapes_last_stats(self._h, L.ptr(c, L.c_i64p)), self._h, "dsp_map_align_shapes_last_stats")
        return {"pairs": int(c[0]), "rows": int(c[1]), "tiles": int(c[2]), "rounds": int(c[3]), "passes": int(c[4]), "exhausted": int(c[5]),
                "evaluations": int(c[6])}

    def mesh_stats(self):
        """Counts of the last mesh extraction on this engine (dsp_mesh_last_stats)."""
        c = np.zeros(5, np.int64)
        e = C.c_float(0.0)
        L.check(L.load().dsp_mesh_last_stats(self._h, L.ptr(c, L.c_i64p), C.byref(e)), self._h, "dsp_mesh_last_stats")
        return {"prepass_points": int(c[0]), "band_points": int(c[1]), "audit_points": int(c[2]), "dense_points": int(c[3]),
                "reruns": int(c[4]), "max_guard_err": float(e.value)}

    def marching_cubes(self, volume, level=0.0, spacing=1.0, origin=0.0):
        """Marching cubes of a host volume on the device: vertices = index * spacing + origin."""
        vol = L.f32(volume)
        if vol.ndim != 3:
            raise ValueError("volume must be 3-D")
        nv, nf = C.c_int64(0), C.c_int64(0)
        L.check(L.load().dsp_marching_cubes(self._h, L.ptr(vol), vol.shape[0], vol.shape[1], vol.shape[2], float(level), float(spacing),
                                            float(origin), C.byref(nv), C.byref(nf)), self._h, "dsp_marching_cubes")
        return self._fetch_mesh(nv, nf)

    def sdf_jacobian(self, code, pts):
        pts = L.f32(pts).reshape(-1, 3)
        code = L.code64(code)
        n = pts.shape[0]
        sdf = np.zeros(n, np.float32)
        grad = np.zeros((n, L.GRAD_DIM), np.float32)
        L.check(L.load().dsp_sdf_jacobian(self._h, L.ptr(code), L.ptr(pts), n, L.ptr(sdf), L.ptr(grad)), self._h, "dsp_sdf_jacobian")
        if self.code_len != L.CODE_LEN:     # d/d[code(code_len), xyz]: drop the unused code columns
            grad = np.ascontiguousarray(np.concatenate([grad[:, :self.code_len], grad[:, L.CODE_LEN:]], 1))
        return sdf, grad

    def sdf_jacobian_lp(self, code, pts, dtype=L.COMPUTE_F16):
        """sdf and d sdf / d [code, xyz] through the 16-bit jacobian kernels of the low-precision compute mode (accuracy measurements)."""
        pts = L.f32(pts).reshape(-1, 3)
        code = L.code64(code)
        n = pts.shape[0]
        sdf = np.zeros(n, np.float32)
        grad = np.zeros((n, L.GRAD_DIM), np.float32)
        L.check(L.load().dsp_sdf_jacobian_lp(self._h, int(dtype), L.ptr(code), L.ptr(pts), n, L.ptr(sdf), L.ptr(grad)), self._h, "dsp_sdf_jacobian_lp")
        if self.code_len != L.CODE_LEN:
            grad = np.ascontiguousarray(np.concatenate([grad[:, :self.code_len], grad[:, L.CODE_LEN:]], 1))
        return sdf, grad

    # -- residual terms -----------------------------------------------------------------------------
    def compute_sdf_loss(self, pts_cam, t_obj_cam, code):
        pts = L.f32(pts_cam).reshape(-1, 3)
        n = pts.shape[0]
        t = L.f32(t_obj_cam).reshape(4, 4)
        code = L.code64(code)
        j7 = np.zeros((n, 7), np.float32)
        jc = np.zeros((n, L.CODE_LEN), np.float32)
        r = np.zeros(n, np.float32)
        L.check(L.load().dsp_compute_sdf_loss(self._h, L.ptr(pts), n, L.ptr(t), L.ptr(code), L.ptr(j7), L.ptr(jc), L.ptr(r)),
                self._h, "dsp_compute_sdf_loss")
        return j7, jc[:, :self.code_len], r

    def compute_render_loss(self, rays, depth_obs, t_obj_cam, sampled_depth, code, th=0.01):
        rays = L.f32(rays).reshape(-1, 3)
        depth_obs = L.f32(depth_obs).reshape(-1)
        sampled = L.f32(sampled_depth).reshape(-1)
        t = L.f32(t_obj_cam).reshape(4, 4)
        code = L.code64(code)
        cap = rays.shape[0] * sampled.shape[0]
        j7 = np.zeros((cap, 7), np.float32)
        jc = np.zeros((cap, L.CODE_LEN), np.float32)
        r = np.zeros(cap, np.float32)
        k = C.c_int64(0)
        v = C.c_int64(0)
        m = C.c_int64(0)
        L.check(L.load().dsp_compute_render_loss(self._h, L.ptr(rays), rays.shape[0], L.ptr(depth_obs), L.ptr(t), L.ptr(sampled),
                                                 sampled.shape[0], L.ptr(code), float(th), C.byref(k), L.ptr(j7), L.ptr(jc),
                                                 L.ptr(r), C.byref(v), C.byref(m)), self._h, "dsp_compute_render_loss")
        stats = dict(V=v.value, m=m.value, K=k.value)
        if k.value < 0:
            return None, stats
        return (j7[:k.value].copy(), jc[:k.value, :self.code_len].copy(), r[:k.value].copy()), stats

    # -- optimiser ----------------------------------------------------------------------------------
    def fail_alloc(self, n):
        """Testing: the (n + 1)-th fresh device allocation of this handle's pool from now on fails like an exhausted HBM (n < 0: off)."""
        L.check(L.load().dsp_debug_fail_alloc(self._h, int(n)), self._h, "dsp_debug_fail_alloc")

    def trim(self):
        """Hand the handle's cached device blocks and pinned staging buffers back to the runtime (dsp_trim): for a process that shares the
        GPU with torch / RCCL / another handle and has just finished a large one-shot batch."""
        L.check(L.load().dsp_trim(self._h), self._h, "dsp_trim")

    def set_stream_priority(self, priority):
        """1 = highest, 0 = default, -1 = lowest queue priority of the handle's HIP stream (dsp_set_stream_priority): who yields on a shared GPU."""
        L.check(L.load().dsp_set_stream_priority(self._h, int(priority)), self._h, "dsp_set_stream_priority")

    def debug_lie(self, kind, x, n_depth=50):
        """Testing: exp_sim3 (kind 0, x[7]), exp_se3 (1, x[6]), the rotation prior + derived state (2, t_obj_cam 4x4) or the Sim(3) state
        update exp_sim3(dx) @ t_obj_cam (3, 16 + 7 floats) evaluated by the device functions the solve kernel calls.  Returns 16 floats."""
        x = L.f32(np.asarray(x, np.float32).reshape(-1))
        out = np.zeros(16, np.float32)
        L.check(L.load().dsp_debug_lie(self._h, int(kind), L.ptr(x), int(n_depth), L.ptr(out)), self._h, "dsp_debug_lie")
        return out

    def batch(self, prm, t_cam_obj, pts, rays, depth, codes=None, trace=False):
        return Batch(self, prm, t_cam_obj, pts, rays, depth, codes, trace)

    def pose_batch(self, prm, t_co_se3, scale, pts, codes, trace=False):
        """The pose-only batch of estimate_pose_batch, device-resident (dsp_batch_create_pose): run / results / set_iterations / trace /
        set_start_state(t_obj_cam) work on it; results()[0] is estimate_pose_batch's output, bit for bit."""
        return Batch(self, prm, t_co_se3, pts, None, None, codes, trace, scale=scale)

    def reconstruct_batch(self, prm, t_cam_obj, pts, rays, depth, codes=None, compute=L.COMPUTE_F32, convergence=None, step_control=None, posterior=None,
                          unknowns=None, obs_weights=None, report=None, prior=None):
        """compute: L.COMPUTE_F32 (default, the parity path) or the opt-in low-precision mode L.COMPUTE_F16 / _BF16 (dsp_batch_set_compute).
        convergence: None (every object runs every iteration) or (pose_tol, code_tol[, min_iterations]) -- Batch.set_convergence.
        posterior: None, "mean" / "sum" or (level, weights) -- Batch.set_posterior; the call then returns a fifth item, Batch.posterior()
        (the first four are bit for bit those of the call without it).
        prior: None, or dict(t_obj_cam, code, Lambda) / (t_obj_cam0, code0, Lambda) of per-object arrays -- Batch.set_prior; the call then
        returns Batch.prior_residual() as its LAST item (behind the posterior, where both are asked for).
        step_control: None (off), True (the defaults), a dict of Batch.set_step_control's keyword arguments or a (lambda0, up, down,
        lambda_min, lambda_max) tuple; the returned items are the same, `loss` is then the loss AT the returned state.
        report: None / False, or True -- Batch.set_report; the call then returns Batch.report() behind the posterior (in front of the prior's
        residual, which stays last).
        obs_weights: None, or (pt_w, ray_w) -- Batch.set_observation_weights; the returned items are the same.
        unknowns: None, or what Batch.set_unknowns takes (a mask, or the names of the live groups); the returned items are the same."""
        if len(pts) == 0:      # an empty shard (more ranks than objects): nothing to run, but the caller still joins the gather
            empty = (np.zeros((0, 4, 4), np.float32), np.zeros((0, self.code_len), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))
            return empty + (() if posterior is None else ({},)) + (({},) if report else ()) + (() if prior is None else ({},))
        b = Batch(self, prm, t_cam_obj, pts, rays, depth, codes)
        try:
            if compute != L.COMPUTE_F32:
                b.set_compute(compute)
            if unknowns is not None:
                b.set_unknowns(unknowns)
            return _run_resident(b, convergence, posterior, prior, step_control, report, obs_weights)
        finally:
            b.close()

    def multiview_batch(self, prm, t_cam_obj, views, codes=None, trace=False):
        """Device-resident multi-view batch: views[i] = the list of dict(t_ref_cam, pts, rays, depth) of object i (MultiviewBatch)."""
        return MultiviewBatch(self, prm, t_cam_obj, views, codes, trace)

    def reconstruct_multiview_batch(self, prm, t_cam_obj, views, codes=None, convergence=None, posterior=None, unknowns=None, obs_weights=None, report=None,
                                    prior=None):
        """dsp_reconstruct_multiview: one pose and one code per object from all its views -> (t_cam_obj, code, loss, status) per object.
        convergence: (pose_tol, code_tol[, min_iterations]) runs a resident batch with that rule (Batch.set_convergence) instead of the one-shot call.
        posterior, report, prior: as reconstruct_batch (a resident batch too; further items, per object -- the report's rows per VIEW).
        obs_weights: as reconstruct_batch, per VIEW (a resident batch too).  unknowns: as reconstruct_batch, per OBJECT (a resident batch too)."""
        n = len(views)
        if n == 0:
            empty = (np.zeros((0, 4, 4), np.float32), np.zeros((0, self.code_len), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))
            return empty + (() if posterior is None else ({},)) + (({},) if report else ()) + (() if prior is None else ({},))
        if convergence is not None or posterior is not None or prior is not None or report or obs_weights is not None or unknowns is not None:
            b = MultiviewBatch(self, prm, t_cam_obj, views, codes)
            try:
                if unknowns is not None:
                    b.set_unknowns(unknowns)
                return _run_resident(b, convergence, posterior, prior, None, report, obs_weights)
            finally:
                b.close()
        vo, t_ref, pts, rays, depth = _flatten_views(views)
        (po, p), (ro, r), (do, d) = _ragged(pts, 3), _ragged(rays, 3), _ragged(depth, 0)
        t = L.f32(np.stack([np.asarray(x, np.float32).reshape(4, 4) for x in t_cam_obj]))
        c = None if codes is None else L.f32(np.stack([L.code64(x) for x in codes]))
        t_out = np.zeros((n, 4, 4), np.float32)
        code = np.zeros((n, L.CODE_LEN), np.float32)
        loss = np.zeros(n, np.float32)
        status = np.zeros(n, np.int32)
        L.check(L.load().dsp_reconstruct_multiview(self._h, C.byref(prm), n, L.ptr(vo, L.c_i64p), L.ptr(t_ref), L.ptr(po, L.c_i64p), L.ptr(p),
                                                   L.ptr(ro, L.c_i64p), L.ptr(r), L.ptr(do, L.c_i64p), L.ptr(d), L.ptr(t), L.ptr(c), L.ptr(t_out),
                                                   L.ptr(code), L.ptr(loss), L.ptr(status, L.c_i32p)), self._h, "dsp_reconstruct_multiview")
        return t_out, np.ascontiguousarray(code[:, :self.code_len]), loss, status

    def estimate_pose_batch(self, prm, t_co_se3, scale, pts, codes, convergence=None, posterior=None, unknowns=None, obs_weights=None, report=None, prior=None):
        """convergence: (pose_tol, code_tol[, min_iterations]) (code_tol is ignored) runs a resident pose batch with that rule instead of the
        one-shot call.  posterior: as reconstruct_batch (a resident batch too); the call then returns (poses, Batch.posterior()).
        report: as reconstruct_batch; Batch.report() follows the posterior (the alive bits are the inlier filter's mask).
        prior: as reconstruct_batch, with (6, 6) Lambdas and t_obj_cam0 carrying the scale; Batch.prior_residual() is then the last item.
        obs_weights: as reconstruct_batch (a resident batch too); the ray weights are ignored.
        unknowns: as reconstruct_batch, with (n, 6) masks or the pose groups (a resident batch too)."""
        n = len(pts)
        if n == 0:
            extra = (() if posterior is None else ({},)) + (({},) if report else ()) + (() if prior is None else ({},))
            return np.zeros((0, 4, 4), np.float32) if not extra else (np.zeros((0, 4, 4), np.float32),) + extra
        if convergence is not None or posterior is not None or prior is not None or report or obs_weights is not None or unknowns is not None:
            b = self.pose_batch(prm, t_co_se3, scale, pts, codes)
            try:
                if unknowns is not None:
                    b.set_unknowns(unknowns)
                res = _run_resident(b, convergence, posterior, prior, None, report, obs_weights)
                return res[0] if len(res) == 4 else (res[0],) + res[4:]
            finally:
                b.close()
        po, p = _ragged(pts, 3)
        t = L.f32(np.stack([np.asarray(x, np.float32).reshape(4, 4) for x in t_co_se3]))
        sc = L.f32(np.asarray(scale, np.float32).reshape(n))
        cd = L.f32(np.stack([L.code64(c) for c in codes]))
        out = np.zeros((n, 4, 4), np.float32)
        L.check(L.load().dsp_estimate_pose_batch(self._h, C.byref(prm), n, L.ptr(po, L.c_i64p), L.ptr(p), L.ptr(t), L.ptr(sc),
                                                 L.ptr(cd), L.ptr(out)), self._h, "dsp_estimate_pose_batch")
        return out

    def close(self):
        if self._h:
            for b in list(self._batches):      # dsp_batch_destroy takes the handle's mutex: never after dsp_destroy
                b.close()
            L.load().dsp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
