"""Optimizer / MeshExtractor -- mirror of reference reconstruct/optimizer.py:26-223.

Same constructor arguments, method names, argument meaning and result fields as the reference, so that
DSP-SLAM's C++ (src/LocalMapping.cc:38-40; src/LocalMapping_util.cc:109-110,179-196,391-426) can call it
unchanged.  The whole Gauss-Newton loop (all iterations) runs on the MI355X inside libdspgn with no host
round trip; `reconstruct_objects` / `estimate_poses_cam_obj` are the batched forms (new, for many
independent objects per call).
"""
import numpy as np
import torch

from reconstruct.utils import ForceKeyErrorDict, create_voxel_grid, convert_sdf_voxels_to_mesh
from reconstruct.loss_utils import get_time
from dsp_slam_amd import engine as _engine
from dsp_slam_amd import _lib as _L
from dsp_slam_amd import observations as _observations


def _f32(a):
    """Eigen hands over Fortran-ordered float32 copies (pybind11 eigen caster); accept any strides / dtype."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


class Optimizer(object):
    def __init__(self, decoder, configs):
        # Attribute names are the reference's (optimizer.py:27-43): C++ reads `code_len` (LocalMapping_util.cc:413), scripts read the rest.
        self.decoder = decoder
        optim_cfg = configs.optimizer
        joint = optim_cfg.joint_optim
        for attr, key in (("k1", "k1"), ("k2", "k2"), ("k3", "k3"), ("k4", "k4"), ("b1", "b1"), ("b2", "b2"), ("lr", "learning_rate"),
                          ("s_damp", "scale_damping"), ("num_iterations_joint_optim", "num_iterations")):
            setattr(self, attr, joint[key])            # KeyError on a missing key, as attribute access on the reference's config dict (utils.py:82-84)
        for attr, key in (("code_len", "code_len"), ("num_depth_samples", "num_depth_samples"), ("cut_off", "cut_off_threshold")):
            setattr(self, attr, optim_cfg[key])
        # only the KITTI configuration carries a pose-only block; elsewhere the reference hard-codes five iterations (:41-43)
        self.num_iterations_pose_only = optim_cfg.pose_only_optim.num_iterations if configs.data_type == "KITTI" else 5
        if self.code_len not in (32, _L.CODE_LEN):      # the two code lengths the reference's C++ casts (LocalMapping_util.cc:413-423)
            raise NotImplementedError("the MI355X decoder kernels are built for 64-D and 32-D codes (got %d)" % self.code_len)
        if decoder is not None and self.code_len != getattr(decoder, "latent_size", self.code_len):
            raise ValueError("optimizer.code_len (%d) does not match the decoder's CodeLength (%d)" % (self.code_len, decoder.latent_size))
        self.verbose = True
        # ADDITION (not in the reference's configs): "compute_dtype": "f16" | "bf16" under "optimizer" opts into the low-precision compute mode
        # (dsp_batch_set_compute: 16-bit MFMA operands, fp32 accumulation -- NOT the parity path; include/dsp_gn.h).  Absent: fp32.
        try:
            dt = optim_cfg["compute_dtype"] if "compute_dtype" in optim_cfg else "f32"
        except TypeError:
            dt = "f32"
        if dt not in ("f32", "f16", "bf16"):
            raise ValueError("optimizer.compute_dtype must be f32, f16 or bf16 (got %r)" % (dt,))
        self.compute = {"f32": _L.COMPUTE_F32, "f16": _L.COMPUTE_F16, "bf16": _L.COMPUTE_BF16}[dt]
        # ADDITION (not in the reference's configs): "pose_tolerance" / "code_tolerance" under "joint_optim" and "pose_tolerance" under
        # "pose_only_optim" switch the per-object convergence rule on (dsp_batch_convergence: an object stops iterating once its step is
        # below the tolerances).  Read with a membership test -- the reference's config dict raises on a missing key -- and absent means off:
        # every object runs every iteration, as in the reference.  One joint tolerance alone leaves the other half of the rule off (inf).
        def optional(block, key):
            try:
                return float(block[key]) if key in block else None
            except TypeError:
                return None
        jp, jc = optional(joint, "pose_tolerance"), optional(joint, "code_tolerance")
        self.convergence_joint = None if jp is None and jc is None else (float("inf") if jp is None else jp, float("inf") if jc is None else jc)
        pp = None
        try:
            if "pose_only_optim" in optim_cfg:
                pp = optional(optim_cfg["pose_only_optim"], "pose_tolerance")
        except TypeError:
            pp = None
        self.convergence_pose_only = None if pp is None else (pp, 0.0)
        # ADDITION (not in the reference's configs): "posterior": "mean" | "sum" under "joint_optim" / "pose_only_optim" switches the posterior
        # pass on (dsp_batch_posterior: pose information and covariance, code variance and the loss AT the returned state; the reference's
        # fields stay bit for bit what they are without it).  Read with a membership test like the tolerances; absent means off.
        def optional_weights(block, where):
            try:
                w = block["posterior"] if "posterior" in block else None
            except TypeError:
                return None
            if w is not None and w not in ("mean", "sum"):
                raise ValueError("optimizer.%s.posterior must be 'mean' or 'sum' (got %r)" % (where, w))
            return w
        self.posterior_joint = optional_weights(joint, "joint_optim")
        self.posterior_pose_only = None
        try:
            if "pose_only_optim" in optim_cfg:
                self.posterior_pose_only = optional_weights(optim_cfg["pose_only_optim"], "pose_only_optim")
        except TypeError:
            pass
        # ADDITION (not in the reference's configs): "step_control" under "joint_optim" switches Levenberg-Marquardt step control on
        # (dsp_batch_step_control): true (Batch.set_step_control's defaults), a dict of its keyword arguments, or a list [lambda0, up, down,
        # lambda_min, lambda_max].  Read with a membership test like the keys above; absent or false means off.  Single-view joint runs only
        # (reconstruct_object / reconstruct_objects): a multi-view batch has no step control.
        try:
            sc = joint["step_control"] if "step_control" in joint else None
        except TypeError:
            sc = None
        if sc is not None and sc is not False and sc is not True:
            allowed = ("lambda0", "up", "down", "lambda_min", "lambda_max")
            if hasattr(sc, "keys"):
                sc = {k: float(sc[k]) for k in sc.keys()}
                if not set(sc) <= set(allowed):
                    raise ValueError("optimizer.joint_optim.step_control takes the keys %s (got %r)" % (", ".join(allowed), sorted(sc)))
            else:
                sc = tuple(float(v) for v in sc)
                if len(sc) != 5:
                    raise ValueError("optimizer.joint_optim.step_control as a list is [lambda0, up, down, lambda_min, lambda_max]")
        self.step_control_joint = None if sc is None or sc is False else sc
        # ADDITION (not in the reference's configs): "report": true under "joint_optim" / "pose_only_optim" switches the observation report on
        # (dsp_batch_report): every surface point and ray evaluated once more at the returned state; good results then carry `observations`,
        # the object's rows (dsp_slam_amd.observations reads them).  Read with a membership test like the keys above; absent or false means off.
        def optional_flag(block):
            try:
                return bool(block["report"]) if "report" in block else False
            except TypeError:
                return False
        self.report_joint = optional_flag(joint)
        self.report_pose_only = False
        try:
            if "pose_only_optim" in optim_cfg:
                self.report_pose_only = optional_flag(optim_cfg["pose_only_optim"])
        except TypeError:
            pass

        # ADDITION (not in the reference's configs): "unknowns": [group, ...] under "joint_optim" / "pose_only_optim" names the LIVE groups of
        # unknowns (dsp_batch_unknowns; dsp_slam_amd.engine.unknowns_mask: translation, rotation, yaw, scale, pose, code, all); every other
        # entry is frozen at its start value.  Read with a membership test like the keys above; absent means every entry is live.  An
        # unknown name raises ValueError here, not at the first call.
        def optional_groups(block, pose_only):
            try:
                g = block["unknowns"] if "unknowns" in block else None
            except TypeError:
                return None
            if g is None:
                return None
            g = [g] if isinstance(g, str) else [str(x) for x in g]
            _engine.unknowns_mask(g, pose_only)
            return g
        self.unknowns_joint = optional_groups(joint, False)
        self.unknowns_pose_only = None
        try:
            if "pose_only_optim" in optim_cfg:
                self.unknowns_pose_only = optional_groups(optim_cfg["pose_only_optim"], True)
        except TypeError:
            pass

    def _params(self):
        return _engine.gn_params(self.k1, self.k2, self.k3, self.k4, self.b1, self.b2, self.lr, self.s_damp,
                                 self.num_iterations_joint_optim, self.num_depth_samples, self.cut_off,
                                 self.num_iterations_pose_only)

    # ---- pose only (reference optimizer.py:45-86) ---------------------------------------------------
    @staticmethod
    def _stack_priors(priors, n_unknowns, code_len):
        """[dict(t_obj_cam, code, Lambda) or None per object] -> the per-object arrays Engine's prior= takes; None = no prior (Lambda 0)."""
        t0 = np.tile(np.eye(4, dtype=np.float32), (len(priors), 1, 1))
        z0 = np.zeros((len(priors), 64), np.float32)
        lam = np.zeros((len(priors), n_unknowns, n_unknowns))
        for i, p in enumerate(priors):
            if p is None:
                continue
            t0[i] = _f32(p["t_obj_cam"]).reshape(4, 4)
            if n_unknowns > 6:
                c = _f32(p["code"]).reshape(-1)[:code_len]
                z0[i, :c.shape[0]] = c
            lam[i] = _engine._prior_lambda(p["Lambda"], n_unknowns)
        return dict(t_obj_cam=t0, code=z0, Lambda=lam)

    @staticmethod
    def _stack_obs_weights(obs_weights, pts_list, rays_list):
        """[(pt_w, ray_w) or None per object] -> the per-member lists Engine's obs_weights= takes; None (or a None half) = all ones."""
        pw, rw = [], []
        for i, w in enumerate(obs_weights):
            p, r = (None, None) if w is None else w
            pw.append(np.ones(len(pts_list[i]), np.float32) if p is None else _f32(p).reshape(-1))
            if rays_list is not None:
                rw.append(np.ones(len(rays_list[i]), np.float32) if r is None else _f32(r).reshape(-1))
        return pw, (rw if rays_list is not None else None)

    def estimate_poses_cam_obj(self, t_co_se3_list, scales, pts_list, codes, return_posterior=False, unknowns=None, obs_weights=None, priors=None):
        """Batched form: lists of per-object inputs -> (B,4,4) float32 array of optimised SE(3) poses.  return_posterior=True: (poses,
        Batch.posterior() dict) -- 6 x 6 pose information / covariance per object, with the weights of pose_only_optim.posterior ("mean" if absent).
        priors: None, or one dict(t_obj_cam (4, 4) with the scale in it, Lambda (6, 6)) or None per object (dsp_batch_prior); the call then
        returns Batch.prior_residual() as its last item.  With pose_only_optim.report set the call returns Batch.report() (per-point sdf and
        the inlier filter's alive bits) behind the posterior, in front of the prior's residual.  obs_weights: None, or one (pt_w, None) or
        None per object -- per-point weights (dsp_batch_observation_weights).  unknowns: None (pose_only_optim.unknowns, or every entry), or
        what Batch.set_unknowns takes: the names of the live groups, or an (n, 6) mask (dsp_batch_unknowns)."""
        kw = {} if self.convergence_pose_only is None else {"convergence": self.convergence_pose_only}
        unknowns = self.unknowns_pose_only if unknowns is None else unknowns
        if unknowns is not None:
            kw["unknowns"] = unknowns
        if obs_weights is not None:
            kw["obs_weights"] = self._stack_obs_weights(obs_weights, pts_list, None)
        if return_posterior:
            kw["posterior"] = self.posterior_pose_only or "mean"
        if self.report_pose_only:
            kw["report"] = True
        if priors is not None:
            kw["prior"] = self._stack_priors(priors, 6, self.code_len)
        return self.decoder.engine.estimate_pose_batch(self._params(), [_f32(t) for t in t_co_se3_list], scales,
                                                       [_f32(p) for p in pts_list], [_f32(c) for c in codes], **kw)

    def estimate_pose_cam_obj(self, t_co_se3, scale, pts, code, unknowns=None, obs_weights=None, prior=None):
        """Pose-only refinement of one detection (reference optimizer.py:45-86; called from LocalMapping_util.cc:109-110).
        t_co_se3: (4, 4) rigid object-to-camera guess; scale: the object's scale (float); pts: (M, 3) surface points in the camera frame;
        code: the object's shape code.  Returns the refined rigid object-to-camera matrix as a (4, 4) CPU torch.Tensor, like the reference.
        prior (an addition): dict(t_obj_cam, Lambda (6, 6)) -- the last estimate of this object and its information (one row of a pose-only
        Batch.posterior() at level 2); the call then returns a dict: t_cam_obj (the tensor), prior_chi2, prior_residual (6,).
        obs_weights (an addition): (pt_w, None) -- one weight per surface point; the return value is what it is without them.
        unknowns (an addition): the names of the live groups, e.g. ["translation", "yaw"], or a (6,) mask; the return value is what it is."""
        ow = None if obs_weights is None else [obs_weights]
        if prior is None and not self.report_pose_only:
            out = self.estimate_poses_cam_obj([t_co_se3], [float(scale)], [pts], [code], unknowns=unknowns, obs_weights=ow)
            return torch.from_numpy(out[0].copy())
        ret = self.estimate_poses_cam_obj([t_co_se3], [float(scale)], [pts], [code], unknowns=unknowns, obs_weights=ow,
                                          priors=None if prior is None else [prior])
        extra = {}
        if self.report_pose_only:       # (an addition, like the prior: the call then returns a dict)
            extra["observations"] = _observations.object_rows(ret[1], 0)
        if prior is not None:
            extra.update(prior_chi2=float(ret[-1]["chi2"][0]), prior_residual=ret[-1]["e"][0].copy())
        return ForceKeyErrorDict(t_cam_obj=torch.from_numpy(ret[0][0].copy()), **extra)

    # ---- joint shape + pose (reference optimizer.py:88-203) -----------------------------------------
    def reconstruct_objects(self, t_cam_obj_list, pts_list, rays_list, depth_list, codes=None, unknowns=None, obs_weights=None, priors=None):
        """Batched form: B independent objects in one device run -> list of result dicts.  priors: None, or one dict(t_obj_cam, code,
        Lambda (71, 71)) or None per object (dsp_batch_prior); good objects then carry prior_chi2 and prior_residual.  obs_weights: None, or
        one (pt_w, ray_w) or None per object (dsp_batch_observation_weights); the result dicts keep their keys.  unknowns: None
        (joint_optim.unknowns, or every entry), or what Batch.set_unknowns takes: the names of the live groups for the whole batch, one list
        of names per object, or an (n, 71) mask (dsp_batch_unknowns); the result dicts keep their keys."""
        B = len(pts_list)
        codes_in = None
        if codes is not None:
            codes_in = [np.zeros(self.code_len, np.float32) if c is None else _f32(c)[:self.code_len] for c in codes]
        kw = {} if self.convergence_joint is None else {"convergence": self.convergence_joint}
        if self.posterior_joint is not None:
            kw["posterior"] = self.posterior_joint
        if priors is not None:
            kw["prior"] = self._stack_priors(priors, 71, self.code_len)
        if self.step_control_joint is not None:
            kw["step_control"] = self.step_control_joint
        if self.report_joint:
            kw["report"] = True
        if obs_weights is not None:
            kw["obs_weights"] = self._stack_obs_weights(obs_weights, pts_list, rays_list)
        unknowns = self.unknowns_joint if unknowns is None else unknowns
        if unknowns is not None:
            kw["unknowns"] = unknowns
        res = self.decoder.engine.reconstruct_batch(
            self._params(), [_f32(x) for x in t_cam_obj_list], [_f32(p) for p in pts_list],
            [_f32(r) for r in rays_list], [_f32(d).reshape(-1) for d in depth_list], codes_in, compute=self.compute, **kw)
        t, code, loss, status = res[:4]
        out = []
        for i in range(B):
            if status[i] == _L.OBJ_GOOD:
                out.append(ForceKeyErrorDict(t_cam_obj=t[i].copy(), code=code[i].copy(), is_good=True,
                                             loss=torch.tensor(float(loss[i])), **self._posterior_fields(res, i), **self._report_fields(res, i),
                                             **self._prior_fields(res, i, priors)))
            else:   # reference: t_cam_obj=None, code=None, is_good=False, loss=<last computed loss> (:131,136,143,150)
                out.append(ForceKeyErrorDict(t_cam_obj=None, code=None, is_good=False, loss=float(loss[i])))
        return out

    def _posterior_fields(self, res, i):
        """The extra result fields of a good object when joint_optim.posterior is set (none otherwise: the dict is the reference's four)."""
        if self.posterior_joint is None:
            return {}
        post = res[4]
        return dict(pose_information=post["info_pose"][i].copy(), pose_covariance=post["cov_pose"][i].copy(),
                    code_variance=post["var_code"][i].copy(), loss_at_result=float(post["loss"][i]),
                    posterior_ok=bool(post["status"][i] == _L.POSTERIOR_OK))

    def _report_fields(self, res, i):
        """`observations` of a good object when joint_optim.report is set (nothing otherwise): Batch.report() follows the posterior."""
        if not self.report_joint:
            return {}
        return dict(observations=_observations.object_rows(res[4 if self.posterior_joint is None else 5], i))

    @staticmethod
    def _prior_fields(res, i, priors):
        """The extra result fields of a good object of a call with priors (none otherwise): Batch.prior_residual() is the call's last item."""
        if priors is None:
            return {}
        return dict(prior_chi2=float(res[-1]["chi2"][i]), prior_residual=res[-1]["e"][i].copy())

    def reconstruct_object(self, t_cam_obj, pts, rays, depth, code=None, unknowns=None, obs_weights=None, prior=None):
        """Joint shape + pose optimisation of one object (reference optimizer.py:88-203; LocalMapping_util.cc:179-180,391-392,402-403).
        t_cam_obj: (4, 4) Sim(3) object-to-camera start; pts: (M, 3) surface points in the camera frame; rays: (R, 3) ray directions, the
        first len(depth) of them foreground; depth: observed depth of the foreground rays (KITTI: one per surface point); code: optional
        start code (zeros when None).  Returns the reference's result dict: t_cam_obj, code, is_good, loss -- attribute access, KeyError on
        anything else.  prior (an addition): dict(t_obj_cam, code, Lambda (71, 71)) -- one row of a level-2 Batch.posterior() can be passed
        as it is -- fuses that earlier estimate into the run (dsp_batch_prior); the result then also has prior_chi2 and prior_residual.
        obs_weights (an addition): (pt_w, ray_w), one weight per surface point / per ray, either None = ones; the result keeps its keys.
        unknowns (an addition): the names of the live groups -- ["pose"] tracks the pose from points and rays with the code held, ["code"]
        refits the shape under a fixed pose, ["translation", "rotation", "code"] keeps a known scale -- or a (71,) mask; same keys."""
        start = get_time()
        rst = self.reconstruct_objects([t_cam_obj], [pts], [rays], [depth], None if code is None else [code], unknowns=unknowns,
                                       obs_weights=None if obs_weights is None else [obs_weights], priors=None if prior is None else [prior])[0]
        if self.verbose and rst.is_good:
            print("Reconstruction takes %f seconds" % (get_time() - start))
        return rst

    def reconstruct_object_multiview(self, t_cam_obj, views, code=None, unknowns=None, obs_weights=None, prior=None):
        """Joint shape + pose optimisation of one object from SEVERAL observations (an addition: the reference's reconstruct_object,
        optimizer.py:88-203, takes one, although its map keeps one per key frame).  t_cam_obj: (4, 4) Sim(3) object-to-camera start in the
        frame of the REFERENCE camera = the camera of views[0]; views: [dict(t_ref_cam, pts, rays, depth), ...] -- t_ref_cam (4, 4) rigid,
        that view's camera -> the reference camera (identity for views[0]); pts / rays / depth as reconstruct_object takes them, in that
        view's camera frame.  All views share one pose and one code; their rows are pooled into one Gauss-Newton system per iteration.
        Same result dict as reconstruct_object; one view gives reconstruct_object's result, bit for bit.  prior: as reconstruct_object.
        obs_weights: None, or one (pt_w, ray_w) or None per VIEW.  unknowns: as reconstruct_object (one mask for the object, not per view)."""
        vs = [dict(t_ref_cam=_f32(v["t_ref_cam"]), pts=_f32(v["pts"]), rays=_f32(v["rays"]), depth=_f32(v["depth"]).reshape(-1)) for v in views]
        codes_in = None if code is None else [_f32(code)[:self.code_len]]
        kw = {} if self.convergence_joint is None else {"convergence": self.convergence_joint}
        if self.posterior_joint is not None:
            kw["posterior"] = self.posterior_joint
        priors = None if prior is None else [prior]
        if priors is not None:
            kw["prior"] = self._stack_priors(priors, 71, self.code_len)
        if self.report_joint:
            kw["report"] = True
        if obs_weights is not None:
            kw["obs_weights"] = self._stack_obs_weights(obs_weights, [v["pts"] for v in vs], [v["rays"] for v in vs])
        unknowns = self.unknowns_joint if unknowns is None else unknowns
        if unknowns is not None:
            kw["unknowns"] = unknowns
        res = self.decoder.engine.reconstruct_multiview_batch(self._params(), [_f32(t_cam_obj)], [vs], codes_in, **kw)
        t, z, loss, status = res[:4]
        if status[0] == _L.OBJ_GOOD:
            return ForceKeyErrorDict(t_cam_obj=t[0].copy(), code=z[0].copy(), is_good=True, loss=torch.tensor(float(loss[0])),
                                     **self._posterior_fields(res, 0), **self._report_fields(res, 0), **self._prior_fields(res, 0, priors))
        return ForceKeyErrorDict(t_cam_obj=None, code=None, is_good=False, loss=float(loss[0]))

    @staticmethod
    def get_shape_code(result):
        """Shape code of a reconstruction result (the C++ side keeps it in MapObject::GetShapeCode,
        src/MapObject.cc:469-473).  Addition named by BASELINE.json; not present in the reference's Python."""
        return result.code


class MeshExtractor(object):
    def __init__(self, decoder, code_len=64, voxels_dim=64, regular_grid=False, prepass=None):
        """regular_grid=False samples the SDF exactly where the reference does (its grid is sheared by a true-division quirk,
        see reconstruct.utils.create_voxel_grid); True samples the regular lattice.  prepass=None (default) decodes every grid point
        in fp32; "f16" / "bf16" decodes the grid with the low-precision prepass and only the surface band in fp32 -- the same meshes,
        bit for bit (include/dsp_gn.h dsp_extract_meshes); it does not pay at 32^3 (profiles/mesh_band.md).  (Additions; the
        reference has no such switches.)"""
        self.decoder = decoder
        self.code_len = code_len
        self.voxels_dim = voxels_dim
        self.regular_grid = bool(regular_grid)
        self.prepass = prepass
        self.voxel_points = create_voxel_grid(vol_dim=self.voxels_dim, regular=self.regular_grid)

    def decode_grid(self, code):
        """SDF on the voxels_dim^3 grid, decoded on the GPU (the part of extract_mesh_from_code that is
        decoder work, reference optimizer.py:217-218)."""
        sdf = self.decoder.engine.decode_sdf(_f32(code)[:self.code_len], self.voxel_points)
        return sdf.reshape(self.voxels_dim, self.voxels_dim, self.voxels_dim)

    def decode_grids(self, codes):
        """Batched grid decode: (n, code_len) codes -> (n, D, D, D) SDF volumes in one kernel launch (the loop of
        extract_map_objects.py:46-63 over a whole map)."""
        codes = np.stack([_f32(c)[:self.code_len] for c in codes])
        sdf = self.decoder.engine.decode_sdf_multi(codes, self.voxel_points)
        return sdf.reshape(codes.shape[0], self.voxels_dim, self.voxels_dim, self.voxels_dim)

    def extract_mesh_from_code(self, code):
        """Grid decode + marching cubes, both on the GPU without the volume leaving HBM (reference optimizer.py:214-223;
        there: GPU decode, then scikit-image marching cubes on the CPU)."""
        start = get_time()
        vertices, faces = self.decoder.engine.extract_mesh(_f32(code)[:self.code_len], self.voxels_dim, regular_grid=self.regular_grid,
                                                           prepass=self.prepass)
        if vertices.shape[0] == 0:
            raise ValueError("Surface level must be within volume data range.")   # what scikit-image raises in the reference
        print("Extract mesh takes %f seconds" % (get_time() - start))
        return ForceKeyErrorDict(vertices=vertices, faces=faces)

    def extract_meshes_from_codes(self, codes):
        """extract_mesh_from_code for many objects in one batched call (dsp_extract_meshes): a list of the same dicts, in the order
        of `codes`.  An object whose surface does not cross the grid gets empty (0, 3) arrays instead of raising.  (Addition.)"""
        codes = [_f32(c)[:self.code_len] for c in codes]
        meshes = self.decoder.engine.extract_meshes(codes, self.voxels_dim, regular_grid=self.regular_grid, prepass=self.prepass)
        return [ForceKeyErrorDict(vertices=v, faces=f) for v, f in meshes]

    def extract_refined_meshes_from_codes(self, codes, steps=6, var_codes=None):
        """extract_meshes_from_codes with every vertex projected onto the decoder's zero set by `steps` capped Newton steps on the
        device (dsp_meshes_refine): dicts with `vertices` (refined), `faces`, `normals` (the decoder's unit gradient), `sdf`,
        `vertices_mc` (the marching-cubes vertices) and -- var_codes given, (n, code_len) code variances -- `sigma`.  (Addition.)"""
        codes = [_f32(c)[:self.code_len] for c in codes]
        meshes = self.decoder.engine.extract_meshes_refined(codes, self.voxels_dim, steps=steps, regular_grid=self.regular_grid,
                                                            prepass=self.prepass, var_code=var_codes)
        return [ForceKeyErrorDict(**m) for m in meshes]
