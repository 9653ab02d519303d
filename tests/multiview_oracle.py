"""Multi-view Gauss-Newton oracle (numpy, CPU): a COMPOSITION of the single-view oracle's own terms -- oracle.dsp_oracle.compute_sdf_loss,
compute_render_loss, compute_rotation_loss_sim3, get_robust_res, exp_sim3 -- evaluated per view at T_oc_v = T_oc @ T_ref_v, with the rows of
all views pooled as one row set; everything else follows oracle.dsp_oracle.reconstruct_object (reference optimizer.py:120-192) line by line.
A view whose render term is None (< 10 in-sphere samples, loss.py:73-74) contributes no render rows in that iteration.  Test helper, not a test."""
import math

import numpy as np

from oracle import dsp_oracle as O

F32 = np.float32


def view_state(t_obj_cam, t_ref_cam, n_depth):
    """T_oc_v = T_oc T_ref_v and the depth samples derived from it (optimizer.py:120-125)."""
    t_v = (np.asarray(t_obj_cam, np.float64) @ np.asarray(t_ref_cam, np.float64)).astype(F32)      # fp64 product of the fp32 matrices, rounded once
    t_co = O._inv(t_v)
    scale = O._det3_cuberoot(t_co[:3, :3])
    d_min = F32(t_co[2, 3] - F32(1.0) * scale)
    d_max = F32(t_co[2, 3] + F32(1.0) * scale)
    return t_v, O.linspace_f32(d_min, d_max, n_depth)


def reconstruct_object_multiview(dec, prm, t_cam_obj, views, code=None, trace=None, t_obj_cam0=None, num_iterations=None, depths_override=None,
                                 sdf_jitter=0.0):
    """views: [dict(t_ref_cam, pts, rays, depth), ...].  Returns dict(t_cam_obj, code, is_good, loss, status) -- status 0 good, 1 no view
    reached 10 in-sphere samples, 2 NaN / empty row set.  trace (list) receives one dict per iteration: pooled H, b, dx, loss, the state,
    and per view V, K, vsum, ksum, depths, t_obj_cam, sets (compute_render_loss's stats: `valid`, `kept`, ...; None where the view's
    render term is None).  sdf_jitter (tests only): passed to compute_render_loss -- the jitter twin of tests/test_gpu_parity.py."""
    c_len = prm.code_len
    z = np.zeros(c_len, F32) if code is None else np.asarray(code, F32)[:c_len].copy()
    t_obj_cam = O._inv(np.asarray(t_cam_obj, F32)) if t_obj_cam0 is None else np.asarray(t_obj_cam0, F32).copy()
    loss = 0.
    fail = lambda status: dict(t_cam_obj=None, code=None, is_good=False, loss=loss, status=status, t_obj_cam=t_obj_cam, z=z)  # noqa: E731
    for e in range(prm.num_iterations if num_iterations is None else num_iterations):
        rows_s, rows_r, per_view = [], [], []
        for iv, v in enumerate(views):
            t_v, sampled = view_state(t_obj_cam, v["t_ref_cam"], prm.num_depth_samples)
            if depths_override is not None:      # tests only: linearise on exactly these depth samples (one row per view; single-iteration runs)
                sampled = np.asarray(depths_override[iv], F32)[:prm.num_depth_samples].copy()
            rays, depth, pts = np.asarray(v["rays"], F32).reshape(-1, 3), np.asarray(v["depth"], F32).reshape(-1), np.asarray(v["pts"], F32).reshape(-1, 3)
            depth_obs = np.concatenate([depth, np.full(rays.shape[0] - depth.shape[0], F32(1.1) * sampled[-1], F32)]).astype(F32)   # :126
            if pts.shape[0]:
                j7, jc, r = O.compute_sdf_loss(dec, pts, t_v, z)                 # :129
                rows_s.append((np.concatenate([j7, jc], -1), r))
            st = {"V": 0}
            rend = O.compute_render_loss(dec, rays, depth_obs, t_v, sampled, z, th=prm.cut_off, stats=st,
                                         sdf_jitter=sdf_jitter) if rays.shape[0] else None
            info = dict(V=st["V"], K=0, vsum=0, ksum=0, depths=sampled, t_obj_cam=t_v, none=rend is None, sets=None if rend is None else st)
            if rend is not None:
                j7, jc, r = rend
                rows_r.append((np.concatenate([j7, jc], -1), r))
                info.update(K=st["K"], vsum=O.set_checksum(*st["valid"]), ksum=O.set_checksum(*st["kept"]))
            per_view.append(info)
        if all(p["none"] for p in per_view):
            return fail(1)
        if not rows_s or not rows_r or sum(r.shape[0] for _, r in rows_r) == 0:
            return fail(2)
        j_s, r_s = np.concatenate([j for j, _ in rows_s]), np.concatenate([r for _, r in rows_s])
        j_r, r_r = np.concatenate([j for j, _ in rows_r]), np.concatenate([r for _, r in rows_r])
        rr_s, sdf_loss, _ = O.get_robust_res(r_s, prm.b2)                        # :134
        rr_r, render_loss, _ = O.get_robust_res(r_r, prm.b1)                     # :148
        if math.isnan(sdf_loss) or math.isnan(render_loss):
            return fail(2)
        j_rot, res_rot = O.compute_rotation_loss_sim3(t_obj_cam)                 # :153 (the reference camera's frame)
        loss = float(F32(prm.k1) * render_loss + F32(prm.k2) * sdf_loss)         # :155
        pd = 7
        hs, bs = O._gram(j_s, rr_s)
        hr, br = O._gram(j_r, rr_r)
        h = (F32(prm.k1) * hr / F32(j_r.shape[0]) + F32(prm.k2) * hs / F32(j_s.shape[0])).astype(F32)      # :162-168
        b = (-F32(prm.k1) * br / F32(j_r.shape[0]) - F32(prm.k2) * bs / F32(j_s.shape[0])).astype(F32)
        h[pd:, pd:] += F32(prm.k3) * np.eye(c_len, dtype=F32)                    # :170
        b[pd:] -= F32(prm.k3) * z                                                # :172
        h[:pd, :pd] += F32(prm.k4) * np.outer(j_rot, j_rot).astype(F32)          # :176,178
        b[:pd] -= F32(prm.k4) * (-(j_rot * res_rot).astype(F32))                 # :177,179 (sign as written)
        h[:pd, :pd] += np.eye(pd, dtype=F32)                                     # :183
        h[pd - 1, pd - 1] += F32(prm.s_damp)                                     # :184
        dx = (O._inv(h) @ b).astype(F32)                                         # :186
        if trace is not None:
            trace.append(dict(H=h.copy(), b=b.copy(), dx=dx.copy(), loss=loss, t_obj_cam=t_obj_cam.copy(), code=z.copy(), views=per_view,
                              M=int(j_s.shape[0]), K=int(j_r.shape[0])))
        t_obj_cam = (O.exp_sim3(F32(prm.lr) * dx[:pd]) @ t_obj_cam).astype(F32)  # :190-191
        z = (z + F32(prm.lr) * dx[pd:pd + c_len]).astype(F32)                    # :192
    return dict(t_cam_obj=O._inv(t_obj_cam), code=z, is_good=True, loss=loss, status=0)


def rot_prior_bound(h_ref, k4):
    """What tests/test_gpu_forensics.py allows on b[3:6] beside 1e-4 of b's largest entry: those entries carry k4 * J_rot * (1 + R_co[1,1])
    with k4 = 1e7, a residual quantised to ulp(1) = 1.2e-7 IN FRONT of the factor -- in the reference itself.  Two ulp, times the jacobian entry."""
    j_rot = np.sqrt(np.abs(np.diag(h_ref)[3:6]) / max(k4, 1.0))
    return k4 * (j_rot + 1e-3) * 2.4e-7


def split_views(o):
    """One observation dealt alternately into two views of the same camera (KITTI layout: foreground ray i belongs to point i)."""
    eye = np.eye(4, dtype=F32)
    m = o["depth"].shape[0]
    views = []
    for k in range(2):
        fg, bg = np.arange(k, m, 2), np.arange(m + k, o["rays"].shape[0], 2)
        views.append(dict(t_ref_cam=eye, pts=o["pts"][k::2], rays=np.concatenate([o["rays"][fg], o["rays"][bg]]), depth=o["depth"][fg]))
    return views


def golden_views(g):
    n = sum(1 for k in g.files if k.endswith("_t_ref_cam"))
    return [dict(t_ref_cam=g["in_v%d_t_ref_cam" % v], pts=g["in_v%d_pts" % v], rays=g["in_v%d_rays" % v], depth=g["in_v%d_depth" % v]) for v in range(n)]


def _insphere_per_ray(t_obj_cam, rays, n_depth):
    t_v, d = view_state(t_obj_cam, np.eye(4, dtype=F32), n_depth)
    p = O.transform_points(t_v, (rays[:, None, :] * d[None, :, None]).astype(F32))
    return (np.sqrt(np.sum(p * p, axis=-1, dtype=F32)) < F32(1.0)).sum(1)


def late_join_case(seed=61, n_depth=50):
    """(t_cam_obj_init, views): a normal first view, and a second view of the same camera that holds only background rays grazing the rim of
    the unit sphere -- outside it at the (perturbed) start pose, inside it at the generating pose -- so that its render term is None in
    iteration 0 and appears in a later iteration.  Geometry only; tests confirm the transition with the composed oracle."""
    from dsp_slam_amd import synth
    o = synth.make_object(seed, n_surface=150, n_background=40)
    t0, tg = O._inv(o["t_cam_obj_init"]), O._inv(o["t_cam_obj_gt"])
    c = o["t_cam_obj_gt"][:3, 3].astype(np.float64)
    s = float(o["scale"])
    u, v = np.meshgrid(np.linspace(-1.3, 1.3, 81), np.linspace(-1.3, 1.3, 81))
    rays = np.stack([(c[0] + s * u.ravel()) / c[2], (c[1] + s * v.ravel()) / c[2], np.ones(u.size)], -1).astype(F32)
    n0, ng = _insphere_per_ray(t0, rays, n_depth), _insphere_per_ray(tg, rays, n_depth)
    pick = np.where((n0 == 0) & (ng >= 2) & (ng <= 12))[0]
    rays = rays[pick][np.argsort(-ng[pick], kind="stable")][:24]
    eye = np.eye(4, dtype=F32)
    return o["t_cam_obj_init"], [dict(t_ref_cam=eye, pts=o["pts"], rays=o["rays"], depth=o["depth"]),
                                 dict(t_ref_cam=eye, pts=np.zeros((0, 3), F32), rays=np.ascontiguousarray(rays), depth=np.zeros(0, F32))]


LEAVING_SEED = 64          # chosen with the composed oracle (tests/test_multiview_metric.py asserts the transition it was chosen for)


def leaving_case(seed=LEAVING_SEED, n_depth=50):
    """late_join_case with the roles of the start and the generating pose swapped: the second view holds only background rays grazing the rim
    of the unit sphere that are inside it at the (perturbed) start pose and outside it at the generating pose -- so that its render rows are
    there in iteration 0 and vanish in a later one.  Geometry only; tests confirm the transition with the composed oracle."""
    from dsp_slam_amd import synth
    o = synth.make_object(seed, n_surface=150, n_background=40)
    t0, tg = O._inv(o["t_cam_obj_init"]), O._inv(o["t_cam_obj_gt"])
    c = o["t_cam_obj_gt"][:3, 3].astype(np.float64)
    s = float(o["scale"])
    u, v = np.meshgrid(np.linspace(-1.3, 1.3, 81), np.linspace(-1.3, 1.3, 81))
    rays = np.stack([(c[0] + s * u.ravel()) / c[2], (c[1] + s * v.ravel()) / c[2], np.ones(u.size)], -1).astype(F32)
    n0, ng = _insphere_per_ray(t0, rays, n_depth), _insphere_per_ray(tg, rays, n_depth)
    pick = np.where((ng == 0) & (n0 >= 2) & (n0 <= 12))[0]
    rays = rays[pick][np.argsort(-n0[pick], kind="stable")][:24]
    eye = np.eye(4, dtype=F32)
    return o["t_cam_obj_init"], [dict(t_ref_cam=eye, pts=o["pts"], rays=o["rays"], depth=o["depth"]),
                                 dict(t_ref_cam=eye, pts=np.zeros((0, 3), F32), rays=np.ascontiguousarray(rays), depth=np.zeros(0, F32))]


ONE_SIDED_SEED = 4          # chosen with the composed oracle (tests/test_multiview_oracle.py asserts the ordering it was chosen for)


def one_sided_case(seed=ONE_SIDED_SEED):
    """An object whose three cameras each see one side only (120 degrees apart... spread over 240 degrees): (object, [single-view start poses])."""
    from dsp_slam_amd import synth
    o = synth.make_object_multiview(seed, n_views=3, n_surface=150, n_background=40, yaw_spread_deg=240.0)
    # the same start estimate, expressed in each view's own camera frame: T_cam_v_obj = inv(T_ref_v) @ T_ref_obj
    starts = [(np.linalg.inv(v["t_ref_cam"].astype(np.float64)) @ o["t_cam_obj_init"].astype(np.float64)).astype(F32) for v in o["views"]]
    return o, starts


def code_error(code, o):
    return float(np.linalg.norm(np.asarray(code, np.float64)[:3] - o["code_gt"][:3].astype(np.float64)))
