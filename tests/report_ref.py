"""numpy references for the observation report (dsp_batch_report, include/dsp_gn.h) -- test infrastructure.

* `chain_ray`: ONE ray with the three chains written sequentially, one float32 operation at a time, as k_render_scan writes them -- what
  dsp_debug_report_ray (csrc/report_math.h) must reproduce bit for bit.
* `evaluate32`: the report of one member restated from unmodified oracle pieces: compute_sdf_loss gives pt_sdf; loss.py:60-114 (transform,
  in-sphere test, decode_sdf, sdf_to_occupancy, cumprod, the depth sum) applied to ALL rays gives depth, hit and the counts; get_robust_res
  gives the sums.  numpy's cumprod / sum are the oracle's summation orders, not the device's.
* `evaluate64`: its fp64 twin through oracle.dsp_oracle._decode64, on the fp32 evaluation's in-sphere set.
* `agreeing_rays`: the rays whose band and kept decisions agree between fp32, its sdf_jitter = +-2e-7 twins and fp64.
* `joint_objects` / `multiview_objects` / `pose_objects`: the inputs of tests/test_gpu_report.py, shared with tools/measure_report.py.
* `TAU_*`: per float field, the worst |fp32 restatement - fp64 twin| over those inputs, as tools/measure_report.py --measure printed them
  (profiles/report.md).  The GPU bound per field is 4 x TAU + 4 ulp32 of the value (`bound`): device and fp32 oracle are two fp32
  evaluations of one formula with different summation orders, each may sit that far from fp64 (the practice of tests/gn_metric.py).
  Never tuned on the device's output.
"""
import numpy as np

from oracle import dsp_oracle as O

F32, F64 = np.float32, np.float64
JITTER = 2e-7

# tools/measure_report.py --measure (CPU only), worst over joint_objects at D = 50 and 64 and multiview_objects at D = 50, rounded up to
# two significant digits as the tool prints them (sum_r: against the fp64 sum over the fp32 evaluation's kept set, sum_r64_on)
TAU_PT_SDF = 6.7e-07
TAU_RAY_DEPTH = 4.1e-05
TAU_RAY_HIT = 1.2e-05
TAU_RAY_RESIDUAL = 4.1e-05
TAU_SUM_S = 7.0e-08
TAU_SUM_R = 4.4e-05
TAU = dict(pt_sdf=TAU_PT_SDF, ray_depth=TAU_RAY_DEPTH, ray_hit=TAU_RAY_HIT, ray_residual=TAU_RAY_RESIDUAL, sum_s=TAU_SUM_S, sum_r=TAU_SUM_R)


def bound(field, value):
    """4 x the measured fp32-to-fp64 distance of the field + 4 ulp32 of the value."""
    v = np.abs(np.asarray(value, F64))
    return 4.0 * TAU[field] + 4.0 * np.spacing(np.maximum(v, np.finfo(F32).tiny).astype(F32)).astype(F64)


# ---- one ray, sequentially ------------------------------------------------------------------------------------------------------------
def chain_ray(depths, sdf, th, depth_obs, is_fg):
    """-> (out4 float32 = d_u, 1 - T_{D-1}, obs - d_u, clipped residual; counts3 int32 = in-sphere, band, kept).  sdf: NaN = not in the sphere."""
    d = np.asarray(depths, F32)
    s = np.asarray(sdf, F32)
    th = F32(th)
    n = d.shape[0]
    o, T, wg = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, bool)
    acc = F32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            if not np.isnan(s[j]):
                cl = min(max(s[j], -th), th)
                o[j] = F32(0.5) - F32(cl / F32(F32(2) * th))
                wg[j] = bool(s[j] > -th and s[j] < th)
            acc = F32(acc * F32(F32(1) - o[j]))
            T[j] = acc
        d_bg = F32(F32(1.1) * d[n - 1])
        du = F32(0)
        for j in range(n):
            du = F32(du + F32(d[j] * F32(o[j] * (F32(1) if j == 0 else T[j - 1]))))
        du = F32(du + F32(d_bg * T[n - 1]))
        obs = F32(depth_obs) if is_fg else d_bg
        res = F32(obs - du)
        clip = res
        if clip > F32(0.30):
            clip = F32(0.30)
        if clip < F32(-0.30):
            clip = F32(-0.30)
        kept, sacc = 0, F32(0)
        for j in range(n - 1, -1, -1):
            sacc = F32(sacc + T[j])
            if wg[j] and F32(sacc / F32(F32(1) - o[j])) > F32(1e-2):
                kept += 1
    return (np.array([du, F32(F32(1) - T[n - 1]), res, clip], F32),
            np.array([int((~np.isnan(s)).sum()), int(wg.sum()), kept], np.int32))


# ---- one member from oracle pieces ----------------------------------------------------------------------------------------------------
def derived_depths(t_obj_cam, n_depth):
    """The depth samples an iteration derives from the pose (optimizer.py:120-125)."""
    t_co = O._inv(np.asarray(t_obj_cam, F32))
    scale = O._det3_cuberoot(t_co[:3, :3])
    return O.linspace_f32(F32(t_co[2, 3] - F32(1.0) * scale), F32(t_co[2, 3] + F32(1.0) * scale), n_depth)


def _ray_fields(occ, d, sdf_grid, in_mask, depth, th, b1, f32):
    """loss.py:84-141 applied to all rays; occ (R, D) with 0 outside the sphere.  f32: float32 throughout (the oracle's operations), else float64."""
    one = F32(1) if f32 else 1.0
    dt = F32 if f32 else F64
    n_rays, n_d = occ.shape
    acc = np.cumprod(one - occ, axis=-1, dtype=dt)                                  # :99
    acc_aug = np.concatenate([np.ones((n_rays, 1), dt), acc], -1)
    o = np.concatenate([occ, np.ones((n_rays, 1), dt)], -1)
    c11 = F32(1.1) if f32 else float(F32(1.1))
    dd = np.concatenate([d, np.array([c11 * d[-1]], dt)], -1)
    d_u = np.sum(dd * (o * acc_aug).astype(dt), axis=-1, dtype=dt)                   # :112-114
    hit = (one - acc[:, -1]).astype(dt)
    n_fg = np.asarray(depth).reshape(-1).shape[0]
    obs = np.concatenate([np.asarray(depth, F32).astype(dt).reshape(-1), np.full(n_rays - n_fg, c11 * d[-1], dt)])      # optimizer.py:126
    with np.errstate(invalid="ignore"):
        res = (obs - d_u).astype(dt)
        band = in_mask & (sdf_grid > -th) & (sdf_grid < th)                          # :88
        suffix = np.cumsum(acc[:, ::-1], axis=-1, dtype=dt)[:, ::-1]                 # sum_{l >= k} T_l  (:121)
        de_do = (suffix / (one - occ)).astype(dt)
        kept = band & (de_do > (F32(1e-2) if f32 else float(F32(1e-2))))             # :125
    clip = np.clip(res, -(F32(0.30) if f32 else float(F32(0.30))), F32(0.30) if f32 else float(F32(0.30)))
    rows = np.repeat(clip, kept.sum(-1))                                             # one residual per kept row, ray-major (:135-140)
    if f32:
        rr = O.get_robust_res(rows, b1)[0]
    else:
        rr = O._robust_rows64(rows, float(F32(b1)))
    return dict(ray_depth=d_u, ray_hit=hit, ray_residual=res, band=band, kept=kept,
                ray_counts=np.stack([in_mask.sum(-1), band.sum(-1), kept.sum(-1)], -1).astype(np.int32),
                sum_r=float(np.sum(rr.astype(F64) ** 2)), K=int(kept.sum()), m=int(band.sum()))


def evaluate32(dec, prm, pts, rays, depth, t_obj_cam, code, depths, sdf_jitter=0.0):
    """The report rows of one member at (t_obj_cam, code, depths), float32, from the oracle's own functions."""
    z = np.asarray(code, F32)[:prm.code_len]
    t = np.asarray(t_obj_cam, F32)
    pts = np.asarray(pts, F32).reshape(-1, 3)
    rays = np.asarray(rays, F32).reshape(-1, 3)
    d = np.asarray(depths, F32)[:prm.num_depth_samples]
    th = F32(prm.cut_off)
    out = dict(M=int(pts.shape[0]))
    if pts.shape[0]:
        out["pt_sdf"] = O.compute_sdf_loss(dec, pts, t, z)[2]
        out["sum_s"] = float(np.sum(O.get_robust_res(out["pt_sdf"], prm.b2)[0].astype(F64) ** 2))
    else:
        out["pt_sdf"], out["sum_s"] = np.zeros(0, F32), 0.0
    pts_cam = (rays[:, None, :] * d[None, :, None]).astype(F32)                      # :60
    pts_obj = O.transform_points(t, pts_cam)                                         # :62-63
    nrm = np.sqrt(np.sum(pts_obj * pts_obj, axis=-1, dtype=F32)).astype(F32)
    in_mask = nrm < F32(1.0)                                                         # :68
    vx, vy = np.where(in_mask)
    out.update(V=int(vx.shape[0]), in_mask=in_mask, pts_obj=pts_obj)
    sdf_grid = np.full(in_mask.shape, np.nan, F32)
    if vx.shape[0]:
        sdf = O.decode_sdf(dec, z, pts_obj[vx, vy, :])                               # :77-78
        if sdf_jitter:
            sdf = (sdf + F32(sdf_jitter) * np.where(np.arange(sdf.shape[0]) % 2 == 0, F32(1), F32(-1))).astype(F32)
        sdf_grid[vx, vy] = sdf
    out["sdf_grid"] = sdf_grid
    occ = np.zeros(in_mask.shape, F32)
    occ[vx, vy] = O.sdf_to_occupancy(sdf_grid[vx, vy], th)                           # :84-86
    out.update(_ray_fields(occ, d, sdf_grid, in_mask, depth, th, prm.b1, True))
    return out


def evaluate64(dec, prm, pts, rays, depth, t_obj_cam, code, depths, in_mask):
    """The fp64 twin on the fp32 evaluation's in-sphere set."""
    z = np.asarray(code, F64)[:prm.code_len]
    t = np.asarray(t_obj_cam, F32).astype(F64)
    r_m, t_v = t[:3, :3], t[:3, 3]
    pts = np.asarray(pts, F32).astype(F64).reshape(-1, 3)
    rays = np.asarray(rays, F32).astype(F64).reshape(-1, 3)
    d = np.asarray(depths, F32).astype(F64)[:prm.num_depth_samples]
    th = float(F32(prm.cut_off))
    out = dict(M=int(pts.shape[0]))
    if pts.shape[0]:
        out["pt_sdf"] = O._decode64(dec, z, pts @ r_m.T + t_v, grad=False)[0]
        out["sum_s"] = float(np.sum(O._robust_rows64(out["pt_sdf"], float(F32(prm.b2))) ** 2))
    else:
        out["pt_sdf"], out["sum_s"] = np.zeros(0), 0.0
    vx, vy = np.where(in_mask)
    sdf_grid = np.full(in_mask.shape, np.nan)
    if vx.shape[0]:
        sdf_grid[vx, vy] = O._decode64(dec, z, (rays[vx] * d[vy, None]) @ r_m.T + t_v, grad=False)[0]
    occ = np.zeros(in_mask.shape)
    occ[vx, vy] = 0.5 - np.clip(sdf_grid[vx, vy], -th, th) / (2.0 * th)
    out.update(V=int(vx.shape[0]), sdf_grid=sdf_grid)
    out.update(_ray_fields(occ, d, sdf_grid, in_mask, depth, th, prm.b1, False))
    return out


def agreeing_rays(dec, prm, pts, rays, depth, t_obj_cam, code, depths, r32=None, r64=None):
    """bool (n_rays,): the band and the kept sets of the ray are the same in fp32, with sdf_jitter = +-2e-7 and in fp64."""
    r32 = r32 or evaluate32(dec, prm, pts, rays, depth, t_obj_cam, code, depths)
    r64 = r64 or evaluate64(dec, prm, pts, rays, depth, t_obj_cam, code, depths, r32["in_mask"])
    ok = np.ones(r32["band"].shape[0], bool)
    twins = [evaluate32(dec, prm, np.zeros((0, 3), F32), rays, depth, t_obj_cam, code, depths, sdf_jitter=s) for s in (JITTER, -JITTER)]
    for other in twins + [r64]:
        ok &= np.all(other["band"] == r32["band"], axis=-1) & np.all(other["kept"] == r32["kept"], axis=-1)
    return ok


HUBER_ROW_MAX = 0.08 + 1e-6      # the most one render row adds to sum_r: |r| <= 0.30 after the clip, (w r)^2 = rho(0.30) = 2 b1 0.30 - b1^2 at b1 = 0.2


def sum_r64_on(r64, kept_counts, b1):
    """sum_r in fp64 over a GIVEN kept set: every kept row of a ray carries the ray's clipped residual, so the sum is
    sum over rays of (kept rows of the ray) x (w r)^2 of the ray's fp64 residual.  With the fp32 evaluation's kept counts this is the
    reference sum_r is held to for EVERY member: it does not depend on how fp64 itself decides the keep test."""
    clip = np.clip(np.asarray(r64["ray_residual"], F64), -float(F32(0.30)), float(F32(0.30)))
    rr = O._robust_rows64(clip, float(F32(b1)))
    return float(np.sum(np.asarray(kept_counts, F64) * rr ** 2))


def band_up_to_first_solid(r32, th):
    """Per ray, the fp32 oracle's band samples up to and including the ray's first solid sample (sdf <= -th: occupancy 1, T = 0 behind it) --
    the band samples that are decoded whatever the ray passes and the prepass skip; samples behind it may or may not be."""
    sdf, band = r32["sdf_grid"], r32["band"]
    with np.errstate(invalid="ignore"):
        solid = r32["in_mask"] & (sdf <= -F32(th))
    behind = np.cumsum(solid, axis=-1) - solid > 0          # strictly behind the first solid sample
    return (band & ~behind).sum(-1).astype(np.int32)


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------------
N_IT = 6


def joint_objects():
    """Two ragged objects -- about 120 points, 60 foreground + 40 background rays; the second with n_foreground != M -- and a third whose
    rays all miss the unit sphere (fewer than 10 in-sphere samples: it ends DSP_OBJ_FEW_SAMPLES)."""
    from dsp_slam_amd import synth
    a = synth.make_object(610, n_surface=120, n_background=40, n_foreground=60)
    b = synth.make_object(611, n_surface=97, n_background=35, n_foreground=70)
    c = synth.make_object(612, n_surface=64, n_background=20)
    c = dict(c, rays=(c["rays"] + np.array([40.0, 0.0, 0.0], np.float32)).astype(np.float32))
    return [a, b, c]


def multiview_objects():
    """Two objects with 3 and 1 views; the second view of the first object has no rays."""
    from dsp_slam_amd import synth
    o3 = synth.make_object_multiview(31, n_views=3, n_surface=90, n_background=30)
    o1 = synth.make_object_multiview(32, n_views=1, n_surface=110, n_background=30)
    v = o3["views"][1]
    o3["views"][1] = dict(v, rays=np.zeros((0, 3), np.float32), depth=np.zeros(0, np.float32))
    return [o3, o1]


def oracle_params(n_depth=50, n_it=N_IT):
    return O.GNParams(num_iterations=n_it, num_depth_samples=n_depth)
