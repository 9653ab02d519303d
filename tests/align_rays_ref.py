"""numpy restatement of the opening comment of dsp_slam_amd/csrc/align_rays_math.h (the arithmetic of dsp_map_align_rays): explicit float32
operations in the comment's order, one rounding each, fmaf restated as tests/query_ref.py does.  The cast itself is tests/raycast_ref.py
(expected(): the march round by round through an engine's decode_sdf / sdf_jacobian), the rows, the tree and the loop are tests/align_ref.py.

evaluator(...) makes the pipeline's evaluation (float32, what the device must return bit for bit when `eng` is the device's Engine);
evaluator64(...) the ALGORITHM with nothing rounded to float32: float64 rays, a float64 sphere tracer and a float64 decoder.  Both have the
signature align_ref.run expects of its `evaluate`.
"""
import numpy as np

import align_ref as A
import query_ref as Q
import raycast_ref as R

F32, F64 = np.float32, np.float64
MISS, HIT, UNDECIDED = R.MISS, R.HIT, R.UNDECIDED


# ---- float32: the comment, step by step --------------------------------------------------------------------------------------------------
def build(T, pts_s, org_s=None):
    """-> p_w, o_w, dir (n, 3) float32 each.  org_s None: the sensor origin."""
    pts_s = np.asarray(pts_s, F32).reshape(-1, 3)
    org_s = np.zeros_like(pts_s) if org_s is None else np.asarray(org_s, F32).reshape(-1, 3)
    rt = A.pose_rt(T)[None]
    with np.errstate(all="ignore"):
        pw, ow = Q.to_object(rt, pts_s)[0], Q.to_object(rt, org_s)[0]
        return pw, ow, (pw - ow).astype(F32)


def residual(ow, pw, obj, t_hit, dist_hit, status, gw, max_gap):
    """-> obj_row (n,) int32, d (n,) float32."""
    ow, pw, gw = [np.asarray(x, F32).reshape(-1, 3) for x in (ow, pw, gw)]
    obj, status = np.asarray(obj, np.int32), np.asarray(status, np.int32)
    t_hit, dist_hit = np.asarray(t_hit, F32), np.asarray(dist_hit, F32)
    with np.errstate(all="ignore"):
        dirv = (pw - ow).astype(F32)
        u, void = R.rays(ow, dirv)
        length = np.sqrt(Q.norm2(dirv)).astype(F32)
        gap = (length - t_hit).astype(F32)
        gu = ((gw[:, 0] * u[:, 0] + gw[:, 1] * u[:, 1]) + gw[:, 2] * u[:, 2]).astype(F32)
        d = Q.fmaf32(gu, gap, dist_hit)
        none = void | (obj < 0)
        matched = ~none & (status == HIT) & np.isfinite(gap) & (np.abs(gap.astype(F64)) <= max_gap)
    return np.where(matched, obj, -1).astype(np.int32), np.where(none, F32(np.inf), d).astype(F32)


def ray_rows(ow, pw, obj, t_hit, dist_hit, status, gw, w, huber, max_dist, max_gap):
    """What dsp_debug_align_ray_rows returns: obj_row, d, sums30."""
    obj_row, d = residual(ow, pw, obj, t_hit, dist_hit, status, gw, max_gap)
    g = np.where((obj_row >= 0)[:, None], np.asarray(gw, F32).reshape(-1, 3), F32(0))      # read only where the row is matched
    return obj_row, d, A.tree_sum(A.row_terms(pw, obj_row, d, g, w, huber, max_dist))


def check(params, raycast, max_gap, n_hyp, n_rays, n_obj):
    """True: dsp_debug_align_rays_check accepts (poses and weights aside).  params: a dict with max_dist."""
    if not R.check(R.params(**raycast)):
        return False
    if not max_gap >= params["max_dist"]:
        return False
    if n_hyp * n_rays > 2 ** 31 - 1:
        return False
    rows = n_hyp * n_rays
    return not (n_obj > 0 and rows > 0 and (n_obj * 1024 * 4 > (64 << 20) or n_obj * (-(-rows // 64)) * 4 > (64 << 20)))


def cast(eng, amap_t, codes, ow, dirv, raycast=None, budget=None):
    """The cast of the rows (o_w, dir) as raycast_ref states it, plus the winners' world gradients: obj, t, dist, status, gw, stats."""
    ex = R.expected(eng, amap_t, codes, ow, dirv, raycast, budget=budget)
    g = ex["geometry"]
    gw = np.zeros((ow.shape[0], 3), F32)
    for o in range(g["exists"].shape[0]):
        idx = np.flatnonzero(ex["obj"] == o)
        if idx.size:
            _, grad = eng.sdf_jacobian(codes[o], R.sample(g["o_o"][o, idx], g["d_o"][o, idx], ex["t"][idx]))
            gw[idx] = A.world_gradient(np.repeat(g["rt"][o:o + 1], idx.size, 0), np.full(idx.size, g["scale"][o], F32), np.asarray(grad)[:, -3:])
    return dict(obj=ex["obj"], t=ex["t"], dist=ex["dist"], status=ex["status"], gw=gw, stats=ex["stats"])


def evaluate(T, pts_s, org_s, w, eng, amap, codes, huber, max_dist, max_gap, raycast=None, budget=None):
    """One evaluation at pose T -> dict(sums, cost, n_used, obj, dist, t, status, cast_obj, pw, gw, stats)."""
    pw, ow, dirv = build(T, pts_s, org_s)
    n = pw.shape[0]
    if amap.t.shape[0] and n:
        c = cast(eng, amap.t, codes, ow, dirv, raycast, budget)
    else:
        c = dict(obj=np.full(n, -1, np.int32), t=np.full(n, np.inf, F32), dist=np.full(n, np.inf, F32), status=np.zeros(n, np.int32),
                 gw=np.zeros((n, 3), F32), stats=None)
    obj_row, d, sums = ray_rows(ow, pw, c["obj"], c["t"], c["dist"], c["status"], c["gw"], w, huber, max_dist, max_gap)
    return dict(sums=sums, cost=A.cost_of(sums, huber, max_dist), n_used=int(sums[A.IDX_N]), obj=obj_row, dist=d, t=c["t"], status=c["status"],
                cast_obj=c["obj"], pw=pw, gw=c["gw"], stats=c["stats"])


def evaluator(eng, codes, org_s, max_gap, raycast=None):
    """The pipeline's evaluation with align_ref.run's signature (its `decode` argument is not used: the engine decodes)."""
    def ev(T, pts_s, w, amap, decode, huber, max_dist):
        return evaluate(T, pts_s, org_s, w, eng, amap, codes, huber, max_dist, max_gap, raycast)
    return ev


# ---- float64: the algorithm --------------------------------------------------------------------------------------------------------------
def cast64(amap, decode, ow, u, eps=1e-3, max_steps=64, t_min=0.0, t_max=np.inf):
    """Sphere tracing in float64 inside every object's unit sphere, nearest hit per ray.  decode(o, p_obj) -> (sdf, d sdf / d xyz) float64.
    -> obj, t, dist, status, gw (world gradient of sdf s at the hit sample)."""
    n = ow.shape[0]
    best_t, best_o, best_d = np.full(n, np.inf), np.full(n, -1, np.int32), np.full(n, np.inf)
    exh_t = np.full(n, np.inf)
    gw = np.zeros((n, 3), F64)
    ok = np.isfinite(ow).all(1) & np.isfinite(u).all(1)
    for o in range(amap.t.shape[0]):
        if not np.isfinite(amap.s_sel[o]):
            continue
        inv = np.linalg.inv(amap.t[o].astype(F64))
        s = float(amap.s[o])
        o_o, d_o = ow @ inv[:3, :3].T + inv[:3, 3], u @ inv[:3, :3].T
        with np.errstate(all="ignore"):
            a, b, c = (d_o * d_o).sum(1), (o_o * d_o).sum(1), (o_o * o_o).sum(1) - 1.0
            disc = b * b - a * c
            q = np.sqrt(disc)
            t_in, t_out = (-b - q) / a, (q - b) / a
            exists = ok & (disc > 0) & (t_out > t_min) & (t_in < t_max)
        idx = np.flatnonzero(exists)
        t, t1 = np.maximum(t_in[idx], t_min), np.minimum(t_out[idx], t_max)
        live = np.ones(idx.size, bool)
        for _ in range(int(max_steps)):
            k = np.flatnonzero(live)
            if k.size == 0:
                break
            sdf, grad = decode(o, o_o[idx[k]] + t[k, None] * d_o[idx[k]])
            dist = np.asarray(sdf, F64) * s
            hit = dist <= eps
            h = k[hit]
            better = t[h] < best_t[idx[h]]
            r = idx[h[better]]
            best_t[r], best_o[r], best_d[r] = t[h[better]], o, dist[hit][better]
            gw[r] = (np.asarray(grad, F64).reshape(-1, 3)[hit][better] @ inv[:3, :3]) * s
            live[h] = False
            adv = k[~hit]
            tn = t[adv] + dist[~hit]
            gone = ~(tn <= t1[adv])
            live[adv[gone]] = False
            t[adv[~gone]] = tn[~gone]
        ex = np.flatnonzero(live)
        np.minimum.at(exh_t, idx[ex], t[ex])
    status = np.where(best_o >= 0, np.where(exh_t < best_t, UNDECIDED, HIT), np.where(np.isfinite(exh_t), UNDECIDED, MISS)).astype(np.int32)
    return dict(obj=best_o, t=best_t, dist=best_d, status=status, gw=gw)


def evaluate64(T, pts_s, org_s, w, amap, decode, huber, max_dist, max_gap, eps=1e-3, max_steps=64):
    pts_s = np.asarray(pts_s, F64).reshape(-1, 3)
    org_s = np.zeros_like(pts_s) if org_s is None else np.asarray(org_s, F64).reshape(-1, 3)
    T = np.asarray(T, F64).reshape(4, 4)
    pw, ow = pts_s @ T[:3, :3].T + T[:3, 3], org_s @ T[:3, :3].T + T[:3, 3]
    dirv = pw - ow
    with np.errstate(all="ignore"):
        length = np.sqrt((dirv * dirv).sum(1))
        u = dirv / length[:, None]
    c = cast64(amap, decode, ow, u, eps, max_steps)
    with np.errstate(all="ignore"):
        gap = length - c["t"]
        d = c["dist"] + (c["gw"] * u).sum(1) * gap
        matched = (c["status"] == HIT) & (c["obj"] >= 0) & np.isfinite(gap) & (np.abs(gap) <= max_gap)
    obj_row = np.where(matched, c["obj"], -1).astype(np.int32)
    d = np.where(c["obj"] >= 0, d, np.inf)
    sums = A.tree_sum(A.row_terms(pw, obj_row, d, c["gw"], None if w is None else np.asarray(w, F64), huber, max_dist))
    return dict(sums=sums, cost=A.cost_of(sums, huber, max_dist), n_used=int(sums[A.IDX_N]), obj=obj_row, dist=d, t=c["t"], status=c["status"],
                cast_obj=c["obj"], pw=pw, gw=c["gw"])


def evaluator64(org_s, max_gap, eps=1e-3, max_steps=64):
    def ev(T, pts_s, w, amap, decode, huber, max_dist):
        return evaluate64(T, pts_s, org_s, w, amap, decode, huber, max_dist, max_gap, eps, max_steps)
    return ev


def observe64(amap, decode, T_true, dirs_s, eps=1e-5, max_steps=256):
    """Observations in float64: the cast of the sensor-frame unit directions dirs_s from the sensor origin at T_true.  -> pts_s (n, 3) (NaN
    rows where nothing is hit), obj (n,)."""
    T = np.asarray(T_true, F64).reshape(4, 4)
    u_s = np.asarray(dirs_s, F64).reshape(-1, 3)
    u_s = u_s / np.sqrt((u_s * u_s).sum(1))[:, None]
    c = cast64(amap, decode, np.broadcast_to(T[:3, 3], u_s.shape).copy(), u_s @ T[:3, :3].T, eps, max_steps)
    hit = (c["status"] == HIT) & (c["obj"] >= 0)
    return np.where(hit[:, None], u_s * c["t"][:, None], np.nan), np.where(hit, c["obj"], -1)
