"""numpy restatement of dsp_slam_amd/csrc/align_math.h (the arithmetic of dsp_map_align) and of the loop around it: the same operations in
the same order and the same summation tree, so that the host functions and the device are held to it bit for bit.

float32 parts (point transform, world gradient) reuse tests/query_ref.py (to_object / fmaf32: one rounding per operation).  float64 parts
are plain numpy / Python float operations, one rounding each; the Cholesky step uses only + - * / sqrt, which IEEE rounds identically
everywhere.  exp_se3 calls sin / cos, which may differ from the C library's in the last place.

The decoder is a callback  decode(o, p_obj (n, 3) float32) -> (sdf (n,) float32, d sdf / d xyz (n, 3) float32)  for object o of the map, so
the same evaluation and loop run on the float64 oracle (CPU; rounded to float32) or on Engine.sdf_jacobian rows (GPU).
"""
import math

import numpy as np

import query_ref as Q

F32, F64 = np.float32, np.float64
BLOCK, WAVE = 256, 64
IDX_H, IDX_B, IDX_COST, IDX_W, IDX_N, NSUM = 0, 21, 27, 28, 29, 30
SMALL_TH2 = 1e-8
OK, CONVERGED, NO_SUPPORT, SINGULAR = 0, 1, 2, 3
NOT_EVALUATED, ACCEPTED, REJECTED = 0, 1, 2
IU = np.triu_indices(6)
DEFAULTS = dict(iterations=10, min_points=6, max_dist=0.3, huber=0.05, damp=0.0, trans_tol=1e-6, rot_tol=1e-6, step_control=None)


# ---- float32: transform and world gradient ---------------------------------------------------------------------------------------------
def pose_rt(T):
    """the pose's [R | t], every entry rounded once to float32: (12,)"""
    return np.asarray(T, F64).reshape(4, 4)[:3, :].astype(F32).reshape(12)


def transform(T, pts_s):
    return Q.to_object(pose_rt(T)[None], pts_s)[0]


def world_gradient(rt, s, g):
    """rt (n, 12), s (n,) of each row's object, g (n, 3) object-frame gradients -> g_w (n, 3): the u of query_ref.normals times s."""
    rt = np.asarray(rt, F32).reshape(-1, 3, 4)
    g = np.asarray(g, F32).reshape(-1, 3)
    s = np.asarray(s, F32).reshape(-1)
    out = np.zeros_like(g)
    with np.errstate(all="ignore"):
        for j in range(3):
            u = Q.fmaf32(rt[:, 2, j], g[:, 2], Q.fmaf32(rt[:, 1, j], g[:, 1], rt[:, 0, j] * g[:, 0]))
            out[:, j] = u * s
    return out


# ---- float64: rows, tree, cost ---------------------------------------------------------------------------------------------------------
def rho(d, huber):
    d = np.asarray(d, F64)
    a = np.abs(d)
    with np.errstate(all="ignore"):
        return np.where(a <= huber, d * d, huber * (2.0 * a - huber))


def row_terms(pw, obj, dist, gw, w, huber, max_dist):
    """-> terms (n, NSUM) float64."""
    pw, gw = np.asarray(pw).reshape(-1, 3), np.asarray(gw).reshape(-1, 3)      # float32 (the pipeline) or float64 (evaluate64)
    n = pw.shape[0]
    obj, dist = np.asarray(obj, np.int32), np.asarray(dist)
    w32 = np.ones(n, F32) if w is None else np.asarray(w)
    term = np.zeros((n, NSUM), F64)
    with np.errstate(all="ignore"):
        valid = np.isfinite(pw).all(1) & (w32 > 0) & np.isfinite(w32)
        used = valid & (obj >= 0) & np.isfinite(dist) & np.isfinite(gw).all(1) & (np.abs(dist.astype(F64)) <= max_dist)
        w64 = w32.astype(F64)
        d = dist.astype(F64)
        a = np.abs(d)
        p, g = pw.astype(F64), gw.astype(F64)
        J = np.stack([g[:, 0], g[:, 1], g[:, 2], p[:, 1] * g[:, 2] - p[:, 2] * g[:, 1], p[:, 2] * g[:, 0] - p[:, 0] * g[:, 2],
                      p[:, 0] * g[:, 1] - p[:, 1] * g[:, 0]], 1)
        wh = np.where(a <= huber, 1.0, huber / a)
        ww = w64 * wh
        k = IDX_H
        for i in range(6):
            t = ww * J[:, i]
            for j in range(i, 6):
                term[:, k] = t * J[:, j]
                k += 1
            term[:, IDX_B + i] = -(t * d)
        term[:, IDX_COST] = w64 * rho(d, huber)
        term[:, IDX_N] = 1.0
        term[~used] = 0.0
        term[valid & ~used, IDX_COST] = (w64 * float(rho(max_dist, huber)))[valid & ~used]
        term[valid, IDX_W] = w64[valid]
    return term


def tree_sum(terms):
    """The written tree: blocks of BLOCK points padded with zeros; inside each wave of WAVE the butterfly l + (l ^ m), m = 32 .. 1; the
    block's waves ascending; the blocks ascending."""
    terms = np.asarray(terms, F64).reshape(-1, NSUM)
    n = terms.shape[0]
    if n == 0:
        return np.zeros(NSUM, F64)
    nb = -(-n // BLOCK)
    x = np.zeros((nb * BLOCK, NSUM), F64)
    x[:n] = terms
    x = x.reshape(nb, BLOCK // WAVE, WAVE, NSUM)
    m = WAVE // 2
    while m >= 1:
        x = x[:, :, :m] + x[:, :, m:2 * m]
        m //= 2
    x = x[:, :, 0]
    blk = x[:, 0]
    for w in range(1, BLOCK // WAVE):
        blk = blk + x[:, w]
    s = blk[0]
    for b in range(1, nb):
        s = s + blk[b]
    return s


def cost_of(sums, huber, max_dist):
    return float(rho(max_dist, huber)) if sums[IDX_W] == 0.0 else float(sums[IDX_COST] / sums[IDX_W])


def full_h(sums):
    H = np.zeros((6, 6), F64)
    H[IU] = sums[IDX_H:IDX_H + 21]
    H[(IU[1], IU[0])] = sums[IDX_H:IDX_H + 21]
    return H


# ---- float64: step ---------------------------------------------------------------------------------------------------------------------
def solve(H, b, damp, lam):
    """Cholesky of H + (damp + lam) I in the header's order -> xi (6,) or None (SINGULAR)."""
    H = np.asarray(H, F64).reshape(6, 6)
    dl = float(damp) + float(lam)
    A = [[float(H[min(i, j), max(i, j)]) for j in range(6)] for i in range(6)]
    for i in range(6):
        A[i][i] = A[i][i] + dl
    Lm = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - Lm[j][k] * Lm[j][k]
        if not (s > 0.0) or not math.isfinite(s):
            return None
        Lm[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            q = A[i][j]
            for k in range(j):
                q = q - Lm[i][k] * Lm[j][k]
            Lm[i][j] = q / Lm[j][j]
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for k in range(i):
            s = s - Lm[i][k] * y[k]
        y[i] = s / Lm[i][i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - Lm[k][i] * x[k]
        x[i] = s / Lm[i][i]
    if not all(math.isfinite(v) for v in x):
        return None
    return np.array(x, F64)


def apply_step(xi, T):
    """exp_se3(xi) T, closed form, in the header's order."""
    xi = [float(v) for v in xi]
    T = np.asarray(T, F64).reshape(4, 4)
    w0, w1, w2 = xi[3], xi[4], xi[5]
    th2 = (w0 * w0 + w1 * w1) + w2 * w2
    th = math.sqrt(th2)
    if th2 < SMALL_TH2:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        sn, cs = math.sin(th), math.cos(th)
        a, b, c = sn / th, (1.0 - cs) / th2, (th - sn) / (th2 * th)
    W = [[0.0, -w2, w1], [w2, 0.0, -w0], [-w1, w0, 0.0]]
    W2 = [[(W[i][0] * W[0][j] + W[i][1] * W[1][j]) + W[i][2] * W[2][j] for j in range(3)] for i in range(3)]
    R = [[((1.0 if i == j else 0.0) + a * W[i][j]) + b * W2[i][j] for j in range(3)] for i in range(3)]
    V = [[((1.0 if i == j else 0.0) + b * W[i][j]) + c * W2[i][j] for j in range(3)] for i in range(3)]
    t = [(V[i][0] * xi[0] + V[i][1] * xi[1]) + V[i][2] * xi[2] for i in range(3)]
    out = np.zeros((4, 4), F64)
    for i in range(3):
        for j in range(3):
            out[i, j] = (R[i][0] * T[0, j] + R[i][1] * T[1, j]) + R[i][2] * T[2, j]
        out[i, 3] = ((R[i][0] * T[0, 3] + R[i][1] * T[1, 3]) + R[i][2] * T[2, 3]) + t[i]
    out[3, 3] = 1.0
    return out


def check_pose(T):
    """align_math::check_pose: True when dsp_map_align accepts the initial pose."""
    T = np.asarray(T, F64).reshape(4, 4)
    if not np.isfinite(T).all() or T[3, 0] != 0 or T[3, 1] != 0 or T[3, 2] != 0 or T[3, 3] != 1:
        return False
    a = T[:3, :3]
    n = [(a[0, c] * a[0, c] + a[1, c] * a[1, c]) + a[2, c] * a[2, c] for c in range(3)]
    s2 = ((n[0] + n[1]) + n[2]) / 3.0
    if not s2 > 0:
        return False
    s = math.sqrt(s2)
    if not abs(s - 1.0) <= Q.RIGID_TOL:
        return False
    for r in range(3):
        for c in range(3):
            d = 0.0
            for k in range(3):
                d = d + (a[k, r] / s) * (a[k, c] / s)
            if not abs(d - (1.0 if r == c else 0.0)) <= Q.RIGID_TOL:
                return False
    with np.errstate(over="ignore"):
        return bool(np.isfinite(T[:3].astype(F32)).all())


# ---- the step rule (csrc/step_rule.h) --------------------------------------------------------------------------------------------------
def decide(first, F, F_acc, sc, lam):
    """-> (decision, lambda); sc = (lambda0, up, down, lambda_min, lambda_max)."""
    lambda0, up, down, lmin, lmax = sc
    if first:
        return ACCEPTED, float(lambda0)
    if F < F_acc:
        return ACCEPTED, lam * down
    return REJECTED, min(max(lam, lmin) * up, lmax)


# ---- one evaluation and the loop -------------------------------------------------------------------------------------------------------
class Map:
    """The map as the query sees it: the reference's inverted poses, and which objects may win."""

    def __init__(self, t_world_obj, codes):
        self.t = np.asarray(t_world_obj, F32).reshape(-1, 4, 4)
        self.rt, self.s, ok = Q.invert(self.t)
        assert ok.all()
        self.s_sel = np.array([s if np.isfinite(np.asarray(c, F32)).all() else np.nan for s, c in zip(self.s, codes)], F32).reshape(-1)


def evaluate(T, pts_s, w, amap, decode, huber, max_dist):
    """One evaluation at pose T -> dict(sums, cost, n_used, obj, dist, pw, gw): transform, containment, decoder rows per object at the
    reference's object-frame points, selection (query_ref), the winner's world gradient, rows and tree."""
    pts_s = np.asarray(pts_s, F32).reshape(-1, 3)
    n = pts_s.shape[0]
    pw = transform(T, pts_s)
    obj, dist, gw = np.full(n, -1, np.int32), np.full(n, np.inf, F32), np.zeros((n, 3), F32)
    if amap.t.shape[0] and n:
        p_obj, inside, _ = Q.candidates(amap.rt, amap.s, pw)
        sdf, sc, ob, pt, gr = [], [], [], [], []
        for o in range(amap.t.shape[0]):
            idx = np.flatnonzero(inside[o])
            if idx.size == 0:
                continue
            v, g = decode(o, p_obj[o, idx])
            sdf.append(np.asarray(v, F32)); gr.append(np.asarray(g, F32).reshape(-1, 3))
            sc.append(np.full(idx.size, amap.s_sel[o], F32)); ob.append(np.full(idx.size, o, np.int32)); pt.append(idx.astype(np.int32))
        if sdf:
            sdf, sc, ob, pt, gr = np.concatenate(sdf), np.concatenate(sc), np.concatenate(ob), np.concatenate(pt), np.concatenate(gr)
            obj, dist = Q.select(sdf, sc, ob, pt, n)
            with np.errstate(all="ignore"):
                win = (obj[pt] == ob) & (Q.keys(sdf * sc, ob) == Q.keys(dist[pt], obj[pt]))
            gw[pt[win]] = world_gradient(amap.rt[ob[win]], amap.s[ob[win]], gr[win])
    sums = tree_sum(row_terms(pw, obj, dist, gw, w, huber, max_dist))
    return dict(sums=sums, cost=cost_of(sums, huber, max_dist), n_used=int(sums[IDX_N]), obj=obj, dist=dist, pw=pw, gw=gw)


def evaluate64(T, pts_s, w, amap, decode, huber, max_dist):
    """The evaluation with nothing rounded to float32 -- the ALGORITHM, not the pipeline: float64 points, transform, containment and
    decoder values (decode returns float64), then the same rows and tree."""
    pts_s = np.asarray(pts_s, F64).reshape(-1, 3)
    T = np.asarray(T, F64).reshape(4, 4)
    n = pts_s.shape[0]
    pw = pts_s @ T[:3, :3].T + T[:3, 3]
    obj, dist, gw = np.full(n, -1, np.int32), np.full(n, np.inf, F64), np.zeros((n, 3), F64)
    for o in range(amap.t.shape[0]):
        inv = np.linalg.inv(amap.t[o].astype(F64))
        s = float(amap.s[o])
        p_o = pw @ inv[:3, :3].T + inv[:3, 3]
        idx = np.flatnonzero((p_o * p_o).sum(1) < 1.0)
        if idx.size == 0 or not np.isfinite(amap.s_sel[o]):
            continue
        v, g = decode(o, p_o[idx])
        d = np.asarray(v, F64) * s
        better = d < dist[idx]
        k = idx[better]
        obj[k], dist[k] = o, d[better]
        gw[k] = (np.asarray(g, F64).reshape(-1, 3)[better] @ inv[:3, :3]) * s
    sums = tree_sum(row_terms(pw, obj, dist, gw, None if w is None else np.asarray(w, F64), huber, max_dist))
    return dict(sums=sums, cost=cost_of(sums, huber, max_dist), n_used=int(sums[IDX_N]), obj=obj, dist=dist, pw=pw, gw=gw)


def run(T0, pts_s, w, amap, decode, evaluate=evaluate, **params):
    """The loop of dsp_map_align for ONE hypothesis -> dict(pose, status, evaluations, steps, cost0, cost, n_used, sums, lam, obj, dist,
    trace=[dict(pose, decision, cost, lam, n_used, sums, xi)]).  evaluate: the pipeline's evaluation above, or evaluate64."""
    p = dict(DEFAULTS)
    p.update(params)
    sc = p["step_control"]
    step_on = sc is not None and any(v != 0 for v in sc)
    iters, huber, max_dist, min_points = p["iterations"], p["huber"], p["max_dist"], p["min_points"]
    T_eval = np.array(T0, F64).reshape(4, 4)
    acc, lam, steps, status, trace, cost0 = None, 0.0, 0, OK, [], None
    n_pts = np.asarray(pts_s).reshape(-1, 3).shape[0]
    if n_pts == 0 or amap.t.shape[0] == 0:
        c = float(rho(max_dist, huber))
        return dict(pose=T_eval, status=NO_SUPPORT, evaluations=0, steps=0, cost0=c, cost=c, n_used=0, sums=np.zeros(NSUM), lam=0.0,
                    obj=np.full(n_pts, -1, np.int32), dist=np.full(n_pts, np.inf, F32), trace=[])
    for e in range(iters):
        ev = evaluate(T_eval, pts_s, w, amap, decode, huber, max_dist)
        ev["pose"] = T_eval
        F, support = ev["cost"], ev["n_used"] >= min_points
        if e == 0:
            cost0 = F
        dec = ACCEPTED
        if step_on:
            dec, lam = decide(True, F, 0.0, sc, lam) if acc is None else decide(False, F if support else math.inf, acc["cost"], sc, lam)
        if dec == ACCEPTED:
            if acc is not None:
                steps += 1
            acc = ev
        rec = dict(pose=T_eval, decision=dec, cost=F, lam=lam, n_used=ev["n_used"], sums=ev["sums"], xi=None)
        trace.append(rec)
        if acc["n_used"] < min_points:
            status = NO_SUPPORT
            break
        H, b = full_h(acc["sums"]), acc["sums"][IDX_B:IDX_B + 6]
        xi, tries = None, 0
        while True:
            xi = solve(H, b, p["damp"], lam)
            if xi is not None or not step_on or tries >= 64 or not lam < sc[4]:
                break
            lam = min(max(lam, sc[3]) * sc[1], sc[4])
            tries += 1
        rec["lam"] = lam
        if xi is None:
            status = SINGULAR
            break
        rec["xi"] = xi
        if np.abs(xi[:3]).max() < p["trans_tol"] and np.abs(xi[3:]).max() < p["rot_tol"]:
            status = CONVERGED
            break
        if e == iters - 1:
            status = OK
            break
        T_eval = apply_step(xi, acc["pose"])
    return dict(pose=acc["pose"], status=status, evaluations=len(trace), steps=steps, cost0=cost0, cost=acc["cost"], n_used=acc["n_used"],
                sums=acc["sums"], lam=lam, obj=acc["obj"], dist=acc["dist"], trace=trace)


# ---- helpers for the tests -------------------------------------------------------------------------------------------------------------
def axis_angle(axis, angle):
    axis = np.asarray(axis, F64)
    axis = axis / np.sqrt((axis * axis).sum())
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def rigid(rot, trans):
    T = np.eye(4)
    T[:3, :3] = rot
    T[:3, 3] = trans
    return T


def offset_pose(rng, T, deg, trans, centre):
    """T moved (on the left, world frame) by a rotation of `deg` degrees about a random axis through `centre` -- the cloud's centroid in
    the world, so that the rotation moves no point by more than deg x the cloud's radius -- and a translation of length `trans` in a
    random direction."""
    centre = np.asarray(centre, F64)
    d = rng.normal(size=3)
    d = d / np.sqrt((d * d).sum()) * trans
    R = axis_angle(rng.normal(size=3), math.radians(deg))
    return rigid(np.eye(3), centre + d) @ rigid(R, np.zeros(3)) @ rigid(np.eye(3), -centre) @ T


def pose_error(T, T_true):
    """(translation error, rotation error in radians) of T against T_true."""
    D = np.asarray(T, F64) @ np.linalg.inv(np.asarray(T_true, F64))
    c = min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1.0) / 2.0))
    s = np.sqrt(((D[:3, :3] - D[:3, :3].T) ** 2).sum() / 8.0)        # |sin|: accurate near zero, where acos is not
    return float(np.sqrt((D[:3, 3] ** 2).sum())), float(math.atan2(s, c))
