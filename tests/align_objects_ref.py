"""numpy restatement of the opening comment of dsp_slam_amd/csrc/align_objects_math.h (the arithmetic of dsp_map_align_objects) and of the
loop around it.  The cast, the gradient, the residual and the match are tests/align_rays_ref.py's, the rows, the tree, the step and the step
rule tests/align_ref.py's; what is restated here is what is new: the composition of a correction with an input pose, the sums SEGMENTED by
the object a ray sees, the sign of b, and the loop over objects that are coupled through one cast.

evaluator(...) makes the pipeline's evaluation (float32 poses; what the device must return bit for bit when `eng` is the device's Engine);
evaluator64(...) the ALGORITHM with nothing rounded to float32.  Both are called as evaluate(C (n_obj, 4, 4) float64) -> dict(sums
(n_obj, NSUM), winner, obj, dist, t, status).
"""
import math

import numpy as np

import align_rays_ref as AR
import align_ref as A
import query_ref as Q

F32, F64 = np.float32, np.float64
NSUM = A.NSUM


# ---- compose ---------------------------------------------------------------------------------------------------------------------------
def compose(C, T0):
    """C (4, 4) float64 rigid, T0 (4, 4) float32 -> (4, 4) float32: C T0 in float64, dot products (a0 b0 + a1 b1) + a2 b2, every entry rounded
    once; T0's own bytes when C is exactly the identity."""
    C = np.asarray(C, F64).reshape(4, 4)
    T0 = np.asarray(T0, F32).reshape(4, 4)
    if np.array_equal(C, np.eye(4)):
        return T0.copy()
    t = T0.astype(F64)
    out = np.zeros((4, 4), F32)
    for i in range(3):
        for j in range(3):
            out[i, j] = F32((C[i, 0] * t[0, j] + C[i, 1] * t[1, j]) + C[i, 2] * t[2, j])
        out[i, 3] = F32(((C[i, 0] * t[0, 3] + C[i, 1] * t[1, 3]) + C[i, 2] * t[2, 3]) + C[i, 3])
    out[3, 3] = 1.0
    return out


def compose_all(C, T0):
    C, T0 = np.asarray(C, F64).reshape(-1, 4, 4), np.asarray(T0, F32).reshape(-1, 4, 4)
    return np.stack([compose(c, t) for c, t in zip(C, T0)]) if C.shape[0] else np.zeros((0, 4, 4), F32)


# ---- the segmented sums ----------------------------------------------------------------------------------------------------------------
def rows(pw, winner, obj_row, d, gw, w, n_obj, huber, max_dist):
    """What dsp_debug_align_objects_rows returns: (n_obj, NSUM).  Object k's rows are those with winner == k in ascending ray order; its sums
    are align_ref's rows through align_ref's tree over that LIST; b negated."""
    winner = np.asarray(winner, np.int32)
    gw = np.asarray(gw).reshape(-1, 3)
    g = np.where((np.asarray(obj_row) >= 0)[:, None], gw, gw.dtype.type(0))      # read only where the row is matched
    terms = A.row_terms(pw, obj_row, d, g, w, huber, max_dist)
    out = np.zeros((n_obj, NSUM), F64)
    for k in range(n_obj):
        out[k] = A.tree_sum(terms[winner == k])
        out[k, A.IDX_B:A.IDX_B + 6] = -out[k, A.IDX_B:A.IDX_B + 6]
    return out


def check(params, raycast, max_gap, has_origins, n_rays, n_obj):
    """True: dsp_debug_align_objects_check accepts (weights aside).  params: a dict with max_dist."""
    if not AR.R.check(AR.R.params(**raycast)):
        return False
    if not max_gap >= params["max_dist"]:
        return False
    if n_rays > 2 ** 31 - 1 or (n_rays > 0 and not has_origins):
        return False
    return not (n_obj > 0 and n_rays > 0 and (n_obj * 1024 * 4 > (64 << 20) or n_obj * (-(-n_rays // 64)) * 4 > (64 << 20)))


# ---- one evaluation ----------------------------------------------------------------------------------------------------------------------
def evaluate(poses32, codes, pts_w, org_w, w, eng, huber, max_dist, max_gap, raycast=None, budget=None):
    """The pipeline's evaluation of the map at the float32 poses: ONE cast of all rays, the rows per winner."""
    pw, ow = np.asarray(pts_w, F32).reshape(-1, 3), np.asarray(org_w, F32).reshape(-1, 3)
    n, n_obj = pw.shape[0], len(codes)
    with np.errstate(all="ignore"):
        dirv = (pw - ow).astype(F32)
    c = AR.cast(eng, np.asarray(poses32, F32).reshape(-1, 4, 4), codes, ow, dirv, raycast, budget)
    obj_row, d = AR.residual(ow, pw, c["obj"], c["t"], c["dist"], c["status"], c["gw"], max_gap)
    sums = rows(pw, c["obj"], obj_row, d, c["gw"], w, n_obj, huber, max_dist)
    return dict(sums=sums, winner=c["obj"], obj=obj_row, dist=d, t=c["t"], status=c["status"], gw=c["gw"], stats=c["stats"])


def evaluator(eng, T0, codes, pts_w, org_w, w, huber, max_dist, max_gap, raycast=None, budget=None):
    T0 = np.asarray(T0, F32).reshape(-1, 4, 4)

    def ev(C):
        return evaluate(compose_all(C, T0), codes, pts_w, org_w, w, eng, huber, max_dist, max_gap, raycast, budget)
    return ev


class Map64:
    """what align_rays_ref.cast64 reads of a map, in float64"""

    def __init__(self, t, codes):
        self.t = np.asarray(t, F64).reshape(-1, 4, 4)
        self.s = np.array([np.cbrt(np.linalg.det(x[:3, :3])) for x in self.t], F64)
        self.s_sel = np.array([s if np.isfinite(np.asarray(c, F32)).all() else np.nan for s, c in zip(self.s, codes)], F64)


def evaluate64(T, codes, decode, pts_w, org_w, w, huber, max_dist, max_gap, eps=1e-3, max_steps=64):
    """The evaluation with nothing rounded to float32: float64 poses T (n_obj, 4, 4), rays, sphere tracer and decoder."""
    pw, ow = np.asarray(pts_w, F64).reshape(-1, 3), np.asarray(org_w, F64).reshape(-1, 3)
    dirv = pw - ow
    with np.errstate(all="ignore"):
        length = np.sqrt((dirv * dirv).sum(1))
        u = dirv / length[:, None]
    c = AR.cast64(Map64(T, codes), decode, ow, u, eps, max_steps)
    with np.errstate(all="ignore"):
        gap = length - c["t"]
        d = c["dist"] + (c["gw"] * u).sum(1) * gap
        matched = (c["status"] == AR.HIT) & (c["obj"] >= 0) & np.isfinite(gap) & (np.abs(gap) <= max_gap)
    obj_row = np.where(matched, c["obj"], -1).astype(np.int32)
    d = np.where(c["obj"] >= 0, d, np.inf)
    sums = rows(pw, c["obj"], obj_row, d, c["gw"], None if w is None else np.asarray(w, F64), len(codes), huber, max_dist)
    return dict(sums=sums, winner=c["obj"], obj=obj_row, dist=d, t=c["t"], status=c["status"], gw=c["gw"])


def evaluator64(T0, codes, decode, pts_w, org_w, w, huber, max_dist, max_gap, eps=1e-3, max_steps=64):
    T0 = np.asarray(T0, F64).reshape(-1, 4, 4)

    def ev(C):
        return evaluate64(np.asarray(C, F64).reshape(-1, 4, 4) @ T0, codes, decode, pts_w, org_w, w, huber, max_dist, max_gap, eps, max_steps)
    return ev


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
def run(n_obj, evaluate, refine=None, n_rays=1, **params):
    """The loop of dsp_map_align_objects: align_ref.run's body per object, the objects evaluated TOGETHER: at every evaluation a live object
    stands at its trial correction and every other one at its accepted correction.  -> a list of dicts per object (correction, status,
    evaluations, steps, cost0, cost, n_used, sums, lam, trace=[dict(pose, decision, cost, lam, n_used, sums, xi)])."""
    p = dict(A.DEFAULTS)
    p.update(params)
    sc = p["step_control"]
    step_on = sc is not None and any(v != 0 for v in sc)
    iters, huber, max_dist, min_points = p["iterations"], p["huber"], p["max_dist"], p["min_points"]
    rho_gate = float(A.rho(max_dist, huber))
    st = [dict(C_eval=np.eye(4), acc=None, lam=0.0, steps=0, status=A.OK, live=bool(refine is None or refine[k]), cost0=rho_gate, trace=[])
          for k in range(n_obj)]
    if n_rays == 0:
        for s in st:
            if s["live"]:
                s["live"], s["status"] = False, A.NO_SUPPORT
    for e in range(iters):
        if not any(s["live"] for s in st):
            break
        C = np.stack([s["C_eval"] if s["live"] else (s["acc"]["pose"] if s["acc"] else np.eye(4)) for s in st])
        ev = evaluate(C)
        for k, s in enumerate(st):
            if not s["live"]:
                continue
            sums = ev["sums"][k]
            F, n_used = A.cost_of(sums, huber, max_dist), int(sums[A.IDX_N])
            support = n_used >= min_points
            if e == 0:
                s["cost0"] = F
            dec = A.ACCEPTED
            if step_on:
                dec, s["lam"] = A.decide(True, F, 0.0, sc, s["lam"]) if s["acc"] is None else A.decide(False, F if support else math.inf, s["acc"]["cost"], sc,
                                                                                                     s["lam"])
            if dec == A.ACCEPTED:
                if s["acc"] is not None:
                    s["steps"] += 1
                s["acc"] = dict(pose=s["C_eval"], sums=sums, cost=F, n_used=n_used)
            rec = dict(pose=s["C_eval"], decision=dec, cost=F, lam=s["lam"], n_used=n_used, sums=sums, xi=None)
            s["trace"].append(rec)
            acc = s["acc"]
            if acc["n_used"] < min_points:
                s["live"], s["status"] = False, A.NO_SUPPORT
                continue
            H, b = A.full_h(acc["sums"]), acc["sums"][A.IDX_B:A.IDX_B + 6]
            xi, tries = None, 0
            while True:
                xi = A.solve(H, b, p["damp"], s["lam"])
                if xi is not None or not step_on or tries >= 64 or not s["lam"] < sc[4]:
                    break
                s["lam"] = min(max(s["lam"], sc[3]) * sc[1], sc[4])
                tries += 1
            rec["lam"] = s["lam"]
            if xi is None:
                s["live"], s["status"] = False, A.SINGULAR
                continue
            rec["xi"] = xi
            if np.abs(xi[:3]).max() < p["trans_tol"] and np.abs(xi[3:]).max() < p["rot_tol"]:
                s["live"], s["status"] = False, A.CONVERGED
                continue
            if e == iters - 1:
                s["live"], s["status"] = False, A.OK
                continue
            s["C_eval"] = A.apply_step(xi, acc["pose"])
    out = []
    for s in st:
        acc = s["acc"]
        out.append(dict(correction=acc["pose"] if acc else np.eye(4), status=s["status"], evaluations=len(s["trace"]), steps=s["steps"], cost0=s["cost0"],
                        cost=acc["cost"] if acc else rho_gate, n_used=acc["n_used"] if acc else 0, sums=acc["sums"] if acc else np.zeros(NSUM), lam=s["lam"],
                        trace=s["trace"]))
    return out


def run64(T0, codes, decode, pts_w, org_w, w=None, refine=None, max_gap=0.6, eps=1e-3, max_steps=64, **params):
    """The float64 loop on its own.  -> run's list, each with `pose`: the float64 pose C_k T_k0."""
    p = dict(A.DEFAULTS)
    p.update(params)
    T0 = np.asarray(T0, F64).reshape(-1, 4, 4)
    ev = evaluator64(T0, codes, decode, pts_w, org_w, w, p["huber"], p["max_dist"], max_gap, eps, max_steps)
    res = run(T0.shape[0], ev, refine, n_rays=np.asarray(pts_w).reshape(-1, 3).shape[0], **params)
    for r, t in zip(res, T0):
        r["pose"] = r["correction"] @ t
    return res
