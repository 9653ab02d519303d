"""numpy restatement of the opening comment of dsp_slam_amd/csrc/align_shapes_math.h (the arithmetic of dsp_map_align_shapes) and of the loop
around it.  The cast, the gradient, the residual and the match are tests/align_rays_ref.py's, compose and the owner rule
tests/align_objects_ref.py's; what is restated here is what is new: the 70-entry jacobian row with the code derivatives, the sums in
sequential blocks, the step on the mean system with regulariser and pins, and the loop whose state carries a code.

evaluator(...) makes the pipeline's evaluation (float32 poses and codes; what the device must return bit for bit when `eng` is the device's
Engine); evaluator64(...) the ALGORITHM with nothing rounded to float32.  Both are called as evaluate(C (n_obj, 4, 4) float64, z (n_obj, 64)
float64) -> dict(sums (n_obj, NSUM), winner, obj, dist, t, status).
"""
import math

import numpy as np

import align_objects_ref as AO
import align_rays_ref as AR
import align_ref as A
import raycast_ref as R

F32, F64 = np.float32, np.float64
BLOCK, CODE, DIM = 128, 64, 70
NPAIR = DIM * (DIM + 1) // 2
IDX_H, IDX_B, IDX_COST, IDX_W, IDX_N, NSUM = 0, NPAIR, NPAIR + DIM, NPAIR + DIM + 1, NPAIR + DIM + 2, NPAIR + DIM + 3
U_CODE, U_POSE = 1, 2
UNKNOWNS = {"code": U_CODE, "pose": U_POSE, "pose+code": U_CODE | U_POSE}
IU = np.triu_indices(DIM)                                  # the pairs i <= j, row-major
PI = np.concatenate([IU[0], np.arange(DIM)])               # sum q < IDX_COST is (ww J[PI[q]]) J[PJ[q]], column DIM of J being -d
PJ = np.concatenate([IU[1], np.full(DIM, DIM)])
DEFAULTS = dict(A.DEFAULTS, damp=1e-4, unknowns="code", code_reg=0.0, code_anchor=0.0, code_tol=1e-6)
assert NSUM == 2558


# ---- rows and sums ---------------------------------------------------------------------------------------------------------------------
def row_terms(pw, obj_row, dist, gw, gcode, w, huber, max_dist):
    """-> terms (n, NSUM) float64.  gw is read only where obj_row >= 0."""
    pw, gw, gcode = np.asarray(pw).reshape(-1, 3), np.asarray(gw).reshape(-1, 3), np.asarray(gcode).reshape(-1, CODE)
    n = pw.shape[0]
    obj_row, dist = np.asarray(obj_row, np.int32), np.asarray(dist)
    w32 = np.ones(n, F32) if w is None else np.asarray(w)
    gw = np.where((obj_row >= 0)[:, None], gw, gw.dtype.type(0))
    with np.errstate(all="ignore"):
        valid = np.isfinite(pw).all(1) & (w32 > 0) & np.isfinite(w32)
        used = valid & (obj_row >= 0) & np.isfinite(dist) & np.isfinite(gw).all(1) & np.isfinite(gcode).all(1) & (np.abs(dist.astype(F64)) <= max_dist)
        w64, d = w32.astype(F64), dist.astype(F64)
        a = np.abs(d)
        p, g = pw.astype(F64), gw.astype(F64)
        J = np.zeros((n, DIM + 1), F64)
        J[:, 0:3] = (-gw).astype(F64)
        J[:, 3] = -(p[:, 1] * g[:, 2] - p[:, 2] * g[:, 1])
        J[:, 4] = -(p[:, 2] * g[:, 0] - p[:, 0] * g[:, 2])
        J[:, 5] = -(p[:, 0] * g[:, 1] - p[:, 1] * g[:, 0])
        J[:, 6:DIM] = gcode.astype(F64)
        J[:, DIM] = -d
        wh = np.where(a <= huber, 1.0, huber / a)
        ww = w64 * wh
        J[~used] = 0.0
        ww[~used] = 0.0
        term = np.zeros((n, NSUM), F64)
        term[:, :IDX_COST] = (ww[:, None] * J[:, PI]) * J[:, PJ]
        term[:, IDX_COST] = np.where(used, w64 * A.rho(d, huber), np.where(valid, w64 * float(A.rho(max_dist, huber)), 0.0))
        term[:, IDX_W] = np.where(valid, w64, 0.0)
        term[:, IDX_N] = used.astype(F64)
    return term


def block_sums(terms):
    """The written order: blocks of BLOCK rows, every block from +0 one row at a time, the blocks ascending from the first."""
    terms = np.asarray(terms, F64).reshape(-1, NSUM)
    total = np.zeros(NSUM, F64)
    for b0 in range(0, terms.shape[0], BLOCK):
        blk = np.zeros(NSUM, F64)
        for r in range(b0, min(b0 + BLOCK, terms.shape[0])):
            blk = blk + terms[r]
        total = blk if b0 == 0 else total + blk
    return total


def rows(pw, winner, obj_row, d, gw, gcode, w, n_obj, huber, max_dist):
    """What dsp_debug_align_shapes_rows returns: (n_obj, NSUM); object k's rows are those with winner == k in ascending ray order."""
    winner = np.asarray(winner, np.int32)
    terms = row_terms(pw, obj_row, d, gw, gcode, w, huber, max_dist)
    return np.stack([block_sums(terms[winner == k]) for k in range(n_obj)]) if n_obj else np.zeros((0, NSUM), F64)


def full_h(sums):
    H = np.zeros((DIM, DIM), F64)
    H[IU] = sums[IDX_H:IDX_H + NPAIR]
    H[(IU[1], IU[0])] = sums[IDX_H:IDX_H + NPAIR]
    return H


# ---- cost and step ---------------------------------------------------------------------------------------------------------------------
def cost_of(sums, z, z0, code_len, code_reg, code_anchor, huber, max_dist):
    mean = float(A.rho(max_dist, huber)) if sums[IDX_W] == 0.0 else float(sums[IDX_COST] / sums[IDX_W])
    zz = dd = 0.0
    for c in range(code_len):
        zz = zz + float(z[c]) * float(z[c])
        e = float(z[c]) - float(z0[c])
        dd = dd + e * e
    return (mean + code_reg * zz) + code_anchor * dd


def pinned(i, unknowns, code_len):
    return not (unknowns & U_POSE) if i < 6 else (not (unknowns & U_CODE) or i - 6 >= code_len)


def solve(H, b, W, z, z0, code_len, unknowns, code_reg, code_anchor, damp, lam):
    """The step on the mean system in the header's order -> dx (70,) or None (SINGULAR)."""
    H = np.asarray(H, F64).reshape(DIM, DIM)
    W = float(W)
    if not (W > 0.0) or not math.isfinite(W):
        return None
    A_ = [[float(H[min(i, j), max(i, j)]) / W for j in range(DIM)] for i in range(DIM)]
    g = [float(b[i]) / W for i in range(DIM)]
    kc = float(code_reg) + float(code_anchor)
    for c in range(CODE):
        A_[6 + c][6 + c] = A_[6 + c][6 + c] + kc
        g[6 + c] = g[6 + c] - (code_reg * float(z[c]) + code_anchor * (float(z[c]) - float(z0[c])))
    dl = float(damp) + float(lam)
    for i in range(DIM):
        A_[i][i] = A_[i][i] + dl
    for i in range(DIM):
        if pinned(i, unknowns, code_len):
            for j in range(DIM):
                A_[i][j] = A_[j][i] = 0.0
            A_[i][i] = 1.0
            g[i] = 0.0
    Lm = [[0.0] * DIM for _ in range(DIM)]
    for j in range(DIM):
        s = A_[j][j]
        Lj = Lm[j]
        for k in range(j):
            s = s - Lj[k] * Lj[k]
        if not (s > 0.0) or not math.isfinite(s):
            return None
        Lj[j] = math.sqrt(s)
        for i in range(j + 1, DIM):
            q = A_[i][j]
            Li = Lm[i]
            for k in range(j):
                q = q - Li[k] * Lj[k]
            Li[j] = q / Lj[j]
    y, x = [0.0] * DIM, [0.0] * DIM
    for i in range(DIM):
        s = g[i]
        for k in range(i):
            s = s - Lm[i][k] * y[k]
        y[i] = s / Lm[i][i]
    for i in range(DIM - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, DIM):
            s = s - Lm[k][i] * x[k]
        x[i] = s / Lm[i][i]
    if not all(math.isfinite(v) for v in x):
        return None
    return np.array(x, F64)


def apply_step(dx, unknowns, code_len, C, z):
    """-> (C_trial (4, 4), z_trial (64,)) float64"""
    C = np.asarray(C, F64).reshape(4, 4)
    z = np.asarray(z, F64).reshape(CODE)
    Ct = A.apply_step(dx[:6], C) if unknowns & U_POSE else C.copy()
    zt = z.copy()
    for c in range(CODE):
        if not pinned(6 + c, unknowns, code_len):
            zt[c] = z[c] + dx[6 + c]
    return Ct, zt


def check_shapes(unknowns, code_reg, code_anchor, code_tol):
    """True: dsp_debug_align_shapes_check accepts the shapes params."""
    if unknowns == 0 or unknowns & ~3:
        return False
    return all(math.isfinite(v) and v >= 0 for v in (code_reg, code_anchor, code_tol))


# ---- one evaluation ----------------------------------------------------------------------------------------------------------------------
def cast(eng, poses32, codes32, ow, dirv, raycast=None, budget=None):
    """align_rays_ref.cast plus the winners' code derivatives times their scale (one float32 multiply): gcode (n, 64)."""
    ex = R.expected(eng, poses32, codes32, ow, dirv, raycast, budget=budget)
    g = ex["geometry"]
    n = ow.shape[0]
    gw, gcode = np.zeros((n, 3), F32), np.zeros((n, CODE), F32)
    for o in range(g["exists"].shape[0]):
        idx = np.flatnonzero(ex["obj"] == o)
        if idx.size:
            _, grad = eng.sdf_jacobian(codes32[o], R.sample(g["o_o"][o, idx], g["d_o"][o, idx], ex["t"][idx]))
            grad = np.asarray(grad, F32)
            s = np.full(idx.size, g["scale"][o], F32)
            gw[idx] = A.world_gradient(np.repeat(g["rt"][o:o + 1], idx.size, 0), s, grad[:, -3:])
            with np.errstate(all="ignore"):         # a 32-D decoder has 32 code derivatives: the rest of the row is zero
                gcode[idx, :grad.shape[1] - 3] = (grad[:, :-3] * s[:, None]).astype(F32)
    return dict(obj=ex["obj"], t=ex["t"], dist=ex["dist"], status=ex["status"], gw=gw, gcode=gcode, stats=ex["stats"])


def evaluate(poses32, codes32, pts_w, org_w, w, eng, huber, max_dist, max_gap, raycast=None, budget=None):
    """The pipeline's evaluation of the map at the float32 poses and codes: ONE cast of all rays, the rows per winner."""
    pw, ow = np.asarray(pts_w, F32).reshape(-1, 3), np.asarray(org_w, F32).reshape(-1, 3)
    codes32 = np.asarray(codes32, F32).reshape(-1, CODE)
    with np.errstate(all="ignore"):
        dirv = (pw - ow).astype(F32)
    c = cast(eng, np.asarray(poses32, F32).reshape(-1, 4, 4), codes32, ow, dirv, raycast, budget)
    obj_row, d = AR.residual(ow, pw, c["obj"], c["t"], c["dist"], c["status"], c["gw"], max_gap)
    sums = rows(pw, c["obj"], obj_row, d, c["gw"], c["gcode"], w, codes32.shape[0], huber, max_dist)
    return dict(sums=sums, winner=c["obj"], obj=obj_row, dist=d, t=c["t"], status=c["status"], gw=c["gw"], gcode=c["gcode"], stats=c["stats"])


def evaluator(eng, T0, pts_w, org_w, w, huber, max_dist, max_gap, raycast=None, budget=None):
    T0 = np.asarray(T0, F32).reshape(-1, 4, 4)

    def ev(C, z):
        with np.errstate(all="ignore"):
            return evaluate(AO.compose_all(C, T0), np.asarray(z, F64).astype(F32), pts_w, org_w, w, eng, huber, max_dist, max_gap, raycast, budget)
    return ev


def evaluate64(T, codes, decode, pts_w, org_w, w, huber, max_dist, max_gap, eps=1e-3, max_steps=64):
    """The evaluation with nothing rounded to float32.  decode(code, p_obj) -> (sdf (n,), gradient (n, 67): d / d code 64, d / d xyz 3)."""
    pw, ow = np.asarray(pts_w, F64).reshape(-1, 3), np.asarray(org_w, F64).reshape(-1, 3)
    T, codes = np.asarray(T, F64).reshape(-1, 4, 4), np.asarray(codes, F64).reshape(-1, CODE)
    dirv = pw - ow
    with np.errstate(all="ignore"):
        length = np.sqrt((dirv * dirv).sum(1))
        u = dirv / length[:, None]
    m = AO.Map64(T, codes)
    c = AR.cast64(m, lambda o, p: (lambda y, g: (y, g[:, -3:]))(*decode(codes[o], p)), ow, u, eps, max_steps)
    gcode = np.zeros((pw.shape[0], CODE), F64)
    for o in range(T.shape[0]):
        idx = np.flatnonzero(c["obj"] == o)
        if idx.size:
            inv = np.linalg.inv(T[o])
            hit = ow[idx] + c["t"][idx, None] * u[idx]
            _, g = decode(codes[o], hit @ inv[:3, :3].T + inv[:3, 3])
            gcode[idx] = g[:, :CODE] * m.s[o]
    with np.errstate(all="ignore"):
        gap = length - c["t"]
        d = c["dist"] + (c["gw"] * u).sum(1) * gap
        matched = (c["status"] == AR.HIT) & (c["obj"] >= 0) & np.isfinite(gap) & (np.abs(gap) <= max_gap)
    obj_row = np.where(matched, c["obj"], -1).astype(np.int32)
    d = np.where(c["obj"] >= 0, d, np.inf)
    sums = rows(pw, c["obj"], obj_row, d, c["gw"], gcode, None if w is None else np.asarray(w, F64), T.shape[0], huber, max_dist)
    return dict(sums=sums, winner=c["obj"], obj=obj_row, dist=d, t=c["t"], status=c["status"], gw=c["gw"], gcode=gcode)


def evaluator64(T0, decode, pts_w, org_w, w, huber, max_dist, max_gap, eps=1e-3, max_steps=64):
    T0 = np.asarray(T0, F64).reshape(-1, 4, 4)

    def ev(C, z):
        return evaluate64(np.asarray(C, F64).reshape(-1, 4, 4) @ T0, z, decode, pts_w, org_w, w, huber, max_dist, max_gap, eps, max_steps)
    return ev


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
def run(codes0, evaluate, refine=None, n_rays=1, code_len=CODE, finite=None, **params):
    """The loop of dsp_map_align_shapes: align_objects_ref.run's with the state (C_k, z_k) and the 70-dimensional step.  codes0 (n_obj, 64)
    float32: the input codes.  finite(k, z32) (optional) -> False when the code bias of the float32 trial code is not finite.  -> a list of
    dicts per object (correction, code (float64), status, evaluations, steps, cost0, cost, n_used, sums, lam, trace=[dict(pose, code,
    decision, cost, lam, n_used, sums, dx)])."""
    p = dict(DEFAULTS)
    p.update(params)
    sc = p["step_control"]
    step_on = sc is not None and any(v != 0 for v in sc)
    iters, huber, max_dist, min_points = p["iterations"], p["huber"], p["max_dist"], p["min_points"]
    unknowns = UNKNOWNS[p["unknowns"]] if isinstance(p["unknowns"], str) else int(p["unknowns"])
    reg, anchor = float(p["code_reg"]), float(p["code_anchor"])
    z0 = np.asarray(codes0, F32).reshape(-1, CODE).astype(F64)
    n_obj = z0.shape[0]

    def F_of(sums, z, k):
        return cost_of(sums, z, z0[k], code_len, reg, anchor, huber, max_dist)
    st = [dict(C_eval=np.eye(4), z_eval=z0[k].copy(), acc=None, lam=0.0, steps=0, status=A.OK, live=bool(refine is None or refine[k]),
               cost0=F_of(np.zeros(NSUM), z0[k], k), trace=[]) for k in range(n_obj)]
    if n_rays == 0:
        for s in st:
            if s["live"]:
                s["live"], s["status"] = False, A.NO_SUPPORT
    for e in range(iters):
        if not any(s["live"] for s in st):
            break
        # a trial state that cannot be evaluated ends its object with SINGULAR at its accepted state
        for k, s in enumerate(st):
            if s["live"] and s["acc"] is not None:
                with np.errstate(all="ignore"):
                    z32 = s["z_eval"].astype(F32)
                ok = bool(np.isfinite(z32).all()) and (finite is None or finite(k, z32))
                if not ok:
                    s["live"], s["status"] = False, A.SINGULAR
        C = np.stack([s["C_eval"] if s["live"] else (s["acc"]["pose"] if s["acc"] else np.eye(4)) for s in st])
        z = np.stack([s["z_eval"] if s["live"] else (s["acc"]["code"] if s["acc"] else z0[k]) for k, s in enumerate(st)])
        if not any(s["live"] for s in st):
            break
        ev = evaluate(C, z)
        for k, s in enumerate(st):
            if not s["live"]:
                continue
            sums = ev["sums"][k]
            F, n_used = F_of(sums, s["z_eval"], k), int(sums[IDX_N])
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
                s["acc"] = dict(pose=s["C_eval"], code=s["z_eval"], sums=sums, cost=F, n_used=n_used)
            rec = dict(pose=s["C_eval"], code=s["z_eval"], decision=dec, cost=F, lam=s["lam"], n_used=n_used, sums=sums, dx=None)
            s["trace"].append(rec)
            acc = s["acc"]
            if acc["n_used"] < min_points:
                s["live"], s["status"] = False, A.NO_SUPPORT
                continue
            H, b = full_h(acc["sums"]), acc["sums"][IDX_B:IDX_B + DIM]
            dx, tries = None, 0
            while True:
                dx = solve(H, b, acc["sums"][IDX_W], acc["code"], z0[k], code_len, unknowns, reg, anchor, p["damp"], s["lam"])
                if dx is not None or not step_on or tries >= 64 or not s["lam"] < sc[4]:
                    break
                s["lam"] = min(max(s["lam"], sc[3]) * sc[1], sc[4])
                tries += 1
            rec["lam"] = s["lam"]
            if dx is None:
                s["live"], s["status"] = False, A.SINGULAR
                continue
            rec["dx"] = dx
            if np.abs(dx[:3]).max() < p["trans_tol"] and np.abs(dx[3:6]).max() < p["rot_tol"] and np.abs(dx[6:]).max() < p["code_tol"]:
                s["live"], s["status"] = False, A.CONVERGED
                continue
            if e == iters - 1:
                s["live"], s["status"] = False, A.OK
                continue
            s["C_eval"], s["z_eval"] = apply_step(dx, unknowns, code_len, acc["pose"], acc["code"])
    out = []
    for k, s in enumerate(st):
        acc = s["acc"]
        out.append(dict(correction=acc["pose"] if acc else np.eye(4), code=acc["code"] if acc else z0[k], status=s["status"], evaluations=len(s["trace"]),
                        steps=s["steps"], cost0=s["cost0"], cost=acc["cost"] if acc else s["cost0"], n_used=acc["n_used"] if acc else 0,
                        sums=acc["sums"] if acc else np.zeros(NSUM), lam=s["lam"], trace=s["trace"]))
    return out


def run64(T0, codes0, decode, pts_w, org_w, w=None, refine=None, max_gap=0.6, eps=1e-3, max_steps=64, **params):
    """The float64 loop on its own.  -> run's list, each with `pose`: the float64 pose C_k T_k0."""
    p = dict(DEFAULTS)
    p.update(params)
    T0 = np.asarray(T0, F64).reshape(-1, 4, 4)
    ev = evaluator64(T0, decode, pts_w, org_w, w, p["huber"], p["max_dist"], max_gap, eps, max_steps)
    res = run(codes0, ev, refine, n_rays=np.asarray(pts_w).reshape(-1, 3).shape[0], **params)
    for r, t in zip(res, T0):
        r["pose"] = r["correction"] @ t
    return res
