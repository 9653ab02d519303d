"""The weighted fp64 linearisation the observation-weight tests compare with (tests/test_weights_host.py, tests/test_gpu_weights.py).
Test helper, not a test.

The objective with per-observation weights (include/dsp_gn.h, dsp_batch_observation_weights):
    E = k2 sum_p w_p (rho_b2 r_p)^2 / sum_p w_p  +  k1 sum_k w_ray(k) (rho_b1 r_k)^2 / sum_k w_ray(k)
so H gets sum w J^T J, b gets -sum w J^T r~, and the divisors are the sums of the weights, pooled over an object's views.

The rows are oracle.dsp_oracle._view_rows64's, untouched: per-row jacobians (and their ReLU-kink twins), robust residuals, and
sets["kept"][0] for the ray of each render row.  A row of weight w among n pooled rows whose weights sum to S is scaled by
sqrt(w n / S) and the scaled rows go through the oracle's own _assemble64, whose J^T J / n, J^T r / n and mean(r^2) are then the weighted
sums over S, kink allowances included; priors and damping are its own, once.  With unit weights every factor is sqrt(n / n) = 1 exactly:
linearise_fp64 / linearise_fp64_multiview bit for bit.  Rows of weight 0 stay as zero rows: N and K stay counts.
"""
import numpy as np

from oracle import dsp_oracle as O

F64 = np.float64


def row_weights(sets, pt_w, ray_w, n_pts):
    """(w_s (N,), w_r (K,)) of one view: its point weights, and for each render row the weight of the row's ray.  None = ones."""
    w_s = np.ones(n_pts, F64) if pt_w is None else np.asarray(pt_w, np.float32).astype(F64).reshape(-1)
    gx = np.zeros(0, np.int64) if sets is None else np.asarray(sets["kept"][0], np.int64).reshape(-1)
    w_r = np.ones(gx.shape[0], F64) if ray_w is None else np.asarray(ray_w, np.float32).astype(F64).reshape(-1)[gx]
    assert w_s.shape[0] == n_pts
    return w_s, w_r


def _scaled(rows, weights):
    """The views' rows scaled for _assemble64; -> (rows, (sum w_s, sum w_r))."""
    n_s, n_k = sum(r["j_s"].shape[0] for r in rows), sum(r["j_r"].shape[0] for r in rows)
    s_s = float(sum(float(np.sum(w[0])) for w in weights))
    s_k = float(sum(float(np.sum(w[1])) for w in weights))
    out = []
    for r, (w_s, w_r) in zip(rows, weights):
        assert w_s.shape[0] == r["j_s"].shape[0] and w_r.shape[0] == r["j_r"].shape[0]
        f_s = np.sqrt(w_s * n_s / s_s) if s_s > 0 else np.zeros_like(w_s)
        f_r = np.sqrt(w_r * n_k / s_k) if s_k > 0 else np.zeros_like(w_r)
        out.append(dict(r, j_s=r["j_s"] * f_s[:, None], j_s2=r["j_s2"] * f_s[:, None], r_s=r["r_s"] * f_s,
                        j_r=r["j_r"] * f_r[:, None], j_r2=r["j_r2"] * f_r[:, None], r_r=r["r_r"] * f_r))
    return out, (s_s, s_k)


def assemble(prm, rows, weights, t_obj_cam, code):
    """rows: [_view_rows64 dict per view]; weights: [(w_s, w_r) per view] (row_weights).  -> the keys tests/gn_metric.scaled_errors reads
    (H, b, dx, Dr, Ds, gr, gs, Lr, Ls, the prior and damping terms, H_flip / b_flip), plus Mw / Kw = the weight sums."""
    scaled, (s_s, s_k) = _scaled(rows, weights)
    lin = O._assemble64(prm, scaled, t_obj_cam, code)
    lin.update(Mw=s_s, Kw=s_k)
    return lin


def linearise(dec, prm, pts, rays, depth, t_obj_cam, code, depths, sets, pt_w=None, ray_w=None):
    """linearise_fp64 with weights (one view)."""
    rows = O._view_rows64(dec, prm, pts, rays, depth, t_obj_cam, code, depths, sets)
    return assemble(prm, [rows], [row_weights(sets, pt_w, ray_w, rows["N"])], t_obj_cam, code)


def linearise_multiview(dec, prm, views, t_obj_cam, code, depths_per_view, sets_per_view, pt_w=None, ray_w=None):
    """linearise_fp64_multiview with weights: pt_w / ray_w = one array (or None) per view, or None for all."""
    rows = []
    lin0 = O.linearise_fp64_multiview(dec, prm, views, t_obj_cam, code, depths_per_view, sets_per_view, rows_out=rows)
    pw = [None] * len(views) if pt_w is None else pt_w
    rw = [None] * len(views) if ray_w is None else ray_w
    weights = [row_weights(s, p, r, row["N"]) for s, p, r, row in zip(sets_per_view, pw, rw, rows)]
    lin = assemble(prm, rows, weights, t_obj_cam, code)
    lin.update(V_views=lin0["V_views"], K_views=lin0["K_views"], N_views=lin0["N_views"])
    return lin


def brute_force(prm, rows, weights, code):
    """The data terms as plain numpy sums, row by row: (Ds, gs, Ls, Dr, gr, Lr) -- what assemble() must agree with."""
    k1, k2 = float(np.float32(prm.k1)), float(np.float32(prm.k2))
    out = []
    for (jk, rk, wi, k) in (("j_s", "r_s", 0, k2), ("j_r", "r_r", 1, k1)):
        n = rows[0][jk].shape[1]
        h, g, l, s = np.zeros((n, n)), np.zeros(n), 0.0, 0.0
        for r, w in zip(rows, weights):
            for j, res, wt in zip(r[jk], r[rk], w[wi]):
                h += wt * np.outer(j, j)
                g += wt * j * res
                l += wt * res * res
                s += wt
        out += [k * h / s, -k * g / s, k * l / s]
    return tuple(out)


def device_sets(mask, deds):
    """The sets a device iteration used, from Batch.debug_samples' in-sphere mask and de_ds grid (de_ds != 0 marks a kept sample), in the
    reference's row order (ray-major, depth-minor): what linearise() takes as `sets`."""
    mask = np.asarray(mask, bool)
    kept = mask & np.isfinite(deds) & (np.asarray(deds) != 0)
    return dict(valid=np.nonzero(mask), kept=np.nonzero(kept))


def pose_only(dec, pts, t_obj_cam, code, pt_w=None, alive=None):
    """The weighted pose-only system (optimizer.py:62-72 with weights) in float64, embedded in the 71-unknown layout tests/gn_metric reads:
    H[:6, :6] = sum w J6^T J6 / sum w + 1e-2 I, b[:6] = -sum w J6^T r / sum w over the alive points, r the RAW residual; the identity and
    zeros elsewhere.  Ds / gs / Ls carry the data terms (k2 = 1), the render and prior terms are zero."""
    prm = O.GNParams(num_iterations=1, b2=1e30, num_depth_samples=2)          # b2 beyond every residual: the robust residual is the raw one
    rows = O._view_rows64(dec, prm, pts, np.zeros((0, 3), np.float32), np.zeros(0, np.float32), t_obj_cam, code, np.array([1.0, 2.0], np.float32), O.NO_SETS)
    w = np.ones(rows["N"], F64) if pt_w is None else np.asarray(pt_w, np.float32).astype(F64)
    if alive is not None:
        w = w * np.asarray(alive, bool)
    s = float(w.sum())
    n = 71
    j, j2, r = rows["j_s"][:, :6], rows["j_s2"][:, :6], rows["r_s"]
    ds, gs = np.zeros((n, n)), np.zeros(n)
    ds[:6, :6] = (j * w[:, None]).T @ j / s
    gs[:6] = -(j * w[:, None]).T @ r / s
    fh, fb = np.zeros((n, n)), np.zeros(n)
    for k in np.where(np.any(j2 != j, axis=1))[0]:
        fh[:6, :6] += w[k] / s * np.abs(np.outer(j2[k], j2[k]) - np.outer(j[k], j[k]))
        fb[:6] += w[k] / s * np.abs((j2[k] - j[k]) * r[k])
    h = ds + np.eye(n)
    h[:6, :6] = ds[:6, :6] + 1e-2 * np.eye(6)
    z = np.zeros(n)
    return dict(H=h, b=gs.copy(), dx=np.linalg.solve(h, gs), Dr=np.zeros((n, n)), Ds=ds, gr=z.copy(), gs=gs, Lr=0.0, Ls=float(np.sum(w * r * r) / s),
                b_code_prior=z.copy(), b_rot=z.copy(), j_rot=np.zeros(7), H_flip=fh, b_flip=fb, Mw=s, N=int(rows["N"]))


def embed6(tr_h, tr_b, tr_dx):
    """A pose-only trace row (6 x 6) in pose_only()'s 71-unknown layout."""
    n = 71
    h, b, dx = np.eye(n, dtype=np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    h[:6, :6], b[:6], dx[:6] = tr_h, tr_b, tr_dx
    return dict(H=h, b=b, dx=dx)
