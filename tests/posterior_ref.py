"""numpy references for the posterior records (dsp_batch_posterior, include/dsp_gn.h) -- test infrastructure.

* `with_damping`: Lambda plus what the solve step adds on top of it (k_solve: `+ 1` on the pose diagonal, `+ s_damp` on sigma, the identity pin of
  code slots beyond the decoder's code length; pose-only: `+ 1e-2`), added in float64 in the solve step's order, so that float32(result) can be
  compared with a trace's H bit for bit.
* `refined_inverse`: numpy.linalg.inv in float64 followed by two Newton-Schulz steps X += X (I - A X) in numpy.longdouble -- the reference the
  device's pivot-free elimination is judged against -- and `marginals` of an inverse.
* `sweep`: the device kernel's elimination restated (k_posterior: symmetric sweep operator, code block first, lower triangle mirrored, one
  multiply-subtract per entry and step).  numpy has no fused multiply-add, so each step's product is rounded once more than on the device: the
  restatement is the kernel's algorithm and schedule, to a few ulp of its bits.  cov_pose then gets the kernel's one refinement step against
  Lambda (residual in long double here, double-double there).
* `pivot_ratios`: smallest pivot / original diagonal entry of pivot-free elimination, in both orders (the singularity rule's quantity).
"""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
SINGULAR_RATIO = 16.0 * FLT_EPSILON


def with_damping(lam, s_damp=0.0, code_len=64, pose_only=False):
    lam = np.array(lam, np.float64, copy=True)
    if pose_only:
        lam[np.arange(6), np.arange(6)] += 1e-2
        return lam
    n = 7 + code_len
    for i in range(n, lam.shape[0]):
        lam[i, i] = 1.0
    for i in range(7):
        lam[i, i] += 1.0
    lam[6, 6] += float(np.float32(s_damp))
    return lam


def refined_inverse(a):
    a = np.asarray(a, np.float64)
    al = a.astype(np.longdouble)
    x = np.linalg.inv(a).astype(np.longdouble)
    eye = np.eye(a.shape[0], dtype=np.longdouble)
    for _ in range(2):
        x = x + x @ (eye - al @ x)
    return x


def marginals(inv, n_pose):
    """(cov_pose, var_code, info_pose) of an inverse (any float type); info_pose = inverse of the pose block of the inverse."""
    inv = np.asarray(inv)
    cov = inv[:n_pose, :n_pose]
    var = np.diag(inv)[n_pose:].copy()
    if inv.dtype == np.longdouble:
        info = refined_inverse(np.asarray(cov, np.float64))
        eye = np.eye(n_pose, dtype=np.longdouble)
        for _ in range(2):
            info = info + info @ (eye - cov @ info)
    else:
        info = np.linalg.inv(cov)
    return cov, var, info


def rel_err(got, ref):
    ref = np.asarray(ref, np.longdouble)
    return float(np.abs(np.asarray(got, np.longdouble) - ref).max() / np.abs(ref).max())


def sweep(lam, n_pose):
    """k_posterior's elimination on the live block `lam` (n x n): -> dict(status 0 / 2, info_pose, cov_pose, var_code)."""
    a = np.array(lam, np.float64, copy=True)
    n = a.shape[0]
    d0 = np.diag(a).copy()
    order = list(range(n_pose, n)) + list(range(n_pose))
    info = a[:n_pose, :n_pose].copy()
    il, jl = np.tril_indices(n)
    for t, k in enumerate(order):
        if t == n - n_pose:
            info = a[:n_pose, :n_pose].copy()
        c = a[:, k].copy()
        d = c[k]
        if not d > SINGULAR_RATIO * d0[k]:
            return dict(status=2, info_pose=info if n == n_pose else np.zeros_like(info), cov_pose=np.zeros((n_pose, n_pose)), var_code=np.zeros(n - n_pose))
        rd = 1.0 / d
        l = c * rd
        new = a[il, jl] - l[il] * c[jl]
        new = np.where(jl == k, l[il], new)
        new = np.where(il == k, l[jl], new)
        new = np.where((il == k) & (jl == k), -rd, new)
        a[il, jl] = new
        a[jl, il] = new
    # cov_pose: one Newton-Schulz step of the pose columns against lam itself, the residual in extended precision (the device: double-double)
    x = -a
    lam_l = np.array(lam, np.float64).astype(np.longdouble)
    res = (np.eye(n, dtype=np.longdouble)[:, :n_pose] - lam_l @ x[:, :n_pose].astype(np.longdouble)).astype(np.float64)
    cov = x[:n_pose, :n_pose] + x[:n_pose, :] @ res
    cov = np.tril(cov) + np.tril(cov, -1).T
    return dict(status=0, info_pose=info, cov_pose=cov, var_code=-np.diag(a)[n_pose:].copy())


def pivot_ratios(a, n_pose):
    """min over pivots of pivot / original diagonal entry for pivot-free elimination, pose block first and code block first."""
    a = np.asarray(a, np.float64)
    n = a.shape[0]
    out = []
    for order in (list(range(n)), list(range(n_pose, n)) + list(range(n_pose))):
        p = a[np.ix_(order, order)].copy()
        d0 = np.diag(p).copy()
        worst = np.inf
        for k in range(n):
            d = p[k, k]
            worst = min(worst, d / d0[k])
            if not d > 0:
                break
            p[k + 1:, k + 1:] -= np.outer(p[k + 1:, k], p[k, k + 1:]) / d
        out.append(float(worst))
    return tuple(out)


def marginalise_sigma(s7):
    s7 = np.asarray(s7, np.float64)
    return s7[:6, :6] - np.outer(s7[:6, 6], s7[6, :6]) / s7[6, 6]


def edge_information(info_pose, scale, gain=1.0):
    """The numpy statement of dsp_pg_edge_information: [omega | upsilon] = [w, s v]."""
    s = np.asarray(info_pose, np.float64)
    s6 = marginalise_sigma(s) if s.shape[0] == 7 else s
    perm = [3, 4, 5, 0, 1, 2]
    d = np.array([1, 1, 1, 1 / scale, 1 / scale, 1 / scale], np.float64)
    return gain * (s6[np.ix_(perm, perm)] * d[:, None] * d[None, :])
