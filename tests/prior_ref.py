"""fp64 numpy restatement of the Gaussian prior on pose and code (include/dsp_gn.h: dsp_batch_prior), built from the definitions alone:
the exponential is a matrix Taylor series (scaling and squaring), V -- the matrix that multiplies v in the Sim(3) exponential -- is read off
that series, and the jacobian is the BCH series as the header states it.  No closed form of the library is repeated here, and the oracle is
not used."""
import numpy as np

HALF_TURN_MARGIN = 1e-3


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def hat(xi):
    """[v, w, sigma] (7) or [v, w] (6, sigma = 0) -> the 4 x 4 generator [[w^ + sigma I, v], [0, 0]]."""
    xi = np.asarray(xi, np.float64)
    m = np.zeros((4, 4))
    m[:3, :3] = skew(xi[3:6]) + (xi[6] if xi.shape[0] == 7 else 0.0) * np.eye(3)
    m[:3, 3] = xi[:3]
    return m


def expm_taylor(a):
    """exp(a) by scaling and squaring around a 24-term Taylor series (|a| / 2^s <= 1/4: the truncation is below 1e-30)."""
    a = np.asarray(a, np.float64)
    norm = np.abs(a).sum(1).max()
    s = 0 if norm <= 0.25 else int(np.ceil(np.log2(norm / 0.25)))
    x = a / (2.0 ** s)
    out, term = np.eye(a.shape[0]), np.eye(a.shape[0])
    for k in range(1, 25):
        term = term @ x / k
        out = out + term
    for _ in range(s):
        out = out @ out
    return out


def Exp(xi):
    return expm_taylor(hat(xi))


def v_matrix(w, sigma):
    """V = int_0^1 exp(a (sigma I + w^)) da: column i is the translation of Exp([e_i, w, sigma])."""
    return np.stack([Exp(np.concatenate([np.eye(3)[i], w, [sigma]]))[:3, 3] for i in range(3)], 1)


def Log(t):
    """The logarithm of the standard Sim(3) exponential of the affine map t (bottom row taken as [0 0 0 1]) -> [v, w, sigma], or None when
    det <= 0 or the rotation angle exceeds pi - 1e-3."""
    t = np.asarray(t, np.float64)
    m = t[:3, :3]
    det = np.linalg.det(m)
    if not det > 0:
        return None
    s = np.cbrt(det)
    sigma = np.log(s)
    r = m / s
    a = 0.5 * np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    sn, cs = np.linalg.norm(a), 0.5 * (np.trace(r) - 1.0)
    th = np.arctan2(sn, cs)
    if not th <= np.pi - HALF_TURN_MARGIN:
        return None
    k = 1.0 + th * th / 6.0 + 7.0 * th ** 4 / 360.0 if th < 1e-4 else th / sn
    w = k * a
    v = np.linalg.solve(v_matrix(w, sigma), t[:3, 3])
    return np.concatenate([v, w, [sigma]])


def affine_inverse(t):
    t = np.asarray(t, np.float64)
    out = np.eye(4)
    out[:3, :3] = np.linalg.inv(t[:3, :3])
    out[:3, 3] = -out[:3, :3] @ t[:3, 3]
    return out


def ad(e):
    """ad([v, w, sigma]) = [[w^ + sigma I, v^, -v], [0, w^, 0], [0, 0, 0]] (7 x 7)."""
    v, w, s = e[:3], e[3:6], e[6]
    m = np.zeros((7, 7))
    m[:3, :3] = skew(w) + s * np.eye(3)
    m[:3, 3:6] = skew(v)
    m[:3, 6] = -v
    m[3:6, 3:6] = skew(w)
    return m


def jac_pose(e, P=7):
    """J_p = I - 1/2 ad(e) + 1/12 ad(e)^2; P = 6: the top-left 6 x 6 with sigma = 0."""
    e7 = np.concatenate([e[:6], [e[6] if P == 7 else 0.0]])
    a = ad(e7)
    return (np.eye(7) - 0.5 * a + a @ a / 12.0)[:P, :P]


def pose_residual(t_oc, t0, P=7):
    """e_p = Log(T_oc T0^-1) in fp64 from the two (float32) matrices, both read as affine maps; P = 6 drops sigma.  None: half a turn."""
    toc = np.array(np.asarray(t_oc, np.float64).reshape(4, 4))
    toc[3] = [0, 0, 0, 1]
    e = Log(toc @ affine_inverse(np.asarray(t0, np.float64).reshape(4, 4)))
    return None if e is None else e[:P]


def terms(t_oc, z, t0, z0, lam, pose_only=False, code_len=64):
    """-> dict(e (P + 64; pose-only: 6), J (n x n), H = J^T Lp J, b = -J^T Lp e, chi2), n = 71 or 6; None: the object ends DSP_OBJ_NAN.
    Rows and columns beyond P + code_len are zero in H and b."""
    P, n = (6, 6) if pose_only else (7, 71)
    lam = np.asarray(lam, np.float64).reshape(n, n)
    ep = pose_residual(t_oc, t0, P)
    if ep is None:
        return None
    e = ep if pose_only else np.concatenate([ep, np.asarray(z, np.float64).reshape(-1)[:64] - np.asarray(z0, np.float64).reshape(-1)[:64]])
    J = np.eye(n)
    J[:P, :P] = jac_pose(np.concatenate([ep, [0.0]])[:7], P)
    H = J.T @ lam @ J
    b = -J.T @ lam @ e
    live = n if pose_only else 7 + code_len
    H[live:, :] = 0.0
    H[:, live:] = 0.0
    b[live:] = 0.0
    return dict(e=e, J=J, H=H, b=b, chi2=float(e @ lam @ e))
