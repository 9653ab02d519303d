"""The conditioned fp64 system the mask-of-unknowns tests compare with (tests/test_unknowns_host.py, tests/test_gpu_unknowns.py).
Test helper, not a test.

dsp_batch_unknowns (include/dsp_gn.h) freezes entries of [v(3), w(3), sigma | code(64)]: a frozen index i is not an unknown, the system is
conditioned on its current value.  In the solve step's layout that is row and column i of H set to zero, H_ii = 1 and b_i = 0, behind
everything else H and b are made of; dx is the solve of the live block and exactly 0 elsewhere.

`condition` takes the dict oracle.dsp_oracle.linearise_fp64 returns (or linearise_fp64_multiview's, weights_ref.assemble's,
weights_ref.pose_only's) and a mask, and returns the same keys for tests/gn_metric.scaled_errors.  At frozen entries the data Grams, the data
and prior parts of b, the rotation prior's jacobian and the ReLU-kink twins are zeroed, so that every scale and every allowance of the
metric vanishes there: a frozen entry of the device's system has to be the pinned value itself, and a frozen dx exactly zero.

`posterior` is the conditioned posterior record: tests/posterior_ref.py's functions on the live block, padded back with zeros.
"""
import numpy as np

import posterior_ref as R

MATRICES = ("Dr", "Ds", "H_flip", "H_code_prior", "H_rot", "H_damp")
VECTORS = ("gr", "gs", "b_flip", "b_code_prior", "b_rot")


def _live(live, n):
    live = np.asarray(live).reshape(-1)
    assert live.shape[0] >= n and np.all((live == 0) | (live == 1)), "a mask is 0 / 1 per unknown"
    return live[:n].astype(bool)          # (a 32-D decoder's system has 39 unknowns: the mask's slots beyond them are not looked at)


def pin(h, b, live):
    """[H | b] with the frozen rows and columns pinned: zeros, H_ii = 1, b_i = 0."""
    h, b = np.array(h, np.float64, copy=True), np.array(b, np.float64, copy=True)
    fz = ~_live(live, h.shape[0])
    h[fz, :] = 0.0
    h[:, fz] = 0.0
    h[fz, fz] = 1.0
    b[fz] = 0.0
    return h, b


def condition(lin, live):
    """The linearisation `lin` conditioned on the frozen entries of `live` (1 = live).  An all-live mask returns lin's own values."""
    n = lin["H"].shape[0]
    lv = _live(live, n)
    out = dict(lin)
    if lv.all():
        return out
    fz = ~lv
    out["H"], out["b"] = pin(lin["H"], lin["b"], lv)
    dx = np.zeros(n)
    if lv.any():
        dx[lv] = np.linalg.solve(out["H"][np.ix_(lv, lv)], out["b"][lv])
    out["dx"] = dx
    for k in MATRICES:
        if k in lin:
            m = np.array(lin[k], np.float64, copy=True)
            m[fz, :] = 0.0
            m[:, fz] = 0.0
            out[k] = m
    for k in VECTORS:
        if k in lin:
            v = np.array(lin[k], np.float64, copy=True)
            v[fz] = 0.0
            out[k] = v
    if "j_rot" in lin:
        j = np.array(lin["j_rot"], np.float64, copy=True)
        j[fz[:j.shape[0]]] = 0.0
        out["j_rot"] = j
    return out


def condition_lambda(lam, g, live):
    """Lambda and g of a level-2 posterior record, conditioned: zeros in frozen rows and columns (no pin: Lambda carries no damping)."""
    lam, g = np.array(lam, np.float64, copy=True), np.array(g, np.float64, copy=True)
    fz = ~_live(live, lam.shape[0])
    lam[fz, :] = 0.0
    lam[:, fz] = 0.0
    g[fz] = 0.0
    return lam, g


def posterior(lam, live, n_pose=7, refined=False):
    """The conditioned posterior of the information matrix `lam` (n x n, n = n_pose + code entries; frozen rows and columns are ignored):
    info_pose = the Schur complement over the live code entries on the live pose entries, cov_pose its inverse on that sub-block, var_code
    the live diagonal of the inverse's code block; zeros at frozen entries.  refined=False: posterior_ref.sweep, the device's elimination
    restated; True: posterior_ref.refined_inverse (long double) and its marginals.  -> dict(status, info_pose, cov_pose, var_code)."""
    lam = np.asarray(lam, np.float64)
    n = lam.shape[0]
    lv = _live(live, n)
    idx = np.nonzero(lv)[0]
    p_idx = np.nonzero(lv[:n_pose])[0]
    c_idx = np.nonzero(lv[n_pose:])[0]
    info, cov, var = np.zeros((n_pose, n_pose)), np.zeros((n_pose, n_pose)), np.zeros(n - n_pose)
    status = 0
    if idx.size:
        blk = lam[np.ix_(idx, idx)]
        if refined:
            inv = R.refined_inverse(blk)
            p = p_idx.size
            rec = dict(status=0, cov_pose=np.asarray(inv[:p, :p], np.float64), var_code=np.asarray(np.diag(inv)[p:], np.float64),
                       info_pose=np.asarray(R.marginals(inv, p)[2], np.float64) if p else np.zeros((0, 0)))
        else:
            rec = R.sweep(blk, p_idx.size)
        status = rec["status"]
        if p_idx.size:
            info[np.ix_(p_idx, p_idx)] = rec["info_pose"]
            cov[np.ix_(p_idx, p_idx)] = rec["cov_pose"]
        var[c_idx] = rec["var_code"]
    return dict(status=status, info_pose=info, cov_pose=cov, var_code=var)
