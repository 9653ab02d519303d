"""The convergence rule of dsp_batch_convergence (include/dsp_gn.h) stated in numpy: what the solve step evaluates, in fp64, on the update
it has just applied.  Tests predict dsp_batch_iterations_used with it from a traced, unstopped run."""
import numpy as np


def n_used(dx, lr, pose_tol, code_tol, min_iterations=1, n_pose=7, pose_only=False):
    """dx: (n_iterations, n_unknowns) per-iteration solutions of ONE object that did not fail (pose entries first); lr: the learning rate
    (a pose-only batch applies dx itself: lr is ignored there, and so is code_tol).  Returns the number of updates applied: e + 1 for the
    first iteration e (0-based) with e + 1 >= min_iterations, max |lr dx_pose| < pose_tol and max |lr dx_code| < code_tol -- strict, so a
    tolerance of 0 stops nothing, inf switches its half off and a NaN step never passes -- or n_iterations if there is none."""
    dx = np.asarray(dx, np.float64)
    f = 1.0 if pose_only else float(np.float32(lr))
    for e in range(dx.shape[0]):
        step = np.abs(f * dx[e])
        ok = bool(np.all(step[:n_pose] < pose_tol))            # a comparison with NaN is False
        if not pose_only:
            ok = ok and bool(np.all(step[n_pose:] < code_tol))
        if ok and e + 1 >= min_iterations:
            return e + 1
    return dx.shape[0]
