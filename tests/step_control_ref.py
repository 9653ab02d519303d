"""Levenberg-Marquardt step control (dsp_batch_step_control, dsp_slam_amd/csrc/step_rule.h) restated for the tests.

rule(): the accept / reject rule in numpy, on a cost sequence.
run():  the rule composed from UNMODIFIED oracle pieces -- one oracle.dsp_oracle.reconstruct_object(num_iterations=1, t_obj_cam0=x, code=z)
        call per linearisation, an fp64 solve of (S + lambda I) dx = b with S the accepted state's float32 system, and the oracle's
        exp_sim3 for the update.  The last iteration evaluates and decides but applies no step, so the returned state is the best
        evaluated state and the returned loss is the loss at it.
"""
import copy

import numpy as np

NOT_EVALUATED, ACCEPTED, REJECTED = 0, 1, 2
F32 = np.float32


def decide(first, cost, f_acc, lam, lambda0, up, down, lambda_min, lambda_max):
    """-> (decision, lambda after it)."""
    if first:
        return ACCEPTED, float(lambda0)
    if cost < f_acc:                   # strict, and false for NaN
        return ACCEPTED, lam * down
    return REJECTED, min(max(lam, lambda_min) * up, lambda_max)


def rule(cost, lambda0=0.0, up=10.0, down=0.1, lambda_min=1.0, lambda_max=float("inf")):
    """The rule applied to a cost sequence -> (decision int32 (n,), lambda float64 (n,) = the value after each decision)."""
    cost = np.asarray(cost, np.float64).reshape(-1)
    dec, lams = np.zeros(cost.shape[0], np.int32), np.zeros(cost.shape[0])
    lam, f_acc = 0.0, 0.0
    for e, c in enumerate(cost):
        dec[e], lam = decide(e == 0, float(c), f_acc, lam, lambda0, up, down, lambda_min, lambda_max)
        if dec[e] == ACCEPTED:
            f_acc = float(c)
        lams[e] = lam
    return dec, lams


def run(dec, prm, obj, num_iterations, lambda0=0.0, up=10.0, down=0.1, lambda_min=1.0, lambda_max=float("inf")):
    """The composed oracle loop on one synth object -> dict(is_good, loss, t_obj_cam, code, decision, cost, lam, step_pose, step_code)."""
    from oracle import dsp_oracle as O
    one = copy.copy(prm)
    one.num_iterations = 1
    n = 7 + prm.code_len
    x = O._inv(np.asarray(obj["t_cam_obj_init"], F32))
    z = np.zeros(prm.code_len, F32)
    x_acc = z_acc = h_acc = b_acc = None
    f_acc, loss_acc, lam = 0.0, float("nan"), 0.0
    decision, cost, lams, step_pose, step_code = [], [], [], [], []
    for e in range(num_iterations):
        tr = []
        r = O.reconstruct_object(dec, one, obj["t_cam_obj_init"], obj["pts"], obj["rays"], obj["depth"], code=z, trace=tr, t_obj_cam0=x)
        if not r["is_good"] or not tr:         # a failing trial fails the object, as in a run without step control
            return dict(is_good=False, loss=r["loss"], t_obj_cam=None, code=None, decision=decision, cost=cost, lam=lams,
                        step_pose=step_pose, step_code=step_code)
        f_e = float(F32(tr[0]["loss"]))
        d, lam = decide(e == 0, f_e, f_acc, lam, lambda0, up, down, lambda_min, lambda_max)
        decision.append(d), cost.append(f_e), lams.append(lam)
        if d == ACCEPTED:
            x_acc, z_acc, f_acc, loss_acc = x.copy(), z.copy(), f_e, tr[0]["loss"]
            h_acc, b_acc = tr[0]["H"].astype(np.float64), tr[0]["b"].astype(np.float64)
        if e + 1 == num_iterations:
            break
        dx = np.linalg.solve(h_acc + lam * np.eye(n), b_acc)
        lr = float(F32(prm.lr))
        step_pose.append(float(np.abs(lr * dx[:7]).max())), step_code.append(float(np.abs(lr * dx[7:]).max()))
        x = (O.exp_sim3(F32(prm.lr) * dx[:7].astype(F32)) @ x_acc).astype(F32)
        z = (z_acc + F32(prm.lr) * dx[7:].astype(F32)).astype(F32)
    return dict(is_good=True, loss=loss_acc, t_obj_cam=x_acc, code=z_acc, decision=decision, cost=cost, lam=lams, step_pose=step_pose,
                step_code=step_code)
