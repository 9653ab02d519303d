"""Entry-by-entry comparison of a Gauss-Newton system (H, b, dx) with the fp64 linearisation (oracle.dsp_oracle.linearise_fp64).

Why not the max-norm.  The older checks bound |dH| by 1e-4 max|H|.  The pose block of H reaches 150-2700 on the recorded runs while the
code block is 0.7-34, and the data part of a code entry is often far smaller than the k3 prior on its diagonal: 1e-4 max|H| is an absolute
tolerance of 0.01-0.3, under which a 10 % error in eight code-gradient columns passes.  b is worse: its code entries are 1e-7..1e-3 of max|b|.

The metric.  D = Dr + Ds is the data Gram (k1 J_r^T J_r / K + k2 J_s^T J_s / N, no prior, no damping).  By Cauchy-Schwarz every data
entry satisfies |D_ij| <= sqrt(D_ii D_jj), and round-off in the sums that form it is of that size times the unit round-off, whatever
cancellation happens inside the sum.  So an implementation's error in H_ij is scaled by

    SH_ij = sqrt(D_ii D_jj)

and its error in b_i (a cancelling sum sum_n J_ni r_n near convergence) by

    s_i = sqrt(Dr_ii Lr) + sqrt(Ds_ii Ls) + |k3 prior_i| + |k4 rotation prior_i|      (Lr = k1 render_loss, Ls = k2 sdf_loss)

H is compared as   |dH_ij| <= TAU_H SH_ij + 4 ulp32(|H_ij|) + A_rot_ij + A_flip_ij + 2 |dH_ij(jitter)|,
b as               |db_i|  <= TAU_B s_i   + 4 ulp32(|b_i|)  + a_rot_i  + a_flip_i  + 2 |db_i(jitter)|,
dx by residual     |H64 (dx - dx64)|_i <= TAU_B s_i + sum_j (TAU_H SH_ij + 4 ulp32(|H_ij|) + A_rot_ij + A_flip_ij) |dx_j| + 4 ulp32(|b_i|)
                                          + a_rot_i + a_flip_i + 2 |H64 (dx(jitter) - dx(oracle))|_i,
so that ill-conditioning of H does not loosen the dx check.  The 4 ulp32 terms let the prior and damping entries (which sit on top of the
data part, k3 on the code diagonal) be compared at a few ulp of the stored float32: they are added into H64 exactly.  A_rot / a_rot are the
rotation prior's own quantisation: k4 J_rot J_rot^T and k4 J_rot (1 + R_co[1,1]) with k4 = 1e7 and J_rot, res_rot formed from O(1) fp32
numbers (absolute error ~2.4e-7, test_oracle_golden's allowance):  A_rot_ij = k4 2.4e-7 (|J_i| + |J_j|),  a_rot_i = k4 2.4e-7 (|J_i| + 1e-3)
on the entries 3:6.  The jitter terms are the existing sdf-round-off allowance (the fp32 oracle re-run with decoded values moved by
+-2e-7, see tests/test_gpu_parity.py), applied entry by entry; they are used only where the caller has that twin.

A_flip / a_flip are the decoder's ReLU kinks.  A surface or render row whose hidden pre-activation lies within fp32 round-off of zero
(oracle.dsp_oracle.RELU_ULPS: the dot product's own round-off plus the rounding of the transformed point carried by d a / d xyz) may take
either side of that ReLU in an fp32 implementation, and its jacobian jumps there -- by 14 % in a surface row of the fp32 oracle's own
`small` run (iteration 2), which alone puts that state's pose block 1.3e-2 from fp64.  linearise_fp64 computes each such row's jacobian
with those masks flipped; A_flip / a_flip are the entrywise changes of H and b that would make, summed over those rows, the same for
every implementation compared.  The sdf jitter cannot stand in for this: it moves decoded values, not the masks of the backward pass.

A scaled error is  max(0, |error| - the allowances other than TAU) / scale;  a system passes when every block's scaled error is <= TAU,
and its own solve residual (solve_residual) is <= TAU_SOLVE.

Choice of TAU.  Measured on the CPU with tools/measure_gn_metric.py --measure: the fp32 oracle (linearising at each recorded state on the
recorded depth samples) and the reference's own recorded system, each against fp64 on the same sets, all allowances above except the
jitter; the worst over every iteration of each recorded run (n = iterations; solve = the system's own solve residual, `solve_residual`):

    run       n  who      H pose  H scale H pose*code H code  b pose  b code  dx      solve
    small    10  oracle   8.7e-06 5.4e-06 9.4e-06    7.5e-06 5.6e-07 5.3e-07 0       2.1e-05
                 ref      9.6e-06 6.1e-06 1.0e-05    8.5e-06 3.9e-07 7.1e-07 0       8.0e-05
    cfg1      5  oracle   7.2e-07 1.0e-07 9.3e-07    8.8e-07 0       0       0       9.1e-06
                 ref      1.0e-06 0       5.3e-07    5.5e-07 0       0       0       1.3e-05
    cfg2     10  oracle   3.6e-06 0       3.5e-06    3.5e-06 0       0       0       3.8e-06
                 ref      4.2e-06 0       4.1e-06    3.9e-06 0       0       0       4.9e-06
    cfg5      5  oracle   0       0       0          0       0       0       0       4.5e-07
                 ref      0       0       0          0       0       0       0       8.5e-07
    redwood   5  oracle   1.1e-05 8.8e-06 1.2e-05    1.1e-05 0       0       0       3.6e-07
                 ref      6.9e-06 4.9e-06 8.1e-06    6.6e-06 0       0       0       5.5e-07
    freiburg  5  oracle   3.4e-06 2.7e-06 4.8e-06    5.8e-06 2.7e-06 2.6e-06 9.7e-07 2.0e-07
                 ref      3.4e-06 2.9e-06 5.2e-06    6.5e-06 1.9e-06 1.8e-06 6.9e-07 4.9e-07
    chairs32  5  oracle   2.2e-05 8.6e-06 2.4e-05    2.2e-05 0       0       0       3.1e-07
                 ref      1.8e-05 8.8e-06 2.3e-05    2.0e-05 0       3.5e-08 0       6.1e-07
    complex  10  oracle   0       0       2.0e-06    4.2e-07 0       0       0       2.7e-06
                 ref      0       0       2.6e-06    1.9e-06 0       0       0       3.0e-06
    bench    26  oracle   2.6e-06 0       2.7e-06    2.0e-06 0       0       0       5.9e-05
                 ref      2.3e-06 0       2.0e-06    1.6e-06 0       0       0       5.7e-05

(bench: the first 26 of the 160 traced bench iterations -- objects 0 and 1 and six iterations of the next; `--bench-only` runs all.)
(0 = the error lies inside the ulp, rotation-prior and ReLU-kink allowances at every entry.)  Without the ReLU-kink allowance the worst
was 3.6e-4 (small iteration 3, pose x code, in BOTH systems), and 1.3e-2 at the fp32 oracle's own state of small iteration 2: both kinks.

    TAU_H     = 1e-3     the cap.  3x the measured worst (2.4e-5) would be 7e-5; the limit is left at the cap because the device is
                         compared at its own states, which the table does not cover (measured there on MI355X: <= 2.3e-6 on small and
                         redwood, every iteration).
    TAU_B     = 6e-4     likewise above 3x the measured 2.7e-6.
    TAU_SOLVE = 2.5e-4   3 x 8.0e-5 (the reference's own inverse-and-multiply at small iteration 2): a sanity bound only.

What this resolves (tests/test_gn_metric.py, at redwood / small / chairs32 states, first and last iteration): a 1 % error in eight code
columns of the render rows, an 8x8 code tile read from its neighbour, and one typical render row's weight doubled are rejected at every
state; the max-norm check passed all but the last.  A 1 % error in the surface rows' code columns is rejected at small only (the render
rows make up almost all of the code columns' data Gram at redwood and chairs32); the 2e-3 render-column error is accepted at small
iteration 0; a 1 % error of b's code entries is accepted at small's last iteration (the k3 prior dominates s_i); dx from a solve with one
pair of H off by 1 % is accepted at every state -- nothing here detects it.
"""
import numpy as np

TAU_H = 1e-3
TAU_B = 6e-4
SDF_ROUNDOFF = 2e-7       # the jitter twin's sdf offset (tests/test_gpu_parity.py)
EPS_ROT = 2.4e-7          # absolute round-off of J_rot and res_rot in fp32 (O(1) operands)
TAU_SOLVE = 2.5e-4        # a system's own solve: |H dx - b|_i <= TAU_SOLVE (|H| |dx| + |b|)_i on its own stored float32 values


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def scales(lin):
    """(SH (n,n), s (n,)) of an fp64 linearisation."""
    d = np.diag(lin["Dr"] + lin["Ds"])
    sh = np.sqrt(np.outer(d, d))
    s = (np.sqrt(np.diag(lin["Dr"]) * lin["Lr"]) + np.sqrt(np.diag(lin["Ds"]) * lin["Ls"]) + np.abs(lin["b_code_prior"])
         + np.abs(lin["b_rot"]))
    return sh, s


def _rot_allowances(lin, k4):
    n = lin["b"].shape[0]
    j = np.zeros(n)
    j[:7] = np.abs(lin["j_rot"])
    a_h = np.zeros((n, n))
    a_b = np.zeros(n)
    if k4 > 0:
        a_h[3:6, 3:6] = k4 * EPS_ROT * (j[3:6, None] + j[None, 3:6])
        a_b[3:6] = k4 * EPS_ROT * (j[3:6] + 1e-3)
    return a_h, a_b


def _block_max(e):
    return dict(pose=float(e[:6, :6].max()), scale=float(max(e[6, :7].max(), e[:7, 6].max())), pose_code=float(max(e[:7, 7:].max(), e[7:, :7].max())),
                code=float(e[7:, 7:].max()))


def scaled_errors(sys_, lin, k4, pair=None):
    """Scaled errors of the system sys_ = dict(H, b, dx) (float32 values) against the fp64 linearisation lin.
    pair = (the fp32 oracle's system, its sdf-jittered twin) for the jitter allowance, or None.
    -> dict(H={block: max scaled error}, b_pose, b_code, dx, worst=max of all)."""
    h64, b64, dx64 = lin["H"], lin["b"], lin["dx"]
    h = np.asarray(sys_["H"], np.float64)
    b = np.asarray(sys_["b"], np.float64)
    dx = np.asarray(sys_["dx"], np.float64)
    sh, s = scales(lin)
    a_h, a_b = _rot_allowances(lin, k4)
    u_h = 4 * ulp32(h64) + a_h + lin["H_flip"]
    u_b = 4 * ulp32(b64) + a_b + lin["b_flip"]
    if pair is not None:
        it, itj = pair
        u_h = u_h + 2 * np.abs(np.asarray(itj["H"], np.float64) - it["H"])
        u_b = u_b + 2 * np.abs(np.asarray(itj["b"], np.float64) - it["b"])
    tiny = 1e-300
    e_h = np.maximum(np.abs(h - h64) - u_h, 0) / np.maximum(sh, tiny)
    e_b = np.maximum(np.abs(b - b64) - u_b, 0) / np.maximum(s, tiny)
    res = np.abs(h64 @ (dx - dx64))
    adx = np.abs(dx64)
    u_dx = u_h @ adx + u_b
    if pair is not None:
        u_dx = u_dx + 2 * np.abs(h64 @ (np.asarray(itj["dx"], np.float64) - it["dx"]))
    e_dx = np.maximum(res - u_dx, 0) / np.maximum(s + sh @ adx, tiny)
    out = dict(H=_block_max(e_h), b_pose=float(e_b[:7].max()), b_code=float(e_b[7:].max()), dx=float(e_dx.max()), solve=solve_residual(sys_))
    out["worst"] = max(max(out["H"].values()), out["b_pose"], out["b_code"], out["dx"])
    return out


def solve_residual(sys_):
    """max_i |H dx - b|_i / (|H| |dx| + |b|)_i of a system's own stored values, in fp64: whether dx solves the H and b it came with.
    A sanity bound (a dx unrelated to H and b fails it); it does NOT see a solve with one pair of H off by 1 % (tests/test_gn_metric.py:
    the fp32 inverse-and-multiply's own residual reaches 8e-5 of this scale)."""
    h, b, dx = (np.asarray(sys_[k], np.float64) for k in ("H", "b", "dx"))
    return float((np.abs(h @ dx - b) / np.maximum(np.abs(h) @ np.abs(dx) + np.abs(b), 1e-300)).max())


def flat(rec, prefix=""):
    """A scaled_errors record as flat {name: value} (for parity_log and the report)."""
    f = {prefix + "H_" + k: v for k, v in rec["H"].items()}
    f.update({prefix + k: rec[k] for k in ("b_pose", "b_code", "dx", "solve")})
    return f


def within_tau(rec, tau_h=None, tau_b=None):
    """True when every block of a scaled_errors record is within TAU."""
    tau_h = TAU_H if tau_h is None else tau_h
    tau_b = TAU_B if tau_b is None else tau_b
    return (max(rec["H"].values()) <= tau_h and max(rec["b_pose"], rec["b_code"]) <= tau_b and rec["dx"] <= max(tau_h, tau_b)
            and rec["solve"] <= TAU_SOLVE)


def assert_within_tau(rec, what=""):
    assert within_tau(rec), "%s: scaled error against fp64 above tau (tau_H %.1e, tau_b %.1e): %s" % (what, TAU_H, TAU_B, flat(rec))


def check_against_fp64(sys_dev, lin, k4, pair=None, what=""):
    """The check the GPU tests use: every block of the device's scaled error within TAU (pair = the fp32 oracle's system at the same
    state on the same sets and its sdf-jittered twin: the jitter allowance, and the oracle's own scaled errors reported beside the
    device's).  -> flat record {dev_*[, oracle_*]} for parity_log."""
    rd = scaled_errors(sys_dev, lin, k4, pair)
    out = flat(rd, "dev_")
    if pair is not None:
        out.update(flat(scaled_errors(pair[0], lin, k4), "oracle_"))
    assert_within_tau(rd, what)
    return out
