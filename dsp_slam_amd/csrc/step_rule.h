// Levenberg-Marquardt step control of resident joint batches (dsp_batch_step_control, include/dsp_gn.h): the accept / reject rule, written
// once for the device and for the host (k_solve<.., STEP = true> and dsp_debug_step_rule run the very same function, so every branch of
// the rule is tested without a GPU).
//
// Each object carries (has_acc, F_acc, lambda), all fp64.  Iteration e has linearised at the object's current state x_e; for e >= 1 that
// state is a TRIAL, reached by a step from the accepted state x_acc.
//
// Cost.  F_e = (double) loss_e, the float32 k1 L_render + k2 L_sdf that k_solve writes to ObjState::loss, plus -- with a prior on -- the
// prior's chi2 = e^T Lp e at x_e.  The cost deliberately leaves out k3 |z|^2 + k4 res_rot^2: the k4 term (1e7) has a zero jacobian on the
// reference's exact-upright branch (res < 1e-7, loss.py:172-173), so the first step tilts freely and a cost with k4 in it jumps by two
// orders of magnitude at iteration 1 (0.30 -> 32.8 on the CPU oracle); it then rejects the very steps that lower the loss and ends worse
// (returned loss 0.070 instead of 0.0103, 14 iterations).  The cost is the quantity the caller gets back as `loss`.
//
// Decision.
//   e == 0 (no accepted state yet): accept; lambda = lambda0.
//   F_e < F_acc (strict; false for NaN, so a tie is a rejection): accept; lambda <- lambda * down.
//   otherwise: reject; lambda <- min(max(lambda, lambda_min) * up, lambda_max).
// Accept: x_acc <- x_e, F_acc <- F_e, and the assembled [H | b] -- the reference's system with its own damping and, with a prior, the
// prior's block -- is saved as it stands before the elimination.  Reject: [H | b] is reloaded from the saved copy, the state the iteration
// "started from" becomes x_acc, and the trial with its linearisation is discarded.
// Step.  (S + lambda I) dx = b with S the accepted state's system; lambda is added in fp64 to the diagonal entries of the live unknowns,
// behind everything else (lambda == 0 adds nothing: the bits of the system stay).  The update exp(lr dx) x_acc follows as without the rule.
//
// No step is applied on the run's last iteration, nor on an iteration whose solved step meets the convergence rule: the object's state is
// put back to x_acc (with everything derived from it), so the returned state is the best EVALUATED state and the returned loss is the
// loss AT that state.  A run of N iterations therefore makes N linearisations and at most N - 1 steps.
//
// A trial state at which the object fails by the reference's rules (< 10 in-sphere samples, K == 0, NaN, singular solve, underivable
// pose) fails the object, as in a run without step control: turning that into a rejection needs the status words other kernels set to
// be reversible, and is left for later.
#pragma once
#include <math.h>
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSP_STEP_HD __host__ __device__
#else
#define DSP_STEP_HD
#endif

namespace step_rule {

constexpr int NOT_EVALUATED = 0, ACCEPTED = 1, REJECTED = 2;

struct Params {
    double lambda0, up, down, lambda_min, lambda_max;
};

// all five zero: the feature is off (the initial state)
inline bool is_off(const Params& p) { return p.lambda0 == 0.0 && p.up == 0.0 && p.down == 0.0 && p.lambda_min == 0.0 && p.lambda_max == 0.0; }

// dsp_batch_step_control's checks of a setting that is not "off": nullptr, or what is wrong
inline const char* check(const Params& p) {
    if (!std::isfinite(p.lambda0) || !std::isfinite(p.up) || !std::isfinite(p.down) || !std::isfinite(p.lambda_min) || std::isnan(p.lambda_max) || p.lambda_max == -INFINITY)
        return "step control: every value must be finite (lambda_max may be +inf)";
    if (p.lambda0 < 0.0) return "step control: lambda0 must be >= 0";
    if (!(p.up > 1.0)) return "step control: up must be > 1";
    if (!(p.down > 0.0 && p.down <= 1.0)) return "step control: down must be in (0, 1]";
    if (!(p.lambda_min > 0.0)) return "step control: lambda_min must be > 0";
    if (p.lambda_max < p.lambda_min) return "step control: lambda_max must be >= lambda_min";
    return nullptr;
}

// One decision.  first: iteration 0 of the run, nothing accepted yet.  lambda: the object's value, updated in place.
DSP_STEP_HD inline int decide(bool first, double F_e, double F_acc, const Params& p, double& lambda) {
    if (first) { lambda = p.lambda0; return ACCEPTED; }
    if (F_e < F_acc) { lambda = lambda * p.down; return ACCEPTED; }
    lambda = fmin(fmax(lambda, p.lambda_min) * p.up, p.lambda_max);
    return REJECTED;
}

}  // namespace step_rule
