// The body of k_solve and k_solve_masked (gn_kernels.hip), included once in each: no include guard, not a header of its own.  In scope:
// the template arguments GROUPS, STOP, PRIOR, STEP, the kernel's arguments, `constexpr bool MASK` and `const unsigned char* live`
// (the mask of unknowns, dsp_batch_unknowns; null where MASK is false).  Everything the mask adds sits under `if constexpr (MASK)`.
    // wn (observation weights; nullptr = off): 2 doubles per member, the sums of the caller's weights that take the place of M (pose-only: Ma)
    // and K as the divisors of the means -- the member's own (k_weight_sums) or, GROUPS, the group's pooled ones (k_group_reduce).  The
    // counts stay counts.  (double)M is what the divisions below widen M to anyway, and (float)(double)M == (float)M: with wn == nullptr
    // every result bit is that of the kernel before it had the argument; with unit weights wn holds (double)M and (double)K exactly.
    static_assert(!(STEP && GROUPS), "step control: joint batches without groups only");
    __shared__ double A[NS1][NS1 + 1];          // [H | b] in rows 0..n-1 (b = column n); b is also kept as ROW n (rows 64 .. 71 are one register of the elimination)
    const int b = blockIdx.x, tid = threadIdx.x;
    if constexpr (GROUPS) { if (grp[b].leader != b) return; }
    const ObjConst c = oc[b];
    ObjState& s = st[b];
    // Everything this launch reads from global memory goes out HERE, before the first of it is waited for -- the status word included
    // (k_solve is a chain of latencies: status -> Gram loads -> state for the prior -> ... was three round trips of ~1 us each).
    const int status = s.status;
    int K = s.K;
    if constexpr (GROUPS) K = gmk[2 * b + 1];
    float pr_tco[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) pr_tco[i] = s.t_co[i];
    const float pr_scale = s.scale;
    // the pose and the code this iteration started from, parked in LDS for the update at the end (visible after the assembly's barrier)
    __shared__ float s_toc0[16], s_code0[CODE_LEN];
    const float park = tid < 16 ? s.t_oc[tid] : (tid >= 64 && tid < 64 + CODE_LEN) ? s.code[tid - 64] : 0.f;
    // The 72 x 72 Gram matrices of the two terms, reduced over the Gram kernel's slices by k_gram_reduce.  (Summing the per-slice partials HERE
    // -- one launch and one kernel boundary less per iteration -- was measured and lost: 786 KB of partials through ONE CU's load path take longer
    // than the 41-workgroup reduce kernel and the boundary together, profiles/r06_removed_experiments.md.)
    const double* G0p = gsum + ((size_t)b * 2 + 0) * (72 * 72);
    const double* G1p = gsum + ((size_t)b * 2 + 1) * (72 * 72);
    auto gram = [=](int term, int idx) -> double { return (term ? G1p : G0p)[idx]; };
    int M = c.n_pts;
    if constexpr (GROUPS) M = gmk[2 * b];
    const int n_alive = s.n_alive;
    const double Mw = wn ? wn[2 * b] : (double)(prm.pose_only && n_alive >= 0 ? n_alive : M);
    const double Kw = wn ? wn[2 * b + 1] : (double)K;
    const int pd = prm.pose_only ? 6 : 7;
    const int n = prm.pose_only ? 6 : NSOLVE;
    // thread (tr, tc) fills column tc of rows tr, tr+12, ... of the joint system: its Gram loads
    const int tr0 = tid / (NSOLVE + 1), j = tid % (NSOLVE + 1);
    constexpr int RG = 12, RPT = (NSOLVE + RG - 1) / RG;
    double g0[RPT], g1[RPT];
    float zq[RPT];
    [[maybe_unused]] double ex[RPT];
    [[maybe_unused]] bool pr_on = false;
    [[maybe_unused]] const double* exb = nullptr;
    if constexpr (PRIOR) {
        int ob = b;
        if constexpr (GROUPS) ob = grp[b].object;
        pr_on = pr.on[ob] != 0;
        exb = pr.extra + (size_t)ob * pr.n * (pr.n + 1);
    }
    // the object's mask (MASK): this thread's column and rows, and every entry in LDS for the steps behind the assembly
    [[maybe_unused]] const unsigned char* lv = nullptr;
    [[maybe_unused]] bool fzj = false, fzi[RPT] = {};
    [[maybe_unused]] unsigned char fz_mine = 0;
    __shared__ unsigned char s_fz[MASK ? NS1 : 1];
    if constexpr (MASK) {
        int ob = b;
        if constexpr (GROUPS) ob = grp[b].object;
        lv = live + (size_t)ob * n;
        fzj = j < n && !lv[j];
        if (tid < n) fz_mine = !lv[tid];
        if (!prm.pose_only) {
#pragma unroll
            for (int q = 0; q < RPT; ++q) fzi[q] = !lv[min(tr0 + RG * q, n - 1)];
        }
    }
    if (!prm.pose_only) {
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const int i = tr0 + RG * q;
            const bool live = tr0 < RG && i < n;
            const int col = (j < n) ? j : 71;            // the augmented column is b = -J^T r~ (Gram column 71)
            const int gi = live ? i * 72 + col : 0;
            g0[q] = gram(0, gi);
            g1[q] = gram(1, gi);
            if constexpr (PRIOR) ex[q] = exb[gi];        // the prior's block has the same 72-column rows (column 71 = b_extra)
            zq[q] = s.code[min(max(i - pd, 0), CODE_LEN - 1)];             // the right-hand side's k3 z term (optimizer.py:172); unconditional: a
                                                                           // load in a branch is waited for at the branch's end
        }
    }
    const double g_loss0 = prm.pose_only ? 0.0 : gram(0, 71 * 72 + 71), g_loss1 = prm.pose_only ? 0.0 : gram(1, 71 * 72 + 71);
    // step control: the object's rule state (iteration 0 has none yet) and, with a prior, chi2 at this state (k_prior_terms, pass kind 2)
    [[maybe_unused]] double sc_Facc = 0.0, sc_lambda = 0.0, sc_chi2 = 0.0;
    [[maybe_unused]] float sc_loss_acc = 0.f, sc_loss = 0.f;
    if constexpr (STEP) {
        if (iter > 0) { sc_Facc = sd.obj[b].F_acc; sc_lambda = sd.obj[b].lambda; sc_loss_acc = sd.obj[b].loss_acc; }
        if constexpr (PRIOR) { if (pr_on) sc_chi2 = pr.res[(size_t)b * prior_math::RES_STRIDE + prior_math::RES_STRIDE - 1]; }
        // the log row of an iteration the object does not evaluate (failed, frozen) reads "not evaluated"; an object left out of a
        // partial re-run keeps the rows of the run that produced its result
        if (tid == 0 && status != DSP_STATUS_SKIP) sd.log[(size_t)iter * n_obj + b] = StepLogEnt{0.0, 0.0, step_rule::NOT_EVALUATED, 0};
    }
    if (status != DSP_STATUS_GOOD) return;
    if (tid < 16) s_toc0[tid] = park;
    if (tid >= 64 && tid < 64 + CODE_LEN) s_code0[tid - 64] = park;
    if constexpr (MASK) { if (tid < n) s_fz[tid] = fz_mine; }
    if (!prm.pose_only) {
        // losses (optimizer.py:134-155): mean of robust residual^2; an empty set gives NaN in the reference
        if (Mw == 0.0 || Kw == 0.0) { if (tid == 0) s.status = DSP_STATUS_NAN; return; }
        const float sdf_loss = (float)g_loss0 / (float)Mw;
        const float ren_loss = (float)g_loss1 / (float)Kw;
        if (isnan(sdf_loss) || isnan(ren_loss)) { if (tid == 0) s.status = DSP_STATUS_NAN; return; }
        if (tid == 0) s.loss = prm.k1 * ren_loss + prm.k2 * sdf_loss;
        if constexpr (STEP) sc_loss = prm.k1 * ren_loss + prm.k2 * sdf_loss;
        float jrot[7], res_rot;
        rotation_prior(pr_tco, pr_scale, jrot, res_rot);
        // only entries 3 and 5 of the prior's jacobian are non-zero; selects instead of a run-time index keep it out of scratch
        const float jrot3 = jrot[3], jrot5 = jrot[5];
        auto jr = [=](int i) { return i == 3 ? jrot3 : (i == 5 ? jrot5 : 0.f); };
        const double w_s = (double)prm.k2 / Mw, w_r = (double)prm.k1 / Kw;
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const int i = tr0 + RG * q;
            if (!(tr0 < RG && i < n)) continue;
            double v;
            if (j < n) {
                v = w_s * g0[q] + w_r * g1[q];                                                 // :161-168
                if (i >= pd && i == j) v += (double)prm.k3;                                    // :170
                // code entries beyond the decoder's code length (32-D codes in the 64-wide state) have a zero jacobian: their rows are
                // k3 on the diagonal and 0 on the right -- pinned to the identity so that they stay decoupled (dx = 0) even with k3 = 0
                if (i >= pd + prm.code_len && i == j) v = 1.0;
                if (i < pd && j < pd) v += (double)prm.k4 * (double)jr(i) * (double)jr(j);       // :176,178
                if constexpr (PRIOR) { if (pr_on && i < pd + prm.code_len && j < pd + prm.code_len) v += ex[q]; }     // J^T Lp J
                if (i < pd && i == j) v += 1.0;                                                // :183
                if (i == pd - 1 && j == pd - 1) v += (double)prm.s_damp;                       // :184
            } else {
                v = -(w_s * g0[q] + w_r * g1[q]);                                              // b = -J^T r~
                if (i >= pd) v -= (double)prm.k3 * (double)zq[q];                              // :172
                if (i >= pd + prm.code_len) v = 0.0;
                if (i < pd) v += (double)prm.k4 * (double)jr(i) * (double)res_rot;             // :177,179 (sign as written)
                if constexpr (PRIOR) { if (pr_on && i < pd + prm.code_len) v += ex[q]; }         // -J^T Lp e
            }
            if constexpr (MASK) { if (fzi[q] || fzj) v = i == j ? 1.0 : 0.0; }                 // frozen: conditioned on, behind everything else
            A[i][j] = v;
        }
    } else {
        // pose-only (optimizer.py:68-72): H = J6^T J6 / M + 1e-2 I, b = -J6^T r / M with the raw residual
        const double Ma = Mw;
        if (Ma == 0.0) {      // no point (left): H = J^T J / 0 is NaN in the reference; the trace still records the count
            if (tid == 0) {
                s.status = DSP_STATUS_NAN;
                if (trace) trace[((size_t)iter * n_obj + b) * TRACE_STRIDE + NSOLVE * NSOLVE + 2 * NSOLVE + 82] = 0.f;
            }
            return;
        }
        for (int e = tid; e < n * (n + 1); e += SOLVE_THREADS) {
            const int i = e / (n + 1), j = e % (n + 1);
            double v;
            if (j < n) {
                v = gram(0, i * 72 + j) / Ma;
                if constexpr (PRIOR) { if (pr_on) v += exb[e]; }
                if (i == j) v += 1e-2;
            } else {
                v = -gram(0, i * 72 + 71) / Ma;
                if constexpr (PRIOR) { if (pr_on) v += exb[e]; }
            }
            if constexpr (MASK) { if (!lv[i] || (j < n && !lv[j])) v = i == j ? 1.0 : 0.0; }
            A[i][j] = v;
        }
    }
    __syncthreads();
    if (trace) {   // [iter][obj][71*71 H | 71 b | 71 dx | 16 t_oc | 64 code | V m K]
        float* tr = trace + ((size_t)iter * n_obj + b) * TRACE_STRIDE;
        for (int e = tid; e < n * n; e += SOLVE_THREADS) tr[(e / n) * NSOLVE + (e % n)] = (float)A[e / n][e % n];
        for (int e = tid; e < n; e += SOLVE_THREADS) tr[NSOLVE * NSOLVE + e] = (float)A[e][n];
        if (tid < 16) tr[NSOLVE * NSOLVE + 2 * NSOLVE + tid] = s.t_oc[tid];
        if (tid < 64) tr[NSOLVE * NSOLVE + 2 * NSOLVE + 16 + tid] = s.code[tid];
        if (tid < 64) tr[5280 + tid] = s.depths[tid];
        if (tid == 0) {
            tr[NSOLVE * NSOLVE + 2 * NSOLVE + 80] = (float)s.V;
            tr[NSOLVE * NSOLVE + 2 * NSOLVE + 81] = (float)s.m;
            // pose-only: K = the points the system was built from (M, or the inlier filter's survivors: Ma above)
            tr[NSOLVE * NSOLVE + 2 * NSOLVE + 82] = prm.pose_only ? (float)(s.n_alive >= 0 ? s.n_alive : M) : (float)s.K;
            tr[NSOLVE * NSOLVE + 2 * NSOLVE + 83] = (float)(s.vsum & 0xffffu);
            tr[NSOLVE * NSOLVE + 2 * NSOLVE + 84] = (float)(s.vsum >> 16);
            tr[NSOLVE * NSOLVE + 2 * NSOLVE + 85] = (float)(s.ksum & 0xffffu);
            tr[NSOLVE * NSOLVE + 2 * NSOLVE + 86] = (float)(s.ksum >> 16);
        }
        __syncthreads();
    }
    if constexpr (STEP) {
        // the decision (uniform: every thread holds the same numbers), then the system the step is solved from
        const double F_e = (double)sc_loss + sc_chi2;
        double lam = sc_lambda;
        const int dec = step_rule::decide(iter == 0, F_e, sc_Facc, sd.p, lam);
        double* sv = sd.sys + (size_t)b * STEP_SYS;
        StepObj& so = sd.obj[b];
        if (dec == step_rule::ACCEPTED) {
            for (int e = tid; e < n * (n + 1); e += SOLVE_THREADS) sv[e] = A[e / (n + 1)][e % (n + 1)];
            if (tid < 16) so.t_oc[tid] = s_toc0[tid];
            if (tid >= 64 && tid < 64 + CODE_LEN) so.code[tid - 64] = s_code0[tid - 64];
            if (tid == 0) { so.F_acc = F_e; so.loss_acc = sc_loss; }
        } else {
            for (int e = tid; e < n * (n + 1); e += SOLVE_THREADS) A[e / (n + 1)][e % (n + 1)] = sv[e];
            if (tid < 16) s_toc0[tid] = so.t_oc[tid];
            if (tid >= 64 && tid < 64 + CODE_LEN) s_code0[tid - 64] = so.code[tid - 64];
            if (tid == 0) s.loss = sc_loss_acc;           // the loss AT the state the object keeps
        }
        if (tid == 0) {
            so.lambda = lam;
            sd.log[(size_t)iter * n_obj + b] = StepLogEnt{F_e, lam, dec, 0};
        }
        __syncthreads();
        // lambda on the diagonal of the live unknowns, behind everything else (0 adds nothing); the elimination's first barrier follows
        if constexpr (MASK) {
            if (lam != 0.0 && tid < pd + prm.code_len && !s_fz[tid]) A[tid][tid] += lam;      // not on a frozen diagonal: H_ii stays 1
        } else {
            if (lam != 0.0 && tid < pd + prm.code_len) A[tid][tid] += lam;
        }
    }
    {
        // 2. H dx = b by elimination in fp64.  H = sum w J^T J + positive diagonal is symmetric (bit for bit: the Gram kernel's fmaf chains
        //    commute) positive definite, so no pivoting is needed (the reference inverts H with fp32 LU, optimizer.py:186).  The right-hand side
        //    rides along as column n (and row n) of the augmented matrix; rows above the pivot are eliminated too, so there is no back substitution:
        //    after step n - 1 column n holds d_i dx_i.
        __shared__ double rdv[NS1];
        __shared__ int s_sing;
        if (tid < n) A[n][tid] = A[tid][n];           // b as row n
        if (tid == 0) s_sing = 0;                     // raised by the panel waves
        {
        // Rows in lanes: wave w < 9 owns
        // columns 8w .. 8w+7 and lane l is row l: v0[jj] = A[l][8w+jj]; rows 64 .. 71 (seven code unknowns and the right-hand side) sit
        // in one more register, vx = A[64 + (l & 7)][8w + (l >> 3)].  A step costs a wave THREE LDS reads (its rows' entries of column
        // k for both register sets, and the per-lane column entry of vx); the pivot and the eight column entries c_jk are rows of the
        // same column, i.e. other lanes' values of the register just read: v_readlane into scalar operands of the FMAs.  Waves whose
        // columns are all finished skip the step.  Values computed for columns <= k are never read again.
        const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;      // w in a scalar register: lane selects below are scalar
        const bool worker = w < 9;
        double* Af = &A[0][0];
        constexpr int LDA = NS1 + 1;
        const int o0 = lane * LDA, oxr = (64 + (lane & 7)) * LDA, oxc = (8 * w + (lane >> 3)) * LDA;
        __syncthreads();
        double v0[8], vx = 0.0;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) v0[jj] = worker ? Af[o0 + 8 * w + jj] : 0.0;
        if (worker) vx = Af[oxr + 8 * w + (lane >> 3)];
        bool sing = false;
        auto readlane_f64 = [](double x, int l) {
            return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
        };
        {
        // Panel schedule.  Every a_ij sees v -= (c_ik rd_k) c_jk for k ascending (tests/test_solve_schedule.py emulates the schedule lane for lane),
        // with ONE barrier per EIGHT pivots.  Wave kb owns
        // columns 8kb .. 8kb+7 whole (rows in lanes), so it can run the eight steps of its panel on its own registers: the pivot and the
        // column entries c_jk are lanes of the register that IS column k (v_readlane), and only the eight extra rows (vx) need the LDS --
        // the wave's own write, read back in order, off the pivot chain.  It publishes each column as it becomes final, with the
        // pivot's reciprocal.  After the barrier the waves to its right apply the eight steps in one burst (LDS reads issued up front).
        // Measured with shader-clock stamps (profiles/r05_latency_kernel_stats.md; the stamp patch: profiles/r06_removed_experiments.patch): panel 2600 cycles, barrier 160,
        // burst of the next panel's wave 2150 -> 18 us for the 71 pivots against 25 with one barrier per pivot (860 cycles each).  Both
        // phases are issue-bound, ~8 cycles per instruction for a lone wave of fp64 FMAs and v_readlane pairs (~40 instructions per
        // step each): raising the next panel wave's priority, bursts of 2 or 8 steps, changed nothing.
        const bool active = worker && 8 * w <= n;                         // pose-only (n = 6): wave 0 alone
#pragma unroll 1
        for (int kb = 0; 8 * kb < n; ++kb) {
            if (active && w == kb) {
                auto panel = [&](auto last_c) {
                    constexpr bool LAST = decltype(last_c)::value;        // wave 8: rows / pivots 64 .. 70 live in vx
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const int k = 8 * kb + t;
                        if (k < n) {                                      // uniform
                            Af[o0 + k] = v0[t];                           // column k is final: publish it (rows 0 .. 63, then rows 64 .. 71)
                            if ((lane >> 3) == t) Af[oxr + k] = vx;
                            const bool open = t < 7 || LAST;              // a column of mine is still open
                            double cix = 0.0, cjx = 0.0;
                            // rows 64 .. 71 of column k and rows 8w .. 8w+7 come back from the LDS: OTHER LANES' writes of this wave.  The
                            // LDS serves a wave's instructions in order, but to the compiler lanes are unrelated threads (without the
                            // fences it hoisted the non-writing lanes' read above the write): wave-scope release / acquire, no instruction
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                            if (open) { cix = Af[oxr + k]; cjx = Af[oxc + k]; }
                            __builtin_amdgcn_sched_barrier(0);
                            // the pivot chain: nothing in it waits for the LDS (except in wave 8, whose column entries are rows of vx)
                            const double d = LAST ? readlane_f64(vx, 9 * t) : readlane_f64(v0[t], k);
                            const double rdk = fast_recip(d);
                            sing = sing || !(d > 0.0);                    // also NaN
                            if (open) {
                                const double l0 = lane == k ? 0.0 : v0[t] * rdk;
#pragma unroll
                                for (int jj = t + 1; jj < 8; ++jj)
                                    v0[jj] = fma(-l0, LAST ? readlane_f64(cix, jj) : readlane_f64(v0[t], 8 * kb + jj), v0[jj]);
                            }
                            __builtin_amdgcn_sched_barrier(0);
                            if (lane == 0) rdv[k] = rdk;
                            if (open) {
                                const double lx = (64 + (lane & 7)) == k ? 0.0 : cix * rdk;
                                vx = fma(-lx, cjx, vx);
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                };
                if (kb == 8) panel(BoolC<true>{}); else panel(BoolC<false>{});
                if (sing && lane == 0) s_sing = 1;
            }
            __syncthreads();                                              // panel kb and its reciprocals are published
            if (active && w > kb) {
                // every column of the panel exists here (8 kb + 7 < 8 w <= n) and every pivot row is one of rows 0 .. 63: straight-line
                // code, in two half-bursts of four steps whose 16 LDS reads are all in flight before the first use
                const int cbase = (w == 8) ? 0 : 8 * w;
                constexpr int BS = 4;       // (8: 125 registers, no faster; 2: slower)
#pragma unroll
                for (int h = 0; h < 8 / BS; ++h) {
                    double ci0[BS], cix[BS], cjx[BS], rk[BS];
#pragma unroll
                    for (int t = 0; t < BS; ++t) {
                        const int k = 8 * kb + BS * h + t;
                        ci0[t] = Af[o0 + k]; cix[t] = Af[oxr + k]; cjx[t] = Af[oxc + k]; rk[t] = rdv[k];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int t = 0; t < BS; ++t) {
                        const int k = 8 * kb + BS * h + t;
                        const double csrc = (w == 8) ? cix[t] : ci0[t];
                        const double l0 = lane == k ? 0.0 : ci0[t] * rk[t], lx = cix[t] * rk[t];
                        // the eight column entries into eight scalar pairs first, then the eight FMAs (one pair reused eight times
                        // serialises v_readlane -> FMA through the scalar write: 2550 -> 2150 cycles per burst)
                        double cj[8];
#pragma unroll
                        for (int jj = 0; jj < 8; ++jj) cj[jj] = readlane_f64(csrc, cbase + jj);
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int jj = 0; jj < 8; ++jj) v0[jj] = fma(-l0, cj[jj], v0[jj]);
                        __builtin_amdgcn_sched_barrier(0);
                        vx = fma(-lx, cjx[t], vx);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        }
        __syncthreads();
        // dx_i = A[i][n] / d_i: column n is register n & 7 of wave n >> 3 (n = 71: wave 8, v0[7] and the vx lanes of column 7; n = 6: wave 0, v0[6])
        if (w == (n >> 3)) {
            const double bn = n == NSOLVE ? v0[NSOLVE & 7] : v0[6];
            if (lane < n) Af[o0 + n] = bn * rdv[lane];
            if ((lane >> 3) == (n & 7) && 64 + (lane & 7) < n) Af[oxr + n] = vx * rdv[64 + (lane & 7)];
        }
        }
        __syncthreads();
        if (s_sing) { if (tid == 0) s.status = DSP_STATUS_NAN; return; }      // uniform
        __syncthreads();
    }
    if constexpr (!STEP) {
    if (trace) {
        float* tr = trace + ((size_t)iter * n_obj + b) * TRACE_STRIDE;
        for (int e = tid; e < n; e += SOLVE_THREADS) tr[NSOLVE * NSOLVE + NSOLVE + e] = (float)A[e][n];
    }
    }
    // the convergence rule, on the step the update below applies (lr dx; pose-only: dx): thread i < n holds entry i
    bool stop_now = false;
    if constexpr (STOP) {
        bool ok = true;
        if (tid < n) {
            const double step = fabs((double)(prm.pose_only ? 1.f : prm.lr) * A[tid][n]);
            ok = step < (tid < pd ? stop.pose_tol : stop.code_tol);        // strict, and false for a NaN step
            if constexpr (MASK) ok = ok || s_fz[tid];                      // a frozen entry's step is 0: it blocks no stop, whatever the tolerance
        }
        stop_now = __syncthreads_and(ok) && iter + 1 >= stop.min_iterations;
    }
    // step control: no step on the run's last iteration or on a step that meets the rule -- dx reads zero (the trace row too) and the
    // update below puts the object back to x_acc, with everything the front of an iteration derives from it
    [[maybe_unused]] bool no_step = false;
    if constexpr (STEP) {
        no_step = sd.last != 0 || stop_now;
        if (no_step && tid < n) A[tid][n] = 0.0;          // (each entry was last read by this very thread)
        __syncthreads();
        if (trace) {
            float* tr = trace + ((size_t)iter * n_obj + b) * TRACE_STRIDE;
            for (int e = tid; e < n; e += SOLVE_THREADS) tr[NSOLVE * NSOLVE + NSOLVE + e] = (float)A[e][n];
        }
    }
    // 3. update (optimizer.py:187-192 / 73-74).  Wave 0 carries the pose (one lane: exp map, 4x4 product, the next iteration's derived
    //    state -- a few us of serial fp64), wave 1 the code, and waves 2.. the next iteration's code bias once the code is in LDS: the
    //    serial pose work no longer sits in front of the bias loop.
    __shared__ float zc[CODE_LEN];
    if (!prm.pose_only && tid >= 64 && tid < 64 + CODE_LEN) {
        const int i = tid - 64;
        float zv = s_code0[i] + prm.lr * (float)A[pd + i][n];
        if constexpr (STEP) { if (no_step) zv = s_code0[i]; }
        if constexpr (MASK) { if (s_fz[pd + i]) zv = s_code0[i]; }      // a frozen code entry keeps its bits (x + 0.f would turn -0.f into +0.f)
        s.code[i] = zv;
        zc[i] = zv;
        // the prepass margin follows the code (this wave holds all CODE_LEN = 64 entries)
        float zmax = fabsf(zv);
        bool bad = zv != zv;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { zmax = fmaxf(zmax, __shfl_xor(zmax, d)); bad = bad || __shfl_xor((int)bad, d); }
        if (i == 0) s.lp_delta = lp_delta_of(bad ? __int_as_float(0x7f800000) : zmax, prm.lp);
    }
    __syncthreads();
    if (tid < 64) {
        // the whole of wave 0 runs the serial pose arithmetic (a wave costs what a lane costs), so that lane 0 stores the matrices and
        // lane i the i-th depth sample; the old pose and code were parked in LDS by the assembly: no global round trip on this path
        float dx[7], dT[16], nt[16];
        for (int i = 0; i < pd; ++i) dx[i] = (prm.pose_only ? 1.f : prm.lr) * (float)A[i][n];
        if (prm.pose_only) exp_se3_dev(dx, dT); else exp_sim3_dev(dx, dT);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc += dT[4 * r + k] * s_toc0[4 * k + cc];
                nt[4 * r + cc] = acc;
            }
        if constexpr (STEP) {
            if (no_step) {
#pragma unroll
                for (int i = 0; i < 16; ++i) nt[i] = s_toc0[i];
            }
        }
        if constexpr (MASK) {
            // no live pose entry: the update is skipped, so t_oc and everything derived from it below keep their bits across iterations
            bool pose_live = false;
            for (int i = 0; i < pd; ++i) pose_live = pose_live || !s_fz[i];
            if (!pose_live) {
#pragma unroll
                for (int i = 0; i < 16; ++i) nt[i] = s_toc0[i];
            }
        }
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s.t_oc[i] = nt[i];
            s.vsum = 0; s.ksum = 0;
            s.V = 0; s.P = 0;      // the wave-per-ray bookkeeping counts into these (k_front_wave, k_band_wave); the scans of the other forms overwrite them
            s.n_iter = iter + 1;   // updates applied (dsp_batch_iterations_used)
        }
        if constexpr (STOP) { if (prm.pose_only && stop_now && tid == 0) s.status = DSP_STATUS_DONE; }
        if (!prm.pose_only) {
            const IterDerived r = derive_iter_core(nt, prm.n_depth);
            if (!r.ok) {
                if (tid == 0) s.status = DSP_STATUS_NAN;
            } else {
                if constexpr (STOP) { if (stop_now && tid == 0) s.status = DSP_STATUS_DONE; }
                if (tid == 0) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) s.t_co[i] = r.t_co[i];
                    s.scale = r.scale;
                }
                // forensics (dsp_batch_set_depth_schedule): the next iteration samples exactly these depths
                const float* dn = depths_next ? depths_next + MAX_DEPTH_SAMPLES * b : nullptr;
                if (tid < prm.n_depth) s.depths[tid] = dn ? dn[tid] : linspace_at(r, tid, prm.n_depth);
                if (tid == 0) {
                    s.dmin = dn ? dn[0] : r.dmin;
                    s.dmax = dn ? dn[prm.n_depth - 1] : r.dmax;
                }
            }
        }
    }
    // 4. the next iteration's per-object code bias (k_code_bias: same k-ordered fmaf chains), by the waves that are not busy with the pose
    if (!prm.pose_only && cbias && tid >= 128) {
        for (int e = tid - 128; e < 2 * WIDTH; e += SOLVE_THREADS - 128) {
            const int which = e / WIDTH, o = e % WIDTH;
            float acc = which == 0 ? cb0[o] : cblat[o];
            const float* w = codew + (size_t)e * CODE_LEN;
            for (int cidx = 0; cidx < CODE_LEN; ++cidx) acc = fmaf(w[cidx], zc[cidx], acc);
            cbias[(size_t)b * 2 * WIDTH + e] = acc;
        }
    }
