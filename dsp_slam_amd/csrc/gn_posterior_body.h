// The body of k_posterior and k_posterior_masked (gn_kernels.hip), included once in each: no include guard, not a header of its own.  In
// scope: the template arguments GROUPS, PRIOR, the kernel's arguments, `constexpr bool MASK` and `const unsigned char* live` (the mask of
// unknowns, dsp_batch_unknowns; null where MASK is false).  Everything the mask adds sits under `if constexpr (MASK)`.
    __shared__ double A[NSOLVE][NSOLVE + 1];
    __shared__ double s_c[NSOLVE + 1], s_d0[NSOLVE + 1];
    __shared__ int s_sing;
    const int b = blockIdx.x, tid = threadIdx.x;
    int n_mem = 1, row_i = b;
    if constexpr (GROUPS) {
        const GroupEnt g = grp[b];
        if (g.leader != b) return;
        n_mem = g.n_members; row_i = g.object;
    }
    const int parked = park[b];
    if (parked == DSP_STATUS_SKIP) return;           // partial re-run: the record of the earlier run stands, like the result row
    ObjState& s = st[b];
    const ObjConst c = oc[b];
    const int status = s.status;
    double* out = rec + (size_t)row_i * rec_stride;
    const int pd = prm.pose_only ? 6 : 7;
    const int n = prm.pose_only ? 6 : pd + prm.code_len;       // live unknowns: the leading n x n block
    int M = c.n_pts, K = s.K, V = s.V;
    if constexpr (GROUPS) {
        M = gmk[2 * b]; K = gmk[2 * b + 1];
        V = 0;
        for (int v = 0; v < n_mem; ++v) if (st[b + v].status == DSP_STATUS_GOOD) V += st[b + v].V;
    }
    if (prm.pose_only) { M = (s.n_alive >= 0) ? s.n_alive : M; K = 0; V = 0; }
    const double Mw = wn ? wn[2 * b] : (double)M, Kw = wn ? wn[2 * b + 1] : (double)K;      // the record's M, V, K stay counts
    __shared__ unsigned char s_fz[MASK ? NSOLVE + 1 : 1];
    if constexpr (MASK) { if (tid < n) s_fz[tid] = !live[(size_t)row_i * (prm.pose_only ? 6 : NSOLVE) + tid]; }     // (visible behind the barrier below)
    const double* G0p = gsum + ((size_t)b * 2 + 0) * (72 * 72);
    const double* G1p = gsum + ((size_t)b * 2 + 1) * (72 * 72);
    // status of the record; the loss at x* in k_solve's float32 arithmetic
    int pstat = 0;
    float loss = 0.f;
    if (status != DSP_STATUS_GOOD) pstat = 1;
    else if (prm.pose_only) { if (Mw == 0.0) pstat = 1; }
    else if (Mw == 0.0 || Kw == 0.0) pstat = 1;
    else {
        const double g_loss0 = G0p[71 * 72 + 71], g_loss1 = G1p[71 * 72 + 71];
        const float sdf_loss = (float)g_loss0 / (float)Mw;
        const float ren_loss = (float)g_loss1 / (float)Kw;
        if (isnan(sdf_loss) || isnan(ren_loss)) pstat = 1;
        else loss = prm.k1 * ren_loss + prm.k2 * sdf_loss;
    }
    __syncthreads();          // every thread has read the status words: put the parked ones back (the pass changes no result)
    for (int v = tid; v < n_mem; v += POST_THREADS) st[b + v].status = park[b + v];
    // the state the record is taken at
    if (level >= 2) {
        float* fs = reinterpret_cast<float*>(out + POST_L1 + NSOLVE * NSOLVE + NSOLVE);
        if (tid < 16) fs[tid] = s.t_oc[tid];
        if (tid < CODE_LEN) fs[16 + tid] = s.code[tid];
        if (tid < MAX_DEPTH_SAMPLES) fs[16 + CODE_LEN + tid] = prm.pose_only ? 0.f : s.depths[tid];
    }
    if (pstat) {              // uniform
        for (int e = tid; e < (level >= 2 ? POST_L1 + NSOLVE * NSOLVE + NSOLVE : POST_L1); e += POST_THREADS) out[e] = 0.0;
        __syncthreads();
        if (tid == 0) { out[162] = (double)pstat; out[164] = (double)M; out[165] = (double)V; out[166] = (double)K; }
        return;
    }
    // 1. Lambda (lower triangle, mirrored) and g
    float jrot3 = 0.f, jrot5 = 0.f, res_rot = 0.f;
    double w_s = 0.0, w_r = 0.0;
    if (!prm.pose_only) {
        float pr_tco[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) pr_tco[i] = s.t_co[i];
        float jrot[7];
        rotation_prior(pr_tco, s.scale, jrot, res_rot);
        jrot3 = jrot[3]; jrot5 = jrot[5];
        w_s = weights ? (double)prm.k2 : (double)prm.k2 / Mw;
        w_r = weights ? (double)prm.k1 : (double)prm.k1 / Kw;
    }
    auto jr = [=](int i) { return i == 3 ? jrot3 : (i == 5 ? jrot5 : 0.f); };
    [[maybe_unused]] bool pr_on = false;
    [[maybe_unused]] const double* exb = nullptr;
    [[maybe_unused]] int xs = 0;             // row length of the prior's block; its last column is b_extra
    if constexpr (PRIOR) {
        pr_on = pr.on[row_i] != 0;
        xs = pr.n + 1;
        exb = pr.extra + (size_t)row_i * pr.n * xs;
    }
    // entry (i, j), i >= j, of Lambda from the Gram sums (also re-read by the refinement of cov_pose below: the sweeps overwrite A)
    auto lam = [&](int i, int j) -> double {
        if constexpr (MASK) { if (s_fz[i] || s_fz[j]) return 0.0; }
        if (prm.pose_only) {
            double v = G0p[i * 72 + j];
            if (!weights) v = v / Mw;
            if constexpr (PRIOR) { if (pr_on) v += exb[i * xs + j]; }
            return v;
        }
        const double g0 = G0p[i * 72 + j], g1 = G1p[i * 72 + j];
        double v = w_s * g0 + w_r * g1;
        if (i >= pd && i == j) v += (double)prm.k3;
        if (i < pd && j < pd) v += (double)prm.k4 * (double)jr(i) * (double)jr(j);
        if constexpr (PRIOR) { if (pr_on) v += exb[i * xs + j]; }
        return v;
    };
    if (!prm.pose_only) {
        for (int e = tid; e < n * (n + 1); e += POST_THREADS) {
            const int i = e / (n + 1), j = e % (n + 1);
            if (j < n) {
                if (j > i) continue;
                const double v = lam(i, j);
                A[i][j] = v;
                A[j][i] = v;
            } else {
                const double g0 = G0p[i * 72 + 71], g1 = G1p[i * 72 + 71];
                double v = -(w_s * g0 + w_r * g1);
                if (i >= pd) v -= (double)prm.k3 * (double)s.code[i - pd];
                if (i < pd) v += (double)prm.k4 * (double)jr(i) * (double)res_rot;
                if constexpr (PRIOR) { if (pr_on) v += exb[i * xs + xs - 1]; }
                if constexpr (MASK) { if (s_fz[i]) v = 0.0; }
                s_c[i] = v;
            }
        }
    } else {
        for (int e = tid; e < n * (n + 1); e += POST_THREADS) {
            const int i = e / (n + 1), j = e % (n + 1);
            if (j < n) {
                if (j > i) continue;
                const double v = lam(i, j);
                A[i][j] = v;
                A[j][i] = v;
            } else {
                double v = -G0p[i * 72 + 71];
                if (!weights) v = v / Mw;
                if constexpr (PRIOR) { if (pr_on) v += exb[i * xs + xs - 1]; }
                if constexpr (MASK) { if (s_fz[i]) v = 0.0; }
                s_c[i] = v;
            }
        }
    }
    if (tid == 0) s_sing = 0;
    __syncthreads();
    if (tid < n) s_d0[tid] = A[tid][tid];
    if (level >= 2) {
        double* L = out + POST_L1;
        for (int e = tid; e < NSOLVE * NSOLVE; e += POST_THREADS) {
            const int i = e / NSOLVE, j = e % NSOLVE;
            L[e] = (i < n && j < n) ? A[i][j] : 0.0;
        }
        if (tid < NSOLVE) L[NSOLVE * NSOLVE + tid] = tid < n ? s_c[tid] : 0.0;
    }
    for (int e = tid; e < POST_L1; e += POST_THREADS) out[e] = 0.0;
    __syncthreads();
    if (prm.pose_only && tid < 36) out[tid] = A[tid / 6][tid % 6];        // info_pose = Lambda, also for a singular one
    // 2. sweeps: the code block, then the pose block
    const double tiny = 16.0 * (double)1.1920928955078125e-07f;
    bool sing = false;
#pragma unroll 1
    for (int t = 0; t < n; ++t) {
        const int k = (t < n - pd) ? pd + t : t - (n - pd);
        if (t == n - pd && !prm.pose_only) {         // the code block is swept: the pose block is the Schur complement
            if (tid < 49) out[tid] = A[tid / 7][tid % 7];
        }
        if constexpr (MASK) { if (s_fz[k]) continue; }            // uniform: not an unknown, no pivot
        if (tid < n) s_c[tid] = A[tid][k];
        __syncthreads();
        const double d = s_c[k];
        if (!(d > tiny * s_d0[k])) { sing = true; break; }          // uniform (also NaN)
        const double rd = 1.0 / d;
        for (int e = tid; e < n * n; e += POST_THREADS) {
            const int i = e / n, j = e % n;
            if (j > i) continue;
            double v;
            if (i == k && j == k) v = -rd;
            else if (j == k) v = s_c[i] * rd;
            else if (i == k) v = s_c[j] * rd;
            else v = fma(-(s_c[i] * rd), s_c[j], A[i][j]);
            A[i][j] = v;
            A[j][i] = v;
        }
        __syncthreads();
    }
    __syncthreads();
    if (sing) {
        if (!prm.pose_only && tid < 49) out[tid] = 0.0;
    } else {
        // 3. cov_pose, refined: one Newton-Schulz step of the pose columns X_p of X = -A against Lambda itself, X_p += X (E_p - Lambda X_p),
        //    with the residual accumulated in double-double (error-free product and sum, explicitly rounded operations: no contraction) --
        //    inverting the 7 x 7 Schur complement by sweeps alone loses cond(info_pose) eps, which pivoted LU does not
        __shared__ double s_R[NSOLVE][7];
        for (int e = tid; e < n * pd; e += POST_THREADS) {
            const int i = e / pd, c = e % pd;
            double hi = (i == c) ? 1.0 : 0.0, lo = 0.0;
            if constexpr (MASK) { if (s_fz[i]) hi = 0.0; }          // E_p on the live pose entries
            for (int k = 0; k < n; ++k) {
                const double l = lam(max(i, k), min(i, k)), x = -A[k][c];
                const double q = __dmul_rn(l, x), qe = __fma_rn(l, x, -q);            // l x = q + qe exactly
                const double sum = __dadd_rn(hi, -q), bb = __dadd_rn(sum, -hi);
                const double err = __dadd_rn(__dadd_rn(hi, -__dadd_rn(sum, -bb)), __dadd_rn(-q, -bb));
                hi = sum;
                lo = __dadd_rn(lo, __dadd_rn(err, -qe));
            }
            s_R[i][c] = __dadd_rn(hi, lo);
        }
        __syncthreads();
        if (tid < pd * pd && tid % pd <= tid / pd) {
            const int a = tid / pd, c = tid % pd;
            double acc = 0.0;
            for (int i = 0; i < n; ++i) acc = __fma_rn(-A[a][i], s_R[i][c], acc);
            const double v = __dadd_rn(-A[a][c], acc);
            out[49 + a * pd + c] = v;
            out[49 + c * pd + a] = v;
        }
        if (tid >= 64 && tid < 64 + n - pd) {
            double vc = -A[pd + tid - 64][pd + tid - 64];
            if constexpr (MASK) { if (s_fz[pd + tid - 64]) vc = 0.0; }
            out[98 + tid - 64] = vc;
        }
    }
    if (tid == 0) { out[162] = sing ? 2.0 : 0.0; out[163] = (double)loss; out[164] = (double)M; out[165] = (double)V; out[166] = (double)K; }
