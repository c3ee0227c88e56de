// pcl_host_robust.hpp -- part of piccolo_hip.hip (included there, in place, after pcl_host_objective.hpp): what a variational context serves once
// its option var_full is on -- the robust-control objective (terminal infidelity of the state, UnitarySensitivityObjective of the variations at
// the terminal knot, regularisers on any component), its Hessian, and the rollout of the stacked state.  The entry points are the plain
// contexts' (no new export); they hand over here behind require(ctx, FEAT_OBJECTIVE).
#pragma once
static_assert(PCL_VAROBJ_MAXC == PCL_VAR_MAXV + 1, "components of a variational knot");

// drop goal, weights and regularisers (option var_full back to 0)
static void var_drop_objective(pcl_ctx *ctx) {
    for (double **q : {&ctx->dformA, &ctx->dformc, &ctx->dgram, &ctx->dcoef}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    ctx->form_R = ctx->form_L = 0;
    ctx->gram_ready = false;
    ctx->form_user = false;
    ctx->var_w.assign((size_t)ctx->var + 1, 0.0);
    ctx->var_w[0] = 1.0;
    ctx->regs.clear();
    ctx->reg_R.clear();
    ctx->regs_dirty = true;
}
static int var_set_full(pcl_ctx *ctx, int64_t on) {
    if ((int)on == ctx->var_full) return PCL_OK;  // (set_gate has checked the value and the kind of context)
    ON_DEVICE(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (on && !ctx->dvar_coef) HIP_TRY(ctx, hipMalloc((void **)&ctx->dvar_coef, (size_t)(ctx->var + 1) * sizeof(double)));
    var_drop_objective(ctx);
    ctx->var_full = (int)on;
    return PCL_OK;
}
// a device array of this family whose allocation may fail for its size (a triangle at d = 64 is 268 MB): PCL_ENOMEM, the pointer stays NULL, the
// sticky HIP error is cleared and the context goes on as before
static int var_alloc(pcl_ctx *ctx, void **buf, size_t bytes, const char *what) {
    const hipError_t e = hipMalloc(buf, bytes);
    if (e == hipSuccess) return PCL_OK;
    *buf = nullptr;
    (void)hipGetLastError();
    return fail(ctx, e == hipErrorOutOfMemory ? PCL_ENOMEM : PCL_EHIP, "%s (%zu B): %s", what, bytes, hipGetErrorString(e));
}
// option large_var_full (large variational contexts): what var_set_full does for var_full
static int var_large_set_full(pcl_ctx *ctx, int64_t on) {
    if ((int)on == ctx->large_var_full) return PCL_OK;  // (set_gate has checked the value and the kind of context)
    ON_DEVICE(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (on && !ctx->dvar_coef) TRY(var_alloc(ctx, (void **)&ctx->dvar_coef, (size_t)(ctx->var + 1) * sizeof(double), "large_var_full = 1: the coefficient buffer"));
    var_drop_objective(ctx);
    ctx->large_var_full = (int)on;
    return PCL_OK;
}
static bool var_unitary(const pcl_ctx *ctx) { return ctx->cols == ctx->desc.d; }
static bool var_has_goal(const pcl_ctx *ctx) { return ctx->dformA || ctx->dformc; }
static bool var_has_sens(const pcl_ctx *ctx) {
    for (int i = 1; i <= ctx->var; ++i)
        if (ctx->var_w[i] != 0.0) return true;
    return false;
}

static int var_set_goal(pcl_ctx *ctx, const double *goal_iso_vec) {
    if (!goal_iso_vec) return fail(ctx, PCL_EINVAL, "pcl_set_goal: NULL");
    if (!var_unitary(ctx)) return fail(ctx, PCL_ENOTIMPL, "pcl_set_goal: unitary (n x d) states only; a ket context takes pcl_set_goal_form");
    ON_DEVICE(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return unitary_form(ctx, goal_iso_vec);
}
static int var_set_goal_subspace(pcl_ctx *ctx, const double *goal_sub_iso_vec, const int32_t *subspace, int32_t ns) {
    if (!goal_sub_iso_vec || !subspace) return fail(ctx, PCL_EINVAL, "pcl_set_goal_subspace: NULL");
    if (!var_unitary(ctx)) return fail(ctx, PCL_ENOTIMPL, "pcl_set_goal_subspace: unitary (n x d) states only");
    if (ns < 1 || ns > ctx->desc.d) return fail(ctx, PCL_EINVAL, "pcl_set_goal_subspace: ns=%d outside 1..d=%d", ns, ctx->desc.d);
    for (int i = 0; i < ns; ++i) {
        if (subspace[i] < 0 || subspace[i] >= ctx->desc.d) return fail(ctx, PCL_EINVAL, "pcl_set_goal_subspace: index %d outside 0..d-1", subspace[i]);
        for (int j = 0; j < i; ++j)
            if (subspace[j] == subspace[i]) return fail(ctx, PCL_EINVAL, "pcl_set_goal_subspace: index %d repeated", subspace[i]);
    }
    // (a large variational context, d up to 64: the size no subspace of d <= 32 reaches; refused here, before anything is replaced.  No kernel of
    // this path stages the subspace in LDS, so the rows of the form are the only limit)
    if (ctx->large_var && 2 * ns * ns + 2 > PCL_FORM_MAX_ROWS)
        return fail(ctx, PCL_ESHAPE, "pcl_set_goal_subspace: a subspace of %d levels needs %d rows of the terminal form (2 ns^2 + 2), %d are available: 45 levels at most", ns, 2 * ns * ns + 2, PCL_FORM_MAX_ROWS);
    ON_DEVICE(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return subspace_form(ctx, goal_sub_iso_vec, subspace, ns);
}
// the loss of component 0 in the general form: R rows of x_dim(component) doubles
static int var_set_goal_form(pcl_ctx *ctx, int32_t scope, int32_t R, const double *A, const double *c) {
    if (scope == 1) return fail(ctx, PCL_ENOTIMPL, "pcl_set_goal_form: scope 1 (a joint term) is not implemented for a variational context; scope 0 is the loss of component 0");
    if (scope != 0) return fail(ctx, PCL_EINVAL, "pcl_set_goal_form: scope must be 0 on a variational context");
    if (R > 4096) return fail(ctx, PCL_ESHAPE, "pcl_set_goal_form: at most 4096 rows");
    ON_DEVICE(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return set_form(ctx, 0, R, A, c, true);
}
static int var_set_weights(pcl_ctx *ctx, const double *w) {
    const int v = ctx->var;
    if (w) {
        for (int i = 0; i <= v; ++i)
            if (!std::isfinite(w[i]) || w[i] < 0.0) return fail(ctx, PCL_EINVAL, "pcl_set_weights: w[%d]=%g; weights are finite and >= 0", i, w[i]);
        if (!var_unitary(ctx))
            for (int i = 1; i <= v; ++i)
                if (w[i] != 0.0)
                    return fail(ctx, PCL_ENOTIMPL, "pcl_set_weights: w[%d]=%g on a ket context; the sensitivity objective is defined for unitaries only", i, w[i]);
    }
    ctx->var_w.assign((size_t)v + 1, 0.0);
    ctx->var_w[0] = 1.0;  // NULL: [1, 0, .., 0]
    if (w) ctx->var_w.assign(w, w + v + 1);
    return PCL_OK;
}

static void var_obj_fill(const pcl_ctx *ctx, PclVarObj &a, const double *Z, double Q) {
    memset(&a, 0, sizeof a);
    const pcl_desc &D = ctx->desc;
    a.Z = Z;
    a.regs = (const PclReg *)ctx->dregs;
    a.Rv = ctx->dreg_R;
    a.n_regs = (int)ctx->regs.size();
    a.member = ctx->dobj;
    a.regval = ctx->dobj + D.batch;
    a.ticket = reinterpret_cast<unsigned int *>(ctx->dobj + D.batch + D.N);
    a.coef = ctx->dvar_coef;
    a.f = PclForm{ctx->dformA, ctx->dformc, ctx->form_R, (int)ctx->var_xdc, 0};
    for (int i = 0; i <= ctx->var; ++i) a.w[i] = ctx->var_w[i], a.xo[i] = ctx->x_offs[i];
    a.v = ctx->var;
    a.d = D.d;
    a.N = D.N;
    a.z_dim = D.z_dim;
    a.dt_off = D.dt_off;
    a.Q = Q;
    a.sigma = 1.0;
}
static int var_objective_dev(pcl_ctx *ctx, const double *Z, double Q, double *value, double *grad) {
    if (!Z || !value) return fail(ctx, PCL_EINVAL, "pcl_objective_dev: NULL pointer");
    if (!var_has_goal(ctx) && !var_has_sens(ctx) && ctx->regs.empty())
        return fail(ctx, PCL_EINVAL, "pcl_objective_dev: no goal, no sensitivity weight and no regulariser set");
    ON_DEVICE(ctx);
    TRY(objective_prepare(ctx));
    PclVarObj a;
    var_obj_fill(ctx, a, Z, Q);
    a.grad = grad;
    a.value = value;
    // ONE launch, with or without a gradient buffer: the regulariser rows and the terminal knot as workgroups of one grid
    hipLaunchKernelGGL(pcl_var_objective_kernel, dim3((unsigned)ctx->desc.N), dim3(256), (size_t)std::max(ctx->form_R, 1) * sizeof(double), ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_objective_launches = 1;
    return PCL_OK;
}

// values: [Gram triangle of component 0 (a goal with quadratic rows)] [per variation with w_i != 0: the dense lower triangle over its terminal
// iso-vec, row-major (i, j <= i)] [per knot, regulariser: as on a plain context]
static long long var_tri(const pcl_ctx *ctx) { return ctx->var_xdc * (ctx->var_xdc + 1) / 2; }
static long long var_hess_goal(const pcl_ctx *ctx) { return var_has_goal(ctx) && ctx->form_R > 0 ? var_tri(ctx) : 0; }
// Each position once: where a regulariser covers entries of a component that has a triangle, the terminal knot's diagonal entries of that
// regulariser are the triangle's (pcl_tri_diag_add_kernel) and leave the knot's block.  The plan: the components with a triangle, the kept slots
// of the terminal knot's block, and per triangle and dt_power the summed R of what it absorbs.
struct VarHessPlan {
    std::vector<int> tri;       // components with a triangle, in emission order
    std::vector<int> last_src;  // slots of the full per-knot block the terminal knot keeps
    std::vector<double> diag;   // [tri][3][L]
    bool absorbs = false;
};
static VarHessPlan var_hess_plan(const pcl_ctx *ctx) {
    VarHessPlan P;
    const long long L = ctx->var_xdc;
    if (var_hess_goal(ctx)) P.tri.push_back(0);
    for (int i = 1; i <= ctx->var; ++i)
        if (ctx->var_w[i] != 0.0) P.tri.push_back(i);
    P.diag.assign(P.tri.size() * 3 * (size_t)L, 0.0);
    int slot = 0;
    for (const PclReg &r : ctx->regs) {
        for (int i = 0; i < r.dim; ++i, ++slot) {
            const long long z = r.off + i;
            bool taken = false;
            for (size_t t = 0; t < P.tri.size() && !taken; ++t) {
                const long long x0 = ctx->x_offs[P.tri[t]];
                if (z >= x0 && z < x0 + L) {
                    P.diag[(t * 3 + r.pw) * (size_t)L + (z - x0)] += ctx->reg_R[r.r0 + i];
                    taken = true;
                }
            }
            if (taken)
                P.absorbs = true;
            else
                P.last_src.push_back(slot);
        }
        const int rest = (r.pw >= 1 ? r.dim : 0) + (r.pw == 2 ? 1 : 0);
        for (int i = 0; i < rest; ++i, ++slot) P.last_src.push_back(slot);
    }
    return P;
}
static int var_objective_hess_nnz(const pcl_ctx *ctx, int64_t *nnz) {
    if (!nnz) return PCL_EINVAL;
    const VarHessPlan P = var_hess_plan(ctx);
    *nnz = (long long)P.tri.size() * var_tri(ctx) + (long long)(ctx->desc.N - 1) * obj_hess_per_knot(ctx) + (long long)P.last_src.size();
    return PCL_OK;
}
static int var_objective_hess_structure(const pcl_ctx *ctx, int64_t *rows, int64_t *cols) {
    if (!rows || !cols) return PCL_EINVAL;
    const pcl_desc &D = ctx->desc;
    const long long base = D.index_base, zN = (long long)(D.N - 1) * D.z_dim, L = ctx->var_xdc;
    const VarHessPlan P = var_hess_plan(ctx);
    long long e = 0;
    auto put = [&](long long a, long long b) {
        rows[e] = std::max(a, b) + base;
        cols[e] = std::min(a, b) + base;
        ++e;
    };
    for (int b : P.tri) {
        const long long x0 = zN + ctx->x_offs[b];
        for (long long i = 0; i < L; ++i)
            for (long long j = 0; j <= i; ++j) put(x0 + i, x0 + j);
    }
    std::vector<std::pair<long long, long long>> knot;  // the full block of one knot, relative to the knot
    for (const PclReg &r : ctx->regs) {
        for (int i = 0; i < r.dim; ++i) knot.emplace_back(r.off + i, r.off + i);
        if (r.pw >= 1)
            for (int i = 0; i < r.dim; ++i) knot.emplace_back(D.dt_off, r.off + i);
        if (r.pw == 2) knot.emplace_back(D.dt_off, D.dt_off);
    }
    for (int k = 0; k < D.N - 1; ++k)
        for (const auto &q : knot) put((long long)k * D.z_dim + q.first, (long long)k * D.z_dim + q.second);
    for (int s : P.last_src) put(zN + knot[s].first, zN + knot[s].second);
    return PCL_OK;
}
static int var_objective_hess_dev(pcl_ctx *ctx, const double *Z, double Q, double sigma, double *vals) {
    if (!Z || !vals) return fail(ctx, PCL_EINVAL, "pcl_objective_hess_dev: NULL pointer");
    ON_DEVICE(ctx);
    const pcl_desc &D = ctx->desc;
    const long long nT = var_tri(ctx), L = ctx->var_xdc;
    const VarHessPlan P = var_hess_plan(ctx);
    const double *zN = Z + (long long)(D.N - 1) * D.z_dim;
    if (P.absorbs && (P.last_src != ctx->var_last_src || P.diag != ctx->var_diag || !ctx->dvar_diag)) {  // (re)upload the plan; rare
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (void **q : {(void **)&ctx->dvar_last_src, (void **)&ctx->dvar_diag}) {
            if (*q) (void)hipFree(*q);
            *q = nullptr;
        }
        ctx->var_last_src.clear();
        ctx->var_diag.clear();
        TRY(var_alloc(ctx, (void **)&ctx->dvar_last_src, std::max<size_t>(P.last_src.size(), 1) * sizeof(int), "pcl_objective_hess_dev: the kept slots of the terminal knot"));
        TRY(var_alloc(ctx, (void **)&ctx->dvar_diag, P.diag.size() * sizeof(double), "pcl_objective_hess_dev: the absorbed diagonals"));
        HIP_TRY(ctx, hipMemcpy(ctx->dvar_last_src, P.last_src.data(), P.last_src.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->dvar_diag, P.diag.data(), P.diag.size() * sizeof(double), hipMemcpyHostToDevice));
        ctx->var_last_src = P.last_src;
        ctx->var_diag = P.diag;
    }
    double *out = vals;
    if (!P.tri.empty()) {  // the coefficients, once: -s w_0 Q sigma and |x_i,N|^2
        PclVarObj a;
        var_obj_fill(ctx, a, Z, Q);
        a.sigma = sigma;
        a.mode = 1;
        hipLaunchKernelGGL(pcl_var_objective_kernel, dim3(1), dim3(256), (size_t)std::max(ctx->form_R, 1) * sizeof(double), ctx->stream, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    for (size_t t = 0; t < P.tri.size(); ++t, out += nT) {
        const int b = P.tri[t];
        if (b == 0) {
            if (!ctx->gram_ready) {  // T = 2 sum_r A_r A_r', once per goal
                const PclForm f{ctx->dformA, ctx->dformc, ctx->form_R, (int)L, 0};
                if (!ctx->dgram) TRY(var_alloc(ctx, (void **)&ctx->dgram, (size_t)nT * sizeof(double), "pcl_objective_hess_dev: the Gram triangle"));
                hipLaunchKernelGGL(pcl_gram_kernel, dim3((unsigned)std::min<long long>((nT + 255) / 256, 4096)), dim3(256), 0, ctx->stream, f, ctx->dgram);
                HIP_TRY(ctx, hipGetLastError());
                ctx->gram_ready = true;
            }
            hipLaunchKernelGGL(pcl_scale_kernel, dim3((unsigned)std::min<long long>((nT + 255) / 256, 8192)), dim3(256), 0, ctx->stream, (const double *)ctx->dgram,
                               (const double *)ctx->dvar_coef, nT, 1, out);
        } else {
            const double c = sigma * ctx->var_w[b] / ((double)D.d * D.d);
            const long long pairs = (nT + 1) / 2;
            // (the staged x is L doubles: 65,536 B at d = 64, where a launch has to ask for its dynamic LDS)
            if ((size_t)L * sizeof(double) >= 65536)
                HIP_TRY(ctx, hipFuncSetAttribute((const void *)pcl_sens_hess_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)L * sizeof(double))));
            hipLaunchKernelGGL(pcl_sens_hess_kernel, dim3((unsigned)std::min<long long>((pairs + 255) / 256, 2048)), dim3(256), (size_t)L * sizeof(double), ctx->stream,
                               zN + ctx->x_offs[b], (const double *)(ctx->dvar_coef + b), c, (int)L, out);
        }
        HIP_TRY(ctx, hipGetLastError());
        if (P.absorbs) {
            hipLaunchKernelGGL(pcl_tri_diag_add_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, ctx->stream, out, (const double *)(ctx->dvar_diag + t * 3 * (size_t)L),
                               zN + D.dt_off, sigma, (int)L);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    const long long pk = obj_hess_per_knot(ctx);
    if (pk) {
        TRY(objective_prepare(ctx));
        const int full = P.absorbs ? D.N - 1 : D.N;  // knots whose block is written in place
        hipLaunchKernelGGL(pcl_reg_hess_kernel, dim3((unsigned)full, 1u), dim3(256), 0, ctx->stream, Z, (const PclReg *)ctx->dregs, (int)ctx->regs.size(),
                           (const double *)ctx->dreg_R, sigma, D.N, D.z_dim, D.dt_off, 0LL, pk, out);
        HIP_TRY(ctx, hipGetLastError());
        if (P.absorbs) {  // the terminal knot: the full block into scratch, the kept slots from there
            if (ctx->var_scratch_cap < pk) {
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                if (ctx->dvar_scratch) (void)hipFree(ctx->dvar_scratch);
                ctx->dvar_scratch = nullptr;
                HIP_TRY(ctx, hipMalloc((void **)&ctx->dvar_scratch, (size_t)pk * sizeof(double)));
                ctx->var_scratch_cap = pk;
            }
            hipLaunchKernelGGL(pcl_reg_hess_kernel, dim3(1u, 1u), dim3(256), 0, ctx->stream, zN, (const PclReg *)ctx->dregs, (int)ctx->regs.size(),
                               (const double *)ctx->dreg_R, sigma, 1, D.z_dim, D.dt_off, 0LL, pk, ctx->dvar_scratch);
            HIP_TRY(ctx, hipGetLastError());
            const int cnt = (int)P.last_src.size();
            if (cnt) {
                hipLaunchKernelGGL(pcl_gather_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)ctx->dvar_scratch,
                                   (const int *)ctx->dvar_last_src, cnt, out + (long long)(D.N - 1) * pk);
                HIP_TRY(ctx, hipGetLastError());
            }
        }
    }
    return PCL_OK;
}

// --- rollout of the stacked state (pcl_kernel_var_rollout.hpp) -----------------------------------------------------------------------------
// The same on a large variational context (pcl_kernel_var_large_rollout.hpp; option large_var_full).  Beside the tile (LD = n | 1) a propagator
// workgroup holds three pairs [V | Vv] of npc columns: six blocks; a chain workgroup holds two pairs [X | Xv] of nc state columns and no tile.
// The widest panel that fits is evened over the panels; launches of few intervals take up to one panel per 16 columns while the grid of
// (1 + v) roles stays within one round of the CUs (option general_slices: that many panels per role at least).  The chain takes slices of 16
// state columns, one matrix-core column tile (option cols_per_slice: that many at most, never more than 16).  One column always fits
// (n = 128, m = 24: 139,568 B and 5,152 B).  Every split gives the same bits.
struct VarLargeRollPlan : LargeTile {
    int P, npc, S, nc;
    size_t lds_e, lds_c;
};
static void var_large_roll_plan(const pcl_ctx *ctx, int n, int cols, int m, int v, long long K, VarLargeRollPlan &R) {
    static_cast<LargeTile &>(R) = large_tile(ctx->max_lds, n, m);  // (the propagator launch's; the chain launch has the slack alone.  NB >= 0: the tile fits for n <= 128)
    const long long budget = ctx->max_lds / (long long)sizeof(double), fixed_c = PL_SLACK;
    const int npc_max = std::max(1, std::min(n, R.NB / 6));
    const int p_min = (n + npc_max - 1) / npc_max;
    const long long want = ctx->opt_general_slices > 0 ? ctx->opt_general_slices : std::min<long long>((n + 15) / 16, ctx->n_cu / std::max(K * (1 + v), 1LL));
    R.P = (int)std::max<long long>(p_min, std::min<long long>(want, n));
    R.npc = (n + R.P - 1) / R.P;
    R.P = (n + R.npc - 1) / R.npc;  // (no panel without a column)
    const int nc_fit = (int)std::max<long long>(1, (budget - fixed_c) / R.LD / 4);
    const int nc_cap = ctx->opt_cols_per_slice > 0 ? (int)std::min<int64_t>(ctx->opt_cols_per_slice, cols) : cols;
    R.nc = std::min(std::min(nc_cap, nc_fit), 16);
    R.S = (cols + R.nc - 1) / R.nc;
    R.lds_e = (size_t)(R.fixed + 6LL * R.LD * R.npc) * sizeof(double);
    R.lds_c = (size_t)(fixed_c + 4LL * R.LD * R.nc) * sizeof(double);
}
static int var_large_rollout_dev(pcl_ctx *ctx, const double *Z, double *X_out) {
    ON_DEVICE(ctx);
    const pcl_desc &D = ctx->desc;
    const int n = ctx->n, v = ctx->var, m = D.n_drives;
    const size_t ws = (size_t)ctx->K * (1 + v) * n * n * sizeof(double);  // [interval][E | L_1 .. L_v], kept until pcl_destroy
    if (!ctx->dexpm) TRY(var_alloc(ctx, (void **)&ctx->dexpm, ws, "pcl_rollout_dev: the propagator workspace"));
    VarLargeRollPlan R;
    var_large_roll_plan(ctx, n, ctx->cols, m, v, ctx->K, R);
    if (R.lds_e > (size_t)ctx->max_lds || R.lds_c > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "pcl_rollout_dev: the large variational rollout needs %zu B of LDS (> %d) for n = %d, m = %d", std::max(R.lds_e, R.lds_c), ctx->max_lds, n, m);
    const long long grid_e = (long long)ctx->K * (1 + v) * R.P, grid_c = (long long)v * R.S;
    if (grid_e > 0x7fffffffLL) return fail(ctx, PCL_ESHAPE, "pcl_rollout_dev: %lld workgroups exceed the grid limit", grid_e);
    KParams p;
    memset(&p, 0, sizeof p);
    p.Z = Z;
    p.xout = X_out;
    p.expm = ctx->dexpm;
    p.G0 = ctx->dvar_tab;  // (build_G as var_large_launch sets it up: the drift, and the drives on the union table)
    p.upos = ctx->dupos;
    p.ucoef = ctx->ducoef;
    p.n_upos = ctx->n_upos;
    p.x_off0 = -1;
    p.d = D.d;
    p.n = n;
    p.m = m;
    p.K = ctx->K;
    p.z_dim = D.z_dim;
    p.u_off = D.u_off;
    p.dt_off = D.dt_off;
    p.batch = 1;
    p.cols = ctx->cols;
    p.LD = R.LD;
    VarLargeRollParams w;
    memset(&w, 0, sizeof w);
    w.gv_val = ctx->dvl_gval;
    w.gv_col = ctx->dvl_gcol;
    w.gv_w = ctx->vl_gw;
    w.v = v;
    for (int b = 0; b <= v; ++b) w.xo[b] = ctx->x_offs[b];
    w.npc = R.npc;
    w.P = R.P;
    w.nc = R.nc;
    w.S = R.S;
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)pcl_var_large_expm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.lds_e));
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)pcl_var_large_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.lds_c));
    p.lds_doubles = (int)(R.lds_e / sizeof(double));
    hipLaunchKernelGGL(pcl_var_large_expm_kernel, dim3((unsigned)grid_e), dim3((unsigned)R.threads), R.lds_e, ctx->stream, p, w);
    HIP_TRY(ctx, hipGetLastError());
    p.lds_doubles = (int)(R.lds_c / sizeof(double));
    hipLaunchKernelGGL(pcl_var_large_chain_kernel, dim3((unsigned)grid_c), dim3((unsigned)R.threads), R.lds_c, ctx->stream, p, w);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_kernel = 360;  // the large variational family's rollout (340 + q: residual + Jacobian, 350 + q: its residual)
    ctx->last_n_stream = 0;
    return PCL_OK;
}
static int var_rollout_dev(pcl_ctx *ctx, const double *Z, double *X_out) {
    ON_DEVICE(ctx);
    const pcl_desc &D = ctx->desc;
    const int n = ctx->n, v = ctx->var, m = D.n_drives;
    const size_t nn = (size_t)n * n;
    VarRollParams p;
    memset(&p, 0, sizeof p);
    p.Z = Z;
    p.xout = X_out;
    if (!ctx->dexpm) HIP_TRY(ctx, hipMalloc((void **)&ctx->dexpm, (size_t)ctx->K * (1 + v) * nn * sizeof(double)));
    p.expm = ctx->dexpm;
    p.G0 = ctx->dvar_tab;
    p.Gj = ctx->dvar_tab + nn;
    p.Gv = ctx->dvar_tab + (1 + (size_t)m) * nn;
    p.n = n;
    p.LD = ((n + 3) & ~3) + 2;
    p.cols = ctx->cols;
    p.m = m;
    p.K = ctx->K;
    p.v = v;
    p.z_dim = D.z_dim;
    p.u_off = D.u_off;
    p.dt_off = D.dt_off;
    p.cc = std::min(16, ctx->cols);
    for (int b = 0; b <= v; ++b) p.xo[b] = ctx->x_offs[b];
    const size_t tile = (size_t)p.LD * n, extra = 32 + 64;  // the drive amplitudes and the column sums behind the tiles
    p.gv_lds = (5 * tile + extra) * sizeof(double) <= (size_t)ctx->max_lds;  // Gv_i in a tile of its own (d <= 30), else read from L2
    const size_t lds_a = ((p.gv_lds ? 5 : 4) * tile + extra) * sizeof(double);
    const size_t lds_b = (2 * tile + 5 * (size_t)p.LD * p.cc) * sizeof(double);
    if (lds_a > (size_t)ctx->max_lds || lds_b > (size_t)ctx->max_lds) return fail(ctx, PCL_ESHAPE, "pcl_rollout_dev: tiles exceed LDS");
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)pcl_var_expm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a));
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)pcl_var_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    hipLaunchKernelGGL(pcl_var_expm_kernel, dim3((unsigned)(p.K * v)), dim3(256), lds_a, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    const int nch = (p.cols + p.cc - 1) / p.cc;
    hipLaunchKernelGGL(pcl_var_chain_kernel, dim3((unsigned)(v * nch)), dim3(256), lds_b, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    return PCL_OK;
}
