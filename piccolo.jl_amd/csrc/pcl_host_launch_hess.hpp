// pcl_host_launch_hess.hpp -- part of piccolo_hip.hip (included there, in place): the launchers of the Hessian of the Lagrangian.  launch_hess at the end
// is the ladder; every kernel family has a launcher of its own that returns PCL_OK (launched), PCL_ENOTIMPL (declined: the ladder goes on) or an error.
#pragma once
// Hessian of the Lagrangian of a large context (pcl_kernel_pade_large_hess.hpp; option large_hess).  The plan: beside the tile (LD = n | 1) a
// unit of nc state columns and mg drives holds nc (10 + 4 mg) column blocks of LD doubles (-S, D, Z_1 .. Z_4, W twice, V twice per drive, the
// four families of accumulators) and nc (mg (m + 1) + 1) partial sums.  The widest nc that leaves room for one drive is taken (option
// cols_per_slice caps it), then the most drives per group that fit (option large_hess_drives caps them); slices and groups are evened.  One
// column and one drive always fit (n = 128, m = 24: 148,032 B).  Every split gives the same bits.
struct LargeHessPlan : LargeTile {
    int sx, nc, mg, ngrp, U;
    size_t lds;
};
static size_t large_hess_lds_bytes(const LargeTile &t, int m, int nc, int mg) {
    return (size_t)(t.fixed + (long long)t.LD * nc * (10 + 4 * mg) + (long long)nc * ((long long)mg * (m + 1) + 1)) * sizeof(double);
}
static void large_hess_plan(const pcl_ctx *ctx, int n, int cols, int m, LargeHessPlan &P) {
    static_cast<LargeTile &>(P) = large_tile(ctx->max_lds, n, m);
    const int nc_cap = ctx->opt_cols_per_slice > 0 ? (int)std::min<int64_t>(ctx->opt_cols_per_slice, cols) : cols;
    const int mg_cap = m > 0 ? (ctx->opt_large_hess_drives > 0 ? (int)std::min<int64_t>(ctx->opt_large_hess_drives, m) : m) : 0;
    const int mg_min = m > 0 ? 1 : 0;
    P.nc = 1;
    for (int nc = nc_cap; nc > 1; --nc)
        if (large_hess_lds_bytes(P, m, nc, mg_min) <= (size_t)ctx->max_lds) {
            P.nc = nc;
            break;
        }
    P.mg = mg_min;
    for (int mg = mg_cap; mg > mg_min; --mg)
        if (large_hess_lds_bytes(P, m, P.nc, mg) <= (size_t)ctx->max_lds) {
            P.mg = mg;
            break;
        }
    P.ngrp = m > 0 ? even_split(m, P.mg) : 1;  // even groups
    P.sx = even_split(cols, P.nc);             // even slices
    P.U = P.sx * P.ngrp;
    P.lds = large_hess_lds_bytes(P, m, P.nc, P.mg);
}
static int large_hess_enable(pcl_ctx *ctx) {
    if (!ctx->dlhpart) {
        ON_DEVICE(ctx);
        const long long m = ctx->desc.n_drives;
        HIP_TRY(ctx, hipMalloc((void **)&ctx->dlhpart, (size_t)ctx->desc.batch * ctx->K * ctx->cols * (m * (m + 1) + 1) * sizeof(double)));
    }
    ctx->large_hess = 1;
    return PCL_OK;
}
static int launch_pade_large_hess(pcl_ctx *ctx, const double *Z, const double *mu, double *hess) {
    if (int rc = resolve_order(ctx, nullptr, "pcl_hess")) return rc;
    KParams p;
    fill_params(ctx, p);
    fill_pade(p, ctx->desc.pade_order);
    p.Z = window_Z(ctx, Z);
    p.mu = mu;
    p.hess = hess;
    p.hpart = ctx->dlhpart;
    LargeHessPlan P;
    large_hess_plan(ctx, p.n, p.cols, p.m, P);
    if (P.lds > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "the large-generator Hessian kernel needs %zu B of LDS (> %d) for n = %d, m = %d", P.lds, ctx->max_lds, p.n, p.m);
    p.LD = P.LD;
    p.nc = P.nc;
    p.S = P.U;
    p.lds_doubles = (int)(P.lds / sizeof(double));
    const long long items = (long long)p.batch * p.K, grid = items * P.U;
    if (int rc = check_grid(ctx, grid)) return rc;
    if (int rc = set_lds_attr(ctx, (const void *)pcl_pade_large_hess_kernel, 9, P.lds)) return rc;
    hipLaunchKernelGGL(pcl_pade_large_hess_kernel, dim3((unsigned)grid), dim3((unsigned)P.threads), P.lds, ctx->stream, p, P.sx, P.mg);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(pcl_pade_large_hess_sum_kernel, dim3((unsigned)items), dim3(256), 0, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_hess_kernel = 290 + p.q;
    return PCL_OK;
}

// Hessian of the Lagrangian of a large variational context (pcl_kernel_var_large_hess.hpp; option large_var_hess).  The plan is large_hess_plan's
// with twice the column blocks -- a unit holds component 0 and the component of the running pass: nc (20 + 8 mg) blocks of LD doubles beside the
// tile -- and the same partial sums: the widest nc that leaves room for one drive (option cols_per_slice caps it), then the most drives per group
// that fit (option large_var_hess_drives caps them), slices and groups evened.  One column and one drive always fit (n = 128, m = 24: 162,480 B).
// Every split gives the same bits.
static size_t var_large_hess_lds_bytes(const LargeTile &t, int m, int nc, int mg) {
    return (size_t)(t.fixed + (long long)t.LD * nc * (20 + 8 * mg) + (long long)nc * ((long long)mg * (m + 1) + 1)) * sizeof(double);
}
static void var_large_hess_plan(const pcl_ctx *ctx, int n, int cols, int m, LargeHessPlan &P) {
    static_cast<LargeTile &>(P) = large_tile(ctx->max_lds, n, m);
    const int nc_cap = ctx->opt_cols_per_slice > 0 ? (int)std::min<int64_t>(ctx->opt_cols_per_slice, cols) : cols;
    const int mg_cap = m > 0 ? (ctx->opt_large_var_hess_drives > 0 ? (int)std::min<int64_t>(ctx->opt_large_var_hess_drives, m) : m) : 0;
    const int mg_min = m > 0 ? 1 : 0;
    P.nc = 1;
    for (int nc = nc_cap; nc > 1; --nc)
        if (var_large_hess_lds_bytes(P, m, nc, mg_min) <= (size_t)ctx->max_lds) {
            P.nc = nc;
            break;
        }
    P.mg = mg_min;
    for (int mg = mg_cap; mg > mg_min; --mg)
        if (var_large_hess_lds_bytes(P, m, P.nc, mg) <= (size_t)ctx->max_lds) {
            P.mg = mg;
            break;
        }
    P.ngrp = m > 0 ? even_split(m, P.mg) : 1;  // even groups
    P.sx = even_split(cols, P.nc);             // even slices
    P.U = P.sx * P.ngrp;
    P.lds = var_large_hess_lds_bytes(P, m, P.nc, P.mg);
}
// option large_var_hess = 1: the workspace of the partial sums and the transposed row tables of the drives and of the variation generators
// (allocated here, on first use, not by pcl_create; the tables come from the lifted host copies the order policy keeps)
static int var_large_hess_alloc(pcl_ctx *ctx, void **buf, size_t bytes, const char *what, const char *key = "large_var_hess") {
    const hipError_t e = hipMalloc(buf, std::max<size_t>(bytes, 8));
    if (e == hipSuccess) return PCL_OK;
    *buf = nullptr;
    (void)hipGetLastError();
    return fail(ctx, e == hipErrorOutOfMemory ? PCL_ENOMEM : PCL_EHIP, "%s = 1: %s (%zu B): %s", key, what, bytes, hipGetErrorString(e));
}
// The row-compressed transposes of the drives (dellt_*) and of the variation generators (dvl_gt*): the tables of both Hessian options of the
// large variational kinds, large_var_hess and large_var_exp_hess (`key`: the one being set)
static int var_large_hess_tables(pcl_ctx *ctx, const char *key) {
    if (ctx->dellt_col && ctx->dellt_val && ctx->dvl_gtcol && ctx->dvl_gtval) return PCL_OK;
    ON_DEVICE(ctx);
    const int n = ctx->n, m = ctx->desc.n_drives, v = ctx->var, nl = ctx->var_nl;
    // rows of A^T = columns of A, entries in ascending row order, zero padded to the widest
    auto rows_t = [&](int cnt, auto at, int floor_w, std::vector<int> &col, std::vector<double> &val) {
        int wd = floor_w;
        for (int t = 0; t < cnt; ++t)
            for (int i = 0; i < n; ++i) {
                int c = 0;
                for (int j = 0; j < n; ++j) c += at(t, j, i) != 0.0;
                wd = std::max(wd, c);
            }
        col.assign((size_t)cnt * n * wd, 0);
        val.assign((size_t)cnt * n * wd, 0.0);
        for (int t = 0; t < cnt; ++t)
            for (int i = 0; i < n; ++i) {
                size_t e = ((size_t)t * n + i) * wd;
                for (int j = 0; j < n; ++j)
                    if (at(t, j, i) != 0.0) col[e] = j, val[e] = at(t, j, i), ++e;
            }
        return wd;
    };
    std::vector<int> dcol, gcol;
    std::vector<double> dval, gval;
    const int etw = rows_t(m, [&](int l, int r, int c) { return ctx->hGj[(size_t)l * nl * nl + r + (size_t)nl * c]; }, m > 0 ? 1 : 0, dcol, dval);
    const int gtw = rows_t(v, [&](int b, int r, int c) { return ctx->hG0[(size_t)((b + 1) * n + r) + (size_t)nl * c]; }, 1, gcol, gval);
    struct Up {
        void **dst;
        const void *src;
        size_t bytes;
        const char *what;
    } ups[] = {{(void **)&ctx->dellt_col, dcol.data(), dcol.size() * sizeof(int), "the transposed drive rows"},
               {(void **)&ctx->dellt_val, dval.data(), dval.size() * sizeof(double), "the transposed drive rows"},
               {(void **)&ctx->dvl_gtcol, gcol.data(), gcol.size() * sizeof(int), "the transposed variation rows"},
               {(void **)&ctx->dvl_gtval, gval.data(), gval.size() * sizeof(double), "the transposed variation rows"}};
    for (const Up &u : ups) {
        if (*u.dst) continue;
        TRY(var_large_hess_alloc(ctx, u.dst, u.bytes, u.what, key));
        if (u.bytes) HIP_TRY(ctx, hipMemcpy(*u.dst, u.src, u.bytes, hipMemcpyHostToDevice));
    }
    ctx->vl_etw = etw;
    ctx->vl_gtw = gtw;
    return PCL_OK;
}
static int var_large_hess_enable(pcl_ctx *ctx) {
    TRY(var_large_hess_tables(ctx, "large_var_hess"));
    if (!ctx->dlhpart) {
        ON_DEVICE(ctx);
        const size_t m = ctx->desc.n_drives;
        TRY(var_large_hess_alloc(ctx, (void **)&ctx->dlhpart, (size_t)ctx->K * ctx->cols * (m * (m + 1) + 1) * sizeof(double), "the workspace of the partial sums"));
    }
    return PCL_OK;
}
static int launch_var_large_hess(pcl_ctx *ctx, const double *Z, const double *mu, double *hess) {
    if (ctx->desc.pade_order == 0)
        return fail(ctx, PCL_EINVAL, "pcl_hess: the context was created with pade_order = 0; call pcl_set_order_policy (or a host-pointer entry point) first");
    if (!ctx->large_var_hess || !ctx->dlhpart) return fail(ctx, PCL_EINVAL, "pcl_hess: option large_var_hess is off");
    const pcl_desc &D = ctx->desc;
    const int n = ctx->n, m = D.n_drives, v = ctx->var;
    LargeHessPlan P;
    var_large_hess_plan(ctx, n, ctx->cols, m, P);
    if (P.lds > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "the large variational Hessian kernel needs %zu B of LDS (> %d) for n = %d, m = %d", P.lds, ctx->max_lds, n, m);
    KParams p;
    memset(&p, 0, sizeof p);
    fill_pade(p, D.pade_order);
    p.Z = Z;
    p.mu = mu;
    p.hess = hess;
    p.hpart = ctx->dlhpart;
    p.G0 = ctx->dvar_tab;
    p.upos = ctx->dupos;
    p.ucoef = ctx->ducoef;
    p.n_upos = ctx->n_upos;
    p.ell_val = ctx->dell_val;
    p.ell_col = ctx->dell_col;
    p.ell_w = ctx->ell_w;
    p.ellt_val = ctx->dellt_val;
    p.ellt_col = ctx->dellt_col;
    p.ellt_w = ctx->vl_etw;
    p.x_off0 = -1;
    p.hess_per = hess_per(ctx);
    p.d = D.d;
    p.n = n;
    p.m = m;
    p.K = ctx->K;
    p.z_dim = D.z_dim;
    p.u_off = D.u_off;
    p.dt_off = D.dt_off;
    p.batch = 1;
    p.cols = ctx->cols;
    p.nc = P.nc;
    p.S = P.U;
    p.LD = P.LD;
    p.lds_doubles = (int)(P.lds / sizeof(double));
    VarLargeHessParams w;
    memset(&w, 0, sizeof w);
    w.gv_val = ctx->dvl_gval;
    w.gv_col = ctx->dvl_gcol;
    w.gv_w = ctx->vl_gw;
    w.gvt_val = ctx->dvl_gtval;
    w.gvt_col = ctx->dvl_gtcol;
    w.gvt_w = ctx->vl_gtw;
    w.v = v;
    for (int b = 0; b <= v; ++b) w.xo[b] = ctx->x_offs[b];
    w.sx = P.sx;
    w.mg = P.mg;
    const long long items = ctx->K, grid = items * P.U;
    if (int rc = check_grid(ctx, grid)) return rc;
    if (int rc = var_set_lds(ctx, (const void *)pcl_var_large_hess_kernel, P.lds)) return rc;
    hipLaunchKernelGGL(pcl_var_large_hess_kernel, dim3((unsigned)grid), dim3((unsigned)P.threads), P.lds, ctx->stream, p, w);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(pcl_pade_large_hess_sum_kernel, dim3((unsigned)items), dim3(256), 0, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_hess_kernel = 340 + p.q;  // the large variational Hessian kernel
    return PCL_OK;
}

// Hessian of the Lagrangian of a large exponential context (pcl_kernel_large_exp_hess.hpp; option large_exp_hess).  The plan, next to
// large_exp_plan (pcl_host_launch_pade.hpp): LD = n | 1, 64 threads per 16-row tile; what the tile leaves of the LDS is NB column blocks of LD
// doubles, a third of them (NBW) per rotating buffer.  A unit of nc state columns and a pair of drive groups of mg drives holds, per state column,
// W, the dW of its drives and the d2W of its pairs: Td = 1 + mg + mg (mg + 1) / 2 columns on the diagonal, To = 1 + 2 mg + mg^2 off it.  Wherever
// there is more than one group the buffer is sized by the OFF-DIAGONAL count (n = 120, 15 columns: mg = 2; mg = 3 would fit a diagonal unit and
// not an off-diagonal one); one group has its diagonal unit alone and is sized by Td; no drives: two columns ([X_k | G X_k] behind the chain).
// Among the slice widths nc <= 16 (option cols_per_slice > 0: that width, or the widest that fits) and the group sizes (option
// large_exp_hess_drives caps them; each evened over its groups) that fit, the plan with the fewest 16-column tile passes per interval is taken,
//     sx (ngrp ceil(nc Td / 16) + ngrp (ngrp - 1) / 2 ceil(nc To / 16)),
// on a tie the fewest units, then the wider slice and the larger group.  U = sx ngrp (ngrp + 1) / 2 units per interval.  The smallest unit needs
// 4 columns per buffer; n = 128 has 9, so nothing is refused for m <= 24, n <= 128.  Every split gives the same bits.
struct LargeExpHessPlan : LargeTile {
    int NBW, sx, nc, mg, ngrp, U, W;
    long long passes;
    size_t lds;
};
static void large_exp_hess_plan(const pcl_ctx *ctx, int n, int cols, int m, LargeExpHessPlan &P) {
    static_cast<LargeTile &>(P) = large_tile(ctx->max_lds, n, m);
    P.NBW = P.NB / 3;
    const int t_min = m == 0 ? 2 : (m == 1 ? 3 : 4);  // the narrowest unit: no drives | one drive | two groups of one
    const int nc_fit = std::max(1, P.NBW / t_min);
    const int nc_hi = std::min(nc_fit, ctx->opt_cols_per_slice > 0 ? (int)std::min<int64_t>(ctx->opt_cols_per_slice, cols) : std::min(cols, 16));
    const int nc_lo = ctx->opt_cols_per_slice > 0 ? nc_hi : 1;
    const int mg_cap = m > 0 ? (ctx->opt_large_exp_hess_drives > 0 ? (int)std::min<int64_t>(ctx->opt_large_exp_hess_drives, m) : m) : 0;
    long long best_p = -1, best_u = -1;
    P.sx = cols, P.nc = 1, P.mg = m > 0 ? 1 : 0, P.ngrp = std::max(m, 1), P.W = t_min;
    for (int nc0 = nc_hi; nc0 >= nc_lo; --nc0) {
        int nc = nc0;
        const int sx = even_split(cols, nc);  // even slices
        for (int mg0 = mg_cap; mg0 >= (m > 0 ? 1 : 0); --mg0) {
            int mg = mg0;
            const int ngrp = m > 0 ? even_split(m, mg) : 1;  // even groups
            const int Td = m > 0 ? 1 + mg + mg * (mg + 1) / 2 : 2, To = 1 + 2 * mg + mg * mg;
            const int W = nc * (ngrp > 1 ? To : Td);
            if (W > P.NBW) continue;
            const long long npo = (long long)ngrp * (ngrp - 1) / 2;
            const long long passes = sx * (ngrp * (long long)((nc * (m > 0 ? Td : 1) + 15) / 16) + npo * ((nc * To + 15) / 16)), units = sx * (ngrp + npo);
            if (best_p < 0 || passes < best_p || (passes == best_p && units < best_u)) best_p = passes, best_u = units, P.sx = sx, P.nc = nc, P.mg = mg, P.ngrp = ngrp, P.W = W;
            if (m == 0) break;
        }
    }
    P.passes = best_p;
    P.U = P.sx * (P.ngrp * (P.ngrp + 1) / 2);
    P.lds = (size_t)(P.fixed + 3LL * P.LD * P.W) * sizeof(double);
}
static int large_exp_hess_enable(pcl_ctx *ctx) {
    if (!ctx->dlehpart) {
        ON_DEVICE(ctx);
        const long long m = ctx->desc.n_drives;
        HIP_TRY(ctx, hipMalloc((void **)&ctx->dlehpart, (size_t)ctx->desc.batch * ctx->K * ctx->cols * ((m + 1) * (m + 2) / 2) * sizeof(double)));
    }
    ctx->large_exp_hess = 1;
    return PCL_OK;
}
static int launch_large_exp_hess(pcl_ctx *ctx, const double *Z, const double *mu, double *hess) {
    KParams p;
    fill_params(ctx, p);
    p.Z = window_Z(ctx, Z);
    p.mu = mu;
    p.hess = hess;
    p.hpart = ctx->dlehpart;
    LargeExpHessPlan P;
    large_exp_hess_plan(ctx, p.n, p.cols, p.m, P);
    if (P.lds > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "the large exponential Hessian kernel needs %zu B of LDS (> %d) for n = %d, m = %d", P.lds, ctx->max_lds, p.n, p.m);
    p.LD = P.LD;
    p.nc = P.nc;
    p.S = P.U;
    p.lds_doubles = (int)(P.lds / sizeof(double));
    const long long items = (long long)p.batch * p.K, grid = items * P.U;
    if (int rc = check_grid(ctx, grid)) return rc;
    if (int rc = set_lds_attr(ctx, (const void *)pcl_large_exp_hess_kernel, 9, P.lds)) return rc;
    hipLaunchKernelGGL(pcl_large_exp_hess_kernel, dim3((unsigned)grid), dim3((unsigned)P.threads), P.lds, ctx->stream, p, P.sx, P.mg, P.ngrp, P.W);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(pcl_large_exp_hess_sum_kernel, dim3((unsigned)items), dim3(256), 0, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_hess_kernel = 320;  // the large exponential Hessian kernel
    return PCL_OK;
}

// Hessian of the Lagrangian of a large variational exponential context (pcl_kernel_var_large_exp_hess.hpp; option large_var_exp_hess).  The plan is
// large_exp_hess_plan's on TWO-COMPONENT column counts: a unit of pass b >= 1 holds component 0 and component b, so per state column 2 Td columns on
// the diagonal (Td = 1 + mg + mg (mg + 1) / 2), 2 To off it (To = 1 + 2 mg + mg^2); wherever there is more than one group the buffer is sized by
// 2 nc To, one group by 2 nc Td, no drives by 4 nc ([X_0 | X_b | (Ghat X')_0 | (Ghat X')_b] behind the chain).  The units of pass 0 use half of
// it.  Among the slice widths nc <= 16 (option cols_per_slice > 0: that width, or the widest that fits) and the group sizes (option
// large_var_exp_hess_drives caps them; each evened over its groups) that fit, the plan with the fewest 16-column tile passes per interval and pass,
//     sx (ngrp ceil(2 nc Td / 16) + ngrp (ngrp - 1) / 2 ceil(2 nc To / 16)),
// is taken, on a tie the fewest units, then the wider slice and the larger group.  U = sx ngrp (ngrp + 1) / 2 units per interval and pass, 1 + v
// passes.  The smallest unit needs 8 columns per buffer; n = 128 has 9, so nothing is refused for m <= 24, n <= 128.  Every split gives the same bits.
static void var_large_exp_hess_plan(const pcl_ctx *ctx, int n, int cols, int m, LargeExpHessPlan &P) {
    static_cast<LargeTile &>(P) = large_tile(ctx->max_lds, n, m);
    P.NBW = P.NB / 3;
    const int t_min = m == 0 ? 2 : (m == 1 ? 3 : 4);  // per component, the narrowest unit: no drives | one drive | two groups of one
    const int nc_fit = std::max(1, P.NBW / (2 * t_min));
    const int nc_hi = std::min(nc_fit, ctx->opt_cols_per_slice > 0 ? (int)std::min<int64_t>(ctx->opt_cols_per_slice, cols) : std::min(cols, 16));
    const int nc_lo = ctx->opt_cols_per_slice > 0 ? nc_hi : 1;
    const int mg_cap = m > 0 ? (ctx->opt_large_var_exp_hess_drives > 0 ? (int)std::min<int64_t>(ctx->opt_large_var_exp_hess_drives, m) : m) : 0;
    long long best_p = -1, best_u = -1;
    P.sx = cols, P.nc = 1, P.mg = m > 0 ? 1 : 0, P.ngrp = std::max(m, 1), P.W = 2 * t_min;
    for (int nc0 = nc_hi; nc0 >= nc_lo; --nc0) {
        int nc = nc0;
        const int sx = even_split(cols, nc);  // even slices
        for (int mg0 = mg_cap; mg0 >= (m > 0 ? 1 : 0); --mg0) {
            int mg = mg0;
            const int ngrp = m > 0 ? even_split(m, mg) : 1;  // even groups
            const int Td = m > 0 ? 1 + mg + mg * (mg + 1) / 2 : 2, To = 1 + 2 * mg + mg * mg;
            const int W = 2 * nc * (ngrp > 1 ? To : Td);
            if (W > P.NBW) continue;
            const long long npo = (long long)ngrp * (ngrp - 1) / 2;
            const long long passes = sx * (ngrp * (long long)((2 * nc * (m > 0 ? Td : 1) + 15) / 16) + npo * ((2 * nc * To + 15) / 16)), units = sx * (ngrp + npo);
            if (best_p < 0 || passes < best_p || (passes == best_p && units < best_u)) best_p = passes, best_u = units, P.sx = sx, P.nc = nc, P.mg = mg, P.ngrp = ngrp, P.W = W;
            if (m == 0) break;
        }
    }
    P.passes = best_p;
    P.U = P.sx * (P.ngrp * (P.ngrp + 1) / 2);
    P.lds = (size_t)(P.fixed + 3LL * P.LD * P.W) * sizeof(double);
}
// option large_var_exp_hess = 1: the transposed row tables (those of large_var_hess) and the two workspaces, allocated here, on first use
static int var_large_exp_hess_enable(pcl_ctx *ctx) {
    TRY(var_large_hess_tables(ctx, "large_var_exp_hess"));
    ON_DEVICE(ctx);
    const size_t m = ctx->desc.n_drives, v = ctx->var, nscal = (m + 1) * (m + 2) / 2;
    if (!ctx->dvleh_part)
        TRY(var_large_hess_alloc(ctx, (void **)&ctx->dvleh_part, (size_t)ctx->K * (1 + v) * ctx->cols * nscal * sizeof(double), "the workspace of the partial sums", "large_var_exp_hess"));
    if (!ctx->dvleh_vec)
        TRY(var_large_hess_alloc(ctx, (void **)&ctx->dvleh_vec, (size_t)ctx->K * v * (m + 1) * (size_t)ctx->var_xdc * sizeof(double), "the workspace of the passes' vectors", "large_var_exp_hess"));
    return PCL_OK;
}
static int launch_var_large_exp_hess(pcl_ctx *ctx, const double *Z, const double *mu, double *hess) {
    if (!ctx->large_var_exp_hess || !ctx->dvleh_part || !ctx->dvleh_vec) return fail(ctx, PCL_EINVAL, "pcl_hess: option large_var_exp_hess is off");
    const pcl_desc &D = ctx->desc;
    const int n = ctx->n, m = D.n_drives, v = ctx->var;
    LargeExpHessPlan P;
    var_large_exp_hess_plan(ctx, n, ctx->cols, m, P);
    if (P.lds > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "the large variational exponential Hessian kernel needs %zu B of LDS (> %d) for n = %d, m = %d", P.lds, ctx->max_lds, n, m);
    KParams p;
    memset(&p, 0, sizeof p);
    p.Z = Z;
    p.mu = mu;
    p.hess = hess;
    p.hpart = ctx->dvleh_part;
    p.G0 = ctx->dvar_tab;  // (build_G as var_large_exp_launch sets it up: the drift, and the drives on the union table)
    p.upos = ctx->dupos;
    p.ucoef = ctx->ducoef;
    p.n_upos = ctx->n_upos;
    p.ell_val = ctx->dell_val;
    p.ell_col = ctx->dell_col;
    p.ell_w = ctx->ell_w;
    p.ellt_val = ctx->dellt_val;
    p.ellt_col = ctx->dellt_col;
    p.ellt_w = ctx->vl_etw;
    p.x_off0 = -1;
    p.hess_per = hess_per(ctx);
    p.d = D.d;
    p.n = n;
    p.m = m;
    p.K = ctx->K;
    p.z_dim = D.z_dim;
    p.u_off = D.u_off;
    p.dt_off = D.dt_off;
    p.batch = 1;
    p.cols = ctx->cols;
    p.nc = P.nc;
    p.S = P.U;
    p.LD = P.LD;
    p.lds_doubles = (int)(P.lds / sizeof(double));
    VarLargeExpHessParams w;
    memset(&w, 0, sizeof w);
    w.gv_val = ctx->dvl_gval;
    w.gv_col = ctx->dvl_gcol;
    w.gv_w = ctx->vl_gw;
    w.gvt_val = ctx->dvl_gtval;
    w.gvt_col = ctx->dvl_gtcol;
    w.gvt_w = ctx->vl_gtw;
    w.vpart = ctx->dvleh_vec;
    w.v = v;
    for (int b = 0; b <= v; ++b) w.xo[b] = ctx->x_offs[b];
    w.sx = P.sx;
    w.mg = P.mg;
    w.ngrp = P.ngrp;
    w.Wc = P.W;
    const long long items = ctx->K, grid = items * (1 + v) * P.U;
    if (int rc = check_grid(ctx, grid)) return rc;
    if (int rc = var_set_lds(ctx, (const void *)pcl_var_large_exp_hess_kernel, P.lds)) return rc;
    hipLaunchKernelGGL(pcl_var_large_exp_hess_kernel, dim3((unsigned)grid), dim3((unsigned)P.threads), P.lds, ctx->stream, p, w);
    HIP_TRY(ctx, hipGetLastError());
    // the sums: per interval one workgroup for the scalars and the first piece of the X_0 vectors, up to 63 more for the rest of them
    const long long vec = (long long)(m + 1) * ctx->var_xdc;
    const unsigned chunks = (unsigned)std::max<long long>(1, std::min<long long>(64, (vec + 255) / 256));
    hipLaunchKernelGGL(pcl_var_large_exp_hess_sum_kernel, dim3((unsigned)items, chunks), dim3(256), 0, ctx->stream, p, w);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_hess_kernel = 370;  // the large variational exponential Hessian kernel
    return PCL_OK;
}

// The Hessian of the Lagrangian in the exponential mode (option exp_hess; pcl_kernel_exp_hess.hpp): five rotating n x n tiles and the
// reduction words; G(u_k) takes a sixth tile where that fits.  *g_lds: whether it does.  Returns the bytes of LDS the kernel needs.
static size_t exp_hess_lds_bytes(const pcl_ctx *ctx, int *g_lds) {
    const size_t tile = (size_t)lds_ld(ctx->n) * ctx->n, five = (5 * tile + 16) * sizeof(double);
    const bool six = five + tile * sizeof(double) <= (size_t)ctx->max_lds;
    if (g_lds) *g_lds = six ? 1 : 0;
    return six ? five + tile * sizeof(double) : five;
}
static int exp_hess_fits(const pcl_ctx *ctx, const char *who) {
    const size_t lds = exp_hess_lds_bytes(ctx, nullptr);
    if (lds > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "%s: the exponential Hessian kernel needs %zu B of LDS (> %d) for n=%d: five n x n tiles of %zu B (served up to n = 62)", who, lds, ctx->max_lds,
                    ctx->n, (size_t)lds_ld(ctx->n) * ctx->n * sizeof(double));
    return PCL_OK;
}
static int launch_exp_hess(pcl_ctx *ctx, const double *Z, const double *mu, double *hess) {
    if (int rc = exp_hess_fits(ctx, "pcl_hess")) return rc;
    KParams p;
    fill_params(ctx, p);
    p.Z = window_Z(ctx, Z);
    p.mu = mu;
    p.hess = hess;
    int g_lds = 0;
    const size_t lds = exp_hess_lds_bytes(ctx, &g_lds);
    const long long items = (long long)p.batch * p.K, grid = items * std::max(p.m, 1);
    if (int rc = check_grid(ctx, grid)) return rc;
    const long long per = 2LL * p.n * p.n + 2, cap = (long long)ctx->desc.batch * ctx->K * per;
    if (int rc = grow_scratch(ctx, &ctx->exph_cap, cap, &ctx->dexph, (size_t)cap)) return rc;
    const size_t lds_prep = ((size_t)p.LD * p.n + 32 + 64 + 2 * (size_t)p.n * p.cols) * sizeof(double);  // G(u_k), the drives, the column sums, X_k and M
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)pcl_exp_hess_prep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_prep));
    hipLaunchKernelGGL(pcl_exp_hess_prep_kernel, dim3((unsigned)items), dim3(256), lds_prep, ctx->stream, p, ctx->dexph);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)pcl_exp_hess_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned threads = p.n > 32 ? 512 : 256;  // (as the Jacobian kernel: a pair of output tiles per wave)
    hipLaunchKernelGGL(pcl_exp_hess_kernel, dim3((unsigned)grid), dim3(threads), lds, ctx->stream, p, (const double *)ctx->dGjd, (const double *)ctx->dexph, g_lds);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_hess_kernel = 100;  // the exponential Hessian kernel
    return PCL_OK;
}

static size_t hess_lds_bytes(const KParams &p) {
    const size_t nscal = (size_t)(p.m + 1) * (p.m + 2) / 2;
    return ((size_t)p.LD * p.n + (6 + 3 * (size_t)p.m) * p.LD * p.nc + 8 + p.m + 5 * nscal) * sizeof(double);
}

template <int EW, bool ANTI>
static const void *hess_v2_kernel(int m) {
    switch (m) {
    case 1: return (const void *)pcl_hess_kernel_v2<EW, 1, 0, ANTI>;
    case 2: return (const void *)pcl_hess_kernel_v2<EW, 2, 0, ANTI>;
    case 3: return (const void *)pcl_hess_kernel_v2<EW, 3, 0, ANTI>;
    case 4: return (const void *)pcl_hess_kernel_v2<EW, 4, 0, ANTI>;
    case 5: return (const void *)pcl_hess_kernel_v2<EW, 5, 0, ANTI>;
    case 6: return (const void *)pcl_hess_kernel_v2<EW, 6, 0, ANTI>;
    }
    return nullptr;
}
#define PCL_HESS_EW 2
static bool hess_v2_supported(const pcl_ctx *ctx) {
    const int m = ctx->desc.n_drives;
    return !ctx->vec && m >= 1 && m <= 6 && ctx->ell_w <= PCL_HESS_EW && ctx->ellt_w <= PCL_HESS_EW;
}
static size_t hess2_lds_bytes(const KParams &p) {
    const size_t nscal = (size_t)(p.m + 1) * (p.m + 2) / 2;
    return ((size_t)p.LD * p.n + 7 * (size_t)p.LD * 16 + 4 * nscal + 4 + 2) * sizeof(double);
}

// hess_kernel 8 (auto at every order but 4): the pattern-compiled kernel with ONE WAVE PER GROUP OF STATE COLUMNS (pcl_kernel_hess_cols.hpp): every
// wave a workgroup of its own with all m + 1 chains of 32 / (m + 1) columns, the scalar entries assembled by the wave of the interval
// that arrives last
static int launch_hess_cols(pcl_ctx *ctx, KParams &p) {
    const pcl_codegen::V4Plan &v4 = *ctx->v4_plan;
    fill_pade(p, ctx->desc.pade_order);
    const long long items = (long long)p.batch * p.K;
    const int cpw = 32 / (p.m + 1), ng = (p.d + cpw - 1) / cpw;
    if (int rc = check_grid(ctx, items * ng)) return rc;
    const size_t ldsc = hess_cols_lds_bytes(p.d, p.m, p.q, pcl_codegen::v4_gather_total(v4));
    if (!ctx->v4_fhessc && ldsc <= (size_t)ctx->max_lds) {
        const std::string src = v4_hess_cols_source(v4, p.q, (int)ctx->opt_v4_variant);
        const std::string key = "hess-cols:" + std::to_string(p.q) + ":" + std::to_string(std::hash<std::string>{}(src));
        ctx->v4_fhessc = jit_compile(ctx->device, key, src, "pcl_hess_cols_kernel", true);
        if (ctx->v4_fhessc) ctx->v4_fhessp = jit_compile(ctx->device, key, src, "pcl_hess_cols_pair_kernel", true);
        if (!ctx->v4_fhessc) {
            ctx->v4_hessc_failed = 1;
            if (int rc = jit_fell_back(ctx, "Hessian of the Lagrangian (column groups)"); rc != PCL_ENOTIMPL) return rc;
        }
    }
    if (!ctx->v4_fhessc) return PCL_ENOTIMPL;
    const long long cap = (long long)ctx->desc.batch * ctx->K;
    if (int rc = grow_scratch(ctx, &ctx->hc_cap, cap, &ctx->dhcx, (size_t)cap * ng * (p.m + 1) * (p.m + 1), false, &ctx->dhcc, (size_t)cap, true)) return rc;
    const V4Tabs T = v4_tabs(ctx);
    ctx->ticket_launched = true;  // (arrival counters + exchange rows: a launch on another stream must not overlap this one)
    // Launches of several trajectories: the chain R_{q-2} .. R_1 is formed ONCE per interval by R-chain waves -- the first `intervals`
    // workgroups of the same launch (pcl_kernel_hess_cols.hpp: hc_rchain_role), lane = (half, column) -- instead of inside each of the interval's
    // column-group waves at 8 of 64 lanes: 15 % of an 8-seed launch at order 8 (profiles/r06_hess_ablations_4.log).  The tiles travel through
    // memory (written through; a counter per interval, reset by the interval's last column-group wave).  One trajectory keeps the chain inside
    // the waves (99 intervals: every wave starts at once, there is nothing to hide the chain waves behind).
    // option hess_rpre: -1 auto | 0 never | 1 R-chain waves  (the same waves as a launch of its own in front measured the same within 1 %: removed; profiles/r06_hess_rpre_*.log)
    // MEASURED (config 3, one box, alternating): 8 seeds 102-107 against 105 us at order 8, 130-134 against 136-138 at order 10; 64 seeds 630-640 against
    // 648-652 and 805-814 against 850-854 -- 3-5 %, not the 15 % the chain costs inside the waves: a chain wave is 20 k cycles of latency in a wave slot
    // and every column-group wave pays a flag and a tile round trip at its start.
    double *rpre = nullptr;
    unsigned int *rflag = nullptr;
    ctx->last_hess_rpre = 0;
    const size_t lds_r = (size_t)p.d * (p.n + 1) * sizeof(double);  // (one tile of d columns: the chain wave's exchange of the halves)
    // (auto: orders 8 and 10 -- two and three products in the chain; at order 6 the one product a wave saves is worth less than the chain waves cost:
    //  64 seeds 523 against 505 us; profiles/r06_hess_rpre_*.log)
    // (... and launches of more column-group waves than the device has wave slots -- 8 per CU: below that a launch is the latency of its waves and the
    //  chain waves only add to it: two trajectories at order 8 42.5 against 39.4 us)
    int rmode = ctx->opt_hess_rpre >= 0 ? (ctx->opt_hess_rpre ? 1 : 0) : ((items * ng > 8LL * std::max(ctx->n_cu, 1) && p.q >= 4) ? 1 : 0);
    if (p.q <= 2) rmode = 0;
    const int nx = ctx->opt_hess_xcd < 0 ? 8 : (int)std::max<int64_t>(1, ctx->opt_hess_xcd);  // (option hess_xcd: see below)
    // (with them a column-group wave holds ONE tile of the R_a -- the next pass's is copied in behind the current one's last use -- instead of q - 2:
    //  18.7 instead of 22.2 KB at config 3, order 10: eight waves per CU instead of seven)
    //  -- where all q - 2 fit without costing a wave per CU (order 8: 20.4 KB, eight either way) they are all copied in at the start: 2 % faster than tile by tile)
    const size_t lds1_ = std::max(hess_cols_lds_bytes(p.d, p.m, p.q, pcl_codegen::v4_gather_total(v4), 1), lds_r), ldsa_ = std::max(ldsc, lds_r);
    const int rt_all = std::min<size_t>(8, (size_t)ctx->max_lds / ldsa_) >= std::min<size_t>(8, (size_t)ctx->max_lds / lds1_) ? 1 : 0;
    const size_t ldsc1 = rt_all ? ldsa_ : lds1_;
    if (rmode && (ldsc1 > (size_t)ctx->max_lds || nx != 8)) rmode = 0;  // (the chain wave and its readers share an XCD's L2: blockIdx equal mod 8)
    if (rmode) {
        const size_t per_item = (size_t)(p.q - 2) * ng * hess_cols_rtile_doubles(p.d, p.m);  // [a][column group][tile as it lies in LDS]
        if (!ctx->dhcf) ctx->hcr_cap = 0;
        // (the tiles zero-filled: a group past its last column: zeros, never written -- copied along)
        if (int rc = grow_scratch(ctx, &ctx->hcr_cap, cap * (long long)per_item, &ctx->dhcr, (size_t)cap * per_item, true, &ctx->dhcf, (size_t)cap, true)) return rc;
        rpre = ctx->dhcr;
        rflag = ctx->dhcf;
        ctx->last_hess_rpre = 1;
    }
    const long long n_rblk = rflag ? (items + 7) / 8 * 8 : 0;  // (one chain wave per interval; a multiple of 8: the column-group waves keep their XCDs)
    p.n_stream = (int)n_rblk;
    void *args[] = {(void *)&p, (void *)&T.tab, (void *)&T.tab_t, (void *)&ctx->dv4_mags, (void *)&T.dcf, (void *)&ctx->dhcx, (void *)&ctx->dhcc, (void *)&rpre, (void *)&rflag, (void *)&rt_all};
    // the waves of an interval on ONE XCD (blockIdx equal mod 8: the lines their neighbouring output runs share merge in that XCD's L2);
    // option hess_xcd: -1 auto (on) | 0 blockIdx order | n: the modulus
    p.S = nx;
    const long long grid_hc = n_rblk + (nx > 1 ? ((items + nx - 1) / nx) * nx * ng : items * ng);
    if (int rc = check_grid(ctx, grid_hc)) return rc;
    // One trajectory per launch (at most n_cu / 2 intervals: every wave runs at once, the launch's time is ONE wave's latency): two waves per column
    // group -- the chain (product, gathers) in one, what a level contributes in the other, two buffers of chain slots between them.  Same values, bitwise.
    // (auto also asks that every workgroup of the launch is resident at once -- LDS decides: 47.5 KB at config 3, order 10: three per CU -- or the launch is two rounds of latencies)
    // MEASURED (config 3, one trajectory, one box, alternating; profiles/r06_hess_pair_*.log): order 4 17.6 -> 16.7 us, order 6 24.0 -> 20.4, order 8 29.1 -> 24.1,
    // order 10 36.0 -> 27.6.
    const size_t ldsp = ldsc + ((size_t)2 * (p.m + 1) * cpw * (p.n + 1) + 2) * sizeof(double);  // (HP_NBUF = 3 buffers of chain slots instead of one + the sync words)
    const bool pair = ctx->v4_fhessp && !rmode && ldsp <= (size_t)ctx->max_lds && (ctx->opt_hess_pair == 1 || (ctx->opt_hess_pair < 0 && p.q >= 2 && 2 * items <= std::max(ctx->n_cu, 1) && items * ng <= (long long)std::max(ctx->n_cu, 1) * (long long)((size_t)ctx->max_lds / ldsp)));  // (order 2: one pass with a product -- nothing to overlap: 13.4 against 13.2 us)
    ctx->last_hess_pair = pair ? 1 : 0;
    if (pair) {
        void *pargs[] = {(void *)&p, (void *)&T.tab, (void *)&T.tab_t, (void *)&ctx->dv4_mags, (void *)&T.dcf, (void *)&ctx->dhcx, (void *)&ctx->dhcc};
        HIP_TRY(ctx, hipModuleLaunchKernel(ctx->v4_fhessp, (unsigned)grid_hc, 1, 1, 128, 1, 1, (unsigned)ldsp, ctx->stream, pargs, nullptr));
    } else
    {
        static const size_t lds_pad = getenv("PCL_HC_LDS_PAD") ? (size_t)atol(getenv("PCL_HC_LDS_PAD")) : 0;  // (occupancy experiment: lab/probes/README.md, round 6)
        HIP_TRY(ctx, hipModuleLaunchKernel(ctx->v4_fhessc, (unsigned)grid_hc, 1, 1, 64, 1, 1, (unsigned)((rflag ? ldsc1 : ldsc) + lds_pad), ctx->stream, args, nullptr));
    }
    ctx->last_hess_kernel = 80 + p.q;
    ctx->last_hess_split = 0;
    return PCL_OK;
}

// hess_kernel 7 (auto where kernel 8 is not available): the pattern-compiled kernel on the products of fused kernel 4 -- any order,
// one workgroup of m + 1 waves per interval (column slices where the m + 3 + 2 (q - 2) tiles do not fit LDS)
static int launch_hess_sparse4(pcl_ctx *ctx, KParams &p) {
    const pcl_codegen::V4Plan &v4 = *ctx->v4_plan;
    fill_pade(p, ctx->desc.pade_order);
    // small launches (at most n_cu / 2 intervals: one trajectory): TWO workgroups per interval, each with half of the drive chains (and its
    // own copy of the W and power chains) -- one wave per SIMD, 512 registers per lane instead of 256 (no spilled values), the 28 scalar
    // entries assembled by the workgroup that arrives last (option hess_split: -1 auto | 0 | 1)
    const long long items = (long long)p.batch * p.K;
    if (items > 0x3fffffffLL) return fail(ctx, PCL_ESHAPE, "too many work items");
    const int nz = p.q > 2 ? p.q - 2 : 0;
    auto bytes_ = [&](int mh_, int nc) { return ((size_t)(mh_ + 3 + 2 * nz + (p.q == 2 ? 1 : 0) /* SH_NTILES */) * nc * (p.n + 1) + (size_t)(p.m + 1) * (p.m + 2) + 8) * sizeof(double); };
    auto cols_ = [&](int mh_) {
        int nc = p.d;
        while (nc > 1 && bytes_(mh_, nc) > (size_t)ctx->max_lds) nc = (nc + 1) / 2;
        return nc;
    };
    // ... and at every size where one workgroup's tiles need column slices and half the drive chains' do not (config 3 at order 10:
    // 15 tiles of 27 columns do not fit 160 KB, 12 do; 8 trajectories per launch 394 -> 267 us)
    const bool split = p.m >= 2 && (ctx->opt_hess_split == 1 || (ctx->opt_hess_split < 0 && (2 * items <= std::max(ctx->n_cu, 1) || (cols_(p.m) < p.d && cols_((p.m + 1) / 2) == p.d))));
    const int ns = split ? 2 : 1, mh = (p.m + ns - 1) / ns;
    auto bytes = [&](int nc) { return bytes_(mh, nc); };
    p.nc = cols_(mh);
    if (ctx->opt_cols_per_slice > 0) p.nc = (int)std::min<int64_t>(p.nc, ctx->opt_cols_per_slice);
    hipFunction_t &fh = split ? ctx->v4_fhess2 : ctx->v4_fhess;
    if (!fh) {
        const std::string src = v4_hess_source(v4, p.q, (int)ctx->opt_v4_variant, ns);
        const std::string key = "hess-sparse4:" + std::to_string(p.q) + ":" + std::to_string(ns) + ":" + std::to_string(std::hash<std::string>{}(src));
        fh = jit_compile(ctx->device, key, src, "pcl_hess_sparse4_kernel", true);
        if (!fh) {
            ctx->v4_hess_failed = 1;
            if (int rc = jit_fell_back(ctx, "Hessian of the Lagrangian"); rc != PCL_ENOTIMPL) return rc;
        }
    }
    if (fh && split)
        if (int rc = grow_scratch(ctx, &ctx->h4_cap, (long long)ctx->desc.batch * ctx->K, &ctx->dh4x, (size_t)ctx->desc.batch * ctx->K * 2 * (mh + 1) * (p.m + 2), false, &ctx->dh4c, (size_t)ctx->desc.batch * ctx->K, true)) return rc;
    if (!fh || bytes(p.nc) > (size_t)ctx->max_lds) return PCL_ENOTIMPL;
    const long long units = items * ns;
    const long long grid = balanced_grid(units, std::max(ctx->n_cu, 1), ctx->opt_grid);  // every workgroup walks the same number of (interval, drive group) units
    const V4Tabs T = v4_tabs(ctx);
    ctx->ticket_launched = true;
    void *args[] = {(void *)&p, (void *)&T.tab, (void *)&T.tab_t, (void *)&ctx->dv4_mags, (void *)&T.dcf, (void *)&ctx->dh4x, (void *)&ctx->dh4c};
    HIP_TRY(ctx, hipModuleLaunchKernel(fh, (unsigned)grid, 1, 1, 64 * (1 + mh), 1, 1, (unsigned)bytes(p.nc), ctx->stream, args, nullptr));
    ctx->last_hess_kernel = 70 + p.q;
    ctx->last_hess_split = split ? 1 : 0;
    return PCL_OK;
}

// any diagonal Pade order (and the cross-check of the order-4 kernels): the general-order kernel, correctness first
static int launch_hess_general(pcl_ctx *ctx, KParams &p) {
    const bool mf = ctx->opt_use_mfma != 0;
    fill_pade(p, ctx->desc.pade_order);
    const size_t npair = (size_t)p.m * (p.m + 1) / 2, nsc = (size_t)(p.m + 1) * (p.m + 2) / 2;
    auto bytes = [&](int nc) { return ((size_t)p.LD * p.n + (6 + 4 * (size_t)p.m + 2 * npair) * p.LD * nc + 8 + p.m + 4 * nsc) * sizeof(double); };
    p.nc = p.cols;
    while (p.nc > 1 && bytes(p.nc) > (size_t)ctx->max_lds) p.nc = (p.nc + 1) / 2;
    const size_t ldsg = bytes(p.nc);
    if (ldsg > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "general-order Hessian kernel needs %zu B of LDS (> %d) for d=%d, m=%d", ldsg, ctx->max_lds, p.d, p.m);
    const long long gridg = (long long)p.batch * p.K;
    if (int rc = check_grid(ctx, gridg)) return rc;
    auto kg = mf ? pcl_hess_general_kernel<true> : pcl_hess_general_kernel<false>;
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)kg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsg));
    hipLaunchKernelGGL(kg, dim3((unsigned)gridg), dim3(256), ldsg, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_hess_kernel = 90 + p.q;
    return PCL_OK;
}

// version 4 (default where it applies): the pattern-compiled kernel -- sparse iso generators, one state column per lane
static size_t hess_sparse_lds_bytes(const pcl_codegen::SpPlan &sp) {  // tiles (odd column stride n + 1), two copies of the sums, counters
    return ((size_t)(5 + sp.m) * (sp.n + 1) * sp.d + 2 * ((size_t)sp.m * (sp.m + 2) + 1) * 4) * sizeof(double) + 64;
}
static int launch_hess_sparse(pcl_ctx *ctx, KParams &p) {
    const pcl_codegen::SpPlan &sp = *ctx->sp_plan;
    const long long items = (long long)p.batch * p.K;
    if (int rc = check_grid(ctx, items)) return rc;
    const size_t ldsp = hess_sparse_lds_bytes(sp);
    if (!ctx->sp_fhess && ldsp <= (size_t)ctx->max_lds) {  // (the source is generated once per context)
        const std::string src = sparse_source(sp);
        const std::string key = "sparse:" + std::to_string(std::hash<std::string>{}(src));
        ctx->sp_fhess = jit_compile(ctx->device, key, src, "pcl_hess_sparse_kernel", true);
        if (ctx->sp_fhess) ctx->sp_fval = jit_compile(ctx->device, key, src, "pcl_sparse_values_kernel", true);
    }
    hipFunction_t fval = ctx->sp_fval, fmain = ctx->sp_fhess;
    if (fmain && fval) {
        if (int rc = grow_scratch(ctx, &ctx->sp_gvals_cap, (long long)ctx->desc.batch * p.K, &ctx->dsp_gvals, (size_t)ctx->desc.batch * p.K * sp.nzp + 32)) return rc;
        {
            void *args[] = {(void *)&p, (void *)&ctx->dsp_pos, (void *)&ctx->dsp_coef, (void *)&ctx->dsp_gvals};
            HIP_TRY(ctx, hipModuleLaunchKernel(fval, (unsigned)items, 1, 1, 256, 1, 1, 0, ctx->stream, args, nullptr));
        }
        const long long grid = balanced_grid(items, std::max(ctx->n_cu, 1), ctx->opt_grid);  // every workgroup walks the same number of intervals
        void *args[] = {(void *)&p, (void *)&ctx->dsp_gvals, (void *)&ctx->dsp_glv};
        HIP_TRY(ctx, hipModuleLaunchKernel(fmain, (unsigned)grid, 1, 1, 64 * (sp.m + 2), 1, 1, (unsigned)ldsp, ctx->stream, args, nullptr));
        ctx->last_hess_kernel = 6;  // the pattern-compiled kernel
        return PCL_OK;
    }
    if (ldsp > (size_t)ctx->max_lds)
        ctx->sp_hess_unfit = 1;  // (the residual kernel of the same source needs one tile per wave and stays available)
    else {
        ctx->sp_failed = 1;
        if (int rc = jit_fell_back(ctx, "Hessian of the Lagrangian (order 4)"); rc != PCL_ENOTIMPL) return rc;
    }
    return PCL_ENOTIMPL;
}

// version 3 (default where its tiles fit LDS): one workgroup per interval, jobs split by drive
static size_t hess3_lds_bytes(const KParams &p) {
    const size_t lde = (p.d & 1) ? (size_t)p.n : (size_t)p.LD;
    const size_t nsc = (size_t)(p.m + 1) * (p.m + 2) / 2;
    return (lde * p.n + (8 + 2 * (size_t)p.m) * lde * 16 + 2 * (size_t)(p.m + 1) + 8 * nsc + 8) * sizeof(double) + 64;
}
static int launch_hess_v3(pcl_ctx *ctx, KParams &p) {
    const size_t lds3 = hess3_lds_bytes(p);
    const bool st27 = ctx->opt_specialize && ctx->drives_antisym && p.d == 27 && p.m == 6;
    const bool st25 = ctx->opt_specialize && ctx->drives_antisym && p.d == 25 && p.m == 4;
    if (lds3 > (size_t)ctx->max_lds) return PCL_ENOTIMPL;
    const void *k3 = st27 ? (const void *)pcl_hess_kernel_v3<PCL_HESS_EW, 6, 27, true>
                   : st25 ? (const void *)pcl_hess_kernel_v3<PCL_HESS_EW, 4, 25, true> : nullptr;
    hipFunction_t j3 = nullptr;
    if (!k3 && ctx->opt_jit && ctx->opt_specialize) {  // any other shape: compiled on first use
        char inst[96];
        snprintf(inst, sizeof inst, "pcl_hess_kernel_v3<%d, %d, %d, %s>", PCL_HESS_EW, p.m, p.d, ctx->drives_antisym ? "true" : "false");
        j3 = jit_function(ctx->device, inst);
    }
    if (!k3 && !j3) return PCL_ENOTIMPL;
    if (k3)
        if (int rc = set_lds_attr(ctx, k3, 7, lds3)) return rc;
    const long long items = (long long)p.batch * p.K;
    if (int rc = check_grid(ctx, items)) return rc;
    const long long grid = balanced_grid(items, std::max(ctx->n_cu, 1), ctx->opt_grid);  // every workgroup walks the same number of intervals
    void *args[] = {(void *)&p};
    if (j3)
        HIP_TRY(ctx, hipModuleLaunchKernel(j3, (unsigned)grid, 1, 1, 512, 1, 1, (unsigned)lds3, ctx->stream, args, nullptr));
    else
        HIP_TRY(ctx, hipLaunchKernel(k3, dim3((unsigned)grid), dim3(512), args, lds3, ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_hess_kernel = j3 ? 5 : 4;  // 4: version 3 (static instance), 5: version 3 compiled on first use
    return PCL_OK;
}

static int launch_hess_v2(pcl_ctx *ctx, KParams &p) {
    // one chunk of 16/(m+1) columns per wave and item when the interval's columns allow it, never more than 16 per slice
    const int ncw = 16 / (p.m + 1);
    int S = (p.cols + 4 * ncw - 1) / (4 * ncw);
    if (ctx->opt_cols_per_slice > 0) S = (p.cols + (int)std::min<int64_t>(ctx->opt_cols_per_slice, 16) - 1) / (int)std::min<int64_t>(ctx->opt_cols_per_slice, 16);
    S = std::max(S, (p.cols + 15) / 16);
    p.nc = (p.cols + S - 1) / S;
    p.S = (p.cols + p.nc - 1) / p.nc;
    const long long nbk = (long long)p.batch * p.K;
    const long long nbk_all = (long long)ctx->desc.batch * p.K;  // scratch is sized for every member, whatever the window
    if (p.S > 1 && !ctx->dhcnt) HIP_TRY(ctx, hipMalloc((void **)&ctx->dhcnt, (size_t)nbk_all * sizeof(unsigned int)));
    if (p.S > 1)
        if (int rc = grow_scratch(ctx, &ctx->hpart_cap, nbk_all * p.S, &ctx->dhpart, (size_t)nbk_all * p.S * ((size_t)(p.m + 1) * (p.m + 2) / 2))) return rc;
    // arrival counters start from zero in every launch (a launch that faulted must not poison the next one)
    if (p.S > 1) HIP_TRY(ctx, hipMemsetAsync(ctx->dhcnt, 0, (size_t)nbk * sizeof(unsigned int), ctx->stream));
    p.hpart = ctx->dhpart;
    p.hcnt = ctx->dhcnt;
    const size_t lds = hess2_lds_bytes(p);
    hipFunction_t jith = nullptr;
    const bool hess_static = ctx->opt_specialize && ctx->drives_antisym && ((p.d == 27 && p.m == 6) || (p.d == 25 && p.m == 4));
    if (!hess_static && ctx->opt_jit && ctx->opt_specialize && ctx->cols == ctx->desc.d && ctx->ell_w >= 1 && p.d >= 12) {  // small d: launch-bound either way
        char inst[96];
        snprintf(inst, sizeof inst, "pcl_hess_kernel_v2<%d, %d, %d, %s>", PCL_HESS_EW, p.m, p.d, ctx->drives_antisym ? "true" : "false");
        jith = jit_function(ctx->device, inst);
    }
    const void *kern = ctx->drives_antisym ? hess_v2_kernel<PCL_HESS_EW, true>(p.m) : hess_v2_kernel<PCL_HESS_EW, false>(p.m);
    if (ctx->opt_specialize && p.d == 27 && p.m == 6 && ctx->drives_antisym)
        kern = (const void *)pcl_hess_kernel_v2<PCL_HESS_EW, 6, 27, true>;  // BASELINE config 3's shape
    else if (ctx->opt_specialize && p.d == 25 && p.m == 4 && ctx->drives_antisym)
        kern = (const void *)pcl_hess_kernel_v2<PCL_HESS_EW, 4, 25, true>;  // two 5-level transmons
    if (!jith)
        if (int rc = set_lds_attr(ctx, kern, 7, lds)) return rc;
    const long long items = nbk * p.S;
    const int per_cu = std::max(1, std::min(2, (int)((size_t)ctx->max_lds / lds)));
    long long grid = std::min<long long>(items, (long long)per_cu * ctx->n_cu);
    if (ctx->opt_grid > 0) grid = std::min<long long>(items, ctx->opt_grid);
    void *args[] = {(void *)&p};
    if (jith)
        HIP_TRY(ctx, hipModuleLaunchKernel(jith, (unsigned)grid, 1, 1, 256, 1, 1, (unsigned)lds, ctx->stream, args, nullptr));
    else
        HIP_TRY(ctx, hipLaunchKernel(kern, dim3((unsigned)grid), dim3(256), args, lds, ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_hess_kernel = jith ? 3 : 2;
    return PCL_OK;
}

static int launch_hess_v1(pcl_ctx *ctx, KParams &p) {
    const bool mf = ctx->opt_use_mfma != 0;
    // column chunk: as many columns as fit in half the LDS (two workgroups per CU)
    p.nc = p.cols;
    while (p.nc > 1 && hess_lds_bytes(p) > (size_t)ctx->max_lds / 2) p.nc = (p.nc + 1) / 2;
    const size_t lds = hess_lds_bytes(p);
    if (lds > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "Hessian kernel needs %zu B of LDS (> %d) for d=%d, m=%d", lds, ctx->max_lds, p.d, p.m);
    const long long grid = (long long)p.batch * p.K;
    auto kern = mf ? pcl_hess_kernel<true> : pcl_hess_kernel<false>;
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_hess_kernel = 1;
    return PCL_OK;
}

static int launch_hess(pcl_ctx *ctx, const double *Z, const double *mu, double *hess) {
    ON_DEVICE(ctx);
    if (int rc = check_device_error(ctx, "pcl_hess")) return rc;
    TRY(require(ctx, FEAT_HESS, "pcl_hess"));
    if (ctx->large_var_exp) return launch_var_large_exp_hess(ctx, Z, mu, hess);
    if (ctx->large_var) return launch_var_large_hess(ctx, Z, mu, hess);
    if (ctx->large_exp) return launch_large_exp_hess(ctx, Z, mu, hess);
    if (ctx->large) return launch_pade_large_hess(ctx, Z, mu, hess);
    if (ctx->exp) return launch_exp_hess(ctx, Z, mu, hess);
    if (ctx->vexp) return var_exp_launch_hess(ctx, Z, mu, hess);
    if (ctx->var) return var_launch_hess(ctx, Z, mu, hess);
    if (int rc = resolve_order(ctx, nullptr, "pcl_hess")) return rc;
    KParams p;
    fill_params(ctx, p);
    p.Z = window_Z(ctx, Z);
    p.mu = mu;
    p.hess = hess;
    const bool mf = ctx->opt_use_mfma != 0;
    // (order 4: the tuned kernel 6 below stays ahead from two trajectories per launch on -- 22.6 against 23.8 us, 56 against 60 at eight; one
    //  trajectory, i.e. at most n_cu / 2 intervals: 18.4 against 20.0 us -- kernel 6 needs its value-table launch first)
    const bool cols_auto = ctx->opt_hess_kernel == 0 && !ctx->opt_general &&
                           (ctx->desc.pade_order != 4 || 2LL * p.batch * p.K <= std::max(ctx->n_cu, 1));
    const bool cols_ok = v4_available(ctx) && ctx->v4_plan->mags.size() <= (size_t)pcl_codegen::kHcMaxMags;  // (8 magnitudes: kernel 7 takes them)
    if ((ctx->opt_hess_kernel == 8 || cols_auto) && cols_ok && !ctx->v4_hessc_failed && p.m >= 1) {
        if (int rc = launch_hess_cols(ctx, p); rc != PCL_ENOTIMPL) return rc;
        if (ctx->opt_hess_kernel == 8) return fail(ctx, PCL_ESHAPE, "hess_kernel=8: the column-group kernel is not available (%s)", g_jit_note.c_str());
    } else if (ctx->opt_hess_kernel == 8) {
        return fail(ctx, PCL_ESHAPE, "hess_kernel=8 needs sparse exact-iso generators of a unitary problem (9 <= d <= 32), 1..6 drives, at most %d distinct drive magnitudes and jit=1",
                    pcl_codegen::kHcMaxMags);
    }
    if ((ctx->opt_hess_kernel == 7 || (ctx->opt_hess_kernel == 0 && ctx->desc.pade_order != 4 && !ctx->opt_general)) && v4_available(ctx) && !ctx->v4_hess_failed) {
        if (int rc = launch_hess_sparse4(ctx, p); rc != PCL_ENOTIMPL) return rc;
        if (ctx->opt_hess_kernel == 7) return fail(ctx, PCL_ESHAPE, "hess_kernel=7: the pattern-compiled general-order kernel is not available (%s)", g_jit_note.c_str());
    } else if (ctx->opt_hess_kernel == 7) {
        return fail(ctx, PCL_ESHAPE, "hess_kernel=7 needs sparse exact-iso generators of a unitary problem (9 <= d <= 32), 1..6 drives and jit=1");
    }
    if (ctx->desc.pade_order != 4 || ctx->opt_general) return launch_hess_general(ctx, p);
    if ((ctx->opt_hess_kernel == 0 || ctx->opt_hess_kernel == 4) && ctx->sp_plan && !ctx->sp_failed && !ctx->sp_hess_unfit && ctx->opt_jit && ctx->desc.d == p.d) {
        if (int rc = launch_hess_sparse(ctx, p); rc != PCL_ENOTIMPL) return rc;
        if (ctx->opt_hess_kernel == 4)
            return fail(ctx, PCL_ESHAPE, "hess_kernel=4: the pattern-compiled kernel is not available (%zu B of LDS needed, %d available; %s)", hess_sparse_lds_bytes(*ctx->sp_plan), ctx->max_lds,
                        g_jit_note.c_str());
    } else if (ctx->opt_hess_kernel == 4) {
        return fail(ctx, PCL_ESHAPE, "hess_kernel=4 needs sparse iso generators (at most %d distinct drive magnitudes), a unitary problem with 9 <= d <= 32, 1..6 drives and jit=1", pcl_codegen::kMaxMags);
    }
    if (mf && (ctx->opt_hess_kernel == 0 || ctx->opt_hess_kernel == 3) && hess_v2_supported(ctx) && ctx->cols == ctx->desc.d && ctx->uell_w <= 2 &&
        ctx->n_upos <= 512 * PCL_NUE_H3 && (ctx->opt_hess_kernel == 3 || ctx->desc.d >= 12)) {
        if (int rc = launch_hess_v3(ctx, p); rc != PCL_ENOTIMPL) return rc;
        if (ctx->opt_hess_kernel == 3) return fail(ctx, PCL_ESHAPE, "hess_kernel=3: no instance for this shape (tiles need %zu B of LDS, jit=%d)", hess3_lds_bytes(p), (int)ctx->opt_jit);
    }
    if (ctx->opt_hess_kernel == 2 && !hess_v2_supported(ctx))
        return fail(ctx, PCL_ESHAPE, "hess_kernel=2 needs 1..6 drives with at most %d entries per row and column (have m=%d, widths %d/%d)",
                    PCL_HESS_EW, p.m, ctx->ell_w, ctx->ellt_w);
    if (mf && ctx->opt_hess_kernel != 1 && hess_v2_supported(ctx) && hess2_lds_bytes(p) <= (size_t)ctx->max_lds) return launch_hess_v2(ctx, p);
    return launch_hess_v1(ctx, p);
}
