// pcl_host_launch_pade.hpp -- part of piccolo_hip.hip (included there, in place): the residual and Jacobian launchers.  launch_fused at the end is the
// ladder; every kernel family has a launcher of its own that returns PCL_OK (launched), PCL_ENOTIMPL (declined: the ladder goes on) or an error.
#pragma once
static size_t fused_lds_bytes(const KParams &p, bool jac) {  // version-1 kernel
    const size_t ncols1 = jac ? (size_t)(2 + p.m) * p.nc : 2 * (size_t)p.nc;
    size_t dbl = (size_t)p.LD * p.n * (jac ? 2 : 1) + 2 * p.LD * ncols1 + 2 * (size_t)p.LD * p.nc + 8 + p.m;
    return dbl * sizeof(double);
}

static const size_t ELL_LDS_MAX_BYTES = 8192;

static size_t fused2_lds_bytes(const KParams &p, bool jac, bool ell_lds) {  // version-2 kernel
    const size_t ncols1 = jac ? (size_t)(2 + p.m) * p.nc : 2 * (size_t)p.nc;
    const size_t n_ell = (size_t)p.m * p.n * p.ell_w;
    size_t bytes = ((size_t)p.LD * p.n * (jac ? 2 : 1) + 2 * p.LD * ncols1 + (size_t)p.LD * p.nc + 2 * (p.m + 1)) * sizeof(double);
    if (jac && ell_lds) bytes += n_ell * sizeof(double) + (n_ell * sizeof(unsigned short) + 7) / 8 * 8;
    return bytes + 128;  // slack: operand tiles may be read past the last buffer's edge
}

static bool ell_fits_lds(const pcl_ctx *ctx) {
    const size_t n_ell = (size_t)ctx->desc.n_drives * ctx->n * ctx->ell_w;
    return n_ell > 0 && n_ell * (sizeof(double) + sizeof(unsigned short)) <= ELL_LDS_MAX_BYTES;
}

// State columns per workgroup.  Every slice recomputes G(u_k)^2, so fewer, wider slices do less
// arithmetic; but (i) two workgroups must fit in one CU's LDS so that one streams while the other
// computes, and (ii) the grid has to cover the chip a few times over.
static int choose_cols_per_slice(const pcl_ctx *ctx, bool jac) {
    const int d = ctx->cols;
    if (ctx->opt_cols_per_slice > 0) return (int)std::min<int64_t>(ctx->opt_cols_per_slice, d);
    KParams p;
    memset(&p, 0, sizeof p);
    p.n = ctx->n;
    p.m = ctx->desc.n_drives;
    p.LD = ((ctx->n + 3) & ~3) + 2;
    p.ell_w = ctx->ell_w;
    const bool v2 = ctx->opt_kernel == 0 || ctx->opt_kernel >= 2;
    const bool ell = ell_fits_lds(ctx);
    auto bytes = [&](int nc) {
        p.nc = nc;
        return v2 ? fused2_lds_bytes(p, jac, ell) : fused_lds_bytes(p, jac);
    };
    const long long bk = (long long)ctx->win_count * ctx->K;
    const long long want = 3LL * std::max(ctx->n_cu, 1);
    int best = 1;
    for (int nc = d; nc >= 1; --nc) {
        if (bytes(nc) > (size_t)ctx->max_lds / 2 && nc > 1) continue;  // keep two workgroups per CU
        const long long S = (d + nc - 1) / nc;
        best = nc;
        if (!jac || bk * S >= want) break;
    }
    return best;
}

static bool v3_supported(const pcl_ctx *ctx) { return 2 + ctx->desc.n_drives <= 16; }
static int v3_ncw(const pcl_ctx *ctx, int nc) { return std::max(1, std::min(nc, 16 / (2 + ctx->desc.n_drives))); }

static size_t fused3_lds_bytes(const pcl_ctx *ctx, const KParams &p, bool tab) {  // version-3 kernel
    const size_t tile = (size_t)p.LD * p.n, wsz = (size_t)p.LD * (16 + 3 * p.ncw);
    const size_t n_ell = (size_t)p.m * p.n * p.ell_w, n_un = (size_t)ctx->n_upos, uw = (size_t)ctx->uell_w;
    size_t bytes = (4 * tile + 4 * wsz + 3 * (size_t)(p.m + 1) + 2) * sizeof(double);
    if (tab) bytes += (n_un * uw + n_un + n_ell) * sizeof(double) + (n_un + n_ell) * 2 + n_un * uw;
    return (bytes + 7) / 8 * 8 + 128;  // slack: operand tiles may be read past the last buffer's edge
}

// v3 cost model: one workgroup per CU walks ceil(items / CUs) items; an item costs max(store stream, matrix work).
// Constants are the measured config-3 phase times (scripts/phase_timing.py, with the stream running): ~7 us per
// 2-column chunk, ~4 us for G(u) + G^2, stream at ~0.85 of the CU's fair HBM share; other shapes scale by MFMA count.
// Role split needs the chunk buffers of matrix waves 4..7 inside the second halves of the G / G^2 double buffers.
// the shape of BASELINE configs 3/4/5 (three 3-level transmons: d = 27, six drives with two entries per row)
// plus two 5-level transmons (d = 25, four drives) and, for launches of one round of workgroups, two 4-level transmons
static bool v3_specialised(const pcl_ctx *ctx) {
    if (!ctx->opt_specialize || ctx->ell_w < 1 || ctx->ell_w > 2) return false;
    const int d = ctx->desc.d, m = ctx->desc.n_drives;
    if (ctx->ell_w == 2 && ((d == 27 && m == 6) || (d == 25 && m == 4))) return true;
    if (ctx->ell_w == 2 && d == 16 && m == 4 && (long long)ctx->win_count * ctx->K <= 512) return true;
    // Other shapes: `kernel_version = 3` compiles the shape on first use (hiprtc) instead of running the run-time-shape
    // instance; measured on d = 22..30 it only ties the persistent two-workgroup kernels, so `auto` does not take it.
    return false;
}
static bool v3_role_split_fits(const pcl_ctx *ctx) {
    const int ncw = v3_ncw(ctx, ctx->desc.d), LD = lds_ld(ctx->n);
    return 2 * (size_t)LD * (16 + 3 * ncw) <= (size_t)LD * ctx->n;
}
// Work split of kernel 3: contiguous column ranges (+ role split) pay off once every CU has a few intervals' worth of
// columns; below that the round-robin slices balance a short launch better (measured: batch >= 3 at config 3).
static bool v3_contiguous(const pcl_ctx *ctx) {
    if (ctx->opt_cols_per_slice > 0 || ctx->opt_contig == 0) return false;
    if (ctx->opt_contig > 0) return true;
    const long long cols = (long long)ctx->win_count * ctx->K * ctx->desc.d;
    return v3_role_split_fits(ctx) && cols >= 28LL * std::max(ctx->n_cu, 1);
}
static int choose_cols_v3(const pcl_ctx *ctx) {
    const int d = ctx->desc.d, n = ctx->n, m = ctx->desc.n_drives;
    if (ctx->opt_cols_per_slice > 0) return (int)std::min<int64_t>(ctx->opt_cols_per_slice, d);
    const double hbm = 0.85 * 6.3e12;  // store-stream rate the kernel sustains chip-wide
    const long long bk = (long long)ctx->win_count * ctx->K;
    const int rt = (n + 15) / 16, ks = (n + 3) / 4;
    const int g2ct = ctx->iso ? (d + 15) / 16 : (n + 15) / 16;
    const double t_chunk = 7.0e-6 * (rt * ks) / (4.0 * 14.0);
    const double t_build = 4.0e-6 * (((rt + 3) / 4) * ((g2ct + 1) / 2) * ks) / 14.0;
    std::vector<double> tt(d + 1, 1e300);
    double best_t = 1e300;
    for (int nc = 1; nc <= d; ++nc) {
        const int ncw = v3_ncw(ctx, nc);
        const long long S = (d + nc - 1) / nc;
        const long long items = bk * S, ncu = std::max(ctx->n_cu, 1);
        const int chunks_per_wave = ((nc + ncw - 1) / ncw + 3) / 4;
        const double t_matrix = t_build + chunks_per_wave * t_chunk;
        const double item_bytes = 2.0 * nc * n * n * 8.0;
        // rounds of up to n_cu items; the HBM rate is shared by the workgroups active in the round (a lone CU tops out
        // at a few times its fair share)
        double t = 0.0;
        for (long long left = items; left > 0; left -= ncu) {
            const double active = (double)std::min(left, ncu);
            const double rate = std::min(hbm / active, 3.0 * hbm / (double)ncu);
            t += std::max(item_bytes / rate, t_matrix);
        }
        // a ragged last slice (d % nc != 0) leaves workgroups with unequal items: charge the mean fill
        const double fill = (double)d / (double)(S * nc);
        tt[nc] = t / std::sqrt(std::max(fill, 0.25)) + 2.0 * t_build;
        best_t = std::min(best_t, tt[nc]);
    }
    // among near-ties take the narrowest slice (more, smaller items balance better across the CUs)
    int best = d;
    for (int nc = d; nc >= 1; --nc)
        if (tt[nc] <= 1.06 * best_t) best = nc;
    return best;
}

// General-order kernel (pade_order != 4, or option general_pade_kernel): slice width from the LDS budget.
static size_t pade_lds_bytes(const KParams &p, bool jac) {
    const size_t tiles = (jac ? 3 : 1) * (size_t)p.LD * p.n;
    const size_t percol = (size_t)(p.q + 1) + 2 + (jac ? 2 + 2 * (size_t)p.m : 0);
    return (tiles + percol * p.LD * p.nc + 8 + p.m) * sizeof(double);
}
// Lock-step general-order kernel (pcl_kernel_pade_v2.hpp).  PCL_ENOTIMPL (no error text): the shape is not taken, the caller
// falls back to the reference formulation.
static int launch_pade_v2(pcl_ctx *ctx, KParams &p) {
    const int n = p.n, m = p.m, cols = p.cols;
    if ((n & 1) || n > 64 || n < 2 || !p.jac) return PCL_ENOTIMPL;
    const int LD = n | 1;
    auto lds_of = [&](int S) {
        const int nc = (cols + S - 1) / S, npc = (n + S - 1) / S;
        return ((size_t)((2 + 2 * (2 + m)) * nc + n + npc) * LD + 80 + m + 8) * sizeof(double);
    };
    const long long items = (long long)p.batch * p.K;
    const int s_max = std::max(cols, 1);
    int S = 1;
    while (S < s_max && lds_of(S) > (size_t)ctx->max_lds) ++S;
    if (lds_of(S) > (size_t)ctx->max_lds) return PCL_ENOTIMPL;
    if (ctx->opt_general_slices > 0)
        S = (int)std::max<int64_t>(S, std::min<int64_t>(ctx->opt_general_slices, s_max));
    else  // few intervals: more, narrower slices while the grid still fits the CUs in one round
        S = std::max(S, (int)std::min<long long>(s_max, ctx->n_cu / std::max(items, 1LL)));
    p.LD = LD;
    p.nc = (cols + S - 1) / S;
    p.S = S;  // (slices beyond the last state column still carry their columns of the powers)
    size_t lds = lds_of(S);
    const size_t ell_bytes = (size_t)m * n * p.ell_w * (sizeof(double) + sizeof(int)) + 16;
    p.ell_lds = m > 0 && lds + ell_bytes <= (size_t)ctx->max_lds;
    if (p.ell_lds) lds += ell_bytes;
    p.lds_doubles = (int)(lds / sizeof(double));
    const long long grid = items * p.S;
    if (int rc = check_grid(ctx, grid)) return rc;
    int rc = set_lds_attr(ctx, (const void *)pcl_pade_v2_kernel, 7, lds);
    if (rc != PCL_OK) return rc;
    hipLaunchKernelGGL(pcl_pade_v2_kernel, dim3((unsigned)grid), dim3(PV2_NT), lds, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_kernel = 190 + p.q;
    ctx->last_n_stream = 0;
    return PCL_OK;
}

// Large-generator kernel (pcl_kernel_pade_large.hpp; contexts created with PCL_LARGE_N).  The plan: LD = n | 1, 64 threads per 16-row tile of G;
// what the one tile leaves of the LDS is NB column blocks of LD doubles.  A chain unit takes nc state columns and mg drives:
// nc (2 + 2 (2 + mg)) blocks (-S, D, and W | V | dW_l twice) with the Jacobian, 4 nc (W alone) without.  The widest nc that leaves room for
// one drive and one power column is taken (option cols_per_slice caps it) and evened over the slices, then the most drives per group that fit,
// evened over the groups;
// then units are added until the panel of ceil(n / U) power columns fits beside the chain blocks and a thread owns at most PL_NP pairs of it,
// and, for launches of few intervals, up to one unit per 16 power columns while the grid stays within one round of the CUs (option
// general_slices: that many units at least).  Every split gives the same bits.
// The payload-only launch (option large_reduce, pcl_eval_jac_merit_dev without values): the same chain units and nothing else -- U = sx ngrp, npc = 0.
struct LargePlan : LargeTile {
    int sx, nc, mg, ngrp, U, npc;
    size_t lds;
};
static void large_plan(const pcl_ctx *ctx, int n, int cols, int m, bool jac, long long items, LargePlan &P, bool payload_only = false) {
    static_cast<LargeTile &>(P) = large_tile(ctx->max_lds, n, m);
    const int nc_cap = ctx->opt_cols_per_slice > 0 ? (int)std::min<int64_t>(ctx->opt_cols_per_slice, cols) : cols;
    P.nc = 1, P.mg = jac && m > 0 ? 1 : 0;
    for (int nc = nc_cap; nc >= 1; --nc) {
        if (!jac) {
            if (4 * nc > P.NB && nc > 1) continue;
            P.nc = nc;
            break;
        }
        const int mg_max = m > 0 ? std::min(m, ((P.NB - 1) / nc - 6) / 2) : 0;
        if ((m > 0 ? mg_max < 1 : 6 * nc + 1 > P.NB) && nc > 1) continue;
        P.nc = nc;
        P.mg = m > 0 ? std::max(mg_max, 1) : 0;
        break;
    }
    P.ngrp = jac && m > 0 ? even_split(m, P.mg) : 1;  // even groups
    P.sx = even_split(cols, P.nc);                    // even slices
    const int chain_units = P.sx * P.ngrp, chain_blocks = P.nc * (jac ? 2 + 2 * (2 + P.mg) : 4);
    P.U = chain_units;
    P.npc = 0;
    if (jac && !payload_only) {
        auto fits = [&](int U) {
            const int npc = (n + U - 1) / U;
            return chain_blocks + npc <= P.NB && ((long long)n * npc + 1) / 2 <= (long long)PL_NP * P.threads;
        };
        while (P.U < n && !fits(P.U)) ++P.U;
        const long long want = ctx->opt_general_slices > 0 ? ctx->opt_general_slices
                                                          : std::min<long long>(std::max(chain_units, (n + 15) / 16), ctx->n_cu / std::max(items, 1LL));
        P.U = (int)std::max<long long>(P.U, std::min<long long>(want, n));
        P.npc = (n + P.U - 1) / P.U;
        P.U = std::max(chain_units, (n + P.npc - 1) / P.npc);  // (no unit without work)
    }
    P.lds = (size_t)(P.fixed + (long long)P.LD * (chain_blocks + P.npc)) * sizeof(double);
}
// mode (option large_reduce): PL_FULL | PL_COMPACT | PL_MERIT (p.mpart, p.mlam set) | PL_PAYLOAD (the same, no values) -- pcl_kernel_pade_large.hpp
static int launch_pade_large(pcl_ctx *ctx, KParams &p, bool want_jac, int mode = PL_FULL) {
    fill_pade(p, ctx->desc.pade_order);
    LargePlan P;
    const long long items = (long long)p.batch * p.K;
    large_plan(ctx, p.n, p.cols, p.m, want_jac, items, P, mode == PL_PAYLOAD);
    if (P.lds > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "the large-generator kernel needs %zu B of LDS (> %d) for n = %d, m = %d", P.lds, ctx->max_lds, p.n, p.m);
    p.LD = P.LD;
    p.nc = P.nc;
    p.S = P.U;
    p.lds_doubles = (int)(P.lds / sizeof(double));
    if (p.nt == 2) p.nt = 0;  // (plain or nontemporal block stores; the hand-written write-through store is kernel 3's and 4's)
    const long long grid = items * P.U;
    if (int rc = check_grid(ctx, grid)) return rc;
    typedef void (*kern_t)(const KParams, const int, const int, const int);
    const kern_t kern = !want_jac             ? (kern_t)pcl_pade_large_kernel<false>
                        : mode == PL_COMPACT  ? (kern_t)pcl_pade_large_kernel<true, PL_COMPACT>
                        : mode == PL_MERIT    ? (kern_t)pcl_pade_large_kernel<true, PL_MERIT>
                        : mode == PL_PAYLOAD  ? (kern_t)pcl_pade_large_kernel<true, PL_PAYLOAD>
                                              : (kern_t)pcl_pade_large_kernel<true>;
    if (int rc = set_lds_attr(ctx, (const void *)kern, want_jac ? 7 : 8, P.lds)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)P.threads), P.lds, ctx->stream, p, P.sx, P.mg, P.npc);
    HIP_TRY(ctx, hipGetLastError());
    // 280 + q the residual | 290 + q residual + Jacobian (with or without the payload's partial sums) | 300 + q the compact values | 310 + q the payload alone
    ctx->last_kernel = (!want_jac ? 280 : mode == PL_COMPACT ? 300 : mode == PL_PAYLOAD ? 310 : 290) + p.q;
    ctx->last_n_stream = 0;
    return PCL_OK;
}

// Large exponential kernel (pcl_kernel_large_exp.hpp; contexts created with PCL_LARGE_N | PCL_LARGE_EXP on the exponential constraint).  The plan:
// LD = n | 1, 64 threads per 16-row tile of G; what the one tile leaves of the LDS is NB column blocks of LD doubles, a third of them (NBW) per
// buffer, since Y, V and the level's result rotate through three.  A chain unit takes nc state columns (at most 16, one column tile of V; option
// cols_per_slice sets another cap) and mg drives: nc (1 + mg) columns (V | dV_l), nc without the Jacobian; the slices are evened.  Among the
// drive-group sizes that leave a column of E beside the chain (option large_exp_drives caps them; each evened over its groups) and, for each,
// the fewest units that fit and the fewest whose columns of E end with the chain's last 16-column tile, the plan with the shortest launch is
// taken: ceil(W / 16) tile passes per unit times the rounds of the grid over the CUs; on a tie the fewest passes in all, then the larger
// group.  Option general_slices: that many units at least.  Every split gives the same bits.
// The payload-only launch (option large_exp_reduce, pcl_eval_jac_merit_dev without values; mode LE_PAYLOAD): the slices of the Jacobian plan, chain
// units alone -- no column of E, so a group may fill a buffer: nc (1 + mg) <= NBW (option large_exp_drives caps mg) -- chosen by the same count
// (tile passes times rounds of the grid, then the fewest passes, then the larger group); U = sx ngrp, npc = 0, LDS = fixed + 3 LD nc (1 + mg).
struct LargeExpPlan : LargeTile {
    int NBW, sx, nc, mg, ngrp, U, npc, W;
    size_t lds;
};
static void large_exp_plan(const pcl_ctx *ctx, int n, int cols, int m, bool jac, long long items, LargeExpPlan &P, bool payload_only = false) {
    static_cast<LargeTile &>(P) = large_tile(ctx->max_lds, n, m);
    P.NBW = P.NB / 3;
    const bool drv = jac && m > 0;
    const int nc_cap = ctx->opt_cols_per_slice > 0 ? (int)std::min<int64_t>(ctx->opt_cols_per_slice, cols) : std::min(cols, 16);
    P.nc = std::max(1, std::min(nc_cap, (P.NBW - (jac ? 1 : 0)) / (drv ? 2 : 1)));
    P.sx = even_split(cols, P.nc);  // even slices
    P.mg = 0, P.ngrp = 1, P.U = P.sx, P.npc = 0;
    if (jac && payload_only) {
        int mg_fit = drv ? std::max(1, std::min(m, P.NBW / P.nc - 1)) : 0;
        if (drv && ctx->opt_large_exp_drives > 0) mg_fit = (int)std::min<int64_t>(mg_fit, ctx->opt_large_exp_drives);
        long long best_t = -1, best_p = -1;
        for (int mg0 = mg_fit; mg0 >= (drv ? 1 : 0); --mg0) {
            int mg = mg0;
            const int ngrp = drv ? even_split(m, mg) : 1;  // even groups
            const int U = P.sx * ngrp;
            const long long tiles = (P.nc * (1 + mg) + 15) / 16, rounds = (std::max(items, 1LL) * U + ctx->n_cu - 1) / std::max(ctx->n_cu, 1);
            const long long t = tiles * rounds, passes = tiles * U;
            if (best_t < 0 || t < best_t || (t == best_t && passes < best_p)) best_t = t, best_p = passes, P.mg = mg, P.ngrp = ngrp, P.U = U;
            if (!drv) break;
        }
    } else if (jac) {
        int mg_fit = drv ? std::max(1, std::min(m, (P.NBW - 1) / P.nc - 1)) : 0;
        if (drv && ctx->opt_large_exp_drives > 0) mg_fit = (int)std::min<int64_t>(mg_fit, ctx->opt_large_exp_drives);
        // per group size two candidates: the fewest units that fit, and the fewest whose columns of E end with the chain's last column tile
        long long best_t = -1, best_p = -1;
        for (int mg0 = mg_fit; mg0 >= (drv ? 1 : 0); --mg0) {
            int mg = mg0;
            const int ngrp = drv ? even_split(m, mg) : 1;  // even groups
            const int cx = P.nc * (1 + mg), npc_max = std::max(1, std::min(n, P.NBW - cx)), npc_16 = std::min(npc_max, 16 * (cx / 16 + 1) - cx);
            for (int cand = 0; cand < 2; ++cand) {
                const int npc0 = cand ? npc_16 : npc_max;
                const int U = std::max(P.sx * ngrp, (n + npc0 - 1) / npc0), npc = (n + U - 1) / U;
                const long long tiles = (cx + npc + 15) / 16, rounds = (std::max(items, 1LL) * U + ctx->n_cu - 1) / std::max(ctx->n_cu, 1);
                const long long t = tiles * rounds, passes = tiles * U;  // the launch's time in tile passes; what it occupies
                if (best_t < 0 || t < best_t || (t == best_t && passes < best_p)) best_t = t, best_p = passes, P.mg = mg, P.ngrp = ngrp, P.U = U;
            }
            if (!drv) break;
        }
        const int chain_units = P.sx * P.ngrp;
        if (ctx->opt_general_slices > 0) P.U = (int)std::max<long long>(P.U, std::min<long long>(ctx->opt_general_slices, n));
        P.npc = (n + P.U - 1) / P.U;
        P.U = std::max(chain_units, (n + P.npc - 1) / P.npc);  // (no unit without work)
    }
    P.W = P.nc * (1 + P.mg) + P.npc;
    P.lds = (size_t)(P.fixed + 3LL * P.LD * P.W) * sizeof(double);
}
// mode (option large_exp_reduce): LE_FULL | LE_COMPACT | LE_MERIT (p.mpart, p.mlam set) | LE_PAYLOAD (the same, no values) -- pcl_kernel_large_exp.hpp
static int launch_large_exp(pcl_ctx *ctx, KParams &p, bool want_jac, int mode = LE_FULL) {
    LargeExpPlan P;
    const long long items = (long long)p.batch * p.K;
    large_exp_plan(ctx, p.n, p.cols, p.m, want_jac, items, P, mode == LE_PAYLOAD);
    if (P.lds > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "the large exponential kernel needs %zu B of LDS (> %d) for n = %d, m = %d", P.lds, ctx->max_lds, p.n, p.m);
    p.LD = P.LD;
    p.nc = P.nc;
    p.S = P.U;
    p.lds_doubles = (int)(P.lds / sizeof(double));
    if (p.nt >= 2) p.nt = 0;  // (plain or nontemporal block stores; the hand-written write-through store is kernel 3's and 4's)
    const long long grid = items * P.U;
    if (int rc = check_grid(ctx, grid)) return rc;
    typedef void (*kern_t)(const KParams, const int, const int, const int);
    const kern_t kern = !want_jac            ? (kern_t)pcl_large_exp_kernel<false>
                        : mode == LE_COMPACT ? (kern_t)pcl_large_exp_kernel<true, LE_COMPACT>
                        : mode == LE_MERIT   ? (kern_t)pcl_large_exp_kernel<true, LE_MERIT>
                        : mode == LE_PAYLOAD ? (kern_t)pcl_large_exp_kernel<true, LE_PAYLOAD>
                                             : (kern_t)pcl_large_exp_kernel<true>;
    if (int rc = set_lds_attr(ctx, (const void *)kern, want_jac ? 7 : 8, P.lds)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)P.threads), P.lds, ctx->stream, p, P.sx, P.mg, P.npc);
    HIP_TRY(ctx, hipGetLastError());
    // the large exponential kernel: 320 residual + Jacobian (with or without the payload's partial sums) | 321 residual only | 322 the compact values | 323 the payload alone
    ctx->last_kernel = !want_jac ? 321 : mode == LE_COMPACT ? 322 : mode == LE_PAYLOAD ? 323 : 320;
    ctx->last_n_stream = 0;
    return PCL_OK;
}

// Pattern-compiled fused residual + Jacobian kernel (pcl_kernel_fused_sparse.hpp; any Pade order): sparse exact-iso generators of
// a unitary problem whose m + 7 chain tiles fit LDS.  PCL_ENOTIMPL (no error text): not taken, the caller goes on to the others.
static bool v4_available(const pcl_ctx *ctx) {
    return ctx->v4_plan && !ctx->v4_failed && ctx->opt_jit && !ctx->vec && ctx->cols == ctx->desc.d;
}
// the generated module of the context's system and order (both kernels), compiled on first use
static int v4_module(pcl_ctx *ctx, int q, int np) {
    if (ctx->v4_f && ctx->v4_feval) return PCL_OK;
    const std::string src = v4_source(*ctx->v4_plan, q, np, (int)ctx->opt_v4_variant);
    const std::string key = "fused-sparse:" + std::to_string(q) + ":" + std::to_string(std::hash<std::string>{}(src));
    ctx->v4_f = jit_compile(ctx->device, key, src, "pcl_fused_sparse_kernel", true);
    ctx->v4_feval = ctx->v4_f ? jit_compile(ctx->device, key, src, "pcl_eval_sparse4_kernel", true) : nullptr;
    ctx->v4_fevalc = (ctx->v4_feval && src.find("#define SP4_COOP 1") != std::string::npos) ? jit_compile(ctx->device, key, src, "pcl_eval_sparse4c_kernel", true) : nullptr;
    if (!ctx->v4_f || !ctx->v4_feval) {
        ctx->v4_f = ctx->v4_feval = ctx->v4_fevalc = nullptr;
        ctx->v4_failed = 1;
        return jit_fell_back(ctx, "residual + Jacobian");
    }
    return PCL_OK;
}
// Residual only on the same products: one wave per interval, 4 waves per workgroup (three tiles each)
static int launch_eval_v4(pcl_ctx *ctx, KParams &p) {
    if (!v4_available(ctx) || !p.delta) return PCL_ENOTIMPL;
    const pcl_codegen::V4Plan &v4 = *ctx->v4_plan;
    fill_pade(p, ctx->desc.pade_order);
    const int np = v4_power_tiles(p.d, p.m, p.q, (size_t)ctx->max_lds);
    if (!np) return PCL_ENOTIMPL;
    if (int rc = v4_module(ctx, p.q, np)) return rc;  // (PCL_ENOTIMPL: the caller goes on to the other kernels)
    const long long items = (long long)p.batch * p.K;
    if (int rc = check_grid(ctx, items)) return rc;
    const int nw = 4;
    const size_t lds = (size_t)nw * 3 * p.d * (p.n + 1) * sizeof(double);
    const int per_cu = std::max(1, (int)((size_t)ctx->max_lds / lds));
    const long long slots = (long long)per_cu * std::max(ctx->n_cu, 1);
    long long grid = std::min<long long>((items + nw - 1) / nw, slots);
    if (ctx->opt_grid > 0) grid = std::min<long long>(ctx->opt_grid, (items + nw - 1) / nw);
    const V4Tabs T = v4_tabs(ctx);
    void *args[] = {(void *)&p, (void *)&T.tab, (void *)&ctx->dv4_mags, (void *)&T.dcf};
    // small launches (up to two intervals per CU: a line-search trial on one to four trajectories): four waves per interval, the products in
    // four row ranges -- config 3, one trajectory: 8.7 -> 6.3 us per launch at order 4, 11.9 -> 7.8 at order 8; four trajectories 9.1 -> 7.9;
    // eight: 10.0 -> 11.8, so one wave per interval above (option eval_coop: -1 auto | 0 | 1)
    // (one wave per interval holds three tiles per wave, 12 in all: more than the LDS from d = 29 on -- the cooperative kernel's four tiles take those systems)
    const bool fits1 = lds <= (size_t)ctx->max_lds;
    if (!fits1 && ctx->opt_eval_coop == 0)
        return fail(ctx, PCL_ESHAPE, "eval_coop=0: one wave per interval needs %zu bytes of LDS at d = %d, the device has %zu", lds, p.d, (size_t)ctx->max_lds);
    const bool coop = ctx->v4_fevalc && (ctx->opt_eval_coop == 1 || !fits1 || (ctx->opt_eval_coop < 0 && items <= 2LL * std::max(ctx->n_cu, 1)));
    if (!coop && !fits1) return PCL_ENOTIMPL;
    ctx->last_eval_coop = coop ? 1 : 0;
    if (coop) {
        const size_t ldsc = (size_t)4 * p.d * (p.n + 1) * sizeof(double);
        const long long gc = ctx->opt_grid > 0 ? std::min<long long>(ctx->opt_grid, items) : std::min<long long>(items, 3LL * std::max(ctx->n_cu, 1));
        HIP_TRY(ctx, hipModuleLaunchKernel(ctx->v4_fevalc, (unsigned)gc, 1, 1, 64 * pcl_codegen::v4_parts(v4, p.q), 1, 1, (unsigned)ldsc, ctx->stream, args, nullptr));
    } else
        HIP_TRY(ctx, hipModuleLaunchKernel(ctx->v4_feval, (unsigned)grid, 1, 1, 64 * nw, 1, 1, (unsigned)lds, ctx->stream, args, nullptr));
    ctx->last_kernel = 80 + p.q;
    ctx->last_n_stream = 0;
    return PCL_OK;
}
static int launch_fused_v4(pcl_ctx *ctx, KParams &p, bool compact, bool want_merit = false);
// (the slice-ticket module could not be had: the same launch with the static split, from a fresh parameter block)
static int launch_fused_v4_static(pcl_ctx *ctx, KParams &p, bool compact, bool want_merit) {
    const int64_t keep = ctx->opt_v4_ticket;
    ctx->opt_v4_ticket = 0;
    p.tick = nullptr;
    p.tick_cpi = p.tick_G = p.tick_ahead = 0;
    const int rc = launch_fused_v4(ctx, p, compact, want_merit);
    ctx->opt_v4_ticket = keep;
    return rc;
}
static int launch_fused_v4(pcl_ctx *ctx, KParams &p, bool compact, bool want_merit) {
    if (!v4_available(ctx) || !p.jac) return PCL_ENOTIMPL;
    fill_pade(p, ctx->desc.pade_order);
    const int np = v4_power_tiles(p.d, p.m, p.q, (size_t)ctx->max_lds);
    if (!np) return PCL_ENOTIMPL;
    if (int rc = v4_module(ctx, p.q, np)) return rc;
    const int d = p.d, m = p.m;
    const long long bk = (long long)p.batch * p.K, ncu = std::max(ctx->n_cu, 1);
    // contiguous column ranges once every CU has about an interval's worth of columns; below that round-robin slices of the
    // intervals (an explicit cols_per_slice or contiguous = 0 / 1 decides otherwise)
    // (compact launches -- unique tiles only, the chains are all of the work -- deal the intervals round-robin: a contiguous range that
    //  ends inside an interval runs that interval's chains in two workgroups; 62.2 against 66.8 us per 8 trajectories)
    p.contig = ctx->opt_cols_per_slice > 0 ? 0 : (ctx->opt_contig >= 0 ? (int)ctx->opt_contig : (!compact && bk * d >= 28 * ncu ? 1 : 0));
    // SLICE TICKETS instead of a static split (launches of several trajectories; see the head of pcl_kernel_fused_sparse.hpp): groups of
    // workgroups walk the intervals in a static order and take slices of a few state columns from the interval's own counter, each when
    // the previous slice's stores are issued -- the front of addresses being written stays tight and the workgroups the memory side
    // serves first take more slices: the time no longer depends on where the values array's pages live.
    const int tick_G = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->opt_v4_group > 0 ? ctx->opt_v4_group : 8, ncu));
    // (the grid a ticket launch gets -- the round-robin split's, below -- must hold one whole group: the kernel divides by gridDim.x / tick_G.  A launch
    //  of fewer slices than CUs under a large v4_group had no group at all; it runs the static split now: the same bits)
    const long long tick_S = std::max<long long>(1, std::min<long long>(d, ncu / std::max<long long>(bk, 1)));
    const long long tick_nc = ctx->opt_cols_per_slice > 0 ? std::min<long long>(ctx->opt_cols_per_slice, d) : (d + tick_S - 1) / tick_S;
    const long long tick_grid = std::min<long long>(bk * ((d + tick_nc - 1) / tick_nc), ncu);
    const bool ticket_ok = !ctx->res_capture && !compact && ctx->dv4_tick && !ctx->v4_ft_failed && ctx->opt_grid <= 0 && m + 10 <= 16 && ncu % tick_G == 0 &&
                           tick_grid >= tick_G && v4_lds_bytes(d, m, np) + 8 * 8 * 128 <= (size_t)ctx->max_lds;
    const bool ticket_auto = ticket_ok && ctx->opt_v4_ticket < 0 && p.q <= 2 && p.contig && ctx->opt_contig < 0 && ctx->opt_cols_per_slice <= 0;
    // auto: which of the two this values array gets (see v4_tune); timed launches are bracketed by events below
    pcl_ctx::V4Tune *tune = nullptr;
    int tune_slot = -1, tune_variant = 1;
    // (a stream that is being captured into a graph takes no part in the sampling: event records would become graph nodes and a query is illegal
    //  there; the launch gets the array's decided variant, else the tickets, and nothing of the sampling state moves)
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    const bool capturing = ticket_auto && ctx->opt_v4_tune != 0 && (hipStreamIsCapturing(ctx->stream, &cap_status) != hipSuccess || cap_status != hipStreamCaptureStatusNone);
    if (capturing) {
        (void)hipGetLastError();
        for (auto &t : ctx->v4_tune)
            if (t.key == (const void *)p.jac && t.units == bk && t.choice >= 0) tune_variant = t.choice;
    } else if (ticket_auto && ctx->opt_v4_tune != 0) {
        pcl_ctx::V4Tune *T = nullptr;
        for (auto &t : ctx->v4_tune)
            if (t.key == (const void *)p.jac && t.units == bk) T = &t;
        if (!T) {  // the least recently used entry makes room
            T = &ctx->v4_tune[0];
            for (auto &t : ctx->v4_tune)
                if (t.stamp < T->stamp) T = &t;
            for (int i = 0; i < 8; ++i) T->pend[i] = false;
            T->key = (const void *)p.jac, T->units = bk, T->calls = 0, T->choice = -1, T->done[0] = T->done[1] = 0, T->best[0] = T->best[1] = 1e30f;
        }
        T->stamp = ++ctx->v4_tune_clock;
        if (T->choice < 0) {
            for (int i = 0; i < 8; ++i)  // timings that have come back
                if (T->pend[i] && hipEventQuery(T->ev[i][1]) == hipSuccess) {
                    float ms = 0.f;
                    if (hipEventElapsedTime(&ms, T->ev[i][0], T->ev[i][1]) == hipSuccess && ms > 0.f) {
                        T->best[T->pend_variant[i]] = std::min(T->best[T->pend_variant[i]], ms);
                        ++T->done[T->pend_variant[i]];
                    }
                    T->pend[i] = false;
                }
            (void)hipGetLastError();  // (hipErrorNotReady of a query is not an error of this call)
            if (T->done[0] >= 3 && T->done[1] >= 3) {
                T->choice = (T->best[0] * 1.02f < T->best[1]) ? 0 : 1;
                ctx->last_v4_tune_static_ns = (int64_t)(T->best[0] * 1e6f), ctx->last_v4_tune_ticket_ns = (int64_t)(T->best[1] * 1e6f);  // (ns)
            } else if (T->calls >= 40)
                T->choice = 1;  // (timings that never come back: tickets)
        }
        if (T->choice >= 0)
            tune_variant = T->choice;
        else {
            tune_variant = T->calls < 2 ? 1 : (T->calls & 1);
            if (T->calls >= 2 && T->done[tune_variant] < 3)
                for (int i = 0; i < 8 && tune_slot < 0; ++i)
                    if (!T->pend[i]) tune_slot = i;
            ++T->calls;
            tune = T;
        }
        ctx->last_v4_tune_choice = T->choice;
    }
    const bool ticket = ticket_ok && (ctx->opt_v4_ticket == 1 || (ticket_auto && tune_variant == 1));
    // (orders 6-10: the P wave's q products per visit are the longer chain -- 8 trajectories at order 8: 246-254 against 232 us)
    if (ticket) {
        // (slices of 4 state columns: 201.7 against 203.7 us per 8 seeds and 1.500 against 1.508 ms per 64 for slices of 3, the round-4 default; 5 the same, 2 / 7 / 9 slower: round 5)
        p.tick_cpi = ctx->opt_v4_ticket_cols > 0 ? (int)std::min<int64_t>(ctx->opt_v4_ticket_cols, d) : std::min(4, d);
        while ((d + p.tick_cpi - 1) / p.tick_cpi > 31) ++p.tick_cpi;  // (the slice index travels in five bits)
        p.tick = ctx->dv4_tick;
        p.tick_G = tick_G;
        p.tick_ahead = (int)ctx->opt_v4_ticket_ahead;
        p.contig = 0;
    }
    ctx->last_v4_ticket = ticket ? p.tick_cpi : 0;
    if (p.contig)
        p.nc = d;
    else if (ctx->opt_cols_per_slice > 0)
        p.nc = (int)std::min<int64_t>(ctx->opt_cols_per_slice, d);
    else {
        const long long S = std::max<long long>(1, std::min<long long>(d, ncu / std::max<long long>(bk, 1)));
        p.nc = (int)((d + S - 1) / S);
    }
    p.S = (d + p.nc - 1) / p.nc;
    p.all_matrix = 0;
    p.n_stream = 0;
    p.tail_mode = (int)ctx->opt_v4_tail_mode;
    p.v4_flags = (int)ctx->opt_v4_flags;
    // write-through block stores (auto, launches that fit the infinity cache) pay at orders 8 and 10 only: one trajectory, plain against
    // write-through: 24.9 / 25.4 us at order 2, 27.2 / 27.6 at 4, 28.1 / 28.9 at 6, 32.4 / 31.9 at 8.  Orders 2 and 4: write-through on every
    // other XCD's workgroups (nt 3, see the kernel) -- plain / write-through / mixed 23.3 / 23.7 / 22.7 us at order 2, 26.1 / 25.6 / 25.5 at 4,
    // 26.2 / 27.2 / 26.5 at 6 (plain stays)
    if (ctx->opt_nt < 0 && p.q < 4 && !ctx->res_capture) p.nt = (p.nt == 2 && p.q <= 2) ? 3 : 0;
    // (the resident evaluator: write-through everywhere -- every request ends with a write-back of the L2, and dirty lines of plain stores make
    //  that 10 us per request: 41 against 32 us per evaluation at config 3)
    if (ctx->opt_nt < 0 && ctx->res_capture) p.nt = 2;
    const long long units = p.contig ? bk * d : bk * p.S;
    if (int rc = check_grid(ctx, units)) return rc;
    const long long g = ctx->opt_grid > 0 ? std::min<long long>(ctx->opt_grid, units) : std::min<long long>(units, ncu);
    const size_t lds = v4_lds_bytes(d, m, np) + (ticket ? 8 * 8 * 128 : 0);  // (+ the dispatcher's ring of controls and steps)
    // tiles of the ring in use: q - 1 when workgroups walk several items (the P wave must not run a whole item ahead: measured
    // 8 % on 8 trajectories per launch), all the module has for one-item launches (0.4 us there); option v4_power_tiles overrides
    p.v4_np = ctx->opt_v4_np > 0 ? (int)std::min<int64_t>(ctx->opt_v4_np, np) : ticket ? np : (units > g ? std::max(1, std::min(np, p.q - 1)) : std::min(np, p.q));
    // the cooperative first item (waves 0-3 build the powers, the stream waves fold) with a ring shorter than q: pays up to order 8 (one
    // trajectory 31.4 -> 29.3-30.5 us), not at order 10 (five powers through three tiles: 35.5 against 34.1 us)
    // (since round 5 the first item's powers beyond the ring borrow the chains' dW tiles -- q - v4_np <= m -- and every order starts cooperatively)
    if (p.q >= 5 && p.v4_np < p.q && (p.q - p.v4_np > m || (p.v4_flags & 16))) p.v4_flags |= 4;
    if (ticket) p.tail_mode = p.tail_mode == 3 ? 0 : p.tail_mode;  // (the writer wave stores delta and the tails of a chain ticket)
    if (want_merit && (p.tail_mode == 3 || ticket)) {
        if (!ctx->dmcols) HIP_TRY(ctx, hipMalloc((void **)&ctx->dmcols, (size_t)ctx->desc.batch * p.K * p.d * (p.m + 2) * sizeof(double)));
        p.mpart = ctx->dmcols;
        p.mlam = ctx->merit_lam;
        ctx->merit_fused = 1;
    }
    const V4Tabs T = v4_tabs(ctx);
    void *args[] = {(void *)&p, (void *)&T.tab, (void *)&ctx->dv4_mags, (void *)&T.dcf};
    hipFunction_t fk = ctx->v4_f;
    if (ticket) {  // (a module of its own: the static launches -- one trajectory: the start-up counts -- run without the ticket roles' code)
        if (!ctx->v4_ft && !ctx->v4_ft_failed) {
            const std::string src = v4_source(*ctx->v4_plan, p.q, np, (int)ctx->opt_v4_variant, 1);
            const std::string key = "fused-sparse-tickets:" + std::to_string(p.q) + ":" + std::to_string(std::hash<std::string>{}(src));
            ctx->v4_ft = jit_compile(ctx->device, key, src, "pcl_fused_sparse_kernel", true);
            if (!ctx->v4_ft) {
                ctx->v4_ft_failed = 1;
                // the static-split module computes the same bits: noted once, an error only under require_jit
                if (jit_fell_back(ctx, "residual + Jacobian (slice tickets; the static split runs instead)") == PCL_EHIP) return PCL_EHIP;
            }
        }
        if (ctx->v4_ft)
            fk = ctx->v4_ft;
        else
            return launch_fused_v4_static(ctx, p, compact, want_merit);
    }
    // ONE item per workgroup (one trajectory per launch, or a few: as many workgroups as round-robin slices): a module of its own, the same kernel
    // text with this launch's shape folded in as constants (SP4_ONE_ITEM) -- the general module carries item loops, three work splits, four tail
    // modes, the A/B flags and the reduce payload through a launch whose start-up counts.  Same arithmetic, same bits.
    bool one_item = !ticket && !compact && !p.contig && units == g && ctx->opt_grid <= 0 && !want_merit && !p.mpart && p.tail_mode == 3 && p.v4_flags == 0 && !ctx->res_capture;
#ifdef PCL_PROFILE
    if (p.prof & (2 | 4 | 8 | 32 | 256)) one_item = false;  // (the experiments live in the general module; the stamps are in both)
#endif
    if (ctx->opt_v4_one_item == 1 && !one_item)
        return fail(ctx, PCL_ESHAPE, "v4_one_item=1: the one-item module serves full-value launches of one round-robin slice per workgroup (no tickets, no contiguous ranges, no grid option, no reduce payload, v4_tail_mode 3, v4_flags 0)");
    one_item = one_item && ctx->opt_v4_one_item != 0 && !ctx->v4_f1_failed;
    if (one_item && !ctx->v4_f1) {  // compiled on the first such launch
        const std::string src = v4_source(*ctx->v4_plan, p.q, np, (int)ctx->opt_v4_variant, 3);
        const std::string key = "fused-sparse-one-item:" + std::to_string(p.q) + ":" + std::to_string(std::hash<std::string>{}(src));
        ctx->v4_f1 = jit_compile(ctx->device, key, src, "pcl_fused_sparse_kernel", true);
        if (!ctx->v4_f1) {
            ctx->v4_f1_failed = 1;
            // the general module computes the same bits: noted once, an error only under require_jit
            if (jit_fell_back(ctx, "residual + Jacobian (one item per workgroup; the general module runs instead)") == PCL_EHIP) return PCL_EHIP;
            one_item = false;
        }
    }
    if (one_item) fk = ctx->v4_f1;
    ctx->last_v4_one_item = one_item ? 1 : 0;
#ifdef PCL_LAB
    if (ctx->res_capture) {  // pcl_resident_start: the launch as data
        ctx->res.p = p, ctx->res.tab = T.tab, ctx->res.dcf = T.dcf, ctx->res.grid = g, ctx->res.lds = lds, ctx->res.block = 64u * (unsigned)(m + 9);
        ctx->res_capture = false;
        return PCL_OK;
    }
#endif
    bool timed = false;
    if (tune && tune_slot >= 0) {  // one timed sample of the per-array choice
        bool ok = true;
        for (int e = 0; e < 2 && ok; ++e)
            if (!tune->ev[tune_slot][e]) ok = hipEventCreate(&tune->ev[tune_slot][e]) == hipSuccess;
        timed = ok && hipEventRecord(tune->ev[tune_slot][0], ctx->stream) == hipSuccess;
    }
    HIP_TRY(ctx, hipModuleLaunchKernel(fk, (unsigned)g, 1, 1, 64 * (m + 9 + (ticket ? 1 : 0)), 1, 1, (unsigned)lds, ctx->stream, args, nullptr));
    if (timed && hipEventRecord(tune->ev[tune_slot][1], ctx->stream) == hipSuccess) {
        tune->pend[tune_slot] = true;
        tune->pend_variant[tune_slot] = ticket ? 1 : 0;
    }
    ctx->last_kernel = 40 + p.q;
    ctx->last_n_stream = 0;
    if (ticket) ctx->ticket_launched = true;
    return PCL_OK;
}

static int launch_pade_general(pcl_ctx *ctx, KParams &p, bool want_jac) {
    fill_pade(p, ctx->desc.pade_order);
    if (want_jac && ctx->opt_general_version != 1) {
        const int rc = launch_pade_v2(ctx, p);
        if (rc != PCL_ENOTIMPL) return rc;
        if (ctx->opt_general_version == 2) return fail(ctx, PCL_ESHAPE, "the lock-step general-order kernel does not take this shape (n = %d, %d columns, m = %d)", p.n, p.cols, p.m);
    }
    p.nc = ctx->opt_cols_per_slice > 0 ? (int)std::min<int64_t>(ctx->opt_cols_per_slice, p.cols) : p.cols;
    while (p.nc > 1 && pade_lds_bytes(p, want_jac) > (size_t)ctx->max_lds) --p.nc;
    const size_t lds = pade_lds_bytes(p, want_jac);
    if (lds > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "general-order kernel needs %zu B of LDS (> %d) for d=%d, m=%d, order %d", lds, ctx->max_lds, p.d, p.m, 2 * p.q);
    p.S = (p.cols + p.nc - 1) / p.nc;
    const long long grid = (long long)p.batch * p.K * p.S;
    if (int rc = check_grid(ctx, grid)) return rc;
    typedef void (*kern_t)(const KParams);
    kern_t kern = want_jac ? (kern_t)pcl_pade_kernel<true> : (kern_t)pcl_pade_kernel<false>;
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)ctx->opt_general_threads), lds, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_kernel = 90 + p.q;
    ctx->last_n_stream = 0;
    return PCL_OK;
}

// the payload's partial sums, (m + 2) per (member, interval), and phi per (output set, interval)
static int merit_scratch(pcl_ctx *ctx) {
    const pcl_desc &D = ctx->desc;
    const int sets = D.batch_mode == PCL_BATCH_TRAJ ? D.batch : 1;
    if (!ctx->dphik) HIP_TRY(ctx, hipMalloc((void **)&ctx->dphik, ((size_t)D.batch * ctx->K * (D.n_drives + 2) + (size_t)sets * ctx->K) * sizeof(double)));
    return PCL_OK;
}

// The exponential mode: one workgroup per (member, interval, drive) for residual + Jacobian, per (member, interval) for the residual alone
// (pcl_kernel_exp.hpp).  G_l has an LDS tile of its own where the five tiles and the X_k tile fit.
static int launch_exp(pcl_ctx *ctx, KParams &p, bool want_jac, int mode = 0) {
    const size_t tile = (size_t)p.LD * p.n;
    const bool fre = want_jac && p.m > 0;
    size_t dbl = (want_jac ? 4 : 3) * tile + (size_t)p.LD * p.cols + 32 + 64;
    int gl_lds = 0;
    if (fre && (dbl + tile) * sizeof(double) <= (size_t)ctx->max_lds) gl_lds = 1, dbl += tile;
    const size_t lds = dbl * sizeof(double);
    if (lds > (size_t)ctx->max_lds) return fail(ctx, PCL_ESHAPE, "the exponential kernel needs %zu B of LDS (> %d) for n=%d, %d columns", lds, ctx->max_lds, p.n, p.cols);
    const long long grid = (long long)p.batch * p.K * (want_jac ? std::max(p.m, 1) : 1);
    if (int rc = check_grid(ctx, grid)) return rc;
    typedef void (*kexp_t)(const KParams, const double *, int);
    // mode (option exp_full): the compact values, or the full values with the payload's partial sums (pcl_kernel_exp.hpp)
    const kexp_t kern = !want_jac ? (kexp_t)pcl_exp_kernel<false>
                        : mode == PCL_EXP_COMPACT ? (kexp_t)pcl_exp_kernel<true, PCL_EXP_COMPACT>
                        : mode == PCL_EXP_MERIT   ? (kexp_t)pcl_exp_kernel<true, PCL_EXP_MERIT>
                                                  : (kexp_t)pcl_exp_kernel<true>;
    if (int rc = set_lds_attr(ctx, (const void *)kern, want_jac ? 0 : 2, lds)) return rc;
    const unsigned threads = p.n > 32 ? 512 : 256;  // (more than eight 16 x 16 output tiles per product: eight waves, a pair of tiles each)
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(threads), lds, ctx->stream, p, (const double *)ctx->dGjd, gl_lds);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_kernel = !want_jac ? 101 : (mode == PCL_EXP_COMPACT ? 102 : 100);  // the exponential kernel: fused | residual only | compact
    ctx->last_n_stream = 0;
    return PCL_OK;
}

// The payload-fused call (pcl_eval_jac_merit_dev): the full values with the residual, of every member
static bool merit_call(const pcl_ctx *ctx, const KParams &p) { return ctx->merit_want && !p.compact && p.delta && ctx->win_first == 0 && ctx->win_count == ctx->desc.batch; }

static int launch_fused_exp(pcl_ctx *ctx, KParams &p) {
    const bool want_jac = p.jac != nullptr;
    if (want_jac && p.compact) return launch_exp(ctx, p, true, PCL_EXP_COMPACT);
    // the payload-fused call (pcl_eval_jac_merit_dev, option exp_full): every member, so that the partial sums are numbered as the sum kernel reads them
    if (want_jac && ctx->exp_full && merit_call(ctx, p)) {
        if (int rc = merit_scratch(ctx)) return rc;
        p.mpart = ctx->dphik;
        p.mlam = ctx->merit_lam;
        ctx->merit_fused = 1;
        return launch_exp(ctx, p, true, PCL_EXP_MERIT);
    }
    return launch_exp(ctx, p, want_jac);
}

// kernel_version 5 (auto wherever it applies: n <= 16 rows, at most 8 state columns, m <= 8 -- BASELINE configs 1 and 2, every system of the
// reference's docs with d <= 8; every order): one wave per interval, one round of global loads, everything else in registers and a few KB
// of LDS (pcl_kernel_fused_small.hpp)
// (9 .. 16 rows: four matrix entries per lane -- residual only 5.3 against 5.9 us at d = 5, but residual + Jacobian 11.2 against the 8.3 us of
//  kernel 1, so `auto` takes the 16-row instance for the residual alone; kernel_version = 5 forces it)
static int launch_fused_small(pcl_ctx *ctx, KParams &p) {
    const bool want_jac = p.jac != nullptr;
    fill_pade(p, ctx->desc.pade_order);
    const long long items = (long long)p.batch * p.K;
    if (int rc = check_grid(ctx, items)) return rc;
    const long long grid = ctx->opt_grid > 0 ? std::min<long long>(ctx->opt_grid, items) : std::min<long long>(items, 16LL * std::max(ctx->n_cu, 1));
    typedef void (*ksm_t)(const KParams, const double *);
    const ksm_t ksm = ctx->n <= 8 ? (want_jac ? (ksm_t)pcl_fused_small_kernel<true, 8> : (ksm_t)pcl_fused_small_kernel<false, 8>)
                                  : (want_jac ? (ksm_t)pcl_fused_small_kernel<true, 16> : (ksm_t)pcl_fused_small_kernel<false, 16>);
    hipLaunchKernelGGL(ksm, dim3((unsigned)grid), dim3(64), 0, ctx->stream, p, (const double *)ctx->dGjd);
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_kernel = 50 + p.q;
    ctx->last_n_stream = 0;
    return PCL_OK;
}

// auto: kernel 3 where its shape-specialised instance applies (BASELINE configs 3/4/5); its run-time-shape instances
// lose to kernels 1 / 2 on every other shape measured (scripts/small_d_probe*.py: up to 3x), so they need kernel_version = 3
static int launch_fused_v3(pcl_ctx *ctx, KParams &p) {
    const bool want_jac = p.jac != nullptr, compact = p.compact != 0;
    if (!(want_jac && (!compact || v3_role_split_fits(ctx)) && (ctx->opt_kernel == 3 || (ctx->opt_kernel == 0 && v3_specialised(ctx))) &&
          ctx->opt_use_mfma != 0 && v3_supported(ctx) && !ctx->vec && ctx->cols == ctx->desc.d)) return PCL_ENOTIMPL;
    // default: contiguous column ranges (one item per interval touched); an explicit cols_per_slice or
    // contiguous = 0 selects the round-robin slices
    p.contig = (compact || v3_contiguous(ctx)) ? 1 : 0;  // compact: contiguous ranges, every workgroup in the matrix role
    p.all_matrix = compact ? 1 : 0;
    p.nc = p.contig ? p.d : choose_cols_v3(ctx);
    if (!p.contig && ctx->opt_cols_per_slice <= 0 && p.nc < 2 && p.d >= 2) p.nc = 2;  // keep the 2-column chunks of the specialised instance
    p.ncw = v3_ncw(ctx, p.nc);
    p.tab_lds = 1;
    size_t lds3 = fused3_lds_bytes(ctx, p, true);
    if (lds3 > (size_t)ctx->max_lds) {  // large union / ELL tables stay in memory
        p.tab_lds = 0;
        lds3 = fused3_lds_bytes(ctx, p, false);
    }
    if (lds3 > (size_t)ctx->max_lds) return PCL_ENOTIMPL;  // double-buffered tiles do not fit (n close to 64): kernel v2
    p.S = (p.d + p.nc - 1) / p.nc;
    const long long items = (long long)p.batch * p.K * p.S;
    if (int rc = check_grid(ctx, items)) return rc;
    typedef void (*kern3_t)(const KParams);
    const int ewr = (p.m <= 8 && ctx->ell_w >= 1 && ctx->ell_w <= 2) ? ctx->ell_w : 0;
    kern3_t kern3 = ewr == 1 ? (kern3_t)pcl_fused_kernel_v3<1, 0, 0, 0> : ewr == 2 ? (kern3_t)pcl_fused_kernel_v3<2, 0, 0, 0> : (kern3_t)pcl_fused_kernel_v3<0, 0, 0, 0>;
    // shape-specialised instances (compile-time d, m, chunk width; two drive entries per row):
    //   three 3-level transmons (BASELINE configs 3/4/5), two 5-level transmons, two 4-level transmons
    bool spec3 = false;
    // pcl_eval_jac_merit_dev: the MERIT instances (built in for config 3's shape, compiled on first use for other shapes)
    const bool want_merit = merit_call(ctx, p);
    if (ewr == 2 && p.ncw == 2 && ctx->opt_specialize) {
        spec3 = true;
        if (p.d == 27 && p.m == 6) kern3 = want_merit ? (kern3_t)pcl_fused_kernel_v3<2, 27, 6, 2, true> : (kern3_t)pcl_fused_kernel_v3<2, 27, 6, 2>;
        else if (p.d == 25 && p.m == 4 && !want_merit) kern3 = (kern3_t)pcl_fused_kernel_v3<2, 25, 4, 2>;  // (merit: compiled on first use)
        else if (p.d == 16 && p.m == 4 && !want_merit) kern3 = (kern3_t)pcl_fused_kernel_v3<2, 16, 4, 2>;
        else spec3 = false;
    }
    hipFunction_t jitf = nullptr;  // run-time compiled instance for this context's shape
    if (!spec3 && ctx->opt_jit && ctx->opt_specialize && ewr >= 1) {
        char inst[96];
        snprintf(inst, sizeof inst, want_merit ? "pcl_fused_kernel_v3<%d, %d, %d, %d, true>" : "pcl_fused_kernel_v3<%d, %d, %d, %d>", ewr, p.d, p.m, p.ncw);
        jitf = jit_function(ctx->device, inst);
    }
    if (!spec3 && !jitf && ctx->opt_kernel == 0) return PCL_ENOTIMPL;  // auto never runs the run-time-shape instances
    ctx->last_kernel = jitf ? 32 : 30 + (spec3 ? 1 : 0);
    if (!jitf) {
        int rc = set_lds_attr(ctx, (const void *)kern3, (want_merit && spec3) ? 8 : 6, lds3);
        if (rc != PCL_OK) return rc;
    }
    const long long units = p.contig ? (long long)p.batch * p.K * p.d : items;  // what the grid is cut into
    const long long g3 = ctx->opt_grid > 0 ? std::min<long long>(ctx->opt_grid, units) : std::min<long long>(units, std::max(ctx->n_cu, 1));
    p.n_stream = 0;
    if (p.contig && !p.all_matrix && g3 >= 2 && v3_role_split_fits(ctx)) {
        const long long want = ctx->opt_stream_wg < 0 ? g3 / 2 : ctx->opt_stream_wg;  // auto: half the workgroups stream
        if (want > 0) p.n_stream = (int)std::min<long long>(want, g3 - 1);
    }
    ctx->last_n_stream = p.n_stream;
    if (want_merit && (spec3 || jitf)) {
        // pcl_eval_jac_merit_dev: the matrix waves also leave the reduce payload's dot products per state column
        if (!ctx->dmcols) HIP_TRY(ctx, hipMalloc((void **)&ctx->dmcols, (size_t)ctx->desc.batch * p.K * p.d * (p.m + 2) * sizeof(double)));
        p.mpart = ctx->dmcols;
        p.mlam = ctx->merit_lam;
        ctx->merit_fused = 1;
    }
    if (jitf) {
        void *args[] = {(void *)&p};
        HIP_TRY(ctx, hipModuleLaunchKernel(jitf, (unsigned)g3, 1, 1, 512, 1, 1, (unsigned)lds3, ctx->stream, args, nullptr));
        return PCL_OK;
    }
    hipLaunchKernelGGL(kern3, dim3((unsigned)g3), dim3(512), lds3, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    return PCL_OK;
}

// residual only (what the solver calls in every line-search trial), sparse iso generators: the pattern-compiled kernel
// (auto: launches with more intervals than CUs -- below that one wave per interval is a longer chain than the matrix-core kernel's)
static int launch_eval_sparse(pcl_ctx *ctx, KParams &p) {
    const pcl_codegen::SpPlan &sp = *ctx->sp_plan;
    const long long items = (long long)p.batch * p.K;
    if (int rc = check_grid(ctx, items)) return rc;
    if (!ctx->sp_feval) {
        const std::string src = sparse_source(sp);
        const std::string key = "sparse:" + std::to_string(std::hash<std::string>{}(src));
        ctx->sp_feval = jit_compile(ctx->device, key, src, "pcl_eval_sparse_kernel", true);
        if (!ctx->sp_feval) {
            ctx->sp_failed = 1;
            if (int rc = jit_fell_back(ctx, "residual"); rc != PCL_ENOTIMPL) return rc;
        }
    }
    if (!ctx->sp_feval) return PCL_ENOTIMPL;
    if (int rc = grow_scratch(ctx, &ctx->sp_gvals_cap, (long long)ctx->desc.batch * p.K, &ctx->dsp_gvals, (size_t)ctx->desc.batch * p.K * sp.nzp + 32)) return rc;
    // one wave per interval; the intervals are spread over the CUs first, then over the waves of a workgroup (<= 8)
    const long long ncu = std::max(ctx->n_cu, 1);
    int nw = (int)std::min<long long>(8, std::max<long long>(1, (items + ncu - 1) / ncu));
    long long grid = std::min<long long>((items + nw - 1) / nw, ncu);
    if (ctx->opt_grid > 0) grid = std::min<long long>(ctx->opt_grid, (items + nw - 1) / nw);
    const size_t ldse = (size_t)nw * (sp.n + 1) * sp.d * sizeof(double);
    void *args[] = {(void *)&p, (void *)&ctx->dsp_gvals, (void *)&ctx->dsp_pos_n, (void *)&ctx->dsp_coef_n};
    HIP_TRY(ctx, hipModuleLaunchKernel(ctx->sp_feval, (unsigned)grid, 1, 1, 64 * nw, 1, 1, (unsigned)ldse, ctx->stream, args, nullptr));
    ctx->last_kernel = 70;  // the pattern-compiled residual kernel
    ctx->last_n_stream = 0;
    return PCL_OK;
}

// residual only, any generators: the dedicated matrix-core kernel for unitary states
static int launch_eval_mfma(pcl_ctx *ctx, KParams &p) {
    typedef void (*kerne_t)(const KParams);
    const int wu = (ctx->uell_w <= 2 && ctx->n_upos <= 256 * PCL_NUE_EV) ? ctx->uell_w : -1;
    const bool spec = ctx->opt_specialize && p.d == 27;
    kerne_t ke = wu == 1 ? (spec ? (kerne_t)pcl_eval_kernel<1, 27> : (kerne_t)pcl_eval_kernel<1, 0>)
               : wu == 2 ? (spec ? (kerne_t)pcl_eval_kernel<2, 27> : (kerne_t)pcl_eval_kernel<2, 0>)
                         : (kerne_t)pcl_eval_kernel<-1, 0>;
    const size_t lde = (p.d & 1) ? (size_t)p.n : (size_t)p.LD;  // the kernel's leading dimension (2*odd)
    const size_t ldse = (lde * p.n + 4 * lde * 16 + 2 * (size_t)(p.m + 1) + 2) * sizeof(double) + 128;
    if (ldse > (size_t)ctx->max_lds) return PCL_ENOTIMPL;
    if (int rc = set_lds_attr(ctx, (const void *)ke, 5, ldse)) return rc;
    const long long items = (long long)p.batch * p.K;
    if (int rc = check_grid(ctx, items)) return rc;
    // two resident workgroups per CU measured best (three: 28 us per 8 trajectories, two: 21.5); every workgroup walks the
    // same number of intervals: grid = items / rounds
    const int per_cu = std::max(1, std::min(2, (int)((size_t)ctx->max_lds / ldse)));
    const long long ge = balanced_grid(items, (long long)per_cu * std::max(ctx->n_cu, 1), ctx->opt_grid);
    ctx->last_kernel = 60 + ((spec && wu > 0) ? 1 : 0);
    ctx->last_n_stream = 0;
    hipLaunchKernelGGL(ke, dim3((unsigned)ge), dim3(256), ldse, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    return PCL_OK;
}

static int launch_fused_v12(pcl_ctx *ctx, KParams &p) {
    const bool want_jac = p.jac != nullptr;
    // auto: small Hilbert dimensions are launch- / latency-bound, one workgroup per item (kernel 1) beats the persistent
    // kernels there (measured: d <= 8 always, d <= 16 while all items fit one round of workgroups)
    const bool v1_auto = ctx->opt_kernel == 0 && (ctx->desc.d <= 8 || (ctx->desc.d <= 16 && (long long)ctx->win_count * ctx->K <= 512));
    const bool v2 = !v1_auto && (ctx->opt_kernel == 0 || ctx->opt_kernel >= 2) && ctx->opt_use_mfma != 0;
    const bool unitary = !ctx->vec && ctx->cols == ctx->desc.d;  // kernel 3 and the specialised instances assume X is n x d
    p.nc = choose_cols_per_slice(ctx, want_jac);
    auto bytes = [&]() { return v2 ? fused2_lds_bytes(p, want_jac, p.ell_lds != 0) : fused_lds_bytes(p, want_jac); };
    size_t lds = bytes();
    while (lds > (size_t)ctx->max_lds && p.nc > 1) {
        p.nc = (p.nc + 1) / 2;
        lds = bytes();
    }
    if (lds > (size_t)ctx->max_lds) return fail(ctx, PCL_ESHAPE, "fused kernel needs %zu B of LDS (> %d)", lds, ctx->max_lds);
    p.S = (p.cols + p.nc - 1) / p.nc;
    const long long grid = (long long)p.batch * p.K * p.S;
    if (int rc = check_grid(ctx, grid, "grid too large")) return rc;
    if (v2) {
        typedef void (*kern_t)(const KParams);
        const int wu = (ctx->uell_w <= 2 && ctx->n_upos <= 1024 && !ctx->desc.per_member_G0) ? ctx->uell_w : -1;
        kern_t kern = want_jac ? (wu == 1 ? (kern_t)pcl_fused_kernel_v2<true, 1, 0, 0, 0> : wu == 2 ? (kern_t)pcl_fused_kernel_v2<true, 2, 0, 0, 0> : (kern_t)pcl_fused_kernel_v2<true, -1, 0, 0, 0>)
                               : (wu == 1 ? (kern_t)pcl_fused_kernel_v2<false, 1, 0, 0, 0> : wu == 2 ? (kern_t)pcl_fused_kernel_v2<false, 2, 0, 0, 0> : (kern_t)pcl_fused_kernel_v2<false, -1, 0, 0, 0>);
        // shape-specialised instance (BASELINE config 3/4/5: three 3-level transmons, d = 27, six drives, 3-column slices)
        if (want_jac && unitary && wu == 1 && p.d == 27 && p.m == 6 && p.nc == 3 && ctx->opt_specialize) kern = (kern_t)pcl_fused_kernel_v2<true, 1, 27, 6, 3>;
        ctx->last_n_stream = 0;
        ctx->last_kernel = 20 + ((unitary && wu == 1 && p.d == 27 && p.m == 6 && p.nc == 3 && ctx->opt_specialize && want_jac) ? 1 : 0);
        {
            int rc = set_lds_attr(ctx, (const void *)kern, want_jac ? 4 : 5, lds);  // wu is fixed per context
            if (rc != PCL_OK) return rc;
        }
        // persistent grid: as many workgroups as are resident at once
        const int per_cu = std::max(1, std::min(2, (int)((size_t)ctx->max_lds / lds)));
        const long long resident = (long long)per_cu * std::max(ctx->n_cu, 1);
        const long long g2 = ctx->opt_grid > 0 ? std::min<long long>(ctx->opt_grid, grid) : std::min(grid, resident);
        hipLaunchKernelGGL(kern, dim3((unsigned)g2), dim3(512), lds, ctx->stream, p);
    } else {
        const bool mf = ctx->opt_use_mfma != 0;
        auto kern = want_jac ? (mf ? pcl_fused_kernel<true, true> : pcl_fused_kernel<true, false>)
                             : (mf ? pcl_fused_kernel<false, true> : pcl_fused_kernel<false, false>);
        int rc = set_lds_attr(ctx, (const void *)kern, (want_jac ? 0 : 2) + (mf ? 0 : 1), lds);
        if (rc != PCL_OK) return rc;
        ctx->last_kernel = 10;
        ctx->last_n_stream = 0;
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, ctx->stream, p);
    }
    HIP_TRY(ctx, hipGetLastError());
    return PCL_OK;
}

static int launch_fused(pcl_ctx *ctx, const double *Z, double *delta, double *jac, bool compact) {
    ON_DEVICE(ctx);
    if (int rc = check_device_error(ctx, "pcl_eval / pcl_jac")) return rc;
    if (ctx->var) {
        if (compact) TRY(require(ctx, FEAT_COMPACT, "the compact Jacobian"));  // (every other kind is refused at the entry point, or takes the host calls' full route)
        return var_launch_fused(ctx, Z, delta, jac, compact && jac);
    }
    if (int rc = resolve_order(ctx, nullptr, "pcl_eval / pcl_jac")) return rc;
    KParams p;
    fill_params(ctx, p);
    p.Z = window_Z(ctx, Z);
    p.delta = delta;
    p.jac = jac;
    p.compact = compact ? 1 : 0;
    p.jac_per = compact ? jac_per_compact(ctx) : jac_per_full(ctx);
    const bool want_jac = jac != nullptr;
    if (ctx->large_exp) {
        if (want_jac && compact) return launch_large_exp(ctx, p, true, LE_COMPACT);
        // the payload-fused call (pcl_eval_jac_merit_dev, option large_exp_reduce): every member, so that the partial sums are numbered as the finish kernel reads them
        if (want_jac && ctx->large_exp_reduce && merit_call(ctx, p)) {
            if (!ctx->dmcols) HIP_TRY(ctx, hipMalloc((void **)&ctx->dmcols, (size_t)ctx->desc.batch * p.K * p.cols * (p.m + 2) * sizeof(double)));
            p.mpart = ctx->dmcols;
            p.mlam = ctx->merit_lam;
            ctx->merit_fused = 1;
            return launch_large_exp(ctx, p, true, LE_MERIT);
        }
        return launch_large_exp(ctx, p, want_jac);
    }
    if (ctx->large) {
        if (want_jac && compact) return launch_pade_large(ctx, p, true, PL_COMPACT);
        // the payload-fused call (pcl_eval_jac_merit_dev, option large_reduce): every member, so that the partial sums are numbered as the finish kernel reads them
        if (want_jac && ctx->large_reduce && merit_call(ctx, p)) {
            if (!ctx->dmcols) HIP_TRY(ctx, hipMalloc((void **)&ctx->dmcols, (size_t)ctx->desc.batch * p.K * p.cols * (p.m + 2) * sizeof(double)));
            p.mpart = ctx->dmcols;
            p.mlam = ctx->merit_lam;
            ctx->merit_fused = 1;
            return launch_pade_large(ctx, p, true, PL_MERIT);
        }
        return launch_pade_large(ctx, p, want_jac);
    }
    if (ctx->exp) return launch_fused_exp(ctx, p);
    // streaming stores of the Jacobian blocks (auto): write-through while the launch's values fit the infinity cache with room to
    // spare (one trajectory of config 3: 133 MB), plain write-back above (see store2)
    if (ctx->opt_nt < 0 && want_jac && !compact && (long long)ctx->win_count * ctx->K * jac_per_full(ctx) * 8 <= (192LL << 20)) p.nt = 2;
    // kernel_version 4: the pattern-compiled fused kernel (sparse iso generators, any order).  auto: every order -- at order 4 it measures
    // 27.2 against 27.4 us for one trajectory, 184 against 190 us for 8 and 7.8 against 10.6 us per evaluation for the compact launches
    // of the host-delivery path (kernel 3 on the same box), and one kernel family behind every entry point keeps the full and the compact
    // values bitwise equal.  Kernel 3 keeps the payload-fused call and contexts that set its own switches.
    const bool v4_auto = ctx->opt_kernel == 0 && (ctx->desc.pade_order != 4 || (ctx->opt_stream_wg < 0 && ctx->opt_use_mfma != 0)) && !ctx->opt_general &&
                         ctx->opt_general_version == 0;
    if (want_jac && (ctx->opt_kernel == 4 || v4_auto)) {
        // the payload-fused call (pcl_eval_jac_merit_dev): kernel 4's otherwise idle writer wave forms the payload's dot products per
        // state column while the item's vectors are in their tiles -- any order
        const int rc = launch_fused_v4(ctx, p, compact, merit_call(ctx, p));
        if (rc != PCL_ENOTIMPL) return rc;
        if (ctx->opt_kernel == 4) return fail(ctx, PCL_ESHAPE, "kernel_version=4 needs sparse exact-iso generators of a unitary problem (9 <= d, tiles within LDS), 1..6 drives and jit=1 (%s)", g_jit_note.c_str());
    }
#ifdef PCL_LAB
    if (ctx->res_capture) return fail(ctx, PCL_ESHAPE, "pcl_resident_start: the resident evaluator is kernel 4's (sparse exact-iso generators of a unitary problem, 9 <= d, tiles within LDS, 1..6 drives, jit = 1; kernel_version 0 or 4)");
#endif
    if (p.nt == 3) p.nt = 2;  // (the mixed mode is kernel 4's)
    // residual only on the same products (eval_kernel 3; auto: every order -- measured against the other residual kernels)
    if (!want_jac && (ctx->opt_eval_kernel == 3 || (ctx->opt_eval_kernel == 0 && ctx->opt_kernel == 0 && !ctx->opt_general && ctx->opt_general_version == 0))) {
        const int rc = launch_eval_v4(ctx, p);
        if (rc != PCL_ENOTIMPL) return rc;
        if (ctx->opt_eval_kernel == 3) return fail(ctx, PCL_ESHAPE, "eval_kernel=3 needs sparse exact-iso generators of a unitary problem (9 <= d, tiles within LDS), 1..6 drives and jit=1 (%s)", g_jit_note.c_str());
    }
    if ((ctx->opt_kernel == 5 || (ctx->opt_kernel == 0 && !ctx->opt_general && ctx->opt_general_version == 0 && (ctx->n <= 8 || !want_jac))) && ctx->n <= 16 &&
        ctx->cols <= 8 && p.m <= 8 && (p.m == 0 || ctx->dGjd))  // (the payload-fused call: this kernel + the separate payload kernels)
        return launch_fused_small(ctx, p);
    if (ctx->opt_kernel == 5) return fail(ctx, PCL_ESHAPE, "kernel_version=5 (the small-system kernel) needs n <= 16 rows, at most 8 state columns and at most 8 drives (n = %d, cols = %d, m = %d)", ctx->n, ctx->cols, p.m);
    if (ctx->desc.pade_order != 4 || ctx->opt_general || ctx->vec) return launch_pade_general(ctx, p, want_jac);
    p.ell_lds = ell_fits_lds(ctx) ? 1 : 0;
    if (int rc = launch_fused_v3(ctx, p); rc != PCL_ENOTIMPL) return rc;
    if (!want_jac && (ctx->opt_eval_kernel == 2 || (ctx->opt_eval_kernel == 0 && (long long)p.batch * p.K > ctx->n_cu)) && ctx->sp_plan && !ctx->sp_failed && ctx->opt_jit &&
        (ctx->opt_kernel == 0 || ctx->opt_kernel >= 3)) {
        if (int rc = launch_eval_sparse(ctx, p); rc != PCL_ENOTIMPL) return rc;
        if (ctx->opt_eval_kernel == 2) return fail(ctx, PCL_ESHAPE, "eval_kernel=2: the pattern-compiled kernel is not available (%s)", g_jit_note.c_str());
    } else if (!want_jac && ctx->opt_eval_kernel == 2) {
        return fail(ctx, PCL_ESHAPE, "eval_kernel=2 needs sparse iso generators, a unitary problem with 9 <= d <= 32, 1..6 drives and jit=1");
    }
    if (!want_jac && ctx->opt_use_mfma != 0 && !ctx->vec && ctx->cols == ctx->desc.d && ctx->desc.d >= 9 && (ctx->opt_kernel == 0 || ctx->opt_kernel >= 3)) {
        if (int rc = launch_eval_mfma(ctx, p); rc != PCL_ENOTIMPL) return rc;
    }
    return launch_fused_v12(ctx, p);
}
