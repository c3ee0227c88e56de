// pcl_host_variational.hpp -- part of piccolo_hip.hip (included there, in place, before pcl_create): batch_mode PCL_BATCH_VARIATIONAL, the
// variational (sensitivity) integrators VariationalUnitaryIntegrator / VariationalKetIntegrator (src/control/integrators.jl:234-264): creation and
// validation, structures, and the launches of pcl_kernel_variational.hpp.
#pragma once
#include "pcl_kernel_variational.hpp"
#include "pcl_kernel_var_rollout.hpp"
#include "pcl_kernel_var_exp.hpp"
#include "pcl_kernel_var_exp_hess.hpp"
#include "pcl_kernel_var_exp_hess_tiles.hpp"
#include "pcl_kernel_var_large.hpp"
#include "pcl_kernel_var_large_hess.hpp"
#include "pcl_kernel_var_large_rollout.hpp"
#include "pcl_kernel_var_large_exp.hpp"
#include "pcl_kernel_var_large_exp_hess.hpp"

// Values per interval: blocks (2 + 4 v) C n^2 (delta_0: -B+, B-; per variation: -B+, B-, -L+_i, L-_i), then the tails x_dim' (m + 1).
// PCL_BATCH_VARIATIONAL_EXP: blocks (1 + 2 v) C n^2 (delta_0: -E; per variation: -E, -L_i), the identity's diagonal x_dim', the tails x_dim' (m + 1).
static long long var_jac_per(const pcl_ctx *c) {
    if (c->vexp) return (1LL + 2LL * c->var) * c->cols * c->n * c->n + c->x_dim * (c->desc.n_drives + 2);
    return (2LL + 4LL * c->var) * c->cols * c->n * c->n + c->x_dim * (c->desc.n_drives + 1);
}

// Validation of a variational descriptor: every check runs before any device call; the message names the field.
// large_var: the descriptor carried PCL_LARGE_N | PCL_LARGE_VAR (generator dimensions up to PCL_LARGE_MAX_N on the Pade constraint)
static int var_validate(const pcl_desc *D, bool large_var) {  // (PCL_LARGE_VAR_EXP: the same limits)
    const int d = D->d, m = D->n_drives;
    if (D->batch < 2) return fail(nullptr, PCL_EINVAL, "pcl_create: batch=%d; PCL_BATCH_VARIATIONAL takes batch = 1 + v with v >= 1 variations", D->batch);
    if (D->per_member_G0 != 1)
        return fail(nullptr, PCL_EINVAL, "pcl_create: per_member_G0=%d; PCL_BATCH_VARIATIONAL takes per_member_G0 = 1 (G0[0] = G_drift, G0[i] = Gv_i)", D->per_member_G0);
    if (D->state_cols == PCL_STATE_VECTOR) return fail(nullptr, PCL_EINVAL, "pcl_create: state_cols=PCL_STATE_VECTOR is not supported by PCL_BATCH_VARIATIONAL");
    if (d < 1) return fail(nullptr, PCL_EINVAL, "pcl_create: d=%d", d);
    // a large variational context also takes 2 .. d - 1 kets: its one kernel and its rollout are planned per slice of state columns, whatever their count
    const bool kets = large_var && d > PCL_MAX_D && D->state_cols > 1 && D->state_cols < d;
    if (D->state_cols != 0 && D->state_cols != 1 && D->state_cols != d && !kets)
        return fail(nullptr, PCL_EINVAL, "pcl_create: state_cols=%d; PCL_BATCH_VARIATIONAL takes d (unitary, or 0) or 1 (ket), and with PCL_LARGE_N | PCL_LARGE_VAR at d > %d any count of kets up to d",
                    D->state_cols, PCL_MAX_D);
    if (m < 0) return fail(nullptr, PCL_EINVAL, "pcl_create: n_drives=%d", m);
    if (D->N < 2) return fail(nullptr, PCL_EINVAL, "pcl_create: N=%d; need N >= 2", D->N);
    if (D->batch_mode == PCL_BATCH_VARIATIONAL_EXP) {
        if (D->pade_order != PCL_ORDER_EXP)
            return fail(nullptr, PCL_EINVAL, "pcl_create: pade_order=%d with batch_mode = PCL_BATCH_VARIATIONAL_EXP; that batch_mode takes pade_order = PCL_ORDER_EXP (-1) only", D->pade_order);
    } else if (D->pade_order != 0 && D->pade_order != 2 && D->pade_order != 4 && D->pade_order != 6 && D->pade_order != 8 && D->pade_order != 10)
        return fail(nullptr, PCL_ENOTIMPL, "pcl_create: pade_order=%d; diagonal Pade orders 2, 4, 6, 8, 10 are implemented (0: chosen by pcl_set_order_policy)", D->pade_order);
    if (D->index_base != 0 && D->index_base != 1) return fail(nullptr, PCL_EINVAL, "pcl_create: index_base=%d; must be 0 or 1", D->index_base);
    if (D->global_dim < 0) return fail(nullptr, PCL_EINVAL, "pcl_create: global_dim=%lld", (long long)D->global_dim);
    if (!D->G0) return fail(nullptr, PCL_EINVAL, "pcl_create: G0 is NULL");
    if (m > 0 && !D->Gj) return fail(nullptr, PCL_EINVAL, "pcl_create: Gj is NULL");
    if (!D->x_offs) return fail(nullptr, PCL_EINVAL, "pcl_create: x_offs is NULL");
    const int cols = D->state_cols > 0 ? D->state_cols : d;
    const long long x_dim = 2LL * d * cols;
    for (int b = 0; b < D->batch; ++b) {
        if (D->x_offs[b] < 0 || D->x_offs[b] + x_dim > D->z_dim)
            return fail(nullptr, PCL_EINVAL, "pcl_create: x_offs[%d]=%d with x_dim=%lld does not fit z_dim=%d", b, D->x_offs[b], x_dim, D->z_dim);
        for (int a = 0; a < b; ++a)
            if (std::llabs((long long)D->x_offs[a] - D->x_offs[b]) < x_dim)
                return fail(nullptr, PCL_EINVAL, "pcl_create: x_offs[%d]=%d and x_offs[%d]=%d overlap (x_dim=%lld)", a, D->x_offs[a], b, D->x_offs[b], x_dim);
    }
    if (D->u_off < 0 || D->u_off + m > D->z_dim) return fail(nullptr, PCL_EINVAL, "pcl_create: u_off=%d with n_drives=%d outside the knot (z_dim=%d)", D->u_off, m, D->z_dim);
    if (D->dt_off < 0 || D->dt_off >= D->z_dim) return fail(nullptr, PCL_EINVAL, "pcl_create: dt_off=%d outside the knot (z_dim=%d)", D->dt_off, D->z_dim);
    for (int b = 0; b < D->batch; ++b) {
        const long long xo = D->x_offs[b];
        if ((D->u_off < xo + x_dim && xo < D->u_off + m) || (D->dt_off >= xo && D->dt_off < xo + x_dim))
            return fail(nullptr, PCL_EINVAL, "pcl_create: x_offs[%d]=%d overlaps u_off / dt_off", b, D->x_offs[b]);
    }
    // shapes the kernels take
    if (large_var && 2 * d > PCL_LARGE_MAX_N)
        return fail(nullptr, PCL_ESHAPE, "pcl_create: generator dimension %d exceeds %d, the most PCL_LARGE_N | PCL_LARGE_VAR serves: one n x n LDS tile would take %zu B of the 163840 B a workgroup can have (132096 B at n = %d)",
                    2 * d, PCL_LARGE_MAX_N, (size_t)((2 * d) | 1) * (2 * d) * sizeof(double), PCL_LARGE_MAX_N);
    if (d > PCL_MAX_D && !large_var) return fail(nullptr, PCL_ESHAPE, "pcl_create: d=%d exceeds %d (LDS-resident generator tiles)", d, PCL_MAX_D);
    if (D->batch - 1 > PCL_VAR_MAXV) return fail(nullptr, PCL_ESHAPE, "pcl_create: %d variations; PCL_BATCH_VARIATIONAL takes at most %d", D->batch - 1, PCL_VAR_MAXV);
    if (m > 24) return fail(nullptr, PCL_ESHAPE, "pcl_create: n_drives=%d exceeds 24", m);
    return PCL_OK;
}

// LDS of pcl_var_exp_kernel: five rotating n x n tiles, a sixth for G(u_k) where that fits (*g_lds).  (LD as lds_ld(n).)
static size_t var_exp_lds_bytes(int n, size_t max_lds, int *g_lds) {
    const size_t tile = (size_t)(((n + 3) & ~3) + 2) * n * sizeof(double), five = 5 * tile;
    const bool six = five + tile <= max_lds;
    if (g_lds) *g_lds = six ? 1 : 0;
    return six ? five + tile : five;
}

static int var_create(const pcl_desc *dsc, pcl_ctx **out, bool large_var_flag = false, bool large_var_exp_flag = false) {
    if (int rc = var_validate(dsc, large_var_flag)) return rc;
    const int d = dsc->d, m = dsc->n_drives, n = 2 * d, v = dsc->batch - 1;
    const int cols = dsc->state_cols > 0 ? dsc->state_cols : d;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, PCL_EHIP, "pcl_create: no HIP device available (%s); this library has no CPU path", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (dsc->device_id < 0 || dsc->device_id >= ndev) return fail(nullptr, PCL_EINVAL, "pcl_create: device_id %d of %d", dsc->device_id, ndev);
    pcl_ctx *ctx = new (std::nothrow) pcl_ctx();
    if (!ctx) return fail(nullptr, PCL_ENOMEM, "pcl_create: out of host memory");
    const size_t nn = (size_t)n * n;
    ctx->desc = *dsc;
    ctx->var = v;
    ctx->vexp = dsc->batch_mode == PCL_BATCH_VARIATIONAL_EXP ? 1 : 0;
    ctx->large_var = large_var_flag && n > 2 * PCL_MAX_D ? 1 : 0;  // (the flags at n <= 64: the ordinary variational context)
    ctx->large_var_exp = ctx->large_var && large_var_exp_flag ? 1 : 0;
    ctx->n = n;
    ctx->K = dsc->N - 1;
    ctx->cols = cols;
    ctx->var_xdc = (long long)n * cols;
    ctx->x_dim = ctx->var_xdc * (v + 1);  // the stacked state: B.x_dim of the reference
    ctx->x_offs.assign(dsc->x_offs, dsc->x_offs + v + 1);
    ctx->win_first = 0;
    ctx->win_count = 1;
    ctx->device = dsc->device_id;
    // the order policy looks at the lifted generator: G0' = var_G(G_drift, [Gv_i]), G_l' = I_{1+v} (x) G_l
    const int nl = (v + 1) * n;
    ctx->var_nl = nl;
    ctx->hG0.assign((size_t)nl * nl, 0.0);
    for (int b = 0; b <= v; ++b)
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) {
                ctx->hG0[(size_t)(b * n + i) + (size_t)nl * (b * n + j)] = dsc->G0[i + (size_t)n * j];
                if (b > 0) ctx->hG0[(size_t)(b * n + i) + (size_t)nl * j] = dsc->G0[(size_t)b * nn + i + (size_t)n * j];
            }
    ctx->hGj.assign((size_t)m * nl * nl, 0.0);
    for (int l = 0; l < m; ++l)
        for (int b = 0; b <= v; ++b)
            for (int j = 0; j < n; ++j)
                for (int i = 0; i < n; ++i) ctx->hGj[(size_t)l * nl * nl + (b * n + i) + (size_t)nl * (b * n + j)] = dsc->Gj[(size_t)l * nn + i + (size_t)n * j];
    ctx->desc.x_offs = nullptr;
    ctx->desc.G0 = ctx->desc.Gj = nullptr;
    // device tables: [G_drift | G_l (m) | Gv_i (v) | the same transposed], n x n column-major each
    const size_t nmat = 1 + (size_t)m + v;
    std::vector<double> tab(2 * nmat * nn);
    auto mat = [&](size_t i) -> const double * { return i == 0 ? dsc->G0 : i <= (size_t)m ? dsc->Gj + (i - 1) * nn : dsc->G0 + (i - m) * nn; };
    for (size_t t = 0; t < nmat; ++t)
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) {
                tab[t * nn + i + (size_t)n * j] = mat(t)[i + (size_t)n * j];
                tab[(nmat + t) * nn + i + (size_t)n * j] = mat(t)[j + (size_t)n * i];
            }
#define VAR_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t e2_ = (expr);                                                                   \
        if (e2_ != hipSuccess) {                                                                   \
            fail(nullptr, PCL_EHIP, "pcl_create: %s: %s", #expr, hipGetErrorString(e2_));          \
            pcl_destroy(ctx);                                                                      \
            return PCL_EHIP;                                                                       \
        }                                                                                          \
    } while (0)
    DeviceGuard dev_guard_(ctx->device);
    VAR_HIP(dev_guard_.err);
    hipDeviceProp_t prop;
    VAR_HIP(hipGetDeviceProperties(&prop, ctx->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fail(nullptr, PCL_EHIP, "pcl_create: device %d is %s; this library is built for gfx950 only", ctx->device, prop.gcnArchName);
        pcl_destroy(ctx);
        return PCL_EHIP;
    }
    ctx->max_lds = (int)prop.maxSharedMemoryPerMultiProcessor;
    ctx->n_cu = prop.multiProcessorCount;
    if (ctx->vexp && !ctx->large_var_exp && var_exp_lds_bytes(n, (size_t)ctx->max_lds, nullptr) > (size_t)ctx->max_lds) {
        fail(nullptr, PCL_ESHAPE, "pcl_create: PCL_BATCH_VARIATIONAL_EXP needs %zu B of LDS (> %d) for n=%d: five n x n tiles of %zu B (served up to n = 62)",
             var_exp_lds_bytes(n, (size_t)ctx->max_lds, nullptr), ctx->max_lds, n, var_exp_lds_bytes(n, (size_t)ctx->max_lds, nullptr) / 5);
        pcl_destroy(ctx);
        return PCL_ESHAPE;
    }
    VAR_HIP(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    // row-compressed (ELL) tables of the column role, [slot t][row i], padded with column 0 / value 0: G(u) on the union pattern of the drift
    // and the drives (a value table per matrix), then every drive, then every variation generator (each group padded to its widest row)
    std::vector<int> icol;
    std::vector<double> ival;
    auto pattern = [&](const std::vector<const double *> &mats) {
        std::vector<std::vector<int>> rows(n);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                bool nz = false;
                for (const double *A : mats) nz |= A[i + (size_t)n * j] != 0.0;
                if (nz) rows[i].push_back(j);
            }
        return rows;
    };
    auto width = [&](const std::vector<const double *> &mats) {
        int w = 1;
        for (const auto &r : pattern(mats)) w = std::max<int>(w, (int)r.size());
        return w;
    };
    auto append = [&](const std::vector<const double *> &mats, int w) {
        const auto rows = pattern(mats);
        const size_t c0 = icol.size(), v0 = ival.size();
        icol.resize(c0 + (size_t)w * n, 0);
        ival.resize(v0 + mats.size() * (size_t)w * n, 0.0);
        for (int i = 0; i < n; ++i)
            for (size_t t = 0; t < rows[i].size(); ++t) {
                icol[c0 + t * n + i] = rows[i][t];
                for (size_t a = 0; a < mats.size(); ++a) ival[v0 + (a * w + t) * n + i] = mats[a][i + (size_t)n * rows[i][t]];
            }
    };
    std::vector<const double *> gm{dsc->G0}, dm, vm;
    for (int l = 0; l < m; ++l) gm.push_back(dsc->Gj + (size_t)l * nn), dm.push_back(dsc->Gj + (size_t)l * nn);
    for (int b = 1; b <= v; ++b) vm.push_back(dsc->G0 + (size_t)b * nn);
    ctx->var_wG = width(gm);
    append(gm, ctx->var_wG);
    ctx->var_off_d = (long long)icol.size();
    ctx->var_voff_d = (long long)ival.size();
    ctx->var_wD = 1;
    for (const double *A : dm) ctx->var_wD = std::max(ctx->var_wD, width({A}));
    for (const double *A : dm) append({A}, ctx->var_wD);
    ctx->var_off_v = (long long)icol.size();
    ctx->var_voff_v = (long long)ival.size();
    ctx->var_wV = 1;
    for (const double *A : vm) ctx->var_wV = std::max(ctx->var_wV, width({A}));
    for (const double *A : vm) append({A}, ctx->var_wV);
    if (upload(ctx, &ctx->dvar_tab, tab) != PCL_OK || upload(ctx, &ctx->dvar_ecol, icol) != PCL_OK || upload(ctx, &ctx->dvar_eval, ival) != PCL_OK) {
        g_create_error = ctx->err;
        pcl_destroy(ctx);
        return PCL_EHIP;
    }
    if (ctx->large_var) {
        // the tables of pcl_var_large_kernel.  The drives as a plain large context has them, so that G(u_k) and the drive terms of component 0 go
        // through its operations: the union pattern with its coefficient table (build_G) and the rows [l][i][ell_w]; the variation generators in
        // rows of the same form, [b][i][vl_gw] (a dense Gv_i is a row of width n)
        std::vector<int> upos, ecol, gcol;
        std::vector<double> ucoef, evalv, gval;
        for (size_t pz = 0; pz < nn; ++pz) {
            bool any = false;
            for (int l = 0; l < m; ++l) any |= dsc->Gj[l * nn + pz] != 0.0;
            if (any) {
                upos.push_back((int)pz);
                for (int l = 0; l < m; ++l) ucoef.push_back(dsc->Gj[l * nn + pz]);
            }
        }
        ctx->n_upos = (int)upos.size();
        auto rows_of = [&](const double *A, int cnt, int floor_w, std::vector<int> &col, std::vector<double> &val) {
            int wd = floor_w;
            for (int t = 0; t < cnt; ++t)
                for (int i = 0; i < n; ++i) {
                    int c = 0;
                    for (int j = 0; j < n; ++j) c += A[t * nn + i + (size_t)n * j] != 0.0;
                    wd = std::max(wd, c);
                }
            col.assign((size_t)cnt * n * wd, 0);
            val.assign((size_t)cnt * n * wd, 0.0);
            for (int t = 0; t < cnt; ++t)
                for (int i = 0; i < n; ++i) {
                    size_t e = ((size_t)t * n + i) * wd;
                    for (int j = 0; j < n; ++j)
                        if (A[t * nn + i + (size_t)n * j] != 0.0) col[e] = j, val[e] = A[t * nn + i + (size_t)n * j], ++e;
                }
            return wd;
        };
        ctx->ell_w = rows_of(dsc->Gj, m, m > 0 ? 1 : 0, ecol, evalv);
        ctx->vl_gw = rows_of(dsc->G0 + nn, v, 1, gcol, gval);
        if (upload(ctx, &ctx->dupos, upos) != PCL_OK || upload(ctx, &ctx->ducoef, ucoef) != PCL_OK || upload(ctx, &ctx->dell_col, ecol) != PCL_OK ||
            upload(ctx, &ctx->dell_val, evalv) != PCL_OK || upload(ctx, &ctx->dvl_gcol, gcol) != PCL_OK || upload(ctx, &ctx->dvl_gval, gval) != PCL_OK) {
            g_create_error = ctx->err;
            pcl_destroy(ctx);
            return PCL_EHIP;
        }
    }
    VAR_HIP(hipHostMalloc((void **)&ctx->herr, 64, hipHostMallocMapped));
    *ctx->herr = 0;
    VAR_HIP(hipHostGetDevicePointer((void **)&ctx->derr, ctx->herr, 0));
#undef VAR_HIP
    *out = ctx;
    return PCL_OK;
}

// Rows knot-major over the stacked state: k x_dim' + b x_dim + c n + i (the reference's B.dim = x_dim' (N - 1)).
template <class I>
static int var_jac_structure(const pcl_ctx *ctx, I *rows, I *cols) {
    const pcl_desc &D = ctx->desc;
    const long long n = ctx->n, C = ctx->cols, m = D.n_drives, xdc = ctx->var_xdc, xd = ctx->x_dim, zd = D.z_dim, base = D.index_base;
    const long long per = var_jac_per(ctx);
    const int v = ctx->var;
    for (long long k = 0; k < ctx->K; ++k) {
        I *r = rows + k * per, *c = cols + k * per;
        long long p = 0;
        auto block = [&](int brow, int bcol, int knot) {  // I_C (x) (n x n) block: rows of component brow, state columns of component bcol at knot
            const long long r0 = k * xd + brow * xdc + base, c0 = (k + knot) * zd + ctx->x_offs[bcol] + base;
            for (long long cc = 0; cc < C; ++cc)
                for (long long j = 0; j < n; ++j)
                    for (long long i = 0; i < n; ++i, ++p) {
                        r[p] = (I)(r0 + cc * n + i);
                        c[p] = (I)(c0 + cc * n + j);
                    }
        };
        block(0, 0, 0);
        if (!ctx->vexp) block(0, 0, 1);
        for (int b = 1; b <= v; ++b) {
            block(b, b, 0);
            if (!ctx->vexp) block(b, b, 1);
            block(b, 0, 0);
            if (!ctx->vexp) block(b, 0, 1);
        }
        if (ctx->vexp)  // d delta / d X'_{k+1} = I: its diagonal, after the blocks
            for (long long q = 0; q < xd; ++q, ++p) {
                r[p] = (I)(k * xd + q + base);
                c[p] = (I)((k + 1) * zd + ctx->x_offs[q / xdc] + q % xdc + base);
            }
        for (int b = 0; b <= v; ++b)
            for (long long cc = 0; cc < C; ++cc)
                for (long long l = 0; l <= m; ++l) {
                    const long long col = k * zd + (l < m ? D.u_off + l : D.dt_off) + base;
                    for (long long i = 0; i < n; ++i, ++p) {
                        r[p] = (I)(k * xd + b * xdc + cc * n + i + base);
                        c[p] = (I)col;
                    }
                }
    }
    return PCL_OK;
}

// Today's segment order (pcl_hess_structure) over the stacked state: entry q of the state is component q / x_dim, offset q % x_dim.
// PCL_BATCH_VARIATIONAL_EXP (option var_exp_hess): the first five segments -- nothing involves X'_{k+1}.
template <class I>
static int var_hess_structure(const pcl_ctx *ctx, I *rows, I *cols) {
    const pcl_desc &D = ctx->desc;
    const long long m = D.n_drives, xd = ctx->x_dim, xdc = ctx->var_xdc, zd = D.z_dim, base = D.index_base;
    const long long per = hess_per(ctx);
    for (long long k = 0; k < ctx->K; ++k) {
        I *r = rows + k * per, *c = cols + k * per;
        const long long uk = k * zd + D.u_off, hk = k * zd + D.dt_off;
        auto xk = [&](long long q, int knot) { return (k + knot) * zd + ctx->x_offs[q / xdc] + q % xdc; };
        long long p = 0;
        auto put = [&](long long a, long long bb) {
            r[p] = (I)(std::max(a, bb) + base);
            c[p] = (I)(std::min(a, bb) + base);
            ++p;
        };
        for (long long i = 0; i < m; ++i)
            for (long long j = 0; j <= i; ++j) put(uk + i, uk + j);
        for (long long j = 0; j < m; ++j) put(hk, uk + j);
        put(hk, hk);
        for (long long l = 0; l < m; ++l)
            for (long long q = 0; q < xd; ++q) put(uk + l, xk(q, 0));
        for (long long q = 0; q < xd; ++q) put(hk, xk(q, 0));
        if (ctx->vexp) continue;
        for (long long l = 0; l < m; ++l)
            for (long long q = 0; q < xd; ++q) put(xk(q, 1), uk + l);
        for (long long q = 0; q < xd; ++q) put(xk(q, 1), hk);
    }
    return PCL_OK;
}

static void var_fill(const pcl_ctx *ctx, VarParams &p) {
    memset(&p, 0, sizeof p);
    const pcl_desc &D = ctx->desc;
    const int m = D.n_drives, v = ctx->var;
    const size_t nn = (size_t)ctx->n * ctx->n, nmat = 1 + (size_t)m + v;
    p.G0 = ctx->dvar_tab;
    p.Gj = ctx->dvar_tab + nn;
    p.Gv = ctx->dvar_tab + (1 + m) * nn;
    p.G0T = ctx->dvar_tab + nmat * nn;
    p.GjT = p.G0T + nn;
    p.GvT = p.G0T + (1 + m) * nn;
    p.gcol = ctx->dvar_ecol;
    p.gval = ctx->dvar_eval;
    p.dcol = ctx->dvar_ecol + ctx->var_off_d;
    p.dval = ctx->dvar_eval + ctx->var_voff_d;
    p.vcol = ctx->dvar_ecol + ctx->var_off_v;
    p.vval = ctx->dvar_eval + ctx->var_voff_v;
    p.wG = ctx->var_wG;
    p.wD = ctx->var_wD;
    p.wV = ctx->var_wV;
    p.jper = var_jac_per(ctx);
    p.hper = hess_per(ctx);
    p.n = ctx->n;
    p.cols = ctx->cols;
    p.m = m;
    p.K = ctx->K;
    p.z_dim = D.z_dim;
    p.u_off = D.u_off;
    p.dt_off = D.dt_off;
    for (int b = 0; b <= v; ++b) p.xo[b] = ctx->x_offs[b];
    const int order = D.pade_order, q = order / 2;
    double f[12];
    f[0] = 1.0;
    for (int i = 1; i < 12; ++i) f[i] = f[i - 1] * i;
    for (int j = 0; j <= q; ++j) p.c[j] = f[2 * q - j] * f[q] / (f[2 * q] * f[j] * f[q - j]);
}

template <int V, int Q>
static const void *var_fused_fn(bool jac) {
    return jac ? (const void *)pcl_var_fused_kernel<V, Q, true> : (const void *)pcl_var_fused_kernel<V, Q, false>;
}
static const void *var_pick_fused(int v, int q, bool jac) {
#define VAR_Q(V)                                            \
    switch (q) {                                            \
        case 1: return var_fused_fn<V, 1>(jac);             \
        case 2: return var_fused_fn<V, 2>(jac);             \
        case 3: return var_fused_fn<V, 3>(jac);             \
        case 4: return var_fused_fn<V, 4>(jac);             \
        case 5: return var_fused_fn<V, 5>(jac);             \
    }
    if (v == 1) { VAR_Q(1) }
    if (v == 2) { VAR_Q(2) }
#undef VAR_Q
    return nullptr;
}
static const void *var_pick_hess(int v, int q) {
#define VAR_Q(V)                                                     \
    switch (q) {                                                     \
        case 1: return (const void *)pcl_var_hess_kernel<V, 1>;      \
        case 2: return (const void *)pcl_var_hess_kernel<V, 2>;      \
        case 3: return (const void *)pcl_var_hess_kernel<V, 3>;      \
        case 4: return (const void *)pcl_var_hess_kernel<V, 4>;      \
        case 5: return (const void *)pcl_var_hess_kernel<V, 5>;      \
    }
    if (v == 1) { VAR_Q(1) }
    if (v == 2) { VAR_Q(2) }
#undef VAR_Q
    return nullptr;
}

static int var_set_lds(pcl_ctx *ctx, const void *f, size_t lds) {
    if (lds > (size_t)ctx->max_lds) return fail(ctx, PCL_ESHAPE, "variational kernel: %zu bytes of LDS exceed the %d of a CU", lds, ctx->max_lds);
    HIP_TRY(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return PCL_OK;
}

// Work split of the fused launch: block workgroups per interval (each folds the powers, then streams a contiguous range of the C copies) and column
// workgroups (eight waves, one state column each).  Auto: every column its own wave; ONE block workgroup per interval, so the powers are folded
// once -- measured at config 3 (N = 100): 137 / 134 / 142 / 219 us for 1 / 2 / 7 / 27 block workgroups at order 4 (v = 1), 208 / 281 / 425 / 895
// at order 10 (profiles/variational_bench_line.json).  Options var_block_wgs / var_col_wgs override; every split gives the same bits.
static int var_split_blocks(const pcl_ctx *ctx) {
    const int C = ctx->cols;
    const int a = ctx->opt_var_blocks > 0 ? (int)ctx->opt_var_blocks : 1;
    return std::max(1, std::min(a, C));
}
static int var_split_cols(const pcl_ctx *ctx) {
    const int C = ctx->cols, w = PCL_VAR_THREADS / 64;
    const int a = ctx->opt_var_cols > 0 ? (int)ctx->opt_var_cols : (C + w - 1) / w;
    return std::max(1, std::min(a, C));
}

// PCL_BATCH_VARIATIONAL_EXP (pcl_kernel_var_exp.hpp): the preparation launch (G(u_k) and its norm per interval), then one workgroup per
// (interval, variation, drive) for residual + Jacobian, per (interval, variation) for the residual alone.
static int var_exp_launch(pcl_ctx *ctx, const double *Z, double *delta, double *vals, bool compact) {
    const pcl_desc &D = ctx->desc;
    const int n = ctx->n, m = D.n_drives, v = ctx->var;
    const size_t nn = (size_t)n * n;
    VarExpParams p;
    memset(&p, 0, sizeof p);
    int g_lds = 0;
    const size_t lds = var_exp_lds_bytes(n, (size_t)ctx->max_lds, &g_lds);
    const bool jac = vals != nullptr;
    const long long grid = (long long)ctx->K * v * (jac ? std::max(m, 1) : 1);
    if (grid > 0x7fffffffLL) return fail(ctx, PCL_ESHAPE, "pcl_eval / pcl_jac: %lld workgroups exceed the grid limit", grid);
    const long long cap = (long long)ctx->K * ((long long)nn + 2);
    if (int rc = grow_scratch(ctx, &ctx->exph_cap, cap, &ctx->dexph, (size_t)cap)) return rc;
    p.Z = Z;
    p.delta = delta;
    p.vals = vals;
    p.G0 = ctx->dvar_tab;
    p.Gj = ctx->dvar_tab + nn;
    p.Gv = ctx->dvar_tab + (1 + m) * nn;
    p.ws = ctx->dexph;
    p.jper = compact ? jac_per_compact(ctx) : var_jac_per(ctx);
    p.compact = compact ? 1 : 0;
    p.n = n;
    p.LD = ((n + 3) & ~3) + 2;
    p.cols = ctx->cols;
    p.m = m;
    p.K = ctx->K;
    p.v = v;
    p.z_dim = D.z_dim;
    p.u_off = D.u_off;
    p.dt_off = D.dt_off;
    p.g_lds = g_lds;
    for (int b = 0; b <= v; ++b) p.xo[b] = ctx->x_offs[b];
    hipLaunchKernelGGL(pcl_var_exp_prep_kernel, dim3((unsigned)ctx->K), dim3(256), 0, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    const void *f = jac ? (const void *)pcl_var_exp_kernel<true> : (const void *)pcl_var_exp_kernel<false>;
    if (int rc = var_set_lds(ctx, f, lds)) return rc;
    const unsigned threads = n > 32 ? 512 : 256;  // (as the exponential kernels: a pair of output tiles per wave)
    void *args[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(f, dim3((unsigned)grid), dim3(threads), args, lds, ctx->stream));
    ctx->last_kernel = jac ? (compact ? 112 : 110) : 111;  // the variational exponential kernel: fused | residual only | compact
    return PCL_OK;
}

// The Hessian of the Lagrangian of PCL_BATCH_VARIATIONAL_EXP (option var_exp_hess; pcl_kernel_var_exp_hess.hpp).  The octuple kernel rotates nine
// n x LD tiles (eight and the scratch) and G(u_k) takes a tenth where that fits; the quadruple kernel five, a sixth, and its reduction words.
static size_t var_exp_hess_tile_bytes(const pcl_ctx *ctx) { return (size_t)lds_ld(ctx->n) * ctx->n * sizeof(double); }
static size_t var_exp_hess_lds_bytes(const pcl_ctx *ctx, bool oct, int *g_lds) {
    const size_t tile = var_exp_hess_tile_bytes(ctx), base = oct ? 9 * tile : 5 * tile + 16 * sizeof(double);
    const bool g = base + tile <= (size_t)ctx->max_lds;
    if (g_lds) *g_lds = g ? 1 : 0;
    return g ? base + tile : base;
}
// The same octuple with four tiles in the workspace (option var_exp_hess_tiles; pcl_kernel_var_exp_hess_tiles.hpp): T, Ta, Tb, Tc and the scratch
// stay resident, G(u_k) takes a sixth tile where that fits.
static size_t var_exp_hess_ws_lds_bytes(const pcl_ctx *ctx, int *g_lds) {
    const size_t tile = var_exp_hess_tile_bytes(ctx), base = 5 * tile;
    const bool g = base + tile <= (size_t)ctx->max_lds;
    if (g_lds) *g_lds = g ? 1 : 0;
    return g ? base + tile : base;
}
static long long var_exp_hess_part_per(const pcl_ctx *ctx) {
    const long long m = ctx->desc.n_drives;
    return (m + 1) * (m + 2) / 2 + (m + 1) * ctx->var_xdc;
}
// option var_exp_hess = 1: the shape check, then the workspace (allocated here, on first use, not by pcl_create)
static int var_exp_hess_enable(pcl_ctx *ctx) {
    const size_t need = var_exp_hess_lds_bytes(ctx, true, nullptr);
    // the plan: nine LDS tiles, or five and four in the workspace (var_exp_hess_tiles = 2: always; 1: where nine do not fit)
    const bool ws_plan = ctx->opt_vexph_tiles == 2 || (ctx->opt_vexph_tiles == 1 && need > (size_t)ctx->max_lds);
    if (!ws_plan && need > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "var_exp_hess = 1: the octuple chain of third Frechet derivatives needs %zu B of LDS (> %d) for n=%d: nine n x n tiles of %zu B (option var_exp_hess_tiles = 1 keeps four of them in the workspace)",
                    need, ctx->max_lds, ctx->n, var_exp_hess_tile_bytes(ctx));
    if (ws_plan && var_exp_hess_ws_lds_bytes(ctx, nullptr) > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "var_exp_hess = 1 with var_exp_hess_tiles = %d: the five resident tiles of the octuple chain need %zu B of LDS (> %d) for n=%d: n x n tiles of %zu B",
                    ctx->opt_vexph_tiles, var_exp_hess_ws_lds_bytes(ctx, nullptr), ctx->max_lds, ctx->n, var_exp_hess_tile_bytes(ctx));
    // the last phase keeps two n x cols products per spent tile, and N_0 .. N_v in three pieces
    if (2 * ctx->cols > ctx->n || ctx->var > 2)
        return fail(ctx, PCL_ESHAPE, "var_exp_hess = 1: %d state columns and %d variations; the kernel's last phase takes cols <= n / 2 = %d and at most 2 variations", ctx->cols, ctx->var, ctx->n / 2);
    if (!ctx->dvexph) {
        ON_DEVICE(ctx);
        const size_t nn = (size_t)ctx->n * ctx->n;
        const size_t ws = (size_t)ctx->K * ((2 + ctx->var) * nn + 2), part = (size_t)ctx->K * (1 + ctx->var) * (size_t)var_exp_hess_part_per(ctx);
        HIP_TRY(ctx, hipMalloc((void **)&ctx->dvexph, ws * sizeof(double)));
        hipError_t e = hipMalloc((void **)&ctx->dvexph_part, part * sizeof(double));
        if (e != hipSuccess) {
            (void)hipFree(ctx->dvexph);
            ctx->dvexph = nullptr;
            HIP_TRY(ctx, e);
        }
    }
    if (ws_plan && !ctx->dvexph_tiles) {  // the homes of Tab, Tac, Tbc, Tabc: 4 n^2 doubles per octuple workgroup
        ON_DEVICE(ctx);
        const size_t homes = (size_t)ctx->K * ctx->var * std::max(ctx->desc.n_drives, 1) * 4 * (size_t)ctx->n * ctx->n;
        HIP_TRY(ctx, hipMalloc((void **)&ctx->dvexph_tiles, homes * sizeof(double)));
    }
    ctx->vexph_ws = ws_plan ? 1 : 0;
    ctx->var_exp_hess = 1;
    return PCL_OK;
}
// option var_exp_hess_tiles: read by var_exp_hess_enable, so it takes effect when var_exp_hess is next set to 1; another value while that
// option is on is refused
static int var_exp_hess_set_tiles(pcl_ctx *ctx, int64_t v) {
    if (v < 0 || v > 2) return fail(ctx, PCL_EINVAL, "var_exp_hess_tiles must be 0, 1 or 2");
    if (v && !ctx->vexp)
        return fail(ctx, PCL_EINVAL, "var_exp_hess_tiles = %d needs a variational context of the exponential constraint (PCL_BATCH_VARIATIONAL_EXP)", (int)v);
    if (ctx->var_exp_hess && v != ctx->opt_vexph_tiles)
        return fail(ctx, PCL_EINVAL, "var_exp_hess_tiles cannot change while var_exp_hess = 1 (it is %d): set var_exp_hess = 0 first", ctx->opt_vexph_tiles);
    ctx->opt_vexph_tiles = (int)v;
    return PCL_OK;
}
static int var_exp_launch_hess(pcl_ctx *ctx, const double *Z, const double *mu, double *hess) {
    ON_DEVICE(ctx);
    if (!ctx->var_exp_hess || !ctx->dvexph) return fail(ctx, PCL_EINVAL, "pcl_hess: option var_exp_hess is off");
    const pcl_desc &D = ctx->desc;
    const int n = ctx->n, m = D.n_drives, v = ctx->var, ml = std::max(m, 1);
    const size_t nn = (size_t)n * n;
    VarExpHessParams p;
    memset(&p, 0, sizeof p);
    int g_quad = 0, g_oct = 0;
    const bool ws_plan = ctx->vexph_ws != 0;
    if (ws_plan && !ctx->dvexph_tiles) return fail(ctx, PCL_EINVAL, "pcl_hess: the workspace of option var_exp_hess_tiles is missing");
    const size_t lds_quad = var_exp_hess_lds_bytes(ctx, false, &g_quad);
    const size_t lds_oct = ws_plan ? var_exp_hess_ws_lds_bytes(ctx, &g_oct) : var_exp_hess_lds_bytes(ctx, true, &g_oct);
    const long long grid = (long long)ctx->K * v * ml;
    p.pper = var_exp_hess_part_per(ctx);
    const long long fin = ((long long)ctx->K * p.pper + 255) / 256;
    if (grid > 0x7fffffffLL || fin > 0x7fffffffLL) return fail(ctx, PCL_ESHAPE, "pcl_hess: %lld workgroups exceed the grid limit", std::max(grid, fin));
    p.Z = Z;
    p.mu = mu;
    p.hess = hess;
    p.G0 = ctx->dvar_tab;
    p.Gj = ctx->dvar_tab + nn;
    p.Gv = ctx->dvar_tab + (1 + m) * nn;
    p.ws = ctx->dvexph;
    p.part = ctx->dvexph_part;
    p.hper = hess_per(ctx);
    p.wsper = (2LL + v) * (long long)nn + 2;
    p.n = n;
    p.LD = lds_ld(n);
    p.cols = ctx->cols;
    p.m = m;
    p.K = ctx->K;
    p.v = v;
    p.z_dim = D.z_dim;
    p.u_off = D.u_off;
    p.dt_off = D.dt_off;
    for (int b = 0; b <= v; ++b) p.xo[b] = ctx->x_offs[b];
    const size_t lds_prep = (nn + 32 + 64 + 2 * (size_t)(1 + v) * ctx->var_xdc) * sizeof(double);  // G(u_k), the drives, the column sums, X'_k and M'
    if (int rc = var_set_lds(ctx, (const void *)pcl_var_exp_hess_prep_kernel, lds_prep)) return rc;
    void *args[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel((const void *)pcl_var_exp_hess_prep_kernel, dim3((unsigned)ctx->K), dim3(256), args, lds_prep, ctx->stream));
    const unsigned threads = n > 32 ? 512 : 256;  // (as the sibling kernels: a pair of output tiles per wave)
    const void *fq = (const void *)pcl_var_exp_hess_kernel<false>;
    const void *fo = ws_plan ? (const void *)pcl_var_exp_hess_tiles_kernel : (const void *)pcl_var_exp_hess_kernel<true>;
    if (int rc = var_set_lds(ctx, fq, lds_quad)) return rc;
    if (int rc = var_set_lds(ctx, fo, lds_oct)) return rc;
    p.g_lds = g_quad;
    HIP_TRY(ctx, hipLaunchKernel(fq, dim3((unsigned)(ctx->K * ml)), dim3(threads), args, lds_quad, ctx->stream));
    p.g_lds = g_oct;
    void *args_ws[] = {&p, &ctx->dvexph_tiles};  // (the plan with tiles in the workspace: the homes as a second argument)
    HIP_TRY(ctx, hipLaunchKernel(fo, dim3((unsigned)grid), dim3(threads), ws_plan ? args_ws : args, lds_oct, ctx->stream));
    HIP_TRY(ctx, hipLaunchKernel((const void *)pcl_var_exp_hess_finish_kernel, dim3((unsigned)fin), dim3(256), args, 0, ctx->stream));
    ctx->last_hess_kernel = ws_plan ? 112 : 110;
    return PCL_OK;
}

// Large variational kernel (pcl_kernel_var_large.hpp; contexts created with PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR).  The plan, every
// branch from (n, C, m, v, intervals, CUs, options): LD = n | 1, 64 threads per 16-row tile of G; what the one tile leaves of the LDS is NB column
// blocks of LD doubles.  A chain unit takes nc state columns and mg drives of all 1 + v components: (1 + v) nc (2 + 2 (2 + mg)) blocks with the
// Jacobian (-S, D, and W | V | dW_l twice), (1 + v) nc 4 without.  Every group forms W and V again, so the widest nc at which ALL drives (option
// var_large_drives caps them) fit one group is taken (option cols_per_slice caps it); where not even one column takes them all, one column and the
// most drives that fit, evened over the groups (n = 128, v = 2: one column, one drive, 24 of the 29 blocks).  Launches of few intervals take
// narrower slices while the chain units stay within half a round of the CUs.  Panel units are workgroups of their own, (1 + v) pu of them: npc
// columns of the powers need three blocks each (P', Q, Q') and a thread owns at most PL_NP pairs; one unit per 16 columns at least (option
// general_slices: that many units per role at least).  Every split gives the same bits.
struct VarLargePlan : LargeTile {
    int sx, nc, mg, ngrp, chain_units, chain_blocks, npc, pu, U;
    size_t lds;
};
static void var_large_plan(const pcl_ctx *ctx, int n, int cols, int m, int v, bool jac, long long items, VarLargePlan &P) {
    const int comp = 1 + v;
    static_cast<LargeTile &>(P) = large_tile(ctx->max_lds, n, m);
    const int nc_cap = ctx->opt_cols_per_slice > 0 ? (int)std::min<int64_t>(ctx->opt_cols_per_slice, cols) : cols;
    const int mg_cap = jac && m > 0 ? (ctx->opt_var_large_drives > 0 ? (int)std::min<int64_t>(ctx->opt_var_large_drives, m) : m) : 0;
    auto blocks = [&](int nc, int mg) { return comp * nc * (jac ? 2 + 2 * (2 + mg) : 4); };
    P.nc = 1;
    for (int nc = nc_cap; nc > 1; --nc)
        if (blocks(nc, mg_cap) <= P.NB) {
            P.nc = nc;
            break;
        }
    P.mg = mg_cap;
    while (P.mg > 1 && blocks(P.nc, P.mg) > P.NB) --P.mg;  // (one column only: the most drives that fit)
    P.ngrp = mg_cap > 0 ? even_split(m, P.mg) : 1;  // even groups
    P.sx = (cols + P.nc - 1) / P.nc;
    const long long want_sx = ctx->n_cu / std::max(2 * items * P.ngrp, 1LL);
    if (want_sx > P.sx) P.sx = (int)std::min<long long>(want_sx, cols);
    P.nc = (cols + P.sx - 1) / P.sx;  // even slices
    P.sx = (cols + P.nc - 1) / P.nc;  // (no unit without work)
    P.chain_units = P.sx * P.ngrp;
    P.chain_blocks = blocks(P.nc, P.mg);
    P.npc = P.pu = 0;
    if (jac) {
        auto fits = [&](int pu) {
            const int npc = (n + pu - 1) / pu;
            return 3 * npc <= P.NB && ((long long)n * npc + 1) / 2 <= (long long)PL_NP * P.threads;
        };
        P.pu = 1;
        while (P.pu < n && !fits(P.pu)) ++P.pu;
        const long long want = ctx->opt_general_slices > 0 ? ctx->opt_general_slices : (n + 15) / 16;
        P.pu = (int)std::max<long long>(P.pu, std::min<long long>(want, n));
        P.npc = (n + P.pu - 1) / P.pu;
        P.pu = (n + P.npc - 1) / P.npc;  // (no unit without work)
    }
    P.U = P.chain_units + comp * P.pu;
    P.lds = (size_t)(P.fixed + (long long)P.LD * std::max(P.chain_blocks, 3 * P.npc)) * sizeof(double);
}
static int var_large_launch(pcl_ctx *ctx, const double *Z, double *delta, double *vals) {
    const pcl_desc &D = ctx->desc;
    const int n = ctx->n, m = D.n_drives, v = ctx->var;
    const bool jac = vals != nullptr;
    VarLargePlan P;
    var_large_plan(ctx, n, ctx->cols, m, v, jac, ctx->K, P);
    if (P.lds > (size_t)ctx->max_lds || P.chain_blocks > P.NB)
        return fail(ctx, PCL_ESHAPE, "the large variational kernel needs %zu B of LDS (> %d) for n = %d, m = %d, v = %d", P.lds, ctx->max_lds, n, m, v);
    KParams p;
    memset(&p, 0, sizeof p);
    fill_pade(p, D.pade_order);
    p.Z = Z;
    p.delta = delta;
    p.jac = vals;
    p.G0 = ctx->dvar_tab;
    p.upos = ctx->dupos;
    p.ucoef = ctx->ducoef;
    p.n_upos = ctx->n_upos;
    p.ell_val = ctx->dell_val;
    p.ell_col = ctx->dell_col;
    p.ell_w = ctx->ell_w;
    p.x_off0 = -1;
    p.jac_per = var_jac_per(ctx);
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
    p.nt = ctx->opt_nt == 1 ? 1 : 0;  // (plain or nontemporal block stores)
    p.lds_doubles = (int)(P.lds / sizeof(double));
    VarLargeParams w;
    memset(&w, 0, sizeof w);
    w.Gv = ctx->dvar_tab + (size_t)(1 + m) * n * n;
    w.gv_val = ctx->dvl_gval;
    w.gv_col = ctx->dvl_gcol;
    w.gv_w = ctx->vl_gw;
    w.v = v;
    for (int b = 0; b <= v; ++b) w.xo[b] = ctx->x_offs[b];
    w.sx = P.sx;
    w.mg = P.mg;
    w.ngrp = P.ngrp;
    w.npc = P.npc;
    w.pu = P.pu;
    const long long grid = (long long)ctx->K * P.U;
    if (grid > 0x7fffffffLL) return fail(ctx, PCL_ESHAPE, "pcl_eval / pcl_jac: %lld workgroups exceed the grid limit", grid);
    const void *f = jac ? (const void *)pcl_var_large_kernel<true> : (const void *)pcl_var_large_kernel<false>;
    if (int rc = var_set_lds(ctx, f, P.lds)) return rc;
    void *args[] = {&p, &w};
    HIP_TRY(ctx, hipLaunchKernel(f, dim3((unsigned)grid), dim3((unsigned)P.threads), args, P.lds, ctx->stream));
    ctx->last_kernel = (jac ? 340 : 350) + p.q;  // the large variational kernel: residual + Jacobian | residual only
    ctx->last_n_stream = 0;
    return PCL_OK;
}

// Large variational exponential kernel (pcl_kernel_var_large_exp.hpp; contexts created with PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR |
// PCL_LARGE_VAR_EXP).  The plan: LD = n | 1, 64 threads per 16-row tile of G; what the one tile leaves of the LDS is NB column blocks of LD doubles,
// a third of them (NBW) per buffer, since Y, V and the level's result rotate through three.  A chain unit takes nc state columns (at most 16; option
// cols_per_slice sets another cap) and mg drives (option large_var_exp_drives caps them) of ALL 1 + v components: (1 + v) nc (1 + mg) columns,
// (1 + v) nc without the Jacobian.  Every group forms the value slot again, and a matrix-core pass costs the same for 1 .. 16 columns, so among
// the (nc, mg) that fit -- slices and groups evened -- the pair with the fewest 16-column passes per interval, sx ngrp ceil(columns / 16), is taken;
// on a tie the fewest units, then the wider slice.  A panel unit takes npc columns of the identity for all components, (1 + v) npc columns: the
// most that fit one pass (16 / (1 + v)) and a buffer; option general_slices: that many panel units at least.  Every split gives the same bits.
struct VarLargeExpPlan : LargeTile {
    int NBW, sx, nc, mg, ngrp, chain_units, npc, pu, U, W;
    long long passes;  // 16-column passes per interval and level: what the launch costs
    size_t lds;
};
static void var_large_exp_plan(const pcl_ctx *ctx, int n, int cols, int m, int v, bool jac, VarLargeExpPlan &P) {
    const int comp = 1 + v;
    static_cast<LargeTile &>(P) = large_tile(ctx->max_lds, n, m);
    P.NBW = P.NB / 3;
    const bool drv = jac && m > 0;
    const int nc_cap = ctx->opt_cols_per_slice > 0 ? (int)std::min<int64_t>(ctx->opt_cols_per_slice, cols) : std::min(cols, 16);
    const int mg_cap = drv ? (ctx->opt_large_var_exp_drives > 0 ? (int)std::min<int64_t>(ctx->opt_large_var_exp_drives, m) : m) : 0;
    // (nothing fits: one column, one drive -- the launch then refuses by its byte count)
    P.nc = 1, P.mg = drv ? 1 : 0, P.ngrp = drv ? m : 1, P.sx = cols;
    long long best = -1, best_u = -1;
    for (int nc0 = nc_cap; nc0 >= 1; --nc0)
        for (int mg0 = mg_cap; mg0 >= (drv ? 1 : 0); --mg0) {
            int nc = nc0, mg = mg0;
            const int sx = even_split(cols, nc), ngrp = drv ? even_split(m, mg) : 1;
            const int cx = comp * nc * (1 + mg);
            if (cx > P.NBW) continue;
            const long long units = (long long)sx * ngrp, cost = units * ((cx + 15) / 16);
            if (best < 0 || cost < best || (cost == best && units < best_u)) best = cost, best_u = units, P.nc = nc, P.mg = mg, P.sx = sx, P.ngrp = ngrp;
        }
    P.chain_units = P.sx * P.ngrp;
    P.npc = P.pu = 0;
    if (jac) {
        const int npc_fit = std::max(1, std::min(n, std::min(P.NBW, 16) / comp));
        P.pu = (n + npc_fit - 1) / npc_fit;
        if (ctx->opt_general_slices > 0) P.pu = (int)std::max<long long>(P.pu, std::min<long long>(ctx->opt_general_slices, n));
        P.npc = (n + P.pu - 1) / P.pu;
        P.pu = (n + P.npc - 1) / P.npc;  // (no unit without work)
    }
    P.U = P.chain_units + P.pu;
    const int cx = comp * P.nc * (1 + P.mg);
    P.W = std::max(cx, comp * P.npc);
    P.passes = (long long)P.chain_units * ((cx + 15) / 16) + (long long)P.pu * ((comp * P.npc + 15) / 16);
    P.lds = (size_t)(P.fixed + 3LL * P.LD * P.W) * sizeof(double);
}
static int var_large_exp_launch(pcl_ctx *ctx, const double *Z, double *delta, double *vals) {
    const pcl_desc &D = ctx->desc;
    const int n = ctx->n, m = D.n_drives, v = ctx->var;
    const bool jac = vals != nullptr;
    VarLargeExpPlan P;
    var_large_exp_plan(ctx, n, ctx->cols, m, v, jac, P);
    if (P.lds > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "the large variational exponential kernel needs %zu B of LDS (> %d) for n = %d, m = %d, v = %d", P.lds, ctx->max_lds, n, m, v);
    KParams p;
    memset(&p, 0, sizeof p);
    p.Z = Z;
    p.delta = delta;
    p.jac = vals;
    p.G0 = ctx->dvar_tab;  // (build_G as var_large_launch sets it up: the drift, and the drives on the union table)
    p.upos = ctx->dupos;
    p.ucoef = ctx->ducoef;
    p.n_upos = ctx->n_upos;
    p.ell_val = ctx->dell_val;
    p.ell_col = ctx->dell_col;
    p.ell_w = ctx->ell_w;
    p.x_off0 = -1;
    p.jac_per = var_jac_per(ctx);
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
    p.nt = ctx->opt_nt == 1 ? 1 : 0;  // (plain or nontemporal block stores)
    p.lds_doubles = (int)(P.lds / sizeof(double));
    VarLargeParams w;
    memset(&w, 0, sizeof w);
    w.gv_val = ctx->dvl_gval;
    w.gv_col = ctx->dvl_gcol;
    w.gv_w = ctx->vl_gw;
    w.v = v;
    for (int b = 0; b <= v; ++b) w.xo[b] = ctx->x_offs[b];
    w.sx = P.sx;
    w.mg = P.mg;
    w.ngrp = P.ngrp;
    w.npc = P.npc;
    w.pu = P.pu;
    const long long grid = (long long)ctx->K * P.U;
    if (grid > 0x7fffffffLL) return fail(ctx, PCL_ESHAPE, "pcl_eval / pcl_jac: %lld workgroups exceed the grid limit", grid);
    const void *f = jac ? (const void *)pcl_var_large_exp_kernel<true> : (const void *)pcl_var_large_exp_kernel<false>;
    if (int rc = var_set_lds(ctx, f, P.lds)) return rc;
    void *args[] = {&p, &w};
    HIP_TRY(ctx, hipLaunchKernel(f, dim3((unsigned)grid), dim3((unsigned)P.threads), args, P.lds, ctx->stream));
    ctx->last_kernel = jac ? 370 : 371;  // the large variational exponential kernel: residual + Jacobian | residual only
    ctx->last_n_stream = 0;
    return PCL_OK;
}

static int var_launch_fused(pcl_ctx *ctx, const double *Z, double *delta, double *vals, bool compact = false) {
    ON_DEVICE(ctx);
    if (ctx->large_var_exp) return var_large_exp_launch(ctx, Z, delta, vals);
    if (ctx->vexp) return var_exp_launch(ctx, Z, delta, vals, compact);
    if (ctx->desc.pade_order == 0)
        return fail(ctx, PCL_EINVAL, "pcl_eval / pcl_jac: the context was created with pade_order = 0; call pcl_set_order_policy (or a host-pointer entry point) first");
    if (ctx->large_var) return var_large_launch(ctx, Z, delta, vals);
    VarParams p;
    var_fill(ctx, p);
    p.Z = Z;
    p.delta = delta;
    p.vals = vals;
    const bool jac = vals != nullptr;
    p.nbw = jac ? (compact ? 1 : var_split_blocks(ctx)) : 0;  // (a compact launch stores every tile once: nothing to split)
    if (compact) p.compact = 1, p.jper = jac_per_compact(ctx);
    p.ncw = var_split_cols(ctx);
    const void *f = var_pick_fused(ctx->var, ctx->desc.pade_order / 2, jac);
    if (!f) return fail(ctx, PCL_ESHAPE, "pcl_eval / pcl_jac: no variational kernel for v=%d, order %d", ctx->var, ctx->desc.pade_order);
    const size_t nn = (size_t)ctx->n * ctx->n;
    // block role: G, P, Q_i tiles; column role: the row-compressed values of G(u_k)
    const size_t lds = std::max(jac ? (2 + ctx->var) * nn : 0, (size_t)ctx->var_wG * ctx->n) * sizeof(double);
    if (int rc = var_set_lds(ctx, f, lds)) return rc;
    const long long grid = (long long)ctx->K * (p.nbw + p.ncw);
    if (grid > 0x7fffffffLL) return fail(ctx, PCL_ESHAPE, "pcl_eval / pcl_jac: %lld workgroups exceed the grid limit", grid);
    void *args[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(f, dim3((unsigned)grid), dim3(PCL_VAR_THREADS), args, lds, ctx->stream));
    ctx->last_kernel = jac ? (compact ? 72 : 70) : 71;  // the variational kernel: fused | residual only | compact
    return PCL_OK;
}

// LDS of the Hessian kernel with w waves: G, G^T | w slabs of V_{l,j} | w rows of m^2 + m + 1 sums
static size_t var_hess_lds(const pcl_ctx *ctx, int q, int w) {
    const size_t m = ctx->desc.n_drives;
    return (2 * (size_t)ctx->n * ctx->n + (size_t)w * (m * q * (ctx->var + 1) * 64 + m * m + m + 1)) * sizeof(double);
}

static int var_launch_hess(pcl_ctx *ctx, const double *Z, const double *mu, double *hess) {
    ON_DEVICE(ctx);
    if (ctx->desc.pade_order == 0)
        return fail(ctx, PCL_EINVAL, "pcl_hess: the context was created with pade_order = 0; call pcl_set_order_policy (or a host-pointer entry point) first");
    const int q = ctx->desc.pade_order / 2;
    VarParams p;
    var_fill(ctx, p);
    p.Z = Z;
    p.mu = mu;
    p.hess = hess;
    // waves per workgroup: as many as the LDS and the state columns allow, at most 8 (a function of the shape only: the sums' order is fixed)
    int w = std::min(8, ctx->cols);
    while (w > 1 && var_hess_lds(ctx, q, w) > (size_t)ctx->max_lds) --w;
    if (var_hess_lds(ctx, q, w) > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "pcl_hess: the variational Hessian's tiles (%zu bytes at order %d) exceed the LDS", var_hess_lds(ctx, q, w), ctx->desc.pade_order);
    p.hw = w;
    const void *f = var_pick_hess(ctx->var, q);
    if (!f) return fail(ctx, PCL_ESHAPE, "pcl_hess: no variational kernel for v=%d, order %d", ctx->var, ctx->desc.pade_order);
    const size_t lds = var_hess_lds(ctx, q, w);
    if (int rc = var_set_lds(ctx, f, lds)) return rc;
    void *args[] = {&p};
    HIP_TRY(ctx, hipLaunchKernel(f, dim3((unsigned)ctx->K), dim3(64 * w), args, lds, ctx->stream));
    ctx->last_hess_kernel = 70;
    return PCL_OK;
}

static int var_set_goal(pcl_ctx *ctx, const double *goal_iso_vec);
static int var_set_goal_subspace(pcl_ctx *ctx, const double *goal_sub_iso_vec, const int32_t *subspace, int32_t ns);
static int var_set_goal_form(pcl_ctx *ctx, int32_t scope, int32_t R, const double *A, const double *c);
static int var_set_weights(pcl_ctx *ctx, const double *w);
static int var_objective_dev(pcl_ctx *ctx, const double *Z, double Q, double *value, double *grad);
static int var_objective_hess_nnz(const pcl_ctx *ctx, int64_t *nnz);
static int var_objective_hess_structure(const pcl_ctx *ctx, int64_t *rows, int64_t *cols);
static int var_objective_hess_dev(pcl_ctx *ctx, const double *Z, double Q, double sigma, double *vals);
static int var_rollout_dev(pcl_ctx *ctx, const double *Z, double *X_out);
static int var_large_rollout_dev(pcl_ctx *ctx, const double *Z, double *X_out);
