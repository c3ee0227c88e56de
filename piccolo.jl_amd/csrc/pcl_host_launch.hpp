// pcl_host_launch.hpp -- part of piccolo_hip.hip (included there, in place): what the launchers share.  The kernels' parameter block, the Pade
// coefficients, the note of a pattern-compiled kernel that could not be had, the device error word, and the idioms of the launch code: the member
// window's trajectories and drift tables, the 31-bit grid check, the balanced persistent grid, the grow-only device scratch.  The launchers
// themselves: pcl_host_launch_pade.hpp (residual and Jacobian), pcl_host_launch_hess.hpp (Hessian of the Lagrangian), pcl_host_variational.hpp.
#pragma once
static int resolve_order(pcl_ctx *ctx, const double *Z_host, const char *where);
// --- launch helpers -------------------------------------------------------------------------
// LD = (n rounded up to 4) + 2  ==  2*odd: conflict-free ds_read_b64 of the MFMA b operand
// (16 columns x 2 k-rows per half-wave land on 32 distinct 8-byte bank pairs).
static int lds_ld(int n) { return ((n + 3) & ~3) + 2; }  // n = generator dimension

static void fill_params(const pcl_ctx *ctx, KParams &p) {
    memset(&p, 0, sizeof p);
    const pcl_desc &D = ctx->desc;
    p.G0 = ctx->dG0 + (D.per_member_G0 ? (long long)ctx->win_first * ctx->n * ctx->n : 0);  // member window: offsets, not kernel logic
    p.upos = ctx->dupos;
    p.ucoef = ctx->ducoef;
    p.n_upos = ctx->n_upos;
    p.csr_ptr = ctx->dcsr_ptr;
    p.csr_col = ctx->dcsr_col;
    p.csr_val = ctx->dcsr_val;
    p.csc_ptr = ctx->dcsc_ptr;
    p.csc_row = ctx->dcsc_row;
    p.csc_val = ctx->dcsc_val;
    p.x_offs = ctx->dxoffs + (D.batch_mode == PCL_BATCH_MEMBERS ? ctx->win_first : 0);
    p.x_off0 = (D.batch_mode != PCL_BATCH_MEMBERS || ctx->win_count == 1) ? (int)ctx->x_offs[D.batch_mode == PCL_BATCH_MEMBERS ? ctx->win_first : 0] : -1;
    p.umap = ctx->dumap;
    p.uell_l = ctx->duell_l;
    p.uell_v = ctx->duell_v;
    p.uell_w = ctx->uell_w;
    p.ell_val = ctx->dell_val;
    p.ell_col = ctx->dell_col;
    p.ell_w = ctx->ell_w;
    p.ellt_val = ctx->dellt_val;
    p.ellt_col = ctx->dellt_col;
    p.ellt_w = ctx->ellt_w;
    p.hpart = ctx->dhpart;
    p.hcnt = ctx->dhcnt;
    p.ug0 = ctx->dug0;
    p.iso = ctx->iso;
    p.z_batch_stride = D.batch_mode == PCL_BATCH_TRAJ ? (long long)D.z_dim * D.N : 0;
    p.g0_batch_stride = D.per_member_G0 ? (long long)ctx->n * ctx->n : 0;
    p.d = D.d;
    p.cols = ctx->cols;
    p.n = ctx->n;
    p.m = D.n_drives;
    p.K = ctx->K;
    p.z_dim = D.z_dim;
    p.u_off = D.u_off;
    p.dt_off = D.dt_off;
    p.batch = ctx->win_count;
    p.LD = lds_ld(ctx->n);
    p.nt = ctx->opt_nt > 0 ? (int)ctx->opt_nt : 0;  // (auto: the fused launch decides by its size)
    p.dbg = ctx->ddbg;
    p.prof = (int)ctx->opt_prof;
    p.hess_per = hess_per(ctx);
    p.err = ctx->derr;
}

// A pattern-compiled kernel was wanted (jit = 1, the shape applies) and could not be had: the slower kernel families serve the context
// (1.5-2.2x for residual + Jacobian, 25-30x for the Hessian at orders 6-10) -- never silently: the note is what pcl_last_error returns
// until the next failure, "jit_fallbacks" counts, and with option require_jit = 1 the call fails instead.
static int jit_fell_back(pcl_ctx *ctx, const char *what) {
    ++ctx->jit_fallbacks;
    {
        std::lock_guard<std::mutex> lock(g_jit_mutex);
        ++g_jit_fallbacks;
    }
    fail(ctx, PCL_EHIP, "%s: the pattern-compiled kernel is not available (%s); %s", what, g_jit_note.c_str(),
         ctx->opt_require_jit ? "require_jit = 1" : "falling back to the built-in kernels (slower; set option require_jit = 1 to make this an error)");
    if (getenv("PCL_VERBOSE")) fprintf(stderr, "piccolo_hip: %s\n", ctx->err.c_str());
    return ctx->opt_require_jit ? PCL_EHIP : PCL_ENOTIMPL;
}

// A barrier-free kernel whose bounded wait gave up (a logic or timing failure: its outputs are partly stale) has set the context's
// error word.  Looked at by every evaluator entry point before it launches and by every call that synchronises.
static int check_device_error(pcl_ctx *ctx, const char *where) {
    if (!ctx->herr) return PCL_OK;
    const int w = __atomic_load_n(ctx->herr, __ATOMIC_ACQUIRE);
    if (!w) return PCL_OK;
    __atomic_store_n(ctx->herr, 0, __ATOMIC_RELEASE);
    if (ctx->dv4_tick) (void)hipMemsetAsync(ctx->dv4_tick, 0, (4 + (size_t)ctx->desc.batch * ctx->K) * sizeof(unsigned int), ctx->stream);  // the launch may have left its counters behind
    // ... and the self-resetting arrival counters of the Hessian kernels (a wave that gave up never made its arrival: the interval's counter -- and the R-chain
    // waves' delivery word, whose stale 1 would pass the NEXT launch the old tiles -- would stay where they are)
    if (ctx->dhcc && ctx->hc_cap > 0) (void)hipMemsetAsync(ctx->dhcc, 0, (size_t)ctx->hc_cap * sizeof(unsigned int), ctx->stream);
    if (ctx->dhcf) (void)hipMemsetAsync(ctx->dhcf, 0, (size_t)ctx->desc.batch * ctx->K * sizeof(unsigned int), ctx->stream);
    if (ctx->dh4c && ctx->h4_cap > 0) (void)hipMemsetAsync(ctx->dh4c, 0, (size_t)ctx->h4_cap * sizeof(unsigned int), ctx->stream);
    return fail(ctx, PCL_EINTERNAL, "%s: an earlier kernel of this context gave up a bounded wait between its waves (device error word 0x%x); "
                "the outputs of that launch are incomplete", where, w);
}

static int set_lds_attr(pcl_ctx *ctx, const void *kern, int slot, size_t lds) {
    if (ctx->lds_set[slot] == lds && ctx->lds_kern[slot] == kern) return PCL_OK;
    ctx->lds_kern[slot] = kern;
    HIP_TRY(ctx, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ctx->lds_set[slot] = lds;
    return PCL_OK;
}

// diagonal Pade coefficients of exp at order 2q: c_j = (2q - j)! q! / ((2q)! j! (q - j)!)
static void fill_pade(KParams &p, int order) {
    p.q = order / 2;
    double f[16];
    f[0] = 1.0;
    for (int i = 1; i < 16; ++i) f[i] = f[i - 1] * i;
    for (int j = 0; j <= p.q; ++j) p.pc[j] = f[2 * p.q - j] * f[p.q] / (f[2 * p.q] * f[j] * f[p.q - j]);
}

// The trajectories of the member window (PCL_BATCH_TRAJ: every member has its own; offsets, not kernel logic)
static const double *window_Z(const pcl_ctx *ctx, const double *Z) { return Z + (ctx->desc.batch_mode == PCL_BATCH_TRAJ ? (long long)ctx->win_first * ctx->desc.z_dim * ctx->desc.N : 0); }
// ... and the drift tables of the pattern-compiled kernels of kernel 4's family (a table per member where the members have their own drifts)
struct V4Tabs {
    const double *tab, *tab_t, *dcf;
};
static V4Tabs v4_tabs(const pcl_ctx *ctx) {
    const pcl_codegen::V4Plan &v4 = *ctx->v4_plan;
    const long long wo = ctx->desc.per_member_G0 ? (long long)ctx->win_first : 0;
    return {ctx->dv4_tab + wo * v4.n_drift_pad, ctx->dv4_tab_t + wo * v4.n_drift_pad, ctx->dv4_dcf + wo * v4.n_dcf_pad};
}
// A grid dimension has 31 bits
static int check_grid(const pcl_ctx *ctx, long long items, const char *msg = "too many work items") { return items > 0x7fffffffLL ? fail(ctx, PCL_ESHAPE, "%s", msg) : PCL_OK; }
// Persistent grid in which every workgroup walks the same number of items: ceil(items / slots) rounds (option grid overrides)
static long long balanced_grid(long long items, long long slots, int64_t opt_grid) {
    const long long rounds = (items + slots - 1) / slots;
    return opt_grid > 0 ? std::min<long long>(items, opt_grid) : (items + rounds - 1) / rounds;
}
// The tile geometry of the large-generator kernels (pcl_device_large.hpp), stated once for their planners: LD = n | 1, 64 threads per 16-row tile of
// G, `fixed` doubles of LDS whatever the plan (the tile, PL_SLACK, the drive amplitudes of build_G) and, in what they leave of max_lds, NB column
// blocks of LD doubles.  Every plan of the family starts from it (struct ...Plan : LargeTile)
struct LargeTile {
    int LD, threads;
    long long fixed;
    int NB;
};
static LargeTile large_tile(int max_lds, int n, int m) {
    LargeTile t;
    t.LD = n | 1;
    t.threads = 64 * ((n + 15) / 16);
    t.fixed = (long long)t.LD * n + PL_SLACK + m + 8;
    t.NB = (int)((max_lds / (long long)sizeof(double) - t.fixed) / t.LD);
    return t;
}
// `total` in pieces of at most `per` (state columns in slices, drives in groups): returns the fewest pieces and evens `per` over them
static int even_split(int total, int &per) {
    const int cnt = (total + per - 1) / per;
    per = (total + cnt - 1) / cnt;
    return cnt;
}
// Grow-only device scratch: nothing while *cap covers `need`; else a (and b, which shares the capacity) are freed and allocated anew with na / nb
// elements, zero-filled on the launch stream where asked, and *cap is set last: a failed allocation leaves no capacity behind.
template <class C, class A, class B = char>
static int grow_scratch(pcl_ctx *ctx, C *cap, long long need, A **a, size_t na, bool zero_a = false, B **b = nullptr, size_t nb = 0, bool zero_b = false) {
    if (*cap >= need) return PCL_OK;
    if (*a) (void)hipFree(*a);
    if (b && *b) (void)hipFree(*b);
    *a = nullptr, *cap = 0;
    if (b) *b = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)a, na * sizeof(A)));
    if (zero_a) HIP_TRY(ctx, hipMemsetAsync(*a, 0, na * sizeof(A), ctx->stream));
    if (b) HIP_TRY(ctx, hipMalloc((void **)b, nb * sizeof(B)));
    if (b && zero_b) HIP_TRY(ctx, hipMemsetAsync(*b, 0, nb * sizeof(B), ctx->stream));
    *cap = need;
    return PCL_OK;
}
