// pcl_host_options.hpp -- part of piccolo_hip.hip (included there, in place): pcl_set_option / pcl_get_option / pcl_debug_timing.  One table, one
// row per key (the switches are listed in OPTIONS.md): what pcl_set_option makes of a value and what pcl_get_option reads.  A key without a setter
// is read-only, one without a reader write-only (OPTIONS.md lists both); either call refuses the other half as an unknown option.
#pragma once
// --- options ---------------------------------------------------------------------------------
enum OptNorm {
    OPT_NONE,              // no setter
    OPT_RAW,               // the value as it is
    OPT_BOOL,              // nonzero -> 1
    OPT_TRI,               // negative -> -1 (auto), else nonzero -> 1
    OPT_SATURATE,          // below a -> a, above b -> b
    OPT_IN_RANGE_ELSE,     // a .. b, anything else -> other
    OPT_ONE_OF_ELSE,       // a, b or c, anything else -> other
    OPT_IN_RANGE_OR_FAIL,  // a .. b (and, with `on`, only on a context with that flag), anything else: PCL_EINVAL with msg (its %s: the key)
    OPT_GATE,              // a gate option of pcl_host_service.hpp (set_gate)
    OPT_FUNCTION,          // set_fn
};
struct OptRow {
    const char *name;
    OptNorm norm;
    int64_t pcl_ctx::*member;  // what the setter stores to, and the reader reads unless get_fn is set
    int64_t a, b, c, other;
    const char *msg;
    int pcl_ctx::*on;
    Gate gate;
    int (*set_fn)(pcl_ctx *, const char *key, int64_t v);
    int64_t (*get_fn)(const pcl_ctx *);
    bool readable;
};
static const int64_t OPT_MAX = INT64_MAX;
using OptGet = int64_t (*)(const pcl_ctx *);
static OptRow opt_row(const char *name, OptNorm norm, int64_t pcl_ctx::*m, int64_t a = 0, int64_t b = 0, int64_t c = 0, int64_t other = 0, const char *msg = nullptr,
                      int pcl_ctx::*on = nullptr) {
    return OptRow{name, norm, m, a, b, c, other, msg, on, GATE_NONE, nullptr, nullptr, true};
}
static OptRow write_only(OptRow r) { return r.readable = false, r; }
static OptRow read_as(OptRow r, OptGet get) { return r.get_fn = get, r; }
static OptRow read_only(const char *name, OptGet get) { return read_as(opt_row(name, OPT_NONE, nullptr), get); }
static OptRow gate_row(const char *name, Gate g) { return OptRow{name, OPT_GATE, nullptr, 0, 0, 0, 0, nullptr, nullptr, g, nullptr, nullptr, true}; }
static OptRow function_row(const char *name, int (*set)(pcl_ctx *, const char *, int64_t), OptGet get) {
    return OptRow{name, OPT_FUNCTION, nullptr, 0, 0, 0, 0, nullptr, nullptr, GATE_NONE, set, get, get != nullptr};
}
#define OPT_READ(expr) [](const pcl_ctx *c) -> int64_t { return (int64_t)(expr); }

// host-pointer entry points: threads expanding the compact values (0 default count | n | -1 sweep over the context's first twelve calls)
static int set_host_threads(pcl_ctx *ctx, const char *, int64_t v) {
    ctx->opt_host_threads = v < 0 ? -1 : v;
    ctx->host_threads_tuned = 0;
    ctx->host_tune_calls = 0;
    for (double &t : ctx->host_tune_t) t = 1e300;
    return PCL_OK;
}
// 0 auto (one launch where it applies) | 2 always regulariser + infidelity launches
static int set_objective_launches(pcl_ctx *ctx, const char *key, int64_t v) {
    if (v != 0 && v != 2) return fail(ctx, PCL_EINVAL, "%s must be 0 or 2", key);
    ctx->opt_objective_launches = v;
    return PCL_OK;
}
// 0: auto, 1: one workgroup per interval, 2: persistent wave-synchronous kernel, 3, 4, 7, 8: DESIGN.md
static int set_hess_kernel(pcl_ctx *ctx, const char *key, int64_t v) {
    if ((v < 0 || v > 4) && v != 7 && v != 8) return fail(ctx, PCL_EINVAL, "%s must be 0 .. 4, 7 or 8", key);
    ctx->opt_hess_kernel = v;
    return PCL_OK;
}
// profiling aid: cycle stamps of workgroup 0 (pcl_debug_timing reads them)
static int set_debug_timing(pcl_ctx *ctx, const char *key, int64_t v) {
#ifndef PCL_PROFILE
    if (v) return fail(ctx, PCL_ENOTIMPL, "%s needs a library built with -DPCL_PROFILE (the shipped kernels carry no stamps)", key);
#endif
    (void)key;
    if (v && !ctx->ddbg) {
        HIP_TRY(ctx, hipMalloc((void **)&ctx->ddbg, PCL_DBG_WORDS * sizeof(long long)));
        HIP_TRY(ctx, hipMemset(ctx->ddbg, 0, PCL_DBG_WORDS * sizeof(long long)));
    } else if (!v && ctx->ddbg) {
        (void)hipFree(ctx->ddbg);
        ctx->ddbg = nullptr;
    }
    return PCL_OK;
}
#ifdef PCL_PROFILE
// timing variants of kernel 4's generated product (WRONG results); recompiles
static int set_v4_variant(pcl_ctx *ctx, const char *, int64_t v) {
    ctx->opt_v4_variant = v;
    ctx->v4_f = ctx->v4_ft = ctx->v4_f1 = ctx->v4_feval = ctx->v4_fevalc = ctx->v4_fhess = ctx->v4_fhess2 = ctx->v4_fhessc = nullptr;
    return PCL_OK;
}
#endif
static int64_t get_effective_cols_per_slice(const pcl_ctx *ctx) {
    return ((ctx->opt_kernel == 3 || (ctx->opt_kernel == 0 && v3_specialised(ctx))) && ctx->opt_use_mfma && v3_supported(ctx) && !ctx->vec && ctx->cols == ctx->desc.d)
               ? (v3_contiguous(ctx) ? ctx->desc.d : choose_cols_v3(ctx))
               : choose_cols_per_slice(ctx, true);
}
static int64_t get_occupancy_v2(const pcl_ctx *ctx) {
    KParams p;
    fill_params(ctx, p);
    p.nc = choose_cols_per_slice(ctx, true);
    const size_t lds = fused2_lds_bytes(p, true, ell_fits_lds(ctx));
    int nb = 0;
    (void)hipFuncSetAttribute((const void *)pcl_fused_kernel_v2<true, 1, 0, 0, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pcl_fused_kernel_v2<true, 1, 0, 0, 0>, 512, lds) != hipSuccess) nb = -1;
    return nb * 1000000LL + (long long)lds;
}
static int64_t get_jit_counter(const int64_t &counter) {
    std::lock_guard<std::mutex> lock(g_jit_mutex);
    return counter;
}

static const OptRow kOptions[] = {
    opt_row("cols_per_slice", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_cols_per_slice, 0, OPT_MAX, 0, 0, "%s must be >= 0"),
    opt_row("use_mfma", OPT_BOOL, &pcl_ctx::opt_use_mfma),
    opt_row("nt_stores", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_nt, -1, 3, 0, 0, "%s must be -1, 0, 1, 2 or 3"),  // -1 auto (by launch size) | 0 plain | 1 nontemporal | 2 write-through
    write_only(opt_row("grid", OPT_RAW, &pcl_ctx::opt_grid)),
    read_only("effective_cols_per_slice", get_effective_cols_per_slice),
    read_only("n_cu", OPT_READ(c->n_cu)),
    // variational contexts: workgroups per interval of the fused launch (0 auto; read: what a launch takes)
    read_as(opt_row("var_block_wgs", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_var_blocks, 0, OPT_MAX, 0, 0, "%s must be >= 0"), OPT_READ(c->var ? var_split_blocks(c) : c->opt_var_blocks)),
    read_as(opt_row("var_col_wgs", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_var_cols, 0, OPT_MAX, 0, 0, "%s must be >= 0"), OPT_READ(c->var ? var_split_cols(c) : c->opt_var_cols)),
    read_only("variations", OPT_READ(c->var)),
    // the gate options (pcl_host_service.hpp has what each opens, on which kind of context, and the words of every refusal)
    gate_row("var_full", GATE_VAR_FULL),        // (0: also drops goal, weights, regularisers)
    gate_row("exp_hess", GATE_EXP_HESS),
    gate_row("exp_full", GATE_EXP_FULL),
    gate_row("var_compact", GATE_VAR_COMPACT),
    gate_row("var_exp_hess", GATE_VAR_EXP_HESS),
    gate_row("large_hess", GATE_LARGE_HESS),
    gate_row("large_exp_hess", GATE_LARGE_EXP_HESS),
    gate_row("large_exp_reduce", GATE_LARGE_EXP_REDUCE),
    gate_row("large_full", GATE_LARGE_FULL),    // (0: also drops goal, weights, regularisers)
    gate_row("large_reduce", GATE_LARGE_REDUCE),
    gate_row("large_var_full", GATE_LARGE_VAR_FULL),  // (0: also drops goal, weights, regularisers)
    gate_row("large_var_hess", GATE_LARGE_VAR_HESS),
    gate_row("large_var_exp_hess", GATE_LARGE_VAR_EXP_HESS),
    // ... the most drives per group of the large launches (0 auto), and the rollout's stages for measurements (0 both launches | 1 the propagators only | 2 the chain only)
    opt_row("var_large_drives", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_var_large_drives, 0, OPT_MAX, 0, 0,
            "%s must be >= 0, on a large variational context (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR, generator dimension above 64)", &pcl_ctx::large_var),
    opt_row("large_var_hess_drives", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_large_var_hess_drives, 0, OPT_MAX, 0, 0,
            "%s must be >= 0, on a large variational context (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR, generator dimension above 64)", &pcl_ctx::large_var),
    opt_row("large_var_exp_drives", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_large_var_exp_drives, 0, OPT_MAX, 0, 0,
            "%s must be >= 0, on a large variational exponential context (PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP, generator dimension above 64)", &pcl_ctx::large_var_exp),
    opt_row("large_var_exp_hess_drives", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_large_var_exp_hess_drives, 0, OPT_MAX, 0, 0,
            "%s must be >= 0, on a large variational exponential context (PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP, generator dimension above 64)", &pcl_ctx::large_var_exp),
    read_only("large_variational_exp", OPT_READ(c->large_var_exp)),  // 1: a large variational exponential context (the four flags at a generator dimension above 64)
    read_only("large_variational", OPT_READ(c->large_var)),  // 1: a large variational context (PCL_LARGE_N | PCL_LARGE_VAR at a generator dimension above 64)
    opt_row("large_hess_drives", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_large_hess_drives, 0, OPT_MAX, 0, 0, "%s must be >= 0, on a large context (PCL_LARGE_N, generator dimension above 64)", &pcl_ctx::large),
    opt_row("large_exp_drives", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_large_exp_drives, 0, OPT_MAX, 0, 0,
            "%s must be >= 0, on a large exponential context (PCL_LARGE_N | PCL_LARGE_EXP, generator dimension above 64)", &pcl_ctx::large_exp),
    opt_row("large_exp_hess_drives", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_large_exp_hess_drives, 0, OPT_MAX, 0, 0,
            "%s must be >= 0, on a large exponential context (PCL_LARGE_N | PCL_LARGE_EXP, generator dimension above 64)", &pcl_ctx::large_exp),
    opt_row("large_rollout_stage", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_large_rollout_stage, 0, 2, 0, 0, "%s must be 0, 1 or 2, on a large context (PCL_LARGE_N, generator dimension above 64)", &pcl_ctx::large),
    // ... where the octuple chain's tiles live: 0 nine in LDS | 1 four in the workspace where nine do not fit | 2 always
    function_row("var_exp_hess_tiles", [](pcl_ctx *c, const char *, int64_t v) { return var_exp_hess_set_tiles(c, v); }, OPT_READ(c->opt_vexph_tiles)),
#ifdef PCL_PROFILE
    write_only(opt_row("profile_flags", OPT_RAW, &pcl_ctx::opt_prof)),  // profiling experiments (results may be WRONG); not present in the shipped library
    function_row("v4_variant", set_v4_variant, nullptr),
#endif
    function_row("host_threads", set_host_threads, OPT_READ(host_threads(c))),
    read_only("host_expand_MBps", OPT_READ(c->host_expand_GBps * 1e3)),  // delivered rate of the fastest call of the thread-count sweep (0 before it has finished)
    opt_row("host_path", OPT_IN_RANGE_ELSE, &pcl_ctx::opt_host_path, 0, 2, 0, 0),  // 0 auto | 1 full values over PCIe | 2 compact values + host expansion
    opt_row("host_chunks", OPT_SATURATE, &pcl_ctx::opt_host_chunks, 1, 8),         // interval chunks of the compact D2H copy that overlap with the expansion
    write_only(opt_row("specialize", OPT_BOOL, &pcl_ctx::opt_specialize)),         // 0: always the run-time-shape kernel instances
    opt_row("jit", OPT_BOOL, &pcl_ctx::opt_jit),                                   // 1 (default): compile the context's shape on first use when no static instance matches
    opt_row("require_jit", OPT_BOOL, &pcl_ctx::opt_require_jit),                   // 1: a pattern-compiled kernel that is wanted and cannot be had is an error (PCL_EHIP), not a fallback
    write_only(opt_row("general_threads", OPT_ONE_OF_ELSE, &pcl_ctx::opt_general_threads, 256, 256, 256, 512)),  // general-order kernel: 256 or 512 (default) threads per workgroup
    write_only(opt_row("general_kernel_version", OPT_IN_RANGE_ELSE, &pcl_ctx::opt_general_version, 0, 2, 0, 0)),  // 0 auto | 1 reference formulation | 2 lock-step kernel (error where it does not fit)
    write_only(opt_row("general_slices", OPT_SATURATE, &pcl_ctx::opt_general_slices, 0, OPT_MAX)),                // lock-step kernel: slices of state columns per interval (0 auto)
    write_only(opt_row("general_pade_kernel", OPT_BOOL, &pcl_ctx::opt_general)),                                  // 1: the general-order kernel also for pade_order 4
    opt_row("stream_workgroups", OPT_RAW, &pcl_ctx::opt_stream_wg),  // kernel 3, contiguous: > 0 = role split with this many stream-role workgroups
    opt_row("contiguous", OPT_TRI, &pcl_ctx::opt_contig),            // kernel 3: 1 = equal contiguous column ranges per workgroup (default), 0 = round-robin slices
    function_row("objective_launches", set_objective_launches, OPT_READ(c->opt_objective_launches)),
    // kernel 4 A/B switches: 1 no raised priority for the P wave | 2 tails only behind the item's last block | 4 no cooperative first item | 8 LDS tiles NaN at kernel start (tests)
    // | 16 the first item's chains do not wait for the cooperative products | 32 no balanced split of the middle column's two blocks between two slices
    write_only(opt_row("v4_flags", OPT_RAW, &pcl_ctx::opt_v4_flags)),
    opt_row("v4_ticket", OPT_TRI, &pcl_ctx::opt_v4_ticket),                          // kernel 4: work items by ticket (-1 auto: full-value launches of several intervals per CU | 0 static split | 1)
    opt_row("v4_one_item", OPT_TRI, &pcl_ctx::opt_v4_one_item),                      // ... the module of launches with one item per workgroup (-1 auto | 0 the general module | 1 require)
    opt_row("v4_ticket_cols", OPT_SATURATE, &pcl_ctx::opt_v4_ticket_cols, 0, OPT_MAX),  // ... state columns per slice ticket (0 auto)
    opt_row("v4_ticket_ahead", OPT_IN_RANGE_ELSE, &pcl_ctx::opt_v4_ticket_ahead, 0, 2, 0, 0),  // ... slices taken ahead of the one being stored
    opt_row("v4_group", OPT_SATURATE, &pcl_ctx::opt_v4_group, 0, OPT_MAX),           // ... workgroups per group (0 auto: 8; must divide the grid)
    write_only(opt_row("v4_power_tiles", OPT_SATURATE, &pcl_ctx::opt_v4_np, 0, OPT_MAX)),  // ... LDS tiles the powers of G rotate through (0 auto)
    write_only(opt_row("v4_tail_mode", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_v4_tail_mode, 0, 3, 0, 0, "%s must be 0 .. 3")),  // 0 writer wave, plain stores | 1 nontemporal | 2 write-through | 3 the stream waves store the tails
    opt_row("v4_tune", OPT_BOOL, &pcl_ctx::opt_v4_tune),  // v4_ticket auto: 1 decide static split / slice tickets per values array by timing both on it | 0 always tickets
    read_only("last_v4_tune_choice", OPT_READ(c->last_v4_tune_choice)),  // of the array the last multi-trajectory launch wrote: -1 still sampling | 0 static split | 1 slice tickets
    read_only("last_v4_tune_static_ns", OPT_READ(c->last_v4_tune_static_ns)),  // best timed launch of each variant on the last decided array
    read_only("last_v4_tune_ticket_ns", OPT_READ(c->last_v4_tune_ticket_ns)),
    // host expansion: bytes per streaming store (0 the widest the host has | 16 | 32 | 64); read: the width the last host expansion used
    read_as(opt_row("host_store_bytes", OPT_ONE_OF_ELSE, &pcl_ctx::opt_host_store_bytes, 16, 32, 64, 0), OPT_READ(c->last_host_store_bytes)),
    read_only("cgroup_quota_cpus_x100", OPT_READ(pcl_host::cgroup_quota_cpus() * 100.0 + 0.5)),  // 100 x the CPUs the cgroup grants the process (cpu.max); 0: no quota
#ifdef PCL_LAB
    opt_row("resident_idle_us", OPT_SATURATE, &pcl_ctx::opt_resident_idle_us, 10, 2000000),  // resident evaluator: the kernel leaves after this long without a request
    read_only("resident_launches", OPT_READ(c->res.launches)),  // starts of the resident kernel since pcl_create (1 + the times it had left when a request came)
#endif
    opt_row("hess_xcd", OPT_SATURATE, &pcl_ctx::opt_hess_xcd, -1, OPT_MAX),  // column-group Hessian kernel: the waves of an interval take blockIdx values equal mod n = one XCD (-1 auto: 8 | 0, 1: blockIdx order)
    opt_row("hess_rpre", OPT_TRI, &pcl_ctx::opt_hess_rpre),  // ... the chain of the R_a in R-chain waves at the head of the launch (-1 auto | 0 | 1)
    opt_row("hess_pair", OPT_TRI, &pcl_ctx::opt_hess_pair),  // ... a chain wave and a contribution wave per column group (-1 auto: launches of at most n_cu / 2 intervals | 0 | 1)
    write_only(opt_row("hess_split", OPT_TRI, &pcl_ctx::opt_hess_split)),  // general-order pattern-compiled Hessian kernel: two workgroups per interval (-1 auto by launch size | 0 | 1)
    write_only(opt_row("eval_coop", OPT_TRI, &pcl_ctx::opt_eval_coop)),    // pattern-compiled residual kernel: four waves per interval (-1 auto by launch size | 0 | 1)
    opt_row("eval_kernel", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_eval_kernel, 0, 3, 0, 0, "%s must be 0 .. 3"),  // residual only: 0 auto, 1 matrix-core kernel, 2 pattern-compiled kernel
    function_row("hess_kernel", set_hess_kernel, OPT_READ(c->opt_hess_kernel)),
    function_row("debug_timing", set_debug_timing, nullptr),
    opt_row("kernel_version", OPT_IN_RANGE_OR_FAIL, &pcl_ctx::opt_kernel, 0, 5, 0, 0, "%s must be 0 (auto), 1, 2, 3, 4 or 5"),
    // what the last launches did, and what pcl_create found
    read_only("last_kernel", OPT_READ(c->last_kernel)),
    read_only("last_stream_workgroups", OPT_READ(c->last_n_stream)),
    read_only("last_hess_kernel", OPT_READ(c->last_hess_kernel)),
    read_only("last_hess_rpre", OPT_READ(c->last_hess_rpre)),
    read_only("last_hess_pair", OPT_READ(c->last_hess_pair)),
    read_only("last_hess_split", OPT_READ(c->last_hess_split)),
    read_only("last_eval_coop", OPT_READ(c->last_eval_coop)),
    read_only("last_v4_ticket", OPT_READ(c->last_v4_ticket)),
    read_only("last_v4_one_item", OPT_READ(c->last_v4_one_item)),
    read_only("last_objective_launches", OPT_READ(c->last_objective_launches)),
    read_only("last_step_launches", OPT_READ(c->last_step_launches)),  // pcl_eval_jac_merit_objective_dev: 2 = fused kernel + one tail launch, 4 = the separate calls
    read_only("last_merit_fused", OPT_READ(c->merit_fused)),
    read_only("jit_compiles", OPT_READ(get_jit_counter(g_jit_compiles))),      // modules this process compiled with hiprtc
    read_only("jit_cache_hits", OPT_READ(get_jit_counter(g_jit_cache_hits))),  // ... and loaded from the prebuilt directory or the on-disk cache instead
    read_only("jit_fallbacks", OPT_READ(c->jit_fallbacks)),                    // pattern-compiled kernels this context wanted and did not get
    read_only("pade_order", OPT_READ(c->desc.pade_order)),                     // the order in use (0: pade_order = 0 at creation and nothing has chosen yet)
    read_only("order_tol_met", OPT_READ(c->order_tol_met)),                    // 1 unless the order policy settled for order 10 with its bound above the tolerance
    read_only("order_theta_1e9", OPT_READ(c->order_theta * 1e9)),              // 1e9 x the bound on |dt G|_2 the order policy worked with
    read_only("ell_width_t", OPT_READ(c->ellt_w)),
    read_only("drives_antisymmetric", OPT_READ(c->drives_antisym)),
    read_only("occupancy_v2", get_occupancy_v2),
    read_only("iso_structured", OPT_READ(c->iso)),
    read_only("ell_width", OPT_READ(c->ell_w)),
    read_only("union_width", OPT_READ(c->uell_w)),
};
static const OptRow *find_option(const char *key) {
    for (const OptRow &r : kOptions)
        if (!strcmp(key, r.name)) return &r;
    return nullptr;
}

extern "C" int pcl_set_option(pcl_ctx *ctx, const char *key, int64_t v) {
    if (!ctx || !key) return PCL_EINVAL;
    const OptRow *r = find_option(key);
    if (!r || r->norm == OPT_NONE) return fail(ctx, PCL_EINVAL, "unknown option '%s'", key);
    switch (r->norm) {
        case OPT_GATE: return set_gate(ctx, r->gate, key, v);
        case OPT_FUNCTION: return r->set_fn(ctx, key, v);
        case OPT_BOOL: v = v != 0; break;
        case OPT_TRI: v = v < 0 ? -1 : (v != 0); break;
        case OPT_SATURATE: v = v < r->a ? r->a : (v > r->b ? r->b : v); break;
        case OPT_IN_RANGE_ELSE: v = v < r->a || v > r->b ? r->other : v; break;
        case OPT_ONE_OF_ELSE: v = v == r->a || v == r->b || v == r->c ? v : r->other; break;
        case OPT_IN_RANGE_OR_FAIL:
            if (v < r->a || v > r->b || (r->on && !(ctx->*(r->on)))) return fail(ctx, PCL_EINVAL, r->msg, key);
            break;
        default: break;
    }
    ctx->*(r->member) = v;
    return PCL_OK;
}
#ifdef PCL_LAB  // include/piccolo_hip_lab.h; the stamps themselves need -DPCL_PROFILE as well
extern "C" int pcl_debug_timing(pcl_ctx *ctx, int64_t *out, int64_t cap) {
    if (!ctx || !out || cap < 0) return PCL_EINVAL;
    if (!ctx->ddbg) return fail(ctx, PCL_EINVAL, "pcl_debug_timing: set option debug_timing first");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, ctx->ddbg, (size_t)std::min<int64_t>(cap, PCL_DBG_WORDS) * sizeof(long long), hipMemcpyDeviceToHost));
    return PCL_OK;
}
#endif

extern "C" int pcl_get_option(const pcl_ctx *ctx, const char *key, int64_t *v) {
    if (!ctx || !key || !v) return PCL_EINVAL;
    const OptRow *r = find_option(key);
    if (!r || !r->readable) return fail(ctx, PCL_EINVAL, "unknown option '%s'", key);
    *v = r->get_fn ? r->get_fn(ctx) : r->norm == OPT_GATE ? ctx->*kGates[r->gate].flag : ctx->*(r->member);
    return PCL_OK;
}
