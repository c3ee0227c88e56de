// pcl_host_service.hpp -- part of piccolo_hip.hip (included there, in place): which kind of context serves which family of entry points, under
// which gate option, and in which words everything else is refused -- one table, read by the entry points (require), by the host route and the
// launch ladders (serves) and by the setters of the gate options (set_gate).  DESIGN.md prints the table ("Context kinds and what they serve").
#pragma once

// The eight kinds of context: what pcl_create made of batch_mode, its flags and pade_order.  A context is of exactly one.
enum Kind { KIND_PLAIN, KIND_EXP, KIND_VAR, KIND_VAR_EXP, KIND_LARGE, KIND_LARGE_EXP, KIND_LARGE_VAR, KIND_LARGE_VAR_EXP, N_KINDS };
static Kind kind_of(const pcl_ctx *c) {
    return c->large_var_exp ? KIND_LARGE_VAR_EXP : c->large_var ? KIND_LARGE_VAR : c->large_exp ? KIND_LARGE_EXP : c->large ? KIND_LARGE : c->vexp ? KIND_VAR_EXP : c->var ? KIND_VAR : c->exp ? KIND_EXP : KIND_PLAIN;
}

// The families of entry points a kind serves, refuses or serves by option (the residual and the Jacobian are served by every kind).
enum Feature {
    FEAT_HESS,        // the Hessian of the Lagrangian: pcl_hess_nnz, pcl_hess_structure[_i64], pcl_hess[_dev]
    FEAT_OBJECTIVE,   // goal, weights, regularisers, pcl_objective[_dev], pcl_objective_hess*, pcl_rollout[_dev]
    FEAT_INFIDELITY,  // pcl_infidelity_dev: the objective's rule on plain and large contexts, never on a variational one
    FEAT_COMPACT,     // the compact Jacobian: pcl_jac_compact_nnz, pcl_eval_jac_compact_dev, pcl_jac_expand_dev, the host calls' compact route
    FEAT_MERIT,       // the merit / reduce payload: pcl_merit_grad_len, pcl_merit_grad_dev, pcl_eval_jac_merit_dev
    FEAT_STEP,        // pcl_eval_jac_merit_objective_dev: the payload AND the objective
    FEAT_COLLECTIVE,  // pcl_comm_init, pcl_reduce_sum[_dev], pcl_set_member_window
    N_FEATURES
};

// The gate options (OPTIONS.md): a context flag each, 0 by default.
enum Gate { GATE_NONE, GATE_EXP_HESS, GATE_EXP_FULL, GATE_VAR_FULL, GATE_VAR_COMPACT, GATE_VAR_EXP_HESS, GATE_LARGE_HESS, GATE_LARGE_FULL, GATE_LARGE_REDUCE,
            GATE_LARGE_EXP_HESS, GATE_LARGE_EXP_REDUCE, GATE_LARGE_VAR_FULL, GATE_LARGE_VAR_HESS, GATE_LARGE_VAR_EXP_HESS, N_GATES };

static int exp_hess_fits(const pcl_ctx *ctx, const char *who);
static int var_exp_hess_enable(pcl_ctx *ctx);
static int large_hess_enable(pcl_ctx *ctx);
static int large_exp_hess_enable(pcl_ctx *ctx);
static int var_large_hess_enable(pcl_ctx *ctx);
static int var_large_exp_hess_enable(pcl_ctx *ctx);
static int var_set_full(pcl_ctx *ctx, int64_t on);
static int large_set_full(pcl_ctx *ctx, int64_t on);
static int var_large_set_full(pcl_ctx *ctx, int64_t on);

#define KIND_BIT(k) (1u << (k))
struct GateInfo {
    int pcl_ctx::*flag;
    unsigned not_impl;                      // kinds on which "<key> = 1" is refused as not implemented, in the kind's words (every other kind that no cell of the table names it for: `needs`)
    const char *needs;                      // "<key> = 1 needs ..." (PCL_EINVAL)
    Feature feature;                        // the family it opens: its cell has the words of a not_impl refusal
    int (*apply)(pcl_ctx *, int64_t on);    // what a permitted 0 or 1 does beyond storing it (nullptr: nothing)
};
static const GateInfo kGates[N_GATES] = {
    {nullptr, 0, nullptr, FEAT_HESS, nullptr},
    {&pcl_ctx::exp_hess, KIND_BIT(KIND_LARGE_EXP) | KIND_BIT(KIND_VAR_EXP) | KIND_BIT(KIND_LARGE_VAR_EXP), "%s = 1 needs a context of the exponential constraint (PCL_ORDER_EXP)", FEAT_HESS,
     [](pcl_ctx *c, int64_t on) { return on ? exp_hess_fits(c, "exp_hess = 1") : PCL_OK; }},
    {&pcl_ctx::exp_full, KIND_BIT(KIND_LARGE_EXP), "%s = 1 needs a plain context of the exponential constraint (PCL_ORDER_EXP, not a variational one)", FEAT_COMPACT, nullptr},
    {&pcl_ctx::var_full, KIND_BIT(KIND_LARGE_VAR) | KIND_BIT(KIND_LARGE_VAR_EXP), "%s = 1 needs a variational context (PCL_BATCH_VARIATIONAL)", FEAT_OBJECTIVE, var_set_full},
    {&pcl_ctx::var_compact, KIND_BIT(KIND_LARGE_VAR) | KIND_BIT(KIND_LARGE_VAR_EXP), "%s = 1 needs a variational context (PCL_BATCH_VARIATIONAL or PCL_BATCH_VARIATIONAL_EXP)", FEAT_COMPACT, nullptr},
    {&pcl_ctx::var_exp_hess, KIND_BIT(KIND_LARGE_VAR_EXP), "%s = 1 needs a variational context of the exponential constraint (PCL_BATCH_VARIATIONAL_EXP)", FEAT_HESS,
     [](pcl_ctx *c, int64_t on) { return on ? var_exp_hess_enable(c) : PCL_OK; }},
    {&pcl_ctx::large_hess, KIND_BIT(KIND_LARGE_EXP), "%s = 1 needs a large context (batch_mode | PCL_LARGE_N at a generator dimension above 64); every other context has its Hessian options of its own", FEAT_HESS,
     [](pcl_ctx *c, int64_t on) { return on ? large_hess_enable(c) : PCL_OK; }},
    {&pcl_ctx::large_full, 0, "%s = 1 needs a large context (batch_mode | PCL_LARGE_N at a generator dimension above 64, on the Pade constraint); every other context serves its objective and rollout without it or by an option of its own", FEAT_OBJECTIVE,
     large_set_full},
    {&pcl_ctx::large_reduce, KIND_BIT(KIND_LARGE_EXP), "%s = 1 needs a large context (batch_mode | PCL_LARGE_N at a generator dimension above 64, on the Pade constraint); every other context serves its compact Jacobian and reduce payload without it or by an option of its own", FEAT_COMPACT,
     nullptr},
    {&pcl_ctx::large_exp_hess, 0, "%s = 1 needs a large exponential context (batch_mode | PCL_LARGE_N | PCL_LARGE_EXP, pade_order = PCL_ORDER_EXP, at a generator dimension above 64); every other context has its Hessian options of its own", FEAT_HESS,
     [](pcl_ctx *c, int64_t on) { return on ? large_exp_hess_enable(c) : PCL_OK; }},
    {&pcl_ctx::large_exp_reduce, 0, "%s = 1 needs a large exponential context (batch_mode | PCL_LARGE_N | PCL_LARGE_EXP, pade_order = PCL_ORDER_EXP, at a generator dimension above 64); every other context serves its compact Jacobian and reduce payload without it or by an option of its own", FEAT_COMPACT,
     nullptr},
    {&pcl_ctx::large_var_full, 0, "%s = 1 needs a large variational context (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR at a generator dimension above 64); every other context serves its objective and rollout without it or by an option of its own", FEAT_OBJECTIVE,
     var_large_set_full},
    {&pcl_ctx::large_var_hess, KIND_BIT(KIND_LARGE_VAR_EXP), "%s = 1 needs a large variational context (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR at a generator dimension above 64); every other context has its Hessian options of its own", FEAT_HESS,
     [](pcl_ctx *c, int64_t on) { return on ? var_large_hess_enable(c) : PCL_OK; }},
    {&pcl_ctx::large_var_exp_hess, 0, "%s = 1 needs a large variational exponential context (PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP, pade_order = PCL_ORDER_EXP, at a generator dimension above 64); every other context has its Hessian options of its own", FEAT_HESS,
     [](pcl_ctx *c, int64_t on) { return on ? var_large_exp_hess_enable(c) : PCL_OK; }},
};

// One cell of the table: served always ({}), never (NEVER), or while every gate it names is on.  `words` replaces the kind's refusal sentence.
struct Cell {
    Gate gate = GATE_NONE, and_gate = GATE_NONE;
    bool never = false;
    const char *words = nullptr;
};
static const Cell ALWAYS{}, NEVER{GATE_NONE, GATE_NONE, true, nullptr};
// The Hessian of the Lagrangian of PCL_BATCH_VARIATIONAL_EXP: its (u_i, u_j) block on component i needs third Frechet derivatives of exp.
static const char kVarExpHessWords[] =
    "%s is not implemented for a variational context of the exponential constraint (PCL_BATCH_VARIATIONAL_EXP): the Hessian of the Lagrangian needs third Frechet derivatives of exp; solve with a quasi-Newton Hessian";
static const Cell kService[N_KINDS][N_FEATURES] = {
    //                 HESS                                     OBJECTIVE           INFIDELITY          COMPACT                  MERIT                    STEP                                      COLLECTIVE
    /* PLAIN     */ {ALWAYS,                                    ALWAYS,             ALWAYS,             ALWAYS,                  ALWAYS,                  ALWAYS,                                   ALWAYS},
    /* EXP       */ {{GATE_EXP_HESS},                           ALWAYS,             ALWAYS,             {GATE_EXP_FULL},         {GATE_EXP_FULL},         {GATE_EXP_FULL},                          ALWAYS},
    /* VAR       */ {ALWAYS,                                    {GATE_VAR_FULL},    NEVER,              {GATE_VAR_COMPACT},      NEVER,                   NEVER,                                    NEVER},
    /* VAR_EXP   */ {{GATE_VAR_EXP_HESS, GATE_NONE, false, kVarExpHessWords}, {GATE_VAR_FULL}, NEVER,   {GATE_VAR_COMPACT},      NEVER,                   NEVER,                                    NEVER},
    /* LARGE     */ {{GATE_LARGE_HESS},                         {GATE_LARGE_FULL},  {GATE_LARGE_FULL},  {GATE_LARGE_REDUCE},     {GATE_LARGE_REDUCE},     {GATE_LARGE_REDUCE, GATE_LARGE_FULL},     ALWAYS},
    /* LARGE_EXP */ {{GATE_LARGE_EXP_HESS},                     {GATE_LARGE_FULL},  {GATE_LARGE_FULL},  {GATE_LARGE_EXP_REDUCE}, {GATE_LARGE_EXP_REDUCE}, {GATE_LARGE_EXP_REDUCE, GATE_LARGE_FULL}, ALWAYS},
    /* LARGE_VAR */ {{GATE_LARGE_VAR_HESS},                     {GATE_LARGE_VAR_FULL}, NEVER,             NEVER,                   NEVER,                   NEVER,                                    NEVER},
    /* LARGE_VAR_EXP */ {{GATE_LARGE_VAR_EXP_HESS},             {GATE_LARGE_VAR_FULL}, NEVER,             NEVER,                   NEVER,                   NEVER,                                    NEVER},
};

static bool serves(const pcl_ctx *ctx, Feature f) {
    const Cell &c = kService[kind_of(ctx)][f];
    return !c.never && (c.gate == GATE_NONE || ctx->*kGates[c.gate].flag) && (c.and_gate == GATE_NONE || ctx->*kGates[c.and_gate].flag);
}

// PCL_ENOTIMPL in the words of the context's kind, one sentence each: `what` is the entry point, or "<key> = 1" from a gate option's setter.
// (Only the large exponential sentence differs between the two: the setters leave its generator dimension out.)
static int refuse(const pcl_ctx *ctx, Feature f, const char *what, bool from_setter = false) {
    if (const char *words = kService[kind_of(ctx)][f].words) return fail(ctx, PCL_ENOTIMPL, words, what);
    char dim[48] = "";
    if (!from_setter) snprintf(dim, sizeof dim, ", generator dimension %d > 64", ctx->n);
    switch (kind_of(ctx)) {
        case KIND_LARGE_EXP:
            return fail(ctx, PCL_ENOTIMPL, "%s is not implemented for a large exponential context (PCL_LARGE_N | PCL_LARGE_EXP%s): residual and Jacobian, and by option large_full the objective and the rollout", what, dim);
        case KIND_LARGE:
            return fail(ctx, PCL_ENOTIMPL, "%s is not implemented for a context created with PCL_LARGE_N (generator dimension %d > 64): residual and Jacobian only", what, ctx->n);
        case KIND_LARGE_VAR:
            return fail(ctx, PCL_ENOTIMPL, "%s is not implemented for a large variational context (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR, generator dimension %d > 64): residual and Jacobian only", what, ctx->n);
        case KIND_LARGE_VAR_EXP:
            return fail(ctx, PCL_ENOTIMPL, "%s is not implemented for a large variational exponential context (PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP, generator dimension %d > 64): residual and Jacobian, and by option large_var_full the objective and the rollout", what, ctx->n);
        case KIND_VAR:
        case KIND_VAR_EXP:
            return fail(ctx, PCL_ENOTIMPL, "%s is not implemented for a variational context (%s)", what, ctx->vexp ? "PCL_BATCH_VARIATIONAL_EXP" : "PCL_BATCH_VARIATIONAL");
        case KIND_EXP:
            return fail(ctx, PCL_ENOTIMPL, "%s is not implemented for a context of the exponential constraint (PCL_ORDER_EXP)", what);
        default:
            return fail(ctx, PCL_EINTERNAL, "%s: the service table refuses a plain context", what);
    }
}

// The gate of an entry point: PCL_OK, or the refusal.  (A NULL context passes: the entry point's own check returns PCL_EINVAL for it.)
static int require(const pcl_ctx *ctx, Feature f, const char *what) { return !ctx || serves(ctx, f) ? PCL_OK : refuse(ctx, f, what); }

// pcl_set_option of a gate option: 0 or 1; 1 on a kind for which some cell of the table names the gate, else refused as GateInfo says.
static int set_gate(pcl_ctx *ctx, Gate g, const char *key, int64_t v) {
    const GateInfo &G = kGates[g];
    if (v != 0 && v != 1) return fail(ctx, PCL_EINVAL, "%s must be 0 or 1", key);
    const Kind kind = kind_of(ctx);
    bool named = false;
    for (const Cell &c : kService[kind]) named = named || c.gate == g || c.and_gate == g;
    if (v && !named) {
        if (!(G.not_impl & KIND_BIT(kind))) return fail(ctx, PCL_EINVAL, G.needs, key);
        char what[64];
        snprintf(what, sizeof what, "%s = 1", key);
        return refuse(ctx, G.feature, what, true);
    }
    if (G.apply) TRY(G.apply(ctx, v));
    ctx->*G.flag = (int)v;
    return PCL_OK;
}
