// piccolo_hip.hip -- libpiccolo_hip.so: C ABI (include/piccolo_hip.h cites the reference interfaces it replaces) and host
// side of the gfx950 (MI355X / CDNA4) Pade collocation constraint evaluator.  One translation unit; the kernels live in
//   pcl_device_common.hpp      parameter block, MFMA tile GEMM on LDS operands, wave-level helpers
//   pcl_kernel_fused_v3.hpp    default residual + Jacobian kernel: persistent, one workgroup per CU, stream / matrix roles
//   pcl_kernels_fused_v2.hpp   fallback (two workgroups per CU); also kets and the compact Jacobian at large n
//   pcl_kernels_reference.hpp  single-role kernel (A/B reference) and the general-order kernel (Pade 2..10)
//   pcl_kernel_eval.hpp        residual only (pcl_eval): persistent, three barriers per interval
//   pcl_device_large.hpp       what the kernels of generator dimensions 66 .. 128 share: the one-tile MFMA product, the A operand and its mask, the sparse row product, the panel registers, the column store
//   pcl_kernel_pade_large.hpp  generator dimensions 66 .. 128 (contexts created with PCL_LARGE_N): one LDS tile, the powers of G by column panels, the drives in groups
//   pcl_kernel_large_exp_hess.hpp   ... its Hessian of the Lagrangian (option large_exp_hess): the adjoint of that recurrence with the second derivative carried, per-column partial sums
//   pcl_kernel_var_large.hpp        ... the variational integrators there (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR): chain units of 1 + v components, panel units of the powers and, one variation at a time, the Frechet powers
//   pcl_kernel_var_large_hess.hpp   ... ... their Hessian of the Lagrangian (option large_var_hess): the chains of pcl_kernel_pade_large_hess.hpp on the lifted generator, one pass per component
//   pcl_kernel_var_large_rollout.hpp ... ... their rollout of the stacked state (option large_var_full): E and the Frechet derivatives L_i by column panels of one substepped Horner recurrence, then the chain of the knots
//   pcl_kernel_var_large_exp.hpp    ... ... the exponential constraint on them (PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP): that recurrence on the lifted pair in action form, the drive derivative carried through it
//   pcl_kernel_var_large_exp_hess.hpp ... ... ... its Hessian of the Lagrangian (option large_var_exp_hess): the adjoint recurrence of pcl_kernel_large_exp_hess.hpp on the lifted generator, one pass per component as workgroups of their own, the passes added by a second launch
//   pcl_kernel_large_exp.hpp        ... the exponential constraint there (PCL_LARGE_N | PCL_LARGE_EXP): the substepped Taylor polynomial in action form, the derivative carried through it
//   pcl_kernel_large_rollout.hpp    ... their rollout (option large_full): substepped Taylor propagators by column panels, then the chain of the knots
//   pcl_kernel_pade_large_hess.hpp  ... their Hessian of the Lagrangian (option large_hess): forward Horner chain, backward chains on G^T, per-column partial sums
//   pcl_kernels_hessian.hpp    Hessian of the Lagrangian: versions 1 (one workgroup per interval) and 2 (column chunks, fallback)
//   pcl_kernel_hessian_v3.hpp  Hessian of the Lagrangian, default: one workgroup per interval, jobs split by drive
//   pcl_kernels_misc.hpp       compact -> full expansion, rollout, derivative / time rows, terminal infidelity
//   pcl_kernel_exp.hpp         the exact exponential integrator (PCL_ORDER_EXP): residual and Jacobian through Frechet pairs
//   pcl_kernel_exp_hess.hpp    ... its Hessian of the Lagrangian (option exp_hess): second Frechet derivatives, one chain per drive
//   pcl_kernel_exp_merit.hpp   ... its reduce payload without the Jacobian (option exp_full): one adjoint pair chain per interval
//   pcl_kernel_var_exp_hess.hpp ... the same of a variational context (option var_exp_hess): third Frechet derivatives, an octuple chain per (variation, drive)
//   pcl_kernel_var_exp_hess_tiles.hpp ... its octuple chain with four tiles in a device workspace (option var_exp_hess_tiles): generator dimensions 46 .. 62
//   pcl_kernel_var_exp.hpp     the variational integrators on the exponential constraint (PCL_BATCH_VARIATIONAL_EXP): residual and Jacobian
// and the host side beside this file in pcl_host_*.hpp, included in place: the launch ladders launch_fused (pcl_host_launch_pade.hpp) and launch_hess
// (pcl_host_launch_hess.hpp) with one launcher per kernel family, on the helpers of pcl_host_launch.hpp; the large rollout's launcher stays in this file.
// pcl_host_service.hpp has the kinds of context, the families of entry points and the one table of which kind serves which family under which option:
// every entry point that a kind may refuse starts with require(ctx, family, its name), and the refusal sentences are stated there, once per kind.
// pcl_host_options.hpp is pcl_set_option / pcl_get_option as one table of keys.
// DESIGN.md has the full account.  No CPU fallback exists: every entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include "piccolo_hip.h"
#ifdef PCL_LAB
#include "piccolo_hip_lab.h"
#endif
#include "pcl_codegen.hpp"
#include "pcl_codegen_v4.hpp"

#define PCL_VERSION_STR "piccolo_hip 0.4.0 (gfx950, pade 2/4/6/8/10)"

#include "pcl_device_common.hpp"
#include "pcl_kernels_reference.hpp"
#include "pcl_kernel_pade_v2.hpp"
#include "pcl_device_large.hpp"
#include "pcl_kernel_pade_large.hpp"
#include "pcl_kernel_pade_large_hess.hpp"
#include "pcl_kernel_large_rollout.hpp"
#include "pcl_kernel_large_exp.hpp"
#include "pcl_kernel_large_exp_hess.hpp"
#include "pcl_kernels_fused_v2.hpp"
#include "pcl_kernel_fused_v3.hpp"
#include "pcl_kernel_eval.hpp"
#include "pcl_kernel_fused_small.hpp"
#include "pcl_kernels_hessian.hpp"
#include "pcl_kernel_hessian_v3.hpp"
#include "pcl_kernels_misc.hpp"
#include "pcl_kernels_objective.hpp"
#include "pcl_kernel_exp_hess.hpp"
#include "pcl_kernel_exp.hpp"  // (its payload variant reduces with the Hessian kernel's exph_block_sum)
#include "pcl_kernel_exp_merit.hpp"
#include "pcl_host_expand.hpp"

// ------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------
static thread_local std::string g_create_error;

struct pcl_ctx {
    pcl_desc desc;
    int n, K;
    int cols;  // state columns (d for unitaries, 1 for kets)
    int vec = 0;  // PCL_STATE_VECTOR: n = desc.d (general generator on one column; general-order kernel only)
    int large = 0;  // PCL_LARGE_N with 66 <= n <= 128: every residual / Jacobian launch is pcl_pade_large_kernel (pcl_kernel_pade_large.hpp); compact Jacobian and merit / reduce are refused without the option large_reduce, and so are the Hessian of the Lagrangian, the rollout and the objective without the options below
    int large_hess = 0;                    // ... option large_hess: the Hessian of the Lagrangian is served (pcl_kernel_pade_large_hess.hpp)
    int64_t opt_large_hess_drives = 0;     // ... ... the most drives per group of that launch (0 auto: as many as fit)
    int large_full = 0;                    // ... option large_full: the objective family and the rollout are served (pcl_kernel_large_rollout.hpp; its workspace is dexpm)
    int large_reduce = 0;                  // ... option large_reduce: the compact Jacobian trio, the host calls' compact route and the merit / reduce payload are served (the modes of pcl_kernel_pade_large.hpp, pcl_expand_large_kernel)
    int64_t opt_large_rollout_stage = 0;   // ... ... measurements: 0 both launches of the rollout | 1 the propagators only | 2 the chain only, on the workspace as it stands
    double *dlhpart = nullptr;             // ... ... its workspace: per (member, interval, state column) the m (m + 1) + 1 partial sums (allocated when the option is first set to 1)
    int large_exp = 0;                     // ... PCL_LARGE_EXP with PCL_ORDER_EXP (then `large` and `exp` are set too): every residual / Jacobian launch is pcl_large_exp_kernel (pcl_kernel_large_exp.hpp); large_full serves the objective and the rollout, the two options below the Hessian of the Lagrangian and the compact Jacobian / reduce payload, everything else is refused
    int64_t opt_large_exp_drives = 0;      // ... ... the most drives per group of that launch (0 auto)
    int large_exp_hess = 0;                // ... ... option large_exp_hess: its Hessian of the Lagrangian is served (pcl_kernel_large_exp_hess.hpp)
    int64_t opt_large_exp_hess_drives = 0; // ... ... ... the most drives per group of that launch (0 auto: as many as fit)
    int large_exp_reduce = 0;              // ... ... option large_exp_reduce: the compact Jacobian trio, the host calls' compact route and the merit / reduce payload are served (the modes of pcl_kernel_large_exp.hpp, pcl_exp_expand_large_kernel)
    double *dlehpart = nullptr;            // ... ... ... its workspace: per (member, interval, state column) the (m + 1)(m + 2) / 2 partial sums (allocated when the option is first set to 1)
    int exp = 0;  // PCL_ORDER_EXP: delta_k = X_{k+1} - exp(dt_k G(u_k)) X_k (pcl_kernel_exp.hpp); no order; the Hessian, the compact Jacobian and the payload by option
    int exp_hess = 0;            // ... option exp_hess: the Hessian of the Lagrangian is served (pcl_kernel_exp_hess.hpp)
    int exp_full = 0;            // ... option exp_full: the compact Jacobian trio, the host expansion and the merit / reduce payload are served
    double *dexph = nullptr;     // ... its workspace: [G(u_k) | W_k | norm] per (member, interval)
    long long exph_cap = 0;
    int var = 0;  // PCL_BATCH_VARIATIONAL: the number of variations v (x_dim is then the stacked (1 + v) x_dim of the components)
    int vexp = 0;           // ... PCL_BATCH_VARIATIONAL_EXP: the exponential constraint on the lifted generator (pcl_kernel_var_exp.hpp; its workspace is dexph)
    int var_exp_hess = 0;   // ... ... option var_exp_hess: its Hessian of the Lagrangian is served (pcl_kernel_var_exp_hess.hpp)
    double *dvexph = nullptr, *dvexph_part = nullptr;  // ... ... that launch's workspace [G(u_k) | norm | W_0 | W_i] and partial sums, per interval
    int opt_vexph_tiles = 0;  // ... ... option var_exp_hess_tiles: 0 nine LDS tiles | 1 four of them in the workspace where nine do not fit | 2 always
    int vexph_ws = 0;         // ... ... the plan in force since var_exp_hess was last set to 1 (pcl_kernel_var_exp_hess_tiles.hpp)
    double *dvexph_tiles = nullptr;  // ... ... the homes of Tab, Tac, Tbc, Tabc per octuple workgroup (allocated when that plan is first chosen)
    long long var_xdc = 0;  // ... x_dim of one component
    int var_nl = 0;         // ... dimension of the lifted generator (the order policy's norms)
    double *dvar_tab = nullptr;  // ... [G_drift | G_l | Gv_i | the same transposed], n x n column-major each
    int *dvar_ecol = nullptr;       // ... row-compressed tables of the column role: G(u)'s union pattern, the drives, the variation generators
    double *dvar_eval = nullptr;
    int var_wG = 0, var_wD = 0, var_wV = 0;
    long long var_off_d = 0, var_voff_d = 0, var_off_v = 0, var_voff_v = 0;
    int64_t opt_var_blocks = 0, opt_var_cols = 0;  // ... block / column workgroups per interval of the fused launch (0 auto)
    int large_var = 0;                    // ... PCL_LARGE_N | PCL_LARGE_VAR with 66 <= n <= 128: every residual / Jacobian launch is pcl_var_large_kernel (pcl_kernel_var_large.hpp); everything else is refused; its tables are dupos / ducoef / dell_* (the drives, as a plain large context has them) and the two below
    int large_var_full = 0;               // ... ... option large_var_full: the robust-control objective family and the rollout of the stacked state are served (pcl_host_robust.hpp, pcl_kernel_var_large_rollout.hpp; its workspace is dexpm)
    int64_t opt_var_large_drives = 0;     // ... ... the most drives per group of that launch (0 auto: all of them where they fit)
    int *dvl_gcol = nullptr;              // ... ... the variation generators row-compressed, [v][n][vl_gw] (row-major, zero padded)
    double *dvl_gval = nullptr;
    int vl_gw = 0;
    int large_var_hess = 0;               // ... ... option large_var_hess: the Hessian of the Lagrangian is served (pcl_kernel_var_large_hess.hpp; its workspace is dlhpart, its tables dellt_* and the two below)
    int64_t opt_large_var_hess_drives = 0;  // ... ... ... the most drives per group of that launch (0 auto: as many as fit)
    int *dvl_gtcol = nullptr;             // ... ... ... the transposed variation generators row-compressed, [v][n][vl_gtw] (allocated when the option is first set to 1)
    double *dvl_gtval = nullptr;
    int vl_gtw = 0, vl_etw = 0;           // ... ... ... the widths of those rows and of the transposed drive rows (dellt_*)
    int large_var_exp = 0;                // ... ... PCL_LARGE_VAR_EXP with PCL_BATCH_VARIATIONAL_EXP (then `large_var` and `vexp` are set too): every residual / Jacobian launch is pcl_var_large_exp_kernel (pcl_kernel_var_large_exp.hpp); large_var_full serves the objective and the rollout, everything else is refused
    int64_t opt_large_var_exp_drives = 0; // ... ... ... the most drives per chain unit of that launch (0 auto: the plan's count)
    int large_var_exp_hess = 0;           // ... ... ... option large_var_exp_hess: its Hessian of the Lagrangian is served (pcl_kernel_var_large_exp_hess.hpp; its tables are dellt_* and dvl_gt*, its workspace the two below)
    int64_t opt_large_var_exp_hess_drives = 0;  // ... ... ... ... the most drives per group of that launch (0 auto: the plan's count)
    double *dvleh_part = nullptr;         // ... ... ... ... per (interval, pass, state column) the (m + 1)(m + 2) / 2 partial sums (allocated when the option is first set to 1)
    double *dvleh_vec = nullptr;          // ... ... ... ... per (interval, pass b >= 1) what the pass adds to the (u_l, X_0) and (dt, X_0) vectors: (m + 1) n cols doubles
    int var_full = 0;            // ... option var_full: the objective and the rollout are served (pcl_host_robust.hpp)
    int var_compact = 0;         // ... option var_compact: the compact Jacobian trio and the host expansion are served (either constraint kind)
    std::vector<double> var_w;   // ... [w_0 | w_1 .. w_v]: the infidelity's weight and the sensitivity terms' coefficients
    double *dvar_coef = nullptr; // ... the objective Hessian's coefficients [-s w_0 Q sigma | |x_i,N|^2]
    // ... regularisers that cover a component with a dense triangle at the terminal knot (pcl_host_robust.hpp: var_hess_plan)
    std::vector<int> var_last_src;    // kept slots of the terminal knot's regulariser block
    std::vector<double> var_diag;     // [triangle][dt_power][x_dim of a component]: R summed over the covering regularisers
    int *dvar_last_src = nullptr;
    double *dvar_diag = nullptr, *dvar_scratch = nullptr;
    long long var_scratch_cap = 0;
    long long x_dim;
    std::vector<int32_t> x_offs;
    int device;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // device copies
    double *dG0 = nullptr, *ducoef = nullptr, *dcsr_val = nullptr, *dcsc_val = nullptr;
    double *dGjd = nullptr;  // small systems (n <= 8): the drives dense, [m][n*n] column-major (pcl_fused_small_kernel)
    int *dupos = nullptr, *dcsr_ptr = nullptr, *dcsr_col = nullptr, *dcsc_ptr = nullptr, *dcsc_row = nullptr, *dxoffs = nullptr;
    int n_upos = 0;
    int *dumap = nullptr, *dell_col = nullptr;
    double *dell_val = nullptr;
    int ell_w = 0, iso = 0, uell_w = 0;
    unsigned char *duell_l = nullptr;
    double *duell_v = nullptr;
    int *dellt_col = nullptr;  // ELL form of G_l^T (Hessian kernel v2)
    double *dellt_val = nullptr;
    int ellt_w = 0;
    int drives_antisym = 0;  // every G_l == -G_l^T exactly
    double *dug0 = nullptr;
    int64_t opt_general_threads = 512;
    int64_t opt_general_version = 0;   // 0 auto (the lock-step kernel where it fits) | 1 reference formulation | 2 lock-step kernel or error
    int64_t opt_general_slices = 0;    // lock-step kernel: slices per interval (0 auto)
    double *dreduce = nullptr;  // staging of pcl_reduce_sum (host buffer)
    int64_t reduce_cap = 0;
    double *dexpm = nullptr, *dxout = nullptr;  // rollout scratch: propagators, staged output of the host-pointer call
    double *dhpart = nullptr;  // Hessian v2 scratch: per (b,k,slice) partial scalar entries + per (b,k) arrival counters
    unsigned int *dhcnt = nullptr;
    long long hpart_cap = 0;
    int64_t opt_hess_kernel = 0, last_hess_kernel = 0;  // 0 = auto
    // pattern-compiled kernels (pcl_codegen.hpp): plan, device tables, per-interval value table of G(u_k)
    pcl_codegen::SpPlan *sp_plan = nullptr;
    int *dsp_pos = nullptr;
    double *dsp_coef = nullptr, *dsp_glv = nullptr, *dsp_gvals = nullptr;
    long long sp_gvals_cap = 0;  // intervals the value table holds
    int sp_failed = 0;           // the source did not compile: the other kernels serve the context
    int sp_hess_unfit = 0;       // the Hessian kernel's tiles do not fit LDS (d = 32 with 5 or 6 drives)
    hipFunction_t sp_fval = nullptr, sp_fhess = nullptr, sp_feval = nullptr;  // compiled on first use, kept for the context's lifetime
    int *dsp_pos_n = nullptr;       // the same tables in the emission order of the residual kernel's products
    double *dsp_coef_n = nullptr;
    // pattern-compiled FUSED residual + Jacobian kernel (pcl_codegen_v4.hpp, any Pade order): plan, drift tables, magnitudes
    pcl_codegen::V4Plan *v4_plan = nullptr;
    double *dv4_tab = nullptr, *dv4_tab_t = nullptr, *dv4_mags = nullptr, *dv4_dcf = nullptr;
    hipFunction_t v4_ft = nullptr;  // the fused kernel of the module WITH the slice-ticket roles (launches of several trajectories)
    int v4_ft_failed = 0;           // ... could not be had: those launches take the static split of v4_f (same bits)
    hipFunction_t v4_f1 = nullptr;  // the fused kernel of the module of launches with ONE item per workgroup (SP4_ONE_ITEM: one trajectory per launch)
    int v4_f1_failed = 0;           // ... could not be had: those launches take the general module v4_f (same bits)
    int64_t opt_v4_one_item = -1;   // -1 auto (every launch the module serves) | 0 the general module | 1 require (a launch it does not serve is an error)
    int64_t last_v4_one_item = 0;   // the last kernel-4 launch ran the one-item module
    // v4_ticket = -1 (auto), launches of several trajectories: static split or slice tickets, decided PER VALUES ARRAY by timing both on it (the
    // two give the same bits).  The static split's time depends on where the array's pages live (181-228 us per 8 seeds by array and box), the
    // tickets' hardly (193-217): neither wins everywhere.  Per array: 2 untimed launches, then 3 + 3 timed ones alternating (events on the launch
    // stream, read back without blocking), then the faster variant for good (tickets unless the static split is 2 % ahead).
    struct V4Tune {
        const void *key = nullptr;
        long long units = 0;
        int calls = 0, choice = -1, done[2] = {0, 0}, pend_variant[8] = {0};
        float best[2] = {1e30f, 1e30f};
        hipEvent_t ev[8][2] = {};
        bool pend[8] = {false};
        unsigned long long stamp = 0;
    } v4_tune[4];
    unsigned long long v4_tune_clock = 0;
    int64_t last_v4_tune_choice = -1, last_v4_tune_static_ns = 0, last_v4_tune_ticket_ns = 0;
    hipFunction_t v4_f = nullptr, v4_feval = nullptr, v4_fevalc = nullptr /* cooperative residual kernel (optional) */, v4_fhess = nullptr, v4_fhess2 = nullptr /* two workgroups per interval */;
    hipFunction_t v4_fhessc = nullptr;  // general-order Hessian, one wave per group of state columns (pcl_kernel_hess_cols.hpp)
    double *dhcx = nullptr;             // ... the waves' rows of reduced sums and the intervals' arrival counters (self-resetting)
    unsigned int *dhcc = nullptr;
    long long hc_cap = 0;
    double *dhcr = nullptr;             // ... [interval][q - 2][d][n]
    unsigned int *dhcf = nullptr;       // ... [interval] R-chain waves that have delivered (self-resetting)
    long long hcr_cap = 0;
    int64_t opt_hess_rpre = -1;         // -1 auto (launches of more than n_cu / 2 intervals: 1) | 0 the chain inside the column-group waves | 1 R-chain waves in the same launch
    int64_t last_hess_rpre = 0;
    hipFunction_t v4_fhessp = nullptr;  // ... launches of at most n_cu / 2 intervals (one trajectory): a chain wave and a contribution wave per column group (pcl_hess_cols_pair_kernel)
    int64_t opt_hess_pair = -1;         // -1 auto (on for such launches) | 0 one wave per column group | 1 wherever the kernel fits
    int64_t last_hess_pair = 0;
    int v4_hessc_failed = 0;
    double *dh4x = nullptr;        // general-order Hessian, two workgroups per interval: their rows of reduced sums ...
    unsigned int *dh4c = nullptr;  // ... and the arrival counters (self-resetting)
    long long h4_cap = 0;
    int64_t opt_hess_split = -1, last_hess_split = 0;  // -1 auto (launches of at most n_cu / 2 intervals) | 0 | 1
    int64_t opt_v4_tune = 1;  // v4_ticket auto: 1 the static split or the slice tickets by timing both on the values array | 0 always tickets (round 4)
    int64_t opt_hess_xcd = -1;  // column-group Hessian kernel: the waves of an interval on one XCD (-1 auto: 8 | 0 / 1 blockIdx order | n)
    int64_t opt_eval_coop = -1, last_eval_coop = 0;  // residual only: four waves per interval (-1 auto: launches of at most two intervals per CU)
    int v4_hess_failed = 0;
    int v4_failed = 0;
    int64_t opt_v4_variant = 0;     // PCL_PROFILE builds: timing variants of the generated product (wrong results)
    int last_objective_launches = 0;  // what the last pcl_objective_dev launched: 1 (one grid) | 2
    int64_t opt_objective_launches = 0;  // 0 auto | 2: always the two launches (A/B, tests)
    int last_step_launches = 0;  // what the last pcl_eval_jac_merit_objective_dev launched (get_option)
    int64_t opt_v4_flags = 0, opt_v4_np = 0;  // kernel 4 A/B switches (KParams::v4_flags); tiles of the powers of G (0 auto)
    int64_t opt_v4_ticket = -1;     // kernel 4: slice tickets (-1 auto: full-value launches of several intervals per CU at orders 2 and 4 | 0 static split | 1)
    int64_t opt_v4_ticket_cols = 0; // ... state columns per slice ticket (0 auto: 3)
    int64_t opt_v4_ticket_ahead = 2; // ... when the next slice is asked for: 0 when the stream waves have issued this one's stores | 1 a slice ahead | 2 at this one's last column (default)
    int64_t opt_v4_group = 0;       // ... workgroups per group (0 auto: 8, one per XCD)
    bool ticket_launched = false;   // a launch that works on the context's self-resetting device counters (slice tickets; the arrival counters and exchange rows of the split / column-group Hessian kernels) has been enqueued on the current stream (see change_stream)
    int64_t last_v4_ticket = 0;     // state columns per block ticket of the last kernel-4 launch (0: static work split)
    unsigned int *dv4_tick = nullptr;  // ... [block ticket, pipelines gone, chain ticket]: zero between launches (the last pipeline out resets them)
    int *herr = nullptr, *derr = nullptr;  // device error word (host-mapped): a barrier-free kernel whose bounded wait gave up sets bit 0
#ifdef PCL_LAB
    // RESIDENT evaluator (pcl_resident_*; pcl_kernel_fused_sparse.hpp, SP4_RESIDENT): kernel 4's workgroups stay on the device and run one
    // evaluation per posted request
    struct Resident {
        hipStream_t stream = nullptr;  // its own: work queued behind a resident kernel waits for it to leave
        hipFunction_t f = nullptr;
        unsigned *hbox = nullptr, *hbox_dev = nullptr, *dbox = nullptr;  // the host's words (mapped) and the device's (layout: see the kernel)
        unsigned *hinit = nullptr;                                        // pinned source of the device words' start values
        KParams *dparams = nullptr, *hparams = nullptr;                   // the evaluation's parameter block in device memory (the kernel reads it per request, where it is used) and its pinned source
        KParams p;
        const double *tab = nullptr, *dcf = nullptr;
        long long grid = 0;
        size_t lds = 0;
        unsigned block = 0, posted = 0;
        bool active = false, launched = false;
        int64_t launches = 0;
    } res;
    bool res_capture = false;            // launch_fused_v4 fills `res` instead of launching
    int64_t opt_resident_idle_us = 5000; // the resident kernel leaves after this long without a request (the next request starts it again)
#else
    static constexpr bool res_capture = false;  // (the shipped library has no resident evaluator: include/piccolo_hip_lab.h)
#endif
    int64_t opt_v4_tail_mode = 3;   // kernel 4: who stores delta and the tails: 0 the writer wave | 1 ... nontemporal | 2 ... write-through | 3 the stream waves (default)
    int64_t opt_eval_kernel = 0;    // 0 auto | 1 matrix-core residual kernel | 2 pattern-compiled
    // staging for the host-pointer entry points
    double *dZ = nullptr, *dmu = nullptr, *ddelta = nullptr, *dvals = nullptr, *dhess = nullptr;
    // options
    // host-pointer entry points: pinned staging + compact D2H + threaded expansion into the caller's array
    pcl_host::Pool *pool = nullptr;
    double *hZ = nullptr, *hcompact = nullptr, *hdelta = nullptr;  // pinned (hipHostMalloc)
    double *dcomp_host = nullptr;                                    // device buffer of the compact values
    hipEvent_t ev_chunk[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t opt_prof = 0;  // -DPCL_PROFILE builds only
    int64_t opt_host_threads = 0, opt_host_path = 0, opt_host_chunks = 4;
    int64_t opt_host_store_bytes = 0, last_host_store_bytes = 0;  // streaming-store width of the host expansion: 0 the widest the host has | 16 | 32 | 64
    int host_threads_tuned = 0;       // auto: the thread count the sweep over the context's first host-delivered calls found fastest
    int host_tune_calls = 0;          // ... calls sampled so far
    double host_tune_t[8] = {1e300, 1e300, 1e300, 1e300, 1e300, 1e300, 1e300, 1e300};
    double host_expand_GBps = 0.0;    // ... the delivered rate of the fastest sampled call
    int win_first = 0, win_count = 0;  // member window (pcl_set_member_window): the members / seeds the evaluator entry points cover
    int64_t opt_cols_per_slice = 0, opt_use_mfma = 1, opt_nt = -1 /* auto by launch size */, opt_kernel = 0;  // 0 = auto: 3 where its specialised instance applies, else 1 / 2 by shape
    long long *ddbg = nullptr;
    void *comm = nullptr;  // ncclComm_t
    double *dgoal = nullptr;  // iso-vec of the goal unitary (pcl_set_goal) or of its subspace block (pcl_set_goal_subspace)
    int *dsub = nullptr;      // subspace indices of an embedded goal
    int n_sub = 0;            // 0: full-space fidelity
    double *dweights = nullptr;  // per member / seed weights of the objective (NULL: ones)
    // the terminal loss in its general form F = c'x + sum_r (A_r'x)^2 (pcl_kernels_objective.hpp): set by pcl_set_goal_form (form_user: value and
    // gradient go through it too) or derived from the unitary goal (for the Hessian of the objective only)
    double *dformA = nullptr, *dformc = nullptr, *dgram = nullptr, *dcoef = nullptr;
    int form_R = 0, form_L = 0, form_scope = 0;
    bool form_user = false, gram_ready = false;
    std::vector<PclReg> regs;    // quadratic regularisers (pcl_add_regularizer)
    std::vector<double> reg_R;
    PclReg *dregs = nullptr;
    double *dreg_R = nullptr;
    bool regs_dirty = false;
    double *dobj = nullptr;      // objective scratch: per-member values | per-knot regulariser values
    double *dphik = nullptr;     // merit scratch: per-interval partial sums
    double *dmcols = nullptr;    // fused merit: per-column partial dot products written by fused kernel 3
    unsigned int *dmticket = nullptr;  // ... arrival ticket of pcl_merit_finish_kernel (zero between launches)
    bool tickets_dirty = true;   // the arrival tickets (objective sum, merit finish) are re-zeroed on the stream before their next use:
                                 // set at allocation and whenever the stream changes (the last-arriving workgroup resets them otherwise)
    const double *merit_lam = nullptr;  // set for the duration of pcl_eval_jac_merit_dev
    int merit_want = 0, merit_fused = 0;
    double *dgrad = nullptr, *dval = nullptr;  // staging of the host-pointer objective call
    int64_t opt_specialize = 1;
    int64_t opt_jit = 1;      // compile shape-specialised instances on first use (hiprtc) for shapes outside the static table
    int64_t opt_require_jit = 0;  // 1: a pattern-compiled kernel that cannot be had (no libhiprtc, no headers, compile error) is an error, not a fallback
    int64_t jit_fallbacks = 0;    // pattern-compiled kernels this context wanted and did not get (the matrix-core / general kernels serve it)
    int64_t opt_general = 0;  // 1: run the general-order kernel also for pade_order 4 (cross-check)
    int64_t opt_contig = -1;     // v3: contiguous column ranges per workgroup (-1: auto by launch size)
    int64_t opt_stream_wg = -1;  // v3, contiguous: stream-role workgroups (-1: auto = half, 0: every workgroup does both)
    int64_t last_n_stream = 0;  // stream-role workgroups of the last kernel-3 launch (0: fused roles / round-robin)
    int64_t last_kernel = 0;  // 10*version + (1 if shape-specialised) of the last fused launch
    int64_t opt_grid = 0;  // 0: resident workgroups (persistent kernel)
    size_t lds_set[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const void *lds_kern[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // last MaxDynamicSharedMemorySize set per kernel variant
    int max_lds = 0;
    int n_cu = 0;
    // order policy (pade_order = 0 in the descriptor): host copies of the generators for the norm bound, the tolerance, what was found
    std::vector<double> hG0, hGj;
    double order_tol = 1e-10, order_theta = 0.0;
    int order_tol_met = 1;  // 0: the order policy had to settle for order 10 above its tolerance (note_order)
    mutable std::string err;
};

static int fail(const pcl_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->err = buf;
    else
        g_create_error = buf;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(ctx, PCL_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

#define TRY(expr)                 \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != PCL_OK) return rc_; \
    } while (0)

// Every entry point runs on the context's device and leaves the caller's current device as it found it.
namespace {
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            changed = err == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
};
}  // namespace
#define ON_DEVICE(ctx)                                                                                         \
    DeviceGuard dev_guard_((ctx)->device);                                                                     \
    if (dev_guard_.err != hipSuccess) return fail(ctx, PCL_EHIP, "hipSetDevice(%d): %s", (ctx)->device, hipGetErrorString(dev_guard_.err))

// LDS of the fused pattern-compiled kernel: m + 4 chain tiles (D, S, W, V, dW_l) + np tiles of the powers of G + counters
static size_t v4_lds_bytes(int d, int m, int np) { return ((size_t)(m + 4 + np) * d * (2 * d + 1) + 24) * sizeof(double); }
// tiles for the powers of G: q + 1 when they fit (one-item launches use q: the stream never waits for the P wave; ticket launches let the
// P wave start the next item's first power while the stream folds this item's last), else as many as fit (>= 2)
static int v4_power_tiles(int d, int m, int q, size_t max_lds) {
    int np = q + 1;
    while (np > 2 && v4_lds_bytes(d, m, np) > max_lds) --np;
    return v4_lds_bytes(d, m, np) <= max_lds ? np : 0;
}

static long long var_jac_per(const pcl_ctx *c);
static long long jac_per_full(const pcl_ctx *c) {
    if (c->var) return var_jac_per(c);
    if (c->exp) return (long long)c->cols * c->n * c->n + c->x_dim * (c->desc.n_drives + 2);  // -E copies | the diagonal of I | tails
    return 2LL * c->cols * c->n * c->n + c->x_dim * (c->desc.n_drives + 1);
}
static long long jac_per_compact(const pcl_ctx *c) {
    // a variational context (option var_compact): -B+ | B- | per variation -L+_i | L-_i | tails; exponential: -E | -L_1 .. -L_v | tails
    if (c->var) return (c->vexp ? 1LL + c->var : 2LL + 2LL * c->var) * c->n * c->n + c->x_dim * (c->desc.n_drives + 1);
    if (c->exp) return (long long)c->n * c->n + c->x_dim * (c->desc.n_drives + 1);  // -E | tails (option exp_full)
    return 2LL * c->n * c->n + c->x_dim * (c->desc.n_drives + 1);
}
static long long hess_per(const pcl_ctx *c) {
    const long long m = c->desc.n_drives;
    if (c->exp || c->vexp) return (m + 1) * (m + 2) / 2 + c->x_dim * (m + 1);  // nothing involves X_{k+1}
    return (m + 1) * (m + 2) / 2 + 2 * c->x_dim * (m + 1);
}
static long long z_len(const pcl_ctx *c) {
    return (long long)c->desc.z_dim * c->desc.N * (c->desc.batch_mode == PCL_BATCH_TRAJ ? c->desc.batch : 1);
}
static long long n_rows(const pcl_ctx *c) { return (long long)c->win_count * c->x_dim * c->K; }        // of the member window
static long long n_rows_all(const pcl_ctx *c) { return (long long)(c->var ? 1 : c->desc.batch) * c->x_dim * c->K; }  // of every member (allocation sizes)

extern "C" const char *pcl_version(void) { return PCL_VERSION_STR; }

extern "C" const char *pcl_last_error(const pcl_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

template <class T>
static int upload(pcl_ctx *ctx, T **dst, const std::vector<T> &src) {
    const size_t bytes = std::max<size_t>(src.size(), 1) * sizeof(T);
    HIP_TRY(ctx, hipMalloc((void **)dst, bytes));
    if (!src.empty()) HIP_TRY(ctx, hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return PCL_OK;
}

#include "pcl_host_jit.hpp"
#include "pcl_host_launch.hpp"
#include "pcl_host_service.hpp"
#include "pcl_host_variational.hpp"

extern "C" int pcl_create(const pcl_desc *dsc, pcl_ctx **out) {
    if (!out) return fail(nullptr, PCL_EINVAL, "pcl_create: out is NULL");
    *out = nullptr;
    if (!dsc) return fail(nullptr, PCL_EINVAL, "pcl_create: desc is NULL");
    if (dsc->struct_size != (int32_t)sizeof(pcl_desc))
        return fail(nullptr, PCL_EINVAL, "pcl_create: desc.struct_size=%d, library expects %zu (ABI mismatch)",
                    dsc->struct_size, sizeof(pcl_desc));
    // PCL_LARGE_N, PCL_LARGE_EXP, PCL_LARGE_VAR and PCL_LARGE_VAR_EXP: stripped here, once; everything below (and the context) sees the plain batch mode
    const bool large_flag = dsc->batch_mode >= 0 && (dsc->batch_mode & PCL_LARGE_N) != 0;
    const bool large_exp_flag = dsc->batch_mode >= 0 && (dsc->batch_mode & PCL_LARGE_EXP) != 0;
    const bool large_var_flag = dsc->batch_mode >= 0 && (dsc->batch_mode & PCL_LARGE_VAR) != 0;
    const bool large_var_exp_flag = dsc->batch_mode >= 0 && (dsc->batch_mode & PCL_LARGE_VAR_EXP) != 0;
    pcl_desc plain_desc = *dsc;
    if (large_var_exp_flag) {
        // the one valid combination: PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP with pade_order = PCL_ORDER_EXP
        plain_desc.batch_mode &= ~(PCL_LARGE_N | PCL_LARGE_EXP | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP);
        dsc = &plain_desc;
        if (!large_flag || !large_var_flag)
            return fail(nullptr, PCL_EINVAL, "pcl_create: PCL_LARGE_VAR_EXP goes with %s (PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP, pade_order = PCL_ORDER_EXP)",
                        !large_flag && !large_var_flag ? "PCL_LARGE_N and PCL_LARGE_VAR" : !large_flag ? "PCL_LARGE_N" : "PCL_LARGE_VAR");
        if (dsc->batch_mode == PCL_BATCH_MEMBERS || dsc->batch_mode == PCL_BATCH_TRAJ)
            return fail(nullptr, PCL_EINVAL, "pcl_create: PCL_LARGE_VAR_EXP is the variational exponential constraint at generator dimensions 66 .. %d: it needs batch_mode PCL_BATCH_VARIATIONAL_EXP, not %s",
                        PCL_LARGE_MAX_N, dsc->batch_mode == PCL_BATCH_MEMBERS ? "PCL_BATCH_MEMBERS" : "PCL_BATCH_TRAJ");
        if (dsc->batch_mode == PCL_BATCH_VARIATIONAL)
            return fail(nullptr, PCL_EINVAL, "pcl_create: PCL_LARGE_VAR_EXP is the variational exponential constraint at generator dimensions 66 .. %d: it needs batch_mode PCL_BATCH_VARIATIONAL_EXP, not PCL_BATCH_VARIATIONAL (the Pade constraint takes PCL_LARGE_N | PCL_LARGE_VAR alone)",
                        PCL_LARGE_MAX_N);
        if (dsc->batch_mode != PCL_BATCH_VARIATIONAL_EXP)
            return fail(nullptr, PCL_EINVAL, "pcl_create: PCL_LARGE_VAR_EXP needs batch_mode PCL_BATCH_VARIATIONAL_EXP, not batch_mode %d", dsc->batch_mode);
        if (dsc->pade_order != PCL_ORDER_EXP)
            return fail(nullptr, PCL_EINVAL, "pcl_create: PCL_LARGE_VAR_EXP is the exponential constraint: it needs pade_order = PCL_ORDER_EXP, not a Pade order (got %d)", dsc->pade_order);
        if (large_exp_flag)
            return fail(nullptr, PCL_EINVAL, "pcl_create: PCL_LARGE_VAR_EXP does not go with PCL_LARGE_EXP: that flag belongs to plain contexts (PCL_BATCH_MEMBERS or PCL_BATCH_TRAJ)");
        return var_create(dsc, out, true, true);
    }
    if (large_flag || large_exp_flag || large_var_flag) {
        plain_desc.batch_mode &= ~(PCL_LARGE_N | PCL_LARGE_EXP | PCL_LARGE_VAR);
        dsc = &plain_desc;
        if (large_var_flag && !large_flag)
            return fail(nullptr, PCL_EINVAL, "pcl_create: PCL_LARGE_VAR goes with PCL_LARGE_N (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR, a diagonal Pade order)");
        if (large_var_flag && dsc->batch_mode != PCL_BATCH_VARIATIONAL && dsc->batch_mode != PCL_BATCH_VARIATIONAL_EXP)
            return fail(nullptr, PCL_EINVAL, "pcl_create: PCL_LARGE_VAR is the variational integrators at generator dimensions 66 .. %d: it goes with PCL_BATCH_VARIATIONAL, not with batch_mode %d (PCL_BATCH_MEMBERS and PCL_BATCH_TRAJ take PCL_LARGE_N alone)",
                        PCL_LARGE_MAX_N, dsc->batch_mode);
        if (large_var_flag && (dsc->batch_mode == PCL_BATCH_VARIATIONAL_EXP || large_exp_flag || dsc->pade_order == PCL_ORDER_EXP))
            return fail(nullptr, PCL_ENOTIMPL, "pcl_create: PCL_LARGE_VAR is not implemented for the exponential constraint (%s); it serves PCL_BATCH_VARIATIONAL at the diagonal Pade orders 2 .. 10",
                        dsc->batch_mode == PCL_BATCH_VARIATIONAL_EXP ? "batch_mode PCL_BATCH_VARIATIONAL_EXP" : large_exp_flag ? "the flag PCL_LARGE_EXP" : "pade_order = PCL_ORDER_EXP");
        if (large_exp_flag && !large_flag)
            return fail(nullptr, PCL_EINVAL, "pcl_create: PCL_LARGE_EXP goes with PCL_LARGE_N (batch_mode | PCL_LARGE_N | PCL_LARGE_EXP, pade_order = PCL_ORDER_EXP)");
        if (!large_var_flag && (dsc->batch_mode == PCL_BATCH_VARIATIONAL || dsc->batch_mode == PCL_BATCH_VARIATIONAL_EXP))
            return fail(nullptr, PCL_ENOTIMPL, "pcl_create: PCL_LARGE_N is not implemented for the variational integrators (batch_mode %s); it goes with PCL_BATCH_MEMBERS or PCL_BATCH_TRAJ -- and with PCL_BATCH_VARIATIONAL on the Pade constraint by the flag PCL_LARGE_VAR beside it",
                        dsc->batch_mode == PCL_BATCH_VARIATIONAL ? "PCL_BATCH_VARIATIONAL" : "PCL_BATCH_VARIATIONAL_EXP");
        if (large_exp_flag && dsc->pade_order != PCL_ORDER_EXP)
            return fail(nullptr, PCL_EINVAL, "pcl_create: PCL_LARGE_EXP is the exponential constraint at generator dimensions 66 .. %d: it needs pade_order = PCL_ORDER_EXP (got %d)", PCL_LARGE_MAX_N, dsc->pade_order);
        if (dsc->pade_order == PCL_ORDER_EXP && !large_exp_flag)
            return fail(nullptr, PCL_ENOTIMPL, "pcl_create: PCL_LARGE_N is not implemented for the exponential constraint (pade_order = PCL_ORDER_EXP); it serves the diagonal Pade orders 2 .. 10 -- and that constraint by the flag PCL_LARGE_EXP beside it");
    }
    if (dsc->batch_mode == PCL_BATCH_VARIATIONAL && dsc->pade_order == PCL_ORDER_EXP)
        return fail(nullptr, PCL_ENOTIMPL, "pcl_create: pade_order = PCL_ORDER_EXP (the exponential constraint) with batch_mode = PCL_BATCH_VARIATIONAL is not implemented; use batch_mode = PCL_BATCH_VARIATIONAL_EXP");
    if (dsc->batch_mode == PCL_BATCH_VARIATIONAL || dsc->batch_mode == PCL_BATCH_VARIATIONAL_EXP) return var_create(dsc, out, large_var_flag);
    const bool vec = dsc->state_cols == PCL_STATE_VECTOR;  // general real d x d generator on one real column
    const int d = dsc->d, m = dsc->n_drives, n = vec ? d : 2 * d;
    if (d < 1 || m < 0 || dsc->N < 2 || dsc->batch < 1)
        return fail(nullptr, PCL_EINVAL, "pcl_create: need d>=1, n_drives>=0, N>=2, batch>=1 (got d=%d m=%d N=%d batch=%d)", d,
                    m, dsc->N, dsc->batch);
    if (n > 2 * PCL_MAX_D && !large_flag)
        return fail(nullptr, PCL_ESHAPE, "pcl_create: generator dimension %d exceeds %d (LDS-resident tiles; d <= %d); batch_mode | PCL_LARGE_N serves the Pade constraint up to %d", n, 2 * PCL_MAX_D,
                    PCL_MAX_D, PCL_LARGE_MAX_N);
    if (n > PCL_LARGE_MAX_N)
        return fail(nullptr, PCL_ESHAPE, "pcl_create: generator dimension %d exceeds %d, the most PCL_LARGE_N serves: one n x n LDS tile would take %zu B of the 163840 B a workgroup can have (132096 B at n = %d)",
                    n, PCL_LARGE_MAX_N, (size_t)(n | 1) * n * sizeof(double), PCL_LARGE_MAX_N);
    const bool large = large_flag && n > 2 * PCL_MAX_D;  // (the flag at n <= 64: the ordinary context)
    if (m > 24) return fail(nullptr, PCL_ESHAPE, "pcl_create: n_drives=%d exceeds 24", m);
    if (dsc->pade_order < PCL_ORDER_EXP)
        return fail(nullptr, PCL_ENOTIMPL, "pcl_create: pade_order=%d; accepted values are the diagonal Pade orders 2, 4, 6, 8, 10, 0 (chosen by pcl_set_order_policy) and PCL_ORDER_EXP (-1, the exponential constraint)", dsc->pade_order);
    if (dsc->pade_order != PCL_ORDER_EXP && dsc->pade_order != 0 && dsc->pade_order != 2 && dsc->pade_order != 4 && dsc->pade_order != 6 && dsc->pade_order != 8 && dsc->pade_order != 10)
        return fail(nullptr, PCL_ENOTIMPL, "pcl_create: pade_order=%d; diagonal Pade orders 2, 4, 6, 8, 10 are implemented (0: chosen by pcl_set_order_policy)", dsc->pade_order);
    if (dsc->index_base != 0 && dsc->index_base != 1) return fail(nullptr, PCL_EINVAL, "pcl_create: index_base must be 0 or 1");
    if (dsc->batch_mode != PCL_BATCH_MEMBERS && dsc->batch_mode != PCL_BATCH_TRAJ)
        return fail(nullptr, PCL_EINVAL, "pcl_create: unknown batch_mode %d", dsc->batch_mode);
    if (!dsc->G0 || (m > 0 && !dsc->Gj) || !dsc->x_offs) return fail(nullptr, PCL_EINVAL, "pcl_create: G0/Gj/x_offs must be non-NULL");
    if (dsc->state_cols < 0 && !vec) return fail(nullptr, PCL_EINVAL, "pcl_create: state_cols=%d", dsc->state_cols);
    const int cols = vec ? 1 : (dsc->state_cols > 0 ? dsc->state_cols : d);
    if (cols > d) return fail(nullptr, PCL_EINVAL, "pcl_create: state_cols=%d exceeds d=%d", cols, d);
    const long long x_dim = (long long)n * cols;
    const int n_off = dsc->batch_mode == PCL_BATCH_MEMBERS ? dsc->batch : 1;
    for (int i = 0; i < n_off; ++i)
        if (dsc->x_offs[i] < 0 || dsc->x_offs[i] + x_dim > dsc->z_dim)
            return fail(nullptr, PCL_EINVAL, "pcl_create: x_offs[%d]=%d with x_dim=%lld does not fit z_dim=%d", i, dsc->x_offs[i],
                        x_dim, dsc->z_dim);
    if (dsc->u_off < 0 || dsc->u_off + m > dsc->z_dim || dsc->dt_off < 0 || dsc->dt_off >= dsc->z_dim)
        return fail(nullptr, PCL_EINVAL, "pcl_create: u_off/dt_off outside the knot (z_dim=%d)", dsc->z_dim);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, PCL_EHIP, "pcl_create: no HIP device available (%s); this library has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (dsc->device_id < 0 || dsc->device_id >= ndev) return fail(nullptr, PCL_EINVAL, "pcl_create: device_id %d of %d", dsc->device_id, ndev);

    pcl_ctx *ctx = new (std::nothrow) pcl_ctx();
    if (!ctx) return fail(nullptr, PCL_ENOMEM, "pcl_create: out of host memory");
    ctx->desc = *dsc;
    ctx->n = n;
    ctx->K = dsc->N - 1;
    ctx->x_dim = x_dim;
    ctx->cols = cols;
    ctx->vec = vec ? 1 : 0;
    ctx->large = large ? 1 : 0;
    ctx->large_exp = large && large_exp_flag ? 1 : 0;
    ctx->exp = dsc->pade_order == PCL_ORDER_EXP ? 1 : 0;
    ctx->x_offs.assign(dsc->x_offs, dsc->x_offs + n_off);
    ctx->hG0.assign(dsc->G0, dsc->G0 + (size_t)n * n * (dsc->per_member_G0 ? dsc->batch : 1));
    if (m > 0) ctx->hGj.assign(dsc->Gj, dsc->Gj + (size_t)m * n * n);
    ctx->desc.x_offs = nullptr;
    ctx->desc.G0 = ctx->desc.Gj = nullptr;
    ctx->device = dsc->device_id;
    ctx->win_first = 0;
    ctx->win_count = dsc->batch;
    if (const char *tk = getenv("PCL_V4_TICKET")) {  // default of option "v4_ticket" (A/B of whole programs: -1 auto | 0 static split | 1 slice tickets)
        const long v = strtol(tk, nullptr, 10);
        if (v >= -1 && v <= 1) ctx->opt_v4_ticket = v;
    }
    if (const char *oi = getenv("PCL_V4_ONE_ITEM")) {  // default of option "v4_one_item" (A/B of whole programs: -1 auto | 0 general module | 1 require)
        const long v = strtol(oi, nullptr, 10);
        if (v >= -1 && v <= 1) ctx->opt_v4_one_item = v;
    }
    if (const char *hp = getenv("PCL_HOST_PATH")) {  // default of option "host_path" (1: full values over PCIe, 2: compact + host expansion)
        const long v = strtol(hp, nullptr, 10);
        if (v >= 0 && v <= 2) ctx->opt_host_path = v;
    }

#define CREATE_TRY(expr)                                                  \
    do {                                                                  \
        int rc_ = (expr);                                                 \
        if (rc_ != PCL_OK) {                                              \
            g_create_error = ctx->err;                                    \
            pcl_destroy(ctx);                                             \
            return rc_;                                                   \
        }                                                                 \
    } while (0)
#define CREATE_HIP(expr)                                                                               \
    do {                                                                                               \
        hipError_t e2_ = (expr);                                                                       \
        if (e2_ != hipSuccess) {                                                                       \
            fail(nullptr, PCL_EHIP, "pcl_create: %s: %s", #expr, hipGetErrorString(e2_));              \
            pcl_destroy(ctx);                                                                          \
            return PCL_EHIP;                                                                           \
        }                                                                                              \
    } while (0)

    DeviceGuard dev_guard_(ctx->device);
    CREATE_HIP(dev_guard_.err);
    hipDeviceProp_t prop;
    CREATE_HIP(hipGetDeviceProperties(&prop, ctx->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fail(nullptr, PCL_EHIP, "pcl_create: device %d is %s; this library is built for gfx950 only", ctx->device, prop.gcnArchName);
        pcl_destroy(ctx);
        return PCL_EHIP;
    }
    ctx->max_lds = (int)prop.maxSharedMemoryPerMultiProcessor;
    ctx->n_cu = prop.multiProcessorCount;
    CREATE_HIP(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;

    // --- drive structures: union pattern (+ coefficient table), CSR and CSC of every G_l ------
    const size_t nn = (size_t)n * n;
    std::vector<int> upos;
    std::vector<double> ucoef;
    for (size_t pz = 0; pz < nn; ++pz) {
        bool any = false;
        for (int l = 0; l < m; ++l) any |= dsc->Gj[l * nn + pz] != 0.0;
        if (any) {
            upos.push_back((int)pz);
            for (int l = 0; l < m; ++l) ucoef.push_back(dsc->Gj[l * nn + pz]);
        }
    }
    ctx->n_upos = (int)upos.size();
    std::vector<int> csr_ptr((size_t)std::max(m, 1) * (n + 1), 0), csr_col, csc_ptr((size_t)std::max(m, 1) * (n + 1), 0), csc_row;
    std::vector<double> csr_val, csc_val;
    for (int l = 0; l < m; ++l) {
        const double *A = dsc->Gj + l * nn;  // column-major: A[i + n*j]
        for (int i = 0; i < n; ++i) {
            csr_ptr[(size_t)l * (n + 1) + i] = (int)csr_col.size();
            for (int j = 0; j < n; ++j)
                if (A[i + (size_t)n * j] != 0.0) {
                    csr_col.push_back(j);
                    csr_val.push_back(A[i + (size_t)n * j]);
                }
        }
        csr_ptr[(size_t)l * (n + 1) + n] = (int)csr_col.size();
        for (int j = 0; j < n; ++j) {
            csc_ptr[(size_t)l * (n + 1) + j] = (int)csc_row.size();
            for (int i = 0; i < n; ++i)
                if (A[i + (size_t)n * j] != 0.0) {
                    csc_row.push_back(i);
                    csc_val.push_back(A[i + (size_t)n * j]);
                }
        }
        csc_ptr[(size_t)l * (n + 1) + n] = (int)csc_row.size();
    }
    int uell_w = 0;
    for (size_t q = 0; q < upos.size(); ++q) {
        int cnt = 0;
        for (int l = 0; l < m; ++l) cnt += ucoef[q * m + l] != 0.0;
        uell_w = std::max(uell_w, cnt);
    }
    uell_w = std::max(uell_w, 1);
    std::vector<unsigned char> uell_l(std::max<size_t>(upos.size(), 1) * uell_w, 0);
    std::vector<double> uell_v(std::max<size_t>(upos.size(), 1) * uell_w, 0.0);
    for (size_t q = 0; q < upos.size(); ++q) {
        int cnt = 0;
        for (int l = 0; l < m; ++l)
            if (ucoef[q * m + l] != 0.0) {
                uell_l[q * uell_w + cnt] = (unsigned char)l;
                uell_v[q * uell_w + cnt] = ucoef[q * m + l];
                ++cnt;
            }
    }
    ctx->uell_w = uell_w;
    std::vector<int> umap(nn, -1);
    for (size_t q = 0; q < upos.size(); ++q) umap[upos[q]] = (int)q;
    int ell_w = m > 0 ? 1 : 0;
    for (int l = 0; l < m; ++l)
        for (int i = 0; i < n; ++i) ell_w = std::max(ell_w, csr_ptr[(size_t)l * (n + 1) + i + 1] - csr_ptr[(size_t)l * (n + 1) + i]);
    std::vector<int> ell_col((size_t)m * n * ell_w, 0);
    std::vector<double> ell_val((size_t)m * n * ell_w, 0.0);
    for (int l = 0; l < m; ++l)
        for (int i = 0; i < n; ++i) {
            const int beg = csr_ptr[(size_t)l * (n + 1) + i], end = csr_ptr[(size_t)l * (n + 1) + i + 1];
            for (int q = beg; q < end; ++q) {
                ell_col[((size_t)l * n + i) * ell_w + (q - beg)] = csr_col[q];
                ell_val[((size_t)l * n + i) * ell_w + (q - beg)] = csr_val[q];
            }
        }
    ctx->ell_w = ell_w;
    int ellt_w = m > 0 ? 1 : 0;
    for (int l = 0; l < m; ++l)
        for (int i = 0; i < n; ++i) ellt_w = std::max(ellt_w, csc_ptr[(size_t)l * (n + 1) + i + 1] - csc_ptr[(size_t)l * (n + 1) + i]);
    std::vector<int> ellt_col((size_t)m * n * ellt_w, 0);
    std::vector<double> ellt_val((size_t)m * n * ellt_w, 0.0);
    for (int l = 0; l < m; ++l)
        for (int i = 0; i < n; ++i) {
            const int beg = csc_ptr[(size_t)l * (n + 1) + i], end = csc_ptr[(size_t)l * (n + 1) + i + 1];
            for (int q = beg; q < end; ++q) {
                ellt_col[((size_t)l * n + i) * ellt_w + (q - beg)] = csc_row[q];
                ellt_val[((size_t)l * n + i) * ellt_w + (q - beg)] = csc_val[q];
            }
        }
    ctx->ellt_w = ellt_w;
    {
        bool anti = true;
        for (int l = 0; l < m && anti; ++l)
            for (int j = 0; j < n && anti; ++j)
                for (int i = 0; i < n; ++i)
                    if (dsc->Gj[(size_t)l * nn + i + (size_t)n * j] != -dsc->Gj[(size_t)l * nn + j + (size_t)n * i]) {
                        anti = false;
                        break;
                    }
        ctx->drives_antisym = anti ? 1 : 0;
    }
    // exact iso structure  M = [[A, -B], [B, A]]  of the drift(s) and of every drive?
    auto is_iso = [&](const double *A) {
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) {
                if (A[(i + d) + (size_t)n * (j + d)] != A[i + (size_t)n * j]) return false;
                if (A[i + (size_t)n * (j + d)] != -A[(i + d) + (size_t)n * j]) return false;
            }
        return true;
    };
    bool iso = !vec;  // the iso(.) block structure only exists for n = 2d
    if (iso)
        for (int bb = 0; bb < (dsc->per_member_G0 ? dsc->batch : 1); ++bb) iso = iso && is_iso(dsc->G0 + bb * nn);
    if (iso)
        for (int l = 0; l < m; ++l) iso = iso && is_iso(dsc->Gj + l * nn);
    ctx->iso = iso ? 1 : 0;
    // pattern-compiled kernels: sparse iso generators of a unitary problem, one state column per lane (d <= 32), m + 2 waves
    if (iso && cols == d && d >= 9 && d <= 32 && m >= 1 && m <= 6 && !ctx->exp) {  // (the exponential mode has its one kernel)
        pcl_codegen::SpPlan plan = pcl_codegen::make_plan(d, m, dsc->G0, dsc->per_member_G0 ? dsc->batch : 1, dsc->Gj);
        if (plan.ok && plan.nz <= 640 && (double)plan.nz <= 0.45 * 2.0 * d * d) ctx->sp_plan = new pcl_codegen::SpPlan(std::move(plan));
    }
    if (ctx->sp_plan) {  // the fused kernel of the same family: one LDS tile per chain (m + 7 tiles of d (n + 1) doubles)
        pcl_codegen::V4Plan v4 = pcl_codegen::make_v4_plan(d, m, dsc->G0, dsc->per_member_G0 ? dsc->batch : 1, dsc->Gj);
        if (v4.ok && v4_power_tiles(d, m, std::max(dsc->pade_order, 2) / 2, (size_t)ctx->max_lds) > 0) ctx->v4_plan = new pcl_codegen::V4Plan(std::move(v4));
    }
    std::vector<double> g0(dsc->G0, dsc->G0 + nn * (dsc->per_member_G0 ? dsc->batch : 1));
    CREATE_TRY(upload(ctx, &ctx->dG0, g0));
    if ((n <= 16 || (ctx->exp && !ctx->large_exp)) && m >= 1) {  // (... and the exponential mode at every n <= 64: the directions of its Frechet pairs)
        std::vector<double> gjd(dsc->Gj, dsc->Gj + nn * m);
        CREATE_TRY(upload(ctx, &ctx->dGjd, gjd));
    }
    CREATE_TRY(upload(ctx, &ctx->dupos, upos));
    CREATE_TRY(upload(ctx, &ctx->ducoef, ucoef));
    CREATE_TRY(upload(ctx, &ctx->dcsr_ptr, csr_ptr));
    CREATE_TRY(upload(ctx, &ctx->dcsr_col, csr_col));
    CREATE_TRY(upload(ctx, &ctx->dcsr_val, csr_val));
    CREATE_TRY(upload(ctx, &ctx->dcsc_ptr, csc_ptr));
    CREATE_TRY(upload(ctx, &ctx->dcsc_row, csc_row));
    CREATE_TRY(upload(ctx, &ctx->dcsc_val, csc_val));
    CREATE_TRY(upload(ctx, &ctx->dumap, umap));
    CREATE_TRY(upload(ctx, &ctx->duell_l, uell_l));
    CREATE_TRY(upload(ctx, &ctx->duell_v, uell_v));
    CREATE_TRY(upload(ctx, &ctx->dell_col, ell_col));
    CREATE_TRY(upload(ctx, &ctx->dell_val, ell_val));
    CREATE_TRY(upload(ctx, &ctx->dellt_col, ellt_col));
    CREATE_TRY(upload(ctx, &ctx->dellt_val, ellt_val));
    {
        std::vector<double> ug0(std::max<size_t>(upos.size(), 1), 0.0);
        for (size_t q = 0; q < upos.size(); ++q) ug0[q] = dsc->G0[upos[q]];
        CREATE_TRY(upload(ctx, &ctx->dug0, ug0));
    }
    std::vector<int> xo(ctx->x_offs.begin(), ctx->x_offs.end());
    CREATE_TRY(upload(ctx, &ctx->dxoffs, xo));
    if (ctx->sp_plan) {
        const pcl_codegen::SpPlan &sp = *ctx->sp_plan;
        std::vector<double> glv(sp.mags);  // the distinct magnitudes of the drives' entries
        glv.resize(std::max<size_t>(glv.size(), 1) + 16, 0.0);
        CREATE_TRY(upload(ctx, &ctx->dsp_pos, sp.pos));
        CREATE_TRY(upload(ctx, &ctx->dsp_coef, sp.coef));
        CREATE_TRY(upload(ctx, &ctx->dsp_glv, glv));
        CREATE_TRY(upload(ctx, &ctx->dsp_pos_n, sp.pos_n));
        CREATE_TRY(upload(ctx, &ctx->dsp_coef_n, sp.coef_n));
    }
    if (ctx->v4_plan) {
        const pcl_codegen::V4Plan &v4 = *ctx->v4_plan;
        const int nb = dsc->per_member_G0 ? dsc->batch : 1;
        std::vector<double> tab((size_t)nb * v4.n_drift_pad, 0.0);
        for (int bb = 0; bb < nb; ++bb)
            for (size_t q = 0; q < v4.drift_pos.size(); ++q) tab[(size_t)bb * v4.n_drift_pad + q] = dsc->G0[(size_t)bb * nn + v4.drift_pos[q]];
        std::vector<double> mg(v4.mags);
        mg.resize(std::max<size_t>(mg.size(), 1) + 16, 0.0);
        std::vector<double> tab_t((size_t)nb * v4.n_drift_pad, 0.0);  // the order G(u)^T x reads the streamed drift entries in
        for (int bb = 0; bb < nb; ++bb)
            for (size_t q = 0; q < v4.drift_pos_t.size(); ++q) tab_t[(size_t)bb * v4.n_drift_pad + q] = dsc->G0[(size_t)bb * nn + v4.drift_pos_t[q]];
        CREATE_TRY(upload(ctx, &ctx->dv4_tab, tab));
        CREATE_TRY(upload(ctx, &ctx->dv4_tab_t, tab_t));
        CREATE_TRY(upload(ctx, &ctx->dv4_mags, mg));
        CREATE_TRY(upload(ctx, &ctx->dv4_dcf, v4.dcf_vals));
        const size_t tick_bytes = (4 + (size_t)dsc->batch * (dsc->N - 1)) * sizeof(unsigned int);
        CREATE_HIP(hipMalloc((void **)&ctx->dv4_tick, tick_bytes));
        CREATE_HIP(hipMemset(ctx->dv4_tick, 0, tick_bytes));
    }
    // device error word, host-mapped: a kernel whose bounded wait gave up sets it; every evaluator entry point and pcl_sync look at it
    CREATE_HIP(hipHostMalloc((void **)&ctx->herr, 64, hipHostMallocMapped));
    *ctx->herr = 0;
    CREATE_HIP(hipHostGetDevicePointer((void **)&ctx->derr, ctx->herr, 0));
#undef CREATE_TRY
#undef CREATE_HIP
    *out = ctx;
    return PCL_OK;
}

extern "C" int pcl_comm_destroy(pcl_ctx *ctx);
extern "C" void pcl_destroy(pcl_ctx *ctx) {
    if (!ctx) return;
    DeviceGuard dev_guard_(ctx->device);
#ifdef PCL_LAB
    if (ctx->res.active) (void)pcl_resident_stop(ctx);  // before any buffer it reads on each request is freed
#endif
    (void)pcl_comm_destroy(ctx);
    void *ptrs[] = {ctx->dhcr, ctx->dhcf, ctx->dhcx, ctx->dhcc, ctx->dh4x, ctx->dh4c, ctx->dGjd, ctx->dG0, ctx->ducoef, ctx->dcsr_val, ctx->dcsc_val, ctx->dupos, ctx->dcsr_ptr, ctx->dcsr_col,
                    ctx->dcsc_ptr, ctx->dcsc_row, ctx->dxoffs, ctx->dZ, ctx->dmu, ctx->ddelta, ctx->dvals, ctx->dhess,
                    ctx->dumap, ctx->dell_col, ctx->dell_val, ctx->duell_l, ctx->duell_v, ctx->ddbg, ctx->dellt_col, ctx->dellt_val,
                    ctx->dhpart, ctx->dhcnt, ctx->dug0, ctx->dexpm, ctx->dxout, ctx->dreduce, ctx->dvar_tab, ctx->dvar_ecol, ctx->dvar_eval, ctx->dexph, ctx->dvexph, ctx->dvexph_part, ctx->dvexph_tiles, ctx->dlhpart, ctx->dlehpart, ctx->dvl_gcol, ctx->dvl_gval, ctx->dvl_gtcol, ctx->dvl_gtval, ctx->dvleh_part, ctx->dvleh_vec};
    for (void *q : ptrs)
        if (q) (void)hipFree(q);
    if (ctx->dgoal) (void)hipFree(ctx->dgoal);
    delete ctx->pool;
    ctx->pool = nullptr;
    for (double *q : {ctx->hZ, ctx->hcompact, ctx->hdelta})
        if (q) (void)hipHostFree(q);
    if (ctx->dcomp_host) (void)hipFree(ctx->dcomp_host);
    for (hipEvent_t e : ctx->ev_chunk)
        if (e) (void)hipEventDestroy(e);
    for (auto &t : ctx->v4_tune)
        for (auto &pr : t.ev)
            for (hipEvent_t e : pr)
                if (e) (void)hipEventDestroy(e);
    for (void *q : {(void *)ctx->dformA, (void *)ctx->dformc, (void *)ctx->dgram, (void *)ctx->dcoef, (void *)ctx->dvar_coef, (void *)ctx->dvar_last_src, (void *)ctx->dvar_diag, (void *)ctx->dvar_scratch})
        if (q) (void)hipFree(q);
    for (void *q : {(void *)ctx->dsub, (void *)ctx->dweights, (void *)ctx->dregs, (void *)ctx->dreg_R, (void *)ctx->dobj, (void *)ctx->dphik, (void *)ctx->dmcols, (void *)ctx->dmticket,
                    (void *)ctx->dgrad, (void *)ctx->dval})
        if (q) (void)hipFree(q);
    for (void *q : {(void *)ctx->dsp_pos, (void *)ctx->dsp_coef, (void *)ctx->dsp_glv, (void *)ctx->dsp_gvals, (void *)ctx->dsp_pos_n, (void *)ctx->dsp_coef_n})
        if (q) (void)hipFree(q);
    delete ctx->sp_plan;
    for (void *q : {(void *)ctx->dv4_tab, (void *)ctx->dv4_tab_t, (void *)ctx->dv4_mags, (void *)ctx->dv4_dcf, (void *)ctx->dv4_tick})
        if (q) (void)hipFree(q);
#ifdef PCL_LAB
    if (ctx->res.stream) (void)hipStreamDestroy(ctx->res.stream);
    if (ctx->res.hbox) (void)hipHostFree(ctx->res.hbox);
    if (ctx->res.hinit) (void)hipHostFree(ctx->res.hinit);
    if (ctx->res.hparams) (void)hipHostFree(ctx->res.hparams);
    if (ctx->res.dparams) (void)hipFree(ctx->res.dparams);
    if (ctx->res.dbox) (void)hipFree(ctx->res.dbox);
#endif
    if (ctx->herr) (void)hipHostFree(ctx->herr);
    delete ctx->v4_plan;
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

extern "C" int pcl_constraint_dim(const pcl_ctx *ctx, int64_t *x_dim, int64_t *rows, int64_t *cols) {
    if (!ctx) return PCL_EINVAL;
    if (x_dim) *x_dim = ctx->x_dim;
    if (rows) *rows = n_rows(ctx);
    if (cols) *cols = z_len(ctx) + ctx->desc.global_dim;
    return PCL_OK;
}
extern "C" int pcl_jac_nnz(const pcl_ctx *ctx, int64_t *nnz, int64_t *per) {
    if (!ctx) return PCL_EINVAL;
    if (per) *per = jac_per_full(ctx);
    if (nnz) *nnz = jac_per_full(ctx) * ctx->win_count * ctx->K;
    return PCL_OK;
}
extern "C" int pcl_set_member_window(pcl_ctx *ctx, int32_t first, int32_t count) {
    if (!ctx) return PCL_EINVAL;
    TRY(require(ctx, FEAT_COLLECTIVE, "pcl_set_member_window"));
    if (first < 0 || count < 1 || (long long)first + count > ctx->desc.batch)
        return fail(ctx, PCL_EINVAL, "pcl_set_member_window: [%d, %d) outside the %d members of this context", first, first + count, ctx->desc.batch);
    ctx->win_first = first;
    ctx->win_count = count;
    return PCL_OK;
}
extern "C" int pcl_jac_compact_nnz(const pcl_ctx *ctx, int64_t *nnz, int64_t *per) {
    if (!ctx) return PCL_EINVAL;
    TRY(require(ctx, FEAT_COMPACT, "pcl_jac_compact_nnz"));
    if (per) *per = jac_per_compact(ctx);
    if (nnz) *nnz = jac_per_compact(ctx) * ctx->win_count * ctx->K;
    return PCL_OK;
}
extern "C" int pcl_hess_nnz(const pcl_ctx *ctx, int64_t *nnz, int64_t *per) {
    if (!ctx) return PCL_EINVAL;
    TRY(require(ctx, FEAT_HESS, "pcl_hess_nnz"));
    if (per) *per = hess_per(ctx);
    if (nnz) *nnz = hess_per(ctx) * ctx->win_count * ctx->K;
    return PCL_OK;
}

template <class I>
static int jac_structure_impl(const pcl_ctx *ctx, I *rows, I *cols) {
    if (!ctx) return PCL_EINVAL;
    if (!rows || !cols) return fail(ctx, PCL_EINVAL, "pcl_jac_structure: NULL output");
    if (ctx->var) return var_jac_structure(ctx, rows, cols);
    const pcl_desc &D = ctx->desc;
    const long long n = ctx->n, d = ctx->cols, m = D.n_drives, xd = ctx->x_dim, zd = D.z_dim, base = D.index_base;
    const long long per = jac_per_full(ctx);
    for (long long b = 0; b < ctx->win_count; ++b) {  // b: member inside the window, bg: member of the context
        const long long bg = ctx->win_first + b;
        const long long xo = ctx->x_offs[D.batch_mode == PCL_BATCH_MEMBERS ? bg : 0];
        const long long voff = D.batch_mode == PCL_BATCH_TRAJ ? bg * zd * D.N : 0;
        for (long long k = 0; k < ctx->K; ++k) {
            I *r = rows + (b * ctx->K + k) * per, *c = cols + (b * ctx->K + k) * per;
            const long long r0 = b * xd * ctx->K + k * xd + base;
            long long p = 0;
            if (ctx->exp) {  // d/dX_{k+1} = I: its diagonal, after the copies of -E
                const long long cb = voff + k * zd + xo + base, cn = voff + (k + 1) * zd + xo + base;
                for (long long cc = 0; cc < d; ++cc)
                    for (long long j = 0; j < n; ++j)
                        for (long long i = 0; i < n; ++i, ++p) {
                            r[p] = (I)(r0 + cc * n + i);
                            c[p] = (I)(cb + cc * n + j);
                        }
                for (long long q = 0; q < xd; ++q, ++p) {
                    r[p] = (I)(r0 + q);
                    c[p] = (I)(cn + q);
                }
            }
            for (int seg = 0; seg < 2 && !ctx->exp; ++seg) {
                const long long cb = voff + (k + seg) * zd + xo + base;
                for (long long cc = 0; cc < d; ++cc)
                    for (long long j = 0; j < n; ++j)
                        for (long long i = 0; i < n; ++i, ++p) {
                            r[p] = (I)(r0 + cc * n + i);
                            c[p] = (I)(cb + cc * n + j);
                        }
            }
            for (long long cc = 0; cc < d; ++cc)  // tail: per state column, the m drive blocks then the dt block
                for (long long l = 0; l <= m; ++l) {
                    const long long col = voff + k * zd + (l < m ? D.u_off + l : D.dt_off) + base;
                    for (long long i = 0; i < n; ++i, ++p) {
                        r[p] = (I)(r0 + cc * n + i);
                        c[p] = (I)col;
                    }
                }
        }
    }
    return PCL_OK;
}
extern "C" int pcl_jac_structure(const pcl_ctx *ctx, int32_t *rows, int32_t *cols) {
    if (ctx && (n_rows(ctx) + 1 > INT32_MAX || z_len(ctx) + ctx->desc.global_dim + 1 > INT32_MAX))
        return fail(ctx, PCL_ESHAPE, "pcl_jac_structure: indices exceed int32; use pcl_jac_structure_i64");
    return jac_structure_impl<int32_t>(ctx, rows, cols);
}
extern "C" int pcl_jac_structure_i64(const pcl_ctx *ctx, int64_t *rows, int64_t *cols) {
    return jac_structure_impl<int64_t>(ctx, rows, cols);
}

template <class I>
static int hess_structure_impl(const pcl_ctx *ctx, I *rows, I *cols) {
    if (!ctx) return PCL_EINVAL;
    if (!rows || !cols) return fail(ctx, PCL_EINVAL, "pcl_hess_structure: NULL output");
    TRY(require(ctx, FEAT_HESS, "pcl_hess_structure"));
    if (ctx->var) return var_hess_structure(ctx, rows, cols);
    const pcl_desc &D = ctx->desc;
    const long long m = D.n_drives, xd = ctx->x_dim, zd = D.z_dim, base = D.index_base;
    const long long per = hess_per(ctx);
    for (long long b = 0; b < ctx->win_count; ++b) {
        const long long bg = ctx->win_first + b;
        const long long xo = ctx->x_offs[D.batch_mode == PCL_BATCH_MEMBERS ? bg : 0];
        const long long voff = D.batch_mode == PCL_BATCH_TRAJ ? bg * zd * D.N : 0;
        for (long long k = 0; k < ctx->K; ++k) {
            I *r = rows + (b * ctx->K + k) * per, *c = cols + (b * ctx->K + k) * per;
            const long long uk = voff + k * zd + D.u_off, hk = voff + k * zd + D.dt_off;
            const long long xk = voff + k * zd + xo, xn = voff + (k + 1) * zd + xo;
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
                for (long long q = 0; q < xd; ++q) put(uk + l, xk + q);
            for (long long q = 0; q < xd; ++q) put(hk, xk + q);
            if (ctx->exp) continue;  // (delta_k is X_{k+1} minus something: no second derivative involves X_{k+1})
            for (long long l = 0; l < m; ++l)
                for (long long q = 0; q < xd; ++q) put(xn + q, uk + l);
            for (long long q = 0; q < xd; ++q) put(xn + q, hk);
        }
    }
    return PCL_OK;
}
extern "C" int pcl_hess_structure(const pcl_ctx *ctx, int32_t *rows, int32_t *cols) {
    if (ctx && z_len(ctx) + ctx->desc.global_dim + 1 > INT32_MAX)
        return fail(ctx, PCL_ESHAPE, "pcl_hess_structure: indices exceed int32; use pcl_hess_structure_i64");
    return hess_structure_impl<int32_t>(ctx, rows, cols);
}
extern "C" int pcl_hess_structure_i64(const pcl_ctx *ctx, int64_t *rows, int64_t *cols) {
    return hess_structure_impl<int64_t>(ctx, rows, cols);
}

#include "pcl_host_launch_pade.hpp"
#include "pcl_host_launch_hess.hpp"

// --- order policy ---------------------------------------------------------------------------------
// The reference's constraint is x_{k+1} = exp(dt_k G(u_k)) x_k (docs/src/concepts/index.md:21); the diagonal Pade residual of order 2q
// deviates from it by  kappa_q theta^(2q+1) (1 + O(theta^2)) |x|,  theta = |dt_k G(u_k)|_2,  kappa_q = (q!)^2 / ((2q)! (2q+1)!)  -- the
// leading term of exp - r_qq.  (Measured on exp-feasible trajectories, scripts/pade_vs_exp.py -> profiles/pade_vs_exp.json: config 3, theta = 0.438:
// 1.6e-5 / 1.6e-11 / 7.9e-15 at orders 4 / 8 / 10 against 2.2e-5 / 2.3e-11 / 1.1e-14 from this bound.)  pade_order = 0 asks for the
// smallest order whose bound is below a tolerance, theta from the problem's bounds (pcl_set_order_policy) or, failing that, from the
// first trajectory a host-pointer entry point sees (with a margin of 1.5 on theta: later iterates move inside their bounds).
static double spectral_norm(const double *A, int n) {
    // Power iteration on A^T A (n <= 64: microseconds) from two generic, non-symmetric start vectors -- a symmetric one (all ones) is
    // annihilated by generators whose rows sum to zero and can sit orthogonal to the top singular vector -- the larger result counts; the
    // guaranteed bound sqrt(|A|_1 |A|_inf) >= |A|_2 stands in when the iteration has nothing to say and caps a result that exceeds it.
    double n1 = 0.0, ninf = 0.0;
    {
        std::vector<double> rs(n, 0.0);
        for (int j = 0; j < n; ++j) {
            double cs = 0.0;
            for (int i = 0; i < n; ++i) cs += std::fabs(A[i + (size_t)n * j]), rs[i] += std::fabs(A[i + (size_t)n * j]);
            n1 = std::max(n1, cs);
        }
        for (int i = 0; i < n; ++i) ninf = std::max(ninf, rs[i]);
    }
    const double upper = std::sqrt(n1 * ninf);
    if (upper == 0.0) return 0.0;
    std::vector<double> x(n), y(n), z(n);
    double best = 0.0;
    for (int seed = 0; seed < 2; ++seed) {
        for (int j = 0; j < n; ++j) x[j] = 1.0 + 0.61803398875 * std::sin(1.0 + (seed ? 2.39996323 : 1.0) * (j + 1)) + (seed ? 0.25 * ((j * 7 + 3) % 5) : 0.0);
        double s = 0.0;
        bool converged = false;
        for (int it = 0; it < 200 && !converged; ++it) {
            for (int i = 0; i < n; ++i) {
                double a = 0.0;
                for (int j = 0; j < n; ++j) a += A[i + (size_t)n * j] * x[j];
                y[i] = a;
            }
            for (int j = 0; j < n; ++j) {
                double a = 0.0;
                for (int i = 0; i < n; ++i) a += A[i + (size_t)n * j] * y[i];
                z[j] = a;
            }
            double nz = 0.0, nx = 0.0;
            for (int j = 0; j < n; ++j) nz += z[j] * z[j], nx += x[j] * x[j];
            if (nz == 0.0) {
                s = 0.0;
                break;
            }
            const double s1 = std::sqrt(std::sqrt(nz) / std::sqrt(nx));
            nz = std::sqrt(nz);
            for (int j = 0; j < n; ++j) x[j] = z[j] / nz;
            converged = it >= 8 && std::fabs(s1 - s) <= 1e-12 * s1;  // (a plateau in the first steps may be a sub-dominant singular value)
            s = s1;
        }
        best = std::max(best, converged ? s : s * 1.01);  // (not converged to round-off: a hair on the safe side)
    }
    if (best == 0.0) return upper;
    return std::min(best, upper);
}
// the smallest diagonal Pade order whose bound is below tol; *met (when given) says whether any order up to 10 is
static int order_for(double theta, double tol, bool *met = nullptr) {
    double fact[12];
    fact[0] = 1.0;
    for (int i = 1; i < 12; ++i) fact[i] = fact[i - 1] * i;
    if (met) *met = true;
    for (int q = 1; q <= 5; ++q) {
        const double kappa = fact[q] * fact[q] / (fact[2 * q] * fact[2 * q + 1]);
        if (kappa * std::pow(theta, 2 * q + 1) <= tol) return 2 * q;
    }
    if (met) *met = false;
    return 10;
}
// (order 10 chosen although its bound exceeds the tolerance: said in pcl_last_error's text -- no error code -- and readable as option order_tol_met)
static void note_order(pcl_ctx *ctx, double theta, bool met) {
    ctx->order_tol_met = met ? 1 : 0;
    if (!met) {
        char buf[320];
        snprintf(buf, sizeof buf, "order policy: |dt G| <= %.3g is too large for any diagonal Pade order up to 10 to stay within %.3g of the exp constraint; order 10 is used (option order_tol_met = 0), or create the context with PCL_ORDER_EXP", theta, ctx->order_tol);
        ctx->err = buf;
        if (getenv("PCL_VERBOSE")) fprintf(stderr, "piccolo_hip: %s\n", buf);
    }
}
static void set_order(pcl_ctx *ctx, int order, double theta) {
    if (ctx->desc.pade_order != order) {  // (modules are per order: the handles of the previous one are dropped, the modules stay cached)
        ctx->v4_f = ctx->v4_ft = ctx->v4_f1 = ctx->v4_feval = ctx->v4_fevalc = ctx->v4_fhess = ctx->v4_fhess2 = ctx->v4_fhessc = ctx->v4_fhessp = nullptr;
        ctx->v4_failed = ctx->v4_hess_failed = ctx->v4_hessc_failed = ctx->v4_ft_failed = ctx->v4_f1_failed = 0;
#ifdef PCL_LAB
        ctx->res.f = nullptr;  // (the resident module bakes the order in as well)
#endif
    }
    ctx->desc.pade_order = order;
    ctx->order_theta = theta;
}
// theta = dt_max max_{|u_l| <= u_max_l} |G_drift + sum_l u_l G_l|_2 over n_g0 drifts (n x n, column-major; any real generators).  The norm is convex
// in u, so the maximum over the box sits at a vertex: all 2^m sign patterns are tried (m <= 10; 64 norms of a 54 x 54 matrix at config 3: tens of
// ms, once per context).  The triangle inequality |G_drift| + sum_l u_max_l |G_l| -- what rounds 3-4 used, and the fallback for m > 10 -- overshoots
// by half where the drives act on different subsystems (config 3: 10.5 against 6.86) and would ask for an order that no trajectory in the box needs.
// Further drifts (ensemble members): |G_drift_b + D| <= max_vertex |G_drift_0 + D| + |G_drift_b - G_drift_0|.
static double policy_theta(int n, int m, const double *G0, size_t n_g0, const double *Gj, double dt_max, const double *u_max) {
    const size_t nn = (size_t)n * n;
    double gd = 0.0;
    for (int l = 0; l < m; ++l) gd += std::fabs(u_max[l]) * spectral_norm(Gj + (size_t)l * nn, n);
    const double tri0 = spectral_norm(G0, n) + gd;
    double vmax = tri0;
    if (m <= 10) {
        std::vector<double> G(nn);
        vmax = 0.0;
        for (unsigned sgn = 0; sgn < (1u << m); ++sgn) {
            for (size_t e = 0; e < nn; ++e) {
                double a = G0[e];
                for (int l = 0; l < m; ++l) a += ((sgn >> l) & 1u ? -1.0 : 1.0) * std::fabs(u_max[l]) * Gj[(size_t)l * nn + e];
                G[e] = a;
            }
            vmax = std::max(vmax, spectral_norm(G.data(), n));
        }
        vmax = std::min(vmax, tri0);
    }
    double theta = dt_max * vmax;
    std::vector<double> Dm(nn);
    for (size_t b = 1; b < n_g0; ++b) {
        for (size_t e = 0; e < nn; ++e) Dm[e] = G0[b * nn + e] - G0[e];
        theta = std::max(theta, dt_max * (vmax + spectral_norm(Dm.data(), n)));
    }
    return theta;
}
// The policy without a context or a device (what pcl_set_order_policy applies; the CPU tests pin it): n = generator dimension (2 d for unitary / ket
// problems), n_g0 drifts.  order_out: the smallest diagonal Pade order whose bound kappa_q theta^(2q+1) is <= tol (10 when none is: *met_out = 0).
extern "C" int pcl_order_for_bounds(int32_t n, int32_t m, const double *G0, int32_t n_g0, const double *Gj, double dt_max, const double *u_max, double tol,
                                    double *theta_out, int32_t *order_out, int32_t *met_out) {
    if (n < 1 || n > 4096 || m < 0 || n_g0 < 1 || !G0 || (m > 0 && (!Gj || !u_max)) || !(dt_max > 0.0) || !(tol > 0.0)) return PCL_EINVAL;
    const double theta = policy_theta(n, m, G0, (size_t)n_g0, Gj, dt_max, u_max);
    bool met = true;
    const int order = order_for(theta, tol, &met);
    if (theta_out) *theta_out = theta;
    if (order_out) *order_out = order;
    if (met_out) *met_out = met ? 1 : 0;
    return PCL_OK;
}
extern "C" int pcl_set_order_policy(pcl_ctx *ctx, double dt_max, const double *u_max, double tol, int32_t *order_out) {
    if (!ctx) return PCL_EINVAL;
    if (ctx->exp || ctx->vexp) return fail(ctx, PCL_EINVAL, "pcl_set_order_policy: the context evaluates the exponential constraint; there is no order to choose");
    if (!(dt_max > 0.0) || !(tol > 0.0) || (ctx->desc.n_drives > 0 && !u_max)) return fail(ctx, PCL_EINVAL, "pcl_set_order_policy: need dt_max > 0, tol > 0 and the drives' bounds");
#ifdef PCL_LAB
    if (ctx->res.active) return fail(ctx, PCL_EINVAL, "pcl_set_order_policy: a resident evaluator is running (pcl_resident_stop first)");
#endif
    const int n = ctx->var ? ctx->var_nl : ctx->n, m = ctx->desc.n_drives;
    const double theta = policy_theta(n, m, ctx->hG0.data(), ctx->hG0.size() / ((size_t)n * n), ctx->hGj.data(), dt_max, u_max);
    ctx->order_tol = tol;
    bool met = true;
    set_order(ctx, order_for(theta, tol, &met), theta);
    note_order(ctx, theta, met);
    if (order_out) *order_out = ctx->desc.pade_order;
    return PCL_OK;
}
// pade_order = 0 and no policy yet: the first trajectory on the host decides (host-pointer entry points); device-pointer entry points
// have nothing to look at
static int resolve_order(pcl_ctx *ctx, const double *Z_host, const char *where) {
    if (ctx->desc.pade_order != 0) return PCL_OK;
    if (!Z_host) return fail(ctx, PCL_EINVAL, "%s: the context was created with pade_order = 0; call pcl_set_order_policy (or a host-pointer entry point) first", where);
    const pcl_desc &D = ctx->desc;
    const int n = ctx->var ? ctx->var_nl : ctx->n, m = D.n_drives;  // (variational: the lifted generator)
    const int nbuf = D.batch_mode == PCL_BATCH_TRAJ ? D.batch : 1;
    std::vector<double> G((size_t)n * n);
    double theta = 0.0;
    for (size_t g0 = 0; g0 * n * n < ctx->hG0.size(); ++g0)
        for (int b = 0; b < nbuf; ++b) {
            // (a multistart constructed from ONE trajectory tiled `batch` times: one pass of norms, not `batch`)
            if (b > 0 && !memcmp(Z_host + (size_t)b * D.N * D.z_dim, Z_host, (size_t)D.N * D.z_dim * sizeof(double))) continue;
            for (int k = 0; k + 1 < D.N; ++k) {
                const double *z = Z_host + ((size_t)b * D.N + k) * D.z_dim;
                for (size_t e = 0; e < (size_t)n * n; ++e) {
                    double a = ctx->hG0[g0 * n * n + e];
                    for (int l = 0; l < m; ++l) a += z[D.u_off + l] * ctx->hGj[(size_t)l * n * n + e];
                    G[e] = a;
                }
                theta = std::max(theta, std::fabs(z[D.dt_off]) * spectral_norm(G.data(), n));
            }
        }
    bool met = true;
    set_order(ctx, order_for(1.5 * theta, ctx->order_tol, &met), 1.5 * theta);
    note_order(ctx, 1.5 * theta, met);
    return PCL_OK;
}

extern "C" int pcl_set_order_from_trajectory(pcl_ctx *ctx, const double *Z_host, double tol, int32_t *order_out) {
    if (!ctx) return PCL_EINVAL;
    if (ctx->exp || ctx->vexp) return fail(ctx, PCL_EINVAL, "pcl_set_order_from_trajectory: the context evaluates the exponential constraint; there is no order to choose");
    if (!Z_host) return fail(ctx, PCL_EINVAL, "pcl_set_order_from_trajectory: NULL trajectory");
#ifdef PCL_LAB
    if (ctx->res.active) return fail(ctx, PCL_EINVAL, "pcl_set_order_from_trajectory: a resident evaluator is running (pcl_resident_stop first)");
#endif
    if (tol > 0.0) ctx->order_tol = tol;
    const int keep = ctx->desc.pade_order;
    ctx->desc.pade_order = 0;  // (resolve_order decides for contexts without an order; set_order drops the previous order's module handles)
    const int rc = resolve_order(ctx, Z_host, "pcl_set_order_from_trajectory");
    if (rc != PCL_OK) {
        ctx->desc.pade_order = keep;
        return rc;
    }
    if (order_out) *order_out = ctx->desc.pade_order;
    return PCL_OK;
}

// --- device-pointer API -----------------------------------------------------------------------
// A launch with slice tickets leaves its counters zero only when it has finished, and so do the Hessian kernels that exchange rows of sums through
// per-context arrival counters (column groups, two workgroups per interval): a launch on ANOTHER stream must not start before that (launches on
// one stream are ordered anyway; the counters' first-use memset is ordered on the stream of that moment too).  Switching streams therefore waits
// for the old one if such a launch may be in flight.
static int change_stream(pcl_ctx *ctx, hipStream_t s) {
    if (s != ctx->stream && ctx->ticket_launched) {
        ON_DEVICE(ctx);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->ticket_launched = false;
    }
    ctx->stream = s;
    ctx->tickets_dirty = true;
    return PCL_OK;
}
extern "C" int pcl_set_stream(pcl_ctx *ctx, void *s) {
    if (!ctx) return PCL_EINVAL;
    return change_stream(ctx, (hipStream_t)s);  // NULL is HIP's legacy default stream
}
extern "C" int pcl_reset_stream(pcl_ctx *ctx) {
    if (!ctx) return PCL_EINVAL;
    return change_stream(ctx, ctx->own_stream);
}
extern "C" int pcl_sync(pcl_ctx *ctx) {
    if (!ctx) return PCL_EINVAL;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_device_error(ctx, "pcl_sync");
}
extern "C" int pcl_eval_dev(pcl_ctx *ctx, const double *Z, double *delta) {
    if (!ctx) return PCL_EINVAL;
    if (!Z || !delta) return fail(ctx, PCL_EINVAL, "pcl_eval_dev: NULL pointer");
    return launch_fused(ctx, Z, delta, nullptr, false);
}
extern "C" int pcl_eval_jac_dev(pcl_ctx *ctx, const double *Z, double *delta, double *vals) {
    if (!ctx) return PCL_EINVAL;
    if (!Z || !vals) return fail(ctx, PCL_EINVAL, "pcl_eval_jac_dev: NULL pointer");
    return launch_fused(ctx, Z, delta, vals, false);
}

#ifdef PCL_LAB
#include "pcl_host_resident.hpp"  // pcl_resident_* (include/piccolo_hip_lab.h): measured, loses, kept for the record
#endif

extern "C" int pcl_jac_dev(pcl_ctx *ctx, const double *Z, double *vals) {  // eval_jacobian alone: no residual is written
    if (!ctx) return PCL_EINVAL;
    if (!Z || !vals) return fail(ctx, PCL_EINVAL, "pcl_jac_dev: NULL pointer");
    return launch_fused(ctx, Z, nullptr, vals, false);
}
extern "C" int pcl_eval_jac_compact_dev(pcl_ctx *ctx, const double *Z, double *delta, double *compact) {
    if (!ctx) return PCL_EINVAL;
    if (!Z || !compact) return fail(ctx, PCL_EINVAL, "pcl_eval_jac_compact_dev: NULL pointer");
    if (!ctx->var || ctx->large_var) TRY(require(ctx, FEAT_COMPACT, "pcl_eval_jac_compact_dev"));  // (a variational context of n <= 64: launch_fused refuses, as "the compact Jacobian")
    return launch_fused(ctx, Z, delta, compact, true);
}
extern "C" int pcl_jac_expand_dev(pcl_ctx *ctx, const double *compact, double *vals) {
    if (!ctx) return PCL_EINVAL;
    if (!compact || !vals) return fail(ctx, PCL_EINVAL, "pcl_jac_expand_dev: NULL pointer");
    TRY(require(ctx, FEAT_COMPACT, "pcl_jac_expand_dev"));
    ON_DEVICE(ctx);
    const long long n_bk = (long long)ctx->win_count * ctx->K;
    if (ctx->var) {  // every distinct tile to its cols copies in every segment it occurs in; at one column too (the tiles of component 0 repeat per variation)
        const int cpi = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->opt_cols_per_slice > 0 ? ctx->opt_cols_per_slice : 3, ctx->cols));
        const long long tail = (long long)ctx->x_dim * (ctx->desc.n_drives + 1), ntile = ctx->vexp ? 1 + ctx->var : 2 + 2 * ctx->var;
        const long long grid = n_bk * (ntile * ((ctx->cols + cpi - 1) / cpi) + (tail + 4095) / 4096);
        if (grid > 0x7fffffffLL) return fail(ctx, PCL_ESHAPE, "pcl_jac_expand_dev: %lld work items exceed the grid limit", grid);
        hipLaunchKernelGGL(pcl_var_expand_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, compact, vals, ctx->cols, ctx->n, ctx->desc.n_drives, ctx->var,
                           ctx->vexp, n_bk, cpi);
        HIP_TRY(ctx, hipGetLastError());
        return PCL_OK;
    }
    if (ctx->exp) {  // [-E | tail] -> [-E x cols | ones | tail], at every column count (one column: the ones are not part of the compact block)
        const int cpi = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->opt_cols_per_slice > 0 ? ctx->opt_cols_per_slice : 3, ctx->cols));
        const long long tail = (long long)ctx->x_dim * (ctx->desc.n_drives + 1);
        if (ctx->large_exp) {  // tiles of up to 8192 element pairs (option large_exp_reduce): workgroups of 2048 pairs each per slice -- pcl_exp_expand_large_kernel
            const long long grid_l = n_bk * ((long long)pcl_expand_large_parts(ctx->n) * ((ctx->cols + cpi - 1) / cpi) + (tail + 4095) / 4096);
            if (grid_l > 0x7fffffffLL) return fail(ctx, PCL_ESHAPE, "pcl_jac_expand_dev: %lld work items exceed the grid limit", grid_l);
            hipLaunchKernelGGL(pcl_exp_expand_large_kernel, dim3((unsigned)grid_l), dim3(256), 0, ctx->stream, compact, vals, ctx->cols, ctx->n, ctx->desc.n_drives, n_bk, cpi,
                               (int)(ctx->opt_nt > 0 ? ctx->opt_nt : 0));
            HIP_TRY(ctx, hipGetLastError());
            return PCL_OK;
        }
        const long long grid = n_bk * ((ctx->cols + cpi - 1) / cpi + (tail + 4095) / 4096);
        if (grid > 0x7fffffffLL) return fail(ctx, PCL_ESHAPE, "pcl_jac_expand_dev: %lld work items exceed the grid limit", grid);
        hipLaunchKernelGGL(pcl_exp_expand_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, compact, vals, ctx->cols, ctx->n, ctx->desc.n_drives, n_bk, cpi);
        HIP_TRY(ctx, hipGetLastError());
        return PCL_OK;
    }
    if (ctx->cols == 1) {  // one state column (kets, compact density vectors): the compact layout IS the full layout
        HIP_TRY(ctx, hipMemcpyAsync(vals, compact, (size_t)(n_bk * jac_per_full(ctx)) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        return PCL_OK;
    }
    // slices of 3 state columns (70 KB per workgroup at config 3), the option cols_per_slice overrides
    const int cpi = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->opt_cols_per_slice > 0 ? ctx->opt_cols_per_slice : 3, ctx->cols));
    const long long tail2 = ((long long)ctx->x_dim * (ctx->desc.n_drives + 1)) >> 1;
    if (ctx->large) {  // tiles of up to 8192 element pairs (option large_reduce): workgroups of 2048 pairs each per (sign, slice) -- pcl_expand_large_kernel
        const long long per_bk_l = 2LL * pcl_expand_large_parts(ctx->n) * ((ctx->cols + cpi - 1) / cpi) + (tail2 + 2047) / 2048;
        const long long grid_l = n_bk * per_bk_l;
        if (grid_l > 0x7fffffffLL) return fail(ctx, PCL_ESHAPE, "pcl_jac_expand_dev: %lld work items exceed the grid limit", grid_l);
        hipLaunchKernelGGL(pcl_expand_large_kernel, dim3((unsigned)grid_l), dim3(256), 0, ctx->stream, compact, vals, ctx->cols, ctx->n, ctx->desc.n_drives, n_bk, cpi,
                           (int)(ctx->opt_nt > 0 ? ctx->opt_nt : 0));
        HIP_TRY(ctx, hipGetLastError());
        return PCL_OK;
    }
    const long long per_bk = 2LL * ((ctx->cols + cpi - 1) / cpi) + (tail2 + 2047) / 2048;
    const long long grid = n_bk * per_bk;
    if (grid > 0x7fffffffLL) return fail(ctx, PCL_ESHAPE, "pcl_jac_expand_dev: %lld work items exceed the grid limit", grid);
    if ((ctx->n & 1) || ((long long)ctx->x_dim * (ctx->desc.n_drives + 1)) % 2) return fail(ctx, PCL_ESHAPE, "pcl_jac_expand_dev: odd block sizes");
    hipLaunchKernelGGL(pcl_expand_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, compact, vals, ctx->cols, ctx->n,
                       ctx->desc.n_drives, n_bk, cpi, (int)(ctx->opt_nt > 0 ? ctx->opt_nt : 0));
    HIP_TRY(ctx, hipGetLastError());
    return PCL_OK;
}
extern "C" int pcl_hess_dev(pcl_ctx *ctx, const double *Z, const double *mu, double *vals) {
    if (!ctx) return PCL_EINVAL;
    if (!Z || !mu || !vals) return fail(ctx, PCL_EINVAL, "pcl_hess_dev: NULL pointer");
    if (ctx->large || ctx->large_var) TRY(require(ctx, FEAT_HESS, "pcl_hess_dev"));  // (every other kind: launch_hess refuses, as "pcl_hess")
    return launch_hess(ctx, Z, mu, vals);
}

// Rollout of a large context (pcl_kernel_large_rollout.hpp; option large_full).  Beside the tile (LD = n | 1) the propagator launch holds three
// blocks of npc columns of E (Y, V, the product); the chain launch holds two blocks of nc state columns and no tile (its operand E_k goes from the
// workspace into registers).  The widest panel that fits is evened over the panels; launches of few intervals take up to one panel per 16
// columns while the grid stays within one round of the CUs (option general_slices: that many panels at least).  The chain takes slices of at most 16 state columns, one matrix-core column tile (option
// cols_per_slice: that many at most), evened.  One column always fits (n = 128, m = 24: 136,472 B and 3,088 B).  Every split gives the same bits.
struct LargeRollPlan : LargeTile {
    int P, npc, S, nc;
    size_t lds_e, lds_c;
};
static void large_roll_plan(const pcl_ctx *ctx, int n, int cols, int m, long long items, LargeRollPlan &R) {
    static_cast<LargeTile &>(R) = large_tile(ctx->max_lds, n, m);  // (the propagator launch's; the chain launch has the slack alone.  NB >= 0: the tile fits for n <= 128)
    const long long budget = ctx->max_lds / (long long)sizeof(double), fixed_c = PL_SLACK;
    const int npc_max = std::max(1, std::min(n, R.NB / 3));
    const int p_min = (n + npc_max - 1) / npc_max;
    const long long want = ctx->opt_general_slices > 0 ? ctx->opt_general_slices : std::min<long long>((n + 15) / 16, ctx->n_cu / std::max(items, 1LL));
    R.P = (int)std::max<long long>(p_min, std::min<long long>(want, n));
    R.npc = (n + R.P - 1) / R.P;
    R.P = (n + R.npc - 1) / R.npc;  // (no panel without a column)
    const int nc_fit = (int)std::max<long long>(1, (budget - fixed_c) / R.LD / 2);
    const int nc_cap = ctx->opt_cols_per_slice > 0 ? (int)std::min<int64_t>(ctx->opt_cols_per_slice, cols) : std::min(cols, 16);
    R.nc = std::min(nc_cap, nc_fit);
    R.S = even_split(cols, R.nc);  // even slices
    R.lds_e = (size_t)(R.fixed + 3LL * R.LD * R.npc) * sizeof(double);
    R.lds_c = (size_t)(fixed_c + 2LL * R.LD * R.nc) * sizeof(double);
}
static int launch_large_rollout(pcl_ctx *ctx, const double *Z, double *X_out) {
    ON_DEVICE(ctx);
    KParams p;
    fill_params(ctx, p);
    p.Z = window_Z(ctx, Z);
    p.xout = X_out;
    if (!ctx->dexpm) {  // the propagators of every member: batch x (N - 1) x n^2 doubles, kept until pcl_destroy
        const hipError_t e = hipMalloc((void **)&ctx->dexpm, (size_t)ctx->desc.batch * p.K * p.n * p.n * sizeof(double));
        if (e != hipSuccess) {
            ctx->dexpm = nullptr;
            (void)hipGetLastError();
            return fail(ctx, e == hipErrorOutOfMemory ? PCL_ENOMEM : PCL_EHIP, "pcl_rollout_dev: the propagator workspace of %zu B: %s",
                        (size_t)ctx->desc.batch * p.K * p.n * p.n * sizeof(double), hipGetErrorString(e));
        }
    }
    p.expm = ctx->dexpm;
    LargeRollPlan R;
    const long long items = (long long)p.batch * p.K;
    large_roll_plan(ctx, p.n, p.cols, p.m, items, R);
    if (R.lds_e > (size_t)ctx->max_lds || R.lds_c > (size_t)ctx->max_lds)
        return fail(ctx, PCL_ESHAPE, "pcl_rollout_dev: the large-generator rollout needs %zu B of LDS (> %d) for n = %d, m = %d", std::max(R.lds_e, R.lds_c), ctx->max_lds, p.n, p.m);
    if (int rc = check_grid(ctx, std::max(items * R.P, (long long)p.batch * R.S))) return rc;
    p.LD = R.LD;
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)pcl_large_expm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.lds_e));
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)pcl_large_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.lds_c));
    p.nc = R.npc;
    p.S = R.P;
    p.lds_doubles = (int)(R.lds_e / sizeof(double));
    if (ctx->opt_large_rollout_stage != 2) {
        hipLaunchKernelGGL(pcl_large_expm_kernel, dim3((unsigned)(items * R.P)), dim3((unsigned)R.threads), R.lds_e, ctx->stream, p);
        HIP_TRY(ctx, hipGetLastError());
    }
    ctx->last_kernel = 270;  // the large family's rollout (280 + q: its residual, 290 + q: residual + Jacobian)
    ctx->last_n_stream = 0;
    if (ctx->opt_large_rollout_stage == 1) return PCL_OK;
    p.nc = R.nc;
    p.S = R.S;
    p.lds_doubles = (int)(R.lds_c / sizeof(double));
    hipLaunchKernelGGL(pcl_large_chain_kernel, dim3((unsigned)((long long)p.batch * R.S)), dim3((unsigned)R.threads), R.lds_c, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    return PCL_OK;
}

extern "C" int pcl_rollout_dev(pcl_ctx *ctx, const double *Z, double *X_out) {
    if (!ctx) return PCL_EINVAL;
    if (!Z || !X_out) return fail(ctx, PCL_EINVAL, "pcl_rollout_dev: NULL pointer");
    TRY(require(ctx, FEAT_OBJECTIVE, "pcl_rollout_dev"));
    if (ctx->large_var) return var_large_rollout_dev(ctx, Z, X_out);
    if (ctx->var) return var_rollout_dev(ctx, Z, X_out);
    if (ctx->large) return launch_large_rollout(ctx, Z, X_out);
    ON_DEVICE(ctx);
    KParams p;
    fill_params(ctx, p);
    p.Z = window_Z(ctx, Z);
    p.xout = X_out;
    if (!ctx->dexpm) HIP_TRY(ctx, hipMalloc((void **)&ctx->dexpm, (size_t)ctx->desc.batch * p.K * p.n * p.n * sizeof(double)));
    p.expm = ctx->dexpm;
    const size_t lds_a = (3 * (size_t)p.LD * p.n + 8 + p.m + 64) * sizeof(double);
    const size_t lds_b = ((size_t)p.LD * p.n + 2 * (size_t)p.LD * p.cols) * sizeof(double);
    if (lds_a > (size_t)ctx->max_lds || lds_b > (size_t)ctx->max_lds) return fail(ctx, PCL_ESHAPE, "pcl_rollout_dev: tiles exceed LDS");
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)pcl_expm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a));
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)pcl_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    hipLaunchKernelGGL(pcl_expm_kernel, dim3((unsigned)((long long)p.batch * p.K)), dim3(256), lds_a, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(pcl_chain_kernel, dim3((unsigned)p.batch), dim3(256), lds_b, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    return PCL_OK;
}

// --- host-pointer API (staging buffers owned by the context) --------------------------------------
static int ensure(pcl_ctx *ctx, double **buf, long long count) {
    if (*buf) return PCL_OK;
    hipError_t e = hipMalloc((void **)buf, (size_t)count * sizeof(double));
    if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? PCL_ENOMEM : PCL_EHIP, "hipMalloc(%lld doubles): %s", count, hipGetErrorString(e));
    return PCL_OK;
}
static int ensure_pinned(pcl_ctx *ctx, double **buf, long long count) {
    if (*buf) return PCL_OK;
    hipError_t e = hipHostMalloc((void **)buf, (size_t)count * sizeof(double), hipHostMallocDefault);
    if (e != hipSuccess) return fail(ctx, PCL_ENOMEM, "hipHostMalloc(%lld doubles): %s", count, hipGetErrorString(e));
    return PCL_OK;
}
// Thread count of the host expansion.  Default (0): min(cores / 2, 32) -- the path is bound by the host's memory writes into the caller's
// pageable array, 16 ... 64 threads deliver 1.0-1.3 k evaluations per second on the boxes of the pool, which count is best changes from box to
// box and from run to run (page placement of the caller's array, neighbours).  host_threads = -1 asks for a sweep: the context's first 2 x 6
// host-delivered calls are each run at one of six candidate counts -- real calls, real results -- and the count whose fastest call was
// shortest serves the context from then on (measured: 1.6 k on one box, no better than the default on two others; hence opt-in).
static const int kHostTuneCand[] = {16, 24, 32, 48, 64, 96};
static const int kHostTuneN = 6;
static int host_threads(const pcl_ctx *ctx) {
    if (ctx->opt_host_threads > 0) return (int)std::min<int64_t>(ctx->opt_host_threads, 256);
    if (ctx->host_threads_tuned > 0) return ctx->host_threads_tuned;
    const unsigned hw = std::max(2u, std::thread::hardware_concurrency());
    if (ctx->opt_host_threads < 0 && ctx->host_tune_calls < 2 * kHostTuneN) return (int)std::min<unsigned>((unsigned)kHostTuneCand[ctx->host_tune_calls % kHostTuneN], hw);
    // ... and never more than the CPUs the cgroup grants (cpu.max): a container that sees 256 hardware threads and is allowed 16 CPUs delivered
    // 1,390 evaluations/s sustained with 16 threads and 650-1,000 with 32 (1,570 per median call: the team wins single calls and is throttled
    // over a run -- round 5, bench.py other_rates.host_delivered.paths)
    unsigned def = std::max(1u, std::min(hw / 2, 32u));
    static const double quota = pcl_host::cgroup_quota_cpus();
    if (quota >= 1.0) def = std::min(def, (unsigned)quota);
    return (int)std::max(1u, def);
}

// Host-pointer evaluation.  Two ways to deliver the Jacobian values into the caller's (pageable) array:
//   full    the kernel writes the full triplet-order values in HBM and 132.8 MB (config 3) cross PCIe;
//   compact the kernel writes only the unique tiles (12.7 MB), they cross PCIe into pinned staging in chunks of intervals,
//           and the host's threads replicate them into the caller's array with streaming stores while the next chunk is
//           in flight -- bound by host memory write bandwidth instead of by PCIe.  Default whenever blocks are replicated.
static int host_eval_jac(pcl_ctx *ctx, const double *Z, double *delta, double *vals) {
    if (!ctx) return PCL_EINVAL;
    if (!Z || (!delta && !vals)) return fail(ctx, PCL_EINVAL, "NULL pointer");
    ON_DEVICE(ctx);
    TRY(resolve_order(ctx, Z, "pcl_eval_jac"));
    const auto t_begin = std::chrono::steady_clock::now();
    const long long nbk = (long long)ctx->win_count * ctx->K, nbk_all = (long long)(ctx->var ? 1 : ctx->desc.batch) * ctx->K;  // (variational: one stacked trajectory)
    const long long nv = jac_per_full(ctx) * nbk;
    // (a context whose compact Jacobian is behind an option that is off: full values, as under host_path 1)
    const bool compact_path = vals && ctx->cols > 1 && ctx->opt_host_path != 1 && serves(ctx, FEAT_COMPACT);
    TRY(ensure(ctx, &ctx->dZ, z_len(ctx)));
    TRY(ensure(ctx, &ctx->ddelta, n_rows_all(ctx)));
    TRY(ensure_pinned(ctx, &ctx->hZ, z_len(ctx)));
    memcpy(ctx->hZ, Z, (size_t)z_len(ctx) * sizeof(double));  // pinned source: the H2D copy is one asynchronous DMA
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dZ, ctx->hZ, z_len(ctx) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (!compact_path) {
        if (vals) TRY(ensure(ctx, &ctx->dvals, jac_per_full(ctx) * nbk_all));
        TRY(launch_fused(ctx, ctx->dZ, ctx->ddelta, vals ? ctx->dvals : nullptr, false));
        if (delta) HIP_TRY(ctx, hipMemcpyAsync(delta, ctx->ddelta, n_rows(ctx) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (vals) HIP_TRY(ctx, hipMemcpyAsync(vals, ctx->dvals, nv * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return check_device_error(ctx, "pcl_eval_jac");
    }
    const long long cper = jac_per_compact(ctx), fper = jac_per_full(ctx);
    TRY(ensure(ctx, &ctx->dcomp_host, cper * nbk_all));
    TRY(ensure_pinned(ctx, &ctx->hcompact, cper * nbk_all));
    TRY(ensure_pinned(ctx, &ctx->hdelta, n_rows_all(ctx)));
    const int n_chunks = (int)std::max<long long>(1, std::min<long long>(std::min<int64_t>(ctx->opt_host_chunks, 8), nbk));
    for (int c = 0; c < n_chunks; ++c)
        if (!ctx->ev_chunk[c]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_chunk[c], hipEventDisableTiming));
    TRY(launch_fused(ctx, ctx->dZ, ctx->ddelta, ctx->dcomp_host, true));
    for (int c = 0; c < n_chunks; ++c) {
        const long long lo = nbk * c / n_chunks, hi = nbk * (c + 1) / n_chunks;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->hcompact + lo * cper, ctx->dcomp_host + lo * cper, (size_t)((hi - lo) * cper) * sizeof(double),
                                    hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_chunk[c], ctx->stream));
    }
    if (delta) HIP_TRY(ctx, hipMemcpyAsync(ctx->hdelta, ctx->ddelta, n_rows(ctx) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    const bool tuning = ctx->opt_host_threads < 0 && ctx->host_threads_tuned == 0 && ctx->host_tune_calls < 2 * kHostTuneN && nv * 8 >= (32LL << 20);
    const int want_threads = host_threads(ctx);
    if (!ctx->pool || ctx->pool->size() != want_threads - 1) {
        delete ctx->pool;
        ctx->pool = new (std::nothrow) pcl_host::Pool(want_threads - 1);  // the calling thread is the last worker
        if (!ctx->pool) return fail(ctx, PCL_ENOMEM, "thread pool");
    }
    const int cols = ctx->cols;
    const long long nn = (long long)ctx->n * ctx->n, tail = ctx->x_dim * (ctx->desc.n_drives + 1), xd = ctx->x_dim;
    const bool expo = ctx->exp != 0;
    const int nvar = ctx->var, vexp = ctx->vexp;
    const double *hc = ctx->hcompact;
    int store_w = 0;
    const pcl_host::stream_copy_fn copy = pcl_host::pick_stream_copy((int)ctx->opt_host_store_bytes, &store_w);
    ctx->last_host_store_bytes = store_w;
    ctx->pool->begin(2 * nbk, [=](long long job) {
        const long long bk = job >> 1;
        if (nvar && vexp)
            pcl_host::expand_interval_var_exp(vals + bk * fper, hc + bk * cper, cols, nn, nvar, xd, tail, (int)(job & 1), copy);
        else if (nvar)
            pcl_host::expand_interval_var(vals + bk * fper, hc + bk * cper, cols, nn, nvar, tail, (int)(job & 1), copy);
        else if (expo)
            pcl_host::expand_interval_exp(vals + bk * fper, hc + bk * cper, cols, nn, xd, tail, (int)(job & 1), copy);
        else
            pcl_host::expand_interval(vals + bk * fper, hc + bk * cper, cols, nn, tail, (int)(job & 1), copy);
    });
    int rc = PCL_OK;
    for (int c = 0; c < n_chunks; ++c) {
        if (rc == PCL_OK && hipEventSynchronize(ctx->ev_chunk[c]) != hipSuccess) rc = PCL_EHIP;
        ctx->pool->publish(2 * (nbk * (c + 1) / n_chunks));  // (on an error the workers still run to completion, on stale bytes)
    }
    ctx->pool->wait();
    if (rc != PCL_OK) return fail(ctx, PCL_EHIP, "hipEventSynchronize: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (delta) memcpy(delta, ctx->hdelta, (size_t)n_rows(ctx) * sizeof(double));
    if (tuning) {  // this call was one sample of the sweep
        const double t_call = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        const int ci = ctx->host_tune_calls % kHostTuneN;
        ctx->host_tune_t[ci] = std::min(ctx->host_tune_t[ci], t_call);
        if (++ctx->host_tune_calls == 2 * kHostTuneN) {
            int bi = 0;
            for (int c = 1; c < kHostTuneN; ++c)
                if (ctx->host_tune_t[c] < ctx->host_tune_t[bi]) bi = c;
            ctx->host_threads_tuned = std::min(kHostTuneCand[bi], (int)std::max(2u, std::thread::hardware_concurrency()));
            ctx->host_expand_GBps = (double)nv * 8.0 / ctx->host_tune_t[bi] / 1e9;
        }
    }
    return check_device_error(ctx, "pcl_eval_jac");
}
extern "C" int pcl_eval(pcl_ctx *ctx, const double *Z, double *delta) {
    if (ctx && !delta) return fail(ctx, PCL_EINVAL, "pcl_eval: delta is NULL");
    return host_eval_jac(ctx, Z, delta, nullptr);
}
extern "C" int pcl_jac(pcl_ctx *ctx, const double *Z, double *vals) {
    if (ctx && !vals) return fail(ctx, PCL_EINVAL, "pcl_jac: vals is NULL");
    return host_eval_jac(ctx, Z, nullptr, vals);
}
extern "C" int pcl_eval_jac(pcl_ctx *ctx, const double *Z, double *delta, double *vals) {
    if (ctx && (!delta || !vals)) return fail(ctx, PCL_EINVAL, "pcl_eval_jac: NULL output");
    return host_eval_jac(ctx, Z, delta, vals);
}
extern "C" int pcl_hess(pcl_ctx *ctx, const double *Z, const double *mu, double *vals) {
    if (!ctx) return PCL_EINVAL;
    if (!Z || !mu || !vals) return fail(ctx, PCL_EINVAL, "pcl_hess: NULL pointer");
    TRY(require(ctx, FEAT_HESS, "pcl_hess"));
    ON_DEVICE(ctx);
    TRY(resolve_order(ctx, Z, "pcl_hess"));
    const long long nv = hess_per(ctx) * ctx->win_count * ctx->K;
    TRY(ensure(ctx, &ctx->dZ, z_len(ctx)));
    TRY(ensure(ctx, &ctx->dmu, n_rows_all(ctx)));
    TRY(ensure(ctx, &ctx->dhess, hess_per(ctx) * (ctx->var ? 1 : ctx->desc.batch) * ctx->K));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dZ, Z, z_len(ctx) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dmu, mu, n_rows(ctx) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TRY(launch_hess(ctx, ctx->dZ, ctx->dmu, ctx->dhess));
    HIP_TRY(ctx, hipMemcpyAsync(vals, ctx->dhess, nv * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_device_error(ctx, "pcl_hess");
}

extern "C" int pcl_rollout(pcl_ctx *ctx, const double *Z, double *X_out) {
    if (!ctx) return PCL_EINVAL;
    if (!Z || !X_out) return fail(ctx, PCL_EINVAL, "pcl_rollout: NULL pointer");
    TRY(require(ctx, FEAT_OBJECTIVE, "pcl_rollout"));
    ON_DEVICE(ctx);
    const long long nv = (long long)ctx->win_count * ctx->desc.N * ctx->x_dim;
    TRY(ensure(ctx, &ctx->dZ, z_len(ctx)));
    TRY(ensure(ctx, &ctx->dxout, (long long)ctx->desc.batch * ctx->desc.N * ctx->x_dim));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dZ, Z, z_len(ctx) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TRY(pcl_rollout_dev(ctx, ctx->dZ, ctx->dxout));
    HIP_TRY(ctx, hipMemcpyAsync(X_out, ctx->dxout, nv * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

#include "pcl_host_objective.hpp"
#include "pcl_host_robust.hpp"
#include "pcl_host_comm.hpp"
#include "pcl_host_options.hpp"
