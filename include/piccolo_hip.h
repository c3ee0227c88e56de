/*
 * piccolo_hip.h -- C ABI of libpiccolo_hip.so: the MI355X (gfx950) evaluator for
 * the Pade-integrator collocation constraint of Piccolo.jl / DirectTrajOpt.jl.
 *
 * This is the drop-in boundary for ONE path of the reference: what a
 * `DirectTrajOpt.AbstractIntegrator` has to provide to the NLP evaluator.  Each
 * entry point names the reference interface it replaces (paths relative to the
 * reference checkout, harmoniqs/Piccolo.jl v2.0.2; [EXT] = un-vendored
 * DirectTrajOpt.jl, known from Piccolo's call sites):
 *
 *   pcl_create            BilinearIntegrator(qtraj::UnitaryTrajectory, N)     src/control/integrators.jl:35-51
 *                         BilinearIntegrator(qtraj::KetTrajectory, N)         src/control/integrators.jl:58-74  (state_cols = 1)
 *                         BilinearIntegrator(qtraj::SamplingTrajectory, N)    src/control/integrators.jl:134-162
 *                         (copies G_drift / G_drives of sys.G, quantum_systems.jl:225-226,
 *                          composite_quantum_systems.jl:124-132, and the component ranges of the
 *                          NamedTrajectory, named_trajectory_conversion.jl:339-351)
 *   pcl_create            VariationalUnitaryIntegrator(sys, traj, :U, [:U_var, ...], :u; scales)   src/control/integrators.jl:247-264
 *                         VariationalKetIntegrator(sys, traj, :psi, [:psi_var, ...], :u; scale)    src/control/integrators.jl:234-245
 *                         (batch_mode PCL_BATCH_VARIATIONAL; VariationalQuantumSystem, variational_quantum_systems.jl:66-124;
 *                          generator var_G(G(u), [G_var_i / scale_i]), isomorphisms.jl:398-422)
 *   pcl_constraint_dim    B.dim == x_dim*(N-1), B.x_dim                        src/control/integrators.jl:307-309
 *   pcl_eval[_dev]        evaluate!(delta, B, traj) [EXT]                      src/control/integrators.jl:311,777
 *   pcl_jac_nnz/structure jacobian structure handed to MOI [EXT]; shape pin    src/control/integrators.jl:780-783
 *   pcl_jac[_dev]         eval_jacobian(B, traj) [EXT]                         src/control/integrators.jl:780
 *   pcl_eval_jac[_dev]    eval_constraint + eval_constraint_jacobian of one IPM iteration (fused)
 *   pcl_hess_nnz/structure, pcl_hess[_dev]
 *                         hessian_structure / Hessian-of-Lagrangian [EXT]      test/aqua.jl:6-9,
 *                                                                              src/control/templates/spline_pulse_problem.jl:96
 *
 * Semantics.  With h = dt_k, G = G0 + sum_j u_{k,j} G_j (n x n, n = 2d), X_k the
 * n x d matrix whose column c is Utilde_k[c*n .. (c+1)*n) (isomorphisms.jl:110-118):
 *     delta_k = B^-(hG) X_{k+1} - B^+(hG) X_k ,   B^{+-}(A) = I +- A/2 + A^2/12      (Pade order 4)
 * (BASELINE.json north_star; the reference's own constraint is the matrix
 * exponential x_{k+1} = exp(h Ghat) x_k, docs/src/concepts/index.md:21, of which
 * this is the (2,2) diagonal Pade discretisation -- see DESIGN.md.)
 *
 * Variable vector = [traj.datavec ; traj.global_data]; component i of knot k is
 * variable k*z_dim + i (integrators.jl:781-783).  Rows: member b, interval k,
 * component r -> b*x_dim*K + k*x_dim + r (integrators are concatenated in
 * prob.integrators order, integrators.jl:316-317); the caller adds the row offset
 * of this integrator block inside the full constraint vector.
 *
 * Jacobian values, per (member b, interval k), contiguous block of
 * jac_nnz_per_interval = 2*d*n*n + x_dim*(m+1) doubles, blocks ordered b-major then k:
 *     seg 0  d delta/d X_k      for c<d, j<n, i<n : -B^+[i,j]   row c*n+i, col x_off + c*n+j     (knot k)
 *     seg 1  d delta/d X_{k+1}  same loop          :  B^-[i,j]                                    (knot k+1)
 *     tail   for c<cols (state column): for l<m, i<n : d delta[c*n+i]/d u_l   col u_off + l         (knot k)
 *                                       then   i<n : d delta[c*n+i]/d dt    col dt_off
 *            (column-major: the (m+1)*n doubles one state column produces are contiguous -- full-line stores)
 * Hessian-of-Lagrangian values per (b,k), hess_nnz_per_interval = (m+1)(m+2)/2 + 2*x_dim*(m+1):
 *     seg 0 (u_i,u_j) j<=i | seg 1 (dt,u_j) | seg 2 (dt,dt) | seg 3 (u_l, X_k[r]) | seg 4 (dt, X_k[r])
 *     seg 5 (X_{k+1}[r], u_l) | seg 6 (X_{k+1}[r], dt)   -- each pair once, as (max index, min index).
 * The order is never assumed by a caller: it is reported by pcl_*_structure.
 *
 * Conventions: every function returns 0 (PCL_OK) or a negative pcl_status; the
 * message is available from pcl_last_error.  No exceptions, no abort(), no
 * pointer retained past a call (G0/Gj/x_offs are copied by pcl_create).  The
 * caller owns all Z/delta/vals/mu/rows/cols buffers.  A pcl_ctx is not
 * thread-safe: one context per (host thread x GPU).  Host-pointer entry points
 * are synchronous; *_dev entry points enqueue on the context's stream and return.
 * There is NO CPU fallback: without a gfx950 device pcl_create fails with PCL_EHIP.
 */
#ifndef PICCOLO_HIP_H
#define PICCOLO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pcl_ctx pcl_ctx;

typedef enum pcl_status {
    PCL_OK = 0,
    PCL_EINVAL = -1,  /* bad argument / descriptor */
    PCL_ENOMEM = -2,  /* host or device allocation failed */
    PCL_EHIP = -3,    /* HIP runtime error (incl. "no GPU") */
    PCL_ERCCL = -4,   /* RCCL error */
    PCL_ESHAPE = -5,  /* shape outside what the kernels support (d > PCL_MAX_D, ...) */
    PCL_ENOTIMPL = -6, /* valid request the library does not implement (e.g. an odd pade_order) */
    PCL_EINTERNAL = -7 /* a kernel of this context reported a failure on the device (a bounded wait between its waves gave up): the
                          outputs of that launch are incomplete; returned by the next evaluator entry point or pcl_sync, then cleared */
} pcl_status;

/* pcl_desc.pade_order: the EXACT exponential constraint instead of a diagonal Pade discretisation of it,
 *     delta_k = X_{k+1} - exp(dt_k G(u_k)) X_k
 * -- the reference's own (docs/src/concepts/index.md:21) -- for steps too large for order 10 (the order policy's order_tol_met = 0).  Chosen at
 * creation only; nothing switches to it on its own.  Shapes: unitary, ket, PCL_STATE_VECTOR; PCL_BATCH_MEMBERS (shared or per-member G0) and
 * PCL_BATCH_TRAJ with the member window; m = 0; PCL_BATCH_VARIATIONAL: PCL_ENOTIMPL (the variational integrators take it as PCL_BATCH_VARIATIONAL_EXP).  Rows as always.  Jacobian values per (member b, interval k),
 * jac_nnz_per_interval = cols*n*n + x_dim*(m + 2) doubles (reported by pcl_jac_structure, never assumed), E = exp(h G), L_l the Frechet derivative
 * of exp at h G along h G_l:
 *     seg 0  d delta/d X_k      for c<cols, j<n, i<n : -E[i,j]   row c*n+i, col x_off + c*n+j     (knot k)
 *     seg 1  d delta/d X_{k+1}  for r<x_dim          : +1        row r,     col x_off + r         (knot k+1; the identity as its diagonal)
 *     tail   per state column c: for l<m, i<n : -(L_l X_k)[i,c]  col u_off + l ; then i<n : -(G E X_k)[i,c]  col dt_off   (the Pade layout)
 * Served: pcl_create / pcl_destroy, pcl_constraint_dim, pcl_jac_nnz, pcl_jac_structure[_i64], pcl_eval[_dev], pcl_jac[_dev], pcl_eval_jac[_dev]
 * (host-pointer calls deliver full values), pcl_set_member_window, streams and sync, options, pcl_deriv_*, pcl_rollout[_dev] and the whole
 * objective family -- the last three with the bits a Pade context of the same system gives.  PCL_ENOTIMPL: pcl_hess[_dev], pcl_hess_nnz,
 * pcl_hess_structure[_i64] (the (u_i, u_j) block of the Hessian of the Lagrangian needs second Frechet derivatives: opt in below, or solve
 * with a quasi-Newton Hessian, the reference's eval_hessian = false), the compact Jacobian trio and the merit / reduce entry points (pcl_merit_grad_len,
 * pcl_merit_grad_dev, pcl_eval_jac_merit_dev, pcl_eval_jac_merit_objective_dev) -- both groups: opt in below.
 * pcl_set_order_policy and pcl_set_order_from_trajectory: PCL_EINVAL (there is no order to choose).  get_option "pade_order" reads -1,
 * "last_kernel" 100 (residual + Jacobian) or 101 (residual only).
 *
 * The Hessian of the Lagrangian, by option: pcl_set_option(ctx, "exp_hess", 1) on such a context (0, the default: the refusals above, in the
 * same words; 1 on any other context: PCL_EINVAL; reading works everywhere) makes the five Hessian entry points serve it, for every shape and
 * batch mode of the mode with a generator dimension n <= 62 (five n x n LDS tiles; beyond: PCL_ESHAPE with the byte counts, from the option).
 * Nothing involves X_{k+1} (delta_k is X_{k+1} minus something), so per (member b, interval k) there are
 * hess_nnz_per_interval = (m+1)(m+2)/2 + x_dim*(m+1) doubles (reported by pcl_hess_nnz, never assumed) -- the Pade layout without its last two
 * groups, lower triangle (row >= col), with M = the interval's multipliers as an n x cols matrix, L2 the second Frechet derivative of exp:
 *     seg 0  (u_i, u_j), j <= i : -<M, L2(hG; hG_i, hG_j) X_k>        seg 3  for l<m, r<x_dim : (u_l, X_k[r])   -(L_l' M)[r]
 *     seg 1  (dt, u_j)          : -<M, (G_j E + G L_j) X_k>           seg 4  for r<x_dim      : (dt,  X_k[r])   -((G E)' M)[r]
 *     seg 2  (dt, dt)           : -<M, G G E X_k>
 * get_option "last_hess_kernel" reads 100 after such a launch.  The other refusals of the mode do not depend on the option.
 *
 * The compact Jacobian, the host expansion and the reduce payload, by option: pcl_set_option(ctx, "exp_full", 1) on such a context (0, the default:
 * the refusals above, in the same words, and host-pointer calls that deliver full values; 1 on any other context -- Pade, variational of either
 * kind --: PCL_EINVAL; reading works everywhere; independent of "exp_hess") serves the seven entry points named above:
 *   - the compact trio: per (member b, interval k) the unique values are  [ -E (n*n) | tail (x_dim*(m+1), exactly the full layout's tail) ],
 *     n*n + x_dim*(m+1) doubles (pcl_jac_compact_nnz; the ones of seg 1 are constants and no part of it).  pcl_eval_jac_compact_dev runs the
 *     recurrence of the full launch and stores one -E per interval ("last_kernel" 102); pcl_jac_expand_dev writes cols copies of -E, x_dim ones and
 *     the tail: bit for bit what pcl_eval_jac_dev writes, and delta has its bits too.  pcl_set_member_window applies as on a Pade context.
 *   - pcl_eval_jac / pcl_jac with more than one state column take the compact path unless "host_path" = 1 (compact launch, chunked copies into
 *     pinned staging, the host's threads replicate): the caller's array receives the bits of the full path.
 *   - pcl_merit_grad_len / pcl_merit_grad_dev as on a Pade context (the tails start behind cols*n*n + x_dim values); pcl_eval_jac_merit_dev forms the
 *     payload's partial sums inside the Jacobian launch, reduced per workgroup in a fixed order ("last_merit_fused" 1; delta and vals exactly as by
 *     pcl_eval_jac_dev); pcl_eval_jac_merit_objective_dev runs its two-call fallback.  All of every member, as documented at the member window.
 *   - pcl_eval_jac_merit_dev with vals_dev == NULL (PCL_EINVAL everywhere else): delta and the payload WITHOUT the Jacobian.  With A = h G(u_k),
 *     W = Lam X_k' and V = L(A'; W):  <Lam, L(A; h G_l) X_k> = h <V, G_l>,  <Lam, G E X_k> = <V, G0> + sum_l u_l <V, G_l>  -- one pair chain per
 *     (member, interval) instead of one per drive, behind the residual-only launch and a preparation launch; a workspace of
 *     batch*K*(2 n*n + 2) doubles is allocated on first use (shared with "exp_hess"), freed by pcl_destroy.  "last_kernel" 103, "last_merit_fused" 0.
 *   Every payload launch is deterministic: two launches give the same bits. */
#define PCL_ORDER_EXP (-1)

#define PCL_MAX_D 32 /* n = 2d <= 64: G(u_k), G^2 and the column tiles stay LDS-resident */

/* batch_mode */
#define PCL_BATCH_MEMBERS 0 /* ONE trajectory buffer; member b owns state columns at x_offs[b]; shared u, dt
                               (SamplingTrajectory: sampling_trajectory.jl:207-237) */
#define PCL_STATE_VECTOR (-1) /* pcl_desc.state_cols: see there */
#define PCL_BATCH_TRAJ 1    /* batch independent trajectory buffers (multistart seeds), Z_b = Z + b*z_dim*N;
                               x_offs[0] is the state offset in each */
#define PCL_BATCH_VARIATIONAL 2 /* the variational (sensitivity) integrators: ONE trajectory whose state is the stack [X; Xv_1; ...; Xv_v]
                               of the state and its first-order sensitivities to v perturbation directions (v = 1, 2 for d <= 32; more:
                               PCL_ESHAPE), evolved by the lifted generator var_G(G(u), [Gv_i]) = [[G, 0..], [Gv_1, G, 0..], .., [Gv_v, 0.., G]]
                               per state column.  batch = 1 + v; x_offs[0] the state, x_offs[i] variation i; per_member_G0 = 1 with
                               G0[0] = G_drift and G0[i] = Gv_i = G(H_var_i) / scale_i (the caller applies the scales); state_cols d
                               (unitary) or 1 (ket), not PCL_STATE_VECTOR (with PCL_LARGE_N | PCL_LARGE_VAR at d > 32 also any count of
                               kets between: see PCL_LARGE_VAR).
                               x_dim (pcl_constraint_dim) is the stacked (1 + v) n C.  Rows are KNOT-major over the stacked state,
                               row k*x_dim + b*(n C) + c*n + i (component b, state column c) -- the reference's B.dim = x_dim (N-1) -- and
                               NOT the member-major order of PCL_BATCH_MEMBERS.  Jacobian values per interval (pcl_jac_structure):
                                 -B^+ and B^- of delta_0 (C n^2 each, I_C (x) .), then per variation i: -B^+ (Xv_i,k), B^- (Xv_i,k+1),
                                 -L^+_i (X_k), L^-_i (X_{k+1}) with L^{+-}_i = sum_{j>=1} c_j (+-h)^j Q_j^i the (i,0) blocks of the
                                 lifted powers; then the tails, (m+1) n per state column for each of the 1 + v components (component-major)
                               -- (2 + 4v) C n^2 + x_dim (m+1) values, no structural zeros.  Hessian: the segments below over the stacked
                               state.  Entry points: create, dimensions, structures, pcl_eval[_dev], pcl_jac[_dev], pcl_eval_jac[_dev],
                               pcl_hess[_dev] (host-pointer calls deliver full values), the order policy (theta of the lifted generator),
                               streams, options, pcl_deriv_*; every other entry point returns PCL_ENOTIMPL -- unless the context's option
                               "var_full" is set to 1 (pcl_set_option; default 0).  Then the robust-control objective and the rollout are
                               served as well: pcl_set_goal, pcl_set_goal_subspace (unitary), pcl_set_goal_form with scope 0 (the loss of
                               component 0, the state itself; A is R x (n C); scope 1 stays PCL_ENOTIMPL), pcl_add_regularizer /
                               pcl_clear_regularizers (any component of the knot), pcl_set_weights, pcl_objective[_dev],
                               pcl_objective_hess_nnz / _structure / [_dev] and pcl_rollout[_dev]; see their comments.  Setting the option
                               back to 0 restores the refusals and drops goal, weights and regularisers.  pcl_infidelity_dev, the merit /
                               reduce entry points and the member window stay PCL_ENOTIMPL whatever the option says; so does the compact
                               Jacobian trio unless the context's option "var_compact" = 1 serves it (see pcl_jac_compact_nnz; the host-pointer
                               calls then deliver through the compact values where C > 1; "last_kernel" reads 72 after a compact launch).
                               The sensitivity term is evaluated at the TERMINAL knot only (the reference's own use, materialize.jl:306-307). */

#define PCL_BATCH_VARIATIONAL_EXP 3 /* the same integrators on the EXACT exponential constraint x'_{k+1} = exp(dt_k Ghat) x'_k of the lifted generator
                               Ghat = var_G(G(u), [Gv_i]) -- what the reference's VariationalUnitaryIntegrator / VariationalKetIntegrator are
                               (BilinearIntegrator(var_G(..))) -- for the steps whose lifted theta no Pade order follows.  The descriptor of
                               PCL_BATCH_VARIATIONAL (batch = 1 + v with v = 1, 2, x_offs per component, per_member_G0 = 1, state_cols d or 1,
                               rows knot-major over the stacked state) with pade_order = PCL_ORDER_EXP; any other order: PCL_EINVAL.  Generator
                               dimension n <= 62 (five n x n LDS tiles; beyond: PCL_ESHAPE with the byte counts, from pcl_create).  With h = dt_k,
                               A = h G(u_k), E = exp(A), L_i = L(A; h Gv_i), L_l = L(A; h G_l) (Frechet derivatives of exp) and
                               L2_il = L2(A; h Gv_i, h G_l) (the second one):
                                 delta_0 = X_{k+1} - E X_k            delta_i = Xv_{i,k+1} - L_i X_k - E Xv_{i,k}
                               Jacobian values per interval (pcl_jac_structure reports them; never assumed):
                                 -E of delta_0 w.r.t. X_k (C n^2, I_C (x) .); per variation i: -E w.r.t. Xv_i,k, then -L_i w.r.t. X_k;
                                 then +1 for r < x_dim' = (1 + v) n C (d delta / d X'_{k+1}, the identity as its diagonal); then the tails,
                                 component-major, per state column c: for l<m the n values of column u_off + l, then the n of column dt_off:
                                   component 0: -(L_l X_k)[:,c]                     and -(G E X_k)[:,c]
                                   component i: -(L2_il X_k + L_l Xv_i,k)[:,c]      and -((Gv_i E + G L_i) X_k + G E Xv_i,k)[:,c]
                               -- (1 + 2v) C n^2 + x_dim' (m + 2) values, no structural zeros.  Served: create / destroy, dimensions,
                               pcl_jac_nnz / _structure[_i64], pcl_eval[_dev], pcl_jac[_dev], pcl_eval_jac[_dev] (host-pointer calls deliver
                               full values), streams, sync, options, pcl_deriv_*; with option "var_full" = 1 the robust-control objective
                               family and pcl_rollout[_dev] exactly as on a PCL_BATCH_VARIATIONAL context, with its bits.  PCL_ENOTIMPL, naming
                               the mode: pcl_hess[_dev], pcl_hess_nnz, pcl_hess_structure[_i64] and option "exp_hess" = 1 (the Hessian of the
                               Lagrangian needs third Frechet derivatives: solve with a quasi-Newton Hessian) unless option "var_exp_hess" = 1
                               is set (generator dimensions up to 44; see pcl_hess), the compact Jacobian trio unless option "var_compact" = 1
                               is set (see pcl_jac_compact_nnz; "last_kernel" 112 after a compact launch), the
                               merit / reduce entry points, the member window, pcl_infidelity_dev.  pcl_set_order_policy and
                               pcl_set_order_from_trajectory: PCL_EINVAL (there is no order to choose).  "var_block_wgs" / "var_col_wgs" have no
                               effect.  get_option "pade_order" reads -1, "variations" v, "last_kernel" 110 (residual + Jacobian) or 111
                               (residual only). */

/* pcl_desc.batch_mode flag, OR-ed with PCL_BATCH_MEMBERS or PCL_BATCH_TRAJ: generator dimensions 66 .. 128 on the Pade constraint -- the
 * reference's transmon-cavity template (4 x 12 levels: n = 96; 4 x 15: n = 120), compact density vectors of 9 .. 11 levels (n = 81, 100, 121),
 * cat-buffer systems, ion chains with phonon modes.  Chosen at creation only; nothing sets it on its own, and without it every context is what
 * it was (n > 64: PCL_ESHAPE).  pcl_create strips the flag and stores the plain batch mode.  With the flag:
 *   n <= 64                the ordinary context: the same kernels, the same bits
 *   66 <= n <= 128         a LARGE context; even n for unitary / ket / multi-ket states, any n (odd included) under PCL_STATE_VECTOR
 *   n > 128                PCL_ESHAPE (one n x n LDS tile is all a workgroup's 163,840 B can hold: 132,096 B at n = 128)
 *   PCL_BATCH_VARIATIONAL, PCL_BATCH_VARIATIONAL_EXP or pade_order = PCL_ORDER_EXP: PCL_ENOTIMPL (the exponential constraint: by the second flag
 *                          PCL_LARGE_EXP, below)
 * -- all decided before the device is touched.  A large context runs one kernel family (pcl_kernel_pade_large.hpp: one LDS tile, the powers of
 * G by column panels, the drives in groups where their chain blocks do not fit beside the tile) at Pade orders 2 .. 10 with
 * shared or per-member G0, both batch modes, the member window, 1 .. d state columns and m = 0 .. 24 drives; values, order and layout are those
 * of every other Pade context.  Every work split gives the same bits and two launches give the same bits (no atomics).
 * Served: pcl_create / pcl_destroy, pcl_constraint_dim, pcl_jac_nnz, pcl_jac_structure[_i64], pcl_eval[_dev], pcl_jac[_dev], pcl_eval_jac[_dev]
 * (host-pointer calls deliver full values unless the option "large_reduce" is on: below), pcl_set_member_window, streams and sync, options,
 * pcl_deriv_*, and pade_order = 0 with
 * pcl_set_order_policy / pcl_set_order_from_trajectory.  PCL_ENOTIMPL, each message naming PCL_LARGE_N: pcl_hess[_dev], pcl_hess_nnz,
 * pcl_hess_structure[_i64] (unless the option "large_hess" is on: below), the compact Jacobian trio and the merit /
 * reduce entry points (pcl_merit_grad_len, pcl_merit_grad_dev, pcl_eval_jac_merit_dev, pcl_eval_jac_merit_objective_dev; unless the option
 * "large_reduce" is on: below), and -- unless the
 * option "large_full" is on: below -- pcl_rollout[_dev] and the objective family (goals, weights, regularisers, pcl_infidelity_dev,
 * pcl_objective[_dev], pcl_objective_hess_*).
 * The Hessian of the Lagrangian: pcl_set_option "large_hess" = 1 (0 by default, never on by itself; PCL_EINVAL on a context that is not large)
 * makes pcl_hess[_dev], pcl_hess_nnz and pcl_hess_structure[_i64] serve a large context -- values, order and structure those of every other
 * Pade context, at orders 2 .. 10, both batch modes, the member window (pcl_kernel_pade_large_hess.hpp: a forward Horner chain and backward
 * chains on G^T, per-column partial sums added in column order by a second launch; no atomics, every work split bitwise equal; DESIGN.md
 * 4.18).  Its device workspace (batch x (N - 1) x state columns x (m^2 + m + 1) doubles) is allocated when the option is first set to 1.
 * Back at 0 the refusals return; without the option solve with a quasi-Newton Hessian (the reference's eval_hessian = false).
 * The objective and the rollout: pcl_set_option "large_full" = 1 (0 by default, never on by itself; PCL_EINVAL on a context that is not large,
 * and for any value outside 0 and 1; independent of "large_hess") makes pcl_set_goal, pcl_set_goal_subspace, pcl_set_goal_form, pcl_set_weights,
 * pcl_add_regularizer, pcl_clear_regularizers, pcl_infidelity_dev, pcl_objective[_dev], pcl_objective_hess_nnz, pcl_objective_hess_structure,
 * pcl_objective_hess[_dev] and pcl_rollout[_dev] serve a large context with the contracts of n <= 64 (matrix and subspace goals: unitary states
 * only; a subspace goal of more than 45 levels is PCL_ESHAPE with the rows or LDS bytes it needs; a unitary goal's Hessian is x_dim (x_dim + 1) / 2
 * doubles per goal and per evaluation, 268 MB at d = 64, and a failed allocation is PCL_ENOMEM).  The rollout is two launches on the one-tile
 * plan (pcl_kernel_large_rollout.hpp: propagators by column panels as a substepped degree-18 Taylor polynomial, then the chain of the knots; no
 * atomics, every work split bitwise equal); its workspace (batch x (N - 1) x n^2 doubles) is allocated at the first rollout.
 * Back at 0 the refusals return and goal, weights and regularisers are dropped.
 * The compact Jacobian and the reduce payload: pcl_set_option "large_reduce" = 1 (0 by default, never on by itself; PCL_EINVAL on a context that
 * is not large, and for any value outside 0 and 1; independent of the other two) makes pcl_jac_compact_nnz, pcl_eval_jac_compact_dev,
 * pcl_jac_expand_dev, pcl_merit_grad_len, pcl_merit_grad_dev and pcl_eval_jac_merit_dev serve a large context with the contracts of n <= 64:
 * the compact layout [-B+ (n^2) | B- (n^2) | tails] per interval (one state column: the full layout), the member window on the compact trio, every
 * member on the merit entry points.  pcl_eval_jac_merit_dev accepts vals = NULL there: delta and the payload alone, chain units only, no Jacobian
 * value formed or written.  pcl_eval_jac_merit_objective_dev needs "large_full" = 1 as well (and a unitary goal); with "large_reduce" alone it
 * stays refused in the same words.  Member weights are the objective family's: pcl_set_weights is served by "large_full".  The host-pointer
 * calls then take the compact route (compact values over PCIe, expanded by the host's threads) when the state has more than one column and
 * "host_path" is not 1.  Modes of the one kernel family (pcl_kernel_pade_large.hpp) and pcl_expand_large_kernel; the compact values have the bits
 * of the full launch's, the expansion the bits of pcl_eval_jac_dev, and the payload of the fused launch the bits of the payload-only launch under
 * every work split (no atomics).  Back at 0 the refusals return.
 * Options: "cols_per_slice" caps the state columns per workgroup (Jacobian, Hessian and the rollout's chain), "general_slices" sets the least
 * number of workgroups per interval of the Jacobian launch and of the rollout's propagator launch, "large_hess_drives" caps the drives per workgroup of the Hessian launch (0 auto; PCL_EINVAL when negative or
 * off a large context); "kernel_version", "general_kernel_version", "general_threads", "use_mfma", "hess_kernel", "nt" = 2 have no effect.
 * get_option "last_kernel" reads 290 + q after a Jacobian launch (with or without the payload's partial sums), 300 + q after a compact launch,
 * 310 + q after a payload-only launch, 280 + q after a residual-only launch and 270 after a rollout,
 * "last_hess_kernel" 290 + q after a Hessian launch (q = pade_order / 2). */
#define PCL_LARGE_N 0x100
#define PCL_LARGE_MAX_N 128

/* A second pcl_desc.batch_mode flag, beside PCL_LARGE_N: the exponential constraint  delta_k = X_{k+1} - exp(dt_k G(u_k)) X_k  at generator
 * dimensions 66 .. 128 -- the sizes at which a step most easily outgrows Pade order 10.  Valid only together with PCL_LARGE_N, PCL_BATCH_MEMBERS
 * or PCL_BATCH_TRAJ, and pade_order = PCL_ORDER_EXP; chosen at creation only, never set on its own; pcl_create strips it as it strips PCL_LARGE_N.
 *   PCL_LARGE_EXP without PCL_LARGE_N, or with a Pade order or order 0      PCL_EINVAL
 *   with a variational batch mode                                           PCL_LARGE_N's refusal of those modes
 *   PCL_LARGE_N with PCL_ORDER_EXP and without this flag                    PCL_ENOTIMPL, as before
 *   both flags, n <= 64                                                     the ordinary exponential context: the same kernels, the same bits
 *   both flags, 66 <= n <= 128                                              a LARGE EXPONENTIAL context (even n, or any n under PCL_STATE_VECTOR)
 *   both flags, n > 128                                                     PCL_ESHAPE
 * -- all decided before the device is touched.  Such a context runs one kernel (pcl_kernel_large_exp.hpp: one LDS tile, the substepped
 * degree-18 Taylor polynomial in action form with the derivative carried through it, s' = ceil(|dt| |G|_1) substeps) with shared or
 * per-member G0, both batch modes, the member window, 1 .. d state columns and m = 0 .. 24 drives.  Values, order, layout and structure are
 * those of the exponential mode at n <= 64: per interval `cols` copies of -E, the diagonal ones of d delta / d X_{k+1}, then the tails
 * -L_l X_k and -G E X_k: cols n^2 + x_dim (m + 2) values.  No atomics: every work split and two launches give the same bits, and the
 * residual-only launch gives the bits of the fused launch's residual.  The cost is linear in s', where the kernels of n <= 64 are logarithmic.
 * Served: pcl_constraint_dim, pcl_jac_nnz, pcl_jac_structure[_i64], pcl_eval[_dev], pcl_jac[_dev], pcl_eval_jac[_dev] (host-pointer calls
 * deliver full values), pcl_set_member_window, streams and sync, options, pcl_deriv_*; and with the option "large_full" = 1 the objective
 * family and pcl_rollout[_dev], on the kernels of a large Pade context (neither depends on the constraint; the rollout then has the
 * discretisation of the rows).  PCL_ENOTIMPL, each message naming PCL_LARGE_EXP: pcl_hess[_dev], pcl_hess_nnz, pcl_hess_structure[_i64], the
 * compact Jacobian trio, the merit / reduce entry points, and the options "exp_hess", "exp_full", "large_hess", "large_reduce" = 1.
 * pcl_set_order_policy / pcl_set_order_from_trajectory: PCL_EINVAL, as on every exponential context.
 * Options: "cols_per_slice" caps the state columns per workgroup, "general_slices" sets the least number of workgroups per interval,
 * "large_exp_drives" caps the drives per workgroup (0 auto; PCL_EINVAL when negative or off such a context).  get_option "pade_order" reads -1,
 * "last_kernel" 320 after a residual + Jacobian launch and 321 after a residual-only launch.
 * Option "large_exp_hess" (default 0, never on by itself; 1 on any other context and any value but 0 and 1: PCL_EINVAL; it reads 0 everywhere
 * else): at 1 pcl_hess, pcl_hess_dev, pcl_hess_nnz and pcl_hess_structure[_i64] are served -- values, order and structure are those of the option
 * "exp_hess" at n <= 62: per interval (m + 1)(m + 2) / 2 + x_dim (m + 1) values [(u_i,u_l), l <= i | (dt,u_l) | (dt,dt) | (u_l,X_k) | (dt,X_k)].
 * pcl_kernel_large_exp_hess.hpp: the adjoint of the Jacobian's substepped recurrence on G^T, started from the multipliers, with the second
 * derivative carried; one workgroup per (interval, slice of state columns, pair of drive groups), per-column partial sums in a
 * workspace (allocated when the option is first set to 1, freed by pcl_destroy) added in column order by a second launch on the same stream: no
 * atomics, every work split, two launches and both pointer paths give the same bits.  Back at 0 the refusals return, in the same words; the
 * compact trio, the merit / reduce entry points and the options "exp_hess", "large_hess" = 1 stay refused at either value.
 * "large_exp_hess_drives" caps the drives per group of that launch (0 auto; PCL_EINVAL when negative or off such a context), "cols_per_slice"
 * its state columns per workgroup; get_option "last_hess_kernel" reads 320 after it.
 * Option "large_exp_reduce" (default 0, never on by itself; 1 on any other context and any value but 0 and 1: PCL_EINVAL; it reads 0 everywhere
 * else; independent of "large_full" and "large_exp_hess"): at 1 pcl_jac_compact_nnz, pcl_eval_jac_compact_dev, pcl_jac_expand_dev,
 * pcl_merit_grad_len, pcl_merit_grad_dev and pcl_eval_jac_merit_dev (vals = NULL accepted: delta and the payload alone) are served with the
 * contracts of the option "exp_full" at n <= 64 -- compact layout per interval [-E (n^2) | tails x_dim (m + 1)], tails in the order of the full
 * layout -- as modes of the one kernel, and the host-pointer calls take the compact route where blocks are replicated (cols > 1,
 * "host_path" != 1).  pcl_eval_jac_merit_objective_dev also needs "large_full" = 1 and a unitary goal; member weights come from pcl_set_weights,
 * hence "large_full".  The compact trio honours the member window, the merit entry points cover every member.  Compact values = full values,
 * expansion = pcl_eval_jac_dev, fused payload = payload alone, every work split: the same bits.  Back at 0 the refusals return, in the same
 * words; "exp_full" and "large_reduce" = 1 stay PCL_ENOTIMPL at either value.  get_option "last_kernel" reads 322 after the compact launch and
 * 323 after the payload-only launch (320 after the full-values launch with or without the payload's partial sums: "last_merit_fused" tells). */
#define PCL_LARGE_EXP 0x200

/* A third pcl_desc.batch_mode flag, beside PCL_LARGE_N: the variational (sensitivity) integrators -- PCL_BATCH_VARIATIONAL on the Pade
 * constraint -- at generator dimensions 66 .. 128: robust control of the transmon-cavity sizes.  Chosen at creation only, never set on its own;
 * pcl_create strips it as it strips the other two.  PCL_BATCH_VARIATIONAL[_EXP] | PCL_LARGE_N WITHOUT this flag keeps PCL_LARGE_N's refusal.
 *   PCL_LARGE_VAR without PCL_LARGE_N, or with PCL_BATCH_MEMBERS / PCL_BATCH_TRAJ           PCL_EINVAL
 *   PCL_LARGE_VAR with PCL_BATCH_VARIATIONAL_EXP or with PCL_LARGE_EXP                      PCL_ENOTIMPL naming PCL_LARGE_VAR
 *   PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR, n <= 64                            the ordinary variational context: same kernels, same bits
 *   the same, 66 <= n <= 128 (n = 2d is even), v = 1 or 2, m <= 24, state_cols d, 1 or any
 *     count of kets between (the kernels are planned per slice of state columns; at n <= 64
 *     a count between stays PCL_EINVAL), pade_order 0 / 2 / 4 / 6 / 8 / 10                  a LARGE VARIATIONAL context
 *   the same, n > 128                                                                       PCL_ESHAPE with the byte counts, as for PCL_LARGE_N
 * -- all decided before the device is touched.  Such a context runs one kernel (pcl_kernel_var_large.hpp, on the one-tile plan of the large
 * family: chain workgroups per (interval, slice of state columns, drive group) carry W, V and the dW_l of all 1 + v components, panel workgroups
 * carry the powers of G and, one variation at a time, its Frechet powers).  Rows, value order, layout and structure are exactly
 * those of PCL_BATCH_VARIATIONAL at n <= 64: (2 + 4v) C n^2 + x_dim (m + 1) values per interval.  No atomics: every work split, two launches
 * and the residual-only launch against the fused launch's residual give the same bits; component 0 (delta_0, its tails, every -B+ | B- copy) has
 * the bits of a plain PCL_LARGE_N context of the same drift and drives.
 * Served: pcl_create / pcl_destroy, pcl_constraint_dim, pcl_jac_nnz, pcl_jac_structure[_i64], pcl_eval[_dev], pcl_jac[_dev], pcl_eval_jac[_dev]
 * (host-pointer calls deliver full values), streams and sync, options, pcl_deriv_*, and pade_order = 0 with pcl_set_order_policy /
 * pcl_set_order_from_trajectory (theta of the lifted generator, host arithmetic on up to 384 x 384).  PCL_ENOTIMPL, each message naming
 * PCL_LARGE_VAR: pcl_hess[_dev], pcl_hess_nnz, pcl_hess_structure[_i64], the options "var_full" = 1 (and the objective family and rollout behind
 * it) and "var_compact" = 1 (and the compact trio), the merit / reduce entry points, the member window, pcl_infidelity_dev.  The options
 * "large_hess", "large_full", "large_reduce", "large_exp_hess", "large_exp_reduce" = 1 are PCL_EINVAL, as on every context that is not of
 * their kind.
 * Options: "cols_per_slice" caps the state columns per chain workgroup, "general_slices" sets the least number of panel workgroups per role,
 * "var_large_drives" caps the drives per group (0 auto; PCL_EINVAL when negative or off such a context); "var_block_wgs" / "var_col_wgs" have
 * no effect.  get_option "last_kernel" reads 340 + q after a residual + Jacobian launch and 350 + q after a residual-only launch.
 * Option "large_var_full" (0 by default, never on by itself; 1 on every other kind of context, and any other value, PCL_EINVAL; readable
 * everywhere, 0 there): at 1 such a context serves pcl_set_goal, pcl_set_goal_subspace, pcl_set_goal_form (scope 0), pcl_set_weights,
 * pcl_add_regularizer, pcl_clear_regularizers, pcl_objective[_dev], pcl_objective_hess_nnz / _structure, pcl_objective_hess[_dev] and
 * pcl_rollout[_dev] with the contracts, layouts and value order of "var_full" at n <= 64: the robust-control objective and the rollout of the
 * stacked state x <- E x, x_i <- E x_i + L_i x, output [N][(1 + v) n C] (pcl_kernel_var_large_rollout.hpp; "last_kernel"
 * 360).  Back at 0 the refusals return in the same words and goal, weights and regularisers are dropped.  "var_full" = 1 stays PCL_ENOTIMPL
 * naming PCL_LARGE_VAR at either value, and so do the Hessian of the Lagrangian (its option is "large_var_hess", below), the compact trio, the merit / reduce entry points, the
 * member window and pcl_infidelity_dev.  A subspace goal of more than 45 levels is PCL_ESHAPE (2 ns^2 + 2 rows of the form against 4096);
 * a failed device allocation (a triangle of the objective's Hessian is 268 MB at d = 64) is PCL_ENOMEM and the context goes on as before.
 * Option "large_var_hess" (0 by default, never on by itself; 1 on every other kind of context, and any other value, PCL_EINVAL; readable
 * everywhere, 0 there): at 1 such a context serves pcl_hess_nnz, pcl_hess_structure[_i64], pcl_hess and pcl_hess_dev with the values, order and
 * structure of PCL_BATCH_VARIATIONAL at n <= 64 for the same pcl_desc: (m + 1)(m + 2) / 2 + 2 x_dim' (m + 1) values per interval over the
 * stacked state (pcl_kernel_var_large_hess.hpp: the chains of the large Hessian kernel on the lifted generator, one pass per component;
 * DESIGN.md 4.28; "last_hess_kernel" 340 + q).  Back at 0 the refusals return in the same words.  Its workspace is allocated when the option
 * is first set to 1 (PCL_ENOMEM when that fails) and freed by pcl_destroy.  "large_var_hess_drives" caps the drives per workgroup of that
 * launch (0 auto; PCL_EINVAL when negative or off such a context), "cols_per_slice" its state columns; every split gives the same bits.  With
 * multipliers that are zero on the variations, the scalars and the vectors of component 0 have the bits of a plain PCL_LARGE_N context with
 * "large_hess" on the same drift and drives.  The other refusals above stay at either value. */
#define PCL_LARGE_VAR 0x400

/* A fourth pcl_desc.batch_mode flag: the variational integrators on the EXACT exponential constraint (PCL_BATCH_VARIATIONAL_EXP, the reference's
 * own BilinearIntegrator(var_G(G(u), [Gv_i]))) at generator dimensions 66 .. 128.  Valid in ONE combination only,
 *     PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP   with   pade_order = PCL_ORDER_EXP;
 * chosen at creation only, pcl_create strips it with the others.  Every descriptor WITHOUT this flag behaves exactly as before (PCL_LARGE_VAR
 * with PCL_BATCH_VARIATIONAL_EXP, PCL_LARGE_EXP or PCL_ORDER_EXP keeps its PCL_ENOTIMPL).  With it, each PCL_EINVAL naming what is missing,
 * before the device is touched:
 *   without PCL_LARGE_N or PCL_LARGE_VAR; with PCL_BATCH_MEMBERS, PCL_BATCH_TRAJ or PCL_BATCH_VARIATIONAL;
 *   with a Pade order (or order 0); with PCL_LARGE_EXP (that flag belongs to plain contexts)                          PCL_EINVAL
 *   all four flags, n <= 64                        the ordinary PCL_BATCH_VARIATIONAL_EXP context: same kernels, same bits (n = 64: its PCL_ESHAPE)
 *   66 <= n <= 128, v = 1 or 2, m <= 24, state_cols d, 1 or any count of kets between              a LARGE VARIATIONAL EXPONENTIAL context
 *   n > 128                                                                                         PCL_ESHAPE with the byte counts, as for PCL_LARGE_VAR
 * Rows, value order, layout, structure, pcl_constraint_dim, pcl_jac_nnz and index_base are exactly those of PCL_BATCH_VARIATIONAL_EXP at
 * n <= 62: (1 + 2v) C n^2 + x_dim' (m + 2) values per interval, no structural zeros.  One kernel (pcl_kernel_var_large_exp.hpp):
 * the substepped degree-18 Taylor polynomial in action form on the lifted pair [V | Vv_i] with the drive derivative carried through it,
 * s' = ceil(|h| |G(u_k)|_1) substeps.  No atomics: every work split, two launches, both pointer paths and the residual-only launch against the
 * fused launch's residual give the same bits; component 0 (delta_0, every copy of -E, its tails) has the bits of a plain
 * PCL_LARGE_N | PCL_LARGE_EXP context of the same drift and drives.  h = 0 gives E = I, L_i = 0 and zero drive tails exactly.
 * Served: pcl_create / pcl_destroy, pcl_constraint_dim, pcl_jac_nnz, pcl_jac_structure[_i64], pcl_eval[_dev], pcl_jac[_dev], pcl_eval_jac[_dev]
 * (host-pointer calls deliver full values), streams and sync, options, and by option "large_var_full" = 1 the objective family and
 * pcl_rollout[_dev] through the kernels of a large variational context (the same bits: neither depends on the constraint; the rollout then has
 * the discretisation of the rows).  pcl_set_order_policy / pcl_set_order_from_trajectory: PCL_EINVAL, as on every exponential context.
 * PCL_ENOTIMPL, each message naming PCL_LARGE_VAR_EXP: pcl_hess[_dev], pcl_hess_nnz, pcl_hess_structure[_i64] (unless option
 * "large_var_exp_hess" is on: below), the compact trio, the merit /
 * reduce / step entry points, the collective and the member window, pcl_infidelity_dev, and the options "large_var_hess", "var_compact",
 * "var_exp_hess", "var_full" and "exp_hess" = 1.  The other large options = 1 are PCL_EINVAL, as on every context that is not of their kind.
 * Option "large_var_exp_hess" (0 by default, never on by itself; 1 on every other kind of context -- all four flags at n <= 64 included -- and
 * any other value, PCL_EINVAL; readable everywhere, 0 there): at 1 such a context serves pcl_hess_nnz, pcl_hess_structure[_i64], pcl_hess and
 * pcl_hess_dev with the values, order and structure of PCL_BATCH_VARIATIONAL_EXP with "var_exp_hess" at n <= 62 for the same pcl_desc:
 * (m + 1)(m + 2) / 2 + x_dim' (m + 1) values per interval, [(u_i,u_j), j <= i | (dt,u_j) | (dt,dt) | (u_l, X'_k) | (dt, X'_k)] over the stacked,
 * component-major state (pcl_kernel_var_large_exp_hess.hpp: the adjoint of the Jacobian's substepped recurrence on the lifted generator with the
 * second derivative carried, one pass per component as workgroups of their own, the passes added in order by a second launch; DESIGN.md 4.30;
 * "last_hess_kernel" 370).  Back at 0 the refusals return in the same words.  Its workspaces and the transposed row tables are allocated when
 * the option is first set to 1 (PCL_ENOMEM when that fails) and freed by pcl_destroy.  "large_var_exp_hess_drives" caps the drives per group of
 * that launch (0 auto; PCL_EINVAL when negative or off such a context), "cols_per_slice" its state columns; no atomics: every split, two
 * launches and both pointer paths give the same bits.  With multipliers that are zero on the variations, the scalars and the vectors of
 * component 0 equal, as numbers, those of a plain PCL_LARGE_N | PCL_LARGE_EXP context with "large_exp_hess" on the same drift and drives.
 * h = 0 gives exact zeros in (u,u) and (u,X').  The other refusals above stay at either value.
 * Options: "cols_per_slice" caps the state columns per chain workgroup, "general_slices" sets the least number of panel workgroups,
 * "large_var_exp_drives" caps the drives per chain workgroup (0 auto; PCL_EINVAL when negative or off such a context); get_option
 * "large_variational_exp" reads 1, "large_variational" 1, "last_kernel" 370 after a residual + Jacobian launch and 371 after a residual-only
 * launch (360 after the rollout).  "jit_compiles" stays 0: the kernel is part of the library. */
#define PCL_LARGE_VAR_EXP 0x800

typedef struct pcl_desc {
    int32_t struct_size; /* = sizeof(pcl_desc) (ABI check) */
    int32_t d;           /* Hilbert-space dimension (sys.levels); n = 2d, x_dim = 2 d^2 */
    int32_t n_drives;    /* m */
    int32_t N;           /* knot points (traj.N); K = N-1 intervals */
    int32_t z_dim;       /* variables per knot (traj.dim) */
    int32_t u_off;       /* 0-based offset of the drive component inside a knot (traj.components[:u][1]-1) */
    int32_t dt_off;      /* 0-based offset of the timestep component */
    int32_t batch;       /* number of members / seeds (>= 1) */
    int32_t batch_mode;  /* PCL_BATCH_MEMBERS, PCL_BATCH_TRAJ, PCL_BATCH_VARIATIONAL or PCL_BATCH_VARIATIONAL_EXP */
    int32_t pade_order;  /* diagonal Pade order p of B^{+-}_p: 2, 4, 6, 8 or 10; 0: the smallest order whose deviation from the reference's
                            exp constraint is below a tolerance -- pcl_set_order_policy, or the first host-pointer call decides;
                            PCL_ORDER_EXP: the exponential constraint itself (see there) */
    int32_t device_id;   /* HIP device ordinal */
    int32_t index_base;  /* 0 (C/Python) or 1 (Julia/MOI) for the emitted structure */
    int32_t per_member_G0; /* 0: one G0 for all members; 1: G0 holds batch matrices (per-member H_drift) */
    int32_t state_cols;  /* columns of the state matrix X (n x state_cols): 0 or d = unitary (Utilde, x_dim = 2 d^2),
                            1 = ket (psitilde = [Re psi; Im psi], x_dim = 2d; KetTrajectory, integrators.jl:58-74);
                            PCL_STATE_VECTOR: the state is a real vector of length d acted on by a general real d x d
                            generator (n = d, odd allowed, d <= 64) -- the compact density vector rhotilde with d = levels^2
                            and the compact Lindbladian generators (DensityTrajectory, integrators.jl:82-95,
                            open_quantum_systems.jl:541-588).  Runs the general-order kernel at every pade_order. */
    int64_t global_dim;  /* traj.global_dim (trailing globals in the variable vector; only shifts nothing, kept for
                            the column count reported by pcl_constraint_dim) */
    const double *G0;      /* n x n column-major (x batch if per_member_G0) : G_drift = iso(-i H_drift) */
    const double *Gj;      /* m matrices n x n column-major                  : G_drives[j] */
    const int32_t *x_offs; /* 0-based state offsets: batch entries (MEMBERS) or 1 entry (TRAJ) */
} pcl_desc;

/* lifecycle ---------------------------------------------------------------- */
int pcl_create(const pcl_desc *desc, pcl_ctx **out);
void pcl_destroy(pcl_ctx *ctx);
/* Message of the last failure on ctx (ctx == NULL: last failure of pcl_create on this thread). */
const char *pcl_last_error(const pcl_ctx *ctx);
const char *pcl_version(void);

/* Order policy.  The reference's constraint is x_{k+1} = exp(dt_k G(u_k)) x_k (docs/src/concepts/index.md:21); the Pade-2q residual deviates from
 * it by kappa_q theta^(2q+1), theta = |dt_k G(u_k)|_2, kappa_q = (q!)^2 / ((2q)! (2q+1)!) (1.6e-5 at order 4, 1.6e-11 at
 * order 8 for BASELINE config 3).  Sets the context's order to the smallest one whose bound at theta = dt_max max_{|u_l| <= u_max[l]} |G_drift + sum_l u_l G_l|_2
 * (the maximum over the box, taken at its 2^m vertices; BASELINE config 3 with |u| <= 0.1, dt <= 0.1: theta = 0.686, order 10 at 1e-10, order 8 at 2e-9)
 * is <= tol and reports it (also: get_option "pade_order").  A context created with pade_order = 0 that never sees this call takes
 * theta = 1.5 x the maximum over the first trajectory a host-pointer entry point is given, tol = 1e-10; its device-pointer entry points
 * return PCL_EINVAL until an order exists. */
int pcl_set_order_policy(pcl_ctx *ctx, double dt_max, const double *u_max /* n_drives */, double tol, int32_t *order_out);
/* The same decision from a trajectory on the HOST (the one the integrator is constructed with -- the reference's constructor,
 * src/control/integrators.jl:35-51, takes it too): theta = 1.5 x max_k |dt_k G(u_k)|_2 over Z_host, tol as set by pcl_set_order_policy
 * (default 1e-10; tol > 0 here overrides).  What a binding calls at construction when the trajectory carries no bounds on u and dt, so that
 * the scalar form B.f, the device-pointer entry points and the host-pointer ones all evaluate ONE order from the first call on.
 * option "order_tol_met" reads 0 (and pcl_last_error carries a note) when even order 10 exceeds the tolerance. */
int pcl_set_order_from_trajectory(pcl_ctx *ctx, const double *Z_host, double tol, int32_t *order_out);
/* The policy itself, without a context or a device: n x n generators (column-major; n = 2 d for unitary and ket problems), n_g0 drifts, m drives.
 * theta_out / order_out / met_out (0: even order 10 exceeds tol) may be NULL. */
int pcl_order_for_bounds(int32_t n, int32_t m, const double *G0, int32_t n_g0, const double *Gj, double dt_max, const double *u_max, double tol,
                         double *theta_out, int32_t *order_out, int32_t *met_out);

/* dimensions --------------------------------------------------------------- */
/* n_rows = batch*x_dim*(N-1); n_cols = z_dim*N*(TRAJ ? batch : 1) + global_dim. Any out pointer may be NULL. */
int pcl_constraint_dim(const pcl_ctx *ctx, int64_t *x_dim, int64_t *n_rows, int64_t *n_cols);
int pcl_jac_nnz(const pcl_ctx *ctx, int64_t *nnz, int64_t *nnz_per_interval);
int pcl_hess_nnz(const pcl_ctx *ctx, int64_t *nnz, int64_t *nnz_per_interval);
/* Sparsity structure in value order. In TRAJ mode trajectory b's variables are offset by b*z_dim*N. */
int pcl_jac_structure(const pcl_ctx *ctx, int32_t *rows, int32_t *cols);
int pcl_jac_structure_i64(const pcl_ctx *ctx, int64_t *rows, int64_t *cols);
int pcl_hess_structure(const pcl_ctx *ctx, int32_t *rows, int32_t *cols);
int pcl_hess_structure_i64(const pcl_ctx *ctx, int64_t *rows, int64_t *cols);

/* host-pointer evaluation (synchronous; includes H2D of Z[,mu] and D2H of the results) ---- */
/* Z: z_dim*N doubles (MEMBERS) or batch*z_dim*N (TRAJ). delta: n_rows. vals: jac nnz. */
int pcl_eval(pcl_ctx *ctx, const double *Z, double *delta);
int pcl_jac(pcl_ctx *ctx, const double *Z, double *vals);
int pcl_eval_jac(pcl_ctx *ctx, const double *Z, double *delta, double *vals);
/* mu: n_rows multipliers; vals: hess nnz. (sigma * objective Hessian is the objective's business.)
 * A PCL_BATCH_VARIATIONAL_EXP context serves pcl_hess[_dev], pcl_hess_nnz and pcl_hess_structure[_i64] only with
 * pcl_set_option(ctx, "var_exp_hess", 1) (0, the default: PCL_ENOTIMPL in the words above): the Hessian of the Lagrangian of the exact lifted
 * constraint, third Frechet derivatives of exp through an octuple chain per (interval, variation, drive).  Values per interval:
 * (m+1)(m+2)/2 + x_dim'*(m+1), x_dim' the stacked state -- the Pade variational layout without its two X'_{k+1} groups, from pcl_hess_structure
 * as always.  Generator dimensions up to n = 44 (nine LDS tiles); beyond, setting the option is PCL_ESHAPE with the byte counts and the
 * context goes on as before.  Two launches give the same bits.  Get "last_hess_kernel" reads 110 after such a launch.
 * pcl_set_option(ctx, "var_exp_hess_tiles", 1) before "var_exp_hess" serves n = 46 .. 62 too: where nine tiles do not fit, four of them
 * (Tab, Tac, Tbc, Tabc) live in a device workspace of K v max(m,1) 4 n^2 doubles, allocated then, and "last_hess_kernel" reads 112; where
 * they fit, nothing changes (110).  2: that plan at every n (the same bits as the LDS plan).  0, the default: as above.  The value is read
 * when "var_exp_hess" is set to 1; another value while that option is 1 is PCL_EINVAL, and so is a non-zero value on any other context. */
int pcl_hess(pcl_ctx *ctx, const double *Z, const double *mu, double *vals);

/* device-pointer evaluation (asynchronous on the context's stream; results stay in HBM) ---- */
/* Launch on the caller's hipStream_t (NULL = HIP's legacy default stream, which is what
 * torch.cuda.current_stream().cuda_stream returns for the default stream). */
int pcl_set_stream(pcl_ctx *ctx, void *hip_stream);
int pcl_reset_stream(pcl_ctx *ctx); /* back to the context's own non-blocking stream (the initial state) */
int pcl_sync(pcl_ctx *ctx);
int pcl_eval_dev(pcl_ctx *ctx, const double *Z_dev, double *delta_dev);
int pcl_eval_jac_dev(pcl_ctx *ctx, const double *Z_dev, double *delta_dev, double *vals_dev);
int pcl_jac_dev(pcl_ctx *ctx, const double *Z_dev, double *vals_dev); /* eval_jacobian alone (integrators.jl:780) */
int pcl_hess_dev(pcl_ctx *ctx, const double *Z_dev, const double *mu_dev, double *vals_dev);

/* Member window: restrict the evaluator entry points (pcl_eval*, pcl_jac*, pcl_hess*, pcl_rollout*, their nnz / structure
 * queries and pcl_constraint_dim's row count) to members / seeds [first, first+count) of the context.  Inputs stay the full
 * buffers (Z of every member; TRAJ mode: of every seed); outputs, multipliers and structure rows are those of the window,
 * numbered from 0.  This is what one member of the reference's Vector{BilinearIntegrator} evaluates
 * (src/control/integrators.jl:134-146: one integrator per ensemble member, rows of each numbered on their own).
 * The objective / merit entry points always cover every member.  Default: all members. */
int pcl_set_member_window(pcl_ctx *ctx, int32_t first, int32_t count);

/* Compact Jacobian: the d diagonal copies of I_d (x) B^{+-} are identical, so per (b,k) only
 * [-B^+ (n*n) | B^- (n*n) | d/du (m*x_dim) | d/ddt (x_dim)] = 2 n^2 + x_dim (m+1) doubles are unique.
 * pcl_eval_jac_compact_dev writes those; pcl_jac_expand_dev replicates them into the full triplet order.
 * A context of the exponential constraint with option "exp_full" = 1 (see PCL_ORDER_EXP): [-E (n*n) | tail (x_dim*(m+1))] = n^2 + x_dim (m+1)
 * doubles per (b,k); the expansion writes cols copies of -E, the x_dim ones of d delta / d X_{k+1}, then the tail.
 * A variational context with option "var_compact" = 1 (either constraint kind; one stacked trajectory, x_dim' = (1 + v) n C), per interval:
 *   PCL_BATCH_VARIATIONAL      [-B^+ | B^- | for i = 1..v: -L^+_i | L^-_i | tails]   (2 + 2v) n^2 + x_dim' (m+1) doubles
 *   PCL_BATCH_VARIATIONAL_EXP  [-E | -L_1 .. -L_v | tails]                           (1 + v) n^2 + x_dim' (m+1) doubles
 * the tails being the x_dim' (m+1) values of the full layout in its order.  The expansion writes every tile to its C copies in every segment
 * where it occurs (-B^+, B^-, -E once per component), the x_dim' ones (exponential) and the tails -- at C = 1 too, where the compact layout
 * still is not the full one.  Expanded values and delta have the bits of pcl_eval_jac_dev.  Without the option: PCL_ENOTIMPL. */
int pcl_jac_compact_nnz(const pcl_ctx *ctx, int64_t *nnz, int64_t *nnz_per_interval);
int pcl_eval_jac_compact_dev(pcl_ctx *ctx, const double *Z_dev, double *delta_dev, double *compact_dev);
int pcl_jac_expand_dev(pcl_ctx *ctx, const double *compact_dev, double *vals_dev);

/* DerivativeIntegrator / time-consistency rows sharing the context's trajectory layout ------
 *   DerivativeIntegrator(x, dx):  x_{k+1} - x_k - dt_k dx_k = 0      src/control/templates/smooth_pulse_problem.jl:267-275
 *   TimeConsistencyConstraint  :  t_{k+1} - t_k - dt_k      = 0      smooth_pulse_problem.jl:277   (pass dx_off = -1)
 * x_off / dx_off: 0-based component offsets inside a knot, dim: component length.  rows = K*dim (x batch in TRAJ mode),
 * row k*dim + r.  Values per interval: [d/dx_k = -1 (dim) | d/dx_{k+1} = +1 (dim) | d/ddx_k = -dt_k (dim; absent when
 * dx_off < 0) | d/ddt_k = -dx_k[r] (dim)]; order reported by pcl_deriv_structure.  In MEMBERS mode the rows are those of
 * the one shared trajectory (not replicated per member). */
int pcl_deriv_nnz(const pcl_ctx *ctx, int32_t dx_off, int32_t dim, int64_t *n_rows, int64_t *nnz);
int pcl_deriv_structure(const pcl_ctx *ctx, int32_t x_off, int32_t dx_off, int32_t dim, int64_t *rows, int64_t *cols);
int pcl_deriv_eval_jac(pcl_ctx *ctx, int32_t x_off, int32_t dx_off, int32_t dim, const double *Z, double *delta, double *vals);
int pcl_deriv_eval_jac_dev(pcl_ctx *ctx, int32_t x_off, int32_t dx_off, int32_t dim, const double *Z_dev, double *delta_dev,
                           double *vals_dev);

/* objective of the unitary problems -------------------------------------------------------------
 *   UnitaryInfidelityObjective: Q * |1 - F(U_N)|,  F = |tr(U_goal' U_N)|^2 / d^2          src/control/objectives.jl:330-337,347-356
 *   ... with an EmbeddedOperator goal: F = (tr(M'M) + |tr M|^2) / (ns (ns+1)),
 *       M = U_goal[sub,sub]' U_N[sub,sub]                                                   src/control/objectives.jl:339-345
 *   SamplingProblem: sum_i (w_i Q) |1 - F_i| + shared regularisers                          src/control/templates/sampling_problem.jl:381-387
 *   QuadraticRegularizer(name, traj, R) x3 [EXT DirectTrajOpt]                              src/control/templates/smooth_pulse_problem.jl:249-251
 * pcl_set_goal copies the goal's iso-vec (x_dim doubles, operator_to_iso_vec(U_goal)); pcl_set_goal_subspace the iso-vec of
 * the ns x ns block unembed(op) (2 ns^2 doubles) and its ns 0-based subspace indices (op.subspace - 1); the later call wins.
 * pcl_set_weights: per member / seed weights w (batch doubles, NULL = ones).  On a variational context (option var_full) w has batch = 1 + v
 * entries: w[0] multiplies the terminal infidelity of the state, w[i] (i = 1..v) is the coefficient of the sensitivity loss of variation i at the
 * terminal knot -- UnitarySensitivityObjective, src/control/objectives.jl:437-453: scale^4 abs2(tr(U'U)) / n^2 = (|x|^2)^2 / d^2 for the iso-vec x,
 * with Qs and scale^4 folded into w[i] by the binding.  NULL = [1, 0, .., 0]: no sensitivity term.  A negative or non-finite entry is PCL_EINVAL;
 * a non-zero w[i >= 1] on a ket context is PCL_ENOTIMPL (the reference has no ket sensitivity objective).
 * pcl_infidelity_dev writes one value per member / seed (value_dev[batch]) and the gradient w.r.t. that member's terminal
 * state (grad_dev[batch*x_dim], iso-vec order); either output may be NULL.
 * Regularisers: J_r = 1/2 sum_k dt_k^p sum_i R_i Z[k, off+i]^2 with p = dt_power in {0, 1, 2}.  DirectTrajOpt is not vendored
 * with the reference and nothing in the reference pins the value; p = 2 (r_k = dt_k v_k, J += r_k' R r_k / 2) is the form of
 * its QuantumCollocation lineage, p = 0 the plain knot-point form -- the binding chooses.
 * pcl_objective[_dev]: the whole objective and its gradient w.r.t. the variable vector.  MEMBERS mode: value[1] = sum over
 * members + regularisers, grad[z_dim*N].  TRAJ mode: value[batch], grad[batch][z_dim*N] (one NLP per seed).  grad may be NULL.
 * Variational context (option var_full): value[1], grad[z_dim*N] of
 *     J = Q w0 |1 - F(X_N)| + sum_i w_i (|Xv_i,N|_F^2)^2 / d^2 + regularisers
 * (no goal: no infidelity term; no goal, no non-zero w_i and no regulariser: PCL_EINVAL), always ONE launch ("last_objective_launches"). */
int pcl_set_goal(pcl_ctx *ctx, const double *goal_iso_vec);
int pcl_set_goal_subspace(pcl_ctx *ctx, const double *goal_sub_iso_vec, const int32_t *subspace, int32_t ns);
int pcl_set_weights(pcl_ctx *ctx, const double *weights);
int pcl_infidelity_dev(pcl_ctx *ctx, const double *Z_dev, double Q, double *value_dev, double *grad_dev);
int pcl_add_regularizer(pcl_ctx *ctx, int32_t off, int32_t dim, const double *R, int32_t dt_power);
int pcl_clear_regularizers(pcl_ctx *ctx);
/* (one launch -- regulariser rows and terminal infidelities as workgroups of one grid -- with a gradient buffer, the members' states one
 *  contiguous run of a row and no regulariser on a state component; two launches otherwise; the same bits; option "objective_launches") */
int pcl_objective_dev(pcl_ctx *ctx, const double *Z_dev, double Q, double *value_dev, double *grad_dev);
int pcl_objective(pcl_ctx *ctx, const double *Z, double Q, double *value, double *grad);

/* Terminal losses of the other state types, and any loss of the shape  Q w |1 - F(x)|,  F(x) = c'x + sum_r (A_r'x)^2 :
 *   KetInfidelityObjective                        F = |<g|psi>|^2                          src/control/objectives.jl:24-60    (2 rows)
 *   CoherentKetInfidelityObjective                F = |sum_i w_i <g_i|psi_i> / sum w|^2    src/control/objectives.jl:96-200   (2 rows, joint)
 *   DensityMatrix[PureState]InfidelityObjective   F = Re tr(rho rho_goal)                  src/control/objectives.jl:387-435  (linear)
 * x = one member's terminal state (scope 0: a term per member / seed with the weights of pcl_set_weights; A is R x x_dim, row-major, c
 * x_dim doubles or NULL) or the terminal states of ALL members of a MEMBERS context in member order (scope 1: one term; A is
 * R x (batch x_dim)).  The host mirror builds A and c from the goals (piccolo.jl_amd/objectives.py).  Replaces a goal set with
 * pcl_set_goal[_subspace]; pcl_objective[_dev] then evaluates it (three small launches). */
int pcl_set_goal_form(pcl_ctx *ctx, int32_t scope, int32_t R, const double *A, const double *c);

/* Hessian of the objective: sigma * grad^2 f, the part of eval_hessian_lagrangian that pcl_hess does not cover (eval_hessian = true,
 * src/control/templates/spline_pulse_problem.jl:96).  Terminal loss (any goal above, pcl_set_goal and pcl_set_goal_subspace included): per
 * term the lower triangle of -s w Q sigma (2 sum_r A_r A_r'), s = sign(1 - F) -- the Gram triangle is formed once per goal, an evaluation
 * is a scaled copy.  Regularisers: d2/dv_i^2 = dt^p R_i, d2/ddt dv_i = p dt^(p-1) R_i v_i, d2/ddt^2 = p (p - 1) / 2 dt^(p-2) sum_i R_i v_i^2.
 * Each entry once as (max index, min index); the order is reported by pcl_objective_hess_structure (index_base as in pcl_desc).
 * Variational context (option var_full): the Gram triangle of component 0, then per variation with w_i != 0 the dense lower triangle over
 * its terminal iso-vec, sigma w_i (4 |x|^2 I + 8 x x') / d^2, then the regularisers' entries.  The structure depends on which w_i are non-zero
 * and on the regularisers: query nnz and structure AFTER pcl_set_weights / pcl_add_regularizer.  Where a regulariser covers a component that has
 * a triangle, its terminal-knot diagonal entries are part of that triangle (each position still once). */
int pcl_objective_hess_nnz(const pcl_ctx *ctx, int64_t *nnz);
int pcl_objective_hess_structure(const pcl_ctx *ctx, int64_t *rows, int64_t *cols);
int pcl_objective_hess_dev(pcl_ctx *ctx, const double *Z_dev, double Q, double sigma, double *vals_dev);
int pcl_objective_hess(pcl_ctx *ctx, const double *Z, double Q, double sigma, double *vals);

/* what a sharded ensemble exchanges: out = [phi | g_u (K x m, interval-major) | g_dt (K)] with
 *   phi = sum_b w_b <lam_b, delta_b>  (lam_dev == NULL: lam = delta and phi = 1/2 sum_b w_b |delta_b|^2, the constraint merit),
 *   g = J^T (w lam) restricted to the SHARED variables u_k, dt_k -- the only part of the Lagrangian gradient to which other
 * ranks' members contribute (member states are rank-private).  MEMBERS mode: one set of pcl_merit_grad_len doubles, to be
 * summed over ranks with pcl_reduce_sum_dev; TRAJ mode: `sets` = batch sets (nothing is shared between seeds). */
int pcl_merit_grad_len(const pcl_ctx *ctx, int64_t *len, int64_t *sets);
int pcl_merit_grad_dev(pcl_ctx *ctx, const double *delta_dev, const double *lam_dev, const double *vals_dev, double *out_dev);
/* (vals_dev == NULL: PCL_EINVAL, except on a context of the exponential constraint with option "exp_full" = 1 -- the payload without the Jacobian.)
 * pcl_eval_jac_dev + pcl_merit_grad_dev in one pass: the fused kernel forms the payload's dot products per state column while the
 * column's vectors are still in LDS (the 1.7 % of the Jacobian values that pcl_merit_grad_dev reads back from HBM are never
 * re-read); delta_dev and vals_dev are written exactly as by pcl_eval_jac_dev.  Launches that do not take fused kernel 3 (other
 * shapes, Pade orders other than 4, a member window) run the two calls one after the other: same outputs, same layout.
 * get_option "last_merit_fused" tells which. */
int pcl_eval_jac_merit_dev(pcl_ctx *ctx, const double *Z_dev, const double *lam_dev, double *delta_dev, double *vals_dev, double *out_dev);
/* pcl_objective_dev + pcl_eval_jac_merit_dev -- everything a rank computes in one step of a sharded ensemble
 * (SamplingProblem: weighted infidelities + regularisers with their gradient, the members' residuals and Jacobian values, the reduce
 * payload) -- in TWO launches instead of four: the fused kernel, then one launch whose workgroups are the regulariser rows, the terminal
 * infidelities and the payload's finish.  Outputs as the two calls write them (value_dev, grad_dev: pcl_objective_dev; the rest:
 * pcl_eval_jac_merit_dev), bit for bit.  Falls back to the two calls where the fused payload does not apply, when grad_dev is NULL, or when a
 * regulariser covers a state component. */
int pcl_eval_jac_merit_objective_dev(pcl_ctx *ctx, const double *Z_dev, const double *lam_dev, double *delta_dev, double *vals_dev, double *out_dev, double Q,
                                     double *value_dev, double *grad_dev);

/* rollout for validation ------------------------------------------------------------------------
 *   unitary_rollout(traj, sys; interpolation = :constant)                       src/quantum/dynamics.jl:631-667
 *   RolloutStates: "a GPU rollout overwrites `states` in place"                 src/quantum/trajectories/ensemble_trajectory.jl:56-71
 * Exact piecewise-constant propagation X_{k+1} = exp(dt_k G(u_k)) X_k from the knot-0 state of every member / trajectory
 * (scaling and squaring, to rounding).  X_out: [batch][N][x_dim] doubles, iso-vec per knot (knot 0 = the input state).
 * Variational context (option var_full): X_out is [N][x_dim] with the stacked x_dim = (1 + v) n C, components in the order of x_offs, propagated
 * exactly under the lifted generator: X <- E X, Xv_i <- E Xv_i + L_i X with E = exp(h G) and L_i the Frechet derivative of exp at h G along
 * h Gv_i (the lifted matrix is never formed); every shape pcl_create accepts.  Component 0 has the bits of a plain context's rollout. */
int pcl_rollout(pcl_ctx *ctx, const double *Z, double *X_out);
int pcl_rollout_dev(pcl_ctx *ctx, const double *Z_dev, double *X_out_dev);

/* multi-GPU: the one exchange of the path ------------------------------------------------------
 * One context per GPU/process.  Rank 0 obtains an id, ships the 128 bytes to the other ranks by any means (MPI,
 * sockets, a file), every rank calls pcl_comm_init; pcl_reduce_sum_dev is an in-place RCCL all-reduce(sum, f64) over
 * xGMI on the context's stream -- used for [merit | d/du | d/ddt] of the shared controls (~5.6 KB: latency-bound).
 * librccl is opened lazily (dlopen); single-GPU users never load it. */
typedef struct pcl_comm_id { char bytes[128]; } pcl_comm_id;
int pcl_comm_get_unique_id(pcl_comm_id *out);
int pcl_comm_init(pcl_ctx *ctx, const pcl_comm_id *id, int32_t rank, int32_t nranks);
int pcl_reduce_sum_dev(pcl_ctx *ctx, double *buf_dev, int64_t n);
int pcl_reduce_sum(pcl_ctx *ctx, double *buf_host, int64_t n); /* same for a host buffer (staged; returns after the sum) */
int pcl_comm_destroy(pcl_ctx *ctx);

/* options --------------------------------------------------------------------
 * A DEPLOYMENT sets none, or only these (everything else is a measurement / test switch, listed with its meaning in OPTIONS.md; every
 * setting gives the same results up to the order of additions inside a kernel family, and inside a family every work split is bitwise
 * equal -- which is what the parity tests use the switches for):
 *   "jit"           1 (default): the pattern-compiled kernels are taken from csrc/prebuilt, from the on-disk cache, or compiled with hiprtc on
 *                   first use; 0: built-in kernel families only
 *   "require_jit"   1: a pattern-compiled kernel that is wanted and cannot be had is PCL_EHIP instead of a (noted, counted) fallback
 *   "host_threads"  threads that expand the compact values into the caller's array in the host-pointer entry points (0 = min(cores / 2, 32);
 *                   -1 = a sweep over the context's first twelve calls), "host_path" (0 auto | 1 full values over PCIe | 2 compact + host expansion)
 *   "v4_ticket"     launches of several trajectories: -1 auto | 0 static split | 1 groups of workgroups + slice tickets
 *   "exp_full"      contexts of the exponential constraint only (1 on any other context: PCL_EINVAL): 1 serves the compact Jacobian trio, the compact
 *                   host-pointer path and the merit / reduce entry points (see PCL_ORDER_EXP); 0 (default) refuses them
 *   "var_compact"   variational contexts only, either constraint kind (1 on any other context: PCL_EINVAL): 1 serves the compact Jacobian trio and
 *                   the compact host-pointer path (see pcl_jac_compact_nnz); 0 (default) refuses them.  Independent of "var_full" / "var_exp_hess"
 *   "var_full"      variational contexts only (1 on any other context: PCL_EINVAL): 1 serves the objective entry points and the rollout
 *                   (see PCL_BATCH_VARIATIONAL); 0 (default) refuses them and drops goal, weights and regularisers
 * and reads: "pade_order" (the order in use), "last_kernel" / "last_hess_kernel" (which kernel family ran), "jit_compiles", "jit_cache_hits",
 * "jit_fallbacks", "n_cu".  Unknown keys return PCL_EINVAL.  Environment: PCL_JIT_CACHE=0, PCL_JIT_CACHE_DIR, PCL_HOST_PATH, PCL_V4_TICKET,
 * PCL_VERBOSE (see OPTIONS.md). */
int pcl_set_option(pcl_ctx *ctx, const char *key, int64_t value);
int pcl_get_option(const pcl_ctx *ctx, const char *key, int64_t *value);

/* Inspection hook (needs no device): the HIP source the library generates and compiles on first use for the
 * pattern-compiled kernels of a system with Hilbert dimension d <= 32 and m <= 6 drives whose generators are exact iso(.)
 * images (G0: n*n column-major, Gj: m such blocks).  *needed = bytes including the terminator; buf may be NULL. */
int pcl_codegen_source(int d, int m, const double *G0, const double *Gj, char *buf, int64_t cap, int64_t *needed);
/* The same for the pattern-compiled FUSED residual + Jacobian kernel (kernel_version 4) at diagonal Pade order 2q, q = 1..5
 * (n_g0 drifts G0[b] span the union pattern: an ensemble's members); PCL_ESHAPE when the drives need more resident
 * coefficients than the kernel keeps. */
int pcl_codegen_source_v4(int d, int m, const double *G0, int n_g0, const double *Gj, int q, int what /* 0 fused residual + Jacobian (+ residual only), 1 Hessian of the Lagrangian (one wave per chain), 5 ... (one wave per group of state columns) */,
                          char *buf, int64_t cap, int64_t *needed);
/* Compile the pattern-compiled module(s) a context of this system would compile on first use and leave the code object under its content
 * hash in out_dir (NULL: <library directory>/prebuilt, which every context looks at before the user's cache and before hiprtc).  Needs
 * libhiprtc, no device.  what: 0 fused residual + Jacobian (+ residual only) at order 2q | 1 general-order Hessian, one workgroup per
 * interval | 2 ... two workgroups per interval | 3 the order-4 Hessian / value-table module (q ignored) | 4 the fused module with the
 * slice-ticket roles (launches of several trajectories) | 5 general-order Hessian, one wave per group of state columns (`auto` at every
 * order but 4) | 7 the fused module of the launches with one item per workgroup (one trajectory per launch; option v4_one_item).  (6, the
 * resident evaluator's module, in lab builds only: piccolo_hip_lab.h.) */
int pcl_jit_prebuild(int d, int m, const double *G0, int n_g0, const double *Gj, int q, int what, const char *out_dir);

#ifdef __cplusplus
}
#endif
#endif /* PICCOLO_HIP_H */
