# HipPadeIntegrator.jl -- Julia-side glue of the drop-in: `DirectTrajOpt.AbstractIntegrator`s whose arithmetic runs in
# libpiccolo_hip.so (HIP kernels on an MI355X) through `ccall`.
#
# STATUS: written against the interface Piccolo.jl v2.0.2 *uses* (call sites cited below).  The abstract type and the
# generic functions live in the un-vendored DirectTrajOpt.jl (compat 0.9.5 / 0.10) and there is no Julia in the build
# container, so this file has NOT been executed.  `selftest.jl` (next to this file) is the script a maintainer runs first:
# it checks this glue against DirectTrajOpt's own `test_integrator` and against `BilinearIntegrator`, and lists the
# DirectTrajOpt generics the glue bound itself to at load time (`HipPade.BOUND_GENERICS`, section "adaptive binding" below).  All arithmetic is in the C
# library (include/piccolo_hip.h); this file only marshals arguments.  See INTEGRATION.md.
#
#   plug-in points in the reference:
#     SmoothPulseProblem(qtraj, N; integrator = HipPadeIntegrator(qtraj, N))
#         src/control/templates/smooth_pulse_problem.jl:123,213-233
#     SamplingProblem(qcp, systems; integrator = (sq, N) -> HipPadeIntegrator(sq, N))     # returns a Vector, one per member
#         src/control/templates/sampling_problem.jl:190-237,292
#     Specs.register_integrator!(:hip_pade, RegistryEntry(factory = (qtraj, N; alg) -> HipPadeIntegrator(qtraj, N)))
#         src/specs/registries.jl:82-86,112,119 ; src/specs/materialize.jl:216-222
module HipPade

using LinearAlgebra, SparseArrays
using NamedTrajectories
using DirectTrajOpt
import DirectTrajOpt: AbstractIntegrator
using Piccolo: get_system, state_name, state_names, drive_name, sampling_member_states,
               UnitaryTrajectory, KetTrajectory, MultiKetTrajectory, DensityTrajectory, MultiDensityTrajectory, SamplingTrajectory,
               compact_lindbladian_generators

const LIB = get(ENV, "PICCOLO_HIP_LIB", "libpiccolo_hip.so")

# mirror of `pcl_desc` (include/piccolo_hip.h) -- field order and widths must match
struct PclDesc
    struct_size::Int32; d::Int32; n_drives::Int32; N::Int32; z_dim::Int32
    u_off::Int32; dt_off::Int32; batch::Int32; batch_mode::Int32; pade_order::Int32
    device_id::Int32; index_base::Int32; per_member_G0::Int32; state_cols::Int32
    global_dim::Int64
    G0::Ptr{Float64}; Gj::Ptr{Float64}; x_offs::Ptr{Int32}
end

_lasterr(ctx) = unsafe_string(ccall((:pcl_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))
check(ctx, rc) = rc == 0 || error("libpiccolo_hip: ", _lasterr(ctx), " (code $rc)")

# One `pcl_ctx` (one GPU, one stream).  A SamplingTrajectory's M member integrators share ONE batched context: the first
# member asked about a trajectory launches the fused kernels for ALL members, the others slice their rows out of the
# cached result (the cache key is the trajectory buffer itself, compared by value, so a stale result is never served).
mutable struct PclCore
    ctx::Ptr{Cvoid}
    n_members::Int
    x_dim::Int                      # per member
    rows_per::Int                   # x_dim * (N-1)
    jac_per::Int                    # Jacobian values per member
    hess_per::Int
    z::Vector{Float64}              # trajectory buffer the cached results belong to
    δ::Vector{Float64}              # all members, member-major
    vals::Vector{Float64}
    have_δ::Bool
    have_vals::Bool
    launches::Int
end

function _destroy!(c::PclCore)
    c.ctx == C_NULL || ccall((:pcl_destroy, LIB), Cvoid, (Ptr{Cvoid},), c.ctx)
    c.ctx = C_NULL
    return nothing
end

mutable struct HipPadeIntegrator <: AbstractIntegrator
    core::PclCore
    member::Int               # 1-based member of the core's ensemble (1 for a single-state integrator)
    x_name::Symbol
    x_names::Vector{Symbol}
    u_name::Symbol
    x_dim::Int
    dim::Int                  # == x_dim * (N - 1)                                    [REF integrators.jl:307-309]
    jac_rows::Vector{Int32}   # 1-based, in value order, numbered inside this integrator's block (never assumed, always queried)
    jac_cols::Vector{Int32}
    hess_rows::Vector{Int32}
    hess_cols::Vector{Int32}
    n_vars::Int
    G0::Matrix{Float64}       # this member's generators (for `f`)
    Gj::Vector{Matrix{Float64}}
    state_cols::Int
    pade_order::Int
    fcore::Union{Nothing,PclCore}   # lazily created 2-knot context behind `B.f`
end

function _create_core(G0s::Vector{Matrix{Float64}}, Gjs::Vector{Matrix{Float64}}, N::Int, z_dim::Int, u_off::Int, dt_off::Int,
                      x_offs::Vector{Int32}, global_dim::Int; device::Integer = 0, pade_order::Integer = 4, state_cols::Integer = 0,
                      exp_hessian::Bool = false, exp_full::Bool = false, large_generator::Bool = false,
                      large_hessian::Bool = false, large_full::Bool = false, large_reduce::Bool = false, large_exp::Bool = false,
                      large_exp_hessian::Bool = false, large_exp_reduce::Bool = false)
    # large_exp_reduce = true (with large_exp = true only): the library's option large_exp_reduce -- pcl_jac_compact_nnz, pcl_eval_jac_compact_dev,
    # pcl_jac_expand_dev, pcl_merit_grad_len, pcl_merit_grad_dev, pcl_eval_jac_merit_dev and the host-pointer calls' compact route are served on the
    # exponential constraint at generator dimensions 66 .. 128 (compact layout [-E | tails] per interval).  At n <= 64 it sets nothing (exp_full is
    # that context's switch).  Never set on its own.
    (large_exp_reduce && !large_exp) &&
        throw(ArgumentError("HipPadeIntegrator: large_exp_reduce = true is the compact Jacobian and the reduce payload of a context created with large_exp = true (large_generator = true, pade_order = :exp): it needs that keyword"))
    # large_exp_hessian = true (with large_exp = true only, hence large_generator = true and pade_order = :exp): the library's option large_exp_hess --
    # the Hessian of the Lagrangian of the exponential constraint at generator dimensions 66 .. 128 (hess_per > 0, eval_hessian = true works).  At
    # n <= 64 it sets nothing (exp_hessian is that context's switch).  Never set on its own.
    (large_exp_hessian && !large_exp) &&
        throw(ArgumentError("HipPadeIntegrator: large_exp_hessian = true is the Hessian of the Lagrangian of a context created with large_exp = true (large_generator = true, pade_order = :exp): it needs that keyword"))
    # large_exp = true (with large_generator = true and pade_order = :exp only): the library's second flag PCL_LARGE_EXP in batch_mode -- the
    # exponential constraint at generator dimensions 66 .. 128, residual and exact Jacobian (hess_per = 0: solve with eval_hessian = false).
    # large_full = true is allowed beside it; the other large options and the exponential ones are refused by the library.  Never set on its own.
    (large_exp && !large_generator) &&
        throw(ArgumentError("HipPadeIntegrator: large_exp = true is the exponential constraint of a context created with large_generator = true: it needs that keyword"))
    (large_exp && pade_order != PCL_ORDER_EXP) &&
        throw(ArgumentError("HipPadeIntegrator: large_exp = true is the exponential constraint at generator dimensions 66 .. 128: it needs pade_order = :exp"))
    # large_reduce = true (the same conditions): the library's option large_reduce -- pcl_jac_compact_nnz, pcl_eval_jac_compact_dev, pcl_jac_expand_dev,
    # the host-pointer calls' compact route and the merit / reduce entry points are served at those dimensions too.  Independent of the other two.
    (large_reduce && !large_generator) &&
        throw(ArgumentError("HipPadeIntegrator: large_reduce = true is the compact Jacobian and the reduce payload of a context created with large_generator = true: it needs that keyword"))
    (large_reduce && pade_order == PCL_ORDER_EXP) &&
        throw(ArgumentError("HipPadeIntegrator: large_reduce = true serves the diagonal Pade orders 2 .. 10: pade_order = :exp has no large contexts"))
    # large_full = true (the same conditions): the library's option large_full -- goals, weights, regularisers, pcl_objective*, pcl_objective_hess*
    # and pcl_rollout* are served at those dimensions too.  Independent of large_hessian; at n <= 64 the ordinary context serves them as always.
    (large_full && !large_generator) &&
        throw(ArgumentError("HipPadeIntegrator: large_full = true is the objective and the rollout of a context created with large_generator = true: it needs that keyword"))
    (large_full && pade_order == PCL_ORDER_EXP && !large_exp) &&
        throw(ArgumentError("HipPadeIntegrator: large_full = true serves the diagonal Pade orders 2 .. 10: pade_order = :exp has no large contexts"))
    # large_hessian = true (with large_generator = true on the Pade constraint only): the library's option large_hess -- the Hessian of the
    # Lagrangian at those dimensions too (hess_per > 0, eval_hessian = true works).  At n <= 64 the ordinary context serves its Hessian as always.
    (large_hessian && !large_generator) &&
        throw(ArgumentError("HipPadeIntegrator: large_hessian = true is the Hessian of the Lagrangian of a context created with large_generator = true: it needs that keyword"))
    (large_hessian && pade_order == PCL_ORDER_EXP) &&
        throw(ArgumentError("HipPadeIntegrator: large_hessian = true serves the diagonal Pade orders 2 .. 10: pade_order = :exp has no large contexts"))
    # large_generator = true: the library's flag PCL_LARGE_N in batch_mode -- generator dimensions 66 .. 128 on the Pade constraint, residual and
    # Jacobian only (no Hessian of the Lagrangian: hess_per = 0, solve with eval_hessian = false).  Never set on its own; at n <= 64 it changes nothing.
    # state_cols: 0 unitary (n = 2d), 1 ket, -1 = PCL_STATE_VECTOR (general n x n generator on one real column, d := n)
    (exp_full && pade_order != PCL_ORDER_EXP) &&
        throw(ArgumentError("HipPadeIntegrator: exp_full = true serves the compact Jacobian and the merit / reduce payload of the exponential constraint: it needs pade_order = :exp"))
    (exp_hessian && pade_order != PCL_ORDER_EXP) &&
        throw(ArgumentError("HipPadeIntegrator: exp_hessian = true is the Hessian of the Lagrangian of the exponential constraint: it needs pade_order = :exp"))
    n = size(G0s[1], 1); d = state_cols == -1 ? n : n ÷ 2; m = length(Gjs)
    large = large_generator && n > 64
    G0 = reduce(vcat, [vec(G) for G in G0s])                       # column-major, one block per member
    Gj = m == 0 ? zeros(1) : reduce(vcat, [vec(G) for G in Gjs])
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve G0 Gj x_offs begin
        desc = PclDesc(sizeof(PclDesc), d, m, N, z_dim, u_off, dt_off,
                       length(x_offs), (large_generator ? PCL_LARGE_N : 0) | (large_exp ? PCL_LARGE_EXP : 0) #= PCL_BATCH_MEMBERS [| PCL_LARGE_N [| PCL_LARGE_EXP]] =#, pade_order #= 2, 4, 6, 8 or 10 =#, device, 1 #= 1-based =#,
                       length(G0s) > 1 ? 1 : 0, state_cols, global_dim,
                       pointer(G0), pointer(Gj), pointer(x_offs))
        rc = ccall((:pcl_create, LIB), Cint, (Ref{PclDesc}, Ref{Ptr{Cvoid}}), desc, ctx)
        rc == 0 || error("pcl_create: ", _lasterr(C_NULL))
    end
    c = ctx[]
    xd = Ref{Int64}(0); nr = Ref{Int64}(0); ncol = Ref{Int64}(0); nnz = Ref{Int64}(0); per = Ref{Int64}(0)
    check(c, ccall((:pcl_constraint_dim, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}), c, xd, nr, ncol))
    M = length(x_offs)
    check(c, ccall((:pcl_jac_nnz, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), c, nnz, per))
    jac_per = Int(nnz[]) ÷ M
    # (PCL_ORDER_EXP: no Hessian of the Lagrangian -- hess_per = 0, the structure is empty, pcl_hess is refused by the library -- unless
    #  exp_hessian switches the library's option exp_hess on, BEFORE the Hessian structure is queried; generator dimensions up to 62)
    exp_hessian && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "exp_hess", 1))
    # (exp_full: the library's option of that name -- the host-pointer calls below then move the compact values over PCIe and expand on the host)
    exp_full && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "exp_full", 1))
    (large && large_hessian) && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "large_hess", 1))
    (large && large_exp && large_exp_hessian) && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "large_exp_hess", 1))
    (large && large_full) && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "large_full", 1))
    (large && large_reduce) && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "large_reduce", 1))
    (large && large_exp && large_exp_reduce) && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "large_exp_reduce", 1))
    served = large ? (large_exp ? large_exp_hessian : large_hessian) : (pade_order != PCL_ORDER_EXP || exp_hessian)
    !served ? (nnz[] = 0) : check(c, ccall((:pcl_hess_nnz, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), c, nnz, per))
    core = PclCore(c, M, Int(xd[]), Int(nr[]) ÷ M, jac_per, Int(nnz[]) ÷ M, Float64[], Float64[], Float64[], false, false, 0)
    finalizer(_destroy!, core)
    return core, Int(ncol[])
end

_window!(core::PclCore, first0::Integer, count::Integer) =
    check(core.ctx, ccall((:pcl_set_member_window, LIB), Cint, (Ptr{Cvoid}, Int32, Int32), core.ctx, first0, count))

# structure of ONE member (rows numbered inside the member's block, columns = global variable indices), 1-based
function _member_structure(core::PclCore, member::Int)
    _window!(core, member - 1, 1)
    jr = Vector{Int32}(undef, core.jac_per); jc = similar(jr)
    check(core.ctx, ccall((:pcl_jac_structure, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}), core.ctx, jr, jc))
    hr = Vector{Int32}(undef, core.hess_per); hc = similar(hr)
    core.hess_per > 0 && check(core.ctx, ccall((:pcl_hess_structure, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}), core.ctx, hr, hc))
    _window!(core, 0, core.n_members)
    return jr, jc, hr, hc
end

function _generators(sys)
    sys.time_dependent && error("HipPadeIntegrator: time-dependent systems use TimeDependentBilinearIntegrator")
    m = sys.n_drives
    e(j) = (u = zeros(m); u[j] = 1.0; u)
    G0 = Matrix{Float64}(sys.G(zeros(m), 0.0))
    Gj = [Matrix{Float64}(sys.G(e(j), 0.0)) - G0 for j in 1:m]      # linear drives: G(u) = G0 + sum u_j G_j
    return G0, Gj
end

# The order in use, asked of the context (never a cached copy of a constructor argument): 0 = not decided yet.
function _order_in_use(core::PclCore)
    v = Ref{Int64}(0)
    check(core.ctx, ccall((:pcl_get_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Ref{Int64}), core.ctx, "pade_order", v))
    return Int(v[])
end

# pade_order = 0 (the default): pcl_set_order_policy with dt_max and |u|_max from traj.bounds when both bounds exist, else
# pcl_set_order_from_trajectory on the trajectory the integrator is constructed with (theta = 1.5 max_k |dt_k G(u_k)|).  Either way the
# order is decided HERE, so B.f, evaluate! and eval_jacobian evaluate one and the same constraint from the first call on.
function _decide_order!(core::PclCore, traj::NamedTrajectory, u_name::Symbol, m::Int, tol::Float64)
    order = _order_from_bounds!(core, traj, u_name, m, tol)
    order != 0 && return order
    Z = Vector{Float64}(traj.datavec)
    out = Ref{Int32}(0)
    GC.@preserve Z check(core.ctx, ccall((:pcl_set_order_from_trajectory, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Float64, Ref{Int32}),
                                         core.ctx, Z, tol, out))
    return Int(out[])
end

function _order_from_bounds!(core::PclCore, traj::NamedTrajectory, u_name::Symbol, m::Int, tol::Float64)
    (m > 0 && haskey(traj.bounds, u_name) && haskey(traj.bounds, traj.timestep)) || return 0
    ub = traj.bounds[u_name]; tb = traj.bounds[traj.timestep]
    umax = Float64[max(abs(ub[1][j]), abs(ub[2][j])) for j in 1:m]
    dtmax = Float64(maximum(abs, vcat(collect(tb[1]), collect(tb[2]))))
    order = Ref{Int32}(0)
    GC.@preserve umax check(core.ctx, ccall((:pcl_set_order_policy, LIB), Cint, (Ptr{Cvoid}, Float64, Ptr{Float64}, Float64, Ref{Int32}),
                                           core.ctx, dtmax, umax, tol, order))
    return Int(order[])
end

# pade_order = :exp (or PCL_ORDER_EXP = -1): the exponential constraint itself, x_{k+1} - exp(dt_k G(u_k)) x_k -- for steps too large for
# order 10; residual and Jacobian only (solve with eval_hessian = false, the reference's default).  Never chosen on its own.
# exp_hessian = true (with pade_order = :exp only): the Hessian of the Lagrangian of that constraint too (the library's option exp_hess:
# second Frechet derivatives of exp on the device), so the reference's templates can run with eval_hessian = true.
# exp_full = true (with pade_order = :exp only): the library's option exp_full -- pcl_eval_jac / pcl_jac deliver the Jacobian values through
# the compact path (one -E per interval over PCIe, replicated by the host's threads) with the bits of the full path, and the compact /
# merit entry points are served.  This glue has not been executed (there is no Julia on the build or test machines), as the rest of this file.
const PCL_ORDER_EXP = -1
const PCL_LARGE_N = 256     # (0x100) pcl_desc.batch_mode flag (keyword large_generator): generator dimensions 66 .. 128: residual and Jacobian, the Hessian of the Lagrangian with large_hessian = true, objective and rollout with large_full = true, compact Jacobian and reduce payload with large_reduce = true
const PCL_LARGE_VAR_EXP = 2048  # (0x800) a fourth batch_mode flag (keyword large_var_exp of the variational integrators, beside large_generator and pade_order = :exp): PCL_BATCH_VARIATIONAL_EXP at generator dimensions 66 .. 128: residual and Jacobian, objective and rollout with large_var_full = true
const PCL_LARGE_VAR = 1024  # (0x400) a third batch_mode flag beside PCL_LARGE_N (keyword large_generator of the variational integrators): PCL_BATCH_VARIATIONAL on the Pade constraint at generator dimensions 66 .. 128: residual and Jacobian, objective and rollout of the stacked state with large_var_full = true
const PCL_LARGE_EXP = 512   # (0x200) a second batch_mode flag beside PCL_LARGE_N (keyword large_exp, with pade_order = :exp): the exponential constraint at generator dimensions 66 .. 128: residual and Jacobian, objective and rollout with large_full = true, the Hessian of the Lagrangian with large_exp_hessian = true, compact Jacobian and reduce payload with large_exp_reduce = true
_order_code(p::Integer) = Int(p)
_order_code(p::Symbol) = p === :exp ? PCL_ORDER_EXP : error("HipPadeIntegrator: pade_order = :$p (a diagonal Pade order, 0 or :exp)")

function _integrators(G0s, Gj, traj::NamedTrajectory, names::Vector{Symbol}, u_name::Symbol;
                      state_cols::Integer = 0, pade_order::Union{Integer, Symbol} = 0, order_tol::Float64 = 1e-10, kwargs...)
    pade_order = _order_code(pade_order)
    x_offs = Int32[traj.components[nm][1] - 1 for nm in names]
    core, n_vars = _create_core(G0s, Gj, traj.N, traj.dim, traj.components[u_name][1] - 1,
                                traj.components[traj.timestep][1] - 1, x_offs, traj.global_dim;
                                state_cols = state_cols, pade_order = pade_order, kwargs...)
    # pade_order = 0 (default): the smallest order that matches the reference's exp constraint [REF docs/src/concepts/index.md:21] to
    # order_tol over the trajectory's bounds (else over the trajectory itself); 2 ... 10 pins the order (BASELINE's metric is quoted on 4)
    pade_order == 0 && _decide_order!(core, traj, u_name, length(Gj), order_tol)
    pade_order = _order_in_use(core)   # read back: the struct never holds a stale 0
    pade_order == 0 && error("HipPadeIntegrator: the Pade order could not be decided")
    Bs = HipPadeIntegrator[]
    for (i, nm) in enumerate(names)
        jr, jc, hr, hc = _member_structure(core, i)
        push!(Bs, HipPadeIntegrator(core, i, nm, [nm], u_name, core.x_dim, core.rows_per, jr, jc, hr, hc, n_vars,
                                    G0s[length(G0s) > 1 ? i : 1], Gj, state_cols, pade_order, nothing))
    end
    return Bs
end

# BilinearIntegrator(qtraj::UnitaryTrajectory, N)                              [REF src/control/integrators.jl:35-51]
function HipPadeIntegrator(qtraj::UnitaryTrajectory, N::Int; kwargs...)
    G0, Gj = _generators(get_system(qtraj))
    return only(_integrators([G0], Gj, NamedTrajectory(qtraj, N), [state_name(qtraj)], drive_name(qtraj); kwargs...))
end

# BilinearIntegrator(qtraj::KetTrajectory, N) [REF integrators.jl:58-74]
function HipPadeIntegrator(qtraj::KetTrajectory, N::Int; kwargs...)
    G0, Gj = _generators(get_system(qtraj))
    return only(_integrators([G0], Gj, NamedTrajectory(qtraj, N), [state_name(qtraj)], drive_name(qtraj); state_cols = 1, kwargs...))
end

# BilinearIntegrator(qtraj::MultiKetTrajectory, N) -> Vector, one per ket, all under the same system [REF integrators.jl:103-117]
function HipPadeIntegrator(qtraj::MultiKetTrajectory, N::Int; kwargs...)
    G0, Gj = _generators(get_system(qtraj))
    return _integrators([G0], Gj, NamedTrajectory(qtraj, N), collect(state_names(qtraj)), drive_name(qtraj); state_cols = 1, kwargs...)
end

# BilinearIntegrator(qtraj::DensityTrajectory, N) [REF integrators.jl:82-95]: compact Lindbladian generators, linear
# drives and constant dissipation rates (compact_lindbladian_generators folds the dissipators into the drift)
function HipPadeIntegrator(qtraj::DensityTrajectory, N::Int; kwargs...)
    Gc_drift, Gc_drives = compact_lindbladian_generators(get_system(qtraj))
    return only(_integrators([Matrix{Float64}(Gc_drift)], [Matrix{Float64}(G) for G in Gc_drives], NamedTrajectory(qtraj, N),
                             [state_name(qtraj)], drive_name(qtraj); state_cols = -1, kwargs...))
end

# BilinearIntegrator(qtraj::SamplingTrajectory, N) -> Vector{<:AbstractIntegrator}, ONE PER MEMBER, in member order
# [REF integrators.jl:134-146]; SamplingProblem rejects anything else [REF sampling_problem.jl:195-223].
# Members that share the drive generators (perturbed drifts: the robust-control use) evaluate through one batched
# context; members whose drive generators differ too (each member uses its full sys.G, [REF integrators.jl:149-162])
# get a context each.
function HipPadeIntegrator(qtraj::SamplingTrajectory, N::Int; kwargs...)
    # Every base the reference samples [REF src/control/integrators.jl:149-226 (_sampling_integrator)]:
    #   Unitary / Ket       one state per member                     -> one integrator per member
    #   MultiKet            a Vector of ket names per member         -> one integrator per ket, all on the member's system
    #   Density             compact Lindbladian of the member        -> one integrator per member (state vector of length levels^2)
    #   MultiDensity        a Vector of density names per member     -> one integrator per density sub-state
    # The result is flat, member-major, sub-states in order: the reference's `reduce(vcat, ...)`.
    base = qtraj.base_trajectory
    dens = base isa DensityTrajectory || base isa MultiDensityTrajectory
    base isa UnitaryTrajectory || base isa KetTrajectory || base isa MultiKetTrajectory || dens ||
        error("HipPadeIntegrator(::SamplingTrajectory): unsupported base trajectory $(typeof(base))")
    sc = base isa UnitaryTrajectory ? 0 : (dens ? -1 : 1)
    traj = NamedTrajectory(qtraj, N)
    u = drive_name(qtraj)
    per = [s isa AbstractVector ? collect(Symbol, s) : Symbol[s] for s in sampling_member_states(qtraj)]   # sub-state names per member
    gens = dens ? [begin
                       Gd, Gs = compact_lindbladian_generators(sys)
                       (Matrix{Float64}(Gd), [Matrix{Float64}(G) for G in Gs])
                   end for sys in qtraj.systems] : [_generators(sys) for sys in qtraj.systems]
    flat = reduce(vcat, per)
    owner = reduce(vcat, [fill(i, length(p)) for (i, p) in enumerate(per)])
    if all(g -> g[2] == gens[1][2], gens)       # exact equality: the same drive generators in every member -> ONE batched context
        return _integrators([gens[i][1] for i in owner], gens[1][2], traj, flat, u; state_cols = sc, kwargs...)
    end
    # members that differ in their drive generators too: a context per member, shared by the member's sub-states
    return reduce(vcat, [_integrators(fill(gens[i][1], length(per[i])), gens[i][2], traj, per[i], u; state_cols = sc, kwargs...) for i in eachindex(per)])
end

# ---- cached fused evaluation -------------------------------------------------------------------------------------
# ---- variational (sensitivity) integrators: batch_mode PCL_BATCH_VARIATIONAL (= 2) -- ONE context over the stacked state
#      vcat(x, x_var_1, ...), generator var_G(G(u), [G_var_i / scale_i]); rows knot-major over the stacked state (B.dim = x_dim (N - 1)).
#      The member window does not exist for this mode: the structure is queried whole.
#      pade_order = :exp (or PCL_ORDER_EXP = -1): batch_mode PCL_BATCH_VARIATIONAL_EXP (= 3), the reference's own constraint
#      x'_{k+1} = exp(dt_k var_G(..)) x'_k on the stacked state -- residual, Jacobian, objective and rollout; no Hessian of the Lagrangian
#      (third Frechet derivatives: the structure stays empty, solve with eval_hessian = false) unless exp_hessian = true (with
#      pade_order = :exp only) switches the library's option var_exp_hess on BEFORE the Hessian structure is queried -- generator
#      dimensions up to 44; never on by itself.  exp_hessian = :workspace sets the option var_exp_hess_tiles = 1 first: where nine LDS tiles do
#      not fit (generator dimensions 46 .. 62, config 3 among them) four of them live in a device workspace.  Any other value: ArgumentError.
#      var_compact = true (any order, or :exp): the library's option var_compact -- pcl_eval_jac / pcl_jac then deliver the Jacobian values
#      through the compact ones (every distinct tile once over PCIe, replicated by the host's threads) where the blocks are replicated;
#      off by default, never on by itself.
#      large_generator = true: the library's flags PCL_LARGE_N | PCL_LARGE_VAR in batch_mode -- generator dimensions 66 .. 128 on the Pade
#      constraint: residual and Jacobian; no Hessian of the Lagrangian unless large_var_hessian = true (the structure stays empty, solve with eval_hessian = false), no
#      objective or rollout from the library unless large_var_full = true.  With pade_order = :exp: ArgumentError.  At 64 and below it
#      changes nothing; never on by itself.
#      large_var_full = true (with large_generator = true on the Pade constraint only): the library's option large_var_full -- the
#      robust-control objective family and the rollout of the stacked state at generator dimensions 66 .. 128; _enable_var_full! then does
#      nothing there (without the keyword it raises the library's message naming PCL_LARGE_VAR, as before).  At 64 and below it sets nothing.
#      large_var_hessian = true (with large_generator = true on the Pade constraint only): the library's option large_var_hess -- the Hessian
#      of the Lagrangian at generator dimensions 66 .. 128, with the values, order and structure of the variational context at 64 and below
#      (the structure is then filled as there).  At 64 and below it sets nothing (that context serves its Hessian always).
#      (These keywords' glue has not been executed: no Julia on the development machines.)
#      large_var_exp = true (with large_generator = true and pade_order = :exp only): the library's fourth flag PCL_LARGE_VAR_EXP -- the exact
#      exponential constraint on the lifted generator at generator dimensions 66 .. 128: residual and Jacobian with the value order of
#      pade_order = :exp at 62 and below; large_var_full = true is allowed beside it, exp_hessian, var_compact and large_var_hessian are not
#      (ArgumentError).  At 64 and below the ordinary variational exponential context serves.  (Glue not executed, as the rest.)
#      large_var_exp_hessian = true (with large_var_exp = true only): the library's option large_var_exp_hess -- the Hessian of the Lagrangian of
#      that constraint at generator dimensions 66 .. 128, with the values, order and structure of pade_order = :exp with exp_hessian = true at
#      62 and below (the structure is then filled as there).  At 64 and below it sets nothing (exp_hessian is that context's switch); never on
#      by itself.  (Glue not executed, as the rest.)
function _variational(sys, traj::NamedTrajectory, x::Symbol, x_vars::AbstractVector{Symbol}, u::Symbol, scales::Vector{Float64}, state_cols::Int;
                      device::Integer = 0, pade_order::Union{Integer, Symbol} = 0, order_tol::Float64 = 1e-10, exp_hessian::Union{Bool, Symbol} = false,
                      var_compact::Bool = false, large_generator::Bool = false, large_hessian::Bool = false, large_full::Bool = false, large_reduce::Bool = false,
                      large_exp::Bool = false, large_exp_hessian::Bool = false, large_exp_reduce::Bool = false, large_var_full::Bool = false,
                      large_var_hessian::Bool = false, large_var_exp::Bool = false, large_var_exp_hessian::Bool = false)
    large_exp_reduce && throw(ArgumentError("HipPadeIntegrator: large_exp_reduce = true is not served on a variational integrator (the flags PCL_LARGE_N and PCL_LARGE_EXP go with a plain context; var_compact is its option)"))
    large_exp_hessian && throw(ArgumentError("HipPadeIntegrator: large_exp_hessian = true is not served on a variational integrator (the flags PCL_LARGE_N and PCL_LARGE_EXP go with a plain context)"))
    large_exp && throw(ArgumentError("HipPadeIntegrator: large_exp = true is not served on a variational integrator (the flags PCL_LARGE_N and PCL_LARGE_EXP go with a plain context)"))
    large_reduce && throw(ArgumentError("HipPadeIntegrator: large_reduce = true is not served on a variational integrator (the flag PCL_LARGE_N goes with the plain Pade constraint; var_compact is its option)"))
    large_full && throw(ArgumentError("HipPadeIntegrator: large_full = true is not served on a variational integrator (the flag PCL_LARGE_N goes with the plain Pade constraint; var_full is its option)"))
    large_hessian && throw(ArgumentError("HipPadeIntegrator: large_hessian = true is not served on a variational integrator (the flag PCL_LARGE_N goes with the plain Pade constraint)"))
    pade_order = _order_code(pade_order)
    expo = pade_order == PCL_ORDER_EXP
    (large_var_exp && !large_generator) &&
        throw(ArgumentError("HipPadeIntegrator: large_var_exp = true is the exponential constraint of a variational context created with large_generator = true (the flags PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP): it needs that keyword"))
    (large_var_exp && !expo) &&
        throw(ArgumentError("HipPadeIntegrator: large_var_exp = true is the variational exponential constraint at generator dimensions 66 .. 128: it needs pade_order = :exp"))
    (large_var_exp && (exp_hessian !== false || var_compact || large_var_hessian)) &&
        throw(ArgumentError("HipPadeIntegrator: large_var_exp = true serves residual and Jacobian, and with large_var_full = true the objective and the rollout: the Hessian of the Lagrangian and the compact Jacobian are not implemented for a large variational exponential context (PCL_LARGE_VAR_EXP), so exp_hessian, var_compact and large_var_hessian stay off"))
    (large_var_exp_hessian && !large_var_exp) &&
        throw(ArgumentError("HipPadeIntegrator: large_var_exp_hessian = true is the Hessian of the Lagrangian of a variational context created with large_var_exp = true (large_generator = true, pade_order = :exp): it needs that keyword"))
    (large_generator && expo && !large_var_exp) &&
        throw(ArgumentError("HipPadeIntegrator: large_generator = true on a variational integrator serves the diagonal Pade orders 2 .. 10: pade_order = :exp has no large variational contexts"))
    (large_var_full && !large_generator) &&
        throw(ArgumentError("HipPadeIntegrator: large_var_full = true is the objective and the rollout of a variational context created with large_generator = true: it needs that keyword"))
    (large_var_full && expo && !large_var_exp) &&
        throw(ArgumentError("HipPadeIntegrator: large_var_full = true serves the diagonal Pade orders 2 .. 10: pade_order = :exp (PCL_BATCH_VARIATIONAL_EXP) has no large variational contexts"))
    (large_var_hessian && !large_generator) &&
        throw(ArgumentError("HipPadeIntegrator: large_var_hessian = true is the Hessian of the Lagrangian of a variational context created with large_generator = true: it needs that keyword"))
    (large_var_hessian && expo) &&
        throw(ArgumentError("HipPadeIntegrator: large_var_hessian = true serves the diagonal Pade orders 2 .. 10: pade_order = :exp (PCL_BATCH_VARIATIONAL_EXP) has no large variational contexts"))
    (exp_hessian isa Symbol && exp_hessian != :workspace) &&
        throw(ArgumentError("HipPadeIntegrator: exp_hessian must be false, true or :workspace (got :$(exp_hessian))"))
    workspace = exp_hessian === :workspace
    exp_hessian = exp_hessian !== false
    (exp_hessian && !expo) &&
        throw(ArgumentError("HipPadeIntegrator: exp_hessian = true is the Hessian of the Lagrangian of the exponential constraint: it needs pade_order = :exp"))
    m = sys.n_drives
    e(j) = (a = zeros(m); a[j] = 1.0; a)
    zu = zeros(m)
    G0 = Matrix{Float64}(sys.G(zu))                                   # the variational system's G takes the controls only
    Gj = [Matrix{Float64}(sys.G(e(j))) - G0 for j in 1:m]
    Gv = [Matrix{Float64}(Gvf(zu)) ./ s for (Gvf, s) in zip(sys.G_vars, scales)]   # sys.G_vars: functions of the controls [REF variational_quantum_systems.jl:66-124]
    names = vcat(x, x_vars...)
    x_offs = Int32[traj.components[nm][1] - 1 for nm in names]
    G0s = reduce(vcat, [vec(G) for G in vcat([G0], Gv)])
    Gjv = m == 0 ? zeros(1) : reduce(vcat, [vec(G) for G in Gj])
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve G0s Gjv x_offs begin
        desc = PclDesc(sizeof(PclDesc), size(G0, 1) ÷ 2, m, traj.N, traj.dim, traj.components[u][1] - 1, traj.components[traj.timestep][1] - 1,
                       length(names), (expo ? 3 #= PCL_BATCH_VARIATIONAL_EXP =# : 2 #= PCL_BATCH_VARIATIONAL =#) | (large_generator ? PCL_LARGE_N | PCL_LARGE_VAR : 0) | (large_var_exp ? PCL_LARGE_VAR_EXP : 0), pade_order, device, 1 #= 1-based =#, 1 #= G0 = [G_drift; Gv_i] =#,
                       state_cols, traj.global_dim, pointer(G0s), pointer(Gjv), pointer(x_offs))
        rc = ccall((:pcl_create, LIB), Cint, (Ref{PclDesc}, Ref{Ptr{Cvoid}}), desc, ctx)
        rc == 0 || error("pcl_create: ", _lasterr(C_NULL))
    end
    c = ctx[]
    xd = Ref{Int64}(0); nr = Ref{Int64}(0); ncol = Ref{Int64}(0); nnz = Ref{Int64}(0); per = Ref{Int64}(0); hnnz = Ref{Int64}(0)
    check(c, ccall((:pcl_constraint_dim, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}), c, xd, nr, ncol))
    check(c, ccall((:pcl_jac_nnz, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), c, nnz, per))
    workspace && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "var_exp_hess_tiles", 1))
    exp_hessian && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "var_exp_hess", 1))
    var_compact && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "var_compact", 1))
    large_var = large_generator && size(G0, 1) > 64                   # (a large variational context: the Hessian of the Lagrangian is refused without large_var_hessian)
    (large_var && large_var_full) && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "large_var_full", 1))
    (large_var && large_var_hessian) && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "large_var_hess", 1))
    lve_hess = large_var && large_var_exp && large_var_exp_hessian    # (a large variational exponential context with its Hessian switched on)
    lve_hess && check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "large_var_exp_hess", 1))
    (!lve_hess && ((expo && !exp_hessian) || (large_var && !large_var_hessian))) ? (hnnz[] = 0; per[] = 0) : check(c, ccall((:pcl_hess_nnz, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), c, hnnz, per))
    core = PclCore(c, 1, Int(xd[]), Int(nr[]), Int(nnz[]), Int(hnnz[]), Float64[], Float64[], Float64[], false, false, 0)
    finalizer(_destroy!, core)
    pade_order == 0 && _decide_order!(core, traj, u, m, order_tol)
    order = _order_in_use(core)
    order == 0 && error("HipPadeIntegrator: the Pade order could not be decided")
    jr = Vector{Int32}(undef, core.jac_per); jc = similar(jr)
    check(c, ccall((:pcl_jac_structure, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}), c, jr, jc))
    hr = Vector{Int32}(undef, core.hess_per); hc = similar(hr)
    (!lve_hess && ((expo && !exp_hessian) || large_var)) || check(c, ccall((:pcl_hess_structure, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}), c, hr, hc))
    # (B.f is refused for the stacked state, see _f: fcore stays `nothing`)
    return HipPadeIntegrator(core, 1, x, names, u, core.x_dim, core.rows_per, jr, jc, hr, hc, Int(ncol[]), G0, Gj, state_cols, order, nothing)
end

# VariationalKetIntegrator(sys, traj, :ψ̃, [:ψ̃_var, ...], :u; scale)          [REF src/control/integrators.jl:234-245]
VariationalKetIntegrator(sys, traj::NamedTrajectory, ψ̃::Symbol, ψ̃_variations::AbstractVector{Symbol}, u::Symbol; scale::Float64 = 1.0, kwargs...) =
    _variational(sys, traj, ψ̃, ψ̃_variations, u, fill(scale, length(sys.G_vars)), 1; kwargs...)

# VariationalUnitaryIntegrator(sys, traj, :Ũ⃗, [:Ũ⃗_var, ...], :u; scales)       [REF src/control/integrators.jl:247-264]
VariationalUnitaryIntegrator(sys, traj::NamedTrajectory, Ũ⃗::Symbol, Ũ⃗_variations::AbstractVector{Symbol}, u::Symbol;
                             scales::AbstractVector{<:Float64} = fill(1.0, length(sys.G_vars)), kwargs...) =
    _variational(sys, traj, Ũ⃗, Ũ⃗_variations, u, Vector{Float64}(scales), 0; kwargs...)

# ---- robust control on a variational integrator: the objective and the rollout (context option "var_full") ----------------------------------
_is_variational(B::HipPadeIntegrator) = length(getfield(B, :x_names)) > 1 && _core(B).n_members == 1
function _enable_var_full!(B::HipPadeIntegrator)
    _is_variational(B) || error("a variational integrator (VariationalUnitaryIntegrator / VariationalKetIntegrator) is required")
    c = _core(B).ctx
    lvf = Ref{Int64}(0)   # a large variational context with large_var_full on serves the objective and the rollout already
    check(c, ccall((:pcl_get_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Ref{Int64}), c, "large_var_full", lvf))
    lvf[] == 1 && return c
    check(c, ccall((:pcl_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Int64), c, "var_full", 1))
    return c
end

# variational_rollout(B, traj): the stacked states vcat(x, x_var_1, ..) at every knot, x_dim x N, by exact propagation under the lifted
# generator (x <- E x, x_var_i <- E x_var_i + L_i x) from the knot-0 state -- next to unitary_rollout [REF src/quantum/dynamics.jl:631-667]
function variational_rollout(B::HipPadeIntegrator, traj::NamedTrajectory)
    c = _enable_var_full!(B)
    z = Vector{Float64}(vec(traj.datavec))
    X = Matrix{Float64}(undef, getfield(B, :x_dim), traj.N)
    check(c, ccall((:pcl_rollout, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), c, z, X))
    return X
end

# bind_robust_objective!(B; goal_iso_vec, Q, sensitivities, regularizers): the objective of a robust-control problem on the device,
#     Q |1 - F(U_N)| + sum_i Qs_i scale_i^4 |tr(U_var_i' U_var_i)|^2 / n^2 (terminal knot) + regularisers
# [REF UnitaryInfidelityObjective objectives.jl:347-356; UnitarySensitivityObjective objectives.jl:437-453, used at [traj.N] by
# src/specs/materialize.jl:306-307].  sensitivities: variation name => (Qs, scale); times other than [traj.N] are not implemented.
# regularizers: (name, R::Vector{Float64}, dt_power).  Returns (value_and_gradient, hessian_structure, hessian) closures over the context.
function bind_robust_objective!(B::HipPadeIntegrator, traj::NamedTrajectory; goal_iso_vec::Union{Nothing,Vector{Float64}} = nothing, Q::Float64 = 100.0,
                                sensitivities::AbstractDict{Symbol,<:Tuple{Real,Real}} = Dict{Symbol,Tuple{Float64,Float64}}(),
                                times::AbstractVector{<:Integer} = [traj.N], regularizers = ())
    times == [traj.N] || error("sensitivity terms at the terminal knot only: times must be [$(traj.N)], got $times")
    names = getfield(B, :x_names)
    c = _enable_var_full!(B)
    w = zeros(length(names)); w[1] = 1.0
    for (nm, (Qs, scale)) in sensitivities
        i = findfirst(==(nm), names)
        (i === nothing || i == 1) && error("the sensitivity term names $nm; it must name one of the variations $(names[2:end])")
        w[i] += Qs * scale^4
    end
    check(c, ccall((:pcl_clear_regularizers, LIB), Cint, (Ptr{Cvoid},), c))
    for (nm, R, p) in regularizers
        r = traj.components[nm]
        Rv = Vector{Float64}(R)
        check(c, ccall((:pcl_add_regularizer, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Int32), c, r[1] - 1, length(r), Rv, p))
    end
    goal_iso_vec === nothing || check(c, ccall((:pcl_set_goal, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), c, goal_iso_vec))
    check(c, ccall((:pcl_set_weights, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), c, w))
    nv = getfield(B, :n_vars)
    function value_and_gradient(z::Vector{Float64})
        val = Ref{Float64}(0.0); g = Vector{Float64}(undef, nv)
        check(c, ccall((:pcl_objective, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Float64, Ref{Float64}, Ptr{Float64}), c, z, Q, val, g))
        return val[], g
    end
    function hessian_structure()   # queried AFTER the weights and regularisers are set: it depends on them
        n = Ref{Int64}(0)
        check(c, ccall((:pcl_objective_hess_nnz, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), c, n))
        rows = Vector{Int64}(undef, n[]); cols = similar(rows)
        check(c, ccall((:pcl_objective_hess_structure, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), c, rows, cols))
        return rows, cols
    end
    function hessian(z::Vector{Float64}, σ::Float64 = 1.0)
        n = Ref{Int64}(0)
        check(c, ccall((:pcl_objective_hess_nnz, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), c, n))
        vals = Vector{Float64}(undef, n[])
        check(c, ccall((:pcl_objective_hess, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Float64, Float64, Ptr{Float64}), c, z, Q, σ, vals))
        return vals
    end
    return value_and_gradient, hessian_structure, hessian
end

function _fresh!(core::PclCore, z::AbstractVector{Float64})
    if length(core.z) != length(z) || core.z != z
        core.z = copy(z)
        core.have_δ = core.have_vals = false
    end
    return core.z
end

function _all_δ!(core::PclCore, z)
    zc = _fresh!(core, z)
    if !core.have_δ
        length(core.δ) == core.rows_per * core.n_members || (core.δ = Vector{Float64}(undef, core.rows_per * core.n_members))
        δ = core.δ
        GC.@preserve zc δ check(core.ctx, ccall((:pcl_eval, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), core.ctx, zc, δ))
        core.have_δ = true; core.launches += 1
    end
    return core.δ
end

function _all_vals!(core::PclCore, z)
    zc = _fresh!(core, z)
    if !core.have_vals
        length(core.δ) == core.rows_per * core.n_members || (core.δ = Vector{Float64}(undef, core.rows_per * core.n_members))
        length(core.vals) == core.jac_per * core.n_members || (core.vals = Vector{Float64}(undef, core.jac_per * core.n_members))
        δ = core.δ; v = core.vals
        GC.@preserve zc δ v check(core.ctx, ccall((:pcl_eval_jac, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), core.ctx, zc, δ, v))
        core.have_δ = core.have_vals = true; core.launches += 1
    end
    return core.vals
end

_core(B::HipPadeIntegrator) = getfield(B, :core)
_rows(B::HipPadeIntegrator) = ((getfield(B, :member) - 1) * _core(B).rows_per + 1):(getfield(B, :member) * _core(B).rows_per)
_jrng(B::HipPadeIntegrator) = ((getfield(B, :member) - 1) * _core(B).jac_per + 1):(getfield(B, :member) * _core(B).jac_per)

# evaluate!(delta, B, traj)                                                   [REF integrators.jl:311,777]
function DirectTrajOpt.evaluate!(δ::AbstractVector{Float64}, B::HipPadeIntegrator, traj::NamedTrajectory)
    length(δ) == getfield(B, :dim) || throw(DimensionMismatch("δ has length $(length(δ)), integrator dim is $(getfield(B, :dim))"))
    copyto!(δ, view(_all_δ!(_core(B), traj.datavec), _rows(B)))
    return δ
end

# eval_jacobian(B, traj) -> sparse (B.dim, traj.dim*traj.N + traj.global_dim)  [REF integrators.jl:780-783]
function DirectTrajOpt.eval_jacobian(B::HipPadeIntegrator, traj::NamedTrajectory)
    vals = _all_vals!(_core(B), traj.datavec)[_jrng(B)]
    return sparse(getfield(B, :jac_rows), getfield(B, :jac_cols), vals, getfield(B, :dim), getfield(B, :n_vars))
end

# ---- what DirectTrajOpt's MOI evaluator needs per IPM iteration, in the shapes this library produces them: triplet structure
#      queried once, values in that order.  DirectTrajOpt is not vendored with Piccolo and its generic names differ between
#      the 0.9 and 0.10 lines, so the methods are defined under this module's own names AND -- at load time -- as methods of
#      whichever of the candidate generics the INSTALLED DirectTrajOpt defines (`_bind_to_directtrajopt!` below); selftest.jl
#      prints what was bound.
jacobian_structure(B::HipPadeIntegrator) = collect(zip(Int.(getfield(B, :jac_rows)), Int.(getfield(B, :jac_cols))))
hessian_structure(B::HipPadeIntegrator) = collect(zip(Int.(getfield(B, :hess_rows)), Int.(getfield(B, :hess_cols))))

function eval_constraint_and_jacobian!(δ::AbstractVector{Float64}, vals::AbstractVector{Float64}, B::HipPadeIntegrator, z::Vector{Float64})
    v = _all_vals!(_core(B), z)
    copyto!(vals, view(v, _jrng(B)))
    copyto!(δ, view(_core(B).δ, _rows(B)))
    return nothing
end

# Jacobian values alone, in structure order (the in-place filler shape)
function eval_jacobian_values!(vals::AbstractVector{Float64}, B::HipPadeIntegrator, z::AbstractVector{Float64})
    copyto!(vals, view(_all_vals!(_core(B), z), _jrng(B)))
    return vals
end

# Hessian of the Lagrangian of THIS integrator's rows: μ is the block's multiplier slice (length B.dim); runs on a
# one-member window of the shared context (every Pade order)
function eval_hessian_of_lagrangian!(vals::Vector{Float64}, B::HipPadeIntegrator, z::Vector{Float64}, μ::Vector{Float64})
    core = _core(B)
    length(μ) == getfield(B, :dim) || throw(DimensionMismatch("μ has length $(length(μ)), integrator dim is $(getfield(B, :dim))"))
    length(vals) == core.hess_per || throw(DimensionMismatch("vals has length $(length(vals)), expected $(core.hess_per)"))
    _window!(core, getfield(B, :member) - 1, 1)
    try
        GC.@preserve z μ vals check(core.ctx, ccall((:pcl_hess, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), core.ctx, z, μ, vals))
    finally
        _window!(core, 0, core.n_members)
    end
    return nothing
end

# Adaptive binding.  For every candidate generic the installed DirectTrajOpt defines, a method for HipPadeIntegrator is added
# that forwards to the functions above; the argument shapes tried are the ones DirectTrajOpt's own BilinearIntegrator methods
# use in the 0.9 / 0.10 lines (structure: (B) or (B, traj); in-place values: (vals, B, traj) / (B, traj) -> values;
# Hessian of the Lagrangian: (vals, B, traj, μ) / (B, traj, μ)).  Names the installed version does not define are skipped --
# the module-local functions stay available either way.  Returns the list of names bound (selftest.jl prints it).
const BOUND_GENERICS = Symbol[]
function _bind_to_directtrajopt!()
    empty!(BOUND_GENERICS)
    z_of(traj) = traj isa NamedTrajectory ? traj.datavec : traj
    for nm in (:jacobian_structure, :get_jacobian_structure)
        isdefined(DirectTrajOpt, nm) || continue
        @eval DirectTrajOpt.$nm(B::HipPadeIntegrator, args...) = jacobian_structure(B)
        push!(BOUND_GENERICS, nm)
    end
    for nm in (:hessian_structure, :hessian_of_lagrangian_structure, :get_hessian_structure)
        isdefined(DirectTrajOpt, nm) || continue
        @eval DirectTrajOpt.$nm(B::HipPadeIntegrator, args...) = hessian_structure(B)
        push!(BOUND_GENERICS, nm)
    end
    for nm in (:jacobian!, :eval_jacobian!, :jacobian_values!)
        isdefined(DirectTrajOpt, nm) || continue
        @eval DirectTrajOpt.$nm(vals::AbstractVector{Float64}, B::HipPadeIntegrator, traj, args...) =
            eval_jacobian_values!(vals, B, $z_of(traj))
        push!(BOUND_GENERICS, nm)
    end
    for nm in (:hessian_of_lagrangian!, :eval_hessian_of_lagrangian!, :hessian_of_lagrangian_values!)
        isdefined(DirectTrajOpt, nm) || continue
        @eval function DirectTrajOpt.$nm(vals::AbstractVector{Float64}, B::HipPadeIntegrator, traj, μ::AbstractVector{Float64}, args...)
            # the C entry point fills a dense Vector{Float64}: a view (or any other AbstractVector) is filled through a temporary
            if vals isa Vector{Float64}
                eval_hessian_of_lagrangian!(vals, B, Vector{Float64}($z_of(traj)), Vector{Float64}(μ))
            else
                tmp = Vector{Float64}(undef, length(vals))
                eval_hessian_of_lagrangian!(tmp, B, Vector{Float64}($z_of(traj)), Vector{Float64}(μ))
                copyto!(vals, tmp)
            end
            return nothing
        end
        push!(BOUND_GENERICS, nm)
    end
    for nm in (:hessian_of_lagrangian, :eval_hessian_of_lagrangian)
        isdefined(DirectTrajOpt, nm) || continue
        @eval function DirectTrajOpt.$nm(B::HipPadeIntegrator, traj, μ::AbstractVector{Float64}, args...)
            vals = Vector{Float64}(undef, _core(B).hess_per)
            eval_hessian_of_lagrangian!(vals, B, Vector{Float64}($z_of(traj)), Vector{Float64}(μ))
            return sparse(Int.(getfield(B, :hess_rows)), Int.(getfield(B, :hess_cols)), vals, getfield(B, :n_vars), getfield(B, :n_vars))
        end
        push!(BOUND_GENERICS, nm)
    end
    return BOUND_GENERICS
end
__init__() = _bind_to_directtrajopt!()

# ---- B.f(x_next, x, u, Δt): the scalar one-interval form the reference reads [REF integrators.jl:518-525,552;
#      src/control/display/inspect.jl:630-636] -- a cached 2-knot context with layout [x | Δt | u] -----------------------
function _f(B::HipPadeIntegrator, x_next::AbstractVector, x::AbstractVector, u::AbstractVector, Δt::Real)
    # a variational integrator (several stacked state names on one context) has no one-interval form here: its generator is the lifted
    # var_G(G(u), [Gv_i]), which a plain two-knot context of the nominal generators does not evaluate
    length(getfield(B, :x_names)) > 1 && error("B.f is not available for a variational integrator (stacked state $(getfield(B, :x_names)))")
    xd = getfield(B, :x_dim); Gj = getfield(B, :Gj); m = length(Gj)
    fc = getfield(B, :fcore)
    if fc === nothing
        fc, _ = _create_core([getfield(B, :G0)], Gj, 2, xd + 1 + m, xd + 1, xd, Int32[0], 0;
                             state_cols = getfield(B, :state_cols), pade_order = _order_in_use(getfield(B, :core)))   # the main context's order, read back
        setfield!(B, :fcore, fc)
    end
    z = zeros(2 * (xd + 1 + m))
    z[1:xd] .= x; z[xd+1] = Δt; z[(xd+2):(xd+1+m)] .= u[1:m]
    z[(xd+1+m+1):(xd+1+m+xd)] .= x_next
    δ = Vector{Float64}(undef, xd)
    GC.@preserve z δ check(fc.ctx, ccall((:pcl_eval, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), fc.ctx, z, δ))
    return δ
end

function Base.getproperty(B::HipPadeIntegrator, s::Symbol)
    s === :f && return (x_next, x, u, Δt) -> _f(B, x_next, x, u, Δt)
    s === :ctx && return getfield(B, :core).ctx
    s === :pade_order && return _order_in_use(getfield(B, :core))   # asked of the context: never a stale copy
    return getfield(B, s)
end
Base.propertynames(B::HipPadeIntegrator, private::Bool = false) = (fieldnames(HipPadeIntegrator)..., :f, :ctx)

export HipPadeIntegrator, VariationalKetIntegrator, VariationalUnitaryIntegrator, variational_rollout, bind_robust_objective!
end # module
