"""Cases for the objective family and the rollout at generator dimensions 66 .. 128 (option large_full on a context created with PCL_LARGE_N;
piccolo.jl_amd/csrc/pcl_kernel_large_rollout.hpp and the objective kernels of n <= 64 behind the option's gate); importable without a GPU.

Systems, layouts, knots and N = 4 are those of tests/large_shape_cases.py (imported, never written to): L1 (n = 66, a ket), L3 (n = 128), L4
(n = 120, 24 drives), L5 (n = 72, five kets), L6 (n = 66 as a unitary of 33 columns), L8 (n = 121, odd, PCL_STATE_VECTOR).  The steps are this
module's, fixed per case from G(u_k) so that the two trajectories of a case walk every branch of the substep rule s' = ceil(|h| |G|_1 / theta):
    seed 0   interval 0   h |G|_1 = -0.8     one substep, a negative step
             interval 1   h |G|_2 = the long step: the smallest of LONG_STEPS (5 for the skew iso generators, 10 for the non-normal vec one,
                          whose spectral radius is half its 2-norm) at which ONE substep in place of s' moves a knot of the float64
                          restatement by 1e-6 of its size or more; several theta: s' >= 3 (the 1-norm of these dense generators is
                          3 .. 9 x the 2-norm)
             interval 2   h = 0              s' = 0: E = I exactly
    seed 1   interval 0   h |G|_1 = +0.8     one substep
             interval 1   h |G|_1 = -2.5     three substeps of a negative step
             interval 2   h |G|_2 = +0.3
A member of another drift (PCL_BATCH_MEMBERS) shares the knots, so its steps are those of drift 0.

The truth of the rollout (`rollout_truth_ld`) is a scaled Taylor series in np.longdouble applied to the state: the step is cut into
ceil(|h| |G|_2 / 0.5) pieces (the 2-norm, not the kernel's 1-norm rule) and each piece is the degree-32 polynomial in Horner form (remainder
0.5^33 / 33! = 1e-47); every product goes through the `mm` hook of tests/vector_shape_cases.py.  `restatement` is the kernel's algorithm in
float64 numpy -- theta = 1, degree 18, s' from the column sums, propagators first, then the chain -- with the same hook and a hook for the
substep rule, where tests/test_large_full_cpu.py injects its faults.  `roll_plan` restates large_roll_plan of piccolo_hip.hip.

The objective cases are dictionaries in the format of tests/objective_cases.py (its `terms`, `objective_truth`, `hessian_truth` and
`grad_labels` serve them as they are): knot [states of the members | dt | t | u], the case's own system, terminal states on both sides of the kink."""
import functools
import math

import numpy as np

import large_shape_cases as lc
import objective_cases as oc
import objective_truth as ot
import vector_shape_cases as vc

N = lc.N
LDS_BYTES = lc.LDS_BYTES
SLACK = lc.SLACK
THETA, DEG, SMAX = 1.0, 18, 1024  # LR_THETA, LR_DEG, LR_SMAX
TRUTH_THETA, TRUTH_DEG = 0.5, 32
NAMES = ("L1", "L3", "L4", "L5", "L6", "L8")
TOL = 1e-11  # every knot, relative to max |X_k| of the truth
SEEN = 1e-7
LONG_STEPS = (5.0, 7.0, 10.0, 14.0)
LD_ = np.longdouble


# ---- the launch code's arithmetic (large_roll_plan, piccolo_hip.hip) --------------------------------------------------------------------------
def roll_plan(n, cols, m, items=N - 1, n_cu=256, cols_per_slice=0, slices=0):
    LD, threads = n | 1, 64 * ((n + 15) // 16)
    budget, tile = LDS_BYTES // 8, LD * n
    fixed_e, fixed_c = tile + SLACK + m + 8, SLACK  # (the chain launch holds no tile: its operand goes from the workspace into registers)
    npc_max = max(1, min(n, (budget - fixed_e) // LD // 3))
    p_min = -(-n // npc_max)
    want = slices if slices > 0 else min((n + 15) // 16, n_cu // max(items, 1))
    P = max(p_min, min(want, n))
    npc = -(-n // P)
    P = -(-n // npc)
    nc_fit = max(1, (budget - fixed_c) // LD // 2)
    nc_cap = min(cols_per_slice, cols) if cols_per_slice > 0 else min(cols, 16)
    nc = min(nc_cap, nc_fit)
    S = -(-cols // nc)
    nc = -(-cols // S)
    return dict(LD=LD, threads=threads, P=P, npc=npc, S=S, nc=nc, bytes_e=(fixed_e + 3 * LD * npc) * 8, bytes_c=(fixed_c + 2 * LD * nc) * 8,
                npce=[max(0, min(npc, n - u * npc)) for u in range(P)], nce=[max(0, min(nc, cols - s * nc)) for s in range(S)])  # fmt: skip


def substeps(h, G):
    """The kernel's rule: s' = ceil(|h| |G|_1 / theta), 0 at h = 0, at most SMAX."""
    x = abs(float(h)) * float(np.abs(np.asarray(G, dtype=float)).sum(axis=0).max())
    return 0 if x == 0 else (int(math.ceil(x / THETA)) if x <= SMAX * THETA else SMAX)


# ---- trajectories -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name, seed=0, drift=0):
    """(layout, G0, Gj, Z, substeps per interval), read-only: the knots of lc.case(name, seed) with this module's steps."""
    lay, _, Gj, Z0, _ = lc.case(name, seed)
    G0 = lc.system(name, 0)[0]
    Z = np.array(Z0)
    G = [vc.g_of(lay, Z, k, G0, Gj) for k in range(N - 1)]
    n1 = [np.abs(g).sum(axis=0).max() for g in G]
    n2 = [np.linalg.norm(g, 2) for g in G]
    if seed % 2 == 0:
        Z[: N - 1, lay.dt_off] = (-0.8 / n1[0], 0.0, 0.0)
        for s in LONG_STEPS:
            Z[1, lay.dt_off] = s / n2[1]
            full = restatement(lay, G0, Gj, Z)
            if knot_errors(restatement(lay, G0, Gj, Z, rule=lambda h, G: min(1, substeps(h, G))), full).max() >= 10 * SEEN:
                break
        else:
            raise AssertionError(name)
    else:
        Z[: N - 1, lay.dt_off] = (0.8 / n1[0], -2.5 / n1[1], 0.3 / n2[2])
    steps = Z[: N - 1, lay.dt_off]
    Z[:, lay.dt_off + 1] = np.cumsum(Z[:, lay.dt_off])
    sp = tuple(substeps(steps[k], G[k]) for k in range(N - 1))
    G0 = lc.system(name, drift)[0]
    for a in (G0, Z):
        a.setflags(write=False)
    return lay, G0, Gj, Z, sp


def pade_case(name="L1"):
    """The knots of `name` with every step at |h| |G|_2 <= 0.3 (0.3, -0.2, 0.1): where the order-10 Pade residual of exact states is of order
    theta^11 1e-10."""
    lay, G0, Gj, Z, _ = case(name)
    Z = np.array(Z)
    for k, th in enumerate((0.3, -0.2, 0.1)):
        Z[k, lay.dt_off] = th / np.linalg.norm(vc.g_of(lay, Z, k, G0, Gj), 2)
    Z.setflags(write=False)
    return lay, G0, Gj, Z


def _cols(lay, v, dtype):
    return np.array(np.asarray(v, dtype=dtype).reshape(lay.C, lay.n).T)


# ---- the truth --------------------------------------------------------------------------------------------------------------------------------
def rollout_truth_values(lay, G0, Gj, Z, mm=vc._mm):
    """[N, x_dim] in longdouble: X_{k+1} = exp(h_k G(u_k)) X_k by the scaled Taylor series applied to the state."""
    G0l, Gl = np.asarray(G0, dtype=LD_), [np.asarray(g, dtype=LD_) for g in Gj]
    X = _cols(lay, Z[0, lay.x_off : lay.x_off + lay.x_dim], LD_)
    out = [X.T.reshape(-1)]
    for k in range(lay.K):
        h = LD_(Z[k, lay.dt_off])
        G = G0l.copy()
        for l in range(lay.m):
            G = G + LD_(Z[k, lay.u_off + l]) * Gl[l]
        s = int(math.ceil(abs(float(h)) * np.linalg.norm(G.astype(float), 2) / TRUTH_THETA))
        for _ in range(s):
            V = X
            for j in range(TRUTH_DEG, 0, -1):
                V = X + (h / s / j) * mm(G, V)
            X = V
        out.append(X.T.reshape(-1))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def rollout_truth_ld(name, seed=0, drift=0):
    lay, G0, Gj, Z, _ = case(name, seed, drift)
    out = rollout_truth_values(lay, G0, Gj, Z)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rollout_truth(name, seed=0, drift=0):
    """The same rounded to float64: what the GPU tests compare with."""
    out = rollout_truth_ld(name, seed, drift).astype(np.float64)
    out.setflags(write=False)
    return out


# ---- the kernel's algorithm in float64 ------------------------------------------------------------------------------------------------------------
def restatement(lay, G0, Gj, Z, mm=vc._mm, rule=substeps):
    """[N, x_dim]: per interval E = T(h_s G)^{s'} I with the degree-18 polynomial in Horner form V <- Y + (h_s / j) G V, then the chain of the
    knots, in float64."""
    E = []
    for k in range(lay.K):
        h, G = float(Z[k, lay.dt_off]), np.array(vc.g_of(lay, Z, k, G0, Gj))
        sp = rule(h, G)
        Y = np.eye(lay.n)
        for _ in range(sp):
            V = Y
            for j in range(DEG, 0, -1):
                V = Y + (h / sp / j) * mm(G, V)
            Y = V
        E.append(Y)
    X = _cols(lay, Z[0, lay.x_off : lay.x_off + lay.x_dim], np.float64)
    out = [X.T.reshape(-1)]
    for k in range(lay.K):
        X = mm(E[k], X)
        out.append(X.T.reshape(-1))
    return np.array(out)


def knot_errors(got, ref, knots=N):
    """Per knot max |got - ref| / max |ref|."""
    got, ref = np.asarray(got).reshape(knots, -1), np.asarray(ref).reshape(knots, -1)
    return np.array([float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in range(knots)])


def subspace_loss_ld(x, Gs, sub, d, wQ):
    """(value, gradient [2 d^2]) of wQ |1 - F|, F = (|M|_F^2 + |tr M|^2) / (ns (ns + 1)), M = Gs' U[sub, sub], in complex longdouble, without the
    rows of the general form (2 ns^2 + 2 rows of 2 d^2 entries: half a gigabyte at ns = 45, d = 64): the gradient with respect to (Re U, Im U) is
    (Re D, Im D) of D = 2 (Gs M + tr(M) Gs) / (ns (ns + 1)).  tests/test_large_full_cpu.py holds it to the rows' truth at ns = 4."""
    CL = np.clongdouble
    sub = np.asarray(sub)
    ns = len(sub)
    X = ot.ld(x).reshape(d, 2 * d)
    U = X[:, :d].T.astype(CL) + CL(1j) * X[:, d:].T.astype(CL)  # [i, c]
    G = np.asarray(Gs).astype(CL)
    M = G.conj().T @ U[np.ix_(sub, sub)]
    t = np.trace(M)
    K = LD_(ns) * LD_(ns + 1)
    F = ((M.real**2 + M.imag**2).sum() + t.real**2 + t.imag**2) / K
    D = 2 * (G @ M + t * G) / K
    s = LD_(1) if 1 - F >= 0 else LD_(-1)
    g = np.zeros(2 * d * d, dtype=LD_)
    for l in range(ns):
        g[sub[l] * 2 * d + sub] = D[:, l].real
        g[sub[l] * 2 * d + d + sub] = D[:, l].imag
    return wQ * s * (1 - F), -s * wQ * g, F


# ---- objective cases (the dictionaries of tests/objective_cases.py) ---------------------------------------------------------------------------------
def _obj(name, base, *, members=1, traj=0, goal, states, weights=None, regs_p=(1,), Q=100.0, launches=None, hess=False, sigma=1.0, seed=0):
    kind, n, cols, m = lc.CASES[base]
    G0, Gj = lc.system(base)
    vec = kind == "vec"
    xd = n * cols
    M = 1 if traj else members
    dt_off = M * xd
    z_dim, u_off = dt_off + 2 + m, dt_off + 2
    rng = np.random.default_rng(16000 + seed)
    nbuf = traj or 1
    Z = 0.4 * rng.standard_normal((nbuf, N, z_dim))
    Z[:, :, dt_off] = 0.05 + 0.1 * rng.random((nbuf, N))
    x_offs = [b * xd for b in range(M)]
    for b, x in enumerate(states):
        if x is not None:
            Z[b if traj else 0, -1, (0 if traj else x_offs[b]) : (0 if traj else x_offs[b]) + xd] = x
    regs = [(u_off, m, 0.2 + np.random.default_rng(16100 + seed + p).random(m), p) for p in regs_p]
    Z.setflags(write=False)
    return dict(name=name, base=base, d=n if vec else n // 2, m=m, N=N, x_offs=x_offs, z_dim=z_dim, dt_off=dt_off, u_off=u_off, traj=traj,
                batch=traj or members, state_cols=-1 if vec else (0 if cols == n // 2 else cols), x_dim=xd, Z=Z, G0=G0, Gj=Gj, goal=goal,
                weights=None if weights is None else np.asarray(weights, float), Q=Q, regs=regs, launches=launches, mutants=(), hess=hess,
                index_base=0, sigma=sigma)  # fmt: skip


def _build():
    out = {}
    rng = np.random.default_rng(16500)
    d6 = 33
    G = oc._unitary(d6, rng)
    # matrix goal on L6: three members with weights, the regulariser on the drive at dt_power 0, 1 and 2; member 0 beyond the kink, 1 before it
    out["mat3"] = _obj("mat3", "L6", members=3, goal=("unitary", G), states=[oc._iso_vec(oc._near(G, 1.1, rng)), oc._iso_vec(oc._near(G, 0.9, rng)), None],
                       weights=[0.5, 0.3, 0.2], regs_p=(0, 1, 2), launches=1, seed=1)  # fmt: skip
    # ... and one member of it for the Hessian: a triangle of 2178 x 2179 / 2 = 2,372,931 entries
    out["mat1"] = _obj("mat1", "L6", goal=("unitary", G), states=[oc._iso_vec(oc._near(G, 1.1, rng))], regs_p=(2,), launches=1, hess=True, sigma=0.37, seed=2)
    sub = [2, 9, 17, 30]
    Gs = oc._unitary(4, rng)
    U = 0.3 * (rng.standard_normal((d6, d6)) + 1j * rng.standard_normal((d6, d6)))
    U[np.ix_(sub, sub)] = oc._near(Gs, 0.9, rng)
    out["sub4"] = _obj("sub4", "L6", goal=("subspace", Gs, sub), states=[oc._iso_vec(U)], regs_p=(1,), launches=1, hess=True, seed=3)
    # L5: five kets of 36 levels in one state of 360 entries
    d5, q = 36, 2
    goals = [(lambda v: v / np.linalg.norm(v))(rng.standard_normal(d5) + 1j * rng.standard_normal(d5)) for _ in range(5)]
    x = 0.1 * rng.standard_normal(360)
    x[q * 72 : q * 72 + 72] = np.concatenate([(1.1 * goals[q]).real, (1.1 * goals[q]).imag + 0.02 * rng.standard_normal(d5)])
    rows = ot.functional_rows(360, q * 72 + np.arange(d5), q * 72 + d5 + np.arange(d5), goals[q])
    out["ket5"] = _obj("ket5", "L5", traj=2, goal=("form", 0, np.asarray(rows, float), None), states=[x, None], weights=[0.6, 0.4], regs_p=(2,), launches=3, seed=4)
    cw = [0.9, 0.1, 0.4, 0.7, 0.2]
    xs = np.concatenate([np.concatenate([(0.9 * g + 0.02 * rng.standard_normal(d5)).real, (0.9 * g).imag]) for g in goals])
    out["coh5"] = _obj("coh5", "L5", goal=("form", 0, np.asarray(ot.coherent_ket_rows(goals, cw), float), None), states=[xs], regs_p=(0, 1), launches=3, hess=True,
                       sigma=2.5, seed=5)  # fmt: skip
    # L8: a density vector of 11 levels, F = Re tr(rho rho_goal) = c' x
    c = rng.standard_normal(121) / 11.0
    xv = 0.4 * rng.standard_normal(121)
    out["den"] = _obj("den", "L8", members=2, goal=("form", 0, None, c), states=[xv * (1.6 / float(c @ xv)), xv * (0.4 / float(c @ xv))], weights=[0.7, 0.3],
                      regs_p=(1,), launches=3, seed=6)  # fmt: skip
    return out


OBJ = _build()
