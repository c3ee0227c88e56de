"""Cases for the Hessian of the Lagrangian on large variational exponential contexts (PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR |
PCL_LARGE_VAR_EXP with option large_var_exp_hess; piccolo.jl_amd/csrc/pcl_kernel_var_large_exp_hess.hpp, planned by var_large_exp_hess_plan in
pcl_host_launch_hess.hpp, restated below); numpy and scipy only, importable without a GPU.

Cases: VL1 .. VL6 of tests/var_large_exp_cases.py (systems, knots, the steps h |G(u_k)|_1 = 0.8, -2.5, the long one, and VL2's h = 0) and
    VH1  128 ket  v = 2  m = 24   the system and knots of tests/var_large_hess_cases.py's VH1, two intervals at h |G|_1 = 0.8 and -2.5: one column
                                  and one drive per group, 300 units per pass
Multipliers: default_rng(seed of the case + 77).standard_normal(K x_dim'), in the stacked order of the rows (var_large_hess_cases.rand_mu's rule).

What var_large_exp_hess_plan gives per case (it does not depend on v >= 1 nor on the interval count): sx slices of nc state columns, ngrp groups
of mg drives, U = sx ngrp (ngrp + 1) / 2 units per interval and pass, W columns per buffer, LDS bytes; tests/test_var_large_exp_hess_cpu.py
asserts every number against the restatement:
            n   state   v  m     sx x nc   ngrp x mg     U    W    bytes
    VL1    66   ket     1  2      1 x 1     1 x 2        1   12    55,776
    VL2    66   unitary 2  3     11 x 3     1 x 3       11   60   132,968
    VL3    96   unitary 1  4     48 x 1     1 x 4       48   30   145,456
    VL4   128   ket     2  1      1 x 1     1 x 1        1    6   151,768
    VL5   120   ket     1 24      1 x 1    24 x 1      300    8   140,672
    VL6    72   ket     2  0      1 x 1     1 x 0        1    4    50,144
    VH1   128   ket     2 24      1 x 1    24 x 1      300    8   158,144
n = 128 unitary with m = 24 and v = 2: 64 x 1 slices, 24 x 1 groups, 19,200 units per pass, W = 8 of the 9 columns a buffer has, 158,144 B.

Truth: var_exp_hess_truth.values (scipy's block expm / expm_frechet on the lifted generator).  For m > 6 (VL5, VH1) segment 0 comes from the
per-drive identity (u_l,u_j) = -h <L2(Ahat^T; M' X'^T, h Ghat_l^T), Ghat_j> -- m block exponentials per interval instead of m (m + 1) / 2 -- which
tests/test_var_large_exp_hess_cpu.py holds to the pairwise truth on VL1 and VL2.  VL5's truth is taken on intervals 0 and 2, VH1's on interval 1.
Segments are variational_shape_cases.hess_codes (variable kinds x relative knot x interval, the X' kinds by component).

emulate_hess is the kernel's component-wise recurrence with its passes in float64 numpy; it shares no code with the truth."""
import dataclasses
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp

import exp_hess_truth as eht
import large_exp_cases as le
import var_exp_hess_truth as veh
import var_exp_truth as vet
import var_large_exp_cases as vx
import var_large_hess_cases as vh
import variational_shape_cases as vsc
import variational_truth as vt

LDS_BYTES = vx.LDS_BYTES
SLACK = vx.SLACK
DEG = vx.DEG
NAMES = vx.NAMES + ["VH1"]
STEPS = vx.STEPS
SEEN = 1e-7
# the intervals whose truth is computed (the others: every interval)
TRUTH_INTERVALS = {"VL5": (0, 2), "VH1": (1,)}
# what var_large_exp_hess_plan gives on 163,840 B: (sx, nc, ngrp, mg, U, W, bytes)
TABLE = {
    "VL1": (1, 1, 1, 2, 1, 12, 55776), "VL2": (11, 3, 1, 3, 11, 60, 132968), "VL3": (48, 1, 1, 4, 48, 30, 145456), "VL4": (1, 1, 1, 1, 1, 6, 151768),
    "VL5": (1, 1, 24, 1, 300, 8, 140672), "VL6": (1, 1, 1, 0, 1, 4, 50144), "VH1": (1, 1, 24, 1, 300, 8, 158144),
}  # fmt: skip


def shape(name):
    """(n, C, v, m)"""
    return vh.shape(name)


# ---- the launch code's arithmetic (var_large_exp_hess_plan, pcl_host_launch_hess.hpp) --------------------------------------------------------------
def unit_columns(mg, diagonal):
    """Columns a unit carries per state column and component: W, the dW of its drives, the d2W of its pairs (no drives: W alone, and two behind
    the chain)."""
    if mg == 0:
        return 2
    return 1 + mg + mg * (mg + 1) // 2 if diagonal else 1 + 2 * mg + mg * mg


def plan(n, cols, m, cols_per_slice=0, drives=0):
    LD, threads = n | 1, 64 * ((n + 15) // 16)
    fixed = LD * n + SLACK + m + 8
    NB = (LDS_BYTES // 8 - fixed) // LD
    NBW = NB // 3
    t_min = 2 if m == 0 else (3 if m == 1 else 4)
    nc_hi = min(max(1, NBW // (2 * t_min)), min(cols_per_slice, cols) if cols_per_slice > 0 else min(cols, 16))
    nc_lo = nc_hi if cols_per_slice > 0 else 1
    mg_cap = (min(drives, m) if drives > 0 else m) if m > 0 else 0
    best = None
    for nc0 in range(nc_hi, nc_lo - 1, -1):
        sx = -(-cols // nc0)
        nc = -(-cols // sx)
        for mg0 in range(mg_cap, (1 if m > 0 else 0) - 1, -1):
            ngrp = -(-m // mg0) if m > 0 else 1
            mg = -(-m // ngrp) if m > 0 else 0
            Td, To = unit_columns(mg, True), unit_columns(mg, False)
            W = 2 * nc * (To if ngrp > 1 else Td)
            if W > NBW:
                continue
            npo = ngrp * (ngrp - 1) // 2
            passes = sx * (ngrp * ((2 * nc * (Td if m > 0 else 1) + 15) // 16) + npo * ((2 * nc * To + 15) // 16))
            units = sx * (ngrp + npo)
            if best is None or (passes, units) < (best["passes"], best["U"]):
                best = dict(sx=sx, nc=nc, mg=mg, ngrp=ngrp, U=units, W=W, passes=passes)
    if best is None:  # (nothing fits: what the launch would refuse by its byte count)
        best = dict(sx=cols, nc=1, mg=1 if m > 0 else 0, ngrp=max(m, 1), U=cols * max(m, 1) * (max(m, 1) + 1) // 2, W=2 * t_min, passes=-1)
    return dict(best, LD=LD, threads=threads, NB=NB, NBW=NBW, bytes=(fixed + 3 * LD * best["W"]) * 8)


# ---- cases, multipliers -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name, zero_gv=False):
    """The VarCase, read-only.  zero_gv: every Gv_i read as zero (the same trajectory)."""
    if name != "VH1":
        return vx.case(name, zero_gv)
    cs0 = vh.case("VH1")
    Z = np.array(cs0.Z[:3])
    cs = dataclasses.replace(cs0, Z=Z, N=3)
    for k, s in enumerate(STEPS):
        Z[k, cs.dt_off] = s / le.norm1(vx.g_of(cs, k))
    Z.setflags(write=False)
    if zero_gv:
        cs.Gv = [np.zeros_like(g) for g in cs.Gv]
    return cs


def substeps(cs, k):
    return le.substeps(cs.Z[k, cs.dt_off], vx.g_of(cs, k))


@functools.lru_cache(maxsize=None)
def rand_mu(name):
    cs = case(name)
    mu = np.random.default_rng(vh.seed(name) + 77).standard_normal(cs.K * cs.xd)
    mu.setflags(write=False)
    return mu


def mu_without_variations(name):
    """The same multipliers with zeros on the rows of every variation component."""
    cs = case(name)
    mu = np.array(rand_mu(name)).reshape(cs.K, 1 + cs.v, cs.xdc)
    mu[:, 1:] = 0.0
    return mu.reshape(-1)


def context_args(cs, **kw):
    return vx.context_args(cs, **kw)


def values_per_interval(cs):
    return veh.nnz_per_interval(cs)


# ---- the truth ------------------------------------------------------------------------------------------------------------------------------------------
def _interval_per_drive(G, Gj, h, X, M):
    """exp_hess_truth.interval_values with segment 0 from the per-drive identity (u_l,u_j) = -h <L2(A^T; M X^T, h G_l^T), G_j>."""
    m = len(Gj)
    A = h * G
    E = scipy.linalg.expm(A)
    L = [scipy.linalg.expm_frechet(A, h * Gj[l], compute_expm=False) for l in range(m)]
    F = [eht.frechet2(A.T, M @ X.T, h * Gj[l].T) for l in range(m)]
    seg = [[-h * np.sum(F[i] * Gj[j])] for i in range(m) for j in range(i + 1)]
    seg += [[-np.sum(M * ((Gj[j] @ E + G @ L[j]) @ X))] for j in range(m)]
    seg.append([-np.sum(M * (G @ G @ E @ X))])
    seg += [(-(L[l].T @ M)).T.reshape(-1) for l in range(m)]
    seg.append((-((G @ E).T @ M)).T.reshape(-1))
    return np.concatenate(seg)


def truth_values(cs, mu, intervals=None, per_drive=None):
    """[K, per] in the library's order; the rows of the intervals not asked for are NaN.  per_drive: segment 0 by the per-drive identity
    (default: for m > 6)."""
    Zl, lay, G0l, Gjl = vt.lifted(cs)
    rm = vt._row_map(cs)
    mul = np.asarray(mu, dtype=np.float64).reshape(cs.K, cs.xd)[:, rm]
    per_drive = cs.m > 6 if per_drive is None else per_drive
    f = _interval_per_drive if per_drive else eht.interval_values
    nsc = (cs.m + 1) * (cs.m + 2) // 2
    out = np.full((cs.K, values_per_interval(cs)), np.nan)
    for k in range(cs.K) if intervals is None else intervals:
        G = G0l + np.tensordot(lay.u(Zl, k), Gjl, axes=1) if cs.m else G0l
        vl_ = f(G, Gjl, lay.dt(Zl, k), lay.X(Zl, k), mul[k].reshape(lay.C, lay.n).T)
        out[k, :nsc] = vl_[:nsc]
        S = vl_[nsc:].reshape(cs.m + 1, cs.xd)
        O = np.empty_like(S)
        O[:, rm] = S
        out[k, nsc:] = O.reshape(-1)
    return out


@functools.lru_cache(maxsize=None)
def truth(name, zero_gv=False):
    """[K, per], read-only; NaN rows on the intervals TRUTH_INTERVALS leaves out."""
    out = truth_values(case(name, zero_gv), rand_mu(name), TRUTH_INTERVALS.get(name))
    out.setflags(write=False)
    return out


def intervals(name):
    return list(TRUTH_INTERVALS.get(name, range(case(name).K)))


@functools.lru_cache(maxsize=None)
def structure(name, base=0):
    return veh.structure(case(name), base)


@functools.lru_cache(maxsize=None)
def codes(name):
    """[K, per]: the segment code of every value."""
    cs = case(name)
    a, b = structure(name)
    c = vsc.hess_codes(cs, a, b).reshape(cs.K, -1)
    c.setflags(write=False)
    return c


def segment_names(name):
    cs = case(name)
    return lambda s: vsc.hess_name(cs, s)


def segment_errors(name, vals, want=None, ks=None):
    """{segment: (err, scale)} over the intervals `ks` (default: those with a truth) against `want` (default: the truth)."""
    want = truth(name) if want is None else want
    ks = intervals(name) if ks is None else ks
    ks, K = list(ks), case(name).K
    pick = lambda a: np.asarray(a).reshape(K, -1)[ks].reshape(-1)
    return vsc.segment_errors(pick(codes(name)), pick(vals), pick(want))


def check(name, vals, tol, what="", want=None, ks=None):
    """Every segment within tol of its own maximum (identically-zero segments: exact zeros).  Returns the worst (relative error, segment)."""
    return vsc.assert_segments(segment_errors(name, vals, want, ks), tol, segment_names(name), "%s %s Hessian" % (name, what))


def worst(errors):
    return max((e / s if s else (0.0 if e == 0 else np.inf)) for e, s in errors.values())


def moved(name, good, bad, ks=None):
    """The largest relative change of a segment between two value arrays, over the intervals ks (default: all)."""
    ks = list(range(case(name).K)) if ks is None else ks
    best = 0.0
    for s, (e, scale) in segment_errors(name, bad, good, ks).items():
        if scale > 0:
            best = max(best, e / scale)
    return best


def component_slices(cs):
    """Within the values of all intervals: (index of every scalar and X_0 vector value, index of every X_b vector value, b > 0), and the index of
    the same X_0 values in a plain exponential context's values on component 0."""
    m, xd, xdc, per = cs.m, cs.xd, cs.xdc, values_per_interval(cs)
    nscal = (m + 1) * (m + 2) // 2
    per0 = nscal + xdc * (m + 1)
    seg = np.arange(m + 1)[:, None]
    x0 = np.concatenate([np.arange(nscal), (nscal + seg * xd + np.arange(xdc)[None]).reshape(-1)])
    p0 = np.concatenate([np.arange(nscal), (nscal + seg * xdc + np.arange(xdc)[None]).reshape(-1)])
    xb = (nscal + seg * xd + np.arange(xdc, xd)[None]).reshape(-1)
    k = np.arange(cs.K)[:, None]
    return (k * per + x0[None]).reshape(-1), (k * per + xb[None]).reshape(-1), (k * per0 + p0[None]).reshape(-1)


def component_vectors(cs, b):
    """(index into ONE interval's values of the (u_l, X_b) and (dt, X_b) vectors, index of the same vectors in a plain exponential context's
    values on that component)."""
    m, xd, xdc = cs.m, cs.xd, cs.xdc
    nscal = (m + 1) * (m + 2) // 2
    seg = np.arange(m + 1)[:, None]
    return (nscal + seg * xd + b * xdc + np.arange(xdc)[None]).reshape(-1), (nscal + seg * xdc + np.arange(xdc)[None]).reshape(-1)


# ---- the kernel's recurrence in float64 numpy ---------------------------------------------------------------------------------------------------------
def emulate_hess(cs, mu, passes=None, ks=None, drop_gv_d2w=False, drop_gv_dw=False, drop_cross=False, updated_w=False, drop_substep=False,
                 drop_pass=False, seg1_without_gv=False, drop_col=False):
    """[K, per] in the library's order (rows of the intervals not in ks: zeros): the component-wise recurrence with its passes (None: 0 .. v).
    Faults: drop_gv_d2w leaves Gv_b^T d2W_b out of d2W_0, drop_gv_dw leaves Gv_b^T dW_b out of dW_0, drop_cross leaves the G_l^T dW_b,i cross
    term out of d2W_b,il, updated_w takes Gv_b^T W_b with THIS level's W_b, drop_substep runs s' - 1 of the s' substeps, drop_pass leaves pass v
    out, seg1_without_gv leaves <dW_b,l, Gv_b X_0> out of segment 1, drop_col leaves the last state column out of the sums."""
    n, C, v, m, K = cs.n, cs.C, cs.v, cs.m, cs.K
    mu = np.asarray(mu, dtype=np.float64).reshape(K, 1 + v, C, n)
    pairs = [(i, l) for i in range(m) for l in range(i + 1)]
    npair, nscal = len(pairs), (m + 1) * (m + 2) // 2
    pi, pl = np.array([p[0] for p in pairs], dtype=int), np.array([p[1] for p in pairs], dtype=int)
    GjT = np.array([cs.Gj[l].T for l in range(m)]).reshape(m * n, n) if m else np.zeros((0, n))
    out = np.zeros((K, values_per_interval(cs)))
    sl = slice(0, C - 1) if drop_col else slice(0, C)
    for k in range(K) if ks is None else ks:
        G = vx.g_of(cs, k)
        GT = G.T
        h = cs.Z[k, cs.dt_off]
        s_ = le.substeps(h, G)
        hs = h / s_ if s_ else 0.0
        X = [cs.Z[k, o : o + cs.xdc].reshape(C, n).T for o in cs.xo]
        scal = np.zeros(nscal)
        vec = np.zeros((m + 1, 1 + v, C, n))

        def left(A, B):  # A @ B[q] for every q, [q, n, C]
            return (A @ B.transpose(1, 0, 2).reshape(n, -1)).reshape(n, B.shape[0], C).transpose(1, 0, 2)

        def drive_terms(dW):  # S[i, l] = G_i^T dW_l, [m, m, n, C]
            return (GjT @ dW.transpose(1, 0, 2).reshape(n, m * C)).reshape(m, n, m, C).transpose(0, 2, 1, 3)

        for b in (range(v) if drop_pass else range(1 + v)) if passes is None else passes:
            comps = [0, b] if b else [0]
            GvT = cs.Gv[b - 1].T if b else None
            Y = {cp: np.zeros((n, C)) for cp in comps}
            Y[b] = mu[k, b].T.copy()
            dY = {cp: np.zeros((m, n, C)) for cp in comps}
            d2Y = {cp: np.zeros((npair, n, C)) for cp in comps}
            for _ in range(s_ - 1 if drop_substep else s_):
                W, dW, d2W = Y, dY, d2Y
                for j in range(DEG, 0, -1):
                    f = hs / j
                    Wn, dWn, d2Wn = {}, {}, {}
                    for cp in reversed(comps):  # component b first: component 0 reads its OLD columns (updated_w: the new W_b)
                        tW = GT @ W[cp]
                        tdW = left(GT, dW[cp]) + ((GjT @ W[cp]).reshape(m, n, C) if m else 0.0)
                        if m:
                            S = drive_terms(dW[cp])
                            td2 = left(GT, d2W[cp]) + S[pi, pl] + (0.0 if drop_cross else S[pl, pi])
                        else:
                            td2 = np.zeros((0, n, C))
                        if b and cp == 0:
                            tW = tW + GvT @ (Wn[b] if updated_w else W[b])
                            if not drop_gv_dw:
                                tdW = tdW + left(GvT, dW[b])
                            if not drop_gv_d2w:
                                td2 = td2 + left(GvT, d2W[b])
                        Wn[cp], dWn[cp], d2Wn[cp] = Y[cp] + f * tW, dY[cp] + f * tdW, d2Y[cp] + f * td2
                    W, dW, d2W = Wn, dWn, d2Wn
                Y, dY, d2Y = W, dW, d2W
            for cp in comps:
                GX = G @ X[cp] + (cs.Gv[b - 1] @ X[0] if cp else 0.0)  # (Ghat X')_cp
                GX1 = G @ X[cp] if (cp and seg1_without_gv) else GX
                GTW = GT @ Y[cp] + (GvT @ Y[b] if (b and cp == 0) else 0.0)  # (Ghat^T W')_cp
                for q in range(npair):
                    scal[q] -= np.sum(d2Y[cp][q][:, sl] * X[cp][:, sl])
                for l in range(m):
                    scal[npair + l] -= np.sum(dY[cp][l][:, sl] * GX1[:, sl]) + np.sum(Y[cp][:, sl] * (cs.Gj[l] @ X[cp])[:, sl])
                scal[npair + m] -= np.sum(GTW[:, sl] * GX[:, sl])
                for l in range(m):
                    vec[l, cp] -= dY[cp][l].T
                vec[m, cp] -= GTW.T
        out[k] = np.concatenate([scal, vec.reshape(-1)])
    return out


# ---- what was read on the CPU (tests/test_var_large_exp_hess_cpu.py prints each case's and asserts the bound) --------------------------------------------
# the emulation against the truth, per segment of the project's component-wise segments, worst over the intervals with a truth
# (the worst are (u,u) and (dt,dt) scalars that cancel: VL3's is the (u,u) segment of the long step, 6.5e-9 of 7.9e4)
CPU_READ = {"VL1": 5.5e-15, "VL2": 9.1e-15, "VL3": 8.2e-14, "VL4": 1.9e-14, "VL5": 3.4e-15, "VL6": 4.0e-15, "VH1": 8.1e-16}
CPU_BOUND = 8.2e-13  # asserted: ten times the worst read; below 1e-12, so the GPU rule of 1e-11 per segment keeps a decade

# ---- the finite-difference yardstick of the public-interface test -----------------------------------------------------------------------------------------
FD_EPS = 1e-5
FD_ORACLE = 7.0e-10  # (measured 6.93e-10) what the scipy truth's H v shows against the central difference of the truth's J^T mu on VL1 (re-measured by the CPU test)


def fd_inputs(cs):
    """(mu, v): multipliers and a direction in the variables, seeded."""
    rng = np.random.default_rng(16600)
    return rng.standard_normal(cs.K * cs.xd), rng.standard_normal(cs.N * cs.z_dim)


def fd_error(Hv, jt_mu, z, v):
    """max |H v - (J(z + eps v)^T mu - J(z - eps v)^T mu) / (2 eps)| relative to max |H v|; jt_mu(z) -> J(z)^T mu."""
    quot = (jt_mu(z + FD_EPS * v) - jt_mu(z - FD_EPS * v)) / (2 * FD_EPS)
    return float(np.abs(Hv - quot).max() / np.abs(Hv).max())


def truth_hessian(cs, mu):
    """scipy CSR, symmetric, of the truth's Hessian of the Lagrangian."""
    r, c = veh.structure(cs)
    nv = cs.N * cs.z_dim
    Lw = sp.csr_matrix((truth_values(cs, mu).reshape(-1), (r, c)), shape=(nv, nv))
    return Lw + sp.tril(Lw, -1).T


def fd_oracle_error():
    """The scipy truth's H v against the central difference of the truth's own Jacobian on VL1."""
    cs = case("VL1")
    mu, v = fd_inputs(cs)
    H = truth_hessian(cs, mu)
    r, c = vet.structure(cs)

    def jt_mu(z):
        cz = dataclasses.replace(cs, Z=z.reshape(cs.N, cs.z_dim))
        return sp.csr_matrix((vet.values(cz), (r, c)), shape=(cs.K * cs.xd, cs.N * cs.z_dim)).T @ mu

    return fd_error(H @ v, jt_mu, np.array(cs.Z).reshape(-1), v)
