"""Cases for the variational exponential constraint at generator dimensions 66 .. 128 (contexts created with PCL_BATCH_VARIATIONAL_EXP |
PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP and pade_order = PCL_ORDER_EXP; piccolo.jl_amd/csrc/pcl_kernel_var_large_exp.hpp, planned by
var_large_exp_plan in pcl_host_variational.hpp, restated below); numpy and scipy only, importable without a GPU.

Systems, knots, states and controls are those of VL1 .. VL6 of tests/var_large_cases.py (the case table and the branch each case sits on are
there); the steps are set from |G(u_k)|_1 of the n x n generator, as in tests/large_exp_cases.py, because the kernel's substep count is
s' = ceil(|h| |G(u_k)|_1):
    interval 0   h |G|_1 = 0.8    (s' = 1)
    interval 1   h |G|_1 = -2.5   (s' = 3, a negative step)
    interval 2   the long step LONG[name], s' >= 20
    interval 3   (VL2 only, N = 5) h = 0 exactly: s' = 0, E = I, L_i = 0 and the drive tails exact zeros
VL7 (n = 128 unitary, v = 2, one interval at h |G|_1 = 0.8) has no truth: 10.5 M values per interval; the GPU test runs the shape once.

What var_large_exp_plan gives for a Jacobian launch (it does not depend on the interval count): sx slices of nc state columns x ngrp groups of mg
drives, all 1 + v components in a unit; pu panel units of npc columns of the identity; U workgroups per interval; W columns per buffer; 16-column
passes per interval and level; LDS bytes -- tests/test_var_large_exp_cpu.py asserts every number against the restatement:
            n   state   v  m     sx x nc   ngrp x mg   pu x npc    U    W  passes    bytes
    VL1    66   ket     1  2      1 x 1     1 x 2       9 x 8     10   16      10    62,208
    VL2    66   unitary 2  3      9 x 4     1 x 3      14 x 5     23   48      41   113,672
    VL3    96   unitary 1  4     16 x 3     1 x 4      12 x 8     28   30      44   145,456
    VL4   128   ket     2  1      1 x 1     1 x 1      43 x 3     44    9      44   161,056
    VL5   120   ket     1 24      1 x 1     4 x 6      18 x 7     22   14      22   158,096
    VL6    72   ket     2  0      1 x 1     1 x 0      15 x 5     16   15      16    69,416
n = 128 unitary with m = 24 and v = 2, the tightest of all: 64 x 1 slices, 12 x 2 groups, 43 x 3 panels, W = 9, 161,240 B.

Truth: var_exp_truth.residual / .values -- scipy's expm / expm_frechet on the lifted generator, no code shared with the recurrence.  Segments are
those of tests/variational_shape_cases.py (row component x variable kind x relative knot x interval).  `emulate` is the kernel's recurrence in
float64 numpy with every product through one `mm` hook; its faults are the mutants tests/test_var_large_exp_cpu.py must see."""
import functools

import numpy as np

import large_exp_cases as le
import large_shape_cases as lc
import var_exp_truth as vet
import var_large_cases as vl
import variational_shape_cases as vsc
import variational_truth as vt
from oracle import pade_oracle as po

LDS_BYTES = vl.LDS_BYTES
SLACK = vl.SLACK
DEG = le.DEG  # LR_DEG
SMAX = le.SMAX  # LR_SMAX
NAMES = vl.NAMES
STEPS = le.STEPS
LONG = {"VL1": 20.5, "VL2": 27.3, "VL3": 33.7, "VL4": 24.1, "VL5": 38.9, "VL6": 21.2}
LD_ = np.longdouble
# what var_large_exp_plan gives for a Jacobian launch: (sx, nc, ngrp, mg, pu, npc, U, W, passes, bytes)
TABLE = {
    "VL1": (1, 1, 1, 2, 9, 8, 10, 16, 10, 62208), "VL2": (9, 4, 1, 3, 14, 5, 23, 48, 41, 113672), "VL3": (16, 3, 1, 4, 12, 8, 28, 30, 44, 145456),
    "VL4": (1, 1, 1, 1, 43, 3, 44, 9, 44, 161056), "VL5": (1, 1, 4, 6, 18, 7, 22, 14, 22, 158096), "VL6": (1, 1, 1, 0, 15, 5, 16, 15, 16, 69416),
}  # fmt: skip


# ---- the launch code's arithmetic (var_large_exp_plan, pcl_host_variational.hpp) ------------------------------------------------------------------
def _even_split(total, per):
    cnt = -(-total // per)
    return cnt, -(-total // cnt)


def var_large_exp_plan(n, cols, m, v, jac=True, cols_per_slice=0, slices=0, drives=0):
    comp = 1 + v
    LD, threads = n | 1, 64 * ((n + 15) // 16)
    fixed = LD * n + SLACK + m + 8
    NB = (LDS_BYTES // 8 - fixed) // LD
    NBW = NB // 3
    drv = jac and m > 0
    nc_cap = min(cols_per_slice, cols) if cols_per_slice > 0 else min(cols, 16)
    mg_cap = (min(drives, m) if drives > 0 else m) if drv else 0
    pick = dict(nc=1, mg=1 if drv else 0, ngrp=m if drv else 1, sx=cols)
    best = None
    for nc0 in range(nc_cap, 0, -1):
        for mg0 in range(mg_cap, (1 if drv else 0) - 1, -1):
            sx, nc = _even_split(cols, nc0)
            ngrp, mg = _even_split(m, mg0) if drv else (1, mg0)
            cx = comp * nc * (1 + mg)
            if cx > NBW:
                continue
            units = sx * ngrp
            key = (units * -(-cx // 16), units)
            if best is None or key < best:
                best, pick = key, dict(nc=nc, mg=mg, ngrp=ngrp, sx=sx)
    nc, mg, ngrp, sx = pick["nc"], pick["mg"], pick["ngrp"], pick["sx"]
    chain_units = sx * ngrp
    npc = pu = 0
    if jac:
        npc_fit = max(1, min(n, min(NBW, 16) // comp))
        pu = -(-n // npc_fit)
        if slices > 0:
            pu = max(pu, min(slices, n))
        npc = -(-n // pu)
        pu = -(-n // npc)
    cx = comp * nc * (1 + mg)
    W = max(cx, comp * npc)
    passes = chain_units * -(-cx // 16) + pu * -(-(comp * npc) // 16)
    return dict(LD=LD, threads=threads, NB=NB, NBW=NBW, sx=sx, nc=nc, ngrp=ngrp, mg=mg, chain_units=chain_units, chain_cols=cx, pu=pu, npc=npc,
                panel_cols=comp * npc, U=chain_units + pu, W=W, passes=passes, bytes=(fixed + 3 * LD * W) * 8)  # fmt: skip


# ---- trajectories --------------------------------------------------------------------------------------------------------------------------------
def g_of(cs, k):
    u = cs.Z[k, cs.u_off : cs.u_off + cs.m]
    return cs.G0 + np.tensordot(u, cs.Gj, axes=1) if cs.m else np.array(cs.G0)


def _with_steps(cs0, steps):
    Z = np.array(cs0.Z)
    cs = vt.VarCase(**{**cs0.__dict__, "Z": Z})
    for k, s in steps.items():
        Z[k, cs.dt_off] = s / le.norm1(g_of(cs, k)) if s else 0.0
    Z.setflags(write=False)
    return cs


@functools.lru_cache(maxsize=None)
def case(name, zero_gv=False):
    """The VarCase, read-only.  zero_gv: every Gv_i read as zero (the same trajectory)."""
    cs0, _ = vl.case(name)
    steps = {0: STEPS[0], 1: STEPS[1], 2: LONG[name]}
    if cs0.N == 5:
        steps[3] = 0.0
    cs = _with_steps(cs0, steps)
    if zero_gv:
        cs.Gv = [np.zeros_like(g) for g in cs.Gv]
    return cs


def case_vl7():
    """n = 128 unitary, v = 2, m = 1, one interval at h |G|_1 = 0.8 (no truth)."""
    return _with_steps(vl.case_vl7(), {0: STEPS[0], 1: 0.1})


def substeps(cs, k):
    return le.substeps(cs.Z[k, cs.dt_off], g_of(cs, k))


def context_args(cs, **kw):
    """Keyword arguments of piccolo_jl_amd.integrators._PclContext for a case (batch_mode and the flags are the caller's)."""
    return vl.context_args(cs, "exp", **kw)


# ---- the truth: scipy on the lifted generator, computed once and never written to -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def truth(name, zero_gv=False):
    """(delta, Jacobian values), flat, in the library's order."""
    cs = case(name, zero_gv)
    out = (vet.residual(cs), vet.values(cs))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def codes(name):
    """(segment code of every residual row, of every Jacobian value)."""
    cs = case(name)
    r, c = vet.structure(cs)
    out = (vsc.residual_codes(cs, np.arange(cs.K * cs.xd)), vsc.jac_codes(cs, r, c))
    for a in out:
        a.setflags(write=False)
    return out


def segment_reads(name, delta, vals, ref=None):
    """({segment: (err, scale)} of delta, of the values) against `ref` (default: the truth)."""
    d, j = truth(name) if ref is None else ref
    dc, jc = codes(name)
    return vsc.segment_errors(dc, delta, d), vsc.segment_errors(jc, vals, j)


def check(name, delta, vals, tol, what="", ref=None):
    """Every segment of delta and of the values within tol of its own maximum (identically-zero segments: exact zeros).  Returns the worst
    (relative error, segment) of each."""
    cs = case(name)
    ed, ej = segment_reads(name, delta, vals, ref)
    wd = vsc.assert_segments(ed, tol, lambda s: vsc.residual_name(cs, s), "%s %s residual" % (name, what))
    wj = vsc.assert_segments(ej, tol, lambda s: vsc.jac_name(cs, s), "%s %s Jacobian" % (name, what))
    return wd, wj


def moved(name, good, bad):
    """The largest relative change of a segment (residual or Jacobian) between two (delta, values) pairs."""
    dc, jc = codes(name)
    return max(vsc.moved(dc, good[0], bad[0]), vsc.moved(jc, good[1], bad[1]))


# ---- the kernel's recurrence in float64 numpy -----------------------------------------------------------------------------------------------------
def emulate(cs, mm=np.matmul, drop_gv_dv=False, drop_gl_vv=False, updated_v=False, drop_substep=False, drop_drive=False, dt_without_gv=False):
    """(delta, values), flat, in the library's order.  Faults: drop_gv_dv leaves Gv_i dV_l out of dVv_il, drop_gl_vv leaves G_l Vv_i out of it,
    updated_v takes Gv_i V with the V of THIS level, drop_substep runs s' - 1 of the s' substeps, drop_drive leaves the last drive out of G(u) and
    of the tails, dt_without_gv leaves Gv_i Y out of component i's dt tail."""
    n, C, v, m, K = cs.n, cs.C, cs.v, cs.m, cs.K
    me = m - 1 if drop_drive else m
    Gj, Gv = cs.Gj, cs.Gv
    delta, vals = [], []
    for k in range(K):
        u = cs.Z[k, cs.u_off : cs.u_off + m]
        G = cs.G0 + np.tensordot(u[:me], Gj[:me], axes=1) if me else np.array(cs.G0)
        h = cs.Z[k, cs.dt_off]
        sp = le.substeps(h, G)
        hs = h / sp if sp else 0.0
        X = [cs.Z[k, o : o + cs.xdc].reshape(C, n).T for o in cs.xo]
        X1 = [cs.Z[k + 1, o : o + cs.xdc].reshape(C, n).T for o in cs.xo]
        # the state columns and the panel of the identity side by side: [X | I], [Xv_i | 0]
        Y = [np.hstack([X[0], np.eye(n)])] + [np.hstack([X[b], np.zeros((n, n))]) for b in range(1, 1 + v)]
        dY = np.zeros((1 + v, n, m * C))  # column l C + c: the derivative along drive l of state column c
        GjS = Gj.reshape(m * n, n)[: me * n]  # the drives stacked by rows: ONE product gives every G_l V
        on = me * C

        def drives(Vc):  # [G_0 Vc | G_1 Vc | ..] as n x (me C)
            return mm(GjS, Vc).reshape(me, n, C).transpose(1, 0, 2).reshape(n, on)

        for _ in range(sp - 1 if drop_substep else sp):
            V, dV = Y, dY
            for j in range(DEG, 0, -1):
                f = hs / j
                Vn = [Y[0] + f * mm(G, V[0])]
                for b in range(1, 1 + v):
                    Vn.append(Y[b] + f * (mm(G, V[b]) + mm(Gv[b - 1], Vn[0] if updated_v else V[0])))
                dVn = np.array(dY)
                if me:
                    dVn[0, :, :on] = dY[0, :, :on] + f * (mm(G, dV[0, :, :on]) + drives(V[0][:, :C]))
                    for b in range(1, 1 + v):
                        t = mm(G, dV[b, :, :on])
                        if not drop_gv_dv:
                            t = t + mm(Gv[b - 1], dV[0, :, :on])
                        if not drop_gl_vv:
                            t = t + drives(V[b][:, :C])
                        dVn[b, :, :on] = dY[b, :, :on] + f * t
                V, dV = Vn, dVn
            Y, dY = V, dV
        dY = dY.reshape(1 + v, n, m, C).transpose(0, 2, 1, 3)  # [b, l, i, c]
        delta.append(np.concatenate([(X1[b] - Y[b][:, :C]).T.reshape(-1) for b in range(1 + v)]))
        dt = [mm(G, Y[0][:, :C])]
        for b in range(1, 1 + v):
            dt.append(mm(G, Y[b][:, :C]) + (0.0 if dt_without_gv else mm(Gv[b - 1], Y[0][:, :C])))
        E = np.tile(-Y[0][:, C:].T.reshape(-1), C)
        blocks = [E]
        for b in range(1, 1 + v):
            blocks += [E, np.tile(-Y[b][:, C:].T.reshape(-1), C)]
        tails = [np.concatenate([-dY[b, l, :, c] for l in range(m)] + [-dt[b][:, c]]) for b in range(1 + v) for c in range(C)]
        vals.append(np.concatenate(blocks + [np.ones(cs.xd)] + tails))
    return np.concatenate(delta), np.concatenate(vals)


# ---- faults of the products, through the `mm` hook -----------------------------------------------------------------------------------------------
mm_zero_last_row_tile = lc.mm_zero_last_row_tile


# ---- scipy's own floor: an np.longdouble scaled Taylor series of the lifted matrix -------------------------------------------------------------------
def _expm_ld(A):
    """exp(A) in longdouble: A / 2^s with |A / 2^s|_1 <= 1/4, the Taylor series to degree 22 (remainder (1/4)^23 / 23! < 1e-36), s squarings."""
    A = np.asarray(A, dtype=LD_)
    nrm = float(np.abs(A).sum(axis=0).max())
    s = max(0, int(np.ceil(np.log2(nrm / 0.25)))) if nrm > 0.25 else 0
    B = A / LD_(2**s)
    E = np.eye(A.shape[0], dtype=LD_)
    T = np.eye(A.shape[0], dtype=LD_)
    for j in range(1, 23):
        T = (T @ B) / LD_(j)
        E = E + T
    for _ in range(s):
        E = E @ E
    return E


def _frechet_action_ld(A, B, x):
    """L(A, B) x in longdouble, L the Frechet derivative of exp at A along B: the Taylor series of exp([[A, 0], [B, A]]) applied to [x; 0] in
    ceil(4 |A|_1) substeps of degree 22 (action form: the 2 x 2 block matrix is never formed)."""
    A, B = np.asarray(A, dtype=LD_), np.asarray(B, dtype=LD_)
    nrm = float(np.abs(A).sum(axis=0).max())
    s = max(1, int(np.ceil(4 * nrm)))
    A, B = A / LD_(s), B / LD_(s)
    y, dy = np.asarray(x, dtype=LD_), np.zeros(x.shape, dtype=LD_)
    for _ in range(s):
        t, dt, ys, dys = y, dy, y, dy
        for j in range(1, 23):
            t, dt = (A @ t) / LD_(j), (A @ dt + B @ t) / LD_(j)
            ys, dys = ys + t, dys + dt
        y, dy = ys, dys
    return dy


def truth_ld(name):
    """(delta, Jacobian values) in np.longdouble, flat, in the library's order, from the lifted matrix Ghat = var_G(G(u_k), [Gv_i]): exp(h Ghat)
    by _expm_ld (its first block column is [E; L_1; ..]), the dt tail -Ghat exp(h Ghat) xhat, the drive tails by _frechet_action_ld with
    I (x) G_l.  Shares no code with scipy, with the oracle's value routines or with `emulate`."""
    cs = case(name)
    n, C, v, m, K = cs.n, cs.C, cs.v, cs.m, cs.K
    delta, vals = [], []
    for k in range(K):
        h = LD_(cs.Z[k, cs.dt_off])
        Gh = np.asarray(po.var_G(g_of(cs, k), list(cs.Gv)), dtype=LD_)
        xh = np.vstack([cs.Z[k, o : o + cs.xdc].reshape(C, n).T for o in cs.xo]).astype(LD_)  # [(1 + v) n, C]
        x1 = np.vstack([cs.Z[k + 1, o : o + cs.xdc].reshape(C, n).T for o in cs.xo]).astype(LD_)
        Eh = _expm_ld(h * Gh)
        yh = Eh @ xh
        delta.append(np.concatenate([(x1 - yh)[b * n : (b + 1) * n].T.reshape(-1) for b in range(1 + v)]))
        dt = -(Gh @ yh)
        dr = [-_frechet_action_ld(h * Gh, h * np.kron(np.eye(1 + v), cs.Gj[l]), xh) for l in range(m)]
        E = np.tile(-Eh[:n, :n].T.reshape(-1), C)
        blocks = [E]
        for b in range(1, 1 + v):
            blocks += [E, np.tile(-Eh[b * n : (b + 1) * n, :n].T.reshape(-1), C)]
        tails = [np.concatenate([dr[l][b * n : (b + 1) * n, c] for l in range(m)] + [dt[b * n : (b + 1) * n, c]]) for b in range(1 + v) for c in range(C)]
        vals.append(np.concatenate(blocks + [np.ones(cs.xd, dtype=LD_)] + tails))
    return np.concatenate(delta), np.concatenate(vals)


# ---- what a plain PCL_LARGE_N | PCL_LARGE_EXP context of (G0, Gj) on one component also computes ------------------------------------------------------
def component_vs_plain(cs, b=0):
    """(index into the stacked delta, into the plain delta, into the values, into the plain values): delta_b, component b's tails and -- for
    b = 0 the -E copies of EVERY component, for b > 0 the copy of block (b, b) -- against a plain large exponential context whose state is
    component b."""
    n, C, v, m, K = cs.n, cs.C, cs.v, cs.m, cs.K
    xdc, nn = n * C, n * n
    per, per0 = vet.nnz_per_interval(cs), C * nn + xdc * (m + 2)
    k = np.arange(K)[:, None]
    dv, d0 = (k * cs.xd + b * xdc + np.arange(xdc)[None]).reshape(-1), (k * xdc + np.arange(xdc)[None]).reshape(-1)
    blk = np.arange(C * nn)
    e_blocks = [0] + [2 * i - 1 for i in range(1, v + 1)] if b == 0 else [2 * b - 1]
    ones0, tails0 = (1 + 2 * v) * C * nn, (1 + 2 * v) * C * nn + cs.xd
    src = [e * C * nn + blk for e in e_blocks] + [ones0 + b * xdc + np.arange(xdc), tails0 + b * xdc * (m + 1) + np.arange(xdc * (m + 1))]
    dst = [blk] * len(e_blocks) + [C * nn + np.arange(xdc), C * nn + xdc + np.arange(xdc * (m + 1))]
    src, dst = np.concatenate(src), np.concatenate(dst)
    return dv, d0, (k * per + src[None]).reshape(-1), (k * per0 + dst[None]).reshape(-1)
