"""Cases for the variational integrators at generator dimensions 66 .. 128 (contexts created with PCL_BATCH_VARIATIONAL | PCL_LARGE_N |
PCL_LARGE_VAR; piccolo.jl_amd/csrc/pcl_kernel_var_large.hpp, planned by var_large_plan in pcl_host_variational.hpp, restated below); numpy only,
importable without a GPU.

Generators, states, controls and steps are those of tests/variational_shape_cases.py: G(H) of a dense complex Hermitian H / sqrt(d) for the
drift, the drives and the variation generators (the latter divided by the scales 3.0, 0.25) unless stated; state AND variation components
0.4 N(0, 1), u ~ 0.4 N(0, 1); N = 4 with the steps fixed from |Ghat(u_k)|_2 of the LIFTED generator:
    interval 0   h |Ghat|_2 = 0.15
    interval 1   h |Ghat|_2 = -0.3
    interval 2   the long step: the smallest of vector_shape_cases.LONG_STEPS at which zeroing c_5 at order 10 moves the interval's residual by
                 1e-7 of its own size or more
    interval 3   (VL2 only, N = 5) Delta t = 0 exactly: its L blocks and d/du tails must be exact zeros
Seeds: 16000 + 17 index.

Cases (n, state, v, m), the smallest shapes at which each branch of the plan and the kernel can go wrong, and what var_large_plan gives for a
Jacobian launch of the case's intervals (3; VL2: 4) on 256 CUs (sx slices of state columns x ngrp groups of mg drives -- launches of few
intervals take narrower slices: VL2 two columns per slice, VL3 two; pu panel units of npc power
columns per role, 1 + v roles; U workgroups per interval; LDS bytes) -- tests/test_var_large_cpu.py asserts every number against the restatement:
    VL1   66 ket      1  2   first large size: five row tiles, two live rows in the last (Hermitian throughout: the        1 x 1 (2)   5 x 14   U 11    58,992 B
                             public constructors take this system)
    VL2   66 unitary  2  3   33 columns; knot [t | X | Xv1 | Xv2 | dt | u] (odd offsets); drive 2 sparse with empty rows,  17 x 1 (3)  5 x 14   U 32    75,080 B
                             Gv_2 diagonal; the Delta t = 0 interval; several slices; 33 copies of every panel
    VL3   96 unitary  1  4   the qubit-cavity generators of bench/bench_large.py (sparse G: the k-mask skips blocks),      24 x 1 (4)  6 x 16   U 36   119,072 B
                             Gv = the cavity number operator
    VL4  128 ket      2  1   the tightest LDS: 29 blocks beside the tile; one column and one drive per chain unit with     1 x 1 (1)   15 x 9   U 46   161,056 B
                             three components (24 blocks), so the panels (27 blocks) are workgroups of their own
    VL5  120 ket      1 24   drive groups: 24 drives, 8 per group (44 of 47 blocks)                                        1 x 3 (8)   8 x 15   U 19   161,000 B
    VL6   72 ket      2  0   drift only; the drift and Gv_1 carry a decay term (H - i diag gamma), which fills the         1 x 1 (0)   5 x 15   U 16    69,416 B
                             diagonal: row width n for G and for Gv_1
n = 128 unitary (64 columns, 10.5 M values per interval at v = 2): its longdouble truth is 19 M lifted values of 16 bytes per interval and was
left out; VL4 stands for that size, and tests/test_var_large_gpu.py runs the shape once (VL7 below, no truth: every value written, component
0 bitwise against a plain large context).

The truth is vector_shape_cases.truth_values (np.longdouble; no code shared with the library or with oracle/pade_oracle.py's value routines)
on the lifted problem of variational_truth.lifted, brought to the library's value order by value_index, which is checked against the lifted
structure (oracle/pade_oracle.jac_structure through variational_truth's maps) position by position.  Segments are variational_shape_cases'
(row component x variable kind x relative knot x interval).

Reference floor: the float64 lifted oracle (pade_oracle.pade_residual / pade_jacobian_values on the lifted problem) against this truth per
segment, relative to the segment's own maximum, over every case and order: tests/test_var_large_cpu.py asserts 1e-13 -- the floor the
variational sweep documents -- and prints the largest."""
import functools

import numpy as np

import variational_shape_cases as vsc
import variational_truth as vt
import vector_shape_cases as vs
from oracle import pade_oracle as po

LDS_BYTES = 163840
ORDERS = vs.ORDERS
SEEN = vs.SEEN
SCALES = vsc.SCALES
NP_PAIRS = 8  # PL_NP
SLACK = 128  # PL_SLACK
LD_ = np.longdouble

# name: (d, ket, v, m)
CASES = {"VL1": (33, True, 1, 2), "VL2": (33, False, 2, 3), "VL3": (48, False, 1, 4), "VL4": (64, True, 2, 1), "VL5": (60, True, 1, 24),
         "VL6": (36, True, 2, 0)}  # fmt: skip
NAMES = list(CASES)
# what var_large_plan gives for a Jacobian launch of the case's intervals on 256 CUs: (sx, nc, ngrp, mg, pu, npc, U, bytes)
TABLE = {
    "VL1": (1, 1, 1, 2, 5, 14, 11, 58992), "VL2": (17, 2, 1, 3, 5, 14, 32, 75080), "VL3": (24, 2, 1, 4, 6, 16, 36, 119072),
    "VL4": (1, 1, 1, 1, 15, 9, 46, 161056), "VL5": (1, 1, 3, 8, 8, 15, 19, 161000), "VL6": (1, 1, 1, 0, 5, 15, 16, 69416),
}  # fmt: skip
VL7 = (64, False, 2, 1)  # n = 128 unitary, N = 2: no truth (see above)
# the long step of interval 2 per case, h |Ghat|_2: what long_step_search finds (tests/test_var_large_cpu.py runs the search and compares; kept here
# so that building a case does not repeat up to twelve longdouble evaluations of a 384 x 384 lifted problem)
LONG = {"VL1": 0.5, "VL2": 1.5, "VL3": 0.65, "VL4": 1.5, "VL5": 0.5, "VL6": 1.5}


def shape(name):
    """(n, C, v, m)"""
    d, ket, v, m = CASES[name]
    return 2 * d, (1 if ket else d), v, m


# ---- the launch code's arithmetic (var_large_plan, pcl_host_variational.hpp) -------------------------------------------------------------------------
def var_large_plan(n, cols, m, v, jac=True, items=3, n_cu=256, cols_per_slice=0, slices=0, drives=0):
    comp = 1 + v
    LD, threads = n | 1, 64 * ((n + 15) // 16)
    fixed = LD * n + SLACK + m + 8
    NB = (LDS_BYTES // 8 - fixed) // LD
    nc_cap = min(cols_per_slice, cols) if cols_per_slice > 0 else cols
    mg_cap = (min(drives, m) if drives > 0 else m) if jac and m > 0 else 0
    blocks = lambda nc, mg: comp * nc * ((2 + 2 * (2 + mg)) if jac else 4)
    nc = 1
    for c in range(nc_cap, 1, -1):
        if blocks(c, mg_cap) <= NB:
            nc = c
            break
    mg = mg_cap
    while mg > 1 and blocks(nc, mg) > NB:
        mg -= 1
    ngrp = -(-m // mg) if mg_cap > 0 else 1
    if mg_cap > 0:
        mg = -(-m // ngrp)
    sx = -(-cols // nc)
    want_sx = n_cu // max(2 * items * ngrp, 1)
    if want_sx > sx:
        sx = min(want_sx, cols)
    nc = -(-cols // sx)
    sx = -(-cols // nc)
    chain_units, chain_blocks = sx * ngrp, blocks(nc, mg)
    npc = pu = 0
    if jac:
        fits = lambda pu: 3 * -(-n // pu) <= NB and (n * -(-n // pu) + 1) // 2 <= NP_PAIRS * threads
        pu = 1
        while pu < n and not fits(pu):
            pu += 1
        want = slices if slices > 0 else (n + 15) // 16
        pu = max(pu, min(want, n))
        npc = -(-n // pu)
        pu = -(-n // npc)
    pairs = -(-((n * npc + 1) // 2) // threads) if jac else 0
    return dict(LD=LD, threads=threads, NB=NB, sx=sx, nc=nc, ngrp=ngrp, mg=mg, chain_units=chain_units, chain_blocks=chain_blocks, pu=pu, npc=npc,
                U=chain_units + comp * pu, panel_blocks=3 * npc, pairs=pairs, bytes=(fixed + LD * max(chain_blocks, 3 * npc)) * 8)  # fmt: skip


# ---- systems and trajectories ----------------------------------------------------------------------------------------------------------------
def _seed(name):
    return 16000 + 17 * int(name[2:])


def _lower(levels):
    return np.diag(np.sqrt(np.arange(1, levels)), 1).astype(complex)


def qubit_cavity(cavity_levels=12):
    """The dispersive qubit-cavity system of bench/bench_large.py, restated from its docstring (rotating frame, rad / ns): (H0, four drive
    Hamiltonians, the cavity number operator) on 4 transmon levels x cavity_levels."""
    two_pi = 2.0 * np.pi
    alpha, chi, kerr = -two_pi * 0.2, -two_pi * 0.002, -two_pi * 1e-5
    b, a = np.kron(_lower(4), np.eye(cavity_levels)), np.kron(np.eye(4), _lower(cavity_levels))
    bd, ad = b.conj().T, a.conj().T
    H0 = 0.5 * alpha * bd @ bd @ b @ b + chi * (ad @ a) @ (bd @ b) + 0.5 * kerr * ad @ ad @ a @ a
    return H0, [b + bd, 1j * (bd - b), a + ad, 1j * (ad - a)], ad @ a


@functools.lru_cache(maxsize=None)
def hamiltonians(name):
    """(H0, [H_l], [Hv_i]) of the case, d x d complex; the variation generators are G(Hv_i) / SCALES[i]."""
    d, ket, v, m = CASES[name] if name in CASES else VL7
    rng = np.random.default_rng(_seed(name))
    H0 = vsc._herm(d, rng)
    Hd = [vsc._herm(d, rng) for _ in range(m)]
    Hv = [vsc._herm(d, rng) for _ in range(v)]
    if name == "VL6":  # a decay term fills the diagonal of the Im H blocks: row width n for G and for Gv_1
        H0 = H0 - 1j * np.diag(0.2 * (0.5 + rng.random(d)))
        Hv[0] = Hv[0] - 1j * np.diag(0.2 * (0.5 + rng.random(d)))
    if name == "VL2":
        S = np.zeros((d, d), dtype=complex)  # drive 2: five entries, most rows (and columns) empty
        S[0, 1], S[1, 0], S[3, 3], S[7, 32], S[32, 7] = 0.7 - 0.4j, 0.7 + 0.4j, -0.9, 0.5j, -0.5j
        Hd[2] = S
        Hv[1] = np.diag(rng.standard_normal(d))  # Gv_2: one entry per row
    if name == "VL3":
        H0, Hd, num = qubit_cavity(d // 4)
        Hv = [num * SCALES[0]]  # (Gv_1 = G(a'a) after the division by the scale)
    return H0, Hd, Hv


@functools.lru_cache(maxsize=None)
def system(name):
    """(G0, Gj [m, n, n], [Gv_i]) -- the variation generators already divided by their scales."""
    H0, Hd, Hv = hamiltonians(name)
    n, m = 2 * H0.shape[0], len(Hd)
    G0 = po.G_of_H(H0)
    Gj = np.array([po.G_of_H(H) for H in Hd]).reshape(m, n, n)
    Gv = [po.G_of_H(H) / s for H, s in zip(Hv, SCALES)]
    for a in [G0, Gj] + Gv:
        a.setflags(write=False)
    return G0, Gj, Gv


def knot(name):
    """(N, z_dim, xo, dt_off, u_off) -- [X | Xv_1 .. | dt | t | u]; VL2: [t | X | Xv1 | Xv2 | dt | u], N = 5; VL7: N = 2."""
    n, C, v, m = shape(name) if name in CASES else (2 * VL7[0], VL7[0], VL7[2], VL7[3])
    xdc = n * C
    if name == "VL2":
        return 5, 1 + (v + 1) * xdc + 1 + m, [1 + b * xdc for b in range(v + 1)], 1 + (v + 1) * xdc, 2 + (v + 1) * xdc
    return (2 if name == "VL7" else 4), (v + 1) * xdc + 2 + m, [b * xdc for b in range(v + 1)], (v + 1) * xdc, (v + 1) * xdc + 2


@functools.lru_cache(maxsize=None)
def case(name):
    """(VarCase, long step), read-only."""
    n, C, v, m = shape(name)
    G0, Gj, Gv = system(name)
    N, z_dim, xo, dt_off, u_off = knot(name)
    rng = np.random.default_rng(_seed(name) + 1)
    Z = 0.4 * rng.standard_normal((N, z_dim))
    cs = vt.VarCase(Z=Z, z_dim=z_dim, N=N, n=n, C=C, m=m, xo=xo, u_off=u_off, dt_off=dt_off, G0=G0, Gv=Gv, Gj=Gj)
    n2 = [vsc._lifted_norm(cs, k) for k in range(3)]
    Z[:, dt_off] = 0.1
    Z[0, dt_off], Z[1, dt_off] = 0.15 / n2[0], -0.3 / n2[1]
    if N == 5:
        Z[3, dt_off] = 0.0
    long_step = LONG[name]
    Z[2, dt_off] = long_step / n2[2]
    t_off = 0 if name == "VL2" else dt_off + 1
    Z[:, t_off] = np.cumsum(Z[:, dt_off])
    Z.setflags(write=False)
    return cs, long_step


def long_step_search(name):
    """The smallest of vector_shape_cases.LONG_STEPS at which zeroing c_5 at order 10 moves interval 2's residual by SEEN of its own size or more
    (None: no such step), and the weights read on the way."""
    cs, _ = case(name)
    Z = np.array(cs.Z)
    norm = abs(cs.Z[2, cs.dt_off]) / LONG[name]  # 1 / |Ghat(u_2)|_2
    seen = {}
    for s in vs.LONG_STEPS:
        Z[2, cs.dt_off] = s * norm
        Zl, lay, G0l, Gjl = vt.lifted(vt.VarCase(**{**cs.__dict__, "Z": Z}))
        seen[s] = vs.top_term_weight(lay, G0l, Gjl, Zl)
        if seen[s] >= SEEN:
            return s, seen
    return None, seen


def case_vl7():
    """n = 128 unitary, v = 2, m = 1, one interval at h |Ghat|_2 = 0.3: the largest value count the ABI admits per interval (no truth)."""
    d, ket, v, m = VL7
    n, C = 2 * d, d
    G0, Gj, Gv = system("VL7")
    N, z_dim, xo, dt_off, u_off = knot("VL7")
    Z = 0.4 * np.random.default_rng(_seed("VL7") + 1).standard_normal((N, z_dim))
    cs = vt.VarCase(Z=Z, z_dim=z_dim, N=N, n=n, C=C, m=m, xo=xo, u_off=u_off, dt_off=dt_off, G0=G0, Gv=Gv, Gj=Gj)
    Z[:, dt_off] = 0.3 / vsc._lifted_norm(cs, 0)
    Z[:, dt_off + 1] = np.cumsum(Z[:, dt_off])
    return cs


def context_args(cs, order, **kw):
    """Keyword arguments of piccolo_jl_amd.integrators._PclContext for a case (batch_mode and the flags are the caller's)."""
    args = dict(d=cs.n // 2, m=cs.m, N=cs.N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=list(cs.xo),
                G0=np.concatenate([cs.G0[None]] + [g[None] for g in cs.Gv]), Gj=cs.Gj, batch=1 + cs.v, per_member_G0=True, pade_order=order,
                state_cols=cs.C)  # fmt: skip
    args.update(kw)
    return args


# ---- the library's structure and value order, restated from include/piccolo_hip.h (PCL_BATCH_VARIATIONAL) ----------------------------------------
def values_per_interval(cs):
    return (2 + 4 * cs.v) * cs.C * cs.n * cs.n + cs.xd * (cs.m + 1)


@functools.lru_cache(maxsize=None)
def _interval_layout(n, C, v, m):
    """Per value of one interval, in the library's order: (row within the interval, column kind, column offset, lifted value index).  Column kind:
    0 a state entry of knot k (offset: component b, then the entry), 1 of knot k + 1, 2 the variable u_l / dt of knot k (offset l, m = dt)."""
    nl, xdc = (1 + v) * n, n * C
    cc, j, i = np.meshgrid(np.arange(C), np.arange(n), np.arange(n), indexing="ij")
    cc, j, i = cc.reshape(-1), j.reshape(-1), i.reshape(-1)
    rows, kind, comp, off, lifted = [], [], [], [], []

    def block(brow, bcol, knt):
        rows.append(brow * xdc + cc * n + i)
        kind.append(np.full(cc.shape, knt))
        comp.append(np.full(cc.shape, bcol))
        off.append(cc * n + j)
        lifted.append(knt * C * nl * nl + cc * nl * nl + (bcol * n + j) * nl + (brow * n + i))

    block(0, 0, 0)
    block(0, 0, 1)
    for b in range(1, v + 1):
        block(b, b, 0)
        block(b, b, 1)
        block(b, 0, 0)
        block(b, 0, 1)
    b_, c_, l_, i_ = [a.reshape(-1) for a in np.meshgrid(np.arange(v + 1), np.arange(C), np.arange(m + 1), np.arange(n), indexing="ij")]
    rows.append(b_ * xdc + c_ * n + i_)
    kind.append(np.full(b_.shape, 2))
    comp.append(np.zeros(b_.shape, dtype=np.int64))
    off.append(l_)
    lifted.append(2 * C * nl * nl + (c_ * (m + 1) + l_) * nl + b_ * n + i_)
    out = tuple(np.concatenate(a).astype(np.int64) for a in (rows, kind, comp, off, lifted))
    for a in out:
        a.setflags(write=False)
    return out


def lib_structure(cs):
    """(rows, cols), index base 0, of every Jacobian value in the library's order."""
    r, kind, comp, off, _ = _interval_layout(cs.n, cs.C, cs.v, cs.m)
    xo = np.asarray(cs.xo)
    col_in_knot = np.where(kind < 2, xo[comp] + off, np.where(off < cs.m, cs.u_off + off, cs.dt_off))
    knot_of = np.where(kind == 1, 1, 0)
    k = np.arange(cs.K)[:, None]
    return (k * cs.xd + r[None]).reshape(-1), ((k + knot_of[None]) * cs.z_dim + col_in_knot[None]).reshape(-1)


def value_index(cs):
    """Index into ONE interval's lifted Jacobian values (truth_values' order for variational_truth.lifted's layout) of every value of the
    library's order."""
    return _interval_layout(cs.n, cs.C, cs.v, cs.m)[4]


def lifted_values(name, order, zero_last_variation=False, gv_k_below=None, **kw):
    """vector_shape_cases.truth_values on the lifted problem, in longdouble: (delta [K xd] in stacked order, the Jacobian values [K, per] in
    the library's order, what of the lifted values the library's structure does not hold).  kw: truth_values' switches (c, drop_drive, drop_col,
    intervals); zero_last_variation: Gv_v read as zero; gv_k_below: the columns of every Gv_i from that index on read as zero."""
    cs, _ = case(name)
    Zl, lay, G0l, Gjl = vt.lifted(cs)
    if zero_last_variation or gv_k_below is not None:
        G0l = np.array(G0l)
        if zero_last_variation:
            G0l[cs.v * cs.n :, : cs.n] = 0
        if gv_k_below is not None:
            G0l[cs.n :, gv_k_below : cs.n] = 0
    d, j, _ = vs.truth_values(lay, G0l, Gjl, Zl, None, order, hessian=False, **kw)
    ds = np.empty_like(d)
    ds[:, vt._row_map(cs)] = d
    vi = value_index(cs)
    rest = np.ones(j.shape[1], dtype=bool)
    rest[vi] = False
    return ds.reshape(-1), j[:, vi], j[:, rest]


@functools.lru_cache(maxsize=None)
def truth_ld(name, order):
    """(delta, Jacobian values in the library's order), flat, in longdouble; computed once and never written to."""
    d, j, rest = lifted_values(name, order)
    assert not np.any(rest)  # the library's structure holds every non-zero of the lifted problem
    out = (d, j.reshape(-1))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truth(name, order):
    """The same rounded to float64: what the GPU tests compare with."""
    out = tuple(a.astype(np.float64) for a in truth_ld(name, order))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def codes(name):
    """(segment code of every residual row, of every Jacobian value): variational_shape_cases.residual_codes / jac_codes."""
    cs, _ = case(name)
    r, c = lib_structure(cs)
    out = (vsc.residual_codes(cs, np.arange(cs.K * cs.xd)), vsc.jac_codes(cs, r, c))
    for a in out:
        a.setflags(write=False)
    return out


def check(name, order, delta, vals, tol, what=""):
    """Every segment of delta and of the Jacobian values within tol of its own size (identically-zero segments: exact zeros).  Returns the
    worst (relative error, segment) of each."""
    cs, _ = case(name)
    d, j = truth(name, order)
    dc, jc = codes(name)
    wd = vsc.assert_segments(vsc.segment_errors(dc, delta, d), tol, lambda s: vsc.residual_name(cs, s), "%s order %d %s residual" % (name, order, what))
    wj = vsc.assert_segments(vsc.segment_errors(jc, vals, j), tol, lambda s: vsc.jac_name(cs, s), "%s order %d %s Jacobian" % (name, order, what))
    return wd, wj


def component0(cs):
    """What of a variational context's outputs a plain context of (G0, Gj) on component 0 also computes: (index into the stacked delta, index
    into the plain delta), and the same for the Jacobian values -- delta_0, the -B+ | B- copies of EVERY component, component 0's tails."""
    n, C, v, m, K = cs.n, cs.C, cs.v, cs.m, cs.K
    xdc, nn = n * C, n * n
    per, per0 = values_per_interval(cs), 2 * C * nn + xdc * (m + 1)
    k = np.arange(K)[:, None]
    dv, d0 = (k * cs.xd + np.arange(xdc)[None]).reshape(-1), (k * xdc + np.arange(xdc)[None]).reshape(-1)
    blk = np.arange(2 * C * nn)
    src = [blk] + [(4 * b - 2) * C * nn + blk for b in range(1, v + 1)] + [(2 + 4 * v) * C * nn + np.arange(xdc * (m + 1))]
    dst = [blk] * (1 + v) + [2 * C * nn + np.arange(xdc * (m + 1))]
    src, dst = np.concatenate(src), np.concatenate(dst)
    return dv, d0, (k * per + src[None]).reshape(-1), (k * per0 + dst[None]).reshape(-1)
