"""Cases that walk the Pade variational kernels (batch_mode PCL_BATCH_VARIATIONAL: pcl_kernel_variational.hpp, launched by
pcl_host_variational.hpp) over the sizes, drives and wave counts at which they branch; numpy only, importable without a GPU.

Generators are dense: G(H) of a dense complex Hermitian H / sqrt(d) for the drift, the drives and the variation generators, the latter divided
by the scales (3.0, 0.25).  The state AND the variation components are random O(1) (0.4 N(0, 1)), so every segment carries weight; u ~ 0.4
N(0, 1); N = 4.  The steps are fixed per case from |Ghat(u_k)|_2 of the LIFTED generator, as tests/vector_shape_cases.py does:
    interval 0   h |Ghat|_2 = 0.15
    interval 1   h |Ghat|_2 = -0.3
    interval 2   the long step: the smallest of vector_shape_cases.LONG_STEPS at which zeroing c_5 at order 10 moves the interval's residual by
                 1e-7 of its own size or more (1e4 x the GPU tolerance)
    interval 3   (W2 only, N = 5) Delta t = 0 exactly

Cases (d, n, state, v, m), what each straddles, and the waves w per workgroup of pcl_var_hess_kernel at orders 2 / 4 / 6 / 8 / 10:
    W1   16 32 unitary 1  2   512 value pairs: the first pair slot exactly full, none beyond; two column workgroups of 8       8/8/8/8/8
    W2   17 34 unitary 2  3   578 pairs: 66 threads in slot 2; C = 17: column workgroups of 5 / 6 / 6 columns; knot               8/8/8/7/6
                              [t | X | Xv1 | Xv2 | dt | u] (odd state offsets); drive 2 sparse with empty rows and Gv_2 diagonal
                              (wD, wV padding); the Delta t = 0 interval; a last Hessian pass with idle waves (17 mod 7 = 3, 17 mod 6 = 5)
    W3   22 44 ket     2  1   968 pairs: slot 2 almost full (456 of 512); one column, seven idle waves in the column role        1
    W4   23 46 unitary 1  4   1058 pairs: 34 threads in slot 3                                                                    8/8/8/7/6
    W5   28 56 unitary 2  2   1568 pairs: 32 threads in slot 4, the first size that enters it; fused LDS 100,352 B               8/8/8/8/7
    W6   32 64 ket     1  6   wG = 64 in the column role at n = 64: every lane, every ELL slot                                   1
    W7    5 10 unitary 2 24   the ABI's most drives; Hessian served at orders 2 - 8, REFUSED at order 10 (190,728 B > 163,840 B)  3/2/1/1/-
    W8    3  6 unitary 1  0   drift only, w = C = 3 < 8 (order 2: Q = 1, no R chain)                                              3/3/3/3/3
    W9    6 12 unitary 2 10   w = 5                                                                                               6/5/3/2/2
    W10  20 40 unitary 2  6   w = 2 with the third wave missing by 129 doubles (17,409 > 17,280); ten passes of accumulation     8/7/4/3/2
Every w from 1 to 8 occurs, a last pass with idle waves at w = 2, 3, 5, 6, 7 and 8 (W2, W4, W5, W7, W9, W10), and both sides of the refusal (W7).  One shape moved:
G(H) of a Hermitian H has a zero diagonal in its Im H blocks, so a dense case has wG = n - 1, not n.  W6's drift therefore carries a decay term
(H - i diag(gamma), gamma ~ 0.2 U(0.5, 1.5)), which fills the diagonal: wG = 64 as the case is meant to have.  tests/test_variational_sweep_cpu.py
recomputes every count above with the launch code's own arithmetic, restated below (pair_slots, split_cols, fused_lds_bytes, hess_lds_bytes,
hess_plan, ell_widths).

The truth is tests/vector_shape_cases.truth_values (np.longdouble, no code shared with oracle/pade_oracle.py's value routines) on the LIFTED
problem of variational_truth.lifted, mapped to the stacked order with variational_truth's row and column maps, rounded to float64 and kept per
(case, order).  Segments are those of jac_label / hess_label (row component x variable kind x relative knot) extended by the interval's index
('#k'): every interval's segment is held to its own size, and one whose truth is identically zero (the L blocks and the d/du tails at
Delta t = 0) must come out as zeros.

Reference floor: the largest deviation of the float64 lifted oracle (variational_truth.residual / jacobian / hessian) from this truth per
segment, relative to the segment's own maximum, over every case and order (tests/test_variational_sweep_cpu.py asserts 1e-13 and prints them):
    residual 3.9e-16 (delta.r2#2, W2, order 10)    Jacobian 9.0e-16 (r2.h@0#1, W5, order 6)    Hessian 1.4e-14 (h.h@0#0, W6, order 10)
No case had to be reseeded (RESEED is empty)."""
import functools

import numpy as np

import variational_truth as vt
import vector_shape_cases as vs
from oracle import pade_oracle as po

LDS_BYTES = 163840
ORDERS = vs.ORDERS
SCALES = (3.0, 0.25)
THREADS = 512  # PCL_VAR_THREADS
PPT = 4  # PCL_VAR_PPT
LD_ = np.longdouble

# name: (d, ket, v, m)
CASES = {
    "W1": (16, False, 1, 2), "W2": (17, False, 2, 3), "W3": (22, True, 2, 1), "W4": (23, False, 1, 4), "W5": (28, False, 2, 2),
    "W6": (32, True, 1, 6), "W7": (5, False, 2, 24), "W8": (3, False, 1, 0), "W9": (6, False, 2, 10), "W10": (20, False, 2, 6),
}  # fmt: skip
# the waves of pcl_var_hess_kernel the table claims, per order 2 / 4 / 6 / 8 / 10 (None: refused)
HESS_WAVES = {
    "W1": (8, 8, 8, 8, 8), "W2": (8, 8, 8, 7, 6), "W3": (1, 1, 1, 1, 1), "W4": (8, 8, 8, 7, 6), "W5": (8, 8, 8, 8, 7), "W6": (1, 1, 1, 1, 1),
    "W7": (3, 2, 1, 1, None), "W8": (3, 3, 3, 3, 3), "W9": (6, 5, 3, 2, 2), "W10": (8, 7, 4, 3, 2),
}  # fmt: skip
# a case whose scalar segment near-cancels draws from another seed: name -> how many seeds further (none needed)
RESEED = {}


def shape(name):
    """(n, C, v, m)"""
    d, ket, v, m = CASES[name]
    return 2 * d, (1 if ket else d), v, m


# ---- the launch code's arithmetic (pcl_host_variational.hpp, pcl_kernel_variational.hpp) ------------------------------------------------------
def pair_slots(n):
    """pcl_var_block_role: (value pairs n^2 / 2, the slots of 512 threads that hold any, the threads the last of them uses)."""
    npair = n * n // 2
    slots = -(-npair // THREADS)
    assert slots <= PPT
    return npair, slots, npair - THREADS * (slots - 1)


def last_slot_start(n):
    """First entry of a tile that the last pair slot owns (pair p holds entries 2 p and 2 p + 1)."""
    return 2 * THREADS * (pair_slots(n)[1] - 1)


def split_blocks(C, opt=0):
    """var_split_blocks: block workgroups per interval."""
    return max(1, min(opt if opt > 0 else 1, C))


def split_cols(C, opt=0):
    """var_split_cols and pcl_var_col_role: (column workgroups per interval, the state columns [ca, cb) of each)."""
    w = THREADS // 64
    ncw = max(1, min(opt if opt > 0 else -(-C // w), C))
    return ncw, [(rc * C // ncw, (rc + 1) * C // ncw) for rc in range(ncw)]


def fused_lds_bytes(n, v, wG, jac=True):
    """var_launch_fused: the block role's G, P, Q_i tiles against the column role's row-compressed G(u_k)."""
    return max((2 + v) * n * n if jac else 0, wG * n) * 8


def hess_lds_bytes(n, m, v, q, w):
    """var_hess_lds"""
    return (2 * n * n + w * (m * q * (v + 1) * 64 + m * m + m + 1)) * 8


def hess_plan(n, C, m, v, order):
    """var_launch_hess: dict(served, w, bytes, passes, idle) -- the waves per workgroup, the passes over the columns they imply and the waves
    idle in the last pass; served False: PCL_ESHAPE with `bytes` in the message."""
    q = order // 2
    w = min(8, C)
    while w > 1 and hess_lds_bytes(n, m, v, q, w) > LDS_BYTES:
        w -= 1
    b = hess_lds_bytes(n, m, v, q, w)
    passes = -(-C // w)
    return dict(served=b <= LDS_BYTES, w=w, bytes=b, passes=passes, idle=passes * w - C)


def ell_widths(G0, Gj, Gv):
    """var_create: (wG, wD, wV) -- the widest row of the union pattern of the drift and the drives, of any drive, of any variation generator;
    at least 1 each."""
    row = lambda mats: int(max(1, np.any([np.asarray(a) != 0 for a in mats], axis=0).sum(axis=1).max()))
    return row([G0] + list(Gj)), max([1] + [row([a]) for a in Gj]), max([1] + [row([a]) for a in Gv])


# ---- systems and trajectories ----------------------------------------------------------------------------------------------------------------
def _herm(d, rng):
    A = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return (A + A.conj().T) / (2 * np.sqrt(d))


def _seed(name):
    return 15000 + 17 * int(name[1:]) + 5 * RESEED.get(name, 0)


@functools.lru_cache(maxsize=None)
def system(name):
    """(G0, Gj [m, n, n], [Gv_i]) -- the variation generators already divided by their scales."""
    d, ket, v, m = CASES[name]
    n = 2 * d
    rng = np.random.default_rng(_seed(name))
    H0 = _herm(d, rng)
    Hd = [_herm(d, rng) for _ in range(m)]
    Hv = [_herm(d, rng) for _ in range(v)]
    if name == "W6":  # a decay term fills the diagonal of the Im H blocks: the union pattern is full, wG = n
        H0 = H0 - 1j * np.diag(0.2 * (0.5 + rng.random(d)))
    if name == "W2":
        S = np.zeros((d, d), dtype=complex)  # drive 2: five entries, twelve of the 17 rows (and columns) empty
        S[0, 1], S[1, 0], S[3, 3], S[7, 16], S[16, 7] = 0.7 - 0.4j, 0.7 + 0.4j, -0.9, 0.5j, -0.5j
        Hd[2] = S
        Hv[1] = np.diag(rng.standard_normal(d))  # Gv_2: one entry per row
    G0 = po.G_of_H(H0)
    Gj = np.array([po.G_of_H(H) for H in Hd]).reshape(m, n, n)
    Gv = [po.G_of_H(H) / s for H, s in zip(Hv, SCALES)]
    for a in [G0, Gj] + Gv:
        a.setflags(write=False)
    return G0, Gj, Gv


def knot(name):
    """(N, z_dim, xo, dt_off, u_off) -- [X | Xv_1 .. | dt | t | u]; W2: [t | X | Xv1 | Xv2 | dt | u], N = 5."""
    n, C, v, m = shape(name)
    xdc = n * C
    if name == "W2":
        return 5, 1 + (v + 1) * xdc + 1 + m, [1 + b * xdc for b in range(v + 1)], 1 + (v + 1) * xdc, 2 + (v + 1) * xdc
    return 4, (v + 1) * xdc + 2 + m, [b * xdc for b in range(v + 1)], (v + 1) * xdc, (v + 1) * xdc + 2


def _lifted_norm(case, k):
    G = case.G0 + (np.tensordot(case.Z[k, case.u_off : case.u_off + case.m], case.Gj, axes=1) if case.m else 0)
    return np.linalg.norm(po.var_G(G, list(case.Gv)), 2)


@functools.lru_cache(maxsize=None)
def case(name):
    """(VarCase, long step), read-only."""
    n, C, v, m = shape(name)
    G0, Gj, Gv = system(name)
    N, z_dim, xo, dt_off, u_off = knot(name)
    rng = np.random.default_rng(_seed(name) + 1)
    Z = 0.4 * rng.standard_normal((N, z_dim))
    cs = vt.VarCase(Z=Z, z_dim=z_dim, N=N, n=n, C=C, m=m, xo=xo, u_off=u_off, dt_off=dt_off, G0=G0, Gv=Gv, Gj=Gj)
    n2 = [_lifted_norm(cs, k) for k in range(3)]
    Z[:, dt_off] = 0.1
    Z[0, dt_off], Z[1, dt_off] = 0.15 / n2[0], -0.3 / n2[1]
    if N == 5:
        Z[3, dt_off] = 0.0
    long_step = None
    for s in vs.LONG_STEPS:
        Z[2, dt_off] = s / n2[2]
        Zl, lay, G0l, Gjl = vt.lifted(cs)
        if vs.top_term_weight(lay, G0l, Gjl, Zl) >= vs.SEEN:
            long_step = s
            break
    assert long_step is not None, name
    t_off = 0 if name == "W2" else dt_off + 1
    Z[:, t_off] = np.cumsum(Z[:, dt_off])
    Z.setflags(write=False)
    return cs, long_step


def thetas(name):
    """h |Ghat(u_k)|_2 per interval."""
    cs, _ = case(name)
    return [cs.Z[k, cs.dt_off] * _lifted_norm(cs, k) for k in range(cs.K)]


def rand_mu(name):
    cs, _ = case(name)
    mu = np.random.default_rng(_seed(name) + 77).standard_normal(cs.K * cs.xd)
    mu.setflags(write=False)
    return mu


# ---- per-segment labels ----------------------------------------------------------------------------------------------------------------------
def _var_kind(case, idx):
    """(kind, knot) of a variable: 'u', 'h', 't' or 'X<b>' (component b of the stacked state)."""
    k, o = idx // case.z_dim, idx % case.z_dim
    kind = np.full(idx.shape, "t", dtype="<U4")
    kind[(o >= case.u_off) & (o < case.u_off + case.m)] = "u"
    kind[o == case.dt_off] = "h"
    for b, xo in enumerate(case.xo):
        kind[(o >= xo) & (o < xo + case.xdc)] = "X%d" % b
    return kind, k


def jac_label(case, r, c):
    """B blocks (row component = column component), L blocks (different components), the d/du and d/dh tails, by row component."""
    kc, knc = _var_kind(case, c)
    br = (r % case.xd) // case.xdc
    rel = knc - r // case.xd
    return np.char.add(np.char.add(np.char.add("r", br.astype(str)), np.char.add(".", kc)), np.char.add("@", rel.astype(str)))


def hess_label(case, a, b):
    """(u,u), (h,u), (h,h) and the X rows by component and knot."""
    ka, kna = _var_kind(case, a)
    kb, knb = _var_kind(case, b)
    return np.char.add(np.char.add(ka, "."), np.char.add(kb, np.char.add("@", (kna - knb).astype(str))))


def check_sparse_segments(ours, truth, label, tol):
    T, D = truth.tocoo(), (ours - truth).tocoo()
    lt, ld = label(T.row, T.col), label(D.row, D.col)
    assert set(ld) <= set(lt)
    for s in np.unique(lt):
        scale = np.abs(T.data[lt == s]).max()
        err = np.abs(D.data[ld == s]).max() if (ld == s).any() else 0.0
        assert err <= tol * scale, "segment %s: max err %.3e, max |ref| %.3e" % (s, err, scale)


# The same labels as integers (millions of values per case): code -> the label's text with the interval appended, 'r1.X0@1#2'.
_KINDS = ("t", "u", "h", "X0", "X1", "X2")


def _kind_code(case, idx):
    k, o = idx // case.z_dim, idx % case.z_dim
    kind = np.zeros(idx.shape, dtype=np.int64)
    kind[(o >= case.u_off) & (o < case.u_off + case.m)] = 1
    kind[o == case.dt_off] = 2
    for b, xo in enumerate(case.xo):
        kind[(o >= xo) & (o < xo + case.xdc)] = 3 + b
    return kind, k


def residual_codes(case, r):
    """row component x interval"""
    return ((r % case.xd) // case.xdc) * case.K + r // case.xd


def residual_name(case, code):
    return "delta.r%d#%d" % (code // case.K, code % case.K)


def jac_codes(case, r, c):
    """jac_label x the interval (the row's)"""
    kc, knc = _kind_code(case, c)
    k = r // case.xd
    return ((((r % case.xd) // case.xdc) * len(_KINDS) + kc) * 3 + (knc - k + 1)) * case.K + k


def jac_name(case, code):
    code, k = divmod(int(code), case.K)
    code, rel = divmod(code, 3)
    br, kc = divmod(code, len(_KINDS))
    return "r%d.%s@%d#%d" % (br, _KINDS[kc], rel - 1, k)


def hess_codes(case, a, b):
    """hess_label x the interval (the knot of the u / h variable: the earlier of the two knots)"""
    ka, kna = _kind_code(case, a)
    kb, knb = _kind_code(case, b)
    return ((ka * len(_KINDS) + kb) * 3 + (kna - knb + 1)) * case.K + np.minimum(kna, knb)


def hess_name(case, code):
    code, k = divmod(int(code), case.K)
    code, rel = divmod(code, 3)
    ka, kb = divmod(code, len(_KINDS))
    return "%s.%s@%d#%d" % (_KINDS[ka], _KINDS[kb], rel - 1, k)


def segment_max(codes, values):
    """{code: max |values|}"""
    u, inv = np.unique(codes, return_inverse=True)
    out = np.zeros(len(u))
    np.maximum.at(out, inv.reshape(-1), np.abs(np.asarray(values, dtype=np.float64)))
    return dict(zip(u.tolist(), out.tolist()))


def segment_errors(codes, got, want, scale_codes=None, scale_values=None):
    """{code: (max |got - want|, max |want| of the segment)}.  scale_codes / scale_values: the whole truth, where `want` is only part of it."""
    err = segment_max(codes, np.asarray(got, dtype=LD_) - np.asarray(want, dtype=LD_))
    scale = segment_max(codes if scale_codes is None else scale_codes, want if scale_values is None else scale_values)
    return {s: (e, scale[s]) for s, e in err.items()}


def assert_segments(errors, tol, name_of, what):
    """Every segment within tol of its own maximum (a segment whose truth is identically zero: exactly zero).  Returns (worst relative error,
    its segment)."""
    worst = (0.0, None)
    for s, (e, scale) in errors.items():
        assert np.isfinite(e) and e <= tol * scale, "%s, segment %s: max err %.3e, max |truth| %.3e (rel %.3e > %.1e)" % (
            what, name_of(s), e, scale, e / scale if scale else np.inf, tol)  # fmt: skip
        if scale > 0 and e / scale > worst[0]:
            worst = (e / scale, name_of(s))
    return worst


def moved(codes, good, bad, only=None):
    """The largest relative change of a segment, against the segment's own maximum in `good`; only: a predicate on the code."""
    best = 0.0
    for s, (e, scale) in segment_errors(codes, bad, good).items():
        if scale > 0 and (only is None or only(s)):
            best = max(best, e / scale)
    return best


# ---- the truth, in np.longdouble, on the lifted problem --------------------------------------------------------------------------------------
# delta [K xd] in stacked order; the Jacobian and the Hessian over every position of the lifted structure, sorted by key = row * ncols + col.
# `jstruct` marks the positions the library's structure has: the blocks (b, b) and (b, 0) and the tails (the lifted generator's other blocks are zero).
@functools.lru_cache(maxsize=None)
def maps(name):
    """Positions of the lifted structure in the case's own rows and variables: Jacobian (rows, cols), Hessian (rows >= cols)."""
    cs, _ = case(name)
    lay = vt.lifted(cs)[1]
    rm, cm = vt._row_map(cs), vt._col_map(cs, lay)
    rows, cols = po.jac_structure(lay)
    jr, jc = (rows // cs.xd) * cs.xd + rm[rows % cs.xd], cm[cols]
    a, b = po.hess_structure(lay)
    a, b = cm[a], cm[b]
    return rm, jr, jc, np.maximum(a, b), np.minimum(a, b)


def lifted_values(name, order, hessian=True, zero_last_variation=False, **kw):
    """vector_shape_cases.truth_values on the lifted problem: (delta [K xd] in stacked order, Jacobian values and Hessian values in the order
    of maps(name)), in longdouble.  kw: truth_values' switches (c, drop_drive, drop_col, intervals); zero_last_variation: Gv_v read as zero."""
    cs, _ = case(name)
    Zl, lay, G0l, Gjl = vt.lifted(cs)
    if zero_last_variation:
        G0l = np.array(G0l)
        G0l[cs.v * cs.n :, : cs.n] = 0
    rm = maps(name)[0]
    mul = rand_mu(name).reshape(cs.K, cs.xd)[:, rm] if hessian else None
    d, j, h = vs.truth_values(lay, G0l, Gjl, Zl, mul, order, hessian=hessian, **kw)
    ds = np.empty_like(d)
    ds[:, rm] = d
    return ds.reshape(-1), j.reshape(-1), None if h is None else h.reshape(-1)


@functools.lru_cache(maxsize=None)
def structure(name):
    """What does not depend on the order: the sorted keys, their segment codes, the permutations that sort them and the structural mask."""
    cs, _ = case(name)
    _, jr, jc, ha, hb = maps(name)
    ncols = cs.N * cs.z_dim
    jkey, hkey = jr * ncols + jc, ha * ncols + hb
    jo, ho = np.argsort(jkey, kind="stable"), np.argsort(hkey, kind="stable")
    for key, o in ((jkey, jo), (hkey, ho)):
        assert np.all(np.diff(key[o]) > 0)  # every position once
    kc, _ = _kind_code(cs, jc[jo])
    br = (jr[jo] % cs.xd) // cs.xdc
    structural = (kc < 3) | (kc - 3 == br) | (kc == 3)
    out = dict(jkey=jkey[jo], jperm=jo, jcode=jac_codes(cs, jr[jo], jc[jo]), jstruct=structural, hkey=hkey[ho], hperm=ho,
               hcode=hess_codes(cs, ha[ho], hb[ho]), dcode=residual_codes(cs, np.arange(cs.K * cs.xd)), ncols=ncols)  # fmt: skip
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truth_ld(name, order):
    """(delta, Jacobian values, Hessian values) in longdouble, the latter two in the order of structure(name)'s sorted keys; computed once."""
    st = structure(name)
    d, j, h = lifted_values(name, order)
    j, h = j[st["jperm"]], h[st["hperm"]]
    assert not np.any(j[~st["jstruct"]])  # the library's structure holds every non-zero of the lifted problem
    for a in (d, j, h):
        a.setflags(write=False)
    return d, j, h


@functools.lru_cache(maxsize=None)
def truth(name, order):
    """The same rounded to float64: what the GPU tests compare with."""
    out = tuple(a.astype(np.float64) for a in truth_ld(name, order))
    for a in out:
        a.setflags(write=False)
    return out


def lookup(keys_sorted, keys):
    """Index of every key in keys_sorted, and whether it is there at all."""
    i = np.minimum(np.searchsorted(keys_sorted, keys), len(keys_sorted) - 1)
    return i, keys_sorted[i] == keys


def value_order(name):
    """Index into the sorted Jacobian truth of every value of the library's layout (var_compact_cases.pade_structure): the truth in value order
    is truth(..)[1][value_order(name)]."""
    import var_compact_cases as vcc

    cs, _ = case(name)
    st = structure(name)
    r, c = vcc.pade_structure(cs)
    i, ok = lookup(st["jkey"], r * st["ncols"] + c)
    assert ok.all() and len(np.unique(i)) == len(i) == int(st["jstruct"].sum())
    return i


def zero_last_pair_slot(name, jac_sorted):
    """The Jacobian truth with the entries that the block role's LAST pair slot stores read as zero: entries >= 2 * 512 * (slots - 1) of every
    copy of every B+-, L+-_i tile."""
    cs, _ = case(name)
    n, C, v = cs.n, cs.C, cs.v
    vo = value_order(name)
    per = (2 + 4 * v) * C * n * n + cs.xd * (cs.m + 1)
    tiles = vo.reshape(cs.K, per)[:, : (2 + 4 * v) * C * n * n].reshape(cs.K, 2 + 4 * v, C, n * n)
    bad = np.array(jac_sorted)
    bad[tiles[..., last_slot_start(n) :].reshape(-1)] = 0
    return bad
