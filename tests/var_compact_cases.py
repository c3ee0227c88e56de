"""What the tests of the option var_compact share (numpy only, importable without a GPU): the two compact layouts of a variational context, the
fold of full values into them, their expansion, the bitwise comparison, the cases and their truth.

Per interval, with nn = n^2, x_dim' = (1 + v) n C and the tails x_dim' (m + 1) values in the order of the full layout:

    Pade         full    [-B+ x C | B- x C | per variation i: -B+ x C | B- x C | -L+_i x C | L-_i x C | tails]
                 compact [-B+ | B- | per variation i: -L+_i | L-_i | tails]
    exponential  full    [-E x C | per variation i: -E x C | -L_i x C | ones (x_dim') | tails]
                 compact [-E | -L_1 .. -L_v | tails]

The cases are the smallest shapes at which the kernels change behaviour (tests/test_var_compact_gpu.py has the table)."""
import functools

import numpy as np

import var_exp_cases as vx
import var_exp_truth
import variational_truth as vt


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------
def n_tiles(v, expo):
    return 1 + v if expo else 2 + 2 * v


def n_segments(v, expo):
    return 1 + 2 * v if expo else 2 + 4 * v


def tile_of_segment(s, expo):
    """The compact tile that segment s of the full layout replicates."""
    if expo:  # -E | per i: -E, -L_i
        return 0 if s == 0 or s % 2 == 1 else s // 2
    if s < 2:  # -B+, B-
        return s
    i, j = divmod(s - 2, 4)  # per i: -B+, B-, -L+_i, L-_i
    return j if j < 2 else 2 + 2 * i + (j - 2)


def tail_len(n, C, v, m):
    return (1 + v) * n * C * (m + 1)


def full_per(n, C, v, m, expo):
    return n_segments(v, expo) * C * n * n + (1 + v) * n * C * (m + 2 if expo else m + 1)


def compact_per(n, C, v, m, expo):
    return n_tiles(v, expo) * n * n + tail_len(n, C, v, m)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    """The comparison of the GPU tests: the same shape and the same 64 bits in every value (so -0.0 is not 0.0, and a NaN only equals itself)."""
    return np.shape(a) == np.shape(b) and bool(np.array_equal(_bits(a), _bits(b)))


def compact_of_full(vals, n, C, v, m, expo):
    """[K, full_per] -> [K, compact_per].  Every copy that is folded away must have the bits of the one that is kept, and (exponential) every one
    must be 1.0: anything else raises ValueError -- the fold hides no wrong copy."""
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    K = vals.shape[0]
    nn, ns, nt = n * n, n_segments(v, expo), n_tiles(v, expo)
    if vals.ndim != 2 or vals.shape[1] != full_per(n, C, v, m, expo):
        raise ValueError("full values of shape %r, expected [K, %d]" % (vals.shape, full_per(n, C, v, m, expo)))
    seg = vals[:, : ns * C * nn].reshape(K, ns, C, nn)
    comp = np.empty((K, compact_per(n, C, v, m, expo)))
    seen = set()
    for s in range(ns):
        t = tile_of_segment(s, expo)
        if t not in seen:
            comp[:, t * nn : (t + 1) * nn] = seg[:, s, 0]
            seen.add(t)
        diff = _bits(seg[:, s]) != _bits(np.broadcast_to(comp[:, None, t * nn : (t + 1) * nn], seg[:, s].shape))
        if diff.any():
            k, c, e = np.argwhere(diff)[0]
            raise ValueError("segment %d (tile %d): copy %d of interval %d differs from the tile at entry %d" % (s, t, c, k, e))
    assert seen == set(range(nt))
    o = ns * C * nn
    if expo:
        xd = (1 + v) * n * C
        diff = _bits(vals[:, o : o + xd]) != _bits(np.ones((K, xd)))
        if diff.any():
            k, e = np.argwhere(diff)[0]
            raise ValueError("the identity's diagonal: entry %d of interval %d is not 1.0" % (e, k))
        o += xd
    comp[:, nt * nn :] = vals[:, o:]
    return comp


def expand_compact(comp, n, C, v, m, expo):
    """[K, compact_per] -> [K, full_per]: plain copies."""
    comp = np.ascontiguousarray(comp, dtype=np.float64)
    K = comp.shape[0]
    nn, ns, nt = n * n, n_segments(v, expo), n_tiles(v, expo)
    if comp.ndim != 2 or comp.shape[1] != compact_per(n, C, v, m, expo):
        raise ValueError("compact values of shape %r, expected [K, %d]" % (comp.shape, compact_per(n, C, v, m, expo)))
    full = np.empty((K, full_per(n, C, v, m, expo)))
    seg = full[:, : ns * C * nn].reshape(K, ns, C, nn)
    for s in range(ns):
        t = tile_of_segment(s, expo)
        seg[:, s] = comp[:, None, t * nn : (t + 1) * nn]
    o = ns * C * nn
    if expo:
        xd = (1 + v) * n * C
        full[:, o : o + xd] = 1.0
        o += xd
    full[:, o:] = comp[:, nt * nn :]
    return full


def of_case(case, expo):
    return dict(n=case.n, C=case.C, v=case.v, m=case.m, expo=expo)


# ---- the structure of the Pade layout (the exponential one: var_exp_truth.structure) -------------------------------------------------------
def pade_structure(case):
    """(rows, cols) of the K intervals of a PCL_BATCH_VARIATIONAL context in value order, index base 0."""
    n, C, v, m, xdc, xd, zd = case.n, case.C, case.v, case.m, case.xdc, case.xd, case.z_dim
    c_, j_, i_ = np.meshgrid(np.arange(C), np.arange(n), np.arange(n), indexing="ij")
    br, bc = (c_ * n + i_).reshape(-1), (c_ * n + j_).reshape(-1)
    c_, l_, i_ = np.meshgrid(np.arange(C), np.arange(m + 1), np.arange(n), indexing="ij")
    tr = (c_ * n + i_).reshape(-1)
    tc = np.where(l_ < m, case.u_off + l_, case.dt_off).reshape(-1)
    rows, cols = [], []
    for k in range(case.K):
        r0, c0 = k * xd, k * zd
        for brow, bcol in [(0, 0)] + [p for b in range(1, v + 1) for p in ((b, b), (b, 0))]:
            for knot in (0, 1):
                rows.append(r0 + brow * xdc + br)
                cols.append(c0 + knot * zd + case.xo[bcol] + bc)
        for b in range(v + 1):
            rows.append(r0 + b * xdc + tr)
            cols.append(c0 + tc)
    return np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
# name -> (builder of (oracle system, H_vars, scales, VarCase), ket)
_BUILD = {
    "pauli_ket": (lambda: vx.pauli(True), True),
    "pauli": (lambda: vx.pauli(False), False),
    "config2_v1": (lambda: vx.config2(1), False),
    "config2_v2": (lambda: vx.config2(2), False),
    "d16": (lambda: vx.transmon(16), False),
    "d17": (lambda: vx.transmon(17), False),
    "d32": (lambda: vx.transmon(32), False),
    "d31": (lambda: vx.transmon(31), False),
    "config3_v1": (lambda: vx.config3(1), False),
    "config3_v2": (lambda: vx.config3(2), False),
    "config3_v1_ket": (lambda: vx.config3(1, ket=True, N=5), True),
    "config3_v2_ket": (lambda: vx.config3(2, ket=True, N=5), True),
}
_SHAPES = ["pauli_ket", "pauli", "config2_v1", "config2_v2", "d16", "d17"]
_CONFIG3 = ["config3_v1", "config3_v2", "config3_v1_ket", "config3_v2_ket"]
# (name, order): order 4 everywhere, 10 too on config 2 and config 3 (the fold differs by order, the store does not); d = 32: all four passes
PADE_CASES = [(nm, 4) for nm in _SHAPES + ["d32"] + _CONFIG3] + [(nm, 10) for nm in ["config2_v1", "config2_v2"] + _CONFIG3]
# d = 31 (n = 62): no LDS tile for G(u_k)
EXP_CASES = [(nm, "exp") for nm in _SHAPES + _CONFIG3 + ["d31"]]
ALL_CASES = PADE_CASES + EXP_CASES


def case_id(p):
    return "%s-%s" % p


@functools.lru_cache(maxsize=None)
def built(name):
    """(oracle system, H_vars, scales, VarCase, ket) -- built once; nobody writes into it."""
    fn, ket = _BUILD[name]
    s, Hv, scales, case = fn()
    case.Z.setflags(write=False)
    return s, Hv, scales, case, ket


@functools.lru_cache(maxsize=None)
def truth(name, order):
    """(values [K, full_per] of the oracle at the library's structure, the scale the existing GPU tests compare against) -- computed once.
    Pade: max |J| (test_variational_gpu._check_all); exponential: max(1, max |values|) (test_parity_gpu.close)."""
    case = built(name)[3]
    if order == "exp":
        vals = var_exp_truth.values(case).reshape(case.K, -1)
        scale = max(1.0, np.abs(vals).max())
    else:
        J, _ = vt.jacobian(case, order)
        r, c = pade_structure(case)
        vals = np.asarray(J[r, c]).reshape(case.K, -1)
        assert abs(np.abs(J).sum() - np.abs(vals).sum()) <= 1e-12 * max(1.0, np.abs(vals).sum())  # the structure holds every value of the lifted problem
        scale = np.abs(J.data).max()
    vals.setflags(write=False)
    return vals, scale


TOL = 1e-11  # of the existing variational / var-exp GPU tests, times the scale above


def matches(got, name, order):
    """The two comparisons of the GPU test in one: `got` [K, full_per] agrees with the truth within TOL x scale.  Returns the worst error."""
    want, scale = truth(name, order)
    got = np.asarray(got).reshape(want.shape)
    err = np.abs(got - want).max()
    return bool(np.isfinite(got).all() and err <= TOL * scale), err


# ---- faults the comparison has to see (test_var_compact_cpu.py) -----------------------------------------------------------------------------
def fault_drop_copy(comp, full, n, C, v, m, expo):
    """An expansion that leaves the last copy of the last segment unwritten (NaN, as the tests pre-fill)."""
    out = expand_compact(comp, n, C, v, m, expo)
    e = n_segments(v, expo) * C * n * n
    out[:, e - n * n : e] = np.nan
    return out


def fault_swap_L(comp, full, n, C, v, m, expo):
    """-L+_1 and L-_1 exchanged in the compact block (exponential: -E and -L_1)."""
    c = comp.copy()
    nn = n * n
    a, b = (0, 1) if expo else (2, 3)
    c[:, a * nn : (a + 1) * nn], c[:, b * nn : (b + 1) * nn] = comp[:, b * nn : (b + 1) * nn], comp[:, a * nn : (a + 1) * nn]
    return expand_compact(c, n, C, v, m, expo)


def fault_missing_one(comp, full, n, C, v, m, expo):
    assert expo
    out = expand_compact(comp, n, C, v, m, expo)
    out[:, n_segments(v, expo) * C * n * n + 1] = np.nan
    return out


def fault_shift_tail(comp, full, n, C, v, m, expo):
    """The tails written one state column (m + 1) n further."""
    out = expand_compact(comp, n, C, v, m, expo)
    t = tail_len(n, C, v, m)
    out[:, -t:] = np.roll(out[:, -t:], (m + 1) * n, axis=1)
    return out
