"""Closed forms of the objective-side operations in np.longdouble (importable without a GPU): the terminal losses Q w |1 - F| with their
gradients and dense lower-triangle Hessians, the quadratic regularisers with first and second derivatives, the derivative /
time-consistency rows and the reduce payload.  Written from the formulas in the comments of pcl_kernels_objective.hpp / pcl_kernels_misc.hpp
and the reference's src/control/objectives.jl; nothing here calls the float64 oracle for the arithmetic under test (the payload takes the
oracle's Jacobian as DATA and forms the dot products here).

Every sum takes an optional `keep` mask over its summation index: the "mutant" truths of tests/test_objective_shapes_cpu.py (a sum that
loses the elements a workgroup's second pass or one wave's partial would have contributed) are these same functions with a mask."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "objective_truth needs an extended-precision np.longdouble (eps %.3e on this platform)" % np.finfo(LD).eps


def ld(a):
    return np.asarray(a, dtype=LD)


def _dot(a, b, keep=None):
    p = ld(a) * ld(b)
    return p.sum() if keep is None else p[keep].sum()


# ---- rows of the general form F = c'x + sum_r (A_r'x)^2 -------------------------------------------------------------------------------
def functional_rows(L, re_idx, im_idx, g):
    """The two real rows (Re, Im) of the complex linear functional  sum_p conj(g_p) (x[re_idx_p] + i x[im_idx_p])."""
    g = np.asarray(g)
    gr, gi = ld(g.real), ld(g.imag)
    rows = np.zeros((2, L), dtype=LD)
    np.add.at(rows[0], re_idx, gr)
    np.add.at(rows[0], im_idx, gi)
    np.add.at(rows[1], re_idx, -gi)
    np.add.at(rows[1], im_idx, gr)
    return rows


def iso_index(d):
    """(re, im) positions of U[i, c] in the iso-vec (column c = [Re U[:, c]; Im U[:, c]]), as d x d index arrays [i, c]."""
    i, c = np.meshgrid(np.arange(d), np.arange(d), indexing="ij")
    return c * 2 * d + i, c * 2 * d + d + i


def unitary_rows(G, keep=None):
    """F = |tr(G'U)|^2 / d^2 = (a'x)^2 + (b'x)^2  [objectives.jl:330-337].  keep: mask over the element index e = c d + i of the trace's sum."""
    G = np.asarray(G)
    d = G.shape[0]
    re, im = iso_index(d)
    re, im, g = re.T.reshape(-1), im.T.reshape(-1), G.T.reshape(-1)  # e = c d + i
    if keep is not None:
        re, im, g = re[keep], im[keep], g[keep]
    return functional_rows(2 * d * d, re, im, g) / LD(d)


def subspace_rows(Gs, sub, d, keep=None):
    """F = (|M|_F^2 + |tr M|^2) / (ns (ns + 1)), M = Gs' U[sub, sub]  [objectives.jl:339-345]: a row pair per entry M[i, j] and one for the trace.
    keep: mask over the entry index e = j ns + i of the sums over M (Frobenius norm and trace)."""
    Gs, sub = np.asarray(Gs), np.asarray(sub)
    ns, L = len(sub), 2 * d * d
    sc = 1 / np.sqrt(LD(ns) * LD(ns + 1))
    rows, tr = [], np.zeros((2, L), dtype=LD)
    for j in range(ns):
        for i in range(ns):
            if keep is not None and not keep[j * ns + i]:
                continue
            r = functional_rows(L, sub[j] * 2 * d + sub, sub[j] * 2 * d + d + sub, Gs[:, i]) * sc  # M[i, j] = sum_k conj(Gs[k, i]) U[sub_k, sub_j]
            rows.append(r)
            if i == j:
                tr += r
    return np.concatenate(rows + [tr])


def ket_rows(goal):
    """F = |<g|psi>|^2  [objectives.jl:24-27], psi-tilde = [Re psi; Im psi]."""
    d = len(goal)
    return functional_rows(2 * d, np.arange(d), d + np.arange(d), goal)


def coherent_ket_rows(goals, weights=None):
    """F = |sum_i w_i <g_i|psi_i> / sum w|^2 over the concatenated kets; no (or uniform) weights: |sum / n|^2  [objectives.jl:96-121]."""
    n, d = len(goals), len(goals[0])
    w = np.ones(n, dtype=LD) if weights is None or len(set(float(x) for x in weights)) == 1 else ld(weights)
    rows = np.zeros((2, 2 * d * n), dtype=LD)
    for q, g in enumerate(goals):
        rows += functional_rows(2 * d * n, q * 2 * d + np.arange(d), q * 2 * d + d + np.arange(d), g) * (w[q] / w.sum())
    return rows


# ---- direct closed forms of the two unitary fidelities (independent of the rows above) ---------------------------------------------------
def _op(x, d):
    X = ld(x).reshape(d, 2 * d)  # row c = column c of U
    return X[:, :d].T, X[:, d:].T  # Re U, Im U as [i, c]


def unitary_fidelity(x, G):
    G = np.asarray(G)
    d = G.shape[0]
    ur, ui = _op(x, d)
    gr, gi = ld(G.real), ld(G.imag)
    tr, ti = (gr * ur + gi * ui).sum(), (gr * ui - gi * ur).sum()
    return (tr * tr + ti * ti) / (LD(d) * LD(d))


def subspace_fidelity(x, Gs, sub, d):
    Gs, sub = np.asarray(Gs), np.asarray(sub)
    ns = len(sub)
    ur, ui = _op(x, d)
    ur, ui = ur[np.ix_(sub, sub)], ui[np.ix_(sub, sub)]
    ar, ai = ld(Gs.real).T, -ld(Gs.imag).T  # Gs'
    mr, mi = ar @ ur - ai @ ui, ar @ ui + ai @ ur
    tr, ti = np.trace(mr), np.trace(mi)
    return ((mr * mr + mi * mi).sum() + tr * tr + ti * ti) / (LD(ns) * LD(ns + 1))


# ---- the loss of one term in the general form -----------------------------------------------------------------------------------------------
def form_fidelity(A, c, x, keep=None):
    F = LD(0) if c is None else _dot(c, x, keep)
    p = np.zeros(0 if A is None else len(A), dtype=LD)
    for r in range(len(p)):
        p[r] = _dot(A[r], x, keep)
        F = F + p[r] * p[r]
    return F, p


def form_loss(A, c, x, wQ, keep=None, flip=False):
    """(value, gradient, s, F) of wQ |1 - F(x)|: value wQ |1 - F|, gradient -s wQ (c + 2 sum_r (A_r'x) A_r), s = sign(1 - F) (flip: the mutant)."""
    F, p = form_fidelity(A, c, x, keep)
    s = LD(1) if 1 - F >= 0 else LD(-1)
    if flip:
        s = -s
    g = np.zeros(len(x), dtype=LD) if c is None else ld(c).copy()
    if A is not None:
        g = g + 2 * (p[:, None] * ld(A)).sum(axis=0)
    return wQ * s * (1 - F), -s * wQ * g, s, F


def gram_tril(A):
    """T[i (i + 1) / 2 + j] = 2 sum_r A[r][i] A[r][j], j <= i: the Hessian of F, packed lower triangle (row-major)."""
    A = ld(A)
    T = 2 * (A.T @ A)
    return T[np.tril_indices(A.shape[1])]


# ---- quadratic regularisers  J = 1/2 sum_k h_k^p sum_i R_i v_{k,i}^2 ------------------------------------------------------------------------
def reg_terms(Z, regs, dt_off, keep_of=None, once=False):
    """Z [N, z_dim]; regs: (off, dim, R, p).  Returns (per-knot values [N], gradient [N, z_dim], Hessian triplets (knot, row, col, value) with
    row >= col inside the knot).  A regulariser that covers dt_off has v_i = h for that i: every derivative below is taken of the function of
    the knot's variables, so the (h, v_i) cross term then lands on (h, h) TWICE (both orders of the mixed partial).
    keep_of(dim): mask over i (mutants).  once: entries covered by an earlier regulariser are not counted again (mutant)."""
    Z = ld(Z)
    N, z_dim = Z.shape
    val, grad = np.zeros(N, dtype=LD), np.zeros((N, z_dim), dtype=LD)
    hk, hr, hc, hv = [], [], [], []
    h = Z[:, dt_off]
    seen = np.zeros(z_dim, dtype=bool)
    kk = np.arange(N)
    for off, dim, R, p in regs:
        R = np.broadcast_to(ld(R), (dim,)).copy()
        if once:
            R[seen[off : off + dim]] = 0
            seen[off : off + dim] = True
        v = Z[:, off : off + dim]
        keep = np.ones(dim, dtype=bool) if keep_of is None else keep_of(dim)
        s = (R * v * v)[:, keep].sum(axis=1)
        w = h**p if p else np.ones(N, dtype=LD)
        val += w * s / 2
        grad[:, off : off + dim] += w[:, None] * R * v
        idx = off + np.arange(dim)
        for i in range(dim):
            hk.append(kk), hr.append(np.full(N, idx[i])), hc.append(np.full(N, idx[i])), hv.append(w * R[i])
        if p >= 1:
            grad[:, dt_off] += p * h ** (p - 1) * s / 2
            for i in range(dim):
                cross = p * h ** (p - 1) * R[i] * v[:, i]
                if idx[i] == dt_off:
                    cross = 2 * cross
                hk.append(kk), hr.append(np.full(N, max(idx[i], dt_off))), hc.append(np.full(N, min(idx[i], dt_off))), hv.append(cross)
        if p == 2:
            hk.append(kk), hr.append(np.full(N, dt_off)), hc.append(np.full(N, dt_off)), hv.append(s)
    if not hk:
        return val, grad, (np.zeros(0, int), np.zeros(0, int), np.zeros(0, int), np.zeros(0, dtype=LD))
    return val, grad, (np.concatenate(hk), np.concatenate(hr), np.concatenate(hc), np.concatenate(hv))


# ---- derivative / time-consistency rows -------------------------------------------------------------------------------------------------------
def deriv_rows(Z, x_off, dx_off, dim, dt_off, z0=0, r0=0, index_base=0):
    """x_{k+1} - x_k - h_k dx_k (dx_off < 0: dx = 1).  Returns (residual [K dim], rows, cols, values) in the library's order per interval:
    [-1 (dim) | +1 (dim) | -h_k (dim, absent for dx = 1) | -dx_k (dim)].  z0 / r0: first variable / row of this trajectory buffer."""
    Z = ld(Z)
    N, z_dim = Z.shape
    h = Z[:-1, dt_off : dt_off + 1]
    dx = Z[:-1, dx_off : dx_off + dim] if dx_off >= 0 else np.ones((N - 1, dim), dtype=LD)
    res = Z[1:, x_off : x_off + dim] - Z[:-1, x_off : x_off + dim] - h * dx
    rows, cols, vals = [], [], []
    r = np.arange(dim)
    for k in range(N - 1):
        rk, vk = r0 + k * dim + index_base + r, z0 + k * z_dim + index_base
        rows += [rk, rk]
        cols += [vk + x_off + r, vk + z_dim + x_off + r]
        vals += [-np.ones(dim, dtype=LD), np.ones(dim, dtype=LD)]
        if dx_off >= 0:
            rows += [rk, rk]
            cols += [vk + dx_off + r, np.full(dim, vk + dt_off)]
            vals += [np.full(dim, -h[k, 0]), -dx[k]]
        else:
            rows += [rk]
            cols += [np.full(dim, vk + dt_off)]
            vals += [-np.ones(dim, dtype=LD)]
    return res.reshape(-1), np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


# ---- reduce payload ------------------------------------------------------------------------------------------------------------------------------
def payload(J_dense, lam, delta, weights, N, z_dim, u_off, m, dt_off, max_job=None):
    """[phi | g_u (K m, k-major) | g_dt (K)] of one output set: g = sum_b w_b J_b' lam_b restricted to (u_k, dt_k), phi = sum_b w_b c <lam_b,
    delta_b> (lam None: lam = delta, c = 1/2).  J_dense: per member the ORACLE's dense Jacobian [K x_dim, N z_dim]; dot products in longdouble.
    max_job: jobs l >= max_job (l < m: d/du_l, l = m: d/ddt, l = m + 1: phi) are dropped (mutant)."""
    K = N - 1
    g, phi = np.zeros(N * z_dim, dtype=LD), LD(0)
    for b, J in enumerate(J_dense):
        w = LD(1) if weights is None else LD(weights[b])
        lb = ld(delta[b] if lam is None else lam[b]).reshape(-1)
        g += w * (ld(J).T @ lb)
        phi += w * (LD(0.5) if lam is None else LD(1)) * _dot(lb, ld(delta[b]).reshape(-1))
    g = g.reshape(N, z_dim)
    gu, gdt = g[:K, u_off : u_off + m].copy(), g[:K, dt_off].copy()
    if max_job is not None:
        gu[:, max_job:] = 0
        if m >= max_job:
            gdt[:] = 0
        if m + 1 >= max_job:
            phi = LD(0)
    return np.concatenate([[phi], gu.reshape(-1), gdt])
