"""Case table of tests/test_robust_shapes_{cpu,gpu}.py (importable without a GPU): the robust-control objective and the rollout of a variational
context (option var_full; pcl_var_objective_kernel, pcl_sens_hess_kernel, pcl_tri_diag_add_kernel, pcl_gather_kernel, the launch code of
pcl_host_robust.hpp, pcl_var_expm_kernel, pcl_var_chain_kernel) on the branch points of that launch code, with np.longdouble truths and mutants.

Systems: drift and variation generators G(H) of dense Hermitians (shape_cases.controlled_hermitians, drift "dense", the variations of the
drift's kind and size), drives as that module draws them.  Knots: 0.4 N(0, 1) in every entry, state and variations alike (O(1)), one entry of
padding in front, z_dim odd: the component rows of the odd knots are not 16-byte aligned.  Q6 and P3 store the components out of order.

Objective cases (unitary, N = 3 unless said; F < 1, terminal state x 0.9, unless said):
    Q1   d =  4  L =   32  v = 2   one pass, nT = 528 even; aligned and 8 bytes off (head and tail peeled together)
    Q2   d = 11  L =  242  v = 1   L < 256 with idle threads, nT = 29,403 odd; terminal state x 1.1: F > 1
    Q3   d = 12  L =  288  v = 2   L just past 256, nT = 41,616 even, aligned and offset; w = [w0, 0, w2]: a regulariser on variation 1 is
                                   not absorbed, one on part of variation 2 is; R replaced and a weight toggled on the open context
    Q4   d = 23  L = 1058  v = 1   1095 sensitivity workgroups, below the cap of 2048
    Q5   d = 26  L = 1352  v = 1   3573 Gram workgroups, below the cap of 4096
    Q6   d = 27  L = 1458  v = 2   2078 / 4155 workgroups: past both caps by a few; knot [Xv2 | X | Xv1 | gap | dt | t | u]; the
                                   eight-regulariser set; R replaced and a weight toggled on the open context
    Q7   d = 32  L = 2048  v = 2   4098 sensitivity, 8196 Gram / scale workgroups; F > 1; aligned and offset; three regularisers of dt_power
                                   0, 1, 2 on the same 700 entries of variation 2
    Q8   d =  6  L =   72  v = 2   subspace goal (levels 0, 2, 5); a regulariser on component 0 absorbed by the Gram triangle; one that
                                   straddles the end of variation 1 and the start of variation 2
    Q9   ket d = 32  L = 64  v = 1   a form of 300 rows with c; regularisers on the state (absorbed) and on the variation (kept)
    Q10  ket d =  5  L = 10  v = 2   a form with c only (R = 0): no triangle, the Hessian is regulariser blocks alone
    Q11  d =  4  L =   32  v = 1   N = 2; 1 - F = 5e-4: just before the kink
    Q12  d = 12  L =  288  v = 1   PCL_BATCH_VARIATIONAL_EXP on Q3's knots (state and variation 2): the Pade context's bits, the same truth
The eight regularisers of Q6: dt_power 0, 1 and 2 on the drives; one on (dt, t), whose range holds dt itself; one on the second half of
variation 1 that runs two entries past its end; one on all of variation 1; two on component 0 with dt_power 0 and 2.

Rollout cases (N = 4; steps per interval from |G(u_k)|_1 and |G(u_k)|_2 as tests/exp_full_cases.py sets them -- 0.2 / |G|_1,
max(2 / |G|_2, 4.5 / |G|_1), -0.5 / |G|_2 -- unless said):
    P1   d = 30  v = 2          five tiles of 149,568 B: the last size with Gv_i in LDS
    P2   d = 29  v = 1          the near side of P1 (144,608 B)
    P3   d = 17  v = 2          column groups 16 + 1; knot [Xv2 | X | Xv1 | ..]
    P4   d = 16  v = 1          exactly one group
    P5   ket d = 5  v = 2       cc = 1, n = 10
    P6   d =  9  v = 2  m = 24  the widest drive loop
    P7   d = 12  v = 2          h |G|_1 = 0.24 (sq = 0), 0.26 (sq = 1), 40 (sq = 8)
    P8   d = 12  v = 1          a zero step (the knot repeats bit for bit) and a negative one
    P9   d = 31  v = 2          PCL_BATCH_VARIATIONAL_EXP, n = 62 (164,448 B: Gv_i from L2); the Pade context's bits

Truths.  Objective: objective_truth's closed forms (form_loss, gram_tril, reg_terms and the goal rows) with the sensitivity term
w s^2 / d^2, s = |x|^2 (gradient 4 w s x / d^2, packed triangle w (4 s [i = j] + 8 x_i x_j) / d^2) and the rule "each position once": a
triangle that exists takes the terminal knot's regulariser diagonals inside its component, the knot's block keeps the rest.  The Hessian is
emitted as the library emits it, [triangles in component order | per-knot blocks | kept slots of the terminal knot], and compared as arrays.
Rollout: the scaled Taylor series of tests/large_full_cases.py (rollout_truth_values) on the lifted problem of tests/variational_truth.py.

Mutants (MUTANTS; CATCHES names the case whose truth differs from each by >= 1e4 x the tolerance, tests/test_robust_shapes_cpu.py asserts it).
A mutant that would change the number of emitted values is written as the assembled matrix sees it: "twice" doubles the absorbed diagonal
at its position, "straddle_first" loses what the second triangle should have taken."""
import functools
import types

import numpy as np

import large_full_cases as lf
import objective_truth as ot
import variational_truth as vt
from oracle import pade_oracle as po
from shape_cases import controlled_hermitians

LD = ot.LD
TOL = 1e-12  # value: TOL max(1, |ref|); gradient and Hessian: TOL max|ref| per segment
ROLL_TOL = 1e-11  # per knot and per component, of max|truth| there
SEEN = 1e4
LDS_BYTES = 163840
SENS_CAP, GRAM_CAP, SCALE_CAP = 2048, 4096, 8192
MUTANTS = ("sens4", "no4s", "drop256", "pass2", "nohead", "notail", "flip", "noweights", "n2", "absorb_twice", "absorb_drop", "absorb_h",
           "straddle_first")  # fmt: skip
# mutant -> (the case that sees it, alignment of the values array in doubles)
CATCHES = {"sens4": ("Q1", 0), "no4s": ("Q1", 0), "drop256": ("Q3", 0), "pass2": ("Q7", 0), "nohead": ("Q1", 1), "notail": ("Q1", 1), "flip": ("Q11", 0),
           "noweights": ("Q1", 0), "n2": ("Q1", 0), "absorb_twice": ("Q8", 0), "absorb_drop": ("Q1", 0), "absorb_h": ("Q7", 0), "straddle_first": ("Q8", 0)}  # fmt: skip


# ---- the launch code's arithmetic (pcl_host_robust.hpp) ---------------------------------------------------------------------------------------
def tri_len(L):
    return L * (L + 1) // 2


def hess_grids(L):
    """(sensitivity, Gram, scale) workgroups before their caps: ceil(ceil(nT / 2) / 256), ceil(nT / 256) twice."""
    nT = tri_len(L)
    return -(-((nT + 1) // 2) // 256), -(-nT // 256), -(-nT // 256)


def roll_lds(n, cols, tiles):
    """var_rollout_dev: (bytes of the expm launch with `tiles` n x n tiles, bytes of the chain launch, state columns per chain workgroup)."""
    ld = ((n + 3) & ~3) + 2
    cc = min(16, cols)
    return (tiles * ld * n + 32 + 64) * 8, (2 * ld * n + 5 * ld * cc) * 8, cc


def gv_in_lds(n):
    return roll_lds(n, 1, 5)[0] <= LDS_BYTES


def squarings(h, G):
    """pcl_var_expm_kernel: theta = |h| |G|_1 halved until it is <= 0.25."""
    theta, sq = abs(float(h)) * float(np.abs(np.asarray(G)).sum(axis=0).max()), 0
    while theta > 0.25 and sq < 60:
        theta *= 0.5
        sq += 1
    return sq


# ---- systems and knots ---------------------------------------------------------------------------------------------------------------------------
def _unitary(d, rng):
    return np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0]


def _iso_vec(U):
    U = np.asarray(U)
    return np.concatenate([np.concatenate([U[:, c].real, U[:, c].imag]) for c in range(U.shape[1])])


def _near(G, scale, rng, eps=0.05):
    d = G.shape[0]
    return scale * G @ (np.eye(d) + eps * (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))) / np.sqrt(d))


def _system(d, m, v, rng):
    """(G0, Gj [m, n, n], [Gv_i]): dense drift, the drives of shape_cases, variation generators of the drift's kind and size."""
    H0, Hd = controlled_hermitians(d, [[l % 3] for l in range(m)], rng, drift="dense")
    Hv = [controlled_hermitians(d, [], rng, drift="dense")[0] for _ in range(v)]
    return po.G_of_H(H0), np.array([po.G_of_H(H) for H in Hd]).reshape(m, 2 * d, 2 * d), [po.G_of_H(H) for H in Hv]


def _knot(L, v, m, order=None, gap=0):
    """[pad | the components in storage `order` | gap | dt | t | u (m) | pad], z_dim odd -> (xo, dt_off, u_off, z_dim)."""
    xo, o = [0] * (v + 1), 1
    for b in order or range(v + 1):
        xo[b] = o
        o += L
    dt_off = o + gap
    z_dim = dt_off + 2 + m + 1
    return xo, dt_off, dt_off + 2, z_dim + 1 - z_dim % 2


def _var_case(d, ket, v, m, N, seed, order=None, gap=0):
    rng = np.random.default_rng(seed)
    n, C = 2 * d, (1 if ket else d)
    G0, Gj, Gv = _system(d, m, v, rng)
    xo, dt_off, u_off, z_dim = _knot(n * C, v, m, order, gap)
    Z = 0.4 * rng.standard_normal((N, z_dim))
    Z[:, dt_off] = 0.05 + 0.1 * rng.random(N)
    return vt.VarCase(Z=Z, z_dim=z_dim, N=N, n=n, C=C, m=m, xo=xo, u_off=u_off, dt_off=dt_off, G0=G0, Gv=Gv, Gj=Gj), rng


def _R(dim, seed):
    return 0.2 + np.random.default_rng(31000 + seed).random(dim)


def _freeze(case):
    for a in [case.Z, case.G0, case.Gj] + list(case.Gv):
        a.setflags(write=False)
    return case


# ---- objective cases ------------------------------------------------------------------------------------------------------------------------------
# name: (d, ket, v, N, m)
OBJ = {"Q1": (4, False, 2, 3, 2), "Q2": (11, False, 1, 3, 2), "Q3": (12, False, 2, 3, 3), "Q4": (23, False, 1, 3, 2), "Q5": (26, False, 1, 3, 2),
       "Q6": (27, False, 2, 3, 3), "Q7": (32, False, 2, 3, 2), "Q8": (6, False, 2, 3, 2), "Q9": (32, True, 1, 3, 2), "Q10": (5, True, 2, 3, 2),
       "Q11": (4, False, 1, 2, 2), "Q12": (12, False, 1, 3, 3)}  # fmt: skip
OBJ_NAMES = tuple(OBJ)
OFFSET_CASES = ("Q1", "Q3", "Q7")  # the values array also 8 bytes off a 16-byte boundary
REOPEN_CASES = ("Q3", "Q6")  # R replaced, a weight set to zero and back, on the open context
F_ABOVE = ("Q2", "Q7")
SUB8 = [0, 2, 5]


def _seed(name):
    return 33000 + 19 * int(name[1:])


def _form_state(A, c, x, target):
    """x scaled so that F(x) = c'x + sum_r (A_r'x)^2 is `target`."""
    lin = float(c @ x) if c is not None else 0.0
    q = float(((A @ x) ** 2).sum()) if A is not None else 0.0
    return x * ((-lin + np.sqrt(lin * lin + 4 * q * target)) / (2 * q) if q else target / lin)


@functools.lru_cache(maxsize=None)
def obj_case(name):
    """A namespace: vc (VarCase), goal, w, Q, sigma, regs, regs2 (the same offsets and sizes, other R; None where the context is not reopened),
    toggle (the weight set to zero and back), exp.  goal: ("unitary", G) | ("subspace", Gs, sub) | ("form", A, c)."""
    if name == "Q12":
        q3 = obj_case("Q3")
        c3 = q3.vc
        vc = vt.VarCase(Z=c3.Z, z_dim=c3.z_dim, N=c3.N, n=c3.n, C=c3.C, m=c3.m, xo=[c3.xo[0], c3.xo[2]], u_off=c3.u_off, dt_off=c3.dt_off, G0=c3.G0,
                        Gv=[c3.Gv[1]], Gj=c3.Gj)  # fmt: skip
        return types.SimpleNamespace(name=name, vc=vc, goal=q3.goal, w=np.array([q3.w[0], q3.w[2]]), Q=q3.Q, sigma=q3.sigma, regs=q3.regs, regs2=None,
                                     toggle=None, exp=True)  # fmt: skip
    d, ket, v, N, m = OBJ[name]
    order, gap = ([2, 0, 1], 2) if name == "Q6" else (None, 0)
    vc, rng = _var_case(d, ket, v, m, N, _seed(name), order, gap)
    L, xo, u_off, dt_off = vc.xdc, vc.xo, vc.u_off, vc.dt_off
    x0 = slice(xo[0], xo[0] + L)
    s = _seed(name)
    w = np.array([0.7, 0.3, 1.9])[: v + 1]
    regs2 = toggle = None
    if name == "Q8":
        Gs = _unitary(3, rng)
        U = 0.3 * (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
        U[np.ix_(SUB8, SUB8)] = _near(Gs, 0.9, rng)
        vc.Z[-1, x0] = _iso_vec(U)
        goal = ("subspace", Gs, SUB8)
    elif ket:
        R = 300 if name == "Q9" else 0
        A = rng.standard_normal((R, L)) / np.sqrt(L) if R else None
        c = rng.standard_normal(L) / np.sqrt(L)
        vc.Z[-1, x0] = _form_state(A, c, vc.Z[-1, x0], 0.6)
        goal = ("form", A, c)
        w = np.array([1.3, 0.0, 0.0])[: v + 1]
    else:
        G = _unitary(d, rng)
        U = _near(G, 1.1 if name in F_ABOVE else 0.9, rng)
        if name == "Q11":  # F is quadratic in the state: scaled to 1 - 5e-4
            U = U * np.sqrt((1 - 5e-4) / float(ot.unitary_fidelity(_iso_vec(U), G)))
        vc.Z[-1, x0] = _iso_vec(U)
        goal = ("unitary", G)
    drives = (u_off, m, _R(m, s), 2)
    if name == "Q1":
        regs = [drives, (xo[1], L, _R(L, s + 1), 1)]
    elif name == "Q3":
        w = np.array([0.7, 0.0, 1.9])
        regs = [drives, (xo[1], L, _R(L, s + 1), 1), (xo[2] + 10, 50, _R(50, s + 2), 0)]
        regs2 = [(o, dim, _R(dim, s + 10 + i), p) for i, (o, dim, _, p) in enumerate(regs)]
        toggle = 2
    elif name == "Q6":
        h2 = L // 2
        regs = [(u_off, m, _R(m, s), 0), (u_off, m, _R(m, s + 1), 1), (u_off, m, _R(m, s + 2), 2), (dt_off, 2, _R(2, s + 3), 1),
                (xo[1] + h2, L - h2 + 2, _R(L - h2 + 2, s + 4), 2), (xo[1], L, _R(L, s + 5), 1), (xo[0], L, _R(L, s + 6), 0), (xo[0], L, _R(L, s + 7), 2)]  # fmt: skip
        regs2 = [(o, dim, _R(dim, s + 10 + i), p) for i, (o, dim, _, p) in enumerate(regs)]
        toggle = 1
    elif name == "Q7":
        regs = [drives] + [(xo[2] + 100, 700, _R(700, s + 1 + p), p) for p in (0, 1, 2)]
    elif name == "Q8":
        regs = [drives, (xo[0], L, _R(L, s + 1), 1), (xo[1] + L - 20, 40, _R(40, s + 2), 2)]
        assert xo[2] == xo[1] + L
    elif name == "Q9":
        regs = [drives, (xo[0], L, _R(L, s + 1), 1), (xo[1], L, _R(L, s + 2), 0)]
    elif name == "Q10":
        regs = [drives, (xo[0], L, _R(L, s + 1), 2), (xo[2], L, _R(L, s + 2), 1)]
    elif name in ("Q4", "Q5"):
        regs = [(u_off, m, _R(m, s), 1 if name == "Q4" else 0)]
    else:
        regs = [drives]
    _freeze(vc)
    return types.SimpleNamespace(name=name, vc=vc, goal=goal, w=w, Q=100.0, sigma=0.8, regs=regs, regs2=regs2, toggle=toggle, exp=False)


# ---- the objective's truth -------------------------------------------------------------------------------------------------------------------------
def _first256(n):
    return np.arange(n) < 256


@functools.lru_cache(maxsize=None)
def goal_rows(name, drop=False):
    """(A, c) of the loss of component 0 in longdouble; drop: the sums of the goal lose their elements beyond 256 (mutant)."""
    q = obj_case(name)
    g, d = q.goal, q.vc.n // 2
    if g[0] == "unitary":
        return ot.unitary_rows(g[1], _first256(d * d) if drop else None), None
    if g[0] == "subspace":
        return ot.subspace_rows(g[1], g[2], d, _first256(len(g[2]) ** 2) if drop else None), None
    return (None if g[1] is None else ot.ld(g[1])), (None if g[2] is None else ot.ld(g[2]))


@functools.lru_cache(maxsize=None)
def _gram(name):
    A = goal_rows(name)[0]
    T = ot.gram_tril(A)
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def _outer(name, b):
    """x x' of the terminal variation b, packed lower triangle, row-major."""
    q = obj_case(name)
    x = ot.ld(q.vc.Z[-1, q.vc.xo[b] : q.vc.xo[b] + q.vc.xdc])
    T = np.outer(x, x)[np.tril_indices(len(x))]
    T.setflags(write=False)
    return T


def _weights(q, w, mut):
    w = np.asarray(q.w if w is None else w, dtype=float)
    return np.ones_like(w) if mut == "noweights" else w


def _sens_s(x, mut):
    x = ot.ld(x)
    return (x[:256] * x[:256]).sum() if mut == "drop256" else (x * x).sum()


def _dd(q, mut):
    d = q.vc.n // 2
    return LD(4 * d * d) if mut == "n2" else LD(d * d)


def objective_truth(name, mut=None, regs=None, w=None):
    """(value, gradient [N, z_dim], F of the goal) in longdouble."""
    q = obj_case(name)
    vc = q.vc
    regs, w = (q.regs if regs is None else regs), _weights(q, w, mut)
    rv, grad, _ = ot.reg_terms(vc.Z, regs, vc.dt_off, _first256 if mut == "drop256" else None)
    value = rv.sum()
    A, c = goal_rows(name, mut == "drop256")
    keepL = _first256(vc.xdc) if mut == "drop256" and q.goal[0] == "form" else None
    val, g, _, F = ot.form_loss(A, c, vc.Z[-1, vc.xo[0] : vc.xo[0] + vc.xdc], LD(w[0]) * LD(q.Q), keepL, mut == "flip")
    value = value + val
    grad[-1, vc.xo[0] : vc.xo[0] + vc.xdc] += g
    dd = _dd(q, mut)
    for b in range(1, vc.v + 1):
        if w[b] == 0:
            continue
        x = ot.ld(vc.Z[-1, vc.xo[b] : vc.xo[b] + vc.xdc])
        s = _sens_s(x, mut)
        value = value + LD(w[b]) * s * s / dd
        grad[-1, vc.xo[b] : vc.xo[b] + vc.xdc] += 4 * LD(w[b]) * s * x / dd
    return value, grad, F


def triangles(name, w=None):
    """Components with a triangle, in emission order: 0 under a goal with quadratic rows, then every variation with a weight."""
    q = obj_case(name)
    w = q.w if w is None else w
    return ([0] if goal_rows(name)[0] is not None and len(goal_rows(name)[0]) else []) + [b for b in range(1, q.vc.v + 1) if w[b] != 0]


def hessian_truth(name, mut=None, regs=None, w=None, head=0, structure=False):
    """sigma grad^2 J as the library emits it: (values, segments [(label, start, stop)], (rows, cols) or None), 0-based.  head: the values
    array starts `head` doubles off a 16-byte boundary (only the peeling mutants look at it)."""
    q = obj_case(name)
    vc = q.vc
    regs, w = (q.regs if regs is None else regs), _weights(q, w, mut)
    N, zd, L, nT = vc.N, vc.z_dim, vc.xdc, tri_len(vc.xdc)
    sig, dd = LD(q.sigma), _dd(q, mut)
    zN = ot.ld(vc.Z[-1])
    h = zN[vc.dt_off]
    tri = triangles(name, w)
    parts, segs, rows, cols = [], [], [], []
    diag_pos = np.arange(L) * (np.arange(L) + 1) // 2 + np.arange(L)
    ti, tj = np.tril_indices(L) if structure and tri else (None, None)
    for t, b in enumerate(tri):
        if b == 0:
            A, c = goal_rows(name)
            _, _, s, _ = ot.form_loss(A, c, zN[vc.xo[0] : vc.xo[0] + L], LD(1), None, mut == "flip")
            T = (-s * LD(w[0]) * LD(q.Q) * sig) * _gram(name)
        else:
            x = zN[vc.xo[b] : vc.xo[b] + L]
            c = sig * LD(w[b]) / dd
            T = (c * (4 if mut == "sens4" else 8)) * _outer(name, b)
            if mut != "no4s":
                T[diag_pos] += 4 * c * _sens_s(x, mut)
            hd = (head + t * nT) % 2
            if mut == "pass2":
                T[hd + 2 * SENS_CAP * 256 : hd + 2 * ((nT - hd) // 2)] = 0
            if mut == "nohead" and hd:
                T[0] = 0
            if mut == "notail" and (nT - hd) % 2:
                T[nT - 1] = 0
        parts.append(T)
        if structure:
            z0 = (N - 1) * zd + vc.xo[b]
            rows.append(z0 + ti), cols.append(z0 + tj)
    # the rule "each position once": the terminal knot's regulariser diagonals inside a component with a triangle are the triangle's
    kept, slot = [], 0
    for off, dim, R, p in regs:
        R = np.broadcast_to(ot.ld(R), (dim,))
        z = off + np.arange(dim)
        owner = np.full(dim, -1)
        for t, b in enumerate(tri):
            owner[(owner < 0) & (z >= vc.xo[b]) & (z < vc.xo[b] + L)] = t
        owners = [t for t in range(len(tri)) if (owner == t).any()]
        for t in owners:
            sel = owner == t
            hp = h if (p == 2 and mut == "absorb_h") else h**p if p else LD(1)
            f = 0 if mut == "absorb_drop" or (mut == "straddle_first" and t != owners[0]) else 2 if mut == "absorb_twice" else 1
            parts[t][diag_pos[z[sel] - vc.xo[tri[t]]]] += f * sig * hp * R[sel]
        kept += list(slot + np.flatnonzero(owner < 0))
        rest = (dim if p >= 1 else 0) + (1 if p == 2 else 0)
        kept += list(range(slot + dim, slot + dim + rest))
        slot += dim + rest
    e = 0
    for t, b in enumerate(tri):
        segs.append(("tri@%d" % b, e, e + nT))
        e += nT
    if slot:
        _, _, (hk, hr, hc, hv) = ot.reg_terms(vc.Z, regs, vc.dt_off)
        blk, br, bc = (a.reshape(slot, N).T for a in (sig * hv, hr, hc))  # [knot, slot]
        kept = np.array(kept, dtype=int)
        for k in range(N):
            sel = np.arange(slot) if k < N - 1 else kept
            if len(sel):
                parts.append(blk[k, sel])
                segs.append(("knot@%d" % k, e, e + len(sel)))
                e += len(sel)
                if structure:
                    rows.append(k * zd + br[k, sel]), cols.append(k * zd + bc[k, sel])
    values = np.concatenate(parts) if parts else np.zeros(0, dtype=LD)
    return values, segs, ((np.concatenate(rows), np.concatenate(cols)) if structure and rows else None)


def grad_labels(name, regs=None, w=None):
    """Segment of every gradient entry: a regulariser's range per knot ("k1.r2"; the first that covers an entry), dt per knot, the terminal
    component rows that carry a term ("x0", "x2"); "zero" for what no term touches."""
    q = obj_case(name)
    vc = q.vc
    regs, w = (q.regs if regs is None else regs), (q.w if w is None else w)
    lab = np.full((vc.N, vc.z_dim), "zero", dtype="U12")
    for k in range(vc.N):
        if any(p >= 1 for _, _, _, p in regs):
            lab[k, vc.dt_off] = "k%d.dt" % k
        for r in range(len(regs) - 1, -1, -1):
            lab[k, regs[r][0] : regs[r][0] + regs[r][1]] = "k%d.r%d" % (k, r)
    for b in range(vc.v + 1):
        if b == 0 or w[b] != 0:
            lab[-1, vc.xo[b] : vc.xo[b] + vc.xdc] = "x%d" % b
    return lab


def check_value(got, ref):
    err = abs(LD(got) - ref) / max(LD(1), abs(ref))
    assert np.isfinite(got) and err <= TOL, "value %r against %r (rel %.3e)" % (got, float(ref), float(err))
    return float(err)


def segment_errors(got, ref, segs):
    """{label: max|got - ref| / max|ref|} over contiguous segments (a segment whose truth is zero: the absolute error)."""
    out = {}
    for lab, a, b in segs:
        scale, err = np.abs(ref[a:b]).max(), np.abs(got[a:b] - ref[a:b]).max()
        out[lab] = float(err / scale) if scale > 0 else float(err)
    return out


def mutant_distance(name, mut, head=0):
    """The largest relative distance of the mutant's truth from the truth, over the value, the gradient's segments and the Hessian's."""
    v0, g0, _ = objective_truth(name)
    v1, g1, _ = objective_truth(name, mut)
    lab = grad_labels(name).reshape(-1)
    worst = float(abs(v1 - v0) / max(LD(1), abs(v0)))
    a, b = g0.reshape(-1), g1.reshape(-1)
    for s in np.unique(lab):
        sel = lab == s
        if np.abs(a[sel]).max() > 0:
            worst = max(worst, float(np.abs(a[sel] - b[sel]).max() / np.abs(a[sel]).max()))
    h0, segs, _ = hessian_truth(name, head=head)
    h1, _, _ = hessian_truth(name, mut, head=head)
    return max([worst] + list(segment_errors(h1, h0, segs).values()))


# ---- rollout cases --------------------------------------------------------------------------------------------------------------------------------
# name: (d, ket, v, m, storage order, steps, PCL_BATCH_VARIATIONAL_EXP); steps: ("norms",) the default, ("theta", h |G|_1 per interval), ("zero",)
ROLL = {
    "P1": (30, False, 2, 2, None, ("norms",), False), "P2": (29, False, 1, 2, None, ("norms",), False), "P3": (17, False, 2, 3, [2, 0, 1], ("norms",), False),
    "P4": (16, False, 1, 2, None, ("norms",), False), "P5": (5, True, 2, 2, None, ("norms",), False), "P6": (9, False, 2, 24, None, ("norms",), False),
    "P7": (12, False, 2, 2, None, ("theta", (0.24, 0.26, 40.0)), False), "P8": (12, False, 1, 2, None, ("zero",), False),
    "P9": (31, False, 2, 2, None, ("norms",), True),
}  # fmt: skip
ROLL_NAMES = tuple(ROLL)
ROLL_N = 4
# the bound of a case: "component" (per knot and component) where the float64 lifted oracle is within ROLL_TOL / 10 of the truth per knot and
# component, else "array" (the whole array, the rule of tests/test_variational_rollout_gpu.py); tests/test_robust_shapes_cpu.py holds this table
# to the oracle's distance
ROLL_RULE = {name: "component" for name in ROLL}


def g_of(case, k):
    return case.G0 + np.tensordot(case.Z[k, case.u_off : case.u_off + case.m], case.Gj, axes=1)


@functools.lru_cache(maxsize=None)
def roll_case(name):
    d, ket, v, m, order, steps, _ = ROLL[name]
    case, _ = _var_case(d, ket, v, m, ROLL_N, 35000 + 23 * int(name[1:]), order)
    for k in range(ROLL_N - 1):
        G = g_of(case, k)
        n1, n2 = np.abs(G).sum(axis=0).max(), np.linalg.norm(G, 2)
        if steps[0] == "theta":
            case.Z[k, case.dt_off] = steps[1][k] / n1
        elif steps[0] == "zero":
            case.Z[k, case.dt_off] = (0.2 / n1, 0.0, -0.5 / n2)[k]
        else:
            case.Z[k, case.dt_off] = (0.2 / n1, max(2.0 / n2, 4.5 / n1), -0.5 / n2)[k]
    case.Z[:, case.dt_off + 1] = np.cumsum(case.Z[:, case.dt_off])
    return _freeze(case)


@functools.lru_cache(maxsize=None)
def roll_truth_ld(name):
    """[N, (1 + v) n C] stacked states in longdouble: the scaled Taylor series on the lifted problem, rows mapped back."""
    case = roll_case(name)
    Zl, lay, G0l, Gjl = vt.lifted(case)
    X = lf.rollout_truth_values(lay, G0l, Gjl, Zl)
    out = np.empty_like(X)
    out[:, vt._row_map(case)] = X
    out.setflags(write=False)
    return out


def roll_errors(got, truth, case):
    """[N, 1 + v]: max|got - truth| / max|truth| per knot and component (stacked order: component b holds [b xdc, (b + 1) xdc))."""
    g, t = (np.asarray(a).reshape(case.N, case.v + 1, case.xdc) for a in (got, truth))
    return (np.abs(g - t).max(axis=2) / np.abs(t).max(axis=2)).astype(float)
