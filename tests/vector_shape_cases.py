"""Cases that walk the Pade kernels over the states that are not a square unitary -- kets, multi-ket states and density vectors -- at the
sizes at which the launch code (piccolo.jl_amd/csrc/pcl_host_launch_pade.hpp, pcl_host_launch_hess.hpp) and the kernels branch; importable without a GPU.

Generators are random and dense, so that edge rows, edge columns and the last k steps of every product carry weight:
    iso    G(H) of a dense complex Hermitian H (ket or multi-ket state, n = 2 d); K5 alone takes po.config_system(3)'s generators
    vec    a general real n x n matrix / sqrt(n) under PCL_STATE_VECTOR (not normal, odd n allowed, one column)
Knot: [X | dt | t | u], u ~ 0.4 N(0, 1), N = 4.  The three steps are fixed per case from G(u_k):
    interval 0   h |G|_2 = 0.15
    interval 1   h |G|_2 = -0.3                          a negative step
    interval 2   h |G|_2 = the long step: the smallest of LONG_STEPS at which zeroing the top coefficient c_5 of order 10 moves the
                 interval's residual by 1e-7 of its own size or more (1e4 x the GPU tolerance).  A random non-normal generator needs
                 more than a skew one: |G x| of a random x is well below |G|_2 |x|.

Cases (kind, n, cols, m), the branch each straddles and the long step chosen:
    K1  iso 18 1  2   first ket past the small kernel; kernel 10 at order 4; two row tiles in the lock-step kernel              0.5
    K2  iso 34 1  3   first d past kernel 10 (kernel 20); three row tiles: one idle wave (16 % 3), two-row edge tile             0.5
    K3  iso 44 1  1   n^2 / 2 = 968 <= 1024: one B+- pair per thread                                                            0.5
    K4  iso 46 1  1   n^2 / 2 = 1058: the second pair partly used                                                               0.5
    K5  iso 54 1  6   config 3's generators as a ket: Hessian kernel 2 with one column, the compile-time 27 / 6 instance         0.5
    K6  iso 64 1  6   largest n: two full pairs per thread, four full row tiles, 21 drive pairs in the general Hessian          0.5
    K7  iso 10 1 24   the ABI's most drives: 300 pairs and 325 scalars in the general Hessian's pair decode and `red` rows      0.5
    M1  iso 12 5  4   lock-step slices S = 5, npc = 3: the last slice has no column of the powers; small kernel for `eval`      0.5
    M2  iso 20 7  2   uneven lock-step slices (npc = 3, the last 2); a column count neither 1 nor d in kernels 10 / 1           0.5
    M3  iso 60 7  6   general Hessian in column chunks of 2, 2, 2, 1 (LDS); kernel 20 with 7 of 30 columns; lock-step S = 7,     0.5
                      npc = 9, the last slice 6 columns
    M4  iso 54 5  6   (added to the issue's table) config 3's generators on five kets: Hessian kernel 2, the 27 / 6 instance, with      0.5
                      more than one column and, under cols_per_slice, partial sums over column slices; lock-step npc = 11, last 10
    V1  vec 15 1  8   the small kernel's 16-row instance, odd n, most drives, `eval` alone; reference formulation for eval_jac  0.8
    V2  vec 16 1  2   last small-kernel size; lock-step at exactly one row tile                                                0.65
    V3  vec 17 1  2   first size past it, odd: the reference formulation for everything                                        0.65
    V4  vec 36 1  3   6-level density size, even: lock-step under PCL_STATE_VECTOR                                             0.65
    V5  vec 49 1  3   7-level density size, n mod 16 = 1                                                                        0.8
    V6  vec 63 1  2   largest odd n                                                                                            0.65
    V7  vec 64 1  2   largest even n under PCL_STATE_VECTOR                                                                    0.65
No shape had to move: tests/test_vector_shapes_cpu.py recomputes every slice, pair, chunk and byte count above with the launch code's own
arithmetic, restated below (lockstep_plan, pade_lds_bytes, hess_general_chunk, hess2_lds_bytes, fused_lds_bytes, fused2_lds_bytes).

The truth (`truth_values`) restates the residual, the Jacobian values and the values of the Hessian of the Lagrangian in np.longdouble from
the definition
    delta = sum_j c_j (-h)^j G^j X_{k+1} - sum_j c_j h^j G^j X_k,
the derivatives by the product rule over the positions of G in G^j (every word G^a G_i G^b G_l G^c applied to a thin matrix), in the
library's value order.  It shares no code with oracle/pade_oracle.py, takes the coefficient vector (a test can zero c_q) and sends every
product through one `mm` hook, where tests/test_vector_shapes_cpu.py injects faults.  The GPU tests compare with it rounded to float64.

Reference floor: the largest deviation of po.pade_residual / pade_jacobian_values / pade_hessian_values from this truth per segment,
relative to the segment's own maximum, over every case and order (tests/test_vector_shapes_cpu.py asserts 1e-13 and prints them):
    residual 4.4e-16 (delta@0, V5, order 10)    Jacobian 4.4e-16 (B+@0, V5, order 8)    Hessian 6.8e-15 (uu@1, K4, order 4)
No case had to be reseeded (RESEED is empty)."""
import functools
import math

import numpy as np

from oracle import pade_oracle as po
from shape_cases import hess_labels, jac_labels, per_interval

N = 4
LDS_BYTES = 163840
ORDERS = (2, 4, 6, 8, 10)
LONG_STEPS = (0.5, 0.65, 0.8, 1.0, 1.25, 1.5)
SEEN = 1e-7
LD_ = np.longdouble

# name: (kind, n, cols, m)
CASES = {
    "K1": ("iso", 18, 1, 2), "K2": ("iso", 34, 1, 3), "K3": ("iso", 44, 1, 1), "K4": ("iso", 46, 1, 1), "K5": ("iso", 54, 1, 6),
    "K6": ("iso", 64, 1, 6), "K7": ("iso", 10, 1, 24), "M1": ("iso", 12, 5, 4), "M2": ("iso", 20, 7, 2), "M3": ("iso", 60, 7, 6),
    "M4": ("iso", 54, 5, 6), "V1": ("vec", 15, 1, 8), "V2": ("vec", 16, 1, 2), "V3": ("vec", 17, 1, 2), "V4": ("vec", 36, 1, 3), "V5": ("vec", 49, 1, 3),
    "V6": ("vec", 63, 1, 2), "V7": ("vec", 64, 1, 2),
}  # fmt: skip
MULTI = tuple(c for c in CASES if CASES[c][2] > 1)
EVEN = tuple(c for c in CASES if CASES[c][1] % 2 == 0)
# a case whose scalar segment near-cancels draws from another seed: name -> how many seeds further (none needed)
RESEED = {}


# ---- the launch code's arithmetic (pcl_host_launch_*.hpp) ------------------------------------------------------------------------------------------
def lds_ld(n):
    return ((n + 3) & ~3) + 2


def lockstep_plan(n, cols, m, items=N - 1, n_cu=256, slices=0):
    """launch_pade_v2: None where the kernel does not take the shape, else the slice count S, the state columns nc and power columns npc per
    slice, what each slice really holds (nce, npce), the LDS bytes (lds_of, without the drives' ELL rows), and per workgroup of 16 waves the
    row tiles, the idle waves and the B+- pairs a thread owns at most."""
    if n % 2 or n > 64 or n < 2:
        return None
    LD = n | 1
    lds_of = lambda S: (((2 + 2 * (2 + m)) * -(-cols // S) + n + -(-n // S)) * LD + 80 + m + 8) * 8
    s_max, S = max(cols, 1), 1
    while S < s_max and lds_of(S) > LDS_BYTES:
        S += 1
    if lds_of(S) > LDS_BYTES:
        return None
    S = max(S, min(slices, s_max)) if slices > 0 else max(S, min(s_max, n_cu // max(items, 1)))
    nc, npc, rt = -(-cols // S), -(-n // S), (n + 15) // 16
    return dict(S=S, nc=nc, npc=npc, nce=[max(0, min(nc, cols - s * nc)) for s in range(S)], npce=[max(0, min(npc, n - s * npc)) for s in range(S)],
                bytes=lds_of(S), row_tiles=rt, idle_waves=16 % rt, pairs=-(-(n * npc // 2) // 1024), last_pair_used=n * npc // 2 - 1024)  # fmt: skip


def pade_lds_bytes(n, m, q, nc, jac):
    """pade_lds_bytes of the reference formulation (pcl_pade_kernel)."""
    LD = lds_ld(n)
    return ((3 if jac else 1) * LD * n + ((q + 1) + 2 + (2 + 2 * m if jac else 0)) * LD * nc + 8 + m) * 8


def reference_cols(n, cols, m, q, jac):
    """launch_pade_general: the state columns per workgroup of pcl_pade_kernel."""
    nc = cols
    while nc > 1 and pade_lds_bytes(n, m, q, nc, jac) > LDS_BYTES:
        nc -= 1
    return nc


def hess_general_bytes(n, m, nc):
    """the `bytes` lambda of the general-order Hessian launch."""
    npair, nsc = m * (m + 1) // 2, (m + 1) * (m + 2) // 2
    return (lds_ld(n) * n + (6 + 4 * m + 2 * npair) * lds_ld(n) * nc + 8 + m + 4 * nsc) * 8


def hess_general_chunk(n, cols, m):
    """(columns per chunk, the chunks' widths) of pcl_hess_general_kernel."""
    nc = cols
    while nc > 1 and hess_general_bytes(n, m, nc) > LDS_BYTES:
        nc = (nc + 1) // 2
    return nc, [min(nc, cols - c) for c in range(0, cols, nc)]


def hess2_lds_bytes(n, m):
    return (lds_ld(n) * n + 7 * lds_ld(n) * 16 + 4 * ((m + 1) * (m + 2) // 2) + 4 + 2) * 8


def hess1_lds_bytes(n, m, nc):
    return (lds_ld(n) * n + (6 + 3 * m) * lds_ld(n) * nc + 8 + m + 5 * ((m + 1) * (m + 2) // 2)) * 8


def fused_lds_bytes(n, m, nc, jac):
    LD, c1 = lds_ld(n), ((2 + m) if jac else 2) * nc
    return (LD * n * (2 if jac else 1) + 2 * LD * c1 + 2 * LD * nc + 8 + m) * 8


def fused2_lds_bytes(n, m, nc, jac, ell_w=0):
    """fused2_lds_bytes; ell_w > 0: with the drives' ELL rows staged in LDS."""
    LD, c1 = lds_ld(n), ((2 + m) if jac else 2) * nc
    b = (LD * n * (2 if jac else 1) + 2 * LD * c1 + LD * nc + 2 * (m + 1)) * 8
    if jac and ell_w:
        b += m * n * ell_w * 8 + (m * n * ell_w * 2 + 7) // 8 * 8
    return b + 128


def drive_width(Gj):
    """The most entries a drive has in one row or one column (the launch code's ell_w / ellt_w)."""
    nz = np.asarray(Gj) != 0
    return int(max(nz.sum(axis=2).max(), nz.sum(axis=1).max())) if len(Gj) else 0


def expected_family(name, order):
    """(last_kernel after eval_jac, last_kernel after eval, last_hess_kernel) that `auto` takes, read from launch_fused / launch_pade_general /
    launch_hess: 190 + q lock-step (even n), 90 + q reference formulation, 50 + q the small kernel (n <= 16, cols <= 8, m <= 8: for the residual
    alone, and for eval_jac only at n <= 8), 10 / 20 the fused order-4 kernels (d <= 16 / above), Hessian 1 / 2 at order 4 (2: one to six drives of
    at most two entries per row and column), 90 + q above.  A PCL_STATE_VECTOR context takes the general-order launch at order 4 as well."""
    kind, n, cols, m = CASES[name]
    q = order // 2
    small = n <= 16 and cols <= 8 and m <= 8
    if order != 4 or kind == "vec":
        return (190 + q if n % 2 == 0 else 90 + q), (50 + q if small else 90 + q), (90 + q if order != 4 else 1)
    fused = 10 if n // 2 <= 16 else 20
    width = drive_width(system(name)[1])
    return (50 + q if small and n <= 8 else fused), (50 + q if small else fused), (2 if 1 <= m <= 6 and width <= 2 else 1)


# ---- systems and trajectories ----------------------------------------------------------------------------------------------------------------
def _herm(d, rng):
    A = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return (A + A.conj().T) / 2


def _seed(name):
    return 12000 + 17 * int(name[1:]) + {"K": 0, "M": 300, "V": 600}[name[0]] + 5 * RESEED.get(name, 0)


def system(name, drift=0):
    """(G0, Gj).  drift > 0: another drift for the same drives (a member of a PCL_BATCH_MEMBERS launch)."""
    kind, n, cols, m = CASES[name]
    rng = np.random.default_rng(_seed(name))
    if kind == "vec":
        G0s = [rng.standard_normal((n, n)) / np.sqrt(n) for _ in range(3)]
        Gj = rng.standard_normal((m, n, n)) / np.sqrt(n)
    else:
        d = n // 2
        G0s = [po.G_of_H(_herm(d, rng)) for _ in range(3)]
        Gj = np.array([po.G_of_H(_herm(d, rng)) for _ in range(m)])
        if name in ("K5", "M4"):  # config 3's own system: three 3-level transmons, six drives of two entries per row
            s3 = po.config_system(3)
            assert s3.levels == d and s3.n_drives == m
            G0s[0], Gj = s3.G_drift, np.array(s3.G_drives)
    return G0s[drift], Gj


def layout(name, members=1):
    """members > 1: the multi-ket integrator's knot [X_0 | X_1 | .. | dt | t | u], member i at x_off = i x_dim."""
    kind, n, cols, m = CASES[name]
    xs = members * n * cols
    if kind == "vec":
        return po.Layout(d=0, m=m, N=N, z_dim=xs + 2 + m, x_off=0, u_off=xs + 2, dt_off=xs, cols=1, gen=n)
    return po.Layout(d=n // 2, m=m, N=N, z_dim=xs + 2 + m, x_off=0, u_off=xs + 2, dt_off=xs, cols=cols)


def g_of(lay, Z, k, G0, Gj):
    return G0 + np.tensordot(Z[k, lay.u_off : lay.u_off + lay.m], Gj, axes=1) if lay.m else G0


def top_term_weight(lay, G0, Gj, Z, k=2, order=10):
    """By how much zeroing c_q moves interval k's residual, relative to the residual's own maximum."""
    c = coeffs(order)
    c0 = c.copy()
    c0[-1] = 0
    a = truth_values(lay, G0, Gj, Z, None, order, c=c, intervals=(k,), hessian=False)[0]
    b = truth_values(lay, G0, Gj, Z, None, order, c=c0, intervals=(k,), hessian=False)[0]
    return float(np.abs(a - b).max() / np.abs(a).max())


@functools.lru_cache(maxsize=None)
def case(name, seed=0, drift=0, members=1):
    """(layout, G0, Gj, Z, long step), read-only.  seed: another trajectory of the same system (a seed of a PCL_BATCH_TRAJ launch).  drift: the
    member's drift on the SAME trajectory -- the members of a PCL_BATCH_MEMBERS launch share the knots, so the steps are those of drift 0."""
    lay = layout(name, members)
    G0, Gj = system(name, 0)
    rng = np.random.default_rng(_seed(name) + 1 + seed + 100 * (members - 1))
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    n2 = [np.linalg.norm(g_of(lay, Z, k, G0, Gj), 2) for k in range(N - 1)]
    Z[0, lay.dt_off], Z[1, lay.dt_off], Z[N - 1, lay.dt_off] = 0.15 / n2[0], -0.3 / n2[1], 0.1
    long_step = None
    for s in LONG_STEPS:
        Z[2, lay.dt_off] = s / n2[2]
        if top_term_weight(lay, G0, Gj, Z) >= SEEN:
            long_step = s
            break
    assert long_step is not None, name
    Z[:, lay.dt_off + 1] = np.cumsum(Z[:, lay.dt_off])
    G0 = system(name, drift)[0]
    for a in (G0, Gj, Z):
        a.setflags(write=False)
    return lay, G0, Gj, Z, long_step


def with_step(lay, G0, Gj, Z, k, theta):
    """A copy of Z with interval k's step at h |G(u_k)|_2 = theta."""
    Z = np.array(Z)
    Z[k, lay.dt_off] = theta / np.linalg.norm(g_of(lay, Z, k, G0, Gj), 2)
    return Z


def rand_mu(size, name, member=0):
    mu = np.random.default_rng(_seed(name) + 77 + member).standard_normal(size)
    mu.setflags(write=False)
    return mu


def residual_labels(lay):
    return per_interval(np.full(lay.x_dim, "delta"), lay.K)


def rollout_labels(lay):
    return np.repeat(np.array(["knot%d" % k for k in range(lay.N)]), lay.x_dim)


# ---- the truth, in np.longdouble -----------------------------------------------------------------------------------------------------------------
def coeffs(order):
    """c_j = (2q - j)! q! / ((2q)! j! (q - j)!), exact integers divided once."""
    q, f = order // 2, math.factorial
    return np.array([LD_(f(2 * q - j) * f(q)) / LD_(f(2 * q) * f(j) * f(q - j)) for j in range(q + 1)], dtype=LD_)


def _mm(A, B):
    return A @ B


def _chain(mm, A, V, k):
    """[V, A V, .., A^k V]"""
    out = [V]
    for _ in range(k):
        out.append(mm(A, out[-1]))
    return out


def _flat(A):
    return A.T.reshape(-1)


def truth_interval(Zk, Zk1, mu_k, lay, G0, Gl, c, x_off, mm=_mm, hessian=True, drop_drive=False, drop_col=False):
    """(delta [x_dim], Jacobian values, Hessian values | None) of one interval in longdouble.  G0, Gl: longdouble.  drop_drive: G(u) formed
    without the last drive.  drop_col: the last state column (of X_k, X_k+1 and mu) read as zero."""
    n, C, m, q = lay.n, lay.C, lay.m, len(c) - 1
    xd = n * C
    h = LD_(Zk[lay.dt_off])
    u = np.asarray(Zk[lay.u_off : lay.u_off + m], dtype=LD_)
    G = G0.copy()
    for l in range(m - (1 if drop_drive else 0)):
        G = G + u[l] * Gl[l]
    col = lambda v: np.array(np.asarray(v, dtype=LD_).reshape(C, n).T)
    Xc, Xn = col(Zk[x_off : x_off + xd]), col(Zk1[x_off : x_off + xd])
    if drop_col:
        Xc[:, -1] = 0
        Xn[:, -1] = 0
    hp, hm = [h**j for j in range(q + 1)], [(-h) ** j for j in range(q + 1)]
    Y = [hm[j] * Xn - hp[j] * Xc for j in range(q + 1)]  # delta = sum_j c_j G^j Y_j
    Y1 = [None] + [-j * (hm[j - 1] * Xn + hp[j - 1] * Xc) for j in range(1, q + 1)]  # dY_j / dh
    P = _chain(mm, G, np.eye(n, dtype=LD_), q)
    Bp, Bm = sum(c[j] * hp[j] * P[j] for j in range(q + 1)), sum(c[j] * hm[j] * P[j] for j in range(q + 1))
    FY = [_chain(mm, G, Y[j], j) for j in range(q + 1)]  # FY[j][a] = G^a Y_j
    FY1 = [None] + [_chain(mm, G, Y1[j], j) for j in range(1, q + 1)]
    delta = sum(c[j] * FY[j][j] for j in range(q + 1))
    tails = []
    for l in range(m):  # sum_j c_j sum_{a + b = j - 1} G^a G_l G^b Y_j
        R = np.zeros((n, C), dtype=LD_)
        for j in range(1, q + 1):
            for b in range(j):
                R = R + c[j] * _chain(mm, G, mm(Gl[l], FY[j][b]), j - 1 - b)[-1]
        tails.append(R)
    tails.append(sum(c[j] * FY1[j][j] for j in range(1, q + 1)) if q else np.zeros((n, C), dtype=LD_))
    tail = np.stack(tails, axis=0).transpose(2, 0, 1).reshape(-1)  # [c][l | dt][i]
    jac = np.concatenate([np.tile(_flat(-Bp), C), np.tile(_flat(Bm), C), tail])
    if not hessian:
        return _flat(delta), jac, None
    M = col(mu_k)
    if drop_col:
        M[:, -1] = 0
    ip = lambda A, B: np.sum(A * B)
    Gt = G.T
    WM = _chain(mm, Gt, M, q)  # (G^T)^a M
    GW = [[mm(Gl[l].T, WM[a]) for a in range(q)] for l in range(m)]  # G_l^T (G^T)^a M
    Y2 = [None, None] + [j * (j - 1) * (hm[j - 2] * Xn - hp[j - 2] * Xc) for j in range(2, q + 1)]
    hh = sum((c[j] * ip(WM[j], Y2[j]) for j in range(2, q + 1)), LD_(0))
    hu = [sum((c[j] * ip(GW[l][a], FY1[j][j - 1 - a]) for j in range(1, q + 1) for a in range(j)), LD_(0)) for l in range(m)]
    F = np.zeros((m, m), dtype=LD_)  # F[i, l] = sum_j c_j sum_{a + b + e = j - 2} <M, G^a G_i G^b G_l G^e Y_j>
    GWs = [np.stack([GW[i][a] for i in range(m)]) for a in range(q - 1)] if m else []
    for l in range(m):
        for j in range(2, q + 1):
            for e in range(j - 1):
                T = _chain(mm, G, mm(Gl[l], FY[j][e]), j - 2 - e)
                for b, Tb in enumerate(T):
                    F[:, l] += c[j] * np.sum(GWs[j - 2 - e - b] * Tb[None], axis=(1, 2))
    uu = [F[i, l] + F[l, i] for i in range(m) for l in range(i + 1)]
    V = []  # V[l][j] = (d_l G^j)^T M = sum_{a + e = j - 1} (G^T)^e G_l^T (G^T)^a M
    for l in range(m):
        Q = [_chain(mm, Gt, GW[l][a], q - 1 - a) for a in range(q)]
        V.append([None] + [sum(Q[a][j - 1 - a] for a in range(j)) for j in range(1, q + 1)])
    out = [np.array(uu + hu + [hh], dtype=LD_)]
    zero = np.zeros((n, C), dtype=LD_)
    out += [_flat(-sum((c[j] * hp[j] * V[l][j] for j in range(1, q + 1)), zero)) for l in range(m)]
    out.append(_flat(-sum((j * c[j] * hp[j - 1] * WM[j] for j in range(1, q + 1)), zero)))
    out += [_flat(sum((c[j] * hm[j] * V[l][j] for j in range(1, q + 1)), zero)) for l in range(m)]
    out.append(_flat(-sum((j * c[j] * hm[j - 1] * WM[j] for j in range(1, q + 1)), zero)))
    return _flat(delta), jac, np.concatenate(out)


def truth_values(lay, G0, Gj, Z, mu, order, x_off=None, c=None, mm=_mm, intervals=None, hessian=True, drop_drive=False, drop_col=False):
    """(delta, Jacobian values, Hessian values | None), each [intervals, ..] in longdouble, in the library's order for `lay`."""
    o = lay.x_off if x_off is None else x_off
    c = coeffs(order) if c is None else np.asarray(c, dtype=LD_)
    G0l, Gl = np.asarray(G0, dtype=LD_), [np.asarray(g, dtype=LD_) for g in Gj]
    ks = range(lay.K) if intervals is None else intervals
    mu = None if mu is None else np.asarray(mu).reshape(lay.K, lay.x_dim)
    out = [truth_interval(Z[k], Z[k + 1], None if mu is None else mu[k], lay, G0l, Gl, c, o, mm, hessian and mu is not None, drop_drive, drop_col) for k in ks]
    return tuple(None if out[0][i] is None else np.array([r[i] for r in out]) for i in range(3))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def truth_ld(name, order, seed=0, drift=0, members=1, member=0):
    """(delta, Jacobian values, mu, Hessian values) of one member, flat, in longdouble; computed once and never written to."""
    lay, G0, Gj, Z, _ = case(name, seed, drift, members)
    mu = rand_mu(lay.K * lay.x_dim, name, member)
    d, j, h = truth_values(lay, G0, Gj, Z, mu, order, x_off=member * lay.x_dim)
    return _ro(d.reshape(-1), j.reshape(-1), mu, h.reshape(-1))


@functools.lru_cache(maxsize=None)
def truth(name, order, seed=0, drift=0, members=1, member=0):
    """The same rounded to float64: what the GPU tests compare with."""
    d, j, mu, h = truth_ld(name, order, seed, drift, members, member)
    return _ro(d.astype(np.float64), j.astype(np.float64), mu, h.astype(np.float64))


@functools.lru_cache(maxsize=None)
def rollout_truth(name):
    lay, G0, Gj, Z, _ = case(name)
    return _ro(po.exact_rollout(Z, lay, G0, Gj))[0]
