"""Cases that walk the exponential-constraint kernels (pcl_exp_kernel, pcl_exp_hess_kernel, pcl_expm_kernel + pcl_chain_kernel, pcl_var_exp*,
both variational Hessian plans) over the generator and column sizes at which their code branches; importable without a GPU.

Generators are random and dense, so that edge rows, edge columns and the last k steps of every product carry weight:
    iso    G(H) of a dense complex Hermitian H (unitary or multi-ket state, n = 2 d)
    vec    a general real n x n matrix / sqrt(n) under PCL_STATE_VECTOR (not normal, odd n allowed, one column)
    variational cases: the iso system and dense Hermitian variations scaled by 1 / 10.
Knot: [X (| Xv_1 ..) | dt | t | u], u ~ 0.4 N(0, 1), N = 4.  The three steps are fixed per case from G(u_k):
    interval 0   h |G|_1 = 0.2                         a nonzero step with no squaring (theta <= 1/4)
    interval 1   h = -0.5 / |G|_2                      a negative step
    interval 2   h = max(2 / |G|_2, 4.5 / |G|_1)       five or more squarings (theta > 4); |G|_1 >= 2.25 |G|_2 on all but the smallest
                                                       generators, where the second bound lifts h |G|_2 to 2.3 (P13) and 2.4 (P15)

Plain cases (kind, n, cols, m) and the branch each straddles; LD = ((n + 3) & ~3) + 2, a tile is LD n doubles, the device has 163 840 B:
    P1   vec 17  1  2   odd, four output tiles, scalar store path at 256 threads
    P2   iso 32 16  3   last 256-thread size, four full tiles
    P3   vec 33  1  1   first odd 512-thread size, one-row edge tile
    P4   iso 34 17  2   nine tiles (the last wave's pair has no partner), odd column count
    P5   iso 48 24  2   exactly three tiles a side, no edge
    P6   vec 49  1  3   odd, n mod 16 = 1 at sixteen tiles
    P7   iso 56 28  2   Hessian: five tiles and 16 words 130 048 B, with G(u_k) in a sixth 156 032 B: fits
    P8   iso 58 29  2   Hessian: five tiles 143 968 B, a sixth would make 172 736 B: G(u_k) is read from the workspace
    P9   iso 58 29  1   Jacobian: four tiles, X_k and 96 words 130 224 B, with G_l in a fifth tile 158 992 B: fits
    P10  iso 60 30  1   Jacobian: 134 688 B, a fifth tile would make 164 448 B: G_l is read through L2
    P11  vec 61  1  2   largest odd n the Hessian serves (five tiles 161 168 B)
    P12  vec 63  1  2   largest odd n; five tiles are 166 448 B: the Hessian is refused with PCL_ESHAPE, eval_jac goes on
    P13  iso 12  3  5   multi-ket, m > cols: two workgroups store no -E block
    P14  iso 20  7  2   multi-ket, uneven deal (4 / 3 copies)
    P15  iso 10  1 24   the ABI's most drives
Batched: P4's system as two PCL_BATCH_MEMBERS members with their own drifts (B1), P1's system as two PCL_BATCH_TRAJ seeds (B2).
Variational cases (d, n, state, m, v): V1 9 18 unitary 2 1 | V2 16 32 ket 3 2 | V3 20 40 unitary 1 1 (the largest nine-tile Hessian in this set) |
V4 24 48 unitary 1 1 | V5 28 56 unitary 1 1 (six tiles 155 904 B: G(u_k) in LDS) | V6 29 58 ket 2 1 (five tiles 143 840 B, six 172 608 B:
G(u_k) from the workspace) | V7 30 60 ket 1 2.  No shape had to move: the byte counts above follow the launch code's own arithmetic.

The emulation (`emu_*`) restates the kernels' recurrences in plain float64 numpy -- Taylor degree 14 by Horner, theta = |h| |G|_1 <= 1/4 after s
halvings, then s squarings of the pair / quadruple -- and shares no code with the truth helpers (scipy expm / expm_frechet / block expm).  The
variational kernels never form the lifted matrix; the emulation does (var_G, with the squaring count taken from the n x n G as the kernels take
it): block for block the lifted recurrence is theirs.  Every product goes through `mm`, which is where tests/test_exp_shapes_cpu.py injects faults.

Reference floor, the largest deviation of the emulation from the committed truths per segment, relative to the segment's own maximum
(tests/test_exp_shapes_cpu.py asserts 1e-13 and prints them), largest value read per mode:
    plain        residual 1.8e-14 (P12)   Jacobian 2.1e-14 (P8, -E of the long step)   Hessian 3.4e-14 (P3, uu)   rollout 1.4e-14 (P6)
    variational  residual 7.3e-15 (V5)    Jacobian 1.3e-14 (V5)                         Hessian 6.5e-14 (V4, hh)   rollout 2.9e-15 (V2)"""
import functools

import numpy as np

from oracle import pade_oracle as po
from shape_cases import per_interval
from variational_truth import VarCase

N = 4
LDS_BYTES = 163840

# name: (kind, n, cols, m)
PLAIN_CASES = {
    "P1": ("vec", 17, 1, 2), "P2": ("iso", 32, 16, 3), "P3": ("vec", 33, 1, 1), "P4": ("iso", 34, 17, 2), "P5": ("iso", 48, 24, 2),
    "P6": ("vec", 49, 1, 3), "P7": ("iso", 56, 28, 2), "P8": ("iso", 58, 29, 2), "P9": ("iso", 58, 29, 1), "P10": ("iso", 60, 30, 1),
    "P11": ("vec", 61, 1, 2), "P12": ("vec", 63, 1, 2), "P13": ("iso", 12, 3, 5), "P14": ("iso", 20, 7, 2), "P15": ("iso", 10, 1, 24),
}  # fmt: skip
HESS_REFUSED = ("P12",)
# name: (d, ket, m, v)
VAR_CASES = {"V1": (9, False, 2, 1), "V2": (16, True, 3, 2), "V3": (20, False, 1, 1), "V4": (24, False, 1, 1), "V5": (28, False, 1, 1),
             "V6": (29, True, 2, 1), "V7": (30, True, 1, 2)}  # fmt: skip
VAR_HESS_LDS = ("V1", "V2", "V3")  # nine LDS tiles fit
VAR_HESS_WS = ("V4", "V6")  # served by var_exp_hess_tiles = 1


# ---- LDS arithmetic of the launch code (pcl_host_launch_pade.hpp launch_exp, pcl_host_launch_hess.hpp exp_hess_lds_bytes, pcl_host_variational.hpp) ---------------------------
def lds_ld(n):
    return ((n + 3) & ~3) + 2


def jac_lds_bytes(n, cols, m):
    """(bytes, G_l has its own tile) of pcl_exp_kernel<true>."""
    tile = lds_ld(n) * n
    dbl = 4 * tile + lds_ld(n) * cols + 96
    gl = m > 0 and (dbl + tile) * 8 <= LDS_BYTES
    return (dbl + (tile if gl else 0)) * 8, gl


def hess_lds_bytes(n):
    """(bytes, G(u_k) has its own tile) of pcl_exp_hess_kernel."""
    tile = lds_ld(n) * n
    five = (5 * tile + 16) * 8
    six = five + tile * 8 <= LDS_BYTES
    return five + (tile * 8 if six else 0), six


def var_lds_bytes(n, tiles=5):
    """(bytes, G(u_k) has its own tile) of pcl_var_exp_kernel (tiles = 5) and of the octuple Hessian kernel (9)."""
    tile = lds_ld(n) * n * 8
    g = (tiles + 1) * tile <= LDS_BYTES
    return (tiles + (1 if g else 0)) * tile, g


# ---- systems and trajectories ----------------------------------------------------------------------------------------------------------------
def _herm(d, rng):
    A = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return (A + A.conj().T) / 2


# P3's first seed left its single (u, u) entry of interval 0 at 1.1e-6 beside (dt, u) = 1.9 -- a near-cancelling scalar, 3e-12 between the
# emulation and the truth -- so that case draws from the next seed.
RESEED = {"P3": 1}


def _seed(name):
    return 9000 + 17 * int(name[1:]) + (500 if name[0] == "V" else 0) + 5 * RESEED.get(name, 0)


def plain_system(name, drift=0):
    """(G0, Gj).  drift > 0: another drift for the same drives (a member of a PCL_BATCH_MEMBERS launch)."""
    kind, n, cols, m = PLAIN_CASES[name]
    rng = np.random.default_rng(_seed(name))
    if kind == "vec":
        G0s = [rng.standard_normal((n, n)) / np.sqrt(n) for _ in range(3)]
        Gj = rng.standard_normal((m, n, n)) / np.sqrt(n)
    else:
        d = n // 2
        G0s = [po.G_of_H(_herm(d, rng)) for _ in range(3)]
        Gj = np.array([po.G_of_H(_herm(d, rng)) for _ in range(m)])
    return G0s[drift], Gj


def plain_layout(name):
    kind, n, cols, m = PLAIN_CASES[name]
    xd = n * cols
    if kind == "vec":
        return po.Layout(d=0, m=m, N=N, z_dim=xd + 2 + m, x_off=0, u_off=xd + 2, dt_off=xd, cols=1, gen=n)
    return po.Layout(d=n // 2, m=m, N=N, z_dim=xd + 2 + m, x_off=0, u_off=xd + 2, dt_off=xd, cols=None if cols == n // 2 else cols)


def _steps(Z, dt_off, u_off, m, G0, Gj):
    for k in range(N - 1):
        G = G0 + np.tensordot(Z[k, u_off : u_off + m], Gj, axes=1)
        n1, n2 = np.abs(G).sum(axis=0).max(), np.linalg.norm(G, 2)
        Z[k, dt_off] = (0.2 / n1, -0.5 / n2, max(2.0 / n2, 4.5 / n1))[k]
    Z[N - 1, dt_off] = 0.1
    Z[:, dt_off + 1] = np.cumsum(Z[:, dt_off])


def squarings(h, G):
    theta, s = abs(h) * np.abs(G).sum(axis=0).max(), 0
    while theta > 0.25 and s < 60:
        theta *= 0.5
        s += 1
    return s


@functools.lru_cache(maxsize=None)
def plain_case(name, seed=0, drift=0):
    """(layout, G0, Gj, Z), read-only.  seed: another trajectory of the same system (a seed of a PCL_BATCH_TRAJ launch).  drift: the member's
    drift on the SAME trajectory -- the members of a PCL_BATCH_MEMBERS launch share the knots, so the steps are those of drift 0."""
    lay = plain_layout(name)
    G0, Gj = plain_system(name, 0)
    rng = np.random.default_rng(_seed(name) + 1 + seed)
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    _steps(Z, lay.dt_off, lay.u_off, lay.m, G0, Gj)
    sq = [squarings(lay.dt(Z, k), G0 + np.tensordot(lay.u(Z, k), Gj, axes=1)) for k in range(lay.K)]
    assert sq[0] == 0 and sq[2] >= 5 and Z[0, lay.dt_off] > 0 > Z[1, lay.dt_off], (name, sq)
    G0 = plain_system(name, drift)[0]
    for a in (G0, Gj, Z):
        a.setflags(write=False)
    return lay, G0, Gj, Z


@functools.lru_cache(maxsize=None)
def var_case(name):
    """VarCase, read-only: knot [X | Xv_1 .. Xv_v | dt | t | u] with random states."""
    d, ket, m, v = VAR_CASES[name]
    n, C = 2 * d, (1 if ket else d)
    rng = np.random.default_rng(_seed(name))
    G0 = po.G_of_H(_herm(d, rng))
    Gj = np.array([po.G_of_H(_herm(d, rng)) for _ in range(m)])
    Gv = [po.G_of_H(_herm(d, rng)) / 10 for _ in range(v)]
    xdc = n * C
    dt_off = (v + 1) * xdc
    z_dim = dt_off + 2 + m
    Z = 0.4 * rng.standard_normal((N, z_dim))
    _steps(Z, dt_off, dt_off + 2, m, G0, Gj)
    sq = [squarings(Z[k, dt_off], G0 + np.tensordot(Z[k, dt_off + 2 :], Gj, axes=1)) for k in range(N - 1)]
    assert sq[0] == 0 and sq[2] >= 5, (name, sq)
    for a in [G0, Gj, Z] + Gv:
        a.setflags(write=False)
    return VarCase(Z=Z, z_dim=z_dim, N=N, n=n, C=C, m=m, xo=[b * xdc for b in range(v + 1)], u_off=dt_off + 2, dt_off=dt_off, G0=G0, Gv=Gv, Gj=Gj)


def rand_mu(size, name):
    mu = np.random.default_rng(_seed(name) + 77).standard_normal(size)
    mu.setflags(write=False)
    return mu


# ---- segment labels (compared with shape_cases.check_segments: no floor at 1) ---------------------------------------------------------------
def jac_labels(n, C, m, K, v=0):
    """One label per Jacobian value: -E (and, per variation, -E.i and -L.i), the ones, one du_l per drive and dh, per component and interval."""
    nb = C * n * n
    per = [np.full(nb, "-E")]
    for i in range(1, v + 1):
        per += [np.full(nb, "-E.%d" % i), np.full(nb, "-L.%d" % i)]
    per.append(np.full((v + 1) * C * n, "ones"))
    for b in range(v + 1):
        sfx = ".%d" % b if v else ""
        per.append(np.tile(np.repeat(np.array(["du%d%s" % (l, sfx) for l in range(m)] + ["dh" + sfx]), n), C))
    return per_interval(np.concatenate(per), K)


def hess_labels(n, C, m, K, v=0):
    """One label per Hessian value: uu, hu, hh, then one u_l.Xk per drive and h.Xk, split per component on a variational layout."""
    per = ["uu"] * (m * (m + 1) // 2) + ["hu"] * m + ["hh"]
    for s in ["u%d.Xk" % l for l in range(m)] + ["h.Xk"]:
        for b in range(v + 1):
            per += [s + (".%d" % b if v else "")] * (C * n)
    return per_interval(np.array(per), K)


def residual_labels(n, C, K, v=0):
    return per_interval(np.concatenate([np.full(C * n, "delta" + (".%d" % b if v else "")) for b in range(v + 1)]), K)


def rollout_labels(xd, n_knots):
    return np.repeat(np.array(["knot%d" % k for k in range(n_knots)]), xd)


# ---- the emulation ---------------------------------------------------------------------------------------------------------------------------
def chain(G, dirs, h, mm=np.matmul, norm1=None, fewer=0):
    """The kernels' scaled recurrence for T_S = the |S|-th Frechet derivative of exp at h G along the directions of S (T_{} = exp(h G)).
    dirs: [(matrix, scaled by h)], at most two.  theta = |h| |G|_1 (or norm1) <= 1/4 after s halvings; Horner, degree 14, with a_h = h 2^-s / j on
    G and the directions scaled by h, a_p = 2^-s / j on the others; then s - fewer squarings.  Returns {(): T, (0,): .., (1,): .., (0, 1): ..}."""
    n = G.shape[0]
    theta, s = abs(h) * (np.abs(G).sum(axis=0).max() if norm1 is None else norm1), 0
    while theta > 0.25 and s < 60:
        theta *= 0.5
        s += 1
    hs, ps = np.ldexp(h, -s), np.ldexp(1.0, -s)
    idx = range(len(dirs))
    subs = [()] + [(x,) for x in idx] + ([(0, 1)] if len(dirs) == 2 else [])
    I = np.eye(n)
    T = {S: (I.copy() if not S else np.zeros((n, n))) for S in subs}
    for j in range(14, 0, -1):
        ah, ap = hs / j, ps / j
        new = {}
        for S in subs:
            acc = ah * mm(G, T[S])
            for x in S:
                D, by_h = dirs[x]
                acc = acc + (ah if by_h else ap) * mm(D, T[tuple(y for y in S if y != x)])
            new[S] = acc + I if not S else acc
        T = new
    for _ in range(max(s - fewer, 0)):
        new = {(): mm(T[()], T[()])}
        for x in idx:
            new[(x,)] = mm(T[()], T[(x,)]) + mm(T[(x,)], T[()])
        if len(dirs) == 2:
            new[(0, 1)] = mm(T[()], T[(0, 1)]) + mm(T[(0, 1)], T[()]) + mm(T[(0,)], T[(1,)]) + mm(T[(1,)], T[(0,)])
        T = new
    return T


def _fewer(k, fewer_on):
    return 1 if k == fewer_on else 0


def emu_eval_jac(Zk, Zk1, G0, Gj, n, C, m, x_off, u_off, dt_off, mm=np.matmul, norm1_of=None, fewer=0):
    """(delta [C n], values) of one interval as pcl_exp_kernel<true> forms them: E and L_l from the pair recurrence, L_l X_k, E X_k, G (E X_k)."""
    h = Zk[dt_off]
    G = G0 + np.tensordot(Zk[u_off : u_off + m], Gj, axes=1) if m else G0
    nrm = None if norm1_of is None else norm1_of(G)
    X, X1 = Zk[x_off : x_off + C * n].reshape(C, n).T, Zk1[x_off : x_off + C * n].reshape(C, n).T
    E, L = None, []
    for l in range(max(m, 1)):
        T = chain(G, [(Gj[l], True)] if m else [], h, mm, nrm, fewer)
        E = T[()]
        if m:
            L.append(T[(0,)])
    Y = mm(E, X)
    tails = [-mm(Ll, X) for Ll in L] + [-mm(G, Y)]  # each n x C
    tail = np.stack(tails, axis=0).transpose(2, 0, 1).reshape(-1)  # [c][l][i]
    vals = np.concatenate([np.tile((-E).T.reshape(-1), C), np.ones(C * n), tail])
    return (X1 - Y).T.reshape(-1), vals


def emu_plain(lay, G0, Gj, Z, x_off=None, mm=np.matmul, fewer_on=None):
    """(delta [K x_dim], values [K nnz]) of one member in the library's order."""
    o = lay.x_off if x_off is None else x_off
    out = [emu_eval_jac(Z[k], Z[k + 1], G0, Gj, lay.n, lay.C, lay.m, o, lay.u_off, lay.dt_off, mm, None, _fewer(k, fewer_on)) for k in range(lay.K)]
    return np.concatenate([d for d, _ in out]), np.concatenate([v for _, v in out])


def emu_hess_interval(Zk, mu_k, G0, Gj, n, C, m, x_off, u_off, dt_off, mm=np.matmul, norm1_of=None, fewer=0):
    """The values of one interval as pcl_exp_hess_kernel forms them: the quadruple on A' = h G' with W = M X_k' (not scaled by h) and h G_l'."""
    h = Zk[dt_off]
    G = G0 + np.tensordot(Zk[u_off : u_off + m], Gj, axes=1) if m else G0
    nrm = None if norm1_of is None else norm1_of(G)
    X, M = Zk[x_off : x_off + C * n].reshape(C, n).T, np.asarray(mu_k).reshape(C, n).T
    W, Gt = mm(M, X.T), G.T
    uu, hu, sl = [], [], []
    T = None
    for l in range(max(m, 1)):
        Q = chain(Gt, [(W, False), (Gj[l].T, True)] if m else [], h, mm, nrm, fewer)
        T = Q[()]
        if m:
            uu += [-h * np.sum(Q[(0, 1)] * Gj[j]) for j in range(l + 1)]
            hu.append(-np.sum(Q[(0,)] * Gj[l]) - np.sum(Q[(0, 1)] * G))
            sl.append((-mm(Q[(1,)], M)).T.reshape(-1))
    U = mm(T, mm(Gt, M))
    hh = -np.sum(mm(Gt, U) * X)
    return np.concatenate([np.array(uu + hu + [hh])] + sl + [(-U).T.reshape(-1)])


def emu_plain_hess(lay, G0, Gj, Z, mu, x_off=None, mm=np.matmul, fewer_on=None):
    o = lay.x_off if x_off is None else x_off
    mu = np.asarray(mu).reshape(lay.K, lay.x_dim)
    return np.concatenate([emu_hess_interval(Z[k], mu[k], G0, Gj, lay.n, lay.C, lay.m, o, lay.u_off, lay.dt_off, mm, None, _fewer(k, fewer_on))
                           for k in range(lay.K)])  # fmt: skip


def emu_rollout(lay, G0, Gj, Z, x_off=None, mm=np.matmul):
    """[N, x_dim]: knot 0 copied, then X <- T X with T of the recurrence (pcl_expm_kernel + pcl_chain_kernel)."""
    o = lay.x_off if x_off is None else x_off
    X = Z[0, o : o + lay.x_dim].reshape(lay.C, lay.n).T
    out = [X.T.reshape(-1)]
    for k in range(lay.K):
        G = G0 + np.tensordot(lay.u(Z, k), Gj, axes=1) if lay.m else G0
        X = mm(chain(G, [], lay.dt(Z, k), mm)[()], X)
        out.append(X.T.reshape(-1))
    return np.array(out)


# -- variational: the same recurrences on the lifted generator, the squaring count from the n x n G
def _lift(case):
    """(lifted G0, lifted drives, knots [lifted state (c, b, i) | dt | u], n') -- built here, not by variational_truth."""
    n, C, v, m = case.n, case.C, case.v, case.m
    nl = (v + 1) * n
    G0l = np.kron(np.eye(v + 1), case.G0)
    for i, g in enumerate(case.Gv, start=1):
        G0l[i * n : (i + 1) * n, :n] += g
    Gjl = np.array([np.kron(np.eye(v + 1), g) for g in case.Gj]).reshape(m, nl, nl)
    Zl = np.zeros((case.N, C * nl + 1 + m))
    for k in range(case.N):
        S = np.stack([case.Z[k, o : o + case.xdc].reshape(C, n) for o in case.xo], axis=1)  # [c][b][i]
        Zl[k, : C * nl] = S.reshape(-1)
        Zl[k, C * nl] = case.Z[k, case.dt_off]
        Zl[k, C * nl + 1 :] = case.Z[k, case.u_off : case.u_off + m]
    return G0l, Gjl, Zl, nl


def _stack(a, case, lead):
    """[..lead.., c, b, i] -> [..lead.., b, c, i], flattened"""
    a = a.reshape(lead + (case.C, case.v + 1, case.n))
    return np.moveaxis(a, -2, -3).reshape(-1)


def emu_var(case, mm=np.matmul, fewer_on=None):
    """(delta [K x_dim'], values [K nnz]) of a PCL_BATCH_VARIATIONAL_EXP context in the library's order."""
    n, C, v, m = case.n, case.C, case.v, case.m
    G0l, Gjl, Zl, nl = _lift(case)
    norm1_of = lambda Gl: np.abs(Gl[:n, :n]).sum(axis=0).max()
    ds, vs = [], []
    for k in range(case.K):
        d, val = emu_eval_jac(Zl[k], Zl[k + 1], G0l, Gjl, nl, C, m, 0, C * nl + 1, C * nl, mm, norm1_of, _fewer(k, fewer_on))
        ds.append(_stack(d, case, ()))
        mE = val[: nl * nl].reshape(nl, nl).T  # -exp(h Ghat): blocks (b, b) = -E, (i, 0) = -L_i, nothing above the diagonal
        assert not np.triu(mE, n)[:n].any()
        blk = lambda a, b: np.tile(mE[a * n : (a + 1) * n, b * n : (b + 1) * n].T.reshape(-1), C)
        out = [blk(0, 0)]
        for i in range(1, v + 1):
            out += [blk(i, i), blk(i, 0)]
        out.append(np.ones(case.xd))
        tail = val[C * nl * nl + C * nl :].reshape(C, m + 1, v + 1, n)  # [c][l][b][i] -> [b][c][l][i]
        out.append(tail.transpose(2, 0, 1, 3).reshape(-1))
        vs.append(np.concatenate(out))
    return np.concatenate(ds), np.concatenate(vs)


def emu_var_hess(case, mu, mm=np.matmul, fewer_on=None):
    n, C, v, m = case.n, case.C, case.v, case.m
    G0l, Gjl, Zl, nl = _lift(case)
    norm1_of = lambda Gl: np.abs(Gl[:n, :n]).sum(axis=0).max()
    nsc = (m + 1) * (m + 2) // 2
    mu = np.asarray(mu).reshape(case.K, v + 1, C, n)
    out = []
    for k in range(case.K):
        mul = mu[k].transpose(1, 0, 2).reshape(-1)  # [c][b][i]
        val = emu_hess_interval(Zl[k], mul, G0l, Gjl, nl, C, m, 0, C * nl + 1, C * nl, mm, norm1_of, _fewer(k, fewer_on))
        out += [val[:nsc], _stack(val[nsc:], case, (m + 1,))]
    return np.concatenate(out)


def emu_var_rollout(case, mm=np.matmul):
    """[N, x_dim'] stacked: knot 0 copied, then the lifted propagator of the recurrence."""
    n = case.n
    G0l, Gjl, Zl, nl = _lift(case)
    X = Zl[0, : case.C * nl].reshape(case.C, nl).T
    out = [_stack(X.T.reshape(-1), case, ())]
    for k in range(case.K):
        G = G0l + np.tensordot(Zl[k, case.C * nl + 1 :], Gjl, axes=1)
        X = mm(chain(G, [], Zl[k, case.C * nl], mm, np.abs(G[:n, :n]).sum(axis=0).max())[()], X)
        out.append(_stack(X.T.reshape(-1), case, ()))
    return np.array(out)


# ---- faults for the sensitivity checks --------------------------------------------------------------------------------------------------------
def mm_drop_last_k_step(n):
    """Every product with the left operand's columns from 4 floor((n - 1) / 4) on (per n x n block) read as zero."""
    k0 = 4 * ((n - 1) // 4)

    def mm(A, B):
        A = np.array(A)
        A[:, np.arange(A.shape[1]) % n >= k0] = 0.0
        return A @ B

    return mm


def mm_drop_last_row_tile(n):
    """Every product with the rows of the last 16-row tile of its output (per block of n rows) left at zero."""
    r0 = 16 * ((n - 1) // 16)

    def mm(A, B):
        Cm = A @ B
        Cm[np.arange(Cm.shape[0]) % n >= r0] = 0.0
        return Cm

    return mm


# ---- the committed truths, computed once per case and never written to ---------------------------------------------------------------------
def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def plain_truth(name, seed=0, drift=0):
    """(delta, values) of one member: po.exp_residual and exp_truth.values (scipy expm / expm_frechet)."""
    import exp_truth

    lay, G0, Gj, Z = plain_case(name, seed, drift)
    return _ro(po.exp_residual(Z, lay, G0, Gj).reshape(-1), exp_truth.values(Z, lay, G0, Gj).reshape(-1))


@functools.lru_cache(maxsize=None)
def plain_hess_truth(name, seed=0, drift=0):
    """(mu, values): exp_hess_truth.values (block expm for the second Frechet derivative)."""
    import exp_hess_truth

    lay, G0, Gj, Z = plain_case(name, seed, drift)
    mu = rand_mu(lay.K * lay.x_dim, name)
    return mu, _ro(exp_hess_truth.values(Z, mu, lay, G0, Gj).reshape(-1))


@functools.lru_cache(maxsize=None)
def plain_rollout_truth(name):
    lay, G0, Gj, Z = plain_case(name)
    return _ro(po.exact_rollout(Z, lay, G0, Gj))


@functools.lru_cache(maxsize=None)
def var_truth(name):
    import var_exp_truth

    case = var_case(name)
    return _ro(var_exp_truth.residual(case), var_exp_truth.values(case))


@functools.lru_cache(maxsize=None)
def var_hess_truth(name):
    import var_exp_hess_truth

    case = var_case(name)
    mu = rand_mu(case.K * case.xd, name)
    return mu, _ro(var_exp_hess_truth.values(case, mu).reshape(-1))


@functools.lru_cache(maxsize=None)
def var_rollout_truth(name):
    """[N, x_dim'] stacked: the product of scipy.linalg.expm of the lifted generator (variational_truth.lifted) from knot 0."""
    import variational_truth as vt

    case = var_case(name)
    Zl, lay, G0l, Gjl = vt.lifted(case)
    R = po.exact_rollout(Zl, lay, G0l, Gjl)
    out = np.empty_like(R)
    out[:, vt._row_map(case)] = R
    return _ro(out)
