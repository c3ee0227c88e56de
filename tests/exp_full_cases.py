"""Cases, truths and numpy restatements for the option exp_full of the exponential constraint (pcl_desc.pade_order = PCL_ORDER_EXP): the compact
Jacobian [-E (n n) | tail], its expansion, and the merit / reduce payload [phi | J'(w lam) on u | on dt] by three routes (from the Jacobian
values, fused into the Jacobian launch, and by one adjoint pair chain per interval without any Jacobian value).  Importable without a GPU.

Cases -- the smallest sizes at which each path can go wrong (N = 4 unless stated):
    a  unitary d = 5         n = 10  cols = 5   m = 2
    b  PCL_STATE_VECTOR      n = 9   cols = 1   m = 2   odd n: scalar stores, the odd merit loop; the host path must stay full
    c  multi-ket             n = 12  cols = 3   m = 5   m > cols: some workgroups own no copy of -E
    d  ket                   n = 12  cols = 1   m = 9   the part kernel's l += 8 wraps
    e  unitary d = 17        n = 34  cols = 17  m = 3   512 threads
    f  unitary d = 27        n = 54  cols = 27  m = 6   the config-3 system, N = 3
    g  unitary d = 32        n = 64  cols = 32  m = 2   N = 3; G_l is not in LDS
    h  unitary d = 3         n = 6   cols = 3   m = 0   no drive
    i  PCL_BATCH_MEMBERS     d = 5, batch 3, per-member G0, unequal weights (a member window on the compact trio)
    j  PCL_BATCH_TRAJ        d = 5, batch 2 (two output sets)
Generators are dense and random as in tests/exp_shape_cases.py (iso: G(H) of a dense Hermitian H; vec: a general real matrix / sqrt(n)), f takes
BASELINE config 3's system.  Knot: [X (per member) | dt | t | u], entries ~ 0.4 N(0, 1).  The steps are fixed from G(u_k) of the first member:
    interval 0   h |G|_1 = 0.2                     no squaring          interval 1   h = max(2 / |G|_2, 4.5 / |G|_1)   five or more squarings
    interval 2   h = -0.5 / |G|_2                  a negative step
Multipliers lam are dense, N(0, 1).

Truth: the payload formed in np.longdouble from exp_truth's Jacobian values (scipy expm / expm_frechet) and po.exp_residual.  Tolerance: the project's
1e-11 (tests/test_exp_integrator_gpu.py), per entry on  sum_b w_b |lam_bk|_2 |column_bk|_2  -- the Cauchy-Schwarz image of "every segment within
1e-11 of its own size" -- and for phi on  sum_bk w_b |lam_bk| |delta_bk|  (half of it when lam = delta, as phi itself is halved)."""
import functools

import numpy as np
import scipy.linalg

import exp_truth
from oracle import pade_oracle as po

TOL = 1e-11
MEMBERS, TRAJ = 0, 1

# name: (kind, n, cols, m, N, batch, batch_mode)
CASES = {
    "a": ("iso", 10, 5, 2, 4, 1, MEMBERS), "b": ("vec", 9, 1, 2, 4, 1, MEMBERS), "c": ("iso", 12, 3, 5, 4, 1, MEMBERS),
    "d": ("iso", 12, 1, 9, 4, 1, MEMBERS), "e": ("iso", 34, 17, 3, 4, 1, MEMBERS), "f": ("cfg3", 54, 27, 6, 3, 1, MEMBERS),
    "g": ("iso", 64, 32, 2, 3, 1, MEMBERS), "h": ("iso", 6, 3, 0, 4, 1, MEMBERS), "i": ("iso", 10, 5, 2, 4, 3, MEMBERS),
    "j": ("iso", 10, 5, 2, 4, 2, TRAJ),
}  # fmt: skip
WEIGHTS = {"i": (0.5, 1.25, 2.0), "j": (0.7, 1.3)}
WINDOW = {"i": (1, 2)}


def _herm(d, rng):
    A = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return (A + A.conj().T) / 2


def _set_steps(Z, lay, G0, Gj):
    for k in range(lay.K):
        G = G0 + np.tensordot(lay.u(Z, k), Gj, axes=1) if lay.m else G0
        n1, n2 = np.abs(G).sum(axis=0).max(), np.linalg.norm(G, 2)
        Z[k, lay.dt_off] = (0.2 / n1, max(2.0 / n2, 4.5 / n1), -0.5 / n2)[k]
    Z[lay.N - 1, lay.dt_off] = 0.1
    Z[:, lay.dt_off + 1] = np.cumsum(Z[:, lay.dt_off])


class Case:
    """lay (x_off of member 0), G0s [batch or 1], Gj, Zfull ([N, z_dim], TRAJ: [batch, N, z_dim]), x_offs, members [(Z, G0, x_off)] in row order."""


@functools.lru_cache(maxsize=None)
def case(name):
    kind, n, cols, m, N, batch, mode = CASES[name]
    rng = np.random.default_rng(4100 + 13 * (ord(name) - ord("a")))
    c = Case()
    c.name, c.n, c.cols, c.m, c.N, c.batch, c.mode = name, n, cols, m, N, batch, mode
    n_g0 = batch if mode == MEMBERS and batch > 1 else 1
    if kind == "vec":
        G0s = [rng.standard_normal((n, n)) / np.sqrt(n) for _ in range(n_g0)]
        Gj = rng.standard_normal((m, n, n)) / np.sqrt(n)
    elif kind == "cfg3":
        so = po.config_system(3)
        G0s, Gj = [np.array(so.G_drift)], np.array(so.G_drives)
        assert Gj.shape == (m, n, n)
    else:
        G0s = [po.G_of_H(_herm(n // 2, rng)) for _ in range(n_g0)]
        Gj = np.array([po.G_of_H(_herm(n // 2, rng)) for _ in range(m)]).reshape(m, n, n)
    xd = n * cols
    n_x = batch if mode == MEMBERS else 1
    z_dim = n_x * xd + 2 + m
    c.x_offs = [b * xd for b in range(n_x)]
    args = dict(m=m, N=N, z_dim=z_dim, x_off=0, u_off=n_x * xd + 2, dt_off=n_x * xd)
    if kind == "vec":
        c.lay = po.Layout(d=0, cols=1, gen=n, **args)
    else:
        c.lay = po.Layout(d=n // 2, cols=None if cols == n // 2 else cols, **args)
    Zs = []
    for _ in range(batch if mode == TRAJ else 1):
        Z = 0.4 * rng.standard_normal((N, z_dim))
        _set_steps(Z, c.lay, G0s[0], Gj)
        Zs.append(Z)
    c.G0s, c.Gj = np.array(G0s), Gj
    c.per_member_G0 = n_g0 > 1
    if mode == TRAJ:
        c.Zfull = np.stack(Zs)
        c.members = [(Zs[b], G0s[0], 0) for b in range(batch)]
    else:
        c.Zfull = Zs[0]
        c.members = [(Zs[0], G0s[b if c.per_member_G0 else 0], c.x_offs[b]) for b in range(batch)]
    c.weights = np.array(WEIGHTS.get(name, (1.0,) * batch))
    c.sets = batch if mode == TRAJ else 1
    c.n_rows = batch * c.lay.K * xd
    c.lam = np.random.default_rng(977 + ord(name)).standard_normal(c.n_rows)
    for a in (c.G0s, c.Gj, c.Zfull, c.weights, c.lam):
        a.setflags(write=False)
    return c


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------
def full_per(n, cols, m):
    return cols * n * n + n * cols * (m + 2)


def compact_per(n, cols, m):
    return n * n + n * cols * (m + 1)


def compact_of_full(vals, n, cols, m):
    """[intervals, full_per] -> [intervals, compact_per]: the first copy of -E and the tail."""
    v = np.asarray(vals).reshape(-1, full_per(n, cols, m))
    return np.concatenate([v[:, : n * n], v[:, cols * n * n + n * cols :]], axis=1)


def expand_compact(comp, n, cols, m):
    """[intervals, compact_per] -> [intervals, full_per]: cols copies of -E, x_dim ones, the tail."""
    c = np.asarray(comp).reshape(-1, compact_per(n, cols, m))
    return np.concatenate([np.tile(c[:, : n * n], (1, cols)), np.ones((c.shape[0], n * cols)), c[:, n * n :]], axis=1)


# ---- truth ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def truth(name):
    """(delta [batch, K, x_dim], values [batch, K, full_per]) of the launch, read-only."""
    c = case(name)
    ds = np.array([po.exp_residual(Z, c.lay, G0, c.Gj, x_off=xo) for Z, G0, xo in c.members])
    vs = np.array([exp_truth.values(Z, c.lay, G0, c.Gj, x_off=xo) for Z, G0, xo in c.members])
    ds.setflags(write=False)
    vs.setflags(write=False)
    return ds, vs


def payload_truth(name, with_lam):
    """(out [sets, 1 + K m + K], scale of the same shape): the payload in np.longdouble from the truth's values, and what the tolerance multiplies."""
    c = case(name)
    ds, vs = truth(name)
    K, n, C, m = c.lay.K, c.n, c.cols, c.m
    lam = (c.lam.reshape(c.batch, K, C * n) if with_lam else ds).astype(np.longdouble)
    tail = vs[:, :, C * n * n + C * n :].reshape(c.batch, K, C, m + 1, n).astype(np.longdouble)
    lm = lam.reshape(c.batch, K, C, n)
    w = c.weights.astype(np.longdouble)
    g_b = w[:, None, None] * np.einsum("bkcli,bkci->bkl", tail, lm)  # [b, K, m + 1]
    s_b = w[:, None, None] * np.sqrt((lm**2).sum(axis=(2, 3)))[:, :, None] * np.sqrt((tail**2).sum(axis=(2, 4)))
    half = np.longdouble(1.0 if with_lam else 0.5)
    phi_b = half * w * np.einsum("bkx,bkx->b", lam, ds.astype(np.longdouble))
    ps_b = half * w * (np.sqrt((lam**2).sum(axis=2)) * np.sqrt((ds.astype(np.longdouble) ** 2).sum(axis=2))).sum(axis=1)

    def pack(phi, g):
        return np.concatenate([[phi], g[:, :m].reshape(-1), g[:, m]])

    if c.mode == TRAJ:
        out = np.array([pack(phi_b[b], g_b[b]) for b in range(c.batch)])
        scale = np.array([pack(ps_b[b], s_b[b]) for b in range(c.batch)])
    else:
        out, scale = pack(phi_b.sum(), g_b.sum(axis=0))[None], pack(ps_b.sum(), s_b.sum(axis=0))[None]
    return out, scale


def worst(out, want, scale):
    """max over the entries of |out - want| / scale (entries whose scale is zero must agree exactly)."""
    err = np.abs(np.asarray(out, dtype=np.longdouble).reshape(want.shape) - want)
    assert not err[scale == 0].any()
    return float((err[scale > 0] / scale[scale > 0]).max())


# ---- the adjoint payload, restated ------------------------------------------------------------------------------------------------------------
def adjoint_payload(name, with_lam, drop_col=False, drop_drive=False, ignore_weight=False, no_h=False, no_g0=False):
    """The payload as the adjoint launch forms it, in float64 numpy / scipy: per (member, interval) W = Lam X_k', V = L(A'; W) with A = h G(u_k)
    (scipy.linalg.expm_frechet), g_u[l] = -h <V, G_l>, g_dt = -(<V, G0> + sum_l u_l <V, G_l>), phi_k = <Lam, delta> (half of it for Lam = delta);
    then the members with their weights.  The keywords inject one fault each (tests/test_exp_full_cpu.py)."""
    c = case(name)
    K, n, C, m, lay = c.lay.K, c.n, c.cols, c.m, c.lay
    ds = truth(name)[0]
    lam = c.lam.reshape(c.batch, K, C * n) if with_lam else ds
    g = np.zeros((c.batch, K, m + 1))
    phi = np.zeros(c.batch)
    for b, (Z, G0, xo) in enumerate(c.members):
        for k in range(K):
            h, u = lay.dt(Z, k), lay.u(Z, k)
            G = G0 + np.tensordot(u, c.Gj, axes=1) if m else G0
            X, Lm = lay.X(Z, k, xo), lam[b, k].reshape(C, n).T
            if drop_col:
                X, Lm = X[:, :-1], Lm[:, :-1]
            V = scipy.linalg.expm_frechet(h * G.T, Lm @ X.T, compute_expm=False)
            dots = [np.sum(V * c.Gj[l]) for l in range(m - 1 if drop_drive and m else m)] + ([0.0] if drop_drive and m else [])
            for l in range(m):
                g[b, k, l] = -(1.0 if no_h else h) * dots[l]
            g[b, k, m] = -((0.0 if no_g0 else np.sum(V * G0)) + sum(u[l] * dots[l] for l in range(m)))
            phi[b] += (1.0 if with_lam else 0.5) * np.dot(lam[b, k], ds[b, k])
    w = np.ones(c.batch) if ignore_weight else c.weights
    g, phi = w[:, None, None] * g, w * phi
    pack = lambda p, gg: np.concatenate([[p], gg[:, :m].reshape(-1), gg[:, m]])
    if c.mode == TRAJ:
        return np.array([pack(phi[b], g[b]) for b in range(c.batch)])
    return pack(phi.sum(), g.sum(axis=0))[None]


def ctx_args(name):
    """Keyword arguments of piccolo_jl_amd.integrators._PclContext for the case (without pade_order / exp_full)."""
    c = case(name)
    lay = c.lay
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=c.x_offs, G0=c.G0s if c.per_member_G0 else c.G0s[0],
                Gj=c.Gj, batch=c.batch, batch_mode=c.mode, per_member_G0=c.per_member_G0)  # fmt: skip
    if lay.gen is not None:
        args.update(d=lay.gen, state_cols=-1)  # PCL_STATE_VECTOR
    elif lay.cols is not None:
        args.update(state_cols=lay.cols)
    return args
