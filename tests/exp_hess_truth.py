"""Truth of the Hessian of the Lagrangian in the exponential mode (option ``exp_hess`` on a PCL_ORDER_EXP context), in the library's layout.

Per interval, with h = dt_k, G = G(u_k), A = h G, E = exp(A), X = X_k (n x cols), M = the interval's multipliers reshaped like delta_k:

    seg 0  (u_i, u_j), j <= i : -<M, L2(A; h G_i, h G_j) X>
    seg 1  (dt, u_j)          : -<M, (G_j E + G L_j) X>          L_j = L(A; h G_j)
    seg 2  (dt, dt)           : -<M, G^2 E X>
    seg 3  (u_l, X_k[r])      : -L_l' M      column-major over the state columns
    seg 4  (dt, X_k[r])       : -(G E)' M

delta_k is X_{k+1} minus something, so nothing involves X_{k+1}: the Pade layout's last two groups do not exist here.

L2, the second Frechet derivative of exp, is the top-right block of ``scipy.linalg.expm`` of the 4n x 4n matrix
[[A, P, Q, 0], [0, A, 0, Q], [0, 0, A, P], [0, 0, 0, A]]; L is ``scipy.linalg.expm_frechet``.  Nothing here runs the scaled Taylor recurrence
of the kernel.  Importable without a GPU."""
import numpy as np
import scipy.linalg

from oracle import pade_oracle as po


def nnz_per_interval(lay):
    return (lay.m + 1) * (lay.m + 2) // 2 + lay.x_dim * (lay.m + 1)


def frechet2(A, P, Q):
    """L2(A; P, Q): the second Frechet derivative of exp at A along P and Q (symmetric in them)."""
    n = A.shape[0]
    Z = np.zeros((n, n))
    B = np.block([[A, P, Q, Z], [Z, A, Z, Q], [Z, Z, A, P], [Z, Z, Z, A]])
    return scipy.linalg.expm(B)[:n, 3 * n :]


def interval_values(G, Gj, h, X, M):
    """The nnz_per_interval values of one interval: G = G(u_k) (n x n), Gj [m, n, n], X and M n x cols."""
    m = len(Gj)
    A = h * G
    E = scipy.linalg.expm(A)
    L = [scipy.linalg.expm_frechet(A, h * Gj[l], compute_expm=False) for l in range(m)]
    out = []
    for i in range(m):
        for j in range(i + 1):
            out.append([-np.sum(M * (frechet2(A, h * Gj[i], h * Gj[j]) @ X))])
    for j in range(m):
        out.append([-np.sum(M * ((Gj[j] @ E + G @ L[j]) @ X))])
    out.append([-np.sum(M * (G @ G @ E @ X))])
    for l in range(m):
        out.append((-(L[l].T @ M)).T.reshape(-1))
    out.append((-((G @ E).T @ M)).T.reshape(-1))
    return np.concatenate(out)


def values(Z, mu, lay, G0, Gj, x_off=None, intervals=None):
    """[K, nnz_per_interval] (or the listed intervals only): mu is [K, x_dim] like delta."""
    mu = np.asarray(mu, dtype=np.float64).reshape(lay.K, lay.x_dim)
    ks = range(lay.K) if intervals is None else intervals
    out = []
    for k in ks:
        G = G0 + np.tensordot(lay.u(Z, k), Gj, axes=1) if lay.m else G0
        M = mu[k].reshape(lay.C, lay.n).T
        out.append(interval_values(G, Gj, lay.dt(Z, k), lay.X(Z, k, x_off), M))
    return np.array(out)


def structure(lay, x_off=None, index_base=0, col0=0):
    """(rows, cols) of one member's K intervals in value order: po.hess_structure without its X_{k+1} groups.  col0: the seed's variable block."""
    r, c = po.hess_structure(lay, x_off)
    per_pade, per = po.hess_nnz_per_interval(lay), nnz_per_interval(lay)
    r = r.reshape(lay.K, per_pade)[:, :per].reshape(-1)
    c = c.reshape(lay.K, per_pade)[:, :per].reshape(-1)
    return r + col0 + index_base, c + col0 + index_base


def dense(vals, lay, x_off=None):
    """Symmetric (z_dim N) x (z_dim N) matrix assembled from the triplets (small cases)."""
    r, c = structure(lay, x_off)
    nv = lay.z_dim * lay.N
    H = np.zeros((nv, nv))
    np.add.at(H, (r, c), np.asarray(vals).reshape(-1))
    return H + np.tril(H, -1).T
