"""Truth of the exponential mode (pcl_desc.pade_order = PCL_ORDER_EXP) in the library's layout, from the committed oracle.

The oracle (``po.exp_residual``, ``po.exp_jacobian_values``) writes the Jacobian of ``delta_k = X_{k+1} - exp(dt_k G(u_k)) X_k`` in the Pade
triplet order, with d delta / d X_{k+1} = I as ``cols`` dense n x n blocks.  The library emits that identity as its diagonal only:

    seg 0  for c < cols, j < n, i < n : -E[i, j]    row c*n+i, col x_off + c*n+j   (knot k)
    seg 1  for r < x_dim              : +1          row r,     col x_off + r       (knot k+1)
    tail   the Pade layout, unchanged

``values`` maps the oracle's values to this layout (and checks that what it drops is exactly zero), ``structure`` builds the expected
triplets, ``dense`` assembles both into a matrix.  Importable without a GPU."""
import numpy as np

from oracle import pade_oracle as po


def nnz_per_interval(lay):
    return lay.C * lay.n * lay.n + lay.x_dim * (lay.m + 2)


def values(Z, lay, G0, Gj, x_off=None):
    """[K, nnz_per_interval]: the oracle's exponential Jacobian values in the library's order."""
    V = po.exp_jacobian_values(Z, lay, G0, Gj, x_off)
    C, n = lay.C, lay.n
    nb = C * n * n
    blocks = V[:, nb : 2 * nb].reshape(lay.K, C, n, n)  # [interval][copy][col j][row i]
    diag = np.einsum("kcii->kci", blocks)
    off = blocks.copy()
    off[:, :, np.arange(n), np.arange(n)] = 0.0
    assert not off.any() and np.array_equal(diag, np.ones_like(diag))  # the oracle's block IS the identity
    return np.concatenate([V[:, :nb], diag.reshape(lay.K, -1), V[:, 2 * nb :]], axis=1)


def structure(lay, x_off=None, index_base=0, row0=0, col0=0):
    """(rows, cols) of one member's K intervals in value order; row0 / col0: the member's row block / the seed's variable block."""
    o = lay.x_off if x_off is None else x_off
    C, n, m, xd, zd = lay.C, lay.n, lay.m, lay.x_dim, lay.z_dim
    c_, j_, i_ = np.meshgrid(np.arange(C), np.arange(n), np.arange(n), indexing="ij")
    blk_r, blk_c = (c_ * n + i_).reshape(-1), (c_ * n + j_).reshape(-1)
    c_, l_, i_ = np.meshgrid(np.arange(C), np.arange(m + 1), np.arange(n), indexing="ij")
    tail_r = (c_ * n + i_).reshape(-1)
    tail_c = np.where(l_ < m, lay.u_off + l_, lay.dt_off).reshape(-1)
    rows, cols = [], []
    for k in range(lay.K):
        rows += [k * xd + blk_r, k * xd + np.arange(xd), k * xd + tail_r]
        cols += [k * zd + o + blk_c, (k + 1) * zd + o + np.arange(xd), k * zd + tail_c]
    rows, cols = np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)
    return rows + row0 + index_base, cols + col0 + index_base


def dense(Z, lay, G0, Gj, x_off=None):
    """(x_dim K) x (z_dim N) Jacobian assembled from the triplets (small cases)."""
    r, c = structure(lay, x_off)
    v = values(Z, lay, G0, Gj, x_off).reshape(-1)
    J = np.zeros((lay.x_dim * lay.K, lay.z_dim * lay.N))
    np.add.at(J, (r, c), v)
    return J
