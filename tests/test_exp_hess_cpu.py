"""tests/exp_hess_truth.py (block expm / expm_frechet) against the committed oracle, without a device.

The truth of the Hessian of the Lagrangian in the exponential mode is checked against central first differences (step 1e-6) of mu' J, with J
from ``po.exp_jacobian_values`` in the library's layout (tests/exp_truth.py).  Every stored entry has its row or its column among the
interval's drives and time step, so differencing mu' J along those m + 1 variables and reading ALL components of the result covers every
entry -- the (u, u), (dt, u), (dt, dt) scalars directly, the (u_l, X_k) and (dt, X_k) slices through the symmetry of the Hessian -- and
shows that nothing involving X_{k+1} is missing.

Tolerance: the worst deviation relative to max(1, |truth|_inf) measured here over the cases below is 2.133e-10 (config 1 at dt = 3; the
others: 2.8e-11 .. 1.5e-10 -- the rounding of mu' J over the step is what the difference sees); the bound is 10 x that, 2.133e-9."""
import numpy as np
import pytest

import exp_hess_truth as eht
import exp_truth
from oracle import pade_oracle as po

STEP = 1e-6
TOL = 2.133e-9


def jt_mu(Z, mu, lay, G0, Gj):
    r, c = exp_truth.structure(lay)
    v = exp_truth.values(Z, lay, G0, Gj).reshape(-1)
    g = np.zeros(lay.z_dim * lay.N)
    np.add.at(g, c, v * mu.reshape(-1)[r])
    return g


def fd_deviation(cfg, dt, k=1, N=3, seed=3):
    so = po.config_system(cfg)
    Z, lay = po.synthetic_trajectory(so, N, seed=seed)
    if dt is not None:
        Z[:, lay.dt_off] = dt
    G0, Gj = so.G_drift, np.array(so.G_drives)
    mu = np.zeros((lay.K, lay.x_dim))
    mu[k] = np.random.default_rng(cfg).standard_normal(lay.x_dim)  # one interval carries multipliers: the others' terms vanish
    vals = np.zeros((lay.K, eht.nnz_per_interval(lay)))
    vals[k] = eht.values(Z, mu, lay, G0, Gj, intervals=[k])[0]
    H = eht.dense(vals, lay)
    worst, scale = 0.0, max(1.0, np.abs(vals).max())
    cols = [k * lay.z_dim + lay.u_off + l for l in range(lay.m)] + [k * lay.z_dim + lay.dt_off]
    for j in cols:
        Zp, Zm = Z.copy().reshape(-1), Z.copy().reshape(-1)
        Zp[j] += STEP
        Zm[j] -= STEP
        fd = (jt_mu(Zp.reshape(Z.shape), mu, lay, G0, Gj) - jt_mu(Zm.reshape(Z.shape), mu, lay, G0, Gj)) / (2 * STEP)
        worst = max(worst, np.abs(fd - H[:, j]).max())
    # nothing outside those rows and columns
    rest = H.copy()
    rest[cols, :] = 0.0
    rest[:, cols] = 0.0
    assert not rest.any()
    return worst / scale


@pytest.mark.parametrize("cfg, dt", [(1, None), (1, 3.0), (2, None), (2, 4.0), (3, None), (3, 1.0)])
def test_truth_against_first_differences_of_the_oracle_jacobian(cfg, dt):
    """Interval 1 of configs 1, 2 and 3 at their default dt (no squaring of the scaled argument, or one or two) and at dt = 3, 4, 1 (several)."""
    dev = fd_deviation(cfg, dt)
    print("config %d dt %s: worst deviation / max(1, |truth|) = %.3e" % (cfg, dt, dev))
    assert dev <= TOL, dev


def test_second_frechet_derivative_is_symmetric_and_matches_a_difference_of_first_ones():
    rng = np.random.default_rng(0)
    n = 6
    A, P, Q = 0.4 * rng.standard_normal((n, n)), rng.standard_normal((n, n)), rng.standard_normal((n, n))
    import scipy.linalg

    L2 = eht.frechet2(A, P, Q)
    assert np.abs(L2 - eht.frechet2(A, Q, P)).max() < 1e-13
    e = 1e-5
    fd = (scipy.linalg.expm_frechet(A + e * Q, P, compute_expm=False) - scipy.linalg.expm_frechet(A - e * Q, P, compute_expm=False)) / (2 * e)
    assert np.abs(L2 - fd).max() < 1e-8 * max(1.0, np.abs(L2).max())


@pytest.mark.parametrize("index_base", [0, 1])
def test_structure_is_the_pade_structure_without_its_next_knot_groups(index_base):
    so = po.config_system(2)
    Z, lay = po.synthetic_trajectory(so, 5, seed=1)
    m, xd, zd = lay.m, lay.x_dim, lay.z_dim
    per = eht.nnz_per_interval(lay)
    assert per == (m + 1) * (m + 2) // 2 + xd * (m + 1) == po.hess_nnz_per_interval(lay) - xd * (m + 1)
    col0 = 7 * zd
    r, c = eht.structure(lay, index_base=index_base, col0=col0)
    pr, pc = po.hess_structure(lay, index_base=index_base)
    pr, pc = pr.reshape(lay.K, -1), pc.reshape(lay.K, -1)
    assert np.array_equal(r.reshape(lay.K, per), pr[:, :per] + col0) and np.array_equal(c.reshape(lay.K, per), pc[:, :per] + col0)
    # what was dropped is exactly the entries with a row in knot k + 1, and nothing kept has one
    for k in range(lay.K):
        lim = (k + 1) * zd + index_base
        assert np.all(pr[k, per:] >= lim) and np.all(pr[k, :per] < lim)
    # entry for entry, spelled out
    rr, cc = [], []
    for k in range(lay.K):
        uk, hk, xk = k * zd + lay.u_off, k * zd + lay.dt_off, k * zd + lay.x_off
        pairs = [(uk + i, uk + j) for i in range(m) for j in range(i + 1)] + [(hk, uk + j) for j in range(m)] + [(hk, hk)]
        pairs += [(uk + l, xk + q) for l in range(m) for q in range(xd)] + [(hk, xk + q) for q in range(xd)]
        rr += [max(p) for p in pairs]
        cc += [min(p) for p in pairs]
    assert np.array_equal(r, np.array(rr) + col0 + index_base) and np.array_equal(c, np.array(cc) + col0 + index_base)


def test_exp_hessian_keyword_needs_the_exponential_order():
    """Raised before any device call: there is no device here.  (The option itself is tested on the GPU.)"""
    import piccolo_jl_amd as pa
    from helpers import traj_from_Z

    so = po.config_system(1)
    Z, lay = po.synthetic_trajectory(so, 4, seed=0)
    G0, Gj = so.G_drift, np.array(so.G_drives)
    for order in (0, 4, 10):
        with pytest.raises(ValueError, match="exp_hessian"):
            pa.integrators._PclContext(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj,
                                       batch=1, batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=order, exp_hessian=True)  # fmt: skip
        traj = traj_from_Z(pa, Z, lay)
        with pytest.raises(ValueError, match="exp_hessian"):
            pa.HipPadeIntegrator(G0, Gj, traj, pade_order=order, exp_hessian=True)
        sysq = pa.QuantumSystem(0.5 * pa.PAULIS["Z"], [pa.PAULIS["X"], pa.PAULIS["Y"]], [1.0, 1.0])
        with pytest.raises(ValueError, match="exp_hessian"):
            pa.BilinearIntegrator(sysq, traj, pade_order=order, exp_hessian=True)
