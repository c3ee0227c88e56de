"""The Hessian of the Lagrangian in the exponential mode (option ``exp_hess`` on a PCL_ORDER_EXP context) on the device, through the C ABI
and the Python mirror: every value against tests/exp_hess_truth.py (block ``expm`` for the second Frechet derivative, ``expm_frechet`` for
the first -- no code path shared with the kernel's recurrence) with ``close(..., 1e-11)``, the mode's existing tolerance, relative to
max(1, |truth|_inf); a numpy run of the kernel's recurrence sits at 1e-16 .. 1.4e-14 of that truth on these systems.

Segment 0 entry by entry is also the symmetry check: a kernel row computes (i, j) with i and j in different roles (i the direction of the
chain, j the generator the result is contracted with), the truth's L2 is symmetric in them."""
import ctypes

import numpy as np
import pytest

import exp_hess_truth as eht
import piccolo_jl_amd as pa
from helpers import ref_case
from oracle import pade_oracle as po
from shape_cases import plain_case
from test_exp_integrator_gpu import config_case, exp_ctx
from test_parity_gpu import close

pytestmark = pytest.mark.gpu
TOL = 1e-11
E_INVAL, E_SHAPE, E_NOTIMPL = pa._lib.PCL_EINVAL, pa._lib.PCL_ESHAPE, pa._lib.PCL_ENOTIMPL


def hess_ctx(lay, G0, Gj, **kw):
    return exp_ctx(lay, G0, Gj, exp_hessian=True, **kw)


def truth(members, mu, lay, traj_mode=False, index_base=0):
    """members: [(Z [N, z_dim], G0, Gj, x_off)] in row order, mu: the launch's multipliers.  (values, rows, cols) of the launch."""
    mu = np.asarray(mu).reshape(len(members), lay.K, lay.x_dim)
    vs, rs, cs = [], [], []
    for b, (Z, G0, Gj, xo) in enumerate(members):
        vs.append(eht.values(Z, mu[b], lay, G0, Gj, x_off=xo).reshape(-1))
        r, c = eht.structure(lay, x_off=xo, index_base=index_base, col0=b * lay.z_dim * lay.N if traj_mode else 0)
        rs.append(r)
        cs.append(c)
    return np.concatenate(vs), np.concatenate(rs), np.concatenate(cs)


def check(c, Zfull, mu, members, lay, traj_mode=False, index_base=0, tol=TOL):
    """One context against the truth: the structure entry for entry (int64 and int32), the device-pointer launch value for value, a second
    launch and the host-pointer call bitwise.  Returns the values."""
    import torch

    v0, r0, c0 = truth(members, mu, lay, traj_mode, index_base)
    assert c.get_option("exp_hess") == 1
    assert c.hess_per == eht.nnz_per_interval(lay) and c.hess_nnz == v0.size
    rows, cols = c.hess_structure()
    assert np.array_equal(rows, r0) and np.array_equal(cols, c0)
    r32, c32 = c.hess_structure(np.int32)
    assert np.array_equal(r32, r0) and np.array_equal(c32, c0)
    assert np.all(rows >= cols)
    Zh = np.ascontiguousarray(Zfull, dtype=np.float64).reshape(-1)
    muh = np.ascontiguousarray(mu, dtype=np.float64).reshape(-1)
    Zd, mud = torch.from_numpy(Zh).cuda(), torch.from_numpy(muh).cuda()
    vd = torch.full((c.hess_nnz,), float("nan"), dtype=torch.float64, device="cuda")
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.hess_dev(Zd, mud, vd)
    c.sync()
    assert c.get_option("last_hess_kernel") == 100
    vals = vd.cpu().numpy()
    assert np.all(np.isfinite(vals))
    per, nsc = eht.nnz_per_interval(lay), (lay.m + 1) * (lay.m + 2) // 2
    a, t = vals.reshape(-1, per), v0.reshape(-1, per)
    scale = max(1.0, np.abs(v0).max())
    print("max|values - truth| / max(1, |truth|): scalars %.3e  state slices %.3e   (|truth|_inf %.3e)"
          % (np.abs(a[:, :nsc] - t[:, :nsc]).max() / scale, np.abs(a[:, nsc:] - t[:, nsc:]).max() / scale, np.abs(v0).max()))  # fmt: skip
    close(vals, v0, tol)
    v2 = torch.full_like(vd, float("nan"))
    c.hess_dev(Zd, mud, v2)  # a second launch: the same bits
    c.sync()
    assert np.array_equal(v2.cpu().numpy(), vals)
    c.set_stream(None)
    assert np.array_equal(c.hess(Zh, muh), vals)  # host pointers
    return vals


def rand_mu(c, seed):
    return np.random.default_rng(seed).standard_normal(c.n_rows)


# ---- 1. parity on the shapes and modes served -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg, N", [(1, 50), (2, 40), (3, 12)])
def test_configs_against_truth(cfg, N):
    """BASELINE configs 1, 2 and 3 (config 3: 11 intervals x 6 workgroups, G(u_k) in its sixth LDS tile; its truth costs ~1 s per interval)."""
    lay, G0, Gj, Z = config_case(cfg, N, seed=11 + cfg)
    c = hess_ctx(lay, G0, Gj)
    check(c, Z, rand_mu(c, cfg), [(Z, G0, Gj, lay.x_off)], lay)
    c.close()


def test_ket():
    rng = np.random.default_rng(105)
    d, m, N = 5, 2, 6
    n = 2 * d
    Hd = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    Hs = [(lambda A: A + A.conj().T)((rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))) * (rng.random((d, d)) < 0.4)) for _ in range(m)]
    so = po.quantum_system(0.3 * (Hd + Hd.conj().T), Hs, [1.0] * m)
    lay = po.Layout(d=d, m=m, N=N, z_dim=n + 2 + 3 * m, x_off=0, u_off=n + 2, dt_off=n, cols=1)
    Z = 0.5 * rng.standard_normal((N, lay.z_dim))
    Z[:, lay.dt_off] = 0.05 + 0.05 * rng.random(N)
    G0, Gj = so.G_drift, np.array(so.G_drives)
    c = hess_ctx(lay, G0, Gj)
    check(c, Z, rand_mu(c, 1), [(Z, G0, Gj, 0)], lay)
    c.close()


def test_compact_density_vector_odd_n():
    """PCL_STATE_VECTOR: a general real generator of odd dimension (levels = 3: n = 9) on one column."""
    rng = np.random.default_rng(34)
    lv, m, N = 3, 2, 7
    H = rng.standard_normal((lv, lv)) + 1j * rng.standard_normal((lv, lv))
    H = 0.5 * (H + H.conj().T)
    Hs = [(lambda A: A + A.conj().T)(rng.standard_normal((lv, lv)) + 1j * rng.standard_normal((lv, lv))) for _ in range(m)]
    a = po.annihilate(lv)
    G0, Gj = po.compact_lindbladian_generators(H, Hs, [0.3 * a, 0.1 * np.diag(np.arange(lv)).astype(complex)])
    Gj = np.array(Gj)
    n = lv * lv
    lay = po.Layout(d=0, m=m, N=N, z_dim=n + 2 + m, x_off=0, u_off=n + 2, dt_off=n, cols=1, gen=n)
    Z = 0.5 * rng.standard_normal((N, lay.z_dim))
    Z[:, lay.dt_off] = 0.05 + 0.05 * rng.random(N)
    c = hess_ctx(lay, G0, Gj)
    check(c, Z, rand_mu(c, 2), [(Z, G0, Gj, 0)], lay)
    c.close()


def test_no_drives():
    """m = 0: the T recurrence alone, (dt, dt) and (dt, X_k)."""
    so = po.config_system(2)
    G0 = so.G_drift
    d, N = 4, 9
    xd = 2 * d * d
    lay = po.Layout(d=d, m=0, N=N, z_dim=xd + 3, x_off=1, u_off=xd + 2, dt_off=xd + 1)
    rng = np.random.default_rng(8)
    Z = rng.standard_normal((N, lay.z_dim))
    Z[:, lay.dt_off] = 0.05 + 0.1 * rng.random(N)
    Gj = np.zeros((0, 2 * d, 2 * d))
    c = hess_ctx(lay, G0, Gj)
    assert c.hess_per == 1 + xd
    check(c, Z, rand_mu(c, 3), [(Z, G0, Gj, 1)], lay)
    c.close()


def test_ensemble_with_per_member_drifts_and_member_window(golden, golden_meta):
    """ref_sampling_robust: three members with their own drifts in one trajectory buffer; then a window of the last two, whose values are
    the slices of the full launch, bitwise."""
    systems, lay, x_offs = ref_case("sampling_robust", golden_meta)
    Z = golden("ref_sampling_robust")["Z"]
    M = len(systems)
    G0s, Gj = np.array([s.G_drift for s in systems]), np.array(systems[0].G_drives)
    c = hess_ctx(lay, G0s, Gj, x_offs=x_offs, batch=M, per_member_G0=True)
    members = [(Z, s.G_drift, Gj, xo) for s, xo in zip(systems, x_offs)]
    mu = rand_mu(c, 4)
    vals = check(c, Z, mu, members, lay)
    per_d, per_v = lay.x_dim * lay.K, eht.nnz_per_interval(lay) * lay.K
    c.set_member_window(1, M - 1)
    assert c.hess_nnz == (M - 1) * per_v and c.n_rows == (M - 1) * per_d
    assert np.array_equal(c.hess(Z, mu[per_d:]), vals[per_v:])
    r, cc = c.hess_structure()
    r0 = np.concatenate([eht.structure(lay, x_off=x_offs[1 + b])[0] for b in range(M - 1)])
    c0 = np.concatenate([eht.structure(lay, x_off=x_offs[1 + b])[1] for b in range(M - 1)])
    assert np.array_equal(r, r0) and np.array_equal(cc, c0)
    c.set_member_window(0, M)
    assert np.array_equal(c.hess(Z, mu), vals)
    c.close()


def test_shared_drift_members():
    """PCL_BATCH_MEMBERS with one G0 for two members at different state offsets."""
    so = po.config_system(1)
    G0, Gj = so.G_drift, np.array(so.G_drives)
    d, m, N = 2, 2, 8
    xd = 2 * d * d
    lay = po.Layout(d=d, m=m, N=N, z_dim=2 * xd + 2 + m, x_off=0, u_off=2 * xd + 2, dt_off=2 * xd)
    rng = np.random.default_rng(21)
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    Z[:, lay.dt_off] = 0.1 + 0.1 * rng.random(N)
    c = hess_ctx(lay, G0, Gj, x_offs=[0, xd], batch=2)
    check(c, Z, rand_mu(c, 5), [(Z, G0, Gj, 0), (Z, G0, Gj, xd)], lay)
    c.close()


def test_batch_traj_three_seeds_and_window():
    lay, G0, Gj, _ = config_case(2, 12, seed=0)
    Zs = np.stack([config_case(2, 12, seed=40 + b)[3] for b in range(3)])
    c = hess_ctx(lay, G0, Gj, batch=3, batch_mode=pa._lib.PCL_BATCH_TRAJ)
    mu = rand_mu(c, 6)
    vals = check(c, Zs, mu, [(Zs[b], G0, Gj, lay.x_off) for b in range(3)], lay, traj_mode=True)
    per_d, per_v = lay.x_dim * lay.K, eht.nnz_per_interval(lay) * lay.K
    c.set_member_window(2, 1)
    assert np.array_equal(c.hess(Zs, mu[2 * per_d :]), vals[2 * per_v :])
    r, cc = c.hess_structure()
    r0, c0 = eht.structure(lay, col0=2 * lay.z_dim * lay.N)
    assert np.array_equal(r, r0) and np.array_equal(cc, c0)
    c.close()


def test_index_base_one():
    lay, G0, Gj, Z = config_case(1, 6, seed=2)
    c = hess_ctx(lay, G0, Gj, index_base=1)
    check(c, Z, rand_mu(c, 7), [(Z, G0, Gj, lay.x_off)], lay, index_base=1)
    c.close()


# ---- 2. steps ------------------------------------------------------------------------------------------------------------------------
def test_zero_and_negative_steps():
    """dt = 0 at one knot: L = L2 = 0, so the (u, u) block and the (u_l, X_k) slices of that interval are exactly zero and nothing is NaN; a
    negative dt at another."""
    lay, G0, Gj, Z = config_case(2, 8, seed=5)
    Z[3, lay.dt_off] = 0.0
    Z[5, lay.dt_off] = -0.13
    c = hess_ctx(lay, G0, Gj)
    vals = check(c, Z, rand_mu(c, 8), [(Z, G0, Gj, lay.x_off)], lay)
    per, m = eht.nnz_per_interval(lay), lay.m
    v3 = vals[3 * per : 4 * per]
    nsc = (m + 1) * (m + 2) // 2
    assert not v3[: m * (m + 1) // 2].any()  # segment 0
    assert not v3[nsc : nsc + m * lay.x_dim].any()  # segment 3
    assert v3[m * (m + 1) // 2 : nsc].all()
    c.close()


@pytest.mark.parametrize("cfg, N, dt", [(2, 6, 4.0), (3, 4, 1.0)])
def test_large_steps_several_squarings(cfg, N, dt):
    """config 2 at dt = 4.0 and config 3 at dt = 1.0: several squarings of the quadruple."""
    lay, G0, Gj, Z = config_case(cfg, N, seed=17, dt=dt)
    G = G0 + np.tensordot(lay.u(Z, 0), Gj, axes=1)
    assert dt * np.abs(G).sum(axis=0).max() > 2.0  # at least four squarings
    c = hess_ctx(lay, G0, Gj)
    check(c, Z, rand_mu(c, 9), [(Z, G0, Gj, lay.x_off)], lay)
    c.close()


# ---- 3. consistency inside the library --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg, N, dt", [(2, 10, None), (2, 5, 4.0)])
def test_directional_derivative_of_the_device_jacobian(cfg, N, dt):
    """H v against the central difference (step 1e-6) of the device's own J' mu, formed on the device from two pcl_jac_dev results.  Bound:
    1e-6 max(1, |fd|_inf), the figure tests/test_plumbing_gpu.py holds a step-1e-6 central difference of device gradients to (truncation
    ~ step^2 |third derivative|, rounding ~ 1e-16 |J' mu| / step: both orders below it)."""
    import torch

    lay, G0, Gj, Z = config_case(cfg, N, seed=29, dt=dt)
    c = hess_ctx(lay, G0, Gj)
    nv = lay.z_dim * lay.N
    rng = np.random.default_rng(12)
    mu = torch.from_numpy(rng.standard_normal(c.n_rows)).cuda()
    v = rng.standard_normal(nv)
    v = torch.from_numpy(v / np.linalg.norm(v)).cuda()
    Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
    jr, jc = (torch.from_numpy(a).cuda() for a in c.jac_structure())
    hr, hc = (torch.from_numpy(a).cuda() for a in c.hess_structure())
    c.set_stream(torch.cuda.current_stream().cuda_stream)

    def jt_mu(Zx):
        vals = torch.empty(c.jac_nnz, dtype=torch.float64, device="cuda")
        c.jac_dev(Zx, vals)
        return torch.zeros(nv, dtype=torch.float64, device="cuda").index_add_(0, jc, vals * mu[jr])

    step = 1e-6
    fd = (jt_mu(Zd + step * v) - jt_mu(Zd - step * v)) / (2 * step)
    hv = torch.empty(c.hess_nnz, dtype=torch.float64, device="cuda")
    c.hess_dev(Zd, mu, hv)
    Hv = torch.zeros(nv, dtype=torch.float64, device="cuda").index_add_(0, hr, hv * v[hc])
    off = hr != hc
    Hv.index_add_(0, hc[off], hv[off] * v[hr[off]])
    c.sync()
    c.set_stream(None)
    err, scale = (Hv - fd).abs().max().item(), max(1.0, fd.abs().max().item())
    print("|H v - fd|_inf %.3e   |fd|_inf %.3e" % (err, fd.abs().max().item()))
    assert err <= 1e-6 * scale, (err, scale)
    c.close()


# ---- 4. the option ----------------------------------------------------------------------------------------------------------------------
def _hess_calls(c, Z):
    import torch

    L, h = c._L, c._h
    Zd = torch.from_numpy(Z.reshape(-1)).cuda()
    n = max(c.n_rows, eht_cap(c))
    buf, out = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    hb, hout = np.zeros(n), np.zeros(n)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    idx = np.zeros(n, dtype=np.int64)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    keep = (Zd, buf, out, hb, hout, idx)
    return keep, [
        ("pcl_hess", lambda: L.pcl_hess(h, Z.ctypes.data, hb.ctypes.data, hout.ctypes.data)),
        ("pcl_hess_dev", lambda: L.pcl_hess_dev(h, Zd.data_ptr(), buf.data_ptr(), out.data_ptr())),
        ("pcl_hess_nnz", lambda: L.pcl_hess_nnz(h, ctypes.byref(a), ctypes.byref(b))),
        ("pcl_hess_structure", lambda: L.pcl_hess_structure(h, idx.ctypes.data_as(i32p), idx.ctypes.data_as(i32p))),
        ("pcl_hess_structure_i64", lambda: L.pcl_hess_structure_i64(h, idx.ctypes.data_as(i64p), idx.ctypes.data_as(i64p))),
    ]


def eht_cap(c):
    return ((c.m + 1) * (c.m + 2) // 2 + c.x_dim * (c.m + 1)) * c.K * c.batch


def test_option_switches_the_five_entry_points_on_and_off():
    """Default 0: every refusal as before, in the same words.  1: served.  Back to 0: refused again, and the context still evaluates."""
    lay, G0, Gj, Z = config_case(2, 6, seed=3)
    c = exp_ctx(lay, G0, Gj)
    want = c.eval(Z)
    assert c.get_option("exp_hess") == 0 and c.hess_nnz == 0
    keep, calls = _hess_calls(c, Z)

    def refused():
        for name, call in calls:
            rc = call()
            msg = c._L.pcl_last_error(c._h).decode()
            assert rc == E_NOTIMPL, (name, rc, msg)
            assert "exponential" in msg and "PCL_ORDER_EXP" in msg and "is not implemented" in msg, (name, msg)
            assert np.array_equal(c.eval(Z), want), name

    refused()
    c.set_option("exp_hess", 1)
    assert c.get_option("exp_hess") == 1
    for name, call in calls:
        assert call() == 0, (name, c._L.pcl_last_error(c._h).decode())
    c.sync()
    with pytest.raises(pa.PclError) as ei:
        c.set_option("exp_hess", 2)
    assert ei.value.code == E_INVAL and c.get_option("exp_hess") == 1
    c.set_option("exp_hess", 0)
    assert c.get_option("exp_hess") == 0
    refused()
    # the mode's other refusals do not depend on the option
    c.set_option("exp_hess", 1)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    assert c._L.pcl_jac_compact_nnz(c._h, ctypes.byref(a), ctypes.byref(b)) == E_NOTIMPL
    assert c._L.pcl_merit_grad_len(c._h, ctypes.byref(a), ctypes.byref(b)) == E_NOTIMPL
    assert np.array_equal(c.eval(Z), want)
    c.close()


def test_option_needs_an_exponential_context():
    lay, G0, Gj, Z = config_case(2, 6, seed=3)
    c = exp_ctx(lay, G0, Gj, pade_order=4)
    assert c.get_option("exp_hess") == 0
    h0 = c.hess(Z, np.ones(c.n_rows))
    with pytest.raises(pa.PclError) as ei:
        c.set_option("exp_hess", 1)
    assert ei.value.code == E_INVAL and "PCL_ORDER_EXP" in str(ei.value)
    c.set_option("exp_hess", 0)  # allowed everywhere
    assert c.get_option("exp_hess") == 0
    assert np.array_equal(c.hess(Z, np.ones(c.n_rows)), h0)
    c.close()
    with pytest.raises(ValueError):
        exp_ctx(lay, G0, Gj, pade_order=4, exp_hessian=True)
    with pytest.raises(pa.PclError) as ei:  # a variational context of the mode does not exist
        exp_ctx(lay, G0, Gj, batch_mode=pa._lib.PCL_BATCH_VARIATIONAL, exp_hessian=True)
    assert ei.value.code == E_NOTIMPL


def test_other_results_are_bitwise_unchanged_by_the_option():
    """Residual, Jacobian, objective, its Hessian, the rollout and the derivative rows of an exponential context before the option, with it
    and after a Hessian launch; the same of an order-4 context (its own Hessian included) around a refused and an accepted set_option."""
    lay, G0, Gj, Z = config_case(2, 16, seed=31)
    goal = po.operator_to_iso_vec(np.linalg.qr(np.random.default_rng(1).standard_normal((4, 4)) + 1j * np.random.default_rng(2).standard_normal((4, 4)))[0])

    def everything(c, with_hess):
        d, v = c.eval_jac(Z)
        val, grad = c.objective(Z, 100.0)
        out = [d, v, c.eval(Z), val, grad, c.objective_hess(Z, 100.0, 0.7), c.rollout(Z)]
        out += list(c.deriv_eval_jac(lay.u_off, lay.u_off + lay.m, lay.m, Z))
        if with_hess:
            out.append(c.hess(Z, np.linspace(-1, 1, c.n_rows)))
        return out

    for order in ("exp", 4):
        c = exp_ctx(lay, G0, Gj, pade_order=order)
        c.set_goal(goal)
        c.add_regularizer(lay.u_off, lay.m, 1e-2, 2)
        before = everything(c, order == 4)
        if order == 4:
            with pytest.raises(pa.PclError):
                c.set_option("exp_hess", 1)
            c.set_option("exp_hess", 0)
        else:
            c.set_option("exp_hess", 1)
            a, b = ctypes.c_int64(), ctypes.c_int64()
            c._chk(c._L.pcl_hess_nnz(c._h, ctypes.byref(a), ctypes.byref(b)))
            c.hess_nnz, c.hess_per = a.value, b.value
            assert np.all(np.isfinite(c.hess(Z, np.linspace(-1, 1, c.n_rows))))
        after = everything(c, order == 4)
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        c.close()


# ---- 5. the LDS boundary ----------------------------------------------------------------------------------------------------------------
def test_largest_served_shape_n62():
    """d = 31 (n = 62, LD = 66): five tiles of 32 736 B and the reduction words, 163 808 of 163 840 B; G(u_k) is read from the workspace."""
    lay, G0, Gj, Z = plain_case("S4", N=3)
    assert lay.d == 31 and lay.m == 4
    c = hess_ctx(lay, G0, Gj)
    check(c, Z, rand_mu(c, 10), [(Z, G0, Gj, 0)], lay)
    c.close()


def test_smallest_refused_shape_n64():
    """d = 32 (n = 64): five tiles are 168 960 B.  The option is refused with the byte counts, the mirror's keyword raises, and the context
    goes on serving residual and Jacobian."""
    lay, G0, Gj, Z = plain_case("S5", N=3)
    assert lay.d == 32
    c = exp_ctx(lay, G0, Gj)
    want = c.eval(Z)
    with pytest.raises(pa.PclError) as ei:
        c.set_option("exp_hess", 1)
    assert ei.value.code == E_SHAPE and "LDS" in str(ei.value) and "169088" in str(ei.value) and "163840" in str(ei.value), str(ei.value)
    assert c.get_option("exp_hess") == 0
    with pytest.raises(pa.PclError) as ei:
        c.hess_structure()
    assert ei.value.code == E_NOTIMPL
    assert np.array_equal(c.eval(Z), want)
    c.close()
    with pytest.raises(pa.PclError) as ei:
        hess_ctx(lay, G0, Gj)
    assert ei.value.code == E_SHAPE


# ---- the reference-style objects ---------------------------------------------------------------------------------------------------------
def test_bilinear_integrator_with_exp_hessian():
    from helpers import traj_from_Z
    from test_parity_gpu import product_system

    lay, G0, Gj, Z = config_case(2, 10, seed=13)
    traj = traj_from_Z(pa, Z, lay)
    with pytest.raises(ValueError):
        pa.BilinearIntegrator(product_system(2), traj, pade_order=4, exp_hessian=True)
    B = pa.BilinearIntegrator(product_system(2), traj, pade_order="exp", exp_hessian=True)
    assert B.pade_order == -1 and B.ctx.get_option("exp_hess") == 1
    mu = np.random.default_rng(3).standard_normal(B.dim)
    v0, r0, c0 = truth([(Z, G0, Gj, lay.x_off)], mu, lay)
    r, c = pa.hessian_structure(B)
    assert np.array_equal(r, r0) and np.array_equal(c, c0)
    H = pa.eval_hessian_of_lagrangian(B, traj, mu).toarray()
    close(H, eht.dense(v0, lay), TOL)
    assert np.array_equal(H, H.T)
    B.close()
