"""The Hessian of the Lagrangian of the exponential constraint at generator dimensions 66 .. 128 on the device (option large_exp_hess on a context
created with PCL_LARGE_N | PCL_LARGE_EXP; piccolo.jl_amd/csrc/pcl_kernel_large_exp_hess.hpp), at the cases of tests/large_exp_hess_cases.py,
through the C ABI.  Every value is compared with scipy's expm / expm_frechet (tests/exp_hess_truth.py) at TOL = 1e-11 PER SEGMENT of every
interval, relative to the segment's own maximum with no floor at 1 (shape_cases.check_segments).  tests/test_large_exp_hess_cpu.py shows that the
kernel's recurrence in float64 agrees with that truth to 3e-13 on these inputs and that each listed fault moves a segment by 1e-7.

Without the feature every parity test here fails at pcl_set_option (PCL_EINVAL: unknown option 'large_exp_hess')."""
import ctypes

import numpy as np
import pytest
import torch

import exp_hess_truth as eht
import large_exp_cases as le
import large_exp_hess_cases as lh
import piccolo_jl_amd as pa
from shape_cases import check_segments

pytestmark = pytest.mark.gpu
TOL = 1e-11
ENOTIMPL, EINVAL = pa._lib.PCL_ENOTIMPL, pa._lib.PCL_EINVAL
MEMBERS, TRAJ = pa._lib.PCL_BATCH_MEMBERS, pa._lib.PCL_BATCH_TRAJ
NAN = float("nan")


def make_ctx(lay, G0, Gj, order="exp", hessian=True, **kw):
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                batch_mode=MEMBERS, pade_order=order, large_generator=True, large_exp=order == "exp", large_exp_hessian=hessian)  # fmt: skip
    if lay.gen is not None:
        args.update(d=lay.gen, state_cols=pa._lib.PCL_STATE_VECTOR)
    else:
        args.update(state_cols=lay.cols)
    args.update(kw)
    c = pa.integrators._PclContext(**args)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()


def nans(k):
    return torch.full((k,), NAN, dtype=torch.float64, device="cuda")


def hess_dev(c, Zd, mud):
    """pcl_hess_dev into a NaN-filled array, as numpy."""
    vd = nans(c.hess_nnz)
    c.hess_dev(Zd, mud, vd)
    c.sync()
    return vd.cpu().numpy()


def worst(errs):
    s = max(errs, key=errs.get)
    return "%.1e (%s)" % (errs[s], s)


def check(lay, got, ref, what):
    """No NaN may remain; every segment of every interval within TOL of the truth."""
    assert not np.isnan(got).any(), what
    er = check_segments(got, ref, lh.labels(lay), TOL)
    print("%s: Hessian of the Lagrangian %s" % (what, worst(er)))
    assert max(er.values()) <= TOL, (what, er)


# ---- every case ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lh.NAMES)
def test_hess_per_segment(name):
    """pcl_hess_dev against the truth; a second launch and the host-pointer call bitwise; the structure; which kernel ran."""
    lay, G0, Gj, Z = le.case(name)
    ref = lh.truth(name)
    c = make_ctx(lay, G0, Gj)
    assert c.large and c.large_exp and c.large_exp_hessian and c.get_option("large_exp_hess") == 1
    assert c.hess_per == eht.nnz_per_interval(lay) and c.hess_nnz == ref.size
    Zd, mud = dev(Z), dev(lh.mu(name))
    got = hess_dev(c, Zd, mud)
    assert c.get_option("last_hess_kernel") == 320
    check(lay, got, ref, name)
    assert np.array_equal(got, hess_dev(c, Zd, mud)), "a second launch"
    c.set_stream(None)
    assert np.array_equal(got, c.hess(Z, lh.mu(name))), "host pointers"
    er, ec = eht.structure(lay)
    for dt in (np.int32, np.int64):
        rows, cols = c.hess_structure(dt)
        assert np.array_equal(rows, er) and np.array_equal(cols, ec), dt
    c.close()


def test_index_base_one():
    lay, G0, Gj, Z = le.case("L1")
    c = make_ctx(lay, G0, Gj, index_base=1)
    er, ec = eht.structure(lay, index_base=1)
    for dt in (np.int32, np.int64):
        rows, cols = c.hess_structure(dt)
        assert np.array_equal(rows, er) and np.array_equal(cols, ec), dt
    check(lay, hess_dev(c, dev(Z), dev(lh.mu("L1"))), lh.truth("L1"), "L1, index_base 1")
    c.close()


# ---- the zero step ----------------------------------------------------------------------------------------------------------------------------------
def test_zero_step():
    """L1 with h = 0 on interval 1: segments 0 and 3 exactly zero there; the other intervals as ever."""
    lay, G0, Gj, Z = le.case("L1z")
    c = make_ctx(lay, G0, Gj)
    got = hess_dev(c, dev(Z), dev(lh.mu("L1z")))
    check(lay, got, lh.truth("L1z"), "L1 with a zero step")
    lab = lh.labels(lay)
    for s in ("seg0@1", "seg3@1"):
        assert np.any(lab == s) and not got[lab == s].any(), s
    for s in ("seg1@1", "seg2@1", "seg4@1"):
        assert got[lab == s].any(), s
    c.close()


def test_no_drives():
    """m = 0 (the system of L1 without its drives, two state columns): W alone -- the (dt,dt) entry and the (dt, X_k) vectors."""
    from oracle import pade_oracle as po

    _, G0, _, Z1 = le.case("L1")
    n, cols = 66, 2
    xs = n * cols
    lay = po.Layout(d=n // 2, m=0, N=le.N, z_dim=xs + 2, x_off=0, u_off=xs + 2, dt_off=xs, cols=cols)
    rng = np.random.default_rng(26900)
    Z = 0.4 * rng.standard_normal((le.N, lay.z_dim))
    Z[:, lay.dt_off] = np.array([0.8, -2.5, 20.5, 0.1]) / le.norm1(G0)
    mu = rng.standard_normal((lay.K, lay.x_dim))
    Gj = np.zeros((0, n, n))
    c = make_ctx(lay, G0, Gj)
    assert c.hess_per == 1 + lay.x_dim
    got = hess_dev(c, dev(Z), dev(mu))
    assert c.get_option("last_hess_kernel") == 320
    check(lay, got, eht.values(Z, mu, lay, G0, Gj).reshape(-1), "no drives")
    c.close()


# ---- every split gives the same bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, key, values", [("L5", "cols_per_slice", (1, 2, 5)), ("L6", "cols_per_slice", (7, 0)),
                                                ("L4", "large_exp_hess_drives", (1, 0)), ("L3", "large_exp_hess_drives", (1, 0))])  # fmt: skip
def test_splits_bitwise(name, key, values):
    lay, G0, Gj, Z = le.case(name)
    c = make_ctx(lay, G0, Gj)
    Zd, mud = dev(Z), dev(lh.mu(name))
    first = hess_dev(c, Zd, mud)
    check(lay, first, lh.truth(name), name)
    for v in values:
        c.set_option(key, v)
        assert c.get_option(key) == v
        assert np.array_equal(first, hess_dev(c, Zd, mud)), (key, v)
    assert c.get_option("last_hess_kernel") == 320
    c.close()


def test_both_knobs_at_once():
    lay, G0, Gj, Z = le.case("L5")
    c = make_ctx(lay, G0, Gj)
    Zd, mud = dev(Z), dev(lh.mu("L5"))
    first = hess_dev(c, Zd, mud)
    for cp, g in ((2, 1), (3, 4), (1, 3)):
        c.set_option("cols_per_slice", cp)
        c.set_option("large_exp_hess_drives", g)
        assert np.array_equal(first, hess_dev(c, Zd, mud)), (cp, g)
    with pytest.raises(pa.PclError) as ei:
        c.set_option("large_exp_hess_drives", -1)
    assert ei.value.code == EINVAL
    c.close()


# ---- batched launches -------------------------------------------------------------------------------------------------------------------------------
def test_members_with_their_own_drifts_and_the_window():
    """L5 as two PCL_BATCH_MEMBERS members with per-member drifts: each against its own truth; the window on the second alone gives its bits."""
    lay, _, Gj, Z = le.case("L5")
    G0s = [le.case("L5", 0, b)[1] for b in range(2)]
    c = make_ctx(lay, np.array(G0s), Gj, x_offs=[0, 0], batch=2, per_member_G0=True)
    per = eht.nnz_per_interval(lay) * lay.K
    assert c.hess_nnz == 2 * per
    mus = [lh.mu("L5", drift=b) for b in range(2)]
    Zd = dev(Z)
    vals = hess_dev(c, Zd, dev(np.stack(mus)))
    for b in range(2):
        check(lay, vals[b * per : (b + 1) * per], lh.truth("L5", drift=b), "members, member %d" % b)
    c.set_member_window(1, 1)
    assert c.hess_nnz == per
    assert np.array_equal(vals[per:], hess_dev(c, Zd, dev(mus[1]))), "the window on member 1"
    c.close()


def test_trajectory_seeds():
    """L7 (odd n) as two PCL_BATCH_TRAJ seeds, each against its own truth; the structure of the launch."""
    lay, G0, Gj, _ = le.case("L7")
    Zs = [le.case("L7", s)[3] for s in range(2)]
    c = make_ctx(lay, G0, Gj, batch=2, batch_mode=TRAJ)
    per = eht.nnz_per_interval(lay) * lay.K
    mus = [lh.mu("L7", seed=s) for s in range(2)]
    vals = hess_dev(c, dev(np.stack(Zs)), dev(np.stack(mus)))
    for s in range(2):
        check(lay, vals[s * per : (s + 1) * per], lh.truth("L7", seed=s), "seeds, seed %d" % s)
    rows, cols = c.hess_structure()
    for s in range(2):
        er, ec = eht.structure(lay, col0=s * lay.z_dim * lay.N)
        assert np.array_equal(rows[s * per : (s + 1) * per], er) and np.array_equal(cols[s * per : (s + 1) * per], ec)
    c.close()


# ---- the option -------------------------------------------------------------------------------------------------------------------------------------
def test_option_switches_the_five_entry_points():
    lay, G0, Gj, Z = le.case("L1")
    c = make_ctx(lay, G0, Gj, hessian=False)
    L, h = c._L, c._h
    assert c.get_option("large_exp_hess") == 0 and c.hess_nnz == 0
    Zd, mud = dev(Z), dev(lh.mu("L1"))
    nnz = eht.nnz_per_interval(lay) * lay.K
    out = nans(nnz)
    hb, ib = np.zeros(nnz), np.zeros(nnz, dtype=np.int64)
    ib2 = np.zeros(nnz, dtype=np.int64)
    i64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    Zh, muh = np.ascontiguousarray(Z).reshape(-1), np.ascontiguousarray(lh.mu("L1")).reshape(-1)
    calls = {
        "pcl_hess_nnz": lambda: L.pcl_hess_nnz(h, i64(ib), i64(ib2)),
        "pcl_hess_structure": lambda: L.pcl_hess_structure(h, i32(ib), i32(ib2)),
        "pcl_hess_structure_i64": lambda: L.pcl_hess_structure_i64(h, i64(ib), i64(ib2)),
        "pcl_hess": lambda: L.pcl_hess(h, Zh.ctypes.data, muh.ctypes.data, hb.ctypes.data),
        "pcl_hess_dev": lambda: L.pcl_hess_dev(h, Zd.data_ptr(), mud.data_ptr(), out.data_ptr()),
    }  # fmt: skip
    words = "%s is not implemented for a large exponential context (PCL_LARGE_N | PCL_LARGE_EXP, generator dimension %d > 64): residual and Jacobian, and by option large_full the objective and the rollout"

    def refused():
        for name, call in calls.items():
            rc = call()
            msg = (L.pcl_last_error(h) or b"").decode()
            assert rc == ENOTIMPL and msg == words % (name.replace("_i64", ""), lay.n), (name, rc, msg)

    def jac_bits():
        dd, vd = nans(c.n_rows), nans(c.jac_nnz)
        c.eval_jac_dev(Zd, dd, vd)
        c.sync()
        return dd.cpu().numpy(), vd.cpu().numpy()

    refused()
    before = jac_bits()
    for key in ("exp_hess", "large_hess"):  # ... at either value of the new option
        for v in (0, 1):
            c.set_option("large_exp_hess", v)
            with pytest.raises(pa.PclError) as ei:
                c.set_option(key, 1)
            assert ei.value.code == ENOTIMPL and "PCL_LARGE_EXP" in str(ei.value) and key in str(ei.value)
    c.set_option("large_exp_hess", 1)
    assert c.get_option("large_exp_hess") == 1 and c.hess_nnz == nnz and c.hess_per == eht.nnz_per_interval(lay)
    for name, call in calls.items():
        assert call() == 0, (name, (L.pcl_last_error(h) or b"").decode())
    c.sync()
    check(lay, out.cpu().numpy(), lh.truth("L1"), "L1, option set afterwards")
    assert np.array_equal(hb, out.cpu().numpy())
    p = out.data_ptr()
    still = {
        "pcl_jac_compact_nnz": lambda: L.pcl_jac_compact_nnz(h, i64(ib), i64(ib2)),
        "pcl_eval_jac_compact_dev": lambda: L.pcl_eval_jac_compact_dev(h, p, p, p),
        "pcl_jac_expand_dev": lambda: L.pcl_jac_expand_dev(h, p, p),
        "pcl_merit_grad_len": lambda: L.pcl_merit_grad_len(h, i64(ib), i64(ib2)),
        "pcl_merit_grad_dev": lambda: L.pcl_merit_grad_dev(h, p, p, p, p),
        "pcl_eval_jac_merit_dev": lambda: L.pcl_eval_jac_merit_dev(h, p, p, p, p, p),
    }  # fmt: skip
    for name, call in still.items():
        rc = call()
        msg = (L.pcl_last_error(h) or b"").decode()
        assert rc == ENOTIMPL and "PCL_LARGE_EXP" in msg and name in msg, (name, rc, msg)
    after = jac_bits()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "the residual + Jacobian launch"
    for bad in (2, -1):
        with pytest.raises(pa.PclError) as ei:
            c.set_option("large_exp_hess", bad)
        assert ei.value.code == EINVAL
    c.set_option("large_exp_hess", 0)
    assert c.get_option("large_exp_hess") == 0 and c.hess_nnz == 0
    refused()
    c.close()


def test_option_needs_a_large_exponential_context():
    import vector_shape_cases as vc

    lay, G0, Gj, Z, _ = vc.case("K5")  # n = 54 with both flags: the ordinary exponential context
    c = make_ctx(lay, G0, Gj, hessian=False)
    lay1, G1, Gj1, _ = le.case("L1")
    pade = make_ctx(lay1, G1, Gj1, order=8, hessian=False)  # a large Pade context
    plain = pa.integrators._PclContext(d=lay.d if lay.gen is None else lay.gen, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off,
                                       x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1, batch_mode=MEMBERS, pade_order=4,
                                       state_cols=pa._lib.PCL_STATE_VECTOR if lay.gen is not None else lay.cols)  # fmt: skip
    for ctx in (c, pade, plain):
        assert ctx.get_option("large_exp_hess") == 0
        with pytest.raises(pa.PclError) as ei:
            ctx.set_option("large_exp_hess", 1)
        assert ei.value.code == EINVAL
        with pytest.raises(pa.PclError) as ei:
            ctx.set_option("large_exp_hess_drives", 1)
        assert ei.value.code == EINVAL
        ctx.set_option("large_exp_hess", 0)
        ctx.close()
    # the keyword at n <= 64 sets nothing: exp_hessian is that context's switch
    c = make_ctx(lay, G0, Gj, hessian=True)
    assert not c.large_exp and not c.large_exp_hessian and c.get_option("large_exp_hess") == 0 and c.hess_nnz == 0
    c.close()


# ---- consistency inside the library ------------------------------------------------------------------------------------------------------------------
def test_directional_derivative_of_the_device_jacobian():
    """H v against the central difference (step 1e-6) of the device's own J' mu, formed on the device from two pcl_jac_dev results.  Step and
    bound are those of tests/test_exp_hess_gpu.py: 1e-6 max(1, |fd|_inf)."""
    lay, G0, Gj, Z = le.case("L5")
    c = make_ctx(lay, G0, Gj)
    nv = lay.z_dim * lay.N
    rng = np.random.default_rng(12)
    mu = torch.from_numpy(rng.standard_normal(c.n_rows)).cuda()
    v = rng.standard_normal(nv)
    v = torch.from_numpy(v / np.linalg.norm(v)).cuda()
    Zd = torch.from_numpy(Z.reshape(-1).copy()).cuda()
    jr, jc = (torch.from_numpy(a).cuda() for a in c.jac_structure())
    hr, hc = (torch.from_numpy(a).cuda() for a in c.hess_structure())

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
    err, scale = (Hv - fd).abs().max().item(), max(1.0, fd.abs().max().item())
    print("|H v - fd|_inf %.3e   |fd|_inf %.3e" % (err, fd.abs().max().item()))
    assert err <= 1e-6 * scale, (err, scale)
    c.close()


# ---- the Python keyword -------------------------------------------------------------------------------------------------------------------------------
def test_bilinear_integrator_keyword():
    """BilinearIntegrator(..., large_generator=True, large_exp=True, large_exp_hessian=True) on a d = 33 ket system: eval_hessian_of_lagrangian
    against the scattered truth."""
    import vector_shape_cases as vc
    from oracle import pade_oracle as po

    d, m, N = 33, 2, 4
    rng = np.random.default_rng(25500)
    s = pa.QuantumSystem(vc._herm(d, rng), [vc._herm(d, rng) for _ in range(m)], [1.0] * m)
    psi = rng.standard_normal(d) + 1j * rng.standard_normal(d)
    psi /= np.linalg.norm(psi)
    times = np.cumsum(np.concatenate(([0.0], 0.05 + 0.05 * rng.random(N - 1))))
    traj = pa.ket_trajectory(s, 0.3 * rng.standard_normal((m, N)), times, psi, psi)
    Z = traj.datavec.reshape(N, traj.dim).copy()
    KET = pa.trajectory.KET
    B = pa.BilinearIntegrator(s, traj, x_name=KET, pade_order="exp", large_generator=True, large_exp=True, large_exp_hessian=True)
    assert B.ctx.large_exp and B.ctx.large_exp_hessian and B.ctx.get_option("large_exp_hess") == 1
    lay = po.Layout(d=d, m=m, N=N, z_dim=traj.dim, x_off=traj.components[KET].start, u_off=traj.components["u"].start,
                    dt_off=traj.components[traj.timestep].start, cols=1)  # fmt: skip
    G0, Gj = s.G_drift, s.G_drives_array()
    mu = np.random.default_rng(3).standard_normal(B.dim)
    v0 = eht.values(Z, mu.reshape(lay.K, lay.x_dim), lay, G0, Gj, x_off=lay.x_off).reshape(-1)
    r0, c0 = eht.structure(lay, x_off=lay.x_off)
    r, c = pa.hessian_structure(B)
    assert np.array_equal(r, r0) and np.array_equal(c, c0)
    check(lay, B.ctx.hess(traj.datavec, mu), v0, "BilinearIntegrator, d = 33 ket")
    assert B.ctx.get_option("last_hess_kernel") == 320
    H = pa.eval_hessian_of_lagrangian(B, traj, mu).toarray()
    Ht = eht.dense(v0, lay, lay.x_off)
    assert H.shape[0] >= Ht.shape[0]
    nz = Ht.shape[0]
    assert np.abs(H[:nz, :nz] - Ht).max() <= TOL * max(1.0, np.abs(Ht).max()) and np.array_equal(H, H.T)
    B.close()
