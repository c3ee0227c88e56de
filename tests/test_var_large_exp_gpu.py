"""The variational exponential constraint at generator dimensions 66 .. 128 on the device (contexts created with PCL_BATCH_VARIATIONAL_EXP |
PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP; piccolo.jl_amd/csrc/pcl_kernel_var_large_exp.hpp), at the cases of tests/var_large_exp_cases.py,
through the C ABI on device pointers.  Every value is compared with scipy's expm / expm_frechet on the lifted generator (var_exp_truth) at
TOL = 1e-11 PER SEGMENT (row component x variable kind x relative knot x interval), relative to the segment's own maximum -- the project's
tolerance for every kernel family -- and a segment whose truth is identically zero must be exact zeros.  tests/test_var_large_exp_cpu.py shows that
a float64 emulation of the kernel's recurrence meets that truth at 7e-14, that scipy meets a longdouble series at 2e-15, and which mutant each
case sees.

Without the feature every test here fails before the device is reached: the binding has no PCL_LARGE_VAR_EXP and its constructors do not know
the keyword (AttributeError / TypeError)."""
import ctypes

import numpy as np
import pytest
import torch

import piccolo_jl_amd as pa
import var_exp_truth as vet
import var_large_exp_cases as vx
from oracle import pade_oracle as po

pytestmark = pytest.mark.gpu
TOL = 1e-11
L = pa._lib
NAN = float("nan")
KIND = "large variational exponential context (PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP"


def make_ctx(cs, **kw):
    c = pa.integrators._PclContext(**vx.context_args(cs, batch_mode=L.PCL_BATCH_VARIATIONAL_EXP, large_generator=True, large_variational=True,
                                                      large_var_exp=True, **kw))  # fmt: skip
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def plain_ctx(cs, b=0):
    """A plain PCL_LARGE_N | PCL_LARGE_EXP context of the same drift and drives on component b of the same knots."""
    c = pa.integrators._PclContext(d=cs.n // 2, m=cs.m, N=cs.N, z_dim=cs.z_dim, u_off=cs.u_off, dt_off=cs.dt_off, x_offs=[cs.xo[b]], G0=cs.G0, Gj=cs.Gj,
                                   batch=1, batch_mode=L.PCL_BATCH_MEMBERS, pade_order="exp", state_cols=cs.C, large_generator=True, large_exp=True)  # fmt: skip
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()


def nans(k):
    return torch.full((k,), NAN, dtype=torch.float64, device="cuda")


def eval_jac_dev(c, Zd):
    """(delta, values) of pcl_eval_jac_dev into NaN-filled arrays, as numpy."""
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    return dd.cpu().numpy(), vd.cpu().numpy()


def eval_dev(c, Zd):
    dd = nans(c.n_rows)
    c.eval_dev(Zd, dd)
    c.sync()
    return dd.cpu().numpy()


def bitwise(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


def refused(code, words, f, *args):
    with pytest.raises(pa.PclError) as ei:
        f(*args)
    assert ei.value.code == code, str(ei.value)
    for w in [words] if isinstance(words, str) else words:
        assert w in str(ei.value), str(ei.value)


# ---- accuracy, per case --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vx.NAMES)
def test_eval_jac_per_segment(name):
    """pcl_eval_jac_dev against the truth (worst deviations read on an MI355X: see DESIGN.md 4.29); pcl_eval_dev alone, pcl_jac_dev alone and a
    second launch give its bits; which kernel ran; the structure at both index bases; nothing compiled at run time."""
    cs = vx.case(name)
    ref = vx.truth(name)
    c = make_ctx(cs)
    assert c.x_dim == cs.xd and c.n_rows == ref[0].size and c.jac_nnz == ref[1].size and c.jac_per == vet.nnz_per_interval(cs)
    assert c.hess_nnz == 0 and c.compact_nnz == 0 and c.get_option("variations") == cs.v and c.pade_order == -1
    assert c.get_option("large_variational_exp") == 1 and c.get_option("large_variational") == 1 and c.large_variational_exp
    Zd = dev(cs.Z)
    got = eval_jac_dev(c, Zd)
    assert c.get_option("last_kernel") == 370
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    wd, wj = vx.check(name, got[0], got[1], TOL, "pcl_eval_jac_dev")
    print("%s: residual %.1e (%s)  Jacobian %.1e (%s)" % (name, wd[0], wd[1], wj[0], wj[1]))
    bitwise((got[0],), (eval_dev(c, Zd),), "pcl_eval_dev alone")
    assert c.get_option("last_kernel") == 371
    v2 = nans(c.jac_nnz)
    c.jac_dev(Zd, v2)
    c.sync()
    bitwise((got[1],), (v2.cpu().numpy(),), "pcl_jac_dev alone")
    bitwise(got, eval_jac_dev(c, Zd), "a second launch")
    r, cc = c.jac_structure()
    er, ec = vet.structure(cs)
    assert np.array_equal(r, er) and np.array_equal(cc, ec)
    assert c.get_option("jit_compiles") == 0
    c.close()
    if name == "VL1":
        c1 = make_ctx(cs, index_base=1)
        r1, cc1 = c1.jac_structure(np.int32)
        assert np.array_equal(r1, er + 1) and np.array_equal(cc1, ec + 1)
        c1.close()


def test_zero_step_interval():
    """VL2's interval of h = 0: -E = -I exactly, L_i and the drive tails exact zeros, the dt tail -(Gv_i X + G Xv_i)."""
    cs = vx.case("VL2")
    c = make_ctx(cs)
    _, vals = eval_jac_dev(c, dev(cs.Z))
    c.close()
    n, C, v, m = cs.n, cs.C, cs.v, cs.m
    iv = vals.reshape(cs.K, -1)[3]
    blk = iv[: (1 + 2 * v) * C * n * n].reshape(1 + 2 * v, C, n * n)
    minus_eye = np.tile(-np.eye(n).reshape(-1), (C, 1))
    assert np.array_equal(blk[0], minus_eye)
    for b in range(1, v + 1):
        assert np.array_equal(blk[2 * b - 1], minus_eye) and not blk[2 * b].any()
    tails = iv[(1 + 2 * v) * C * n * n + cs.xd :].reshape(1 + v, C, m + 1, n)
    assert not tails[:, :, :m].any()
    G = vx.g_of(cs, 3)
    X = [cs.Z[3, o : o + cs.xdc].reshape(C, n) for o in cs.xo]
    for b in range(1 + v):
        want = -(X[b] @ G.T + (X[0] @ cs.Gv[b - 1].T if b else 0.0))
        assert np.abs(tails[b, :, m] - want).max() <= 1e-13 * np.abs(want).max()


# ---- host pointers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["VL1", "VL2"])
def test_host_pointer_calls_deliver_the_same_bits(name):
    cs = vx.case(name)
    c = make_ctx(cs)
    first = eval_jac_dev(c, dev(cs.Z))
    Z = cs.Z.reshape(-1)
    d, v = c.eval_jac(Z, np.full(c.n_rows, NAN), np.full(c.jac_nnz, NAN))
    bitwise(first, (d, v), "pcl_eval_jac")
    bitwise((first[0],), (c.eval(Z, np.full(c.n_rows, NAN)),), "pcl_eval")
    bitwise((first[1],), (c.jac(Z, np.full(c.jac_nnz, NAN)),), "pcl_jac")
    c.close()


# ---- every split -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["VL2", "VL5"])
def test_every_split_bitwise(name):
    """cols_per_slice, general_slices and large_var_exp_drives, one at a time and together."""
    cs = vx.case(name)
    c = make_ctx(cs)
    Zd = dev(cs.Z)
    first = eval_jac_dev(c, Zd)

    def same(what):
        bitwise(first, eval_jac_dev(c, Zd), what)
        bitwise((first[0],), (eval_dev(c, Zd),), ("pcl_eval_dev", what))

    for cp in (1, 2, 0):
        c.set_option("cols_per_slice", cp)
        same(("cols_per_slice", cp))
    for s in (cs.n, 0):
        c.set_option("general_slices", s)
        same(("general_slices", s))
    for g in (1, 2, cs.m, 0):
        c.set_option("large_var_exp_drives", g)
        assert c.get_option("large_var_exp_drives") == g
        same(("large_var_exp_drives", g))
    c.set_option("cols_per_slice", 2)
    c.set_option("general_slices", 17)
    c.set_option("large_var_exp_drives", 2)
    same("all three")
    assert c.get_option("last_kernel") == 371
    refused(L.PCL_EINVAL, "large_var_exp_drives", c.set_option, "large_var_exp_drives", -1)
    c.close()
    p = plain_ctx(cs)
    refused(L.PCL_EINVAL, ["large_var_exp_drives", "PCL_LARGE_VAR_EXP"], p.set_option, "large_var_exp_drives", 1)
    p.close()


# ---- component 0 has the bits of a plain large exponential context -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["VL2", "VL3", "VL4"])
def test_component_0_has_the_bits_of_a_plain_large_exponential_context(name):
    """delta_0, component 0's tails and the -E copies of EVERY component against a PCL_LARGE_N | PCL_LARGE_EXP context of the same drift and drives."""
    cs = vx.case(name)
    Zd = dev(cs.Z)
    c = make_ctx(cs)
    d, v = eval_jac_dev(c, Zd)
    c.close()
    p = plain_ctx(cs)
    assert p.get_option("large_variational_exp") == 0
    d0, v0 = eval_jac_dev(p, Zd)
    assert p.get_option("last_kernel") == 320
    p.close()
    dv, dp, jv, jp = vx.component_vs_plain(cs)
    assert len(np.unique(dp)) == d0.size and len(np.unique(jp)) == v0.size
    assert np.array_equal(d[dv], d0[dp]), "delta_0"
    assert np.array_equal(v[jv], v0[jp]), "the -E copies, the ones and component 0's tails"


@pytest.mark.parametrize("name", ["VL1", "VL2"])
def test_zero_variation_generators(name):
    """Gv_i = 0: the -L_i block exactly zero, and component i's rows (delta_i, its -E copy, its tails) those of a plain large exponential context
    on Xv_i."""
    cs = vx.case(name, True)
    Zd = dev(cs.Z)
    c = make_ctx(cs)
    d, v = eval_jac_dev(c, Zd)
    c.close()
    n, C = cs.n, cs.C
    per = v.reshape(cs.K, -1)
    for b in range(1, cs.v + 1):
        assert not per[:, 2 * b * C * n * n : (2 * b + 1) * C * n * n].any(), "-L_%d" % b
        p = plain_ctx(cs, b)
        d0, v0 = eval_jac_dev(p, Zd)
        p.close()
        dv, dp, jv, jp = vx.component_vs_plain(cs, b)
        assert len(np.unique(dp)) == d0.size and len(np.unique(jp)) == v0.size
        assert np.array_equal(d[dv], d0[dp]), "delta_%d" % b
        assert np.array_equal(v[jv], v0[jp]), "component %d's -E copy, ones and tails" % b


def test_largest_value_count_is_written_everywhere():
    """n = 128 unitary, v = 2: 10.5 M values per interval, no truth (tests/var_large_exp_cases.py): nothing stays NaN, and component 0 has the
    plain large exponential context's bits."""
    cs = vx.case_vl7()
    Zd = dev(cs.Z)
    c = make_ctx(cs)
    assert c.jac_per == 5 * 64 * 128 * 128 + 3 * 128 * 64 * 3
    d, v = eval_jac_dev(c, Zd)
    c.close()
    assert not np.isnan(d).any() and not np.isnan(v).any()
    p = plain_ctx(cs)
    d0, v0 = eval_jac_dev(p, Zd)
    p.close()
    dv, dp, jv, jp = vx.component_vs_plain(cs)
    assert np.array_equal(d[dv], d0[dp]) and np.array_equal(v[jv], v0[jp])


# ---- large_var_full: the objective family and the rollout, through the kernels of the Pade kind -------------------------------------------------------------
def _pade_ctx(cs):
    c = pa.integrators._PclContext(**vx.vl.context_args(cs, 8, batch_mode=L.PCL_BATCH_VARIATIONAL, large_generator=True, large_variational=True,
                                                         large_var_full=True))  # fmt: skip
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def _objective_family(c, cs, Zd):
    """(value, gradient, the objective's Hessian values, the rollout) with a goal and, on a unitary, a sensitivity weight."""
    rng = np.random.default_rng(5)
    if cs.C > 1:
        goal = rng.standard_normal(c.goal_dim)
        c.set_goal(goal / np.linalg.norm(goal))
    else:  # a ket: F = (a_1'x)^2 + (a_2'x)^2
        A = rng.standard_normal((2, c.goal_dim))
        c.set_goal_form(0, A / np.linalg.norm(A, axis=1, keepdims=True), None)
    c.set_weights(np.array([1.0] + [0.3 if cs.C > 1 else 0.0] * cs.v))
    Zf = cs.Z.reshape(-1)
    val, grad = c.objective(Zf, 2.0)
    hv = c.objective_hess(Zf, 2.0, 1.0)
    xo = nans(cs.N * cs.xd)
    c.rollout_dev(Zd, xo)
    c.sync()
    return np.asarray(val), np.asarray(grad), np.asarray(hv), xo.cpu().numpy()


@pytest.mark.parametrize("name", ["VL1", "VL2"])
def test_large_var_full_serves_objective_and_rollout_with_the_pade_kinds_bits(name):
    cs = vx.case(name)
    Zd = dev(cs.Z)
    c = make_ctx(cs, large_var_full=True)
    assert c.get_option("large_var_full") == 1
    got = _objective_family(c, cs, Zd)
    assert c.get_option("last_kernel") == 360
    # the context's own rollout satisfies its own rows: delta at the rolled-out states
    X = got[3].reshape(cs.N, cs.xd)
    Z2 = np.array(cs.Z)
    for b, o in enumerate(cs.xo):
        Z2[:, o : o + cs.xdc] = X[:, b * cs.xdc : (b + 1) * cs.xdc]
    d = eval_dev(c, dev(Z2))
    print("%s: max |delta| at the context's own rollout %.1e of max |X| %.1e" % (name, np.abs(d).max(), np.abs(X).max()))
    assert np.abs(d).max() <= 1e-12 * np.abs(X).max()
    c.close()
    p = _pade_ctx(cs)
    want = _objective_family(p, cs, Zd)
    p.close()
    assert not any(np.isnan(a).any() for a in got)
    bitwise(got, want, "objective, gradient, objective Hessian, rollout")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_the_kinds_words():
    """Every family the kind does not serve: PCL_ENOTIMPL in one sentence naming the flag; the context is usable afterwards."""
    cs = vx.case("VL1")
    c = make_ctx(cs)
    Zd = dev(cs.Z)
    first = eval_jac_dev(c, Zd)
    buf = nans(max(c.jac_nnz, cs.N * cs.xd))
    one = torch.zeros(1, dtype=torch.float64, device="cuda")

    def not_impl(what, f, *args):
        refused(L.PCL_ENOTIMPL, [what + " is not implemented for a " + KIND, "generator dimension 66 > 64", "large_var_full"], f, *args)

    not_impl("pcl_hess_nnz", lambda: c._chk(c._L.pcl_hess_nnz(c._h, ctypes.byref(ctypes.c_int64()), ctypes.byref(ctypes.c_int64()))))
    not_impl("pcl_jac_compact_nnz", lambda: c._chk(c._L.pcl_jac_compact_nnz(c._h, ctypes.byref(ctypes.c_int64()), ctypes.byref(ctypes.c_int64()))))
    not_impl("pcl_hess_structure", c.hess_structure)
    not_impl("pcl_hess_dev", c.hess_dev, Zd, buf, buf)
    not_impl("pcl_hess", c.hess, cs.Z.reshape(-1), np.ones(c.n_rows), np.zeros(8))
    not_impl("pcl_eval_jac_compact_dev", c.eval_jac_compact_dev, Zd, buf, buf)
    not_impl("pcl_merit_grad_dev", c.merit_grad_dev, buf, buf, buf, buf)
    not_impl("pcl_eval_jac_merit_dev", c.eval_jac_merit_dev, Zd, buf, buf, buf, buf)
    not_impl("pcl_eval_jac_merit_objective_dev", c.eval_jac_merit_objective_dev, Zd, buf, buf, buf, buf, 1.0, one, buf)
    not_impl("pcl_set_member_window", c.set_member_window, 0, 1)
    not_impl("pcl_infidelity_dev", c.infidelity_dev, Zd, 1.0, one, buf)
    not_impl("pcl_reduce_sum_dev", c.reduce_sum_dev, buf)
    for key in ("large_var_hess", "var_compact", "var_exp_hess", "var_full", "exp_hess"):
        refused(L.PCL_ENOTIMPL, [key + " = 1 is not implemented for a " + KIND, "large_var_full"], c.set_option, key, 1)
        c.set_option(key, 0)
        assert c.get_option(key) == 0
    for key in ("large_hess", "large_full", "large_reduce", "large_exp_hess", "large_exp_reduce"):
        refused(L.PCL_EINVAL, key + " = 1 needs", c.set_option, key, 1)
    # the objective family and the rollout: without large_var_full, with it, without it again
    not_impl("pcl_rollout_dev", c.rollout_dev, Zd, buf)
    not_impl("pcl_set_goal", c.set_goal, np.ones(c.goal_dim))
    not_impl("pcl_objective", c.objective, cs.Z.reshape(-1), 1.0)
    c.set_option("large_var_full", 1)
    c.rollout_dev(Zd, buf)
    c.sync()
    assert c.get_option("last_kernel") == 360
    not_impl("pcl_hess_dev", c.hess_dev, Zd, buf, buf)  # (the other refusals stay at either value)
    c.set_option("large_var_full", 0)
    not_impl("pcl_rollout_dev", c.rollout_dev, Zd, buf)
    # the order calls: as on every exponential context
    refused(L.PCL_EINVAL, "exponential constraint", c.set_order_policy, 0.1, 1.0)
    refused(L.PCL_EINVAL, "exponential constraint", c.set_order_from_trajectory, cs.Z.reshape(-1))
    bitwise(first, eval_jac_dev(c, Zd), "after the refusals")
    assert c.get_option("jit_compiles") == 0
    c.close()


# ---- small n, n > 128 -----------------------------------------------------------------------------------------------------------------------------------------
def test_all_four_flags_at_n_54_are_the_ordinary_context():
    import variational_truth as vt

    d, v, m, N = 27, 1, 2, 4
    n = 2 * d
    rng = np.random.default_rng(91)
    herm = lambda: (lambda A: (A + A.conj().T) / (2 * np.sqrt(d)))(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
    G0, Gj, Gv = po.G_of_H(herm()), np.array([po.G_of_H(herm()) for _ in range(m)]), [po.G_of_H(herm()) / 3.0]
    z_dim = 2 * n + 2 + m
    Z = 0.4 * rng.standard_normal((N, z_dim))
    Z[:, 2 * n] = [0.05, -0.08, 0.3, 0.1]
    cs = vt.VarCase(Z=Z, z_dim=z_dim, N=N, n=n, C=1, m=m, xo=[0, n], u_off=2 * n + 2, dt_off=2 * n, G0=G0, Gv=Gv, Gj=Gj)
    Zd = dev(Z)
    c = make_ctx(cs)
    assert not c.large_variational_exp and c.get_option("large_variational_exp") == 0 and c.get_option("large_variational") == 0
    got = eval_jac_dev(c, Zd)
    assert c.get_option("last_kernel") == 110
    c.close()
    o = pa.integrators._PclContext(**vx.context_args(cs, batch_mode=L.PCL_BATCH_VARIATIONAL_EXP))
    o.set_stream(torch.cuda.current_stream().cuda_stream)
    want = eval_jac_dev(o, Zd)
    o.close()
    bitwise(got, want, "the four flags at n = 54")
    with pytest.raises(pa.PclError) as ei:
        make_ctx(vt.VarCase(Z=np.zeros((3, 2 * 64 + 3)), z_dim=2 * 64 + 3, N=3, n=64, C=1, m=1, xo=[0, 64], u_off=130, dt_off=128, G0=np.zeros((64, 64)),
                            Gv=[np.zeros((64, 64))], Gj=np.zeros((1, 64, 64))))  # fmt: skip
    assert ei.value.code == L.PCL_ESHAPE and "served up to n = 62" in str(ei.value)


# ---- the public constructors ------------------------------------------------------------------------------------------------------------------------------------
def test_public_constructors_on_vl1():
    """VariationalKetIntegrator and VariationalUnitaryIntegrator with large_generator=True, large_var_exp=True, pade_order="exp" on VL1's
    Hamiltonians, through evaluate_ and eval_jacobian."""
    import var_large_cases as vl

    cs = vx.case("VL1")
    H0, Hd, Hv = vl.hamiltonians("VL1")
    sysv = pa.VariationalQuantumSystem(H0, list(Hd), list(Hv), [1.0] * cs.m)
    comps = {"ψ̃": cs.Z[:, cs.xo[0] : cs.xo[0] + cs.xdc].T, "ψ̃_var": cs.Z[:, cs.xo[1] : cs.xo[1] + cs.xdc].T, "Δt": cs.Z[:, cs.dt_off][None],
             "t": cs.Z[:, cs.dt_off + 1][None], "u": cs.Z[:, cs.u_off : cs.u_off + cs.m].T}  # fmt: skip
    traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
    assert np.array_equal(traj.datavec, cs.Z.reshape(-1))
    with pytest.raises(ValueError, match="large_generator=True on a variational integrator"):  # without the keyword: as ever
        pa.VariationalKetIntegrator(sysv, traj, "ψ̃", ["ψ̃_var"], "u", scale=vl.SCALES[0], pade_order="exp", large_generator=True)
    B = pa.VariationalKetIntegrator(sysv, traj, "ψ̃", ["ψ̃_var"], "u", scale=vl.SCALES[0], pade_order="exp", large_generator=True, large_var_exp=True)
    assert B.ctx.large_variational_exp and B.pade_order == -1 and B.dim == cs.K * cs.xd
    delta, vals = B.ctx.eval_jac(traj.datavec)
    wd, wj = vx.check("VL1", delta, vals, TOL, "through VariationalKetIntegrator")
    print("VariationalKetIntegrator, large_var_exp=True: residual %.1e  Jacobian %.1e" % (wd[0], wj[0]))
    out = np.zeros(B.dim)
    pa.evaluate_(out, B, traj)
    assert np.array_equal(out, delta)
    J = pa.eval_jacobian(B, traj)
    r, c = vet.structure(cs)
    assert J.shape == (B.dim, cs.N * cs.z_dim) and np.array_equal(np.asarray(J[r, c]).reshape(-1), vals)
    with pytest.raises(pa.PclError, match="PCL_LARGE_VAR_EXP"):
        pa.hessian_structure(B)
    B.close()
    # the unitary constructor: a 33-level unitary on the same Hamiltonians, one launch of every value against the context's own numbers
    rng = np.random.default_rng(3)
    xdc = cs.n * (cs.n // 2)
    comps = {"Ũ⃗": 0.4 * rng.standard_normal((xdc, cs.N)), "Ũ⃗_var": 0.4 * rng.standard_normal((xdc, cs.N)), "Δt": cs.Z[:, cs.dt_off][None],
             "t": cs.Z[:, cs.dt_off + 1][None], "u": cs.Z[:, cs.u_off : cs.u_off + cs.m].T}  # fmt: skip
    traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
    B = pa.VariationalUnitaryIntegrator(sysv, traj, "Ũ⃗", ["Ũ⃗_var"], "u", scales=[vl.SCALES[0]], pade_order="exp", large_generator=True, large_var_exp=True)
    assert B.ctx.large_variational_exp and B.ctx.x_dim == 2 * xdc
    out = np.full(B.dim, NAN)
    pa.evaluate_(out, B, traj)
    delta, vals = B.ctx.eval_jac(traj.datavec)
    assert np.array_equal(out, delta) and not np.isnan(vals).any() and B.ctx.get_option("last_kernel") == 370
    B.close()
