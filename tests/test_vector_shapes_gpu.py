"""The Pade kernels on the device for the states that are not a square unitary -- kets, multi-ket states, density vectors -- at the sizes of
tests/vector_shape_cases.py (the case table and the branch each case straddles are there), through _PclContext / the C ABI.  Every value is
compared with the longdouble truth of that module, rounded to float64, at TOL = 1e-11 PER SEGMENT, relative to the segment's own maximum with
no floor at 1 (shape_cases.check_segments).  tests/test_vector_shapes_cpu.py shows that the oracle agrees with that truth to 1e-13 on these
inputs and that each case sees a zeroed top coefficient, a dropped k step, a dropped row tile, an ignored column, drive or drive pair at 1e-7.

Which kernel `auto` runs per case and order is asserted against vector_shape_cases.expected_family and shown in the test ids
(eval_jac / eval / hess: 190 + q lock-step, 90 + q reference formulation and general Hessian, 50 + q small kernel, 10 / 20 fused order-4
kernels, 1 / 2 order-4 Hessian kernels)."""
import numpy as np
import pytest
import torch

import piccolo_jl_amd as pa
import vector_shape_cases as vc
from oracle import pade_oracle as po
from shape_cases import check_segments, hess_labels, jac_labels

pytestmark = pytest.mark.gpu
TOL = 1e-11
ESHAPE = pa._lib.PCL_ESHAPE
NAMES = list(vc.CASES)
NAN = float("nan")


def make_ctx(lay, G0, Gj, order, **kw):
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                batch_mode=pa._lib.PCL_BATCH_MEMBERS, pade_order=order)  # fmt: skip
    if lay.gen is not None:
        args.update(d=lay.gen, state_cols=pa._lib.PCL_STATE_VECTOR)
    else:
        args.update(state_cols=lay.cols)
    host_path = kw.pop("host_path", 1)
    args.update(kw)
    c = pa.integrators._PclContext(**args)
    c.set_option("host_path", host_path)
    return c


def run_all(c, Z, mu):
    """((delta, values, Hessian values), (last_kernel after eval_jac, after eval, last_hess_kernel), delta of eval)"""
    delta, vals = c.eval_jac(Z)
    kj = c.get_option("last_kernel")
    d2 = c.eval(Z)
    ke = c.get_option("last_kernel")
    h = c.hess(Z, mu)
    return (delta, vals, h), (kj, ke, c.get_option("last_hess_kernel")), d2


def worst(errs):
    s = max(errs, key=errs.get)
    return "%.1e (%s)" % (errs[s], s)


def check_values(lay, got, ref, what=""):
    """got, ref: (delta | None, values | None, Hessian values | None)"""
    out = []
    for g, r, labels, kind in zip(got, ref, (vc.residual_labels(lay), jac_labels(lay), hess_labels(lay)), ("residual", "Jacobian", "Hessian")):
        if g is not None:
            out.append("%s %s" % (kind, worst(check_segments(g, r, labels, TOL))))
    print(what + ": " + "  ".join(out))


def bitwise(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


def family_id(name, order):
    return "%s-%d-%d/%d/%d" % ((name, order) + vc.expected_family(name, order))


# ---- what `auto` runs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, order", [pytest.param(n, o, id=family_id(n, o)) for n in NAMES for o in vc.ORDERS])
def test_auto_per_segment(name, order):
    lay, G0, Gj, Z, _ = vc.case(name)
    d0, v0, mu, h0 = vc.truth(name, order)
    c = make_ctx(lay, G0, Gj, order)
    assert c.n_rows == d0.size and c.jac_nnz == v0.size and c.hess_nnz == h0.size
    got, fam, d2 = run_all(c, Z, mu)
    print("%s order %d ran eval_jac %d, eval %d, hess %d" % ((name, order) + fam))
    check_values(lay, got, (d0, v0, h0), "%s order %d" % (name, order))
    check_segments(d2, d0, vc.residual_labels(lay), TOL)
    assert fam == vc.expected_family(name, order), (name, order, fam)
    assert np.array_equal(got[2], c.hess(Z, mu))  # bitwise repeatable
    c.close()


# ---- every family and work split a case admits ---------------------------------------------------------------------------------------------------
def _set(c, **opts):
    for k, v in opts.items():
        c.set_option(k, v)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("order", [4, 10])
def test_forced_families(name, order):
    """Across families the values agree within TOL (each is held to the truth); within a family, whatever the work split, bitwise."""
    kind, n, cols, m = vc.CASES[name]
    q = order // 2
    lay, G0, Gj, Z, _ = vc.case(name)
    ref = vc.truth(name, order)
    ref, mu = (ref[0], ref[1], ref[3]), ref[2]
    c = make_ctx(lay, G0, Gj, order)
    ej = lambda: c.eval_jac(Z)
    label = "%s order %d " % (name, order)
    if order == 4:  # the general-order kernels as a second implementation of kernels 10 / 20 / 1 / 2 (a vector context runs them anyway)
        c.set_option("general_pade_kernel", 1)
        got, fam, d2 = run_all(c, Z, mu)
        assert fam == ((190 + q if n % 2 == 0 else 90 + q), 90 + q, 90 + q), fam
        check_values(lay, got, ref, label + "general_pade_kernel")
        check_segments(d2, ref[0], vc.residual_labels(lay), TOL)
    # the reference formulation: thread counts and, on several columns, the columns per workgroup
    c.set_option("general_kernel_version", 1)
    first = ej()
    assert c.get_option("last_kernel") == 90 + q
    check_values(lay, first + (None,), ref, label + "reference formulation")
    c.set_option("general_threads", 256)
    bitwise(first, ej(), "general_threads")
    for cp in (1, 2, 3) if cols > 1 else ():
        c.set_option("cols_per_slice", cp)
        bitwise(first, ej(), ("reference formulation, cols_per_slice", cp))
        assert c.get_option("last_kernel") == 90 + q
    _set(c, general_threads=512, cols_per_slice=0)
    # the lock-step kernel (even n), slices
    c.set_option("general_kernel_version", 2)
    if n % 2 == 0:
        lock = ej()
        assert c.get_option("last_kernel") == 190 + q
        check_values(lay, lock + (None,), ref, label + "lock-step")
        for s in sorted({1, 2, cols}):
            c.set_option("general_slices", s)
            bitwise(lock, ej(), ("general_slices", s))
            assert c.get_option("last_kernel") == 190 + q
        c.set_option("general_slices", 0)
    else:
        with pytest.raises(pa.PclError) as ei:
            ej()
        assert ei.value.code == ESHAPE
    _set(c, general_kernel_version=0, general_pade_kernel=0)
    # without the matrix cores: the general Hessian; at order 4 kernels 10 and 1
    c.set_option("use_mfma", 0)
    got, fam, _ = run_all(c, Z, mu)
    assert (fam[0], fam[2]) == ((10, 1) if order == 4 and kind == "iso" else (vc.expected_family(name, order)[0], 1 if order == 4 else 90 + q)), fam
    check_values(lay, got, ref, label + "use_mfma = 0")
    c.set_option("use_mfma", 1)
    # the small kernel's 16-row instance with the Jacobian
    if name in ("V1", "V2", "M1"):
        c.set_option("kernel_version", 5)
        got, fam, d2 = run_all(c, Z, mu)
        assert fam[:2] == (50 + q, 50 + q), fam
        check_values(lay, got, ref, label + "kernel_version = 5")
        check_segments(d2, ref[0], vc.residual_labels(lay), TOL)
        c.set_option("kernel_version", 0)
    if order == 4 and kind == "iso":
        # kernels 10 and 20 against each other, and their column slices
        res = {}
        for kv in (1, 2):
            c.set_option("kernel_version", kv)
            res[kv] = ej()
            assert c.get_option("last_kernel") == 10 * kv
            check_values(lay, res[kv] + (None,), ref, label + "kernel_version = %d" % kv)
            check_segments(c.eval(Z), ref[0], vc.residual_labels(lay), TOL)
            assert c.get_option("last_kernel") == 10 * kv
            for cp in (1, 2, 3) if cols > 1 else ():
                c.set_option("cols_per_slice", cp)
                bitwise(res[kv], ej(), ("kernel_version", kv, "cols_per_slice", cp))
            c.set_option("cols_per_slice", 0)
        c.set_option("kernel_version", 0)
        # Hessian kernels 1 and 2
        c.set_option("hess_kernel", 1)
        h1 = c.hess(Z, mu)
        assert c.get_option("last_hess_kernel") == 1
        check_values(lay, (None, None, h1), ref, label + "hess_kernel = 1")
        c.set_option("hess_kernel", 2)
        if vc.expected_family(name, 4)[2] == 2:
            h2 = c.hess(Z, mu)
            assert c.get_option("last_hess_kernel") == 2
            check_values(lay, (None, None, h2), ref, label + "hess_kernel = 2")
            for cp in (1, 2, 3) if cols > 1 else ():  # the scalar entries are sums over the slices: within TOL, every slicing repeatable
                c.set_option("cols_per_slice", cp)
                hs = c.hess(Z, mu)
                check_values(lay, (None, None, hs), ref, label + "hess_kernel = 2, cols_per_slice = %d" % cp)
                assert np.array_equal(hs, c.hess(Z, mu))
            c.set_option("cols_per_slice", 0)
            c.set_option("specialize", 0)  # the run-time-shape instance against the 27 / 6 one
            hr = c.hess(Z, mu)
            assert c.get_option("last_hess_kernel") == 2
            check_values(lay, (None, None, hr), ref, label + "hess_kernel = 2, specialize = 0")
            print(label + "specialize = 0 against the 27/6 instance: max |difference| %.1e" % np.abs(hr - h2).max())
            c.set_option("specialize", 1)
        else:  # dense drives: more than two entries per row
            with pytest.raises(pa.PclError) as ei:
                c.hess(Z, mu)
            assert ei.value.code == ESHAPE
    c.close()


# ---- steps of zero and long steps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["K2", "M2", "V3", "V7"])
def test_zero_and_long_steps(name):
    """Interval 0 at h = 0 (the blocks are -I and I, the tails stay finite, every segment is held to its own size), interval 2 at h |G|_2 = 2."""
    lay, G0, Gj, Z, _ = vc.case(name)
    Z = vc.with_step(lay, G0, Gj, Z, 2, 2.0)
    Z[0, lay.dt_off] = 0.0
    mu = vc.rand_mu(lay.K * lay.x_dim, name)
    ref = tuple(a.astype(np.float64).reshape(-1) for a in vc.truth_values(lay, G0, Gj, Z, mu, 10))
    c = make_ctx(lay, G0, Gj, 10)
    got, fam, d2 = run_all(c, Z, mu)
    check_values(lay, got, ref, name + " h = 0 and h |G| = 2")
    check_segments(d2, ref[0], vc.residual_labels(lay), TOL)
    jl = jac_labels(lay)
    eye = np.tile(np.eye(lay.n).reshape(-1), lay.C)
    assert np.array_equal(got[1][jl == "B+@0"], -eye) and np.array_equal(got[1][jl == "B-@0"], eye)
    c.close()


# ---- batched launches ----------------------------------------------------------------------------------------------------------------------------
def batched(which):
    """(layout, context keywords, G0, Gj, Z of the launch, per member: (truth keywords, Z, G0, x_off))"""
    if which == "members":  # K2's system, two members with their own drifts on one trajectory
        lay, _, Gj, Z, _ = vc.case("K2")
        G0s = [vc.case("K2", 0, b)[1] for b in range(2)]
        return "K2", lay, dict(x_offs=[0, 0], batch=2, per_member_G0=True), np.array(G0s), Gj, Z, [(dict(drift=b), Z, G0s[b], 0) for b in range(2)]
    if which == "traj":  # V5's system, two seeds
        lay, G0, Gj, _, _ = vc.case("V5")
        Zs = [vc.case("V5", s)[3] for s in range(2)]
        return "V5", lay, dict(batch=2, batch_mode=pa._lib.PCL_BATCH_TRAJ), G0, Gj, np.stack(Zs), [(dict(seed=s), Zs[s], G0, 0) for s in range(2)]
    lay, G0, Gj, Z, _ = vc.case("M2", 0, 0, 3)  # three states in one knot sharing one system: the multi-ket integrator's layout
    xd = lay.x_dim
    return "M2", lay, dict(x_offs=[0, xd, 2 * xd], batch=3), G0, Gj, Z, [(dict(members=3, member=i), Z, G0, i * xd) for i in range(3)]


@pytest.mark.parametrize("which", ["members", "traj", "shared"])
@pytest.mark.parametrize("order", [4, 8])
def test_batched(which, order):
    """Every member's slice against its own truth, and bitwise what a context of that member alone gives."""
    name, lay, kw, G0, Gj, Z, members = batched(which)
    c = make_ctx(lay, G0, Gj, order, **kw)
    nb = len(members)
    per_d, per_v, per_h = lay.x_dim * lay.K, po.jac_nnz_per_interval(lay) * lay.K, po.hess_nnz_per_interval(lay) * lay.K
    assert c.n_rows == nb * per_d and c.jac_nnz == nb * per_v and c.hess_nnz == nb * per_h
    truths = [vc.truth(name, order, **tk) for tk, _, _, _ in members]
    mu = np.concatenate([t[2] for t in truths])
    (delta, vals, h), fam, d2 = run_all(c, Z, mu)
    for b, (tk, Zb, G0b, xo) in enumerate(members):
        t = truths[b]
        mine = (delta[b * per_d : (b + 1) * per_d], vals[b * per_v : (b + 1) * per_v], h[b * per_h : (b + 1) * per_h])
        check_values(lay, mine, (t[0], t[1], t[3]), "%s order %d member %d" % (which, order, b))
        check_segments(d2[b * per_d : (b + 1) * per_d], t[0], vc.residual_labels(lay), TOL)
        one = make_ctx(lay, G0b, Gj, order, x_offs=[xo])
        alone, fam1, _ = run_all(one, Zb, t[2])
        assert fam1 == fam, (fam1, fam)
        bitwise(mine, alone, (which, order, b))
        one.close()
    c.close()


# ---- host paths ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["K6", "M3", "V6"])
def test_host_paths_bitwise(name):
    """Order 10: full values over the bus, compact values with the host expansion and the device-pointer call give the same bits."""
    lay, G0, Gj, Z, _ = vc.case(name)
    mu = vc.truth(name, 10)[2]
    c = make_ctx(lay, G0, Gj, 10)
    assert c.compact_nnz == (c.jac_nnz if lay.C == 1 else lay.K * (2 * lay.n * lay.n + lay.x_dim * (lay.m + 1)))
    d1, v1 = c.eval_jac(Z)
    c.set_option("host_path", 2)
    d2, v2 = c.eval_jac(Z)
    bitwise((d1, v1), (d2, v2), "host_path 1 against 2")
    bitwise((v1,), (c.jac(Z),), "the Jacobian alone")
    Zd = torch.from_numpy(np.array(Z, dtype=np.float64).reshape(-1)).cuda()
    mud = torch.from_numpy(np.array(mu)).cuda()
    dd, vd, hd = (torch.full((k,), NAN, dtype=torch.float64, device="cuda") for k in (c.n_rows, c.jac_nnz, c.hess_nnz))
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.eval_jac_dev(Zd, dd, vd)
    c.hess_dev(Zd, mud, hd)
    c.sync()
    c.set_stream(None)
    bitwise((d1, v1, c.hess(Z, mu)), (dd.cpu().numpy(), vd.cpu().numpy(), hd.cpu().numpy()), "device pointers")
    c.close()


# ---- rollout ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["K6", "M2", "V6"])
def test_rollout(name):
    lay, G0, Gj, Z, _ = vc.case(name)
    c = make_ctx(lay, G0, Gj, 10)
    X = c.rollout(Z)[0]
    assert np.array_equal(X[0], Z[0, : lay.x_dim])  # knot 0 is copied
    print("%s: rollout %s" % (name, worst(check_segments(X, vc.rollout_truth(name), vc.rollout_labels(lay), TOL))))
    c.close()


# ---- structure through the C ABI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["M2", "V5"])
@pytest.mark.parametrize("index_base", [0, 1])
def test_structure_through_the_abi(name, index_base):
    """pcl_jac_structure / pcl_hess_structure (and the 64-bit entries) equal po.jac_structure / po.hess_structure.  (A context needs a device:
    this is why the comparison is not in the CPU file.)"""
    lay, G0, Gj, Z, _ = vc.case(name)
    c = make_ctx(lay, G0, Gj, 10, index_base=index_base)
    for dtype in (np.int32, np.int64):
        bitwise(c.jac_structure(dtype), po.jac_structure(lay, index_base=index_base), "Jacobian structure")
        bitwise(c.hess_structure(dtype), po.hess_structure(lay, index_base=index_base), "Hessian structure")
    c.close()


# ---- a six-level density matrix through the integrator ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [4, 10])
def test_six_level_density_through_the_integrator(order):
    """OpenQuantumSystem at levels = 6 (n = 36, a general real generator that is not iso(-iH)) through BilinearIntegrator: residual, Jacobian,
    structure and the Hessian of the Lagrangian -- at order 10 as well -- against the longdouble truth."""
    levels, m, N = 6, 2, 4
    rng = np.random.default_rng(600 + order)
    H = rng.standard_normal((levels, levels)) + 1j * rng.standard_normal((levels, levels))
    H = 0.5 * (H + H.conj().T)
    Hs = [(lambda A: A + A.conj().T)(rng.standard_normal((levels, levels)) + 1j * rng.standard_normal((levels, levels))) for _ in range(m)]
    Ls = [0.3 * pa.annihilate(levels), 0.1 * np.diag(np.arange(levels)).astype(complex)]
    sys_ = pa.OpenQuantumSystem(H, Hs, [1.0] * m, Ls)
    G0, Gj = po.compact_lindbladian_generators(H, Hs, Ls)
    Gj = np.array(Gj)
    n2 = levels * levels
    psi = rng.standard_normal(levels) + 1j * rng.standard_normal(levels)
    psi /= np.linalg.norm(psi)
    rho0 = np.outer(psi, psi.conj())
    times = np.cumsum(np.concatenate(([0.0], 0.02 + 0.02 * rng.random(N - 1))))
    traj = pa.density_trajectory(sys_, 0.5 * rng.standard_normal((m, N)), times, rho0, rho0)
    Z = traj.datavec.reshape(N, traj.dim).copy()
    Z[1:, :n2] += 0.05 * rng.standard_normal((N - 1, n2))  # an infeasible iterate: residuals of the states' size
    traj.update(Z.reshape(-1))
    lay = po.Layout(d=0, m=m, N=N, z_dim=traj.dim, x_off=0, u_off=traj.components["u"].start, dt_off=traj.components["Δt"].start, cols=1, gen=n2)
    B = pa.BilinearIntegrator(sys_, traj, pade_order=order)
    assert B.x_dim == n2 and B.dim == n2 * (N - 1)
    mu = rng.standard_normal(lay.K * lay.x_dim)
    ref = tuple(a.astype(np.float64).reshape(-1) for a in vc.truth_values(lay, G0, Gj, Z, mu, order))
    got, fam, d2 = run_all(B.ctx, traj.datavec, mu)
    q = order // 2
    # (the integrator passes an even density size as d = n / 2 with one column -- PCL_STATE_VECTOR is for odd sizes -- so order 4 takes the fused
    #  kernel, number 20 at d = 18, and Hessian kernel 1 on the general real generator; the other orders the lock-step kernel)
    assert fam == ((20, 20, 1) if order == 4 else (190 + q, 90 + q, 90 + q)), fam
    check_values(lay, got, ref, "six-level density, order %d" % order)
    check_segments(d2, ref[0], vc.residual_labels(lay), TOL)
    bitwise(pa.jacobian_structure(B), po.jac_structure(lay), "Jacobian structure")
    bitwise(pa.hessian_structure(B), po.hess_structure(lay), "Hessian structure")
    B.close()
