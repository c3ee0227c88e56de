"""GPU tests of the plain contexts at Pade orders 2, 6, 8 and 10 on general system shapes (tests/shape_cases.py): random sparse iso
systems that straddle the pattern-compiled kernels' limits (kV4MaxCf, kMaxMags, resident / streamed drift classes, d = 9 .. 32, the
union pattern's size) and the shapes that fall back (more than 6 drives, dense non-iso generators, d = 8).  Every value against the
oracle per segment (a small segment is held to its own size), the family `auto` ran, every family and work split a case admits forced
(the same bits within a family), refusals of the families it does not admit, steps of zero and large steps, launch invariance,
per-member drifts, a knot with the controls before the state, and the order policy of the default constructor."""
import math

import numpy as np
import pytest

import piccolo_jl_amd as pa
from oracle import pade_oracle as po
from shape_cases import (PLAIN_CASES, assert_sensitive, check_segments, controlled_hermitians, g_norm, hess_labels, jac_labels, lower_order,
                         plain_case)  # fmt: skip

pytestmark = pytest.mark.gpu
TOL = 1e-11
ESHAPE = pa._lib.PCL_ESHAPE
PATTERN = ("S1", "S2", "S3", "S4", "S5", "S6")  # iso, 9 <= d <= 32, m <= 6, within kV4MaxCf / kMaxMags / the union pattern's size
FALLBACK = ("F1", "F2", "F3", "F4a", "F4b", "F5", "F6")


def make_ctx(lay, G0, Gj, x_offs=None, **kw):
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=x_offs or [lay.x_off], G0=G0,
                Gj=Gj, batch=1, batch_mode=pa._lib.PCL_BATCH_MEMBERS)  # fmt: skip
    host_path = kw.pop("host_path", 1)
    args.update(kw)
    c = pa.integrators._PclContext(**args)
    c.set_option("host_path", host_path)
    c.set_option("require_jit", 1)  # a pattern-compiled kernel that cannot be built is an error, not a fallback
    return c


def expected_family(name, order, c):
    """(eval_jac last_kernel, eval last_kernel, last_hess_kernel) `auto` runs at order 2q != 4.
    Kernel 4 family (40 + q fused, 80 + q residual, 80 + q column-group Hessian, 70 + q where the latter's table does not take the
    magnitudes) where the generator and the LDS take the system; d = 32 with
    six drives has no LDS for kernel 4's tiles (lock-step 190 + q) and falls through to the general-order Hessian (90 + q).  Elsewhere:
    the lock-step kernel (even n <= 64) for the residual and Jacobian, the reference formulation (90 + q) for the residual alone, the
    small-system kernel (50 + q) for the residual alone of n <= 16 rows."""
    q = order // 2
    if name == "S2":  # 8 distinct drive magnitudes: more than the column-group kernel's gathers' table holds (kHcMaxMags = 7): kernel 7
        return 40 + q, 80 + q, 70 + q
    if name in ("S1", "S3", "S4", "S5"):
        return 40 + q, 80 + q, 80 + q
    if name == "F5":
        return 190 + q, 50 + q, 90 + q
    return 190 + q, 90 + q, 90 + q


def oracle(lay, G0, Gj, Z, mu, order, x_off=None):
    return (po.pade_residual(Z, lay, G0, Gj, order, x_off).reshape(-1), po.pade_jacobian_values(Z, lay, G0, Gj, order, x_off).reshape(-1),
            po.pade_hessian_values(Z, mu, lay, G0, Gj, order, x_off).reshape(-1))  # fmt: skip


def check_values(lay, got, ref, tol=TOL):
    check_segments(got[0], ref[0], np.full(ref[0].size, "delta"), tol)
    check_segments(got[1], ref[1], jac_labels(lay), tol)
    check_segments(got[2], ref[2], hess_labels(lay), tol)


def run_all(c, Z, mu):
    delta, vals = c.eval_jac(Z)
    kj = c.get_option("last_kernel")
    d2 = c.eval(Z)
    ke = c.get_option("last_kernel")
    h = c.hess(Z, mu.reshape(-1))
    kh = c.get_option("last_hess_kernel")
    return (delta, vals, h), (kj, ke, kh), d2


@pytest.mark.parametrize("name,order", [(n, o) for n in PATTERN + FALLBACK for o in (2, 6, 8, 10)])
def test_auto_against_oracle_per_segment(name, order):
    lay, G0, Gj, Z = plain_case(name)
    mu = np.random.default_rng(order).standard_normal((lay.K, lay.x_dim))
    ref = oracle(lay, G0, Gj, Z, mu, order)
    lo = oracle(lay, G0, Gj, Z, mu, lower_order(order))
    for a, b in zip(ref, lo):
        assert_sensitive(a, b, TOL)
    c = make_ctx(lay, G0, Gj, pade_order=order)
    assert c.get_option("iso_structured") == (0 if name.startswith("F4") else 1)
    got, fam, d2 = run_all(c, Z, mu)
    check_values(lay, got, ref)
    check_segments(d2, ref[0], np.full(ref[0].size, "delta"), TOL)
    assert fam == expected_family(name, order, c), (name, order, fam)
    assert np.array_equal(got[2], c.hess(Z, mu.reshape(-1)))
    c.close()


# ---- every family and work split a case admits, at order 10 (and at order 6 for S3 and S4) ------------------------------------------------
def _bitwise_family(c, Z, mu, settings, what):
    """Run `what` under every option setting; all must give the same bits.  Returns the first result, or the PclError of a refusal."""
    first = None
    for s in settings:
        for k, v in s.items():
            c.set_option(k, v)
        r = what()
        if first is None:
            first = r
        else:
            for a, b in zip(first, r):
                assert np.array_equal(a, b), (s,)
    return first


def _reset(c):
    for k, v in (("kernel_version", 0), ("eval_kernel", 0), ("general_kernel_version", 0), ("hess_kernel", 0), ("contiguous", -1), ("grid", 0),
                 ("cols_per_slice", 0), ("v4_tail_mode", 3), ("eval_coop", -1), ("general_slices", 0), ("hess_split", -1), ("hess_pair", -1),
                 ("hess_rpre", -1)):  # fmt: skip
        c.set_option(k, v)


def _refused(fn):
    with pytest.raises(pa.PclError) as ei:
        fn()
    assert ei.value.code == ESHAPE, (ei.value.code, str(ei.value))


def force_families(name, order, lay, G0, Gj, Z, mu, ref):
    q = order // 2
    c = make_ctx(lay, G0, Gj, pade_order=order)
    ej = lambda: c.eval_jac(Z)
    ev = lambda: (c.eval(Z),)
    hs = lambda: (c.hess(Z, mu.reshape(-1)),)
    v4 = name in ("S1", "S2", "S3", "S4", "S5")
    cols = v4 and name != "S2"  # (S2: 8 drive magnitudes, kernel 8 refuses them)
    dlabels = np.full(ref[0].size, "delta")
    results = {}
    # kernel 4: column splits, grids, tail modes
    c.set_option("kernel_version", 4)
    if v4:
        splits = [dict(contiguous=cn, grid=g, cols_per_slice=cp, v4_tail_mode=tm) for cn, g, cp, tm in
                  ((-1, 0, 0, 3), (0, 0, 5, 3), (1, 3, 0, 3), (1, 1000, 0, 0), (0, 1, 7, 0))]  # fmt: skip
        results["k4"] = _bitwise_family(c, Z, mu, splits, ej)
        assert c.get_option("last_kernel") == 40 + q
        check_values(lay, (results["k4"][0], results["k4"][1], ref[2]), ref)
    else:
        _refused(ej)
    _reset(c)
    # the pattern-compiled residual kernel, one and four waves per interval (one wave per interval holds 12 tiles: from d = 29 on they do
    # not fit the LDS, and forcing it is refused)
    c.set_option("eval_kernel", 3)
    if v4:
        coops = (0, 1) if lay.d < 29 else (1,)
        first = None
        for e in coops:
            c.set_option("eval_coop", e)
            r = c.eval(Z)
            # (streamed drift classes -- S3 -- have no cooperative kernel: SP4_COOP 0 in the source, one wave per interval whatever is asked)
            assert c.get_option("last_kernel") == 80 + q and c.get_option("last_eval_coop") == (0 if name == "S3" else e)
            if first is None:
                first = r
                check_segments(r, ref[0], dlabels, TOL)
            assert np.array_equal(r, first)
        if lay.d >= 29:
            c.set_option("eval_coop", 0)
            with pytest.raises(pa.PclError) as ei:
                c.eval(Z)
            assert ei.value.code == ESHAPE and "LDS" in str(ei.value), str(ei.value)
            c.set_option("eval_coop", -1)
            assert np.array_equal(c.eval(Z), first)  # (nothing launched: the context goes on)
        results["e3"] = (first,)
    else:
        _refused(ev)
    _reset(c)
    # the general-order kernels: reference formulation and lock-step, several slicings
    for gv in (1, 2):
        c.set_option("general_kernel_version", gv)
        results["g%d" % gv] = _bitwise_family(c, Z, mu, [dict(general_slices=s) for s in (0, 1, 3)], ej)
        assert c.get_option("last_kernel") == (90 if gv == 1 else 190) + q
        check_values(lay, (results["g%d" % gv][0], results["g%d" % gv][1], ref[2]), ref)
    _reset(c)
    hlabels = hess_labels(lay)
    # the pattern-compiled Hessian kernels
    c.set_option("hess_kernel", 7)
    if v4:
        first = None
        for split in (0, 1):
            c.set_option("hess_split", split)
            h = hs()[0]
            assert c.get_option("last_hess_kernel") == 70 + q and c.get_option("last_hess_split") == (split if lay.m >= 2 else 0)
            if first is None:
                first = h
                check_segments(h, ref[2], hlabels, TOL)
            assert np.array_equal(h, first)
        results["h7"] = (first,)
    else:
        _refused(hs)
    c.set_option("hess_split", -1)
    c.set_option("hess_kernel", 8)
    if cols:
        # (the pair kernel addresses its LDS with 16-bit offsets: d = 32 from order 8 on runs one wave per column group whatever is asked)
        pair_ok = not (lay.d == 32 and q >= 4)
        first = None
        for pair in (0, 1):
            c.set_option("hess_rpre", 0)
            c.set_option("hess_pair", pair)
            h = hs()[0]
            assert c.get_option("last_hess_kernel") == 80 + q and c.get_option("last_hess_pair") == (pair if pair_ok else 0)
            if first is None:
                first = h
                check_segments(h, ref[2], hlabels, TOL)
            assert np.array_equal(h, first)
        results["h8"] = (first,)
        c.set_option("hess_rpre", 1)
        c.set_option("hess_pair", 0)
        h1 = hs()[0]
        assert c.get_option("last_hess_kernel") == 80 + q
        check_segments(h1, ref[2], hlabels, TOL)
        if c.get_option("last_hess_rpre") == 1:  # (u,u) scalars: the documented last-bit difference of the R-chain waves
            nuu = lay.m * (lay.m + 1) // 2
            per = po.hess_nnz_per_interval(lay)
            uu = (np.arange(h1.size) % per) < nuu
            assert np.array_equal(h1[~uu], first[~uu])
            assert np.abs(h1[uu] - first[uu]).max() <= 1e-13 * np.abs(first[uu]).max()
        else:  # (no R-chain waves where their tiles do not fit: the same kernel as above)
            assert np.array_equal(h1, first)
        # across families: 1e-13 where the existing tests assert it (kernel 8 against kernel 7)
        assert np.abs(first - results["h7"][0]).max() <= 1e-13 * np.abs(results["h7"][0]).max()
    else:
        _refused(hs)
    _reset(c)
    # compact values + host expansion against full values
    c.set_option("host_path", 2)
    d2, v2 = c.eval_jac(Z)
    c.set_option("host_path", 1)
    d1, v1 = c.eval_jac(Z)
    assert np.array_equal(d1, d2) and np.array_equal(v1, v2)
    c.close()
    return results


@pytest.mark.parametrize("name,order", [(n, 10) for n in PATTERN + FALLBACK] + [("S3", 6), ("S4", 6)])
def test_forced_families_and_work_splits(name, order):
    lay, G0, Gj, Z = plain_case(name)
    mu = np.random.default_rng(order + 1).standard_normal((lay.K, lay.x_dim))
    force_families(name, order, lay, G0, Gj, Z, mu, oracle(lay, G0, Gj, Z, mu, order))


# ---- steps of zero and large steps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S1", "S4", "S6", "F4a"])
def test_zero_and_large_timesteps(name):
    """One interval with Delta t = 0 exactly, one with h |G(u)|_2 = 2: every family gives finite values equal to the oracle (whose formulas
    are polynomial in h).  Kernel 7 formed h^(j-2) as h^(j-1) / h: 0 / 0 in the (h,h) entry at a step of zero."""
    lay, G0, Gj, Z = plain_case(name, N=5, seed=1)
    Z[1, lay.dt_off] = 0.0
    Z[2, lay.dt_off] = 2.0 / g_norm(lay, Z, 2, G0, Gj)
    mu = np.random.default_rng(3).standard_normal((lay.K, lay.x_dim))
    for order in (6, 10):
        ref = oracle(lay, G0, Gj, Z, mu, order)
        assert np.all(np.isfinite(ref[2]))
        assert ref[2].reshape(lay.K, -1)[1, lay.m * (lay.m + 1) // 2 + lay.m] != 0.0  # (h,h) at h = 0: 2 c_2 <W_2, Y_2>
        c = make_ctx(lay, G0, Gj, pade_order=order)
        got, fam, d2 = run_all(c, Z, mu)
        check_values(lay, got, ref)
        c.close()
        force_families(name, order, lay, G0, Gj, Z, mu, ref)


# ---- launch invariance ----------------------------------------------------------------------------------------------------------------------
def test_batch_of_seeds_equals_single_launches():
    """S4 at order 10: a PCL_BATCH_TRAJ launch of 3 seeds and each seed alone give the same bits (delta, J, and the Hessian with the R-chain
    waves forced in both: hess_rpre 1)."""
    order = 10
    lay, G0, Gj, Z0 = plain_case("S4")
    Zs = [plain_case("S4", seed=s)[3] for s in range(3)]
    mus = np.random.default_rng(12).standard_normal((3, lay.K, lay.x_dim))
    cb = make_ctx(lay, G0, Gj, pade_order=order, batch=3, batch_mode=pa._lib.PCL_BATCH_TRAJ)
    c1 = make_ctx(lay, G0, Gj, pade_order=order)
    db, vb = cb.eval_jac(np.stack(Zs))
    db, vb = db.reshape(3, -1), vb.reshape(3, -1)
    assert cb.get_option("last_kernel") == 40 + order // 2
    per = po.hess_nnz_per_interval(lay) * lay.K
    nuu = lay.m * (lay.m + 1) // 2
    uu = (np.arange(per) % po.hess_nnz_per_interval(lay)) < nuu
    for rpre in (-1, 1):
        cb.set_option("hess_rpre", rpre)
        c1.set_option("hess_rpre", rpre)
        hb = cb.hess(np.stack(Zs), mus.reshape(-1)).reshape(3, -1)
        rb = cb.get_option("last_hess_rpre")
        for i in range(3):
            d1, v1 = c1.eval_jac(Zs[i])
            assert np.array_equal(d1, db[i]) and np.array_equal(v1, vb[i])
            h1 = c1.hess(Zs[i], mus[i].reshape(-1))
            if c1.get_option("last_hess_rpre") == rb:
                assert np.array_equal(h1, hb[i])
            else:
                assert np.array_equal(h1[~uu], hb[i][~uu])
                assert np.abs(h1[uu] - hb[i][uu]).max() <= 1e-13 * np.abs(hb[i][uu]).max()
            check_segments(h1, po.pade_hessian_values(Zs[i], mus[i], lay, G0, Gj, order).reshape(-1), hess_labels(lay), TOL)
    cb.close()
    c1.close()


@pytest.mark.parametrize("order", [6, 10])
def test_large_residual_launch_at_d32(order):
    """`eval` of more intervals than 2 n_cu at d = 32 (S5): `auto` would take one wave per interval, whose 12 tiles do not fit the LDS
    there -- it runs the cooperative kernel, against the oracle; forcing one wave per interval is refused before any launch."""
    lay0, G0, Gj, _ = plain_case("S5")
    c0 = make_ctx(lay0, G0, Gj)
    n_cu = c0.get_option("n_cu")
    c0.close()
    N = 40
    lay = po.Layout(d=lay0.d, m=lay0.m, N=N, z_dim=lay0.z_dim, x_off=0, u_off=lay0.u_off, dt_off=lay0.dt_off)
    B = (2 * n_cu) // lay.K + 1
    assert B * lay.K > 2 * n_cu
    rng = np.random.default_rng(77)
    Zs = np.stack([0.4 * rng.standard_normal((N, lay.z_dim)) for _ in range(B)])
    for Z in Zs:
        for k in range(lay.K):
            Z[k, lay.dt_off] = (0.15 + 0.3 * rng.random()) / g_norm(lay, Z, k, G0, Gj)
    c = make_ctx(lay, G0, Gj, pade_order=order, batch=B, batch_mode=pa._lib.PCL_BATCH_TRAJ)
    d = c.eval(Zs).reshape(B, -1)
    assert c.get_option("last_kernel") == 80 + order // 2 and c.get_option("last_eval_coop") == 1
    for i in range(0, B, max(1, B // 6)):
        check_segments(d[i], po.pade_residual(Zs[i], lay, G0, Gj, order).reshape(-1), np.full(d[i].size, "delta"), TOL)
    c.set_option("eval_coop", 0)
    with pytest.raises(pa.PclError) as ei:
        c.eval(Zs)
    assert ei.value.code == ESHAPE and "LDS" in str(ei.value)
    c.set_option("eval_coop", -1)
    assert np.array_equal(c.eval(Zs).reshape(B, -1), d)
    c.close()


# ---- per-member drifts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [8, 10])
def test_per_member_drifts_streamed_classes(order):
    """S3's pattern with three members' drift values perturbed (the same pattern, streamed value classes), member-major rows."""
    H0, Hd = controlled_hermitians(20, [[0, 1], [2], [0, 3]], np.random.default_rng(7003), "continuous")
    Gj = np.array([po.G_of_H(H) for H in Hd])
    rng = np.random.default_rng(33)
    G0s = []
    for _ in range(3):
        R = 1 + 0.05 * rng.standard_normal(H0.shape)
        G0s.append(po.G_of_H(H0 * (R + R.T) / 2))  # the same pattern, every member's values its own
    d, m, N = 20, 3, 4
    xd = 2 * d * d
    lay = po.Layout(d=d, m=m, N=N, z_dim=3 * xd + 2 + m, x_off=0, u_off=3 * xd + 2, dt_off=3 * xd)
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    for k in range(N - 1):
        Z[k, lay.dt_off] = 0.3 / g_norm(lay, Z, k, G0s[0], Gj)
    mu = rng.standard_normal((3, lay.K, xd))
    c = make_ctx(lay, np.array(G0s), Gj, x_offs=[0, xd, 2 * xd], pade_order=order, batch=3, per_member_G0=True)
    got, fam, d2 = run_all(c, Z, mu)
    q = order // 2
    assert fam == (40 + q, 80 + q, 80 + q), fam
    per_d, per_j, per_h = lay.K * xd, po.jac_nnz_per_interval(lay) * lay.K, po.hess_nnz_per_interval(lay) * lay.K
    for i in range(3):
        ref = oracle(lay, G0s[i], Gj, Z, mu[i], order, x_off=i * xd)
        mine = (got[0][i * per_d : (i + 1) * per_d], got[1][i * per_j : (i + 1) * per_j], got[2][i * per_h : (i + 1) * per_h])
        check_values(lay, mine, ref)
        check_segments(d2[i * per_d : (i + 1) * per_d], ref[0], np.full(per_d, "delta"), TOL)
    c.close()


# ---- layout: controls and Delta t before the state -------------------------------------------------------------------------------------------
def test_controls_before_the_state_and_index_base():
    order = 10
    G0, Gj = plain_case("S5")[1:3]
    d, m, N = 32, 2, 4
    xd = 2 * d * d
    x_off = 3 + m + 2
    lay = po.Layout(d=d, m=m, N=N, z_dim=x_off + xd + 2, x_off=x_off, u_off=1, dt_off=1 + m + 1)
    rng = np.random.default_rng(55)
    Z = 0.4 * rng.standard_normal((N, lay.z_dim))
    for k in range(N - 1):
        Z[k, lay.dt_off] = 0.3 / g_norm(lay, Z, k, G0, Gj)
    mu = rng.standard_normal((lay.K, xd))
    ref = oracle(lay, G0, Gj, Z, mu, order)
    for base in (0, 1):
        c = make_ctx(lay, G0, Gj, pade_order=order, index_base=base)
        got, fam, d2 = run_all(c, Z, mu)
        assert fam == (45, 85, 85), fam
        check_values(lay, got, ref)
        r, cc = c.jac_structure()
        r0, c0 = po.jac_structure(lay, index_base=base)
        assert np.array_equal(r, r0) and np.array_equal(cc, c0)
        r, cc = c.hess_structure()
        r0, c0 = po.hess_structure(lay, index_base=base)
        assert np.array_equal(r, r0) and np.array_equal(cc, c0)
        c.close()


# ---- the default constructor's order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S1", "F4a"])
def test_default_constructor_order(name):
    """pade_order = 0: the order the policy's rule gives for theta = 1.5 max_k |dt_k G(u_k)|_2 (as in
    test_order_policy_picks_the_order_that_matches_the_exp_constraint), and the oracle's values at that order."""
    lay, G0, Gj, Z = plain_case(name)
    theta = max(abs(Z[k, lay.dt_off]) * g_norm(lay, Z, k, G0, Gj) for k in range(lay.K))
    kappa = lambda q: math.factorial(q) ** 2 / (math.factorial(2 * q) * math.factorial(2 * q + 1))
    want = next((2 * q for q in range(1, 6) if kappa(q) * (1.5 * theta) ** (2 * q + 1) <= 1e-10), 10)
    c = make_ctx(lay, G0, Gj, pade_order=0)
    delta, vals = c.eval_jac(Z)
    assert c.pade_order == want
    mu = np.random.default_rng(2).standard_normal((lay.K, lay.x_dim))
    check_values(lay, (delta, vals, c.hess(Z, mu.reshape(-1))), oracle(lay, G0, Gj, Z, mu, want))
    c.close()
