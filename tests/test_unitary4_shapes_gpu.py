"""The order-4 kernels of the square unitary state on the device, at the sizes of tests/unitary4_cases.py (the case table and the branch each
case straddles are there), through _PclContext / the C ABI.  Every value is compared with the longdouble truth of
vector_shape_cases.truth_values, rounded to float64, at TOL = 1e-11 PER SEGMENT of every interval, relative to the segment's own maximum with
no floor at 1 (shape_cases.check_segments); a segment whose truth is identically zero (the h = 0 interval) must be exactly zero.
tests/test_unitary4_shapes_cpu.py shows that every case sits on the claimed side of its branch, that the float64 oracle agrees with that
truth to 1e-13 on these inputs and that each case sees a zeroed c_2, a dropped drive, a dropped column and a product without its last row,
column or inner index at 1e-7.

Which kernel runs is asserted against the launch rules restated in unitary4_cases (fused_family, eval_family, hess_family) with the
context's own n_cu.  Family -> cases (a: what `auto` runs, f: forced through kernel_version / eval_kernel / hess_kernel / use_mfma /
specialize / jit, b: the launch of several trajectories):
    last_kernel 10        a U2 U3 U6a U6b U9a U9b U10a U10c, b U5 (512 intervals), f every case (kernel_version 1; use_mfma 0)
    last_kernel 20        a U7b U10b U11 U12 U13 U14 U15 U16, b U5 (516 intervals) U7a, f every case (kernel_version 2)
    last_kernel 30/31/32  a U7a U8 (31), f U4 U17 U6b U7b U9a (32), U10a and U7a / U8 with specialize 0 (30)
    last_kernel 42        a U4 U17, b U4
    last_kernel 52        a U1 (eval_jac and eval) U2 U3 (eval), f U2 U3 (kernel_version 5)
    last_kernel 60/61     a every case from d = 9 on without kernel 4 (eval), f U4 U17 (eval_kernel 1)
    last_kernel 70        f U4 U17 U14 U15 (eval_kernel 2), b U4
    last_kernel 82        a U4 U17 (eval), b U4
    last_hess_kernel 1    a U3 U9b U10a U10b U13, f every case (hess_kernel 1; use_mfma 0)
    last_hess_kernel 2/3  a U1 U2 U5 U6a (2) U10c U12 U15 (3), f U4 U6b U9a U17 (hess_kernel 2: 2 below d = 12, 3 from there), with
                          specialize 0 every case they take (2)
    last_hess_kernel 4/5  a U8 (4) U6b U7a U7b U9a U11 U16 (5), f U4 U17 U6a (hess_kernel 3)
    last_hess_kernel 6    a U14, f U4 U17 (hess_kernel 4), b U4 (515 intervals: the rule of `auto` flips from 82 to 6)
    last_hess_kernel 72   f U4 U17 (hess_kernel 7)
    last_hess_kernel 82   a U4 U17
Families a case does not admit are asserted refused with PCL_ESHAPE.

Largest relative error read per segment kind on an MI355X (256 CUs), over every case, family and work split of this module:
    delta 2.8e-16   B+- 2.2e-16   du 5.0e-16   dh 7.0e-16   uu 1.5e-13   hu 1.1e-13   hh 1.7e-13   X rows 7.7e-16"""
import numpy as np
import pytest
import torch

import piccolo_jl_amd as pa
import unitary4_cases as uc
from oracle import pade_oracle as po
from shape_cases import check_segments

pytestmark = pytest.mark.gpu
TOL = 1e-11
ESHAPE = pa._lib.PCL_ESHAPE
NAMES = list(uc.CASES)
NAN = float("nan")
K3 = ("U4", "U17", "U6b", "U7a", "U7b", "U8", "U9a", "U10a", "U11", "U13")  # kernel_version 3 is forced here (an instance is compiled where none is built in)
H3 = ("U4", "U17", "U6a")  # hess_kernel 3 where `auto` does not run it already
H2 = ("U4", "U17", "U6b", "U9a")  # hess_kernel 2 with the instance compiled on first use; elsewhere with specialize 0
_read = {}


def make_ctx(name, n_knots=uc.N, seeds=0, **kw):
    """seeds > 0: a PCL_BATCH_TRAJ context of that many trajectories."""
    lay, (G0, Gj) = uc.layout(name, n_knots), uc.system(name)
    M = uc.MEMBERS.get(name, 1)
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=uc.x_offs(name), G0=G0, Gj=Gj, batch=M,
                batch_mode=pa._lib.PCL_BATCH_MEMBERS, per_member_G0=name in uc.MEMBERS, pade_order=4, state_cols=0)  # fmt: skip
    if seeds:
        args.update(batch=seeds, batch_mode=pa._lib.PCL_BATCH_TRAJ)
    args.update(kw)
    c = pa.integrators._PclContext(**args)
    c.set_option("host_path", 1)
    c.set_option("require_jit", 1)  # a pattern-compiled kernel that cannot be built is an error, not a fallback
    return c


def note(errs):
    """Keep the largest relative error per segment kind (printed by every test: the table of DESIGN.md 4.5.1)."""
    for s, v in errs.items():
        k = s.split("@")[0]
        kind = k if k in ("delta", "du", "dh", "uu", "hu", "hh") else "B+-" if k in ("B+", "B-") else "X rows"
        _read[kind] = max(_read.get(kind, 0.0), v)


def check(name, got, what, n_knots=uc.N, seed=0, ref=None):
    """got: (delta | None, values | None, Hessian values | None) of every member of the launch, against each member's truth."""
    lay = uc.layout(name, n_knots)
    M = uc.MEMBERS.get(name, 1)
    out = []
    for g, lab, kind, i in zip(got, uc.labels(lay), ("residual", "Jacobian", "Hessian"), (0, 1, 3)):
        if g is None:
            continue
        per = g.size // M
        worst = {}
        for b in range(M):
            r = (ref if ref is not None else uc.truth(name, seed, n_knots, b))[i]
            try:
                e = check_segments(g[b * per : (b + 1) * per], r, lab, TOL)
            except AssertionError as err:
                raise AssertionError("%s, %s, member %d, %s: %s" % (name, what, b, kind, err)) from None
            note(e)
            worst.update({k: max(v, worst.get(k, 0.0)) for k, v in e.items()})
        s = max(worst, key=worst.get)
        out.append("%s %.1e (%s)" % (kind, worst[s], s))
    print("%s, %s: %s" % (name, what, "  ".join(out)))


def mu_of(name, n_knots=uc.N, seed=0):
    return np.concatenate([uc.rand_mu(name, seed, n_knots, b) for b in range(uc.MEMBERS.get(name, 1))])


def bitwise(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


def refused(fn, *words):
    with pytest.raises(pa.PclError) as ei:
        fn()
    assert ei.value.code == ESHAPE, (ei.value.code, str(ei.value))
    for w in words:
        assert w in str(ei.value), str(ei.value)


def _set(c, **opts):
    for k, v in opts.items():
        c.set_option(k, v)


def _reset(c):
    _set(c, kernel_version=0, eval_kernel=0, hess_kernel=0, use_mfma=1, specialize=1, jit=1, contiguous=-1, stream_workgroups=-1, grid=0,
         cols_per_slice=0, v4_tail_mode=3, eval_coop=-1, hess_split=-1, hess_pair=-1)  # fmt: skip


def family(c, fn, splits, want, key="last_kernel"):
    """fn() under every work split: the kernel `want` each time (a tuple: one of them), the same bits, and the same bits in a second launch.
    Returns the first result."""
    first = None
    for s in splits:
        _set(c, **s)
        for rep in range(2 if first is None else 1):
            r = fn()
            k = c.get_option(key)
            assert k in want if isinstance(want, tuple) else k == want, (s, k, want)
            if first is None:
                first = r
            bitwise(first, r, (want, s, rep))
    _set(c, **{k: (-1 if k in ("contiguous", "stream_workgroups", "hess_split", "hess_pair", "eval_coop") else 3 if k == "v4_tail_mode" else 0) for s in splits for k in s})
    return first


GRIDS = [dict(grid=g) for g in (0, 1, 3, 1000)]


def teardown_module(module):
    print("largest relative error per segment kind: " + "   ".join("%s %.1e" % (k, _read[k]) for k in ("delta", "B+-", "du", "dh", "uu", "hu", "hh", "X rows") if k in _read))


# ---- what `auto` runs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_auto_per_segment(name):
    p, lay = uc.props(name), uc.layout(name)
    M = uc.MEMBERS.get(name, 1)
    Z, mu = uc.trajectory(name), mu_of(name)
    c = make_ctx(name)
    n_cu, items = c.get_option("n_cu"), M * lay.K
    assert c.n_rows == M * lay.K * lay.x_dim and c.jac_nnz == M * lay.K * po.jac_nnz_per_interval(lay) and c.hess_nnz == M * lay.K * po.hess_nnz_per_interval(lay)
    assert (c.get_option("iso_structured"), c.get_option("drives_antisymmetric"), c.get_option("ell_width"), c.get_option("ell_width_t"), c.get_option("union_width")) == \
        (int(p["iso"]), int(p["anti"]), p["ell_w"], p["ellt_w"], p["uell_w"])  # fmt: skip
    delta, vals = c.eval_jac(Z)
    kj = c.get_option("last_kernel")
    d2 = c.eval(Z)
    ke = c.get_option("last_kernel")
    h = c.hess(Z, mu)
    fam = (kj, ke, c.get_option("last_hess_kernel"))
    print("%s ran eval_jac %d, eval %d, hess %d" % ((name,) + fam))
    check(name, (delta, vals, h), "auto %d/%d/%d" % fam)
    check(name, (d2, None, None), "auto, eval alone")
    assert fam == (uc.fused_family(p, items), uc.eval_family(p, items, n_cu), uc.hess_family(p, items, n_cu)), (name, fam)
    bitwise((vals, h, delta), (c.jac(Z), c.hess(Z, mu), c.eval_jac(Z)[0]), "jac alone, a second Hessian launch, a second eval_jac")
    c.close()


# ---- every family a case admits, and its work splits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forced_families(name):
    """Each family against the truth; within a family the same bits whatever the work split, and in a second launch."""
    p, lay = uc.props(name), uc.layout(name)
    M, d = uc.MEMBERS.get(name, 1), lay.d
    Z, mu = uc.trajectory(name), mu_of(name)
    c = make_ctx(name)
    n_cu, items = c.get_option("n_cu"), M * lay.K
    ej, ev, hs = (lambda: c.eval_jac(Z)), (lambda: (c.eval(Z),)), (lambda: (c.hess(Z, mu),))
    cps = [dict(cols_per_slice=v) for v in (0, 1, 3, d)]
    ran = []

    def fused(want, splits, **opts):
        _set(c, **opts)
        if want == "ESHAPE":
            refused(ej)
        else:
            r = family(c, ej, splits, want)
            check(name, r + (None,), "eval_jac %s -> %s" % (opts, want))
            ran.append(c.get_option("last_kernel"))
        _reset(c)

    def resid(want, splits, **opts):
        _set(c, **opts)
        if want == "ESHAPE":
            refused(ev)
        else:
            r = family(c, ev, splits, want)
            check(name, r + (None, None), "eval %s -> %s" % (opts, want))
            ran.append(c.get_option("last_kernel"))
        _reset(c)

    def hess(want, splits, *words, **opts):
        _set(c, **opts)
        if want == "ESHAPE":
            refused(hs, *words)
        else:
            r = family(c, hs, splits, want, "last_hess_kernel")
            check(name, (None, None) + r, "hess %s -> %s" % (opts, want))
            ran.append(100 + c.get_option("last_hess_kernel"))
        _reset(c)

    # residual + Jacobian: kernels 10 and 20 (column slices, the persistent grid), the small kernel, kernel 4, without the matrix cores
    fused(10, cps, kernel_version=1)
    fused(20, cps + GRIDS[1:], kernel_version=2)
    fused(uc.fused_family(p, items, use_mfma=0), cps[:2], use_mfma=0)
    fused(uc.fused_family(p, items, kernel_version=5), GRIDS, kernel_version=5)
    v4_splits = [dict(contiguous=cn, grid=g, cols_per_slice=cp, v4_tail_mode=tm) for cn, g, cp, tm in ((-1, 0, 0, 3), (0, 0, 5, 3), (1, 3, 0, 3), (1, 1000, 0, 0), (0, 1, 7, 0))]
    fused(uc.fused_family(p, items, kernel_version=4), v4_splits, kernel_version=4)
    if p["sp"]:
        fused(uc.fused_family(p, items, jit=0), cps[:1], jit=0)
    if name in K3:
        # kernel 3: round-robin slices, contiguous ranges, the role split (slices of at least 16 / (2 + m) columns: one chunk width, one instance)
        want = uc.fused_family(p, items, kernel_version=3)
        w = max(2, 16 // (2 + lay.m))
        k3 = [dict(contiguous=0, cols_per_slice=w), dict(contiguous=0, cols_per_slice=d, grid=3), dict(contiguous=1, cols_per_slice=0, stream_workgroups=0, grid=0),
              dict(contiguous=1, stream_workgroups=0, grid=1), dict(contiguous=1, stream_workgroups=1, grid=3), dict(contiguous=1, stream_workgroups=2, grid=1000)]  # fmt: skip
        fused(want, (k3 if want != 20 else cps), kernel_version=3)
        if want == 31:  # the run-time-shape instance behind the built-in one
            fused(30, k3[:3], kernel_version=3, specialize=0)
            fused(uc.fused_family(p, items, specialize=0), cps[:1], specialize=0)
    # residual alone
    resid(10, cps[:2], kernel_version=1)
    resid(20, GRIDS, kernel_version=2)
    resid(uc.eval_family(p, items, n_cu, eval_kernel=1), GRIDS, eval_kernel=1)
    resid(uc.eval_family(p, items, n_cu, eval_kernel=2), GRIDS, eval_kernel=2)
    coop = [dict(eval_coop=e, grid=g) for e in (0, 1) for g in (0, 3)]
    resid(uc.eval_family(p, items, n_cu, eval_kernel=3), coop, eval_kernel=3)
    if uc.small_kernel(p, False):
        resid(52, GRIDS, kernel_version=5)
    # the Hessian of the Lagrangian
    hess(1, [dict()], hess_kernel=1)
    hess(uc.hess_family(p, items, n_cu, use_mfma=0, jit=0), [dict()], use_mfma=0, jit=0)
    want2 = uc.hess_family(p, items, n_cu, hess_kernel=2, specialize=0)
    if want2 == "ESHAPE":
        hess("ESHAPE", None, "widths %d/%d" % (p["ell_w"], p["ellt_w"]), hess_kernel=2)
    else:
        assert want2 == 2
        hess(2, GRIDS, hess_kernel=2, specialize=0)
        if name in H2:
            hess(uc.hess_family(p, items, n_cu, hess_kernel=2), GRIDS, hess_kernel=2)
        # column slices: the scalar entries are sums of the slices' partial sums -- against the truth, and repeatable
        for cp in (1, 5):
            _set(c, hess_kernel=2, specialize=0, cols_per_slice=cp)
            r = hs()
            check(name, (None, None) + r, "hess_kernel 2, cols_per_slice %d" % cp)
            bitwise(r, hs(), ("hess_kernel 2, cols_per_slice", cp))
            _reset(c)
    if name in H3:
        hess(uc.hess_family(p, items, n_cu, hess_kernel=3), GRIDS, hess_kernel=3)
    auto_h = uc.hess_family(p, items, n_cu)
    if auto_h in (4, 5, 6):
        hess(auto_h, GRIDS)
    if auto_h == 4:
        hess(uc.hess_family(p, items, n_cu, specialize=0), GRIDS, specialize=0)
    want4 = uc.hess_family(p, items, n_cu, hess_kernel=4)
    hess(want4, GRIDS, *(("%d B" % uc.hess_sparse_lds_bytes(p), "%d available" % uc.LDS_BYTES) if p["sp"] and want4 == "ESHAPE" else ()), hess_kernel=4)
    hess(uc.hess_family(p, items, n_cu, hess_kernel=7), [dict(hess_split=s, grid=g) for s in (0, 1) for g in (0, 3)], hess_kernel=7)
    hess(uc.hess_family(p, items, n_cu, hess_kernel=8), [dict(hess_pair=0), dict(hess_pair=1)], hess_kernel=8)
    if p["sp"]:
        hess(uc.hess_family(p, items, n_cu, jit=0), GRIDS, jit=0)
    print("%s ran %s" % (name, sorted(set(ran))))
    c.close()


# ---- controls back and forth ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["U4", "U8", "U14", "U17"])
def test_controls_back_and_forth(name):
    """One context: u, then -1.7 u, then u again, each against its own truth (the pattern-compiled kernels read their value tables through the
    scalar cache; the static instances keep G(u) in LDS across the intervals a workgroup walks)."""
    Z0, Z1, mu = uc.trajectory(name), uc.flipped(name), uc.rand_mu(name)
    c = make_ctx(name)
    runs = []
    for Z, ref, what in ((Z0, None, "u"), (Z1, uc.flipped_truth(name), "-1.7 u"), (Z0, None, "u again")):
        delta, vals = c.eval_jac(Z)
        d2 = c.eval(Z)
        h = c.hess(Z, mu)
        check(name, (delta, vals, h), what, ref=ref)
        check(name, (d2, None, None), what + ", eval alone", ref=ref)
        runs.append((delta, vals, d2, h))
    bitwise(runs[0], runs[2], "u and u again")
    if uc.props(name)["sp"]:  # the pattern-compiled kernels that `auto` does not run here
        for opts in (dict(hess_kernel=4), dict(eval_kernel=2)):
            _set(c, **opts)
            for Z, ref, what in ((Z0, None, "u"), (Z1, uc.flipped_truth(name), "-1.7 u"), (Z0, None, "u again")):
                check(name, (c.eval(Z), None, c.hess(Z, mu)), "%s %s" % (what, opts), ref=ref)
            _reset(c)
    c.close()


# ---- pointer and batch paths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["U4", "U7a", "U16"])
def test_pointer_paths_and_member_window(name):
    """host_path 1 and 2 and the device-pointer calls give the same bits; a member window gives the rows of the full launch."""
    lay = uc.layout(name)
    Z, mu = uc.trajectory(name), mu_of(name)
    c = make_ctx(name)
    d1, v1 = c.eval_jac(Z)
    k1 = c.get_option("last_kernel")
    h1, e1 = c.hess(Z, mu), c.eval(Z)
    c.set_option("host_path", 2)
    d2, v2 = c.eval_jac(Z)
    k2 = c.get_option("last_kernel")
    bitwise((v2,), (c.jac(Z),), "host_path 2: jac alone")
    c.set_option("host_path", 1)
    # (the compact launch behind host_path 2 takes kernel 3 only where its role split fits the tile: at U7a, d = 16, it does not and kernel 10
    #  runs -- the same bits as that family's full values, and the truth's values per segment)
    assert (k1, k2) == ((31, 10) if name == "U7a" else (k1, k1)), (k1, k2)
    if k2 != k1:
        check(name, (d2, v2, None), "host_path 2 (kernel %d)" % k2)
        c.set_option("kernel_version", k2 // 10)
        bitwise(c.eval_jac(Z), (d2, v2), "host_path 1 against 2, kernel %d" % k2)
        assert c.get_option("last_kernel") == k2
        c.set_option("kernel_version", 0)
    else:
        bitwise((d1, v1), (d2, v2), "host_path 1 against 2")
    Zd, mud = torch.from_numpy(np.array(Z).reshape(-1)).cuda(), torch.from_numpy(np.array(mu)).cuda()
    dd, vd, hd = (torch.full((k,), NAN, dtype=torch.float64, device="cuda") for k in (c.n_rows, c.jac_nnz, c.hess_nnz))
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.eval_jac_dev(Zd, dd, vd)
    c.hess_dev(Zd, mud, hd)
    c.sync()
    c.set_stream(None)
    bitwise((d1, v1, h1), (dd.cpu().numpy(), vd.cpu().numpy(), hd.cpu().numpy()), "device pointers")
    if name in uc.MEMBERS:
        M = uc.MEMBERS[name]
        pd, pv, ph = d1.size // M, v1.size // M, h1.size // M
        c.set_member_window(1, 2)
        assert (c.n_rows, c.jac_nnz, c.hess_nnz) == (2 * pd, 2 * pv, 2 * ph)
        dw, vw = c.eval_jac(Z)
        bitwise((dw, vw, c.eval(Z), c.hess(Z, mu[pd:])), (d1[pd:], v1[pv:], e1[pd:], h1[ph:]), "member window (1, 2)")
        check(name, (np.concatenate([d1[:pd], dw]), np.concatenate([v1[:pv], vw]), None), "member window (1, 2)")
        c.set_member_window(0, M)
        bitwise((d1, v1), c.eval_jac(Z), "the window reset")
    c.close()


@pytest.mark.parametrize("name", ["U4", "U7a"])
def test_batch_of_seeds_equals_single_launches(name):
    """A PCL_BATCH_TRAJ launch of three seeds: every seed against its truth and bitwise what its own launch gives; the window (1, 2)."""
    lay, p = uc.layout(name), uc.props(name)
    Zs, mus = np.stack([uc.trajectory(name, s) for s in range(3)]), np.concatenate([uc.rand_mu(name, s) for s in range(3)])
    cb, c1 = make_ctx(name, seeds=3), make_ctx(name)
    db, vb = cb.eval_jac(Zs)
    kj = cb.get_option("last_kernel")
    eb, hb = cb.eval(Zs), cb.hess(Zs, mus)
    fam = (kj, cb.get_option("last_kernel"), cb.get_option("last_hess_kernel"))
    n_cu = cb.get_option("n_cu")
    assert fam == (uc.fused_family(p, 3 * lay.K), uc.eval_family(p, 3 * lay.K, n_cu), uc.hess_family(p, 3 * lay.K, n_cu)), fam
    pd, pv, ph = db.size // 3, vb.size // 3, hb.size // 3
    for s in range(3):
        mine = (db[s * pd : (s + 1) * pd], vb[s * pv : (s + 1) * pv], hb[s * ph : (s + 1) * ph])
        check(name, mine, "seed %d of 3" % s, seed=s)
        d1, v1 = c1.eval_jac(Zs[s])
        k1 = c1.get_option("last_kernel")
        alone = (d1, v1, c1.hess(Zs[s], uc.rand_mu(name, s)), c1.eval(Zs[s]))
        assert (k1, c1.get_option("last_kernel"), c1.get_option("last_hess_kernel")) == fam
        bitwise(mine + (eb[s * pd : (s + 1) * pd],), alone, ("seed", s))
    cb.set_member_window(1, 2)
    dw, vw = cb.eval_jac(Zs)
    bitwise((dw, vw, cb.hess(Zs, mus[pd:])), (db[pd:], vb[pv:], hb[ph:]), "window (1, 2) of the seeds")
    cb.close()
    c1.close()


# ---- launches of more than 512 intervals ----------------------------------------------------------------------------------------------------------
def _batch(batch):
    name = "U5" if batch.startswith("U5") else batch
    B, Nb = uc.BATCHES[batch]
    return name, B, Nb, uc.layout(name, Nb), uc.props(name)


def _check_batch(batch, got, ref, lab, what):
    B = ref.shape[0]
    try:
        e = uc.check_segments_batch(got.reshape(B, -1), ref, lab, TOL)
    except AssertionError as err:
        raise AssertionError("%s, %s: %s" % (batch, what, err)) from None
    note(e)
    s = max(e, key=e.get)
    print("%s, %s: %.1e (%s)" % (batch, what, e[s], s))


def test_u4_launch_of_515_intervals():
    """103 seeds x 5 intervals: kernel 4 with several items per workgroup, the pattern-compiled residual kernel 70 with three waves per workgroup
    and an idle wave in the last one (at 256 CUs), the Hessian rule on kernel 6 with three intervals per workgroup; the grids forced too."""
    name, B, Nb, lay, p = _batch("U4")
    Zs, ds, js, mus, hs = uc.batch_truth("U4", True)
    rl, jl, hl = uc.labels(lay)
    c = make_ctx(name, Nb, seeds=B)
    n_cu, items = c.get_option("n_cu"), B * lay.K
    ej = lambda: c.eval_jac(Zs)
    first = family(c, ej, [dict(), dict(grid=3), dict(contiguous=1, grid=1000)], 42)
    assert uc.fused_family(p, items) == 42
    _check_batch("U4", first[0], ds, rl, "eval_jac, delta")
    _check_batch("U4", first[1], js, jl, "eval_jac, values")
    r = family(c, lambda: (c.eval(Zs),), [dict(grid=g, eval_coop=e) for g, e in ((0, -1), (3, 0), (1000, 1))], uc.eval_family(p, items, n_cu))
    _check_batch("U4", r[0], ds, rl, "eval (82)")
    c.set_option("eval_kernel", 2)
    r = family(c, lambda: (c.eval(Zs),), GRIDS, 70)
    _check_batch("U4", r[0], ds, rl, "eval_kernel 2 (70), %d waves per workgroup, %d workgroups, %d idle" % uc.eval_sparse_grid(items, n_cu))
    c.set_option("eval_kernel", 0)
    h = family(c, lambda: (c.hess(Zs, mus.reshape(-1)),), GRIDS, uc.hess_family(p, items, n_cu), "last_hess_kernel")
    assert uc.hess_family(p, items, n_cu) == 6
    _check_batch("U4", h[0], hs, hl, "hess (6), %d workgroups" % uc.balanced_grid(items, n_cu))
    # single launches of the same families: the same bits
    c1 = make_ctx(name, Nb)
    _set(c1, hess_kernel=4)
    pd, pv, ph = ds.shape[1], js.shape[1], hs.shape[1]
    for s in (0, 51, B - 1):
        d1, v1 = c1.eval_jac(Zs[s])
        bitwise((d1, v1, c1.hess(Zs[s], mus[s])), (first[0][s * pd : (s + 1) * pd], first[1][s * pv : (s + 1) * pv], h[0][s * ph : (s + 1) * ph]), ("seed", s))
        assert c1.get_option("last_kernel") == 42 and c1.get_option("last_hess_kernel") == 6
    c1.close()
    c.close()


@pytest.mark.parametrize("batch", ["U5a", "U5b", "U7a"])
def test_both_sides_of_512_intervals(batch):
    """512 intervals: kernel 10, one workgroup per item; 516: kernel 20, whose persistent grid wraps (U7a: the specialised kernel 3 and kernel 10
    both stop holding).  Every interval against the truth; the forced kernel in single launches gives the same bits."""
    name, B, Nb, lay, p = _batch(batch)
    Zs, ds, js, _, _ = uc.batch_truth(batch, False)
    rl, jl, _ = uc.labels(lay)
    c = make_ctx(name, Nb, seeds=B)
    n_cu, items = c.get_option("n_cu"), B * lay.K
    want = uc.fused_family(p, items)
    assert want == (10 if items <= 512 else 20)
    first = family(c, lambda: c.eval_jac(Zs), [dict()] + (GRIDS[1:] if want == 20 else []), want)
    if want == 20:
        work, resident = uc.fused2_grid(p, items, n_cu)
        assert work > resident
    _check_batch(batch, first[0], ds, rl, "eval_jac (%d), delta" % want)
    _check_batch(batch, first[1], js, jl, "eval_jac (%d), values" % want)
    r = family(c, lambda: (c.eval(Zs),), GRIDS, uc.eval_family(p, items, n_cu))
    _check_batch(batch, r[0], ds, rl, "eval (%d)" % uc.eval_family(p, items, n_cu))
    bitwise((first[1],), (c.jac(Zs),), "jac alone")
    c1 = make_ctx(name, Nb)
    c1.set_option("kernel_version", want // 10)
    pd, pv = ds.shape[1], js.shape[1]
    for s in (0, B // 2, B - 1):
        bitwise(c1.eval_jac(Zs[s]), (first[0][s * pd : (s + 1) * pd], first[1][s * pv : (s + 1) * pv]), ("seed", s))
        assert c1.get_option("last_kernel") == want
    c1.close()
    c.close()
