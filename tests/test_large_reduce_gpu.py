"""The option large_reduce of a large context (PCL_LARGE_N, generator dimensions 66 .. 128) on the device, through the C ABI on device pointers: the
compact Jacobian (mode PL_COMPACT of pcl_kernel_pade_large.hpp), its device expansion (pcl_expand_large_kernel), the host-pointer calls' compact
route, and the merit / reduce payload by its three routes -- from full values (pcl_merit_grad_dev), fused with the full-values launch (PL_MERIT), and
alone (PL_PAYLOAD, vals = NULL).  Cases, multipliers and the truth: tests/large_reduce_cases.py.

Tolerance: 1e-11 PER SEGMENT, relative to the segment's own largest magnitude with no floor at 1 (shape_cases.check_segments), against the longdouble
truth -- the compact values against the truth's tiles taken once, the payload against the payload formed in longdouble from the longdouble delta and
tails.  tests/test_large_reduce_cpu.py shows the float64 reference within 1e-13 of both and that the payload sees five faults at 1e-7.  Everything
else is bitwise: compact against full, expansion against pcl_eval_jac_dev, launch against launch, the fused against the payload-only launch, every
split against the default.

Without the feature setting the option is PCL_EINVAL (an unknown option), so every test here fails on the parent."""
import ctypes

import numpy as np
import pytest
import torch

import large_reduce_cases as rc
import piccolo_jl_amd as pa
import vector_shape_cases as vc
from oracle import pade_oracle as po
from shape_cases import check_segments, jac_labels

pytestmark = pytest.mark.gpu
TOL = 1e-11
EINVAL, ENOTIMPL = pa._lib.PCL_EINVAL, pa._lib.PCL_ENOTIMPL
MEMBERS, TRAJ = pa._lib.PCL_BATCH_MEMBERS, pa._lib.PCL_BATCH_TRAJ
NAN = float("nan")
K = rc.N - 1
SEVEN = ["pcl_jac_compact_nnz", "pcl_eval_jac_compact_dev", "pcl_jac_expand_dev", "pcl_merit_grad_len", "pcl_merit_grad_dev", "pcl_eval_jac_merit_dev",
         "pcl_eval_jac_merit_objective_dev"]  # fmt: skip


def make_ctx(lay, G0, Gj, order, reduce=True, **kw):
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                batch_mode=MEMBERS, pade_order=order, large_generator=True, large_reduce=reduce)  # fmt: skip
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


def host(t):
    a = t.cpu().numpy()
    assert not np.isnan(a).any()
    return a


def eval_jac_dev(c, Zd):
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    return host(dd), host(vd)


def compact_dev(c, Zd):
    """(delta, compact values as numpy, the compact values on the device)."""
    dd, cd = nans(c.n_rows), nans(c.compact_nnz)
    c.eval_jac_compact_dev(Zd, dd, cd)
    c.sync()
    return host(dd), host(cd), cd


def expand_dev(c, cd):
    vd = nans(c.jac_nnz)
    c.jac_expand_dev(cd, vd)
    c.sync()
    return host(vd)


def refused(call, code, *words):
    with pytest.raises(pa.PclError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def seven_calls(c):
    L, h = c._L, c._h
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    ib = np.zeros(64, dtype=np.int64)
    p = buf.data_ptr()
    i64 = ib.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    calls = {
        "pcl_jac_compact_nnz": lambda: L.pcl_jac_compact_nnz(h, i64, i64),
        "pcl_eval_jac_compact_dev": lambda: L.pcl_eval_jac_compact_dev(h, p, p, p),
        "pcl_jac_expand_dev": lambda: L.pcl_jac_expand_dev(h, p, p),
        "pcl_merit_grad_len": lambda: L.pcl_merit_grad_len(h, i64, i64),
        "pcl_merit_grad_dev": lambda: L.pcl_merit_grad_dev(h, p, p, p, p),
        "pcl_eval_jac_merit_dev": lambda: L.pcl_eval_jac_merit_dev(h, p, p, p, p, p),
        "pcl_eval_jac_merit_objective_dev": lambda: L.pcl_eval_jac_merit_objective_dev(h, p, p, p, p, p, 1.0, p, p),
    }  # fmt: skip
    assert list(calls) == SEVEN
    return calls, (buf, ib)


def all_refused(c, n, names=SEVEN):
    calls, keep = seven_calls(c)
    for name in names:
        code = calls[name]()
        msg = (c._L.pcl_last_error(c._h) or b"").decode()
        assert code == ENOTIMPL and msg == "%s is not implemented for a context created with PCL_LARGE_N (generator dimension %d > 64): residual and Jacobian only" % (name, n), (name, code, msg)
    del keep


def worst(errs):
    s = max(errs, key=errs.get)
    return "%.1e (%s)" % (errs[s], s)


# ---- 1. the option off ------------------------------------------------------------------------------------------------------------------------------
def test_option_off_keeps_the_refusals_and_the_full_host_route():
    lay, G0, Gj, Z, _ = rc.case("L5")
    c = make_ctx(lay, G0, Gj, 6, reduce=False)
    c.set_option("large_reduce", 0)
    assert c.get_option("large_reduce") == 0 and not c.large_reduce and c.compact_nnz == 0 and c.compact_per == 0
    all_refused(c, 72)
    dev_call = eval_jac_dev(c, dev(Z))
    assert c.get_option("last_kernel") == 293
    c.set_stream(None)
    d, v = c.eval_jac(Z)  # five columns: full values all the same
    assert c.get_option("last_kernel") == 293 and c.get_option("host_store_bytes") == 0
    assert np.array_equal(d, dev_call[0]) and np.array_equal(v, dev_call[1]) and np.array_equal(c.jac(Z), dev_call[1])
    check_segments(v, rc.truth("L5", 6)[1], jac_labels(lay), TOL)
    c.close()


# ---- 2. the option's gates --------------------------------------------------------------------------------------------------------------------------
def test_option_gates():
    lay, G0, Gj, Z, _ = vc.case("K5")  # n = 54: the flag gives the ordinary context
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                batch_mode=MEMBERS, state_cols=lay.cols)  # fmt: skip
    for kw in (dict(pade_order=8, large_generator=True), dict(pade_order=8), dict(pade_order="exp")):
        c = pa.integrators._PclContext(**args, **kw)
        assert c.get_option("large_reduce") == 0
        refused(lambda: c.set_option("large_reduce", 1), EINVAL, "large_reduce")
        refused(lambda: c.set_option("large_reduce", 2), EINVAL, "large_reduce")
        c.set_option("large_reduce", 0)
        assert c.get_option("large_reduce") == 0
        c.close()
    # both keywords at n <= 64: the option is not set, the ordinary context serves its compact Jacobian as it does without them
    c = pa.integrators._PclContext(**args, pade_order=8, large_generator=True, large_reduce=True)
    plain = pa.integrators._PclContext(**args, pade_order=8)
    assert not c.large and not c.large_reduce and c.get_option("large_reduce") == 0 and c.compact_nnz == plain.compact_nnz > 0
    c.close()
    plain.close()
    import robust_truth as rt
    from variational_truth import h_var_drift, make_case

    v = rt.var_context(pa, make_case(po.config_system(2), [po.G_of_H(h_var_drift(2, 2)) / 10], N=4, seed=3))
    assert v.get_option("large_reduce") == 0
    refused(lambda: v.set_option("large_reduce", 1), EINVAL, "large_reduce")
    v.set_option("large_reduce", 0)
    v.close()
    # a large context: 2 and -1 are refused, 1 serves, 0 refuses again; independent of large_hess
    lay, G0, Gj, Z, _ = rc.case("L6")
    c = make_ctx(lay, G0, Gj, 4, reduce=False)
    for bad in (2, -1):
        refused(lambda: c.set_option("large_reduce", bad), EINVAL, "large_reduce")
    all_refused(c, 66)
    c.set_option("large_reduce", 1)
    assert c.get_option("large_reduce") == 1 and c.large_reduce and c.get_option("large_hess") == 0 and c.get_option("large_full") == 0
    assert c.compact_per == rc.compact_per(66, 33, 1) and c.compact_nnz == K * c.compact_per and c.merit_grad_len() == (rc.payload_len(1), 1)
    refused(lambda: c.hess_structure(np.int32), ENOTIMPL, "PCL_LARGE_N")
    c.set_option("large_hess", 1)
    assert c.get_option("large_reduce") == 1
    c.set_option("large_hess", 0)
    # pcl_eval_jac_merit_objective_dev also needs large_full: without it, today's refusal
    all_refused(c, 66, ["pcl_eval_jac_merit_objective_dev"])
    Zd = dev(Z)
    assert compact_dev(c, Zd)[1].size == c.compact_nnz
    c.set_option("large_reduce", 0)
    assert c.get_option("large_reduce") == 0 and c.compact_nnz == 0
    all_refused(c, 66)
    c.set_option("large_full", 1)  # ... and large_full alone does not serve it either
    all_refused(c, 66)
    c.close()


# ---- 3. the compact launch and its expansion ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.NAMES)
@pytest.mark.parametrize("order", rc.ORDERS_COMPACT)
def test_compact_launch_and_expansion(name, order):
    kind, n, cols, m = rc.CASES[name]
    lay, G0, Gj, Z, _ = rc.case(name)
    q = order // 2
    c = make_ctx(lay, G0, Gj, order)
    per = 2 * n * n + n * cols * (m + 1)
    assert c.compact_per == per and c.compact_nnz == K * per == K * rc.compact_per(n, cols, m)
    if cols == 1:
        assert c.compact_nnz == c.jac_nnz
    Zd = dev(Z)
    delta, vals = eval_jac_dev(c, Zd)
    assert c.get_option("last_kernel") == 290 + q
    dc, comp, cd = compact_dev(c, Zd)
    assert c.get_option("last_kernel") == 300 + q
    ref = rc.compact_of(rc.truth(name, order)[1], n, cols, m)
    errs = check_segments(comp, ref, rc.compact_labels(n, cols, m), TOL)
    print("%s order %d: compact values %s" % (name, order, worst(errs)))
    assert np.array_equal(dc, delta), "delta of the compact launch"
    assert np.array_equal(comp, rc.compact_of(vals, n, cols, m)), "compact against full values"
    d2, comp2, _ = compact_dev(c, Zd)
    assert np.array_equal(d2, delta) and np.array_equal(comp2, comp), "a second compact launch"
    c2 = nans(c.compact_nnz)  # delta = NULL: the values alone
    c.eval_jac_compact_dev(Zd, None, c2)
    c.sync()
    assert np.array_equal(host(c2), comp)
    assert np.array_equal(expand_dev(c, cd), vals), "expansion"
    if name in ("L5", "L6"):
        for cps in (1, 2):
            c.set_option("cols_per_slice", cps)
            assert np.array_equal(expand_dev(c, cd), vals), ("expansion, cols_per_slice", cps)
            assert np.array_equal(compact_dev(c, Zd)[1], comp), ("compact launch, cols_per_slice", cps)
        c.set_option("cols_per_slice", 0)
    if name == "R1":
        for nt in (0, 1):
            c.set_option("nt_stores", nt)
            assert np.array_equal(expand_dev(c, cd), vals), ("expansion, nt", nt)
            assert np.array_equal(compact_dev(c, Zd)[1], comp), ("compact launch, nt", nt)
    c.close()


# ---- 4. the payload by its three routes ---------------------------------------------------------------------------------------------------------------
def route1(c, dd, lamd, vd, length):
    out = nans(length)
    c.merit_grad_dev(dd, lamd, vd, out)
    c.sync()
    return host(out)


def route2(c, Zd, lamd, q, length):
    d2, v2, o2 = nans(c.n_rows), nans(c.jac_nnz), nans(length)
    c.eval_jac_merit_dev(Zd, lamd, d2, v2, o2)
    c.sync()
    assert c.get_option("last_kernel") == 290 + q and c.get_option("last_merit_fused") == 1
    return host(d2), host(v2), host(o2)


def route3(c, Zd, lamd, q, length, rows=None):
    d3, o3 = nans(c.n_rows if rows is None else rows), nans(length)
    c.eval_jac_merit_dev(Zd, lamd, d3, None, o3)
    c.sync()
    assert c.get_option("last_kernel") == 310 + q and c.get_option("last_merit_fused") == 0
    return host(d3), host(o3)


@pytest.mark.parametrize("name", rc.NAMES)
@pytest.mark.parametrize("order", rc.ORDERS_PAYLOAD)
def test_payload_routes(name, order):
    kind, n, cols, m = rc.CASES[name]
    lay, G0, Gj, Z, _ = rc.case(name)
    q = order // 2
    c = make_ctx(lay, G0, Gj, order)
    length, sets = c.merit_grad_len()
    assert (length, sets) == (rc.payload_len(m), 1)
    labels = rc.payload_labels(m)
    Zd = dev(Z)
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    delta, vals = host(dd), host(vd)
    d_ld, j_ld = rc.truth_ld(name, order)
    for lams in (None, [rc.lam(name)]):
        what = "%s order %d, lam %s" % (name, order, "= delta" if lams is None else "explicit")
        lamd = None if lams is None else dev(lams[0])
        ref = rc.payload_ld(name, [d_ld], [j_ld], lams).astype(np.float64)
        c.set_option("cols_per_slice", 0)
        c.set_option("general_slices", 0)
        o1 = route1(c, dd, lamd, vd, length)
        e1 = check_segments(o1, ref, labels, TOL)
        assert np.array_equal(route1(c, dd, lamd, vd, length), o1), "route 1, a second launch"
        d2, v2, o2 = route2(c, Zd, lamd, q, length)
        e2 = check_segments(o2, ref, labels, TOL)
        assert np.array_equal(d2, delta) and np.array_equal(v2, vals), "route 2: delta and the full values"
        assert np.array_equal(route2(c, Zd, lamd, q, length)[2], o2), "route 2, a second launch"
        d3, o3 = route3(c, Zd, lamd, q, length)
        check_segments(o3, ref, labels, TOL)
        assert np.array_equal(d3, delta), "route 3: delta"
        assert np.array_equal(o3, o2), "route 3 against route 2"
        assert np.array_equal(route3(c, Zd, lamd, q, length)[1], o3), "route 3, a second launch"
        print("%s: from full values %s, fused / alone %s" % (what, worst(e1), worst(e2)))
        for cps, sl in rc.splits(name)[1:]:
            c.set_option("cols_per_slice", cps)
            c.set_option("general_slices", sl)
            d2s, v2s, o2s = route2(c, Zd, lamd, q, length)
            assert np.array_equal(o2s, o2) and np.array_equal(d2s, delta) and np.array_equal(v2s, vals), ("route 2", cps, sl)
            d3s, o3s = route3(c, Zd, lamd, q, length)
            assert np.array_equal(o3s, o2) and np.array_equal(d3s, delta), ("route 3", cps, sl)
    c.close()


# ---- 5. batches -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [4, 10])
def test_members_weights_and_the_window(order):
    """L5 as two PCL_BATCH_MEMBERS members with their own drifts and weights (0.25, 0.75): one output set; under the window (1, 1) the compact trio
    covers member 1, the payload every member.  (The weights are the objective family's: pcl_set_weights is served by large_full.)"""
    name = "L5"
    kind, n, cols, m = rc.CASES[name]
    q = order // 2
    lay, _, Gj, Z, _ = rc.case(name)
    G0s = [rc.case(name, 0, b)[1] for b in range(2)]
    w = [0.25, 0.75]
    c = make_ctx(lay, np.array(G0s), Gj, order, x_offs=[0, 0], batch=2, per_member_G0=True, large_full=True)
    c.set_weights(w)
    length, sets = c.merit_grad_len()
    assert (length, sets) == (rc.payload_len(m), 1)
    per_d, per_v, per_c = K * n * cols, K * rc.full_per(n, cols, m), K * rc.compact_per(n, cols, m)
    assert c.compact_nnz == 2 * per_c
    Zd = dev(Z)
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    delta, vals = host(dd), host(vd)
    truths = [rc.truth_ld(name, order, drift=b) for b in range(2)]
    labels = rc.payload_labels(m)
    outs = {}
    for lams in (None, [rc.lam(name, b) for b in range(2)]):
        lamd = None if lams is None else dev(np.stack(lams))
        ref = rc.payload_ld(name, [t[0] for t in truths], [t[1] for t in truths], lams, w).astype(np.float64)
        o1 = route1(c, dd, lamd, vd, length)
        d2, v2, o2 = route2(c, Zd, lamd, q, length)
        d3, o3 = route3(c, Zd, lamd, q, length)
        for o in (o1, o2, o3):
            check_segments(o, ref, labels, TOL)
        assert np.array_equal(o2, o3) and np.array_equal(d2, delta) and np.array_equal(v2, vals) and np.array_equal(d3, delta)
        outs[lams is None] = (lamd, o1, o3)
    _, comp, cd = compact_dev(c, Zd)
    for b in range(2):
        assert np.array_equal(comp[b * per_c : (b + 1) * per_c], rc.compact_of(vals[b * per_v : (b + 1) * per_v], n, cols, m))
    assert np.array_equal(expand_dev(c, cd), vals)
    # the window (1, 1)
    c.set_member_window(1, 1)
    assert c.compact_nnz == per_c and c.jac_nnz == per_v and c.n_rows == per_d
    dw, cw, cdw = compact_dev(c, Zd)
    assert np.array_equal(dw, delta[per_d:]) and np.array_equal(cw, comp[per_c:]), "the compact launch in the window"
    assert np.array_equal(expand_dev(c, cdw), vals[per_v:]), "the expansion in the window"
    for lamd, o1, o3 in outs.values():  # the merit entry points cover every member, whatever the window says
        d3, o3w = route3(c, Zd, lamd, q, length, rows=2 * per_d)
        assert np.array_equal(o3w, o3) and np.array_equal(d3, delta)
        assert np.array_equal(route1(c, dd, lamd, vd, length), o1)
    c.close()


@pytest.mark.parametrize("order", [4, 10])
def test_trajectory_seeds_give_two_sets(order):
    name = "L5"
    kind, n, cols, m = rc.CASES[name]
    q = order // 2
    lay, G0, Gj, _, _ = rc.case(name)
    Zs = [rc.case(name, s)[3] for s in range(2)]
    c = make_ctx(lay, G0, Gj, order, batch=2, batch_mode=TRAJ)
    length, sets = c.merit_grad_len()
    assert (length, sets) == (rc.payload_len(m), 2)
    Zd = dev(np.stack(Zs))
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    delta, vals = host(dd), host(vd)
    truths = [rc.truth_ld(name, order, seed=s) for s in range(2)]
    labels = rc.payload_labels(m)
    for lams in (None, [rc.lam(name, s) for s in range(2)]):
        lamd = None if lams is None else dev(np.stack(lams))
        o1 = route1(c, dd, lamd, vd, 2 * length)
        d2, v2, o2 = route2(c, Zd, lamd, q, 2 * length)
        d3, o3 = route3(c, Zd, lamd, q, 2 * length)
        assert np.array_equal(o2, o3) and np.array_equal(d2, delta) and np.array_equal(v2, vals) and np.array_equal(d3, delta)
        for s in range(2):
            ref = rc.payload_ld(name, [truths[s][0]], [truths[s][1]], None if lams is None else [lams[s]]).astype(np.float64)
            for o in (o1, o2):
                check_segments(o[s * length : (s + 1) * length], ref, labels, TOL)
    _, comp, cd = compact_dev(c, Zd)
    assert np.array_equal(comp, rc.compact_of(vals, n, cols, m)) and np.array_equal(expand_dev(c, cd), vals)
    c.close()


# ---- 6. the host-pointer route ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L6", "R1"])
def test_host_pointer_route(name):
    order, q = 6, 3
    lay, G0, Gj, Z, _ = rc.case(name)
    c = make_ctx(lay, G0, Gj, order)
    delta, vals = eval_jac_dev(c, dev(Z))
    c.set_stream(None)
    d, v = c.eval_jac(Z)
    assert c.get_option("host_store_bytes") > 0 and c.get_option("last_kernel") == 300 + q, "the compact route"
    assert np.array_equal(d, delta) and np.array_equal(v, vals)
    assert np.array_equal(c.jac(Z), vals) and c.get_option("last_kernel") == 300 + q
    c.set_option("host_path", 1)
    d1, v1 = c.eval_jac(Z)
    assert c.get_option("last_kernel") == 290 + q, "host_path = 1: the full route"
    assert np.array_equal(d1, delta) and np.array_equal(v1, vals)
    c.set_option("host_path", 0)
    c.set_option("large_reduce", 0)  # the option off: the full route again
    d0, v0 = c.eval_jac(Z)
    assert c.get_option("last_kernel") == 290 + q and np.array_equal(d0, delta) and np.array_equal(v0, vals)
    c.close()


def test_host_pointer_route_of_a_ket_stays_full():
    lay, G0, Gj, Z, _ = rc.case("L1")
    c = make_ctx(lay, G0, Gj, 6)
    delta, vals = eval_jac_dev(c, dev(Z))
    c.set_stream(None)
    d, v = c.eval_jac(Z)
    assert c.get_option("host_store_bytes") == 0 and c.get_option("last_kernel") == 293
    assert np.array_equal(d, delta) and np.array_equal(v, vals)
    c.close()


# ---- 7. the ensemble step ---------------------------------------------------------------------------------------------------------------------------
def test_ensemble_step_gives_the_bits_of_the_separate_calls():
    name, order = "L6", 4
    kind, n, cols, m = rc.CASES[name]
    lay, G0, Gj, Z, _ = rc.case(name)
    c = make_ctx(lay, G0, Gj, order, large_full=True)
    rng = np.random.default_rng(77700)
    goal = np.linalg.qr(rng.standard_normal((33, 33)) + 1j * rng.standard_normal((33, 33)))[0]
    c.set_goal(po.operator_to_iso_vec(goal))
    c.add_regularizer(lay.u_off, m, 1e-2, 2)
    Zd = dev(Z)
    length, sets = c.merit_grad_len()
    for lamd in (None, dev(rc.lam(name))):
        d1, v1, o1, val1, g1 = nans(c.n_rows), nans(c.jac_nnz), nans(length), nans(1), nans(c.z_len)
        c.eval_jac_merit_objective_dev(Zd, lamd, d1, v1, o1, 100.0, val1, g1)
        c.sync()
        assert c.get_option("last_merit_fused") == 1 and c.get_option("last_step_launches") == 2 and c.get_option("last_kernel") == 292
        d2, v2, o2, val2, g2 = nans(c.n_rows), nans(c.jac_nnz), nans(length), nans(1), nans(c.z_len)
        c.objective_dev(Zd, 100.0, val2, g2)
        c.eval_jac_merit_dev(Zd, lamd, d2, v2, o2)
        c.sync()
        for a, b in ((d1, d2), (v1, v2), (o1, o2), (val1, val2), (g1, g2)):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    c.set_option("large_full", 0)  # without large_full: today's refusal
    all_refused(c, 66, ["pcl_eval_jac_merit_objective_dev"])
    c.close()


# ---- 8. the host mirror -------------------------------------------------------------------------------------------------------------------------------
def test_bilinear_integrator_keyword():
    import large_hess_cases as hc

    s, traj, Z, lay = hc.ket33_problem()
    KET = pa.trajectory.KET
    B = pa.BilinearIntegrator(s, traj, x_name=KET, pade_order=8, large_generator=True, large_reduce=True)
    c = B.ctx
    assert c.large and c.large_reduce and not c.large_full and c.compact_nnz == c.jac_nnz > 0 and c.compact_per == c.jac_per
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    G0, Gj = s.G_drift, s.G_drives_array()
    d_ld, j_ld, _ = vc.truth_values(lay, G0, Gj, Z, None, 8, hessian=False)
    Zd = dev(traj.datavec)
    delta, comp, cd = compact_dev(c, Zd)
    check_segments(comp, j_ld.astype(np.float64).reshape(-1), jac_labels(lay), TOL)
    assert np.array_equal(expand_dev(c, cd), comp)
    length, sets = c.merit_grad_len()
    assert (length, sets) == (1 + K * 2 + K, 1)
    ref = rc.payload_ld(("iso", 66, 1, 2), [d_ld], [j_ld], None).astype(np.float64)
    d3, o3 = route3(c, Zd, None, 4, length)
    check_segments(o3, ref, rc.payload_labels(2), TOL)
    assert np.array_equal(d3, delta)
    o1 = route1(c, dev(delta), None, cd, length)
    check_segments(o1, ref, rc.payload_labels(2), TOL)
    B.close()
    with pytest.raises(ValueError):
        pa.BilinearIntegrator(s, traj, x_name=KET, pade_order=8, large_reduce=True)
