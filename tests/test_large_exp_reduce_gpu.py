"""The option large_exp_reduce of a large exponential context (PCL_LARGE_N | PCL_LARGE_EXP, pade_order = PCL_ORDER_EXP, generator dimensions 66 .. 128) on
the device, through the C ABI on device pointers: the compact Jacobian (mode LE_COMPACT of pcl_kernel_large_exp.hpp), its device expansion
(pcl_exp_expand_large_kernel), the host-pointer calls' compact route, and the merit / reduce payload by its three routes -- from full values
(pcl_merit_grad_dev), fused with the full-values launch (LE_MERIT), and alone (LE_PAYLOAD, vals = NULL).  Cases, multipliers and the truth:
tests/large_exp_reduce_cases.py.

Tolerance: the project's 1e-11 -- the compact values PER SEGMENT of every interval, relative to the segment's own largest magnitude with no floor at 1
(shape_cases.check_segments), against the scipy truth's tiles taken once; the payload per entry on the Cauchy-Schwarz scale
sum_b w_b |lam_bk|_2 |column_bk|_2 (phi: sum w |lam| |delta|, halved for lam = delta) against the payload formed in longdouble from that truth, entries
of scale zero exact.  tests/test_large_exp_reduce_cpu.py shows the float64 emulation within 1e-13 of that payload and that it sees six faults at 1e-7.
Everything else is bitwise: compact against full, expansion against pcl_eval_jac_dev, launch against launch, the fused against the payload-only
launch, every split against the default.

Without the feature the option and the keyword are unknown, so every test here fails on the parent."""
import ctypes

import numpy as np
import pytest
import torch

import large_exp_reduce_cases as xc
import piccolo_jl_amd as pa
from oracle import pade_oracle as po
from shape_cases import check_segments

pytestmark = pytest.mark.gpu
TOL = 1e-11
EINVAL, ENOTIMPL = pa._lib.PCL_EINVAL, pa._lib.PCL_ENOTIMPL
MEMBERS, TRAJ = pa._lib.PCL_BATCH_MEMBERS, pa._lib.PCL_BATCH_TRAJ
NAN = float("nan")
K = xc.K
SEVEN = ["pcl_jac_compact_nnz", "pcl_eval_jac_compact_dev", "pcl_jac_expand_dev", "pcl_merit_grad_len", "pcl_merit_grad_dev", "pcl_eval_jac_merit_dev",
         "pcl_eval_jac_merit_objective_dev"]  # fmt: skip


def make_ctx(lay, G0, Gj, reduce=True, **kw):
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                batch_mode=MEMBERS, pade_order="exp", large_generator=True, large_exp=True, large_exp_reduce=reduce)  # fmt: skip
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
    assert c.get_option("last_kernel") == 320
    return host(dd), host(vd), dd, vd


def compact_dev(c, Zd):
    """(delta, compact values as numpy, the compact values on the device)."""
    dd, cd = nans(c.n_rows), nans(c.compact_nnz)
    c.eval_jac_compact_dev(Zd, dd, cd)
    c.sync()
    assert c.get_option("last_kernel") == 322
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
        want = ("%s is not implemented for a large exponential context (PCL_LARGE_N | PCL_LARGE_EXP, generator dimension %d > 64): residual and Jacobian, "
                "and by option large_full the objective and the rollout" % (name, n))
        assert code == ENOTIMPL and msg == want, (name, code, msg)
    del keep


def payload_ok(out, ref, scale, what):
    w = xc.worst(out, ref, scale)
    assert w <= TOL, (what, w)
    return w


# ---- 1. the option off ------------------------------------------------------------------------------------------------------------------------------
def test_option_off_keeps_the_refusals_and_the_full_host_route():
    lay, G0, Gj, Z = xc.case("L5")
    c = make_ctx(lay, G0, Gj, reduce=False)
    c.set_option("large_exp_reduce", 0)
    assert c.get_option("large_exp_reduce") == 0 and not c.large_exp_reduce and c.compact_nnz == 0 and c.compact_per == 0
    all_refused(c, 72)
    delta, vals, _, _ = eval_jac_dev(c, dev(Z))
    c.set_stream(None)
    d, v = c.eval_jac(Z)  # five columns: full values all the same
    assert c.get_option("last_kernel") == 320 and c.get_option("host_store_bytes") == 0
    assert np.array_equal(d, delta) and np.array_equal(v, vals) and np.array_equal(c.jac(Z), vals)
    c.close()


# ---- 2. the option's gates --------------------------------------------------------------------------------------------------------------------------
def test_option_gates():
    import vector_shape_cases as vc

    lay, G0, Gj, Z, _ = vc.case("K5")  # n = 54: the flags give the ordinary contexts
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                batch_mode=MEMBERS, state_cols=lay.cols)  # fmt: skip
    for kw in (dict(pade_order="exp", large_generator=True, large_exp=True), dict(pade_order=8, large_generator=True), dict(pade_order=8), dict(pade_order="exp")):
        c = pa.integrators._PclContext(**args, **kw)
        assert c.get_option("large_exp_reduce") == 0
        refused(lambda: c.set_option("large_exp_reduce", 1), EINVAL, "large_exp_reduce")
        refused(lambda: c.set_option("large_exp_reduce", 2), EINVAL, "large_exp_reduce")
        c.set_option("large_exp_reduce", 0)
        assert c.get_option("large_exp_reduce") == 0
        c.close()
    # the keywords at n <= 64: the option is not set, the ordinary exponential context refuses its compact Jacobian as it does without them
    c = pa.integrators._PclContext(**args, pade_order="exp", large_generator=True, large_exp=True, large_exp_reduce=True)
    assert not c.large and not c.large_exp and not c.large_exp_reduce and c.get_option("large_exp_reduce") == 0 and c.compact_nnz == 0
    c.close()
    # a Pade large context
    lay, G0, Gj, Z = xc.case("L1")
    pargs = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=1,
                 batch_mode=MEMBERS, state_cols=lay.cols, pade_order=8, large_generator=True)  # fmt: skip
    c = pa.integrators._PclContext(**pargs)
    assert c.large and c.get_option("large_exp_reduce") == 0
    refused(lambda: c.set_option("large_exp_reduce", 1), EINVAL, "large_exp_reduce")
    c.set_option("large_exp_reduce", 0)
    c.close()
    import robust_truth as rt
    from variational_truth import h_var_drift, make_case

    v = rt.var_context(pa, make_case(po.config_system(2), [po.G_of_H(h_var_drift(2, 2)) / 10], N=4, seed=3))
    assert v.get_option("large_exp_reduce") == 0
    refused(lambda: v.set_option("large_exp_reduce", 1), EINVAL, "large_exp_reduce")
    v.set_option("large_exp_reduce", 0)
    v.close()
    # a large exponential context: 2 and -1 are refused, 1 serves, 0 refuses again; independent of large_full and large_exp_hess
    lay, G0, Gj, Z = xc.case("L6")
    c = make_ctx(lay, G0, Gj, reduce=False)
    for bad in (2, -1):
        refused(lambda: c.set_option("large_exp_reduce", bad), EINVAL, "large_exp_reduce")
    all_refused(c, 66)
    c.set_option("large_exp_reduce", 1)
    assert c.get_option("large_exp_reduce") == 1 and c.large_exp_reduce and c.get_option("large_exp_hess") == 0 and c.get_option("large_full") == 0
    assert c.compact_per == xc.compact_per(66, 33, 1) and c.compact_nnz == K * c.compact_per and c.merit_grad_len() == (xc.payload_len(1), 1)
    refused(lambda: c.hess_structure(np.int32), ENOTIMPL, "PCL_LARGE_EXP")
    for key in ("exp_full", "large_reduce"):  # still not implemented here, with the option on
        refused(lambda: c.set_option(key, 1), ENOTIMPL, "PCL_LARGE_EXP", key)
        c.set_option(key, 0)
    c.set_option("large_exp_hess", 1)
    assert c.get_option("large_exp_reduce") == 1
    c.set_option("large_exp_hess", 0)
    # pcl_eval_jac_merit_objective_dev also needs large_full: without it, today's refusal
    all_refused(c, 66, ["pcl_eval_jac_merit_objective_dev"])
    assert compact_dev(c, dev(Z))[1].size == c.compact_nnz
    c.set_option("large_exp_reduce", 0)
    assert c.get_option("large_exp_reduce") == 0 and c.compact_nnz == 0
    all_refused(c, 66)
    for key in ("exp_full", "large_reduce"):
        refused(lambda: c.set_option(key, 1), ENOTIMPL, "PCL_LARGE_EXP", key)
    c.set_option("large_full", 1)  # ... and large_full alone does not serve it either
    all_refused(c, 66)
    c.close()


# ---- 3. the compact launch and its expansion ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", xc.NAMES)
def test_compact_launch_and_expansion(name):
    kind, n, cols, m = xc.CASES[name]
    lay, G0, Gj, Z = xc.case(name)
    c = make_ctx(lay, G0, Gj)
    per = n * n + n * cols * (m + 1)
    assert c.compact_per == per == xc.compact_per(n, cols, m) and c.compact_nnz == K * per < c.jac_nnz
    Zd = dev(Z)
    delta, vals, _, _ = eval_jac_dev(c, Zd)
    dc, comp, cd = compact_dev(c, Zd)
    errs = check_segments(comp, xc.compact_of_full(xc.truth(name)[1], n, cols, m), xc.compact_labels(n, cols, m), TOL)
    worst = max(errs, key=errs.get)
    print("%s: compact values %.1e (%s)" % (name, errs[worst], worst))
    assert np.array_equal(dc, delta), "delta of the compact launch"
    assert np.array_equal(comp, xc.compact_of_full(vals, n, cols, m)), "compact against full values"
    d2, comp2, _ = compact_dev(c, Zd)
    assert np.array_equal(d2, delta) and np.array_equal(comp2, comp), "a second compact launch"
    c2 = nans(c.compact_nnz)  # delta = NULL: the values alone
    c.eval_jac_compact_dev(Zd, None, c2)
    c.sync()
    assert np.array_equal(host(c2), comp)
    assert np.array_equal(expand_dev(c, cd), vals), "expansion"
    if n & 1:  # the scalar path at an offset of one double too
        cs, vs = nans(c.compact_nnz + 1), nans(c.jac_nnz + 1)
        cs[1:] = cd
        c.jac_expand_dev(cs[1:], vs[1:])
        c.sync()
        assert np.array_equal(host(vs[1:]), vals) and bool(torch.isnan(vs[0]))
    if name in ("L5", "L6", "X1"):
        for cps in (1, 2):
            c.set_option("cols_per_slice", cps)
            assert np.array_equal(expand_dev(c, cd), vals), ("expansion, cols_per_slice", cps)
            assert np.array_equal(compact_dev(c, Zd)[1], comp), ("compact launch, cols_per_slice", cps)
        c.set_option("cols_per_slice", 0)
    if name == "X1":
        for nt in (0, 1):
            c.set_option("nt_stores", nt)
            assert np.array_equal(expand_dev(c, cd), vals), ("expansion, nt", nt)
            assert np.array_equal(compact_dev(c, Zd)[1], comp), ("compact launch, nt", nt)
    if name == "L1z":  # the zero step: -E = -I, zero drive tails, exactly
        v = comp[per : 2 * per]
        assert np.array_equal(v[: n * n], -np.eye(n).reshape(-1)) and not v[n * n :].reshape(m + 1, n)[:m].any()
    c.close()


# ---- 4. the payload by its three routes ---------------------------------------------------------------------------------------------------------------
def route1(c, dd, lamd, vd, length):
    out = nans(length)
    c.merit_grad_dev(dd, lamd, vd, out)
    c.sync()
    return host(out)


def route2(c, Zd, lamd, length):
    d2, v2, o2 = nans(c.n_rows), nans(c.jac_nnz), nans(length)
    c.eval_jac_merit_dev(Zd, lamd, d2, v2, o2)
    c.sync()
    assert c.get_option("last_kernel") == 320 and c.get_option("last_merit_fused") == 1
    return host(d2), host(v2), host(o2)


def route3(c, Zd, lamd, length, rows=None):
    d3, o3 = nans(c.n_rows if rows is None else rows), nans(length)
    c.eval_jac_merit_dev(Zd, lamd, d3, None, o3)
    c.sync()
    assert c.get_option("last_kernel") == 323 and c.get_option("last_merit_fused") == 0
    return host(d3), host(o3)


@pytest.mark.parametrize("name", xc.NAMES)
def test_payload_routes(name):
    kind, n, cols, m = xc.CASES[name]
    lay, G0, Gj, Z = xc.case(name)
    c = make_ctx(lay, G0, Gj)
    length, sets = c.merit_grad_len()
    assert (length, sets) == (xc.payload_len(m), 1)
    Zd = dev(Z)
    delta, vals, dd, vd = eval_jac_dev(c, Zd)
    d_t, j_t = xc.truth(name)
    for lams in (None, [xc.lam(name)]):
        what = "%s, lam %s" % (name, "= delta" if lams is None else "explicit")
        lamd = None if lams is None else dev(lams[0])
        ref, scale = xc.payload(name, [d_t], [j_t], lams)
        for key in ("cols_per_slice", "general_slices", "large_exp_drives"):
            c.set_option(key, 0)
        o1 = route1(c, dd, lamd, vd, length)
        e1 = payload_ok(o1, ref, scale, what + ", from full values")
        assert np.array_equal(route1(c, dd, lamd, vd, length), o1), "route 1, a second launch"
        d2, v2, o2 = route2(c, Zd, lamd, length)
        e2 = payload_ok(o2, ref, scale, what + ", fused")
        assert np.array_equal(d2, delta) and np.array_equal(v2, vals), "route 2: delta and the full values"
        assert np.array_equal(route2(c, Zd, lamd, length)[2], o2), "route 2, a second launch"
        d3, o3 = route3(c, Zd, lamd, length)
        assert np.array_equal(d3, delta), "route 3: delta"
        assert np.array_equal(o3, o2), "route 3 against route 2"
        assert np.array_equal(route3(c, Zd, lamd, length)[1], o3), "route 3, a second launch"
        print("%s: from full values %.1e, fused / alone %.1e of the scale" % (what, e1, e2))
        if name == "L1z":  # the zero step: exact zeros on the drive entries of interval 1
            assert not o2[1 + m : 1 + 2 * m].any() and not o1[1 + m : 1 + 2 * m].any() and o2[1 + K * m + 1] != 0
        for cps, sl, dr in xc.splits(name)[1:]:
            c.set_option("cols_per_slice", cps)
            c.set_option("general_slices", sl)
            c.set_option("large_exp_drives", dr)
            d2s, v2s, o2s = route2(c, Zd, lamd, length)
            assert np.array_equal(o2s, o2) and np.array_equal(d2s, delta) and np.array_equal(v2s, vals), ("route 2", cps, sl, dr)
            d3s, o3s = route3(c, Zd, lamd, length)
            assert np.array_equal(o3s, o2) and np.array_equal(d3s, delta), ("route 3", cps, sl, dr)
    c.close()


# ---- 5. batches -------------------------------------------------------------------------------------------------------------------------------------
def test_members_weights_and_the_window():
    """L5 as two PCL_BATCH_MEMBERS members with their own drifts and weights (0.25, 0.75): one output set; under the window (1, 1) the compact trio
    covers member 1, the payload every member.  (The weights are the objective family's: pcl_set_weights is served by large_full.)"""
    name = "L5"
    kind, n, cols, m = xc.CASES[name]
    lay, _, Gj, Z = xc.case(name)
    G0s = [xc.case(name, 0, b)[1] for b in range(2)]
    w = [0.25, 0.75]
    c = make_ctx(lay, np.array(G0s), Gj, x_offs=[0, 0], batch=2, per_member_G0=True, large_full=True)
    c.set_weights(w)
    length, sets = c.merit_grad_len()
    assert (length, sets) == (xc.payload_len(m), 1)
    per_d, per_v, per_c = K * n * cols, K * xc.full_per(n, cols, m), K * xc.compact_per(n, cols, m)
    assert c.compact_nnz == 2 * per_c
    Zd = dev(Z)
    delta, vals, dd, vd = eval_jac_dev(c, Zd)
    truths = [xc.truth(name, drift=b) for b in range(2)]
    outs = {}
    for lams in (None, [xc.lam(name, b) for b in range(2)]):
        lamd = None if lams is None else dev(np.stack(lams))
        ref, scale = xc.payload(name, [t[0] for t in truths], [t[1] for t in truths], lams, w)
        o1 = route1(c, dd, lamd, vd, length)
        d2, v2, o2 = route2(c, Zd, lamd, length)
        d3, o3 = route3(c, Zd, lamd, length)
        for o in (o1, o2, o3):
            payload_ok(o, ref, scale, "two weighted members")
        assert np.array_equal(o2, o3) and np.array_equal(d2, delta) and np.array_equal(v2, vals) and np.array_equal(d3, delta)
        outs[lams is None] = (lamd, o1, o3)
    _, comp, cd = compact_dev(c, Zd)
    for b in range(2):
        assert np.array_equal(comp[b * per_c : (b + 1) * per_c], xc.compact_of_full(vals[b * per_v : (b + 1) * per_v], n, cols, m))
        check_segments(comp[b * per_c : (b + 1) * per_c], xc.compact_of_full(truths[b][1], n, cols, m), xc.compact_labels(n, cols, m), TOL)
    assert np.array_equal(expand_dev(c, cd), vals)
    # the window (1, 1)
    c.set_member_window(1, 1)
    assert c.compact_nnz == per_c and c.jac_nnz == per_v and c.n_rows == per_d
    dw, cw, cdw = compact_dev(c, Zd)
    assert np.array_equal(dw, delta[per_d:]) and np.array_equal(cw, comp[per_c:]), "the compact launch in the window"
    assert np.array_equal(expand_dev(c, cdw), vals[per_v:]), "the expansion in the window"
    for lamd, o1, o3 in outs.values():  # the merit entry points cover every member, whatever the window says
        d3, o3w = route3(c, Zd, lamd, length, rows=2 * per_d)
        assert np.array_equal(o3w, o3) and np.array_equal(d3, delta)
        assert np.array_equal(route1(c, dd, lamd, vd, length), o1)
    c.close()


def test_trajectory_seeds_give_two_sets():
    name = "L7"
    kind, n, cols, m = xc.CASES[name]
    lay, G0, Gj, _ = xc.case(name)
    Zs = [xc.case(name, s)[3] for s in range(2)]
    c = make_ctx(lay, G0, Gj, batch=2, batch_mode=TRAJ)
    length, sets = c.merit_grad_len()
    assert (length, sets) == (xc.payload_len(m), 2)
    Zd = dev(np.stack(Zs))
    delta, vals, dd, vd = eval_jac_dev(c, Zd)
    truths = [xc.truth(name, seed=s) for s in range(2)]
    for lams in (None, [xc.lam(name, s) for s in range(2)]):
        lamd = None if lams is None else dev(np.stack(lams))
        o1 = route1(c, dd, lamd, vd, 2 * length)
        d2, v2, o2 = route2(c, Zd, lamd, 2 * length)
        d3, o3 = route3(c, Zd, lamd, 2 * length)
        assert np.array_equal(o2, o3) and np.array_equal(d2, delta) and np.array_equal(v2, vals) and np.array_equal(d3, delta)
        for s in range(2):
            ref, scale = xc.payload(name, [truths[s][0]], [truths[s][1]], None if lams is None else [lams[s]])
            for o in (o1, o2):
                payload_ok(o[s * length : (s + 1) * length], ref, scale, "two seeds, seed %d" % s)
    _, comp, cd = compact_dev(c, Zd)
    assert np.array_equal(comp, xc.compact_of_full(vals, n, cols, m)) and np.array_equal(expand_dev(c, cd), vals)
    c.close()


# ---- 6. the host-pointer route ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L6", "X1"])
def test_host_pointer_route(name):
    lay, G0, Gj, Z = xc.case(name)
    c = make_ctx(lay, G0, Gj)
    delta, vals, _, _ = eval_jac_dev(c, dev(Z))
    c.set_stream(None)
    d, v = c.eval_jac(Z)
    assert c.get_option("host_store_bytes") > 0 and c.get_option("last_kernel") == 322, "the compact route"
    assert np.array_equal(d, delta) and np.array_equal(v, vals)
    assert np.array_equal(c.jac(Z), vals) and c.get_option("last_kernel") == 322
    c.set_option("host_path", 1)
    d1, v1 = c.eval_jac(Z)
    assert c.get_option("last_kernel") == 320, "host_path = 1: the full route"
    assert np.array_equal(d1, delta) and np.array_equal(v1, vals)
    c.set_option("host_path", 0)
    c.set_option("large_exp_reduce", 0)  # the option off: the full route again
    d0, v0 = c.eval_jac(Z)
    assert c.get_option("last_kernel") == 320 and np.array_equal(d0, delta) and np.array_equal(v0, vals)
    c.close()


def test_host_pointer_route_of_a_ket_stays_full():
    lay, G0, Gj, Z = xc.case("L1")
    c = make_ctx(lay, G0, Gj)
    delta, vals, _, _ = eval_jac_dev(c, dev(Z))
    c.set_stream(None)
    d, v = c.eval_jac(Z)
    assert c.get_option("host_store_bytes") == 0 and c.get_option("last_kernel") == 320
    assert np.array_equal(d, delta) and np.array_equal(v, vals)
    c.close()


# ---- 7. the ensemble step ---------------------------------------------------------------------------------------------------------------------------
def test_ensemble_step_gives_the_bits_of_the_separate_calls():
    name = "L6"
    kind, n, cols, m = xc.CASES[name]
    lay, G0, Gj, Z = xc.case(name)
    c = make_ctx(lay, G0, Gj, large_full=True)
    rng = np.random.default_rng(77700)
    goal = np.linalg.qr(rng.standard_normal((33, 33)) + 1j * rng.standard_normal((33, 33)))[0]
    c.set_goal(po.operator_to_iso_vec(goal))
    c.add_regularizer(lay.u_off, m, 1e-2, 2)
    Zd = dev(Z)
    length, sets = c.merit_grad_len()
    for lamd in (None, dev(xc.lam(name))):
        d1, v1, o1, val1, g1 = nans(c.n_rows), nans(c.jac_nnz), nans(length), nans(1), nans(c.z_len)
        c.eval_jac_merit_objective_dev(Zd, lamd, d1, v1, o1, 100.0, val1, g1)
        c.sync()
        # (an exponential context takes the two calls: the objective's one-launch tail, the fused launch, the payload's finish)
        assert c.get_option("last_merit_fused") == 1 and c.get_option("last_kernel") == 320 and c.get_option("last_step_launches") == 3
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
    import exp_truth as xt
    import vector_shape_cases as vc

    d, m, N = 33, 2, 4
    rng = np.random.default_rng(25500)
    s = pa.QuantumSystem(vc._herm(d, rng), [vc._herm(d, rng) for _ in range(m)], [1.0] * m)
    psi = rng.standard_normal(d) + 1j * rng.standard_normal(d)
    psi /= np.linalg.norm(psi)
    times = np.cumsum(np.concatenate(([0.0], 0.05 + 0.05 * rng.random(N - 1))))
    traj = pa.ket_trajectory(s, 0.3 * rng.standard_normal((m, N)), times, psi, psi)
    Z = traj.datavec.reshape(N, traj.dim).copy()
    Z[1:, : 2 * d] += 0.05 * rng.standard_normal((N - 1, 2 * d))  # an infeasible iterate: residuals of the states' size
    traj.update(Z.reshape(-1))
    KET = pa.trajectory.KET
    B = pa.BilinearIntegrator(s, traj, x_name=KET, pade_order="exp", large_generator=True, large_exp=True, large_exp_reduce=True)
    c = B.ctx
    n = 2 * d
    assert c.large and c.large_exp and c.large_exp_reduce and not c.large_full and c.compact_per == n * n + n * (m + 1) and c.compact_nnz == K * c.compact_per
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    lay = po.Layout(d=d, m=m, N=N, z_dim=traj.dim, x_off=traj.components[KET].start, u_off=traj.components["u"].start,
                    dt_off=traj.components[traj.timestep].start, cols=1)  # fmt: skip
    G0, Gj = s.G_drift, s.G_drives_array()
    d_t, j_t = po.exp_residual(Z, lay, G0, Gj).reshape(-1), xt.values(Z, lay, G0, Gj).reshape(-1)
    Zd = dev(traj.datavec)
    delta, comp, cd = compact_dev(c, Zd)
    check_segments(comp, xc.compact_of_full(j_t, n, 1, m), xc.compact_labels(n, 1, m), TOL)
    vals = expand_dev(c, cd)
    assert np.array_equal(vals, eval_jac_dev(c, Zd)[1])
    length, sets = c.merit_grad_len()
    assert (length, sets) == (xc.payload_len(m), 1)
    ref, scale = xc.payload("L1", [d_t], [j_t], None)  # (L1's sizes: iso 66, one column, two drives)
    d3, o3 = route3(c, Zd, None, length)
    payload_ok(o3, ref, scale, "BilinearIntegrator, payload alone")
    assert np.array_equal(d3, delta)
    payload_ok(route1(c, dev(delta), None, dev(vals), length), ref, scale, "BilinearIntegrator, from full values")
    B.close()
    with pytest.raises(ValueError):
        pa.BilinearIntegrator(s, traj, x_name=KET, pade_order="exp", large_generator=True, large_exp_reduce=True)
