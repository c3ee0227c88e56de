"""The large-generator Pade kernels (contexts created with PCL_LARGE_N) over the regimes of their launch plans, at the cases of
tests/large_plan_cases.py (the table and what each case sits on are there), through the C ABI into NaN-filled arrays: pcl_eval_dev (280 + q),
pcl_eval_jac_dev (290 + q), pcl_hess_dev under large_hess (290 + q), and under large_reduce the compact launch (300 + q), pcl_jac_expand_dev, the
fused payload (290 + q) and the payload alone (310 + q), with lam = delta and with explicit multipliers.

Values: 1e-11 PER SEGMENT of every interval, relative to the segment's own maximum with no floor (shape_cases.check_segments' rule, on the labels of
shape_cases.jac_labels / hess_labels; a segment that is identically zero must be exact zeros), against the longdouble truth of
tests/vector_shape_cases.py rounded to float64; the payload against large_reduce_cases.payload_ld on that truth.  tests/test_large_plan_cpu.py holds
the float64 oracle within 1e-13 of the same truth and shows that the truth sees the fault each case exists for.

Bit for bit, at N = 4 and at the long launches (the case's four knots as 29 / 100 seeds of one PCL_BATCH_TRAJ launch: 87 / 300 items, whose truth is the
three-interval launch): compact = full, expansion = pcl_eval_jac_dev, fused payload = payload alone, the residual alone = the fused launch's delta, a
second launch = the first, host pointers = device pointers, every forced split = the default plan.

The plan each launch takes is the restated one (lc.large_plan, hc.hess_plan) at the context's CU count; where that is 256, 304 or 128 the tests also
assert that it is the row of the committed tables.

ERR lines (pytest -s) carry the largest relative error per segment kind; DESIGN.md 4.17.1 has what an MI355X gave.

83 tests; 27 s of wall time on an MI355X, the slowest (P1 at order 10: 5.3 million Jacobian values compared on the host) 3.7 s; the truths
are computed once per (case, order) and shared by every test of the case."""
import re

import numpy as np
import pytest
import torch

import large_plan_cases as pc
import piccolo_jl_amd as pa
from oracle import pade_oracle as po

pytestmark = pytest.mark.gpu
TOL = pc.TOL
MEMBERS, TRAJ = pa._lib.PCL_BATCH_MEMBERS, pa._lib.PCL_BATCH_TRAJ
NAN = float("nan")
K = pc.K
CASE_ORDERS = [(name, order) for name in pc.NAMES for order in pc.ORDERS[name]]


def make_ctx(name, order, seeds=1):
    lay, G0, Gj, _, _ = pc.case(name)
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=seeds,
                batch_mode=TRAJ if seeds > 1 else MEMBERS, pade_order=order, large_generator=True, large_hessian=True, large_reduce=True)  # fmt: skip
    if lay.gen is not None:
        args.update(d=lay.gen, state_cols=pa._lib.PCL_STATE_VECTOR)
    else:
        args.update(state_cols=lay.cols)
    c = pa.integrators._PclContext(**args)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    kind, n, cols, m = pc.shape(name)
    items = seeds * K
    assert c.large and c.get_option("large_hess") == 1 and c.get_option("large_reduce") == 1
    assert c.n_rows == items * n * cols and c.jac_nnz == items * po.jac_nnz_per_interval(lay) and c.hess_nnz == items * po.hess_nnz_per_interval(lay)
    assert c.compact_nnz == items * pc.rc.compact_per(n, cols, m) and c.merit_grad_len() == (pc.rc.payload_len(m), seeds if seeds > 1 else 1)
    return c


def plans(c, name, items=K):
    """The plans of the context's launches by the restated rules at its CU count; held to the committed tables where they have a row for it."""
    n_cu = c.get_option("n_cu")
    p, h = pc.jac_plan(name, items=items, n_cu=n_cu), pc.hess_plan(name)
    assert p["bytes"] <= pc.LDS_BYTES and h["bytes"] <= pc.LDS_BYTES and p["pairs"] <= pc.lc.NP_PAIRS
    row = (p["U"], p["sx"], p["ngrp"], p["mg"], p["npc"], p["bytes"])
    if items == K and name in pc.TABLE and n_cu in (256, 304, 128):
        assert row == pc.TABLE[name] and ((h["U"], h["sx"], h["nc"], h["ngrp"], h["mg"], h["bytes"]), h["nce"], h["mge"]) == pc.HESS_TABLE[name]
    if (name, items, n_cu) in pc.LONG:
        assert (p["U"], p["npc"], p["npce"], p["pairs"], p["bytes"]) == pc.LONG[(name, items, n_cu)]
    return p, h


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()


def nans(k):
    return torch.full((k,), NAN, dtype=torch.float64, device="cuda")


def compact_of_dev(v, name):
    kind, n, cols, m = pc.shape(name)
    nn = n * n
    v = v.view(-1, pc.rc.full_per(n, cols, m))
    return torch.cat([v[:, :nn], v[:, cols * nn : cols * nn + nn], v[:, 2 * cols * nn :]], dim=1).reshape(-1)


def jac_family(c, name, Zd, lamd, q, hess=None):
    """Every launch of the residual + Jacobian family once, into NaN-filled device arrays, `last_kernel` asserted each time, and the identities between
    them bit for bit: the residual alone = delta, compact = full, expansion = full, fused payload = payload alone (with their deltas and values).
    Returns {delta, vals, compact, pay (lam = delta), paylam}; with hess = mu on the device also {hess}."""
    out = {}
    sets = c.batch if c.batch_mode == TRAJ else 1
    length = c.merit_grad_len()[0] * sets
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    assert c.get_option("last_kernel") == 290 + q
    assert not bool(torch.isnan(dd).any()) and not bool(torch.isnan(vd).any())
    d0 = nans(c.n_rows)
    c.eval_dev(Zd, d0)
    c.sync()
    assert c.get_option("last_kernel") == 280 + q and torch.equal(d0, dd), "the residual alone"
    dc, cd = nans(c.n_rows), nans(c.compact_nnz)
    c.eval_jac_compact_dev(Zd, dc, cd)
    c.sync()
    assert c.get_option("last_kernel") == 300 + q and torch.equal(dc, dd) and torch.equal(cd, compact_of_dev(vd, name)), "compact against full"
    ex = nans(c.jac_nnz)
    c.jac_expand_dev(cd, ex)
    c.sync()
    assert torch.equal(ex, vd), "the expansion"
    del ex
    for key, lm in (("pay", None), ("paylam", lamd)):
        d2, v2, o2 = nans(c.n_rows), nans(c.jac_nnz), nans(length)
        c.eval_jac_merit_dev(Zd, lm, d2, v2, o2)
        c.sync()
        assert c.get_option("last_kernel") == 290 + q and c.get_option("last_merit_fused") == 1
        assert torch.equal(d2, dd) and torch.equal(v2, vd), "delta and values of the fused launch"
        del v2
        d3, o3 = nans(c.n_rows), nans(length)
        c.eval_jac_merit_dev(Zd, lm, d3, None, o3)
        c.sync()
        assert c.get_option("last_kernel") == 310 + q and c.get_option("last_merit_fused") == 0
        assert torch.equal(d3, dd) and torch.equal(o3, o2), "the payload alone against the fused payload"
        out[key] = o2
    out.update(delta=dd, vals=vd, compact=cd)
    if hess is not None:
        out["hess"] = hess_launch(c, Zd, hess, q)
    return out


def hess_launch(c, Zd, mud, q):
    hd = nans(c.hess_nnz)
    c.hess_dev(Zd, mud, hd)
    c.sync()
    assert c.get_option("last_hess_kernel") == 290 + q and not bool(torch.isnan(hd).any())
    return hd


def same(a, b, what):
    """Two families of outputs, bit for bit; b may be one trajectory's outputs against a's several seeds of it."""
    for key in b:
        x, y = a[key], b[key]
        assert x.numel() % y.numel() == 0 and torch.equal(x.view(-1, y.numel()), y.view(1, -1).expand(x.numel() // y.numel(), -1)), (what, key)


def kind_of(segment):
    """delta | B+ | B- | du | dh | uu | hu | hh | u.Xk | h.Xk | Xn.u | Xn.h | phi | gu | gdt: the segment without its interval and drive."""
    return re.sub(r"u\d+", "u", segment.split("@")[0].replace("Xk1", "Xn"))


def report(name, order, errs):
    worst = {}
    for e in errs:
        for s, v in e.items():
            k = kind_of(s)
            worst[k] = max(worst.get(k, 0.0), v)
    print("ERR %s %d " % (name, order) + " ".join("%s=%.1e" % kv for kv in sorted(worst.items())))


def inputs(name, seeds=1):
    """(Z, mu, lam) on the device: the case's own trajectory, multipliers and payload multipliers, `seeds` times over."""
    rep = lambda a: np.tile(np.asarray(a).reshape(-1), seeds)
    return dev(rep(pc.case(name)[3])), dev(rep(pc.rand_mu(name))), dev(rep(pc.lam(name)))


# ---- every case and order against the truth ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", CASE_ORDERS)
def test_values_per_segment(name, order):
    q = order // 2
    c = make_ctx(name, order)
    p, h = plans(c, name)
    Zd, mud, lamd = inputs(name)
    got = jac_family(c, name, Zd, lamd, q, hess=mud)
    d, j = pc.truth(name, order)
    errs = [pc.check(got["delta"].cpu().numpy(), d, name, "delta"), pc.check(got["vals"].cpu().numpy(), j, name, "jac"),
            pc.check(got["compact"].cpu().numpy(), pc.compact_of(j, name), name, "compact"),
            pc.check(got["pay"].cpu().numpy(), pc.payload_truth(name, order, False), name, "payload"),
            pc.check(got["paylam"].cpu().numpy(), pc.payload_truth(name, order, True), name, "payload"),
            pc.check(got["hess"].cpu().numpy(), pc.hess_truth(name, order), name, "hess")]  # fmt: skip
    o1 = nans(got["pay"].numel())  # ... and the payload from the full values
    c.merit_grad_dev(got["delta"], lamd, got["vals"], o1)
    c.sync()
    errs.append(pc.check(o1.cpu().numpy(), pc.payload_truth(name, order, True), name, "payload"))
    report(name, order, errs)
    same(jac_family(c, name, Zd, lamd, q, hess=mud), got, "a second launch")
    print("%s order %d: Jacobian U %d (%d x %d, npc %d), Hessian U %d (%d x %d)" % (name, order, p["U"], p["sx"], p["ngrp"], p["npc"], h["U"], h["sx"], h["ngrp"]))
    c.close()


# ---- forced splits and host pointers at N = 4 ------------------------------------------------------------------------------------------------------------
def forced(c, name, Zd, mud, lamd, q, ref, items=K):
    jac, hess = pc.forced_splits(name, c.get_option("n_cu"), items)
    for kw in jac:
        for key, v in kw.items():
            c.set_option(key, v)
        same(jac_family(c, name, Zd, lamd, q), {k: ref[k] for k in ("delta", "vals", "compact", "pay", "paylam")}, kw)
        for key in kw:
            c.set_option(key, 0)
    for kw in hess:
        for key, v in kw.items():
            c.set_option(key, v)
        same({"hess": hess_launch(c, Zd, mud, q)}, {"hess": ref["hess"]}, kw)
        for key in kw:
            c.set_option(key, 0)
    same(jac_family(c, name, Zd, lamd, q, hess=mud), ref, "back to the default plan")


def host_pointers(c, name, seeds, got):
    lay, G0, Gj, Z, _ = pc.case(name)
    Zh, muh = np.tile(Z.reshape(-1), seeds), np.tile(pc.rand_mu(name), seeds)
    c.set_stream(None)
    d, v = c.eval_jac(Zh)
    assert np.array_equal(d, got["delta"].cpu().numpy()) and np.array_equal(v, got["vals"].cpu().numpy()), "pcl_eval_jac"
    assert np.array_equal(c.eval(Zh), d) and np.array_equal(c.jac(Zh), v), "pcl_eval, pcl_jac"
    assert np.array_equal(c.hess(Zh, muh), got["hess"].cpu().numpy()), "pcl_hess"


@pytest.mark.parametrize("name", pc.NAMES)
@pytest.mark.parametrize("order", [4, 10])
def test_forced_splits_and_host_pointers_bitwise(name, order):
    q = order // 2
    c = make_ctx(name, order)
    Zd, mud, lamd = inputs(name)
    ref = jac_family(c, name, Zd, lamd, q, hess=mud)
    pc.check(ref["vals"].cpu().numpy(), pc.truth(name, order)[1], name, "jac")
    pc.check(ref["hess"].cpu().numpy(), pc.hess_truth(name, order), name, "hess")
    forced(c, name, Zd, mud, lamd, q, ref)
    host_pointers(c, name, 1, ref)
    c.close()


# ---- long launches --------------------------------------------------------------------------------------------------------------------------------------
def three_intervals(name, order):
    c = make_ctx(name, order)
    Zd, mud, lamd = inputs(name)
    ref = jac_family(c, name, Zd, lamd, order // 2, hess=mud)
    pc.check(ref["delta"].cpu().numpy(), pc.truth(name, order)[0], name, "delta")
    pc.check(ref["vals"].cpu().numpy(), pc.truth(name, order)[1], name, "jac")
    pc.check(ref["hess"].cpu().numpy(), pc.hess_truth(name, order), name, "hess")
    c.close()
    return ref


@pytest.mark.parametrize("name", pc.LONG_NAMES)
@pytest.mark.parametrize("items", list(pc.SEEDS))
@pytest.mark.parametrize("order", [4, 10])
def test_long_launch_gives_the_bits_of_three_intervals(name, items, order):
    q, seeds = order // 2, pc.SEEDS[items]
    ref = three_intervals(name, order)
    c = make_ctx(name, order, seeds)
    p, h = plans(c, name, items)
    print("%s order %d, %d items on %d CUs: U %d, npc %s, %d pairs per thread" % (name, order, items, c.get_option("n_cu"), p["U"], p["npce"], p["pairs"]))
    Zd, mud, lamd = inputs(name, seeds)
    got = jac_family(c, name, Zd, lamd, q, hess=mud)
    same(got, ref, "the long launch against three intervals")
    same(jac_family(c, name, Zd, lamd, q, hess=mud), got, "a second launch")
    forced(c, name, Zd, mud, lamd, q, got, items)
    host_pointers(c, name, seeds, got)
    c.close()


def test_bench_shape_at_87_items():
    """P1 (d = 60, four drives) as 29 trajectories: the plan of three intervals, 87 x 48 = 4,176 workgroups."""
    name, order, seeds = "P1", 4, 29
    ref = three_intervals(name, order)
    c = make_ctx(name, order, seeds)
    p, h = plans(c, name, 87)
    assert (p["U"], p["sx"], p["ngrp"], p["npc"]) == (48, 12, 4, 3) and 87 * p["U"] == 4176
    Zd, mud, lamd = inputs(name, seeds)
    same(jac_family(c, name, Zd, lamd, order // 2, hess=mud), ref, "87 items against three intervals")
    c.close()


# ---- the mutated truths are refused -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.MUTANT_NAMES)
def test_the_mutated_truth_is_refused(name):
    """The values that pass against the truth fail against the truth with the fault the case exists for (a dropped column, drive, pair slot or row tile)."""
    order = pc.MUTANT_ORDER
    c = make_ctx(name, order)
    Zd, mud, lamd = inputs(name)
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    d, v, hs = dd.cpu().numpy(), vd.cpu().numpy(), hess_launch(c, Zd, mud, order // 2).cpu().numpy()
    pc.check(d, pc.truth(name, order)[0], name, "delta")
    pc.check(v, pc.truth(name, order)[1], name, "jac")
    pc.check(hs, pc.hess_truth(name, order), name, "hess")
    muts = pc.mutants(name)
    assert muts
    for what, (bd, bj, bh) in muts.items():
        with pytest.raises(AssertionError):
            pc.check(v, bj.astype(np.float64), name, "jac")
        if bh is not None:
            with pytest.raises(AssertionError):
                pc.check(hs, bh.astype(np.float64), name, "hess")
    c.close()


# ---- no drive at all ------------------------------------------------------------------------------------------------------------------------------------------
def test_drive_less_structure_and_counts():
    """P5 (m = 0): pcl_jac_nnz / pcl_hess_nnz and both structures are those of a system without a drive column."""
    lay = pc.layout("P5")
    n = 104
    c = make_ctx("P5", 6)
    assert c.jac_nnz == K * (2 * n * n + n) and c.jac_per == 2 * n * n + n and c.hess_nnz == K * (1 + 2 * n) and c.hess_per == 1 + 2 * n
    assert c.compact_nnz == c.jac_nnz and c.merit_grad_len() == (1 + K, 1)
    for dtype in (np.int32, np.int64):
        rows, cols = c.jac_structure(dtype)
        er, ec = po.jac_structure(lay)
        assert np.array_equal(rows, er) and np.array_equal(cols, ec)
        rows, cols = c.hess_structure(dtype)
        er, ec = po.hess_structure(lay)
        assert np.array_equal(rows, er) and np.array_equal(cols, ec)
    c.close()
