"""The large exponential kernels (contexts created with PCL_LARGE_N | PCL_LARGE_EXP, pade_order = PCL_ORDER_EXP) over the regimes of their launch plans,
at the cases of tests/large_exp_plan_cases.py (the table and what each case stands on are there), through the C ABI on device pointers into NaN-filled
arrays: pcl_eval_jac_dev (last_kernel 320), pcl_eval_dev (321), under large_exp_reduce the compact launch (322), pcl_jac_expand_dev, the fused payload
(320) and the payload alone (323), with lam = delta and with explicit multipliers, and under large_exp_hess pcl_hess_dev (last_hess_kernel 320).

Values: TOL = 1e-11 PER SEGMENT of every interval, relative to the segment's own maximum with no floor (shape_cases.check_segments' rule), against scipy's
expm / expm_frechet through the committed oracle (exp_truth, exp_hess_truth); the payload per entry on its Cauchy-Schwarz scale against the payload formed
in longdouble from that truth, entries of scale zero exact.  tests/test_large_exp_plan_cpu.py holds the float64 emulation within 1e-12 of the same truths
and shows that every mutant is seen at 1e-7.

Bit for bit, at N = 4 and at the long launches (the case's four knots as 29 / 100 seeds of one PCL_BATCH_TRAJ launch: 87 / 300 items, whose truth is the
three-interval launch): the residual alone = the fused launch's delta, compact = full tile by tile, expansion = pcl_eval_jac_dev, fused payload = payload
alone, a second launch = the first, every forced split = the plan's own launch, the Hessian included.

The plan each launch is expected to take is the restated one (qc.jac_plan, qc.payload_plan, qc.eval_plan, qc.hess_plan) at the context's CU count; where
that is 256, 304 or 128 the tests also assert that it is the row of the committed tables.

ERR lines (pytest -s) carry the largest relative error per kind of segment; DESIGN.md 4.21.1 has what an MI355X gave."""
import re

import numpy as np
import pytest
import torch

import exp_hess_truth as eht
import exp_truth as xt
import large_exp_plan_cases as qc
import large_exp_reduce_cases as xc
import piccolo_jl_amd as pa

pytestmark = pytest.mark.gpu
TOL = qc.TOL
MEMBERS, TRAJ = pa._lib.PCL_BATCH_MEMBERS, pa._lib.PCL_BATCH_TRAJ
NAN = float("nan")
K = qc.K
JAC_KEYS = ("delta", "vals", "compact", "pay", "paylam")


def make_ctx(name, seeds=1, **kw):
    lay, G0, Gj, _ = qc.case(name)
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=[lay.x_off], G0=G0, Gj=Gj, batch=seeds,
                batch_mode=TRAJ if seeds > 1 else MEMBERS, pade_order="exp", large_generator=True, large_exp=True, large_exp_reduce=True,
                large_exp_hessian=True)  # fmt: skip
    if lay.gen is not None:
        args.update(d=lay.gen, state_cols=pa._lib.PCL_STATE_VECTOR)
    else:
        args.update(state_cols=lay.cols)
    args.update(kw)
    c = pa.integrators._PclContext(**args)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    kind, n, cols, m = qc.CASES[name]
    members = args["batch"]
    assert c.large and c.large_exp and c.get_option("large_exp_reduce") == 1 and c.get_option("large_exp_hess") == 1 and c.get_option("pade_order") == -1
    assert c.jac_per == xt.nnz_per_interval(lay) == xc.full_per(n, cols, m) and c.hess_per == eht.nnz_per_interval(lay) and c.compact_per == xc.compact_per(n, cols, m)
    assert c.n_rows == members * K * n * cols and c.jac_nnz == members * K * c.jac_per and c.hess_nnz == members * K * c.hess_per
    assert c.compact_nnz == members * K * c.compact_per and c.merit_grad_len() == (xc.payload_len(m), seeds if seeds > 1 else 1)
    return c


def plans(c, name, items=K):
    """The plans of the context's launches by the restated rules at its CU count; held to the committed tables where they have a row for it."""
    n_cu = c.get_option("n_cu")
    p, q, e, h = qc.jac_plan(name, items, n_cu), qc.payload_plan(name, items, n_cu), qc.eval_plan(name), qc.hess_plan(name)
    for x in (p, q, e, h):
        assert x["bytes"] <= qc.LDS_BYTES and x["W"] <= x["NBW"] and x["threads"] <= 512
    if n_cu in qc.CUS:
        assert qc.jac_row(p) == qc.table_row(qc.JAC_TABLE, name, items, n_cu) and qc.payload_row(q) == qc.table_row(qc.PAYLOAD_TABLE, name, items, n_cu)
    assert (qc.eval_row(e), e["nce"]) == qc.EVAL_TABLE[name] and (qc.hess_row(h), h["nce"], h["mge"]) == qc.HESS_TABLE[name]
    return p, q, e, h


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()


def nans(k):
    return torch.full((k,), NAN, dtype=torch.float64, device="cuda")


def whole(t, what):
    assert not bool(torch.isnan(t).any()), "NaN left in " + what
    return t


def compact_of_dev(v, name):
    """Each interval's first copy of -E and its tails, tile by tile, from the full values on the device."""
    kind, n, cols, m = qc.CASES[name]
    nn = n * n
    v = v.view(-1, xc.full_per(n, cols, m))
    return torch.cat([v[:, :nn], v[:, cols * nn + cols * n :]], dim=1).reshape(-1)


def hess_launch(c, Zd, mud):
    hd = nans(c.hess_nnz)
    c.hess_dev(Zd, mud, hd)
    c.sync()
    assert c.get_option("last_hess_kernel") == 320
    return whole(hd, "the Hessian")


def jac_trio(c, name, Zd):
    """The full launch, the residual alone, the compact launch and the expansion, with the identities between them: {delta, vals, compact}."""
    dd, vd = nans(c.n_rows), nans(c.jac_nnz)
    c.eval_jac_dev(Zd, dd, vd)
    c.sync()
    assert c.get_option("last_kernel") == 320
    whole(dd, "delta"), whole(vd, "the full values")
    d0 = nans(c.n_rows)
    c.eval_dev(Zd, d0)
    c.sync()
    assert c.get_option("last_kernel") == 321 and torch.equal(d0, dd), "the residual alone"
    dc, cd = nans(c.n_rows), nans(c.compact_nnz)
    c.eval_jac_compact_dev(Zd, dc, cd)
    c.sync()
    assert c.get_option("last_kernel") == 322 and torch.equal(dc, dd) and torch.equal(cd, compact_of_dev(vd, name)), "compact against full"
    ex = nans(c.jac_nnz)
    c.jac_expand_dev(cd, ex)
    c.sync()
    assert torch.equal(ex, vd), "the expansion"
    return dict(delta=dd, vals=vd, compact=cd)


def family(c, name, Zd, lamd, mud=None):
    """Every launch of the residual + Jacobian family once, into NaN-filled device arrays, `last_kernel` asserted each time, and the identities between
    them bit for bit: the residual alone = delta, compact = full, expansion = full, fused payload = payload alone (with their deltas and values).
    Returns {delta, vals, compact, pay (lam = delta), paylam}; with mud also {hess}.  At most two arrays of full values live at a time."""
    sets = c.batch if c.batch_mode == TRAJ else 1
    length = c.merit_grad_len()[0] * sets
    out = jac_trio(c, name, Zd)
    dd, vd = out["delta"], out["vals"]
    for key, lm in (("pay", None), ("paylam", lamd)):
        d2, v2, o2 = nans(c.n_rows), nans(c.jac_nnz), nans(length)
        c.eval_jac_merit_dev(Zd, lm, d2, v2, o2)
        c.sync()
        assert c.get_option("last_kernel") == 320 and c.get_option("last_merit_fused") == 1
        assert torch.equal(d2, dd) and torch.equal(v2, vd), "delta and values of the fused launch"
        del v2
        d3, o3 = nans(c.n_rows), nans(length)
        c.eval_jac_merit_dev(Zd, lm, d3, None, o3)
        c.sync()
        assert c.get_option("last_kernel") == 323 and c.get_option("last_merit_fused") == 0
        assert torch.equal(d3, dd) and torch.equal(whole(o3, "the payload"), o2), "the payload alone against the fused payload"
        out[key] = o2
    if mud is not None:
        out["hess"] = hess_launch(c, Zd, mud)
    return out


def same(a, b, what):
    """Two families of outputs, bit for bit; b may be one trajectory's outputs against a's several seeds of it."""
    for key in b:
        x, y = a[key], b[key]
        assert x.numel() % y.numel() == 0 and torch.equal(x.view(-1, y.numel()), y.view(1, -1).expand(x.numel() // y.numel(), -1)), (what, key)


def inputs(name, seeds=1):
    """(Z, mu, lam) on the device: the case's own trajectory, multipliers and payload multipliers, `seeds` times over."""
    rep = lambda a: np.tile(np.asarray(a).reshape(-1), seeds)
    return dev(rep(qc.case(name)[3])), dev(rep(qc.mu(name))), dev(rep(qc.lam(name)))


def kind_of(segment):
    """delta | -E | ones | du | dh | seg0 .. seg4: the segment without its interval and drive."""
    return re.sub(r"du\d+", "du", segment.split("@")[0])


def held_to_the_truth(name, got, report=True):
    """delta, the full and the compact values and the Hessian per segment, both payloads on their scale; returns (and prints) the worst per kind."""
    d, j = qc.truth(name)
    errs = [qc.check(got["delta"].cpu().numpy(), d, name, "delta"), qc.check(got["vals"].cpu().numpy(), j, name, "jac"),
            qc.check(got["compact"].cpu().numpy(), qc.compact_of(j, name), name, "compact")]  # fmt: skip
    if "hess" in got:
        errs.append(qc.check(got["hess"].cpu().numpy(), qc.hess_truth(name), name, "hess"))
    worst = {}
    for e in errs:
        for s, v in e.items():
            worst[kind_of(s)] = max(worst.get(kind_of(s), 0.0), v)
    for key, explicit in (("pay", False), ("paylam", True)):
        ref, scale = qc.payload_truth(name, explicit)
        worst[key] = qc.worst(got[key].cpu().numpy(), ref, scale)
        assert worst[key] <= TOL, (name, key, worst[key])
    if report:
        print("ERR %s " % name + " ".join("%s=%.1e" % kv for kv in sorted(worst.items())))
    return worst


# ---- every case against the truth ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qc.NAMES)
def test_values_per_segment(name):
    lay = qc.layout(name)
    c = make_ctx(name)
    p, q, e, h = plans(c, name)
    Zd, mud, lamd = inputs(name)
    got = family(c, name, Zd, lamd, mud)
    held_to_the_truth(name, got)
    o1 = nans(got["pay"].numel())  # ... and the payload from the full values
    c.merit_grad_dev(got["delta"], lamd, got["vals"], o1)
    c.sync()
    assert qc.worst(o1.cpu().numpy(), *qc.payload_truth(name, True)) <= TOL
    same(family(c, name, Zd, lamd, mud), got, "a second launch")
    er, ec = eht.structure(lay)
    assert c.hess_nnz == er.size == qc.hess_truth(name).size
    for dt in (np.int32, np.int64):
        rows, cols = c.hess_structure(dt)
        assert np.array_equal(rows, er) and np.array_equal(cols, ec), dt
    print("%s on %d CUs: Jacobian U %d = %d x %d chain units, npc %d, W %d of %d; payload alone U %d (mg %d); residual alone U %d; Hessian U %d = %d x %d pairs (mg %d), W %d"
          % (name, c.get_option("n_cu"), p["U"], p["sx"], p["ngrp"], p["npc"], p["W"], p["NBW"], q["U"], q["mg"], e["U"], h["U"], h["sx"], h["pairs"], h["mg"], h["W"]))  # fmt: skip
    c.close()


# ---- forced splits, bitwise against the plan's own launch ---------------------------------------------------------------------------------------------
def forced(c, name, Zd, mud, lamd, ref):
    jac, hess = qc.forced_splits(name)
    for kw in jac:
        for key, v in kw.items():
            c.set_option(key, v)
        same(family(c, name, Zd, lamd), {k: ref[k] for k in JAC_KEYS}, kw)
        for key in kw:
            c.set_option(key, 0)
    for kw in hess:
        for key, v in kw.items():
            c.set_option(key, v)
        same({"hess": hess_launch(c, Zd, mud)}, {"hess": ref["hess"]}, kw)
        for key in kw:
            c.set_option(key, 0)
    same(family(c, name, Zd, lamd, mud), ref, "back to the plan's own launch (every option 0)")


@pytest.mark.parametrize("name", qc.NAMES)
def test_forced_splits_bitwise(name):
    c = make_ctx(name)
    plans(c, name)
    Zd, mud, lamd = inputs(name)
    ref = family(c, name, Zd, lamd, mud)
    qc.check(ref["vals"].cpu().numpy(), qc.truth(name)[1], name, "jac")
    qc.check(ref["hess"].cpu().numpy(), qc.hess_truth(name), name, "hess")
    forced(c, name, Zd, mud, lamd, ref)
    c.close()


# ---- the host-pointer route ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Q3", "Q8"])
def test_host_pointer_route_gives_the_bits_of_the_device_call(name):
    """A unitary case (48 copies of -E: pcl_eval_jac takes the compact launch and expands on the host) and an odd-n case (one column: nothing to save,
    the full launch; the stores are the scalar ones)."""
    kind, n, cols, m = qc.CASES[name]
    lay, G0, Gj, Z = qc.case(name)
    c = make_ctx(name)
    Zd, mud, lamd = inputs(name)
    got = family(c, name, Zd, lamd, mud)
    delta, vals = got["delta"].cpu().numpy(), got["vals"].cpu().numpy()
    qc.check(vals, qc.truth(name)[1], name, "jac")
    c.set_stream(None)
    d, v = c.eval_jac(Z)
    assert c.get_option("last_kernel") == (322 if cols > 1 else 320) and (c.get_option("host_store_bytes") > 0) == (cols > 1)
    assert np.array_equal(d, delta) and np.array_equal(v, vals), "pcl_eval_jac"
    assert np.array_equal(c.jac(Z), vals) and np.array_equal(c.eval(Z), delta), "pcl_jac, pcl_eval"
    assert np.array_equal(c.hess(Z, qc.mu(name)), got["hess"].cpu().numpy()), "pcl_hess"
    c.close()


# ---- long launches ---------------------------------------------------------------------------------------------------------------------------------------
def three_intervals(name):
    c = make_ctx(name)
    Zd, mud, lamd = inputs(name)
    ref = family(c, name, Zd, lamd, mud)
    c.close()
    return ref


@pytest.mark.parametrize("name", qc.LONG_NAMES)
@pytest.mark.parametrize("items", list(qc.SEEDS))
def test_long_launch_gives_the_bits_of_three_intervals(name, items):
    seeds = qc.SEEDS[items]
    ref = three_intervals(name)
    c = make_ctx(name, seeds)
    p, q, e, h = plans(c, name, items)
    print("%s, %d items on %d CUs: Jacobian U %d (mg %d, npc %d, W %d: %d tiles), payload alone U %d (mg %d)"
          % (name, items, c.get_option("n_cu"), p["U"], p["mg"], p["npc"], p["W"], qc.tiles(p), q["U"], q["mg"]))  # fmt: skip
    assert c.jac_nnz * 8 * 2 + c.n_rows * 8 * 6 <= 512 << 20, "two arrays of full values and the deltas stay under 512 MB"
    Zd, mud, lamd = inputs(name, seeds)
    got = family(c, name, Zd, lamd, mud)
    same(got, ref, "the long launch against three intervals")
    first = {k: v.view(seeds, -1)[0] for k, v in got.items()}  # seed 0 held to the truth once more
    held_to_the_truth(name, first, report=False)
    del got, first
    same(family(c, name, Zd, lamd, mud), ref, "a second launch")
    c.close()


# ---- members with their own drifts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Q7", "Q3"])
def test_members_with_their_own_drifts_and_the_window(name):
    """Two PCL_BATCH_MEMBERS members with per-member drifts on the case's trajectory: each against its own truth, Hessian included; the window on the
    second alone gives its bits, and so does a context of that member alone."""
    lay, _, Gj, Z = qc.case(name)
    G0s = [qc.case(name, b)[1] for b in range(2)]
    assert not np.array_equal(G0s[0], G0s[1])
    c = make_ctx(name, x_offs=[0, 0], batch=2, G0=np.array(G0s), per_member_G0=True)
    Zd = dev(Z)
    mus = [qc.mu(name, b) for b in range(2)]
    got = jac_trio(c, name, Zd)
    got["hess"] = hess_launch(c, Zd, dev(np.stack(mus)))
    for b in range(2):
        mine = {k: got[k].view(2, -1)[b].cpu().numpy() for k in ("delta", "vals", "compact", "hess")}
        d, j = qc.truth(name, b)
        errs = [qc.check(mine["delta"], d, name, "delta"), qc.check(mine["vals"], j, name, "jac"), qc.check(mine["compact"], qc.compact_of(j, name), name, "compact"),
                qc.check(mine["hess"], qc.hess_truth(name, b), name, "hess")]  # fmt: skip
        print("%s, member %d: %s" % (name, b, " ".join("%.1e" % max(e.values()) for e in errs)))
    c.set_member_window(1, 1)
    assert c.n_rows == got["delta"].numel() // 2 and c.jac_nnz == got["vals"].numel() // 2 and c.hess_nnz == got["hess"].numel() // 2
    window = dict(jac_trio(c, name, Zd), hess=hess_launch(c, Zd, dev(mus[1])))
    for k, v in window.items():
        assert torch.equal(v, got[k].view(2, -1)[1]), ("the window on member 1", k)
    c.close()
    one = make_ctx(name, G0=G0s[1])
    alone = dict(jac_trio(one, name, Zd), hess=hess_launch(one, Zd, dev(mus[1])))
    for k in alone:
        assert torch.equal(alone[k], got[k].view(2, -1)[1]), ("member 1 alone", k)
    one.close()


# ---- the mutants of the new regimes are refused ---------------------------------------------------------------------------------------------------------------
def test_the_mutants_of_the_new_regimes_are_refused():
    """What passes against the truth fails against the emulation with the fault the case exists for: Q1's payload with the last slice of 4 taken as
    7, Q7's Hessian with the group of 3 taken as 4, Q3's values without the second of its three column tiles."""
    for name in ("Q1", "Q7", "Q3"):
        c = make_ctx(name)
        p, q, e, h = plans(c, name)
        Zd, mud, lamd = inputs(name)
        got = family(c, name, Zd, lamd, mud)
        held_to_the_truth(name, got, report=False)
        if name == "Q1":
            ref, scale = qc.payload_truth(name, True)
            bad = qc.as_if_full_payload(name, p["nce"], True)
            assert bad is not None and qc.worst(got["paylam"].cpu().numpy(), bad, scale) >= qc.SEEN
        elif name == "Q7":
            with pytest.raises(AssertionError):
                qc.check(got["hess"].cpu().numpy(), qc.first_group_size_hess(name, h["mge"]), name, "hess")
        else:
            with pytest.raises(AssertionError):
                qc.check(got["vals"].cpu().numpy(), qc.second_tile(name, p)[1], name, "jac")
        c.close()
