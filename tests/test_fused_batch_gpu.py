"""The pattern-compiled fused kernel's launches of several trajectories on the device, at the sizes of tests/fused_batch_cases.py (the case table and
what each case straddles are there): several items per workgroup, contiguous column ranges, groups of workgroups with slice tickets, the reduce
payload under tickets -- and the column-group Hessian either side of its R-chain rule.  All through the device-pointer entry points, with require_jit 1
and kernel_version 4 (a system kernel 4 does not take is an error), every output prefilled with NaN before every launch.

The reference launch of a (case, order) is the static round-robin split (v4_ticket 0, contiguous 0): EVERY trajectory of it is compared with the
longdouble truth (vector_shape_cases.truth_values rounded to float64) at TOL = 1e-11 per segment of every interval, relative to the segment's own
maximum with no floor (unitary4_cases.check_segments_batch); a segment whose truth is identically zero (d/du at h = 0) must be exactly zero.  Every other
launch -- contiguous ranges, a grid of 7 workgroups under both splits and tail modes 3 and 0, v4_flags 8 and 4, tickets under every group size, slice
width and request time, five ticket launches in a row, member windows, jac_dev alone, single-trajectory launches of the one-item module -- must give
the reference's bits.  last_v4_ticket and last_v4_one_item are asserted against fused_batch_cases.launch with the context's own n_cu.
tests/test_fused_batch_cpu.py shows that every case sits where the table says, and that a stale ring slot and a slice from the wrong interval are seen.

Largest relative error read per output on an MI355X (256 CUs), one run: see the README's Parity section."""
import numpy as np
import pytest
import torch

import fused_batch_cases as fc
import piccolo_jl_amd as pa
import unitary4_cases as uc
from shape_cases import check_segments

pytestmark = pytest.mark.gpu
TOL = fc.TOL
NAN = float("nan")
CASE_ORDERS = [(name, order) for name in fc.FUSED + ("B7",) for order in fc.CASES[name][1]]
# every launch starts from these (v4_ticket auto is modelled without the timed choice: v4_tune 0)
DEFAULTS = dict(v4_ticket=0, v4_tune=0, v4_group=0, v4_ticket_cols=0, v4_ticket_ahead=2, contiguous=-1, grid=0, v4_tail_mode=3, v4_flags=0, v4_power_tiles=0,
                cols_per_slice=0)  # fmt: skip
_read = {}


def make_ctx(name, order, seeds=0):
    """seeds > 0: a PCL_BATCH_TRAJ context of that many trajectories; 0: the case's own members (one trajectory of one member for the plain cases)."""
    lay, (G0, Gj), M = fc.layout(name), fc.system(name), fc.CASES[name][3]
    args = dict(d=lay.d, m=lay.m, N=lay.N, z_dim=lay.z_dim, u_off=lay.u_off, dt_off=lay.dt_off, x_offs=fc.x_offs(name), G0=G0, Gj=Gj, batch=M,
                batch_mode=pa._lib.PCL_BATCH_MEMBERS, per_member_G0=M > 1, pade_order=order, state_cols=0)  # fmt: skip
    if M == 1:
        args.update(batch=max(seeds, 1), batch_mode=pa._lib.PCL_BATCH_TRAJ)
    c = pa.integrators._PclContext(**args)
    c.set_option("host_path", 1)
    c.set_option("require_jit", 1)
    c.set_option("kernel_version", 4)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


def note(kind, errs):
    _read[kind] = max(_read.get(kind, 0.0), max(errs.values()))


def teardown_module(module):
    print("largest relative error per output: " + "   ".join("%s %.1e" % kv for kv in _read.items()))


def nan_buf(n):
    return torch.full((int(n),), NAN, dtype=torch.float64, device="cuda")


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()  # (a copy: the truth's arrays are read-only)


class Fused:
    """eval_jac_dev of one context under option sets, each launch checked against the restated launch arithmetic."""

    def __init__(self, name, order, c, Zd, n_cu):
        self.name, self.c, self.Zd, self.n_cu, self.q = name, c, Zd, n_cu, order // 2
        self.d, self.m = fc.dims(name)
        self.K = fc.layout(name).K
        self.coop = name != "B4"  # (streamed drift classes: SP4_COOP 0)

    def model(self, intervals, **opts):
        return fc.launch(self.d, self.m, self.q, intervals, self.n_cu, coop=self.coop, **{**DEFAULTS, **opts})

    def set(self, **opts):
        for k, v in {**DEFAULTS, **opts}.items():
            self.c.set_option(k, v)

    def check_launch(self, intervals, opts):
        c, want = self.c, self.model(intervals, **opts)
        got = (c.get_option("last_kernel"), c.get_option("last_v4_ticket"), c.get_option("last_v4_one_item"))
        assert got == (40 + self.q, want["ticket"], want["one_item"]), (self.name, opts, intervals, got, want)

    def run(self, intervals, **opts):
        c = self.c
        self.set(**opts)
        dd, out = nan_buf(c.n_rows), nan_buf(c.jac_nnz)
        c.eval_jac_dev(self.Zd, dd, out)
        c.sync()
        self.check_launch(intervals, opts)
        return dd, out


def same(got, ref, what):
    for g, r in zip(got, ref):
        assert torch.equal(g, r), what


def against_truth(name, got, ref, lab, kind, what):
    try:
        e = uc.check_segments_batch(got.cpu().numpy().reshape(ref.shape[0], -1), ref, lab, TOL)
    except AssertionError as err:
        raise AssertionError("%s, %s, %s: %s" % (name, what, kind, err)) from None
    note(kind, e)
    s = max(e, key=e.get)
    print("%s, %s, %s: %.1e (%s)" % (name, what, kind, e[s], s))


# ---- residual + Jacobian --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", CASE_ORDERS)
def test_every_split_gives_the_reference_bits(name, order):
    lay = fc.layout(name)
    K, M = lay.K, fc.CASES[name][3]
    c1 = make_ctx(name, order)  # one trajectory (the ensemble: the launch itself)
    n_cu = c1.get_option("n_cu")
    B = M if M > 1 else fc.seeds(name, n_cu)
    Zs, ds, js, _, _ = fc.batch_truth(name, order, B)
    c = c1 if M > 1 else make_ctx(name, order, B)
    F = Fused(name, order, c, dev(Zs), n_cu)
    bk, g_all = B * K, max(fc.group_values(n_cu))
    rl, jl, _ = fc.labels(name)
    # 1. the static round-robin split: every trajectory against the truth
    ref = F.run(bk, v4_ticket=0, contiguous=0)
    against_truth(name, ref[0], ds, rl, "delta", "order %d, round-robin" % order)
    against_truth(name, ref[1], js, jl, "Jacobian", "order %d, round-robin" % order)
    # 2. the other static splits
    static = [dict(), dict(contiguous=1)] + [dict(contiguous=cn, grid=7, v4_tail_mode=tm) for cn in (0, 1) for tm in (3, 0)]
    static += [dict(contiguous=cn, grid=g, v4_flags=f) for f in (8, 4) for cn, g in ((0, 0), (1, 0), (0, 7), (1, 7))]
    if (name, order) == ("B1", 10):  # a ring of two tiles: q - v4_np > m, the rule adds flag 4
        static += [dict(contiguous=cn, v4_power_tiles=2) for cn in (0, 1)]
        assert F.model(bk, contiguous=0, v4_power_tiles=2)["flags"] == 4
    for o in static:
        same(F.run(bk, v4_ticket=0, **o), ref, (name, order, o))
    # 3. slice tickets: group sizes, slice widths, request times, the P wave not held to eight visits ahead, NaN tiles
    tickets = [dict(v4_group=g) for g in fc.group_values(n_cu)] + [dict(v4_ticket_cols=cc) for cc in fc.TICKET_COLS[name]]
    tickets += [dict(v4_ticket_ahead=a, v4_group=g) for a in (0, 1, 2) for g in (0, g_all)] + [dict(v4_flags=64), dict(v4_flags=8), dict(v4_flags=64, v4_group=g_all)]
    tickets += [dict(v4_group=1, v4_ticket_cols=fc.TICKET_COLS[name][0], v4_ticket_ahead=0), dict(v4_ticket=-1)]
    ran = set()
    for o in tickets:
        same(F.run(bk, **{"v4_ticket": 1, **o}), ref, (name, order, o))
        ran.add(c.get_option("last_v4_ticket"))
    if fc.ticket_ok(lay.d, lay.m, order // 2, bk, n_cu):
        assert ran >= {fc.tick_cpi(lay.d, cc) for cc in fc.TICKET_COLS[name]} | {4}, ran
    else:
        assert ran == {0}, ran
    # 4. five ticket launches in a row, no synchronisation between them: the last pipeline out re-zeroes the counters
    F.set(v4_ticket=1)
    outs = [(nan_buf(c.n_rows), nan_buf(c.jac_nnz)) for _ in range(5)]
    for dd, out in outs:
        c.eval_jac_dev(F.Zd, dd, out)
    c.sync()
    F.check_launch(bk, dict(v4_ticket=1))
    for i, o in enumerate(outs):
        same(o, ref, (name, order, "launch %d of five in a row" % i))
    del outs
    # 5. member windows -- fewer intervals than the counters last saw -- and the full window again
    pd, pv = ref[0].numel() // B, ref[1].numel() // B
    sweep = [dict(v4_ticket=0), dict(v4_ticket=-1), dict(v4_ticket=1), dict(v4_ticket=1, v4_group=g_all), dict(v4_ticket=1, v4_group=1)]
    for first, count in fc.windows(name, n_cu):
        c.set_member_window(first, count)
        part = (ref[0][first * pd : (first + count) * pd], ref[1][first * pv : (first + count) * pv])
        for o in sweep:
            same(F.run(count * K, **o), part, (name, order, "window", first, count, o))
        c.set_member_window(0, B)
        for o in sweep[:3]:
            same(F.run(bk, **o), ref, (name, order, "the full window after", first, count, o))
    # 6. jac_dev alone (no residual buffer) under tickets
    F.set(v4_ticket=1)
    vals = nan_buf(c.jac_nnz)
    c.jac_dev(F.Zd, vals)
    c.sync()
    F.check_launch(bk, dict(v4_ticket=1))
    assert torch.equal(vals, ref[1]), (name, order, "jac_dev")
    # 7. single-trajectory launches (the one-item module) of the first, a middle and the last seed
    if M == 1:
        F1 = Fused(name, order, c1, None, n_cu)
        for s in (0, B // 2, B - 1):
            F1.Zd = dev(Zs[s])
            got = F1.run(K)
            assert c1.get_option("last_v4_one_item") == 1
            same(got, (ref[0][s * pd : (s + 1) * pd], ref[1][s * pv : (s + 1) * pv]), (name, order, "seed", s))
        c1.close()
    c.close()


def test_b7_payload_under_tickets():
    """pcl_eval_jac_merit_dev on the ensemble: the payload is formed by the writer wave of whichever workgroup takes an interval's chain ticket.  v4_ticket
    0, 1, -1: the same bits (delta, values, payload), the payload fused, and within TOL per segment of the payload formed in longdouble from the truth."""
    name, order = "B7", 4
    lay, M = fc.layout(name), fc.CASES[name][3]
    c = make_ctx(name, order)
    n_cu = c.get_option("n_cu")
    F = Fused(name, order, c, dev(fc.trajectory(name)), n_cu)
    plain = F.run(M * lay.K, v4_ticket=0, contiguous=0)
    ln, sets = c.merit_grad_len()
    assert (ln, sets) == (1 + lay.K * lay.m + lay.K, 1)
    res = []
    for tk in (0, 1, -1):
        F.set(v4_ticket=tk)
        dd, out, pay = nan_buf(c.n_rows), nan_buf(c.jac_nnz), nan_buf(ln)
        c.eval_jac_merit_dev(F.Zd, None, dd, out, pay)
        c.sync()
        want = F.model(M * lay.K, v4_ticket=tk, merit=True)
        assert (c.get_option("last_kernel"), c.get_option("last_merit_fused"), c.get_option("last_v4_ticket")) == (42, 1, want["ticket"]), (tk, want)
        assert (want["ticket"] > 0) == (tk == 1)
        res.append((dd, out, pay))
    for r in res:
        same(r[:2], plain, "delta and values of the payload call")
        assert torch.equal(r[2], res[0][2]), "payload"
    rows = [fc.truth_one(name, order, member=i) for i in range(M)]
    truth = fc.payload_ld(name, [r[0] for r in rows], [r[1] for r in rows]).astype(np.float64)
    e = check_segments(res[0][2].cpu().numpy(), truth, fc.payload_labels(name), TOL)
    note("payload", e)
    print("B7 payload: %.1e (%s)" % (max(e.values()), max(e, key=e.get)))
    c.close()


# ---- the column-group Hessian either side of its R-chain rule ------------------------------------------------------------------------------------------
def test_h1_hessian_either_side_of_the_rchain_rule():
    """U17 at order 8 (cpw = 10, ng = 2), one PCL_BATCH_TRAJ context: the full window has items ng just above 8 n_cu -- R-chain waves, their block count
    padded to a multiple of 8 -- the longest window at or below has none.  Every trajectory against the truth per segment; the common trajectories
    bitwise equal outside the (u, u) entries, those within 1e-13 of their segment (the documented last-bit difference of the R-chain waves)."""
    name, order = "H1", 8
    lay = fc.layout(name)
    K, (d, m) = lay.K, fc.dims(name)
    c1 = make_ctx(name, order)
    n_cu = c1.get_option("n_cu")
    c1.close()
    B = fc.seeds(name, n_cu)
    ng = fc.hess_groups(d, m)[1]
    Bw = (8 * n_cu // ng) // K  # the longest window without R-chain waves
    assert fc.hess_rpre_auto(B * K, d, m, order // 2, n_cu) == 1 and fc.hess_rpre_auto(Bw * K, d, m, order // 2, n_cu) == 0 and (B * K) % 8 != 0 and Bw < B
    Zs, _, _, mus, hs = fc.batch_truth(name, order, B, True)
    hl = fc.labels(name)[2]
    c = make_ctx(name, order, B)
    c.set_option("hess_rpre", -1)
    Zd, mud = dev(Zs), dev(mus)
    full = nan_buf(c.hess_nnz)
    c.hess_dev(Zd, mud, full)
    c.sync()
    assert (c.get_option("last_hess_kernel"), c.get_option("last_hess_rpre")) == (84, 1)
    against_truth(name, full, hs, hl, "Hessian", "%d intervals, R-chain waves" % (B * K))
    c.set_member_window(0, Bw)
    part = nan_buf(c.hess_nnz)
    c.hess_dev(Zd, mud, part)
    c.sync()
    assert (c.get_option("last_hess_kernel"), c.get_option("last_hess_rpre")) == (84, 0) and part.numel() * B == full.numel() * Bw
    against_truth(name, part, hs[:Bw], hl, "Hessian", "%d intervals, no R-chain waves" % (Bw * K))
    a, b = full.cpu().numpy().reshape(B, -1)[:Bw], part.cpu().numpy().reshape(Bw, -1)
    uu = np.char.startswith(hl, "uu@")
    assert np.array_equal(a[:, ~uu], b[:, ~uu])
    worst = 0.0
    for s in np.unique(hl[uu]):
        sel = hl == s
        scale, err = np.abs(b[:, sel]).max(axis=1), np.abs(a[:, sel] - b[:, sel]).max(axis=1)
        assert np.all(err <= 1e-13 * scale), (s, float(err.max()))
        worst = max(worst, float(np.max(err[scale > 0] / scale[scale > 0], initial=0.0)))
    print("H1: (u, u) with against without R-chain waves: %.1e of the segment" % worst)
    c.set_member_window(0, B)
    again = nan_buf(c.hess_nnz)
    c.hess_dev(Zd, mud, again)
    c.sync()
    assert c.get_option("last_hess_rpre") == 1 and torch.equal(again, full)
    c.close()
