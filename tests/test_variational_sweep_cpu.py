"""The cases of tests/variational_shape_cases.py before any GPU is involved: that each can do its job in tests/test_variational_sweep_gpu.py.

Plan: the case table (pair slots, column workgroups, LDS bytes, the Hessian kernel's waves, passes and idle waves, the refusal at W7 / order 10)
is recomputed with the launch code's arithmetic as variational_shape_cases restates it.

Reference floor: for every case and order in (2, 4, 6, 8, 10) the float64 lifted oracle (variational_truth.residual / jacobian / hessian) agrees
with the longdouble truth per segment to 1e-13 of the segment's own maximum -- a condition on the inputs, which leaves the GPU comparison at
1e-11 a factor 100 for the kernels' summation order.  Largest value read per output kind (segment, case, order):
    residual 3.9e-16 (delta.r2#2, W2, order 10)    Jacobian 9.0e-16 (r2.h@0#1, W5, order 6)    Hessian 1.4e-14 (h.h@0#0, W6, order 10)

Sensitivity: every case sees each fault the kernels' shape handling could have, applied to the truth alone, in at least one segment of every
output the fault touches at 1e-7 relative or more (1e4 x the GPU tolerance): the top coefficient c_q zeroed (interval 2, every order); the last
drive ignored; the last state column ignored (the one the last Hessian pass and the last column workgroup own); the last variation's coupling
Gv_v read as zero; the entries of the B+- and L+-_i tiles that the block role's last pair slot stores read as zero."""
import numpy as np
import pytest

import variational_shape_cases as W
import variational_truth as vt

FLOOR = 1e-13
GPU_TOL = 1e-11
SEEN = 1e4 * GPU_TOL
NAMES = list(W.CASES)
_floors = {}


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
def test_case_table_sits_where_the_launch_code_branches():
    plan = {nm: [W.hess_plan(*W.shape(nm)[:2], W.shape(nm)[3], W.shape(nm)[2], o) for o in W.ORDERS] for nm in NAMES}
    # the Hessian kernel's waves, and the refusal
    for nm in NAMES:
        assert tuple(p["w"] if p["served"] else None for p in plan[nm]) == W.HESS_WAVES[nm], nm
        assert all(p["bytes"] <= W.LDS_BYTES for p in plan[nm] if p["served"])
    refused = [(nm, o) for nm in NAMES for o, p in zip(W.ORDERS, plan[nm]) if not p["served"]]
    assert refused == [("W7", 10)] and plan["W7"][4]["bytes"] == 190728 > W.LDS_BYTES and plan["W7"][4]["w"] == 1
    assert plan["W7"][3]["served"] and plan["W7"][3]["w"] == 1  # the same system at order 8
    served = [p for nm in NAMES for p in plan[nm] if p["served"]]
    assert {p["w"] for p in served} == set(range(1, 9))  # every wave count
    assert {p["w"] for p in served if p["idle"] > 0 and p["passes"] > 1} >= {3, 5, 6, 7}  # a last pass with idle waves (w = 4: W10 at order 6, five full passes)
    assert [(p["w"], p["passes"], p["idle"]) for p in plan["W2"][3:]] == [(7, 3, 4), (6, 3, 1)] and 17 % 7 == 3 and 17 % 6 == 5
    assert [(p["w"], p["passes"], p["idle"]) for p in plan["W4"][3:]] == [(7, 4, 5), (6, 4, 1)]
    assert (plan["W5"][4]["w"], plan["W5"][4]["passes"]) == (7, 4)
    assert (plan["W8"][0]["w"], plan["W8"][0]["passes"], W.shape("W8")[1]) == (3, 1, 3)  # w = C < 8
    assert (plan["W9"][1]["w"], plan["W9"][1]["passes"], plan["W9"][1]["idle"]) == (5, 2, 4)
    p = plan["W10"][4]  # the third wave misses by 129 doubles; ten passes
    assert (p["w"], p["passes"], p["idle"]) == (2, 10, 0) and W.hess_lds_bytes(40, 6, 2, 5, 3) // 8 - 2 * 40 * 40 == 17409
    assert W.LDS_BYTES // 8 - 2 * 40 * 40 == 17280 and 17409 - 17280 == 129
    assert plan["W3"][4]["w"] == plan["W6"][4]["w"] == 1  # kets
    # the shape of test_variational_shapes_gpu.test_v4_many_drives (n = 18, C = 9, m = 12, v = 2, order 10): served with one wave
    p = W.hess_plan(18, 9, 12, 2, 10)
    assert p["served"] and p["w"] == 1 and p["bytes"] == 98600
    # the block role's pair slots
    slots = {nm: W.pair_slots(W.shape(nm)[0]) for nm in NAMES}
    assert slots["W1"] == (512, 1, 512) and slots["W2"] == (578, 2, 66) and slots["W3"] == (968, 2, 456) and slots["W4"] == (1058, 3, 34)
    assert slots["W5"] == (1568, 4, 32) and slots["W6"] == (2048, 4, 512) and slots["W10"] == (800, 2, 288)
    assert W.pair_slots(54)[1] == 3 and W.pair_slots(56)[1] == 4  # 56: the first size that enters the fourth slot
    assert {s[1] for s in slots.values()} == {1, 2, 3, 4}
    assert W.last_slot_start(32) == 0 and W.last_slot_start(34) == 1024 and W.last_slot_start(46) == 2048 and W.last_slot_start(56) == 3072
    # the column role's workgroups
    assert W.split_cols(16) == (2, [(0, 8), (8, 16)])
    assert W.split_cols(17) == (3, [(0, 5), (5, 11), (11, 17)])
    assert W.split_cols(1) == (1, [(0, 1)]) and W.split_cols(3) == (1, [(0, 3)]) and W.split_cols(28)[0] == 4
    assert W.split_cols(17, 1) == (1, [(0, 17)]) and W.split_cols(17, 17)[0] == 17 and W.split_cols(5, 99)[0] == 5
    assert W.split_blocks(17) == 1 and W.split_blocks(17, 2) == 2 and W.split_blocks(5, 99) == 5
    # the ELL widths and the fused launch's LDS
    for nm in NAMES:
        n, C, v, m = W.shape(nm)
        G0, Gj, Gv = W.system(nm)
        wG, wD, wV = W.ell_widths(G0, Gj, Gv)
        # G(H) of a Hermitian H: Im H has a zero diagonal, n - 1 entries per row; W6's decay term fills it
        assert wG == (n if nm == "W6" else n - 1) and wV == n - 1 and wD == (n - 1 if m else 1), nm
        assert W.fused_lds_bytes(n, v, wG) == (2 + v) * n * n * 8 <= W.LDS_BYTES and W.fused_lds_bytes(n, v, wG, jac=False) == wG * n * 8
    assert W.fused_lds_bytes(56, 2, 55) == 100352 and W.fused_lds_bytes(64, 1, 64, jac=False) == 32768
    # W2: the sparse drive (empty rows) and the diagonal variation generator are padded to the widest of their group
    G0, Gj, Gv = W.system("W2")
    rows = (Gj[2] != 0).sum(axis=1)
    assert rows.max() == 2 and (rows == 0).sum() == 34 - 10 and W.ell_widths(G0, Gj[2:], Gv[1:])[1:] == (2, 1) and W.ell_widths(G0, Gj, Gv)[1:] == (33, 33)
    # W2's knot: odd state offsets, the controls last, five knots with a step of exactly zero
    cs, _ = W.case("W2")
    assert cs.N == 5 and [o % 2 for o in cs.xo] == [1, 1, 1] and cs.Z[3, cs.dt_off] == 0.0 and cs.u_off == cs.dt_off + 1 == cs.z_dim - 3


@pytest.mark.parametrize("name", NAMES)
def test_steps(name):
    cs, long_step = W.case(name)
    th = W.thetas(name)
    assert np.allclose(th[:3], [0.15, -0.3, long_step], rtol=1e-12) and (cs.K == 3 or th[3] == 0.0)
    Zl, lay, G0l, Gjl = vt.lifted(cs)
    w = W.vs.top_term_weight(lay, G0l, Gjl, Zl)
    assert w >= SEEN
    if long_step > W.vs.LONG_STEPS[0]:  # the smallest that does
        Zs = np.array(Zl)
        Zs[2, lay.dt_off] *= W.vs.LONG_STEPS[W.vs.LONG_STEPS.index(long_step) - 1] / long_step
        assert W.vs.top_term_weight(lay, G0l, Gjl, Zs) < SEEN
    for b in range(cs.v + 1):  # every component carries weight
        assert np.abs(cs.Z[:, cs.xo[b] : cs.xo[b] + cs.xdc]).max() > 0.4
    print("%s: long step %.2f, c_5 moves the residual by %.1e" % (name, long_step, w))


def test_integer_labels_are_the_text_labels():
    """jac_codes / hess_codes name the segments of jac_label / hess_label, with the interval appended."""
    for name in ("W2", "W8"):
        cs, _ = W.case(name)
        _, jr, jc, ha, hb = W.maps(name)
        for codes, text, name_of, k in ((W.jac_codes(cs, jr, jc), W.jac_label(cs, jr, jc), W.jac_name, jr // cs.xd),
                                        (W.hess_codes(cs, ha, hb), W.hess_label(cs, ha, hb), W.hess_name, np.minimum(ha, hb) // cs.z_dim)):  # fmt: skip
            want = np.char.add(np.char.add(text, "#"), k.astype(str))
            u, first = np.unique(codes, return_index=True)
            assert len(u) == len(np.unique(want))
            for s, i in zip(u, first):
                assert name_of(cs, s) == want[i]
                assert np.all(want[codes == s] == want[i])


# ---- the reference floor ----------------------------------------------------------------------------------------------------------------------
def _on_keys(keys_sorted, M, ncols):
    """The values of a scipy matrix at the sorted keys (every stored position must be one of them)."""
    M = M.tocoo()
    i, ok = W.lookup(keys_sorted, M.row.astype(np.int64) * ncols + M.col)
    assert ok.all()
    out = np.zeros(len(keys_sorted))
    out[i] = M.data
    return out


@pytest.mark.parametrize("name", NAMES)
def test_oracle_floor(name):
    cs, _ = W.case(name)
    st = W.structure(name)
    mu = W.rand_mu(name)
    for order in W.ORDERS:
        d, j, h = W.truth_ld(name, order)
        J, pos = vt.jacobian(cs, order)
        H, hpos = vt.hessian(cs, order, mu)
        assert np.array_equal(np.sort(pos), st["jkey"]) and np.array_equal(np.sort(hpos), st["hkey"])  # the same structure
        errs = (W.segment_errors(st["dcode"], vt.residual(cs, order), d), W.segment_errors(st["jcode"], _on_keys(st["jkey"], J, st["ncols"]), j),
                W.segment_errors(st["hcode"], _on_keys(st["hkey"], H, st["ncols"]), h))  # fmt: skip
        line = []
        for kind, e, name_of in zip(("residual", "Jacobian", "Hessian"), errs, (W.residual_name, W.jac_name, W.hess_name)):
            v, s = W.assert_segments(e, FLOOR, lambda c: name_of(cs, c), "%s order %d, %s" % (name, order, kind))
            line.append("%s %.1e (%s)" % (kind, v, s))
            if v > _floors.get(kind, (0.0,))[0]:
                _floors[kind] = (v, s, name, order)
        print("%s order %d: %s" % (name, order, "  ".join(line)))
    print("reference floor so far: " + "  ".join("%s %.1e (%s, %s, order %d)" % ((k,) + v) for k, v in _floors.items()))


def test_zero_step_segments_are_zero_in_the_truth():
    """W2's interval 3 (Delta t = 0): B+ = B- = I, and the L blocks and the d/du tails are identically zero -- segments held to exact zeros."""
    cs, _ = W.case("W2")
    st = W.structure("W2")
    for order in (2, 10):
        d, j, h = W.truth("W2", order)
        smax = W.segment_max(st["jcode"][st["jstruct"]], j[st["jstruct"]])
        zero = sorted(W.jac_name(cs, s) for s, v in smax.items() if v == 0)
        assert zero == sorted(["r%d.X0@%d#3" % (b, r) for b in (1, 2) for r in (0, 1)] + ["r%d.u@0#3" % b for b in (0, 1, 2)])
        assert all(v > 0 for s, v in smax.items() if s % cs.K != 3)


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_case_sees_a_zeroed_top_coefficient(name):
    """Interval 2, every order: the residual, the Jacobian values and the Hessian values each move by 1e-7 of a segment's size or more."""
    cs, _ = W.case(name)
    st = W.structure(name)
    at2 = lambda s: s % cs.K == 2
    for order in W.ORDERS:
        d, j, h = W.truth_ld(name, order)
        c0 = W.vs.coeffs(order)
        c0[-1] = 0
        bd, bj, bh = W.lifted_values(name, order, c=c0)
        got = [W.moved(st["dcode"], d, bd, at2), W.moved(st["jcode"], j, bj[st["jperm"]], at2), W.moved(st["hcode"], h, bh[st["hperm"]], at2)]
        print("%s order %d, c_q = 0: residual %.1e  Jacobian %.1e  Hessian %.1e" % ((name, order) + tuple(got)))
        assert min(got) >= SEEN, (name, order, got)


@pytest.mark.parametrize("name", NAMES)
def test_every_case_sees_the_shape_faults(name):
    n, C, v, m = W.shape(name)
    cs, _ = W.case(name)
    st = W.structure(name)
    nk = len(W._KINDS)
    scalar = lambda s: (s // (cs.K * 3)) // nk < 3 and (s // (cs.K * 3)) % nk < 3  # (u,u), (h,u), (h,h): the sums over the state columns
    last_rows = lambda s: (s // (cs.K * 3)) // nk == v  # Jacobian rows of the last component
    for order in (2, 4, 10) if name == "W8" else (4, 10):
        d, j, h = W.truth_ld(name, order)
        # (drift only at order 2: (h,h) = sum_{j >= 2} is identically zero, no scalar entry carries weight -- the column's own rows then)
        faults = {"last state column": (dict(drop_col=True), None, scalar if m or order > 2 else None), "last variation's coupling": (dict(zero_last_variation=True), last_rows, None)}
        if m:
            faults["last drive"] = (dict(drop_drive=True), None, None)
        for what, (kw, jonly, honly) in faults.items():
            bd, bj, bh = W.lifted_values(name, order, **kw)
            sd, sj, sh = W.moved(st["dcode"], d, bd), W.moved(st["jcode"], j, bj[st["jperm"]], jonly), W.moved(st["hcode"], h, bh[st["hperm"]], honly)
            print("%s order %d, %s: residual moved by %.1e, Jacobian by %.1e, Hessian by %.1e" % (name, order, what, sd, sj, sh))
            assert min(sd, sj, sh) >= SEEN, (name, order, what, sd, sj, sh)
        # the block role's last pair slot: the tiles' entries from 2 * 512 * (slots - 1) on
        bad = W.zero_last_pair_slot(name, j)
        hit = int((bad != j).sum())
        tiles = (2 + 4 * v) * C * cs.K
        assert 0 < hit <= tiles * (n * n - W.last_slot_start(n))  # (an entry that is zero anyway does not count)
        blocks = lambda s: (s // (cs.K * 3)) % nk >= 3
        sj = W.moved(st["jcode"], j, bad, blocks)
        print("%s order %d, last pair slot (%d threads): Jacobian moved by %.1e" % (name, order, W.pair_slots(n)[2], sj))
        assert sj >= SEEN and W.moved(st["jcode"], j, bad, lambda s: not blocks(s)) == 0.0
