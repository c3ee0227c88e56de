"""The cases of tests/unitary4_cases.py before any GPU is involved: that each can do its job in tests/test_unitary4_shapes_gpu.py.

Branch table: every claim of the case table is recomputed from the matrices (n_upos, the ELL widths, antisymmetry, the iso structure, the
pattern-compiled plans' limits) and with the launch code's arithmetic restated in unitary4_cases (v1_auto, v3_specialised, ell_fits_lds, the
wu rules, hess_v2_supported, the d >= 12 rules, nw, balanced_grid and the byte formulas), at n_cu = 256 and, where a rule reads n_cu, at 304 and 128.

Oracle floor: po.pade_residual, po.pade_jacobian_values and po.pade4_hessian_values agree with the longdouble truth per segment to 1e-13 of the
segment's own maximum -- a condition on the inputs (no near-cancelling scalar segment), which leaves the GPU comparison at 1e-11 a factor 100
for the kernels' summation order.  Largest value read (segment, case):
    residual 2.2e-16 (delta@1, U16)    Jacobian 5.2e-16 (dh@3, U12)    Hessian 1.4e-14 (hh@2, U6a)

Fault sensitivity: a zeroed c_2, the last drive dropped, the last state column dropped, and every product without its last row, its last
column or its last inner index each move a segment of the Jacobian and a segment of the Hessian by 1e-7 of its own size or more (1e4 x the
GPU tolerance).

Segments that matter: every case has a (u, u) or (h, u) segment below 0.1 of its interval's largest Hessian segment -- what a comparison
against the whole array's maximum does not hold."""
import numpy as np
import pytest

import unitary4_cases as uc
from oracle import pade_oracle as po
from shape_cases import check_segments, cf_pairs, n_mags

FLOOR = 1e-13
GPU_TOL = 1e-11
SEEN = 1e4 * GPU_TOL
NAMES = list(uc.CASES)
_floors = {}


def worst(errs):
    s = max(errs, key=errs.get)
    return errs[s], s


# ---- the case table's claims ----------------------------------------------------------------------------------------------------------------------
def test_branch_table():
    P = {name: uc.props(name) for name in NAMES}
    one = lambda name: 4 * uc.MEMBERS.get(name, 1)  # intervals of the one-trajectory launch
    auto = lambda name, n_cu=256: (uc.fused_family(P[name], one(name)), uc.eval_family(P[name], one(name), n_cu), uc.hess_family(P[name], one(name), n_cu))
    assert uc.ORDER == 4 and uc.STEPS == (0.15, -0.3, 0.0, 0.5)
    for name, (kind, d, m, par) in uc.CASES.items():
        p = P[name]
        assert (p["d"], p["n"], p["m"]) == (d, 2 * d, m) and p["iso"] == (kind != "real") and p["anti"] == (kind != "real"), name
        assert p["sp"] == (kind == "ctl"), name  # a dense drift fills the union pattern: no pattern-compiled kernel
        assert uc.v3_fits(p) == (d < 31), name  # (four double-buffered tiles of n = 62 or 64 rows exceed the LDS: kernel 3 declines)
        for n_cu in (128, 256, 304):  # one trajectory of four intervals: no rule below reads n_cu at these sizes
            assert auto(name, n_cu) == auto(name), name
    widths = lambda name: (P[name]["ell_w"], P[name]["ellt_w"], P[name]["uell_w"])
    # U1 .. U3: the small kernel
    assert auto("U1") == (52, 52, 2) and P["U1"]["n"] == 8 and widths("U1") == (1, 1, 1)
    assert uc.fused_family(P["U1"], 4, kernel_version=1) == 10 and uc.fused_family(P["U1"], 4, kernel_version=2) == 20
    assert uc.hess_family(P["U1"], 4, 256, hess_kernel=3) == 5  # (the d >= 12 rule is auto's)
    assert auto("U2") == (10, 52, 2) and P["U2"]["d"] % 2 == 1 and uc.v1_auto(P["U2"], 10**6)
    assert auto("U3") == (10, 52, 1) and not uc.hess_v2_supported(P["U3"]) and widths("U3")[:2] == (1, 1)
    assert uc.hess_family(P["U3"], 4, 256, hess_kernel=2) == "ESHAPE" and uc.small_kernel(P["U3"], False) and not uc.small_kernel(dict(P["U3"], m=9), False)
    # U4, U17: the pattern-compiled family; U4's launch of 515 intervals
    for name in ("U4", "U17"):
        p = P[name]
        assert auto(name) == (42, 82, 82) and widths(name) == (2, 2, 1) and p["v4"] and p["hc"]
        f = lambda **kw: uc.fused_family(p, 4, **kw)
        e = lambda **kw: uc.eval_family(p, 4, 256, **kw)
        h = lambda **kw: uc.hess_family(p, 4, 256, **kw)
        assert (f(kernel_version=3), f(kernel_version=2), f(kernel_version=1), f(kernel_version=5)) == (32, 20, 10, "ESHAPE")
        assert (f(kernel_version=3, jit=0), f(jit=0), f(use_mfma=0)) == (30, 10, 10)
        assert (e(eval_kernel=2), e(eval_kernel=1), e(eval_kernel=3), e(jit=0), e(eval_kernel=2, jit=0)) == (70, 60, 82, 60, "ESHAPE")
        assert (h(hess_kernel=4), h(hess_kernel=7), h(hess_kernel=3), h(hess_kernel=2), h(hess_kernel=1), h(hess_kernel=8)) == (6, 72, 5, 2 if p["d"] < 12 else 3, 1, 82)
        assert (h(jit=0), h(hess_kernel=3, jit=0), h(hess_kernel=4, jit=0), h(use_mfma=0, jit=0)) == (2, "ESHAPE", "ESHAPE", 1)
    assert P["U4"]["d"] == 9 and not uc.props("U3")["sp"]  # the smallest pattern-compiled d
    B, Nb = uc.BATCHES["U4"]
    items = B * (Nb - 1)
    assert items == 515
    for n_cu in (256, 304):
        assert 2 * 4 <= n_cu < 2 * items and uc.hess_family(P["U4"], items, n_cu) == 6 and uc.eval_family(P["U4"], items, n_cu) == 82
        assert uc.eval_family(P["U4"], items, n_cu, eval_kernel=2) == 70 and uc.fused_family(P["U4"], items) == 42
    assert uc.eval_sparse_grid(items, 256) == (3, 172, 1) and uc.eval_sparse_grid(items, 304) == (2, 258, 1)
    assert uc.balanced_grid(items, 256) == 172 and -(-items // 172) == 3 and uc.balanced_grid(items, 304) == 258  # several intervals per workgroup
    assert uc.balanced_grid(items, 256, 3) == 3 and uc.balanced_grid(items, 256, 1000) == 515
    assert items * 9 < 28 * 256  # (below the contiguous ranges and the slice tickets of kernel 4: the static split, the same bits in every launch)
    # U5: the two sides of d <= 16 && win_count K <= 512
    (Ba, Na), (Bb, Nb) = uc.BATCHES["U5a"], uc.BATCHES["U5b"]
    assert Ba * (Na - 1) == 512 and Bb * (Nb - 1) == 516 and auto("U5") == (10, 60, 2)
    assert uc.fused_family(P["U5"], 512) == 10 and uc.fused_family(P["U5"], 516) == 20
    for n_cu in (256, 304):
        work, resident = uc.fused2_grid(P["U5"], 516, n_cu)
        assert work > resident, (work, resident)  # the persistent grid wraps
    assert 516 * po.jac_nnz_per_interval(uc.layout("U5")) * 8 == 34675200 and po.jac_nnz_per_interval(uc.layout("U5")) == 8400
    # U6: the d >= 12 rules of the Hessian
    assert auto("U6a") == (10, 60, 2) and auto("U6b") == (10, 60, 5)
    assert uc.hess_family(P["U6b"], 4, 256, hess_kernel=2) == 3 and uc.hess_family(P["U6a"], 4, 256, hess_kernel=2) == 2
    assert uc.hess_family(P["U6a"], 4, 256, hess_kernel=3) == 5 and uc.hess_family(P["U6b"], 4, 256, jit=0) == 2
    assert uc.hess_family(P["U6b"], 4, 256, hess_kernel=2, specialize=0) == 2
    # U7, U8: the specialised instances of kernel 3
    assert auto("U7a") == (31, 60, 5) and auto("U7b") == (20, 60, 5) and widths("U7a") == widths("U7b") == widths("U8") == (2, 2, 2)
    assert uc.v3_specialised(P["U7a"], 512) and not uc.v3_specialised(P["U7a"], 516) and not uc.v3_specialised(P["U7b"], 4)
    B, Nb = uc.BATCHES["U7a"]
    assert B * (Nb - 1) == 516 and uc.fused_family(P["U7a"], 516) == 20 and not uc.v1_auto(P["U7a"], 516) and uc.v1_auto(P["U7a"], 512)
    assert uc.fused_family(P["U7a"], 4, specialize=0) == 10 and uc.fused_family(P["U7a"], 4, kernel_version=3, specialize=0) == 30
    assert uc.fused_family(P["U7b"], 4, kernel_version=3) == 32 and uc.fused_wu(P["U7a"]) == 2
    assert auto("U8") == (31, 60, 4) and uc.hess_family(P["U8"], 4, 256, specialize=0) == 2 and uc.hess_family(P["U8"], 4, 256, hess_kernel=2) == 2
    assert P["U8"]["d"] % 2 == 1 and uc.hess3_lds_bytes(P["U8"]) == (50 * 50 + 16 * 50 * 16 + 10 + 8 * 15 + 8) * 8 + 64
    assert uc.eval_mfma_lds_bytes(P["U8"]) == (50 * 50 + 4 * 50 * 16 + 10 + 2) * 8 + 128
    # U9: general real drives, not antisymmetric
    assert auto("U9a") == (10, 60, 5) and auto("U9b") == (10, 60, 1) and widths("U9a") == (2, 2, 2) and widths("U9b") == (2, 3, 2)
    assert uc.hess_family(P["U9a"], 4, 256, hess_kernel=2) == 3 and uc.hess_family(P["U9a"], 4, 256, hess_kernel=2, specialize=0) == 2
    assert uc.hess_family(P["U9b"], 4, 256, hess_kernel=2) == "ESHAPE" and not uc.hess_v2_supported(P["U9b"])
    assert np.array_equal(uc.system("U9a")[0], uc.system("U9b")[0]) and (uc.system("U9a")[1] != uc.system("U9b")[1]).sum() == 2
    # U10: the union pattern's size and width
    assert (P["U10a"]["n_upos"], P["U10b"]["n_upos"], P["U10c"]["n_upos"]) == (1024, 1156, 24)
    assert (uc.fused_wu(P["U10a"]), uc.fused_wu(P["U10b"]), uc.fused_wu(P["U10c"])) == (2, -1, -1) and widths("U10c") == (1, 1, 3)
    assert (uc.eval_wu(P["U10a"]), uc.eval_wu(P["U10b"]), uc.eval_wu(P["U10c"])) == (2, -1, -1)
    assert auto("U10a") == (10, 60, 1) and auto("U10b") == (20, 60, 1) and auto("U10c") == (10, 60, 3)
    assert uc.fused_family(P["U10a"], 4, kernel_version=2) == 20 and uc.fused_family(P["U10a"], 4, kernel_version=3) == 30
    # U11 .. U13: d = 32
    assert auto("U11") == (20, 60, 5) and auto("U12") == (20, 60, 3) and auto("U13") == (20, 60, 1)
    assert uc.hess3_lds_bytes(P["U11"]) == 135728 <= uc.LDS_BYTES < uc.hess3_lds_bytes(P["U12"]) == 204784 and P["U12"]["uell_w"] <= 2
    for name in ("U11", "U12", "U13"):
        assert uc.fused_family(P[name], 4, kernel_version=3) == 20 and not uc.v3_fits(P[name])  # falls back
        for n_cu in (256, 304):
            assert uc.fused2_slices(P[name], 4, n_cu)[1] > 1, name  # column slices
    assert uc.ell_fits_lds(P["U12"]) and not uc.ell_fits_lds(P["U13"]) and 6 * 64 * 3 * 10 > 8192 >= 6 * 64 * 2 * 10
    assert widths("U13")[:2] == (3, 3) and uc.hess1_chunk(P["U13"]) == 2 and uc.hess1_chunk(P["U3"]) == 8
    assert uc.hess_lds_bytes(P["U13"], 4) > uc.LDS_BYTES // 2 >= uc.hess_lds_bytes(P["U13"], 2)
    # U14, U15: the pattern-compiled Hessian's tiles
    assert auto("U14") == (20, 60, 6) and auto("U15") == (20, 60, 3)
    assert uc.hess_sparse_lds_bytes(P["U14"]) == 158608 <= uc.LDS_BYTES and uc.hess_sparse_lds_bytes(P["U15"]) == 168768 > 166400 > uc.LDS_BYTES
    for name in ("U14", "U15"):
        assert not P[name]["v4"] and uc.v4_power_tiles(P[name]["d"], 5, 2) == 0 and uc.v4_power_tiles(P[name]["d"], 4 if name == "U14" else 3, 2) > 0
        assert uc.eval_family(P[name], 4, 256, eval_kernel=2) == 70 and uc.fused_family(P[name], 4, kernel_version=4) == "ESHAPE"
        assert uc.hess_family(P[name], 4, 256, hess_kernel=7) == uc.hess_family(P[name], 4, 256, hess_kernel=8) == "ESHAPE"
    assert uc.hess_family(P["U15"], 4, 256, hess_kernel=4) == "ESHAPE" and uc.hess_family(P["U14"], 4, 256, hess_kernel=4) == 6
    # U16: per-member drifts, the knot's layout
    lay = uc.layout("U16")
    assert auto("U16") == (20, 60, 5) and uc.fused_wu(P["U16"]) == -1 and uc.fused_wu(dict(P["U16"], per_member=False)) == 1
    assert uc.x_offs("U16") == [5, 805, 1605] and lay.u_off < lay.dt_off < lay.x_off and lay.x_off % 2 == 1 and uc.system("U16")[0].shape == (3, 40, 40)
    # the controlled systems: the drives' magnitudes as pcl_codegen counts them, the seeds
    for name in ("U4", "U14", "U15", "U17"):
        mags = uc.CASES[name][3][0]
        Gj = uc.system(name)[1]
        assert np.unique(np.round(np.abs(Gj[Gj != 0]), 12)).size == n_mags(mags) <= 7 and cf_pairs(mags) <= 16
        assert uc._first_ctl_seed(name, uc.CTL_BASE[name]) == uc.CTL_SEEDS[name]
    assert uc.RESEED == {"U5": 1}


@pytest.mark.parametrize("name", NAMES)
def test_steps(name):
    lay, (G0, Gj), Z = uc.layout(name), uc.system(name), uc.trajectory(name)
    th = [Z[k, lay.dt_off] * np.linalg.norm(uc.g_of(lay, Z, k, uc.member_G0(name), Gj), 2) for k in range(lay.K)]
    assert np.allclose(th, uc.STEPS, rtol=1e-12, atol=0) and Z[2, lay.dt_off] == 0.0
    # an interval of h = 0: the blocks are -I and I; the d/du tails, the (u, u) entries and the (u_l, X) rows are exact zeros in the truth
    d, j, mu, h = uc.truth(name)
    _, jl, hl = uc.labels(lay)
    assert np.array_equal(j[jl == "B+@2"], -np.tile(np.eye(lay.n).reshape(-1), lay.C)) and np.array_equal(j[jl == "B-@2"], np.tile(np.eye(lay.n).reshape(-1), lay.C))
    zero = [s for s in np.unique(hl) if not np.any(h[hl == s])] + [s for s in np.unique(jl) if not np.any(j[jl == s])]
    assert sorted(zero) == sorted(["du@2", "uu@2"] + ["u%d.Xk@2" % l for l in range(lay.m)] + ["Xk1.u%d@2" % l for l in range(lay.m)]), zero
    assert np.any(h[hl == "hh@2"]) and np.any(h[hl == "hu@2"]) and np.any(j[jl == "dh@2"])


# ---- the reference floor ----------------------------------------------------------------------------------------------------------------------------
def _floor(name, lay, G0, Gj, Z, ref, x_off=None):
    d, j, mu, h = ref
    rl, jl, hl = uc.labels(lay)
    er = check_segments(po.pade_residual(Z, lay, G0, Gj, 4, x_off), d, rl, FLOOR)
    ej = check_segments(po.pade_jacobian_values(Z, lay, G0, Gj, 4, x_off), j, jl, FLOOR)
    eh = check_segments(po.pade4_hessian_values(Z, mu.reshape(lay.K, -1), lay, G0, Gj, x_off), h, hl, FLOOR)
    for kind, e in (("residual", er), ("Jacobian", ej), ("Hessian", eh)):
        v, s = worst(e)
        if v > _floors.get(kind, (0.0,))[0]:
            _floors[kind] = (v, s, name)
    print("%s: residual %.1e (%s)  Jacobian %.1e (%s)  Hessian %.1e (%s)" % ((name,) + worst(er) + worst(ej) + worst(eh)))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_floor(name):
    lay, Gj, Z = uc.layout(name), uc.system(name)[1], uc.trajectory(name)
    for member in range(uc.MEMBERS.get(name, 1)):
        _floor(name, lay, uc.member_G0(name, member), Gj, Z, uc.truth(name, member=member), uc.x_offs(name)[member])
    print("reference floor so far: " + "  ".join("%s %.1e (%s, %s)" % ((k,) + v) for k, v in _floors.items()))


def test_oracle_floor_of_the_other_launches():
    """The -1.7 u trajectories of the controls-back-and-forth test, and samples of the launches of several trajectories."""
    for name in ("U4", "U8", "U14"):
        lay, (G0, Gj) = uc.layout(name), uc.system(name)
        Z, mu = uc.flipped(name), uc.rand_mu(name)
        _floor(name + " (-1.7 u)", lay, G0, Gj, Z, uc.flipped_truth(name))
    for batch, hessian in (("U4", True), ("U5b", False), ("U7a", False)):
        name = "U5" if batch.startswith("U5") else batch
        B, Nb = uc.BATCHES[batch]
        lay, (G0, Gj) = uc.layout(name, Nb), uc.system(name)
        Zs, ds, js, mus, hs = uc.batch_truth(batch, hessian)
        rl, jl, hl = uc.labels(lay)
        for s in (0, B // 2, B - 1):
            check_segments(po.pade_residual(Zs[s], lay, G0, Gj, 4), ds[s], rl, FLOOR)
            check_segments(po.pade_jacobian_values(Zs[s], lay, G0, Gj, 4), js[s], jl, FLOOR)
            if hessian:
                check_segments(po.pade4_hessian_values(Zs[s], mus[s].reshape(lay.K, -1), lay, G0, Gj), hs[s], hl, FLOOR)


def test_check_segments_batch_is_check_segments_per_trajectory():
    Zs, ds, js, mus, hs = uc.batch_truth("U4", True)
    lay = uc.layout("U4", uc.BATCHES["U4"][1])
    hl = uc.labels(lay)[2]
    bad = np.array(hs)
    bad *= 1 + 3e-12
    worst_b = uc.check_segments_batch(bad, hs, hl, GPU_TOL)
    per = [check_segments(bad[s], hs[s], hl, GPU_TOL) for s in range(0, len(hs), 17)]
    assert all(worst_b[k] >= max(p[k] for p in per) for k in worst_b) and max(worst_b.values()) < 4e-12
    i = int(np.flatnonzero(hl == "uu@3")[0])
    bad[57, i] += 1e-10 * abs(hs[57, i])  # one scalar of one trajectory
    with pytest.raises(AssertionError, match="trajectory 57, segment uu@3"):
        uc.check_segments_batch(bad, hs, hl, GPU_TOL)
    with pytest.raises(AssertionError, match="segment uu@3"):
        check_segments(bad[57], hs[57], hl, GPU_TOL)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fault_sensitivity(name):
    lay, Gj, Z = uc.layout(name), uc.system(name)[1], uc.trajectory(name)
    member = uc.MEMBERS.get(name, 1) - 1
    G0, xo = uc.member_G0(name, member), uc.x_offs(name)[member]
    d, j, mu, h = uc.truth_ld(name, member=member)
    _, jl, hl = uc.labels(lay)
    c0 = uc.vc.coeffs(4)
    c0[2] = 0
    faults = {"c_2 = 0": dict(c=c0), "last drive": dict(drop_drive=True), "last state column": dict(drop_col=True), "last row of a product": dict(mm=uc.mm_last_row),
              "last column of a product": dict(mm=uc.mm_last_col), "last inner index of a product": dict(mm=uc.mm_last_inner)}  # fmt: skip
    for what, kw in faults.items():
        bd, bj, bh = uc.truth_of(lay, G0, Gj, Z, mu, x_off=xo, **kw)
        sj, sh = uc.seen(j, bj, jl), uc.seen(h, bh, hl)
        if what == "last state column":  # its own rows move by all they hold: ask the sums over the columns, the scalar entries
            scal = np.isin(np.char.partition(hl, "@")[:, 0], ("uu", "hu", "hh"))
            sh = uc.seen(h[scal], bh[scal], hl[scal])
        print("%s, %s: Jacobian moved by %.1e, Hessian by %.1e" % (name, what, sj, sh))
        assert sj >= SEEN and sh >= SEEN, (name, what, sj, sh)


@pytest.mark.parametrize("name", NAMES)
def test_segments_that_matter(name):
    """A (u, u) or (h, u) segment below 0.1 of its interval's largest Hessian segment: a bound relative to the whole array's maximum (floored at 1)
    lets such a segment be wrong by many times its size."""
    lay = uc.layout(name)
    h, hl = uc.truth(name)[3], uc.labels(lay)[2]
    ratios = []
    for k in range(lay.K):
        if uc.STEPS[k] == 0.0:
            continue
        seg = {s: np.abs(h[hl == s]).max() for s in np.unique(hl) if s.endswith("@%d" % k)}
        ratios.append(min(seg["uu@%d" % k], seg["hu@%d" % k]) / max(seg.values()))
    print("%s: smallest scalar segment / largest segment of its interval: %s" % (name, " ".join("%.1e" % r for r in ratios)))
    assert min(ratios) < 0.1, (name, ratios)


def test_every_family_runs_on_two_cases():
    """By the launch rules, over `auto` and the documented options: each family of the order-4 ladders is reached by at least two cases
    (tests/test_unitary4_shapes_gpu.py asserts the kernel that really ran against the same rules)."""
    fused, hess = {}, {}
    for name in NAMES:
        p, items = uc.props(name), 4 * uc.MEMBERS.get(name, 1)
        for kv in range(6):
            for spec in (0, 1):
                fused.setdefault(uc.fused_family(p, items, kernel_version=kv, specialize=spec), set()).add(name)
            for ek in range(4):
                fused.setdefault(uc.eval_family(p, items, 256, eval_kernel=ek, kernel_version=kv), set()).add(name)
        for hk in (0, 1, 2, 3, 4, 7, 8):
            for spec in (0, 1):
                hess.setdefault(uc.hess_family(p, items, 256, hess_kernel=hk, specialize=spec), set()).add(name)
    for batch, (B, Nb) in uc.BATCHES.items():
        name = "U5" if batch.startswith("U5") else batch
        fused.setdefault(uc.fused_family(uc.props(name), B * (Nb - 1)), set()).add(batch)
        hess.setdefault(uc.hess_family(uc.props(name), B * (Nb - 1), 256), set()).add(batch)
    for fam in (10, 20, (30, 31, 32), 42, 52, 60, 70, 82):
        cases = set().union(*(fused.get(k, set()) for k in (fam if isinstance(fam, tuple) else (fam,))))
        assert len(cases) >= 2, (fam, cases)
    for k in (30, 31, 32):
        assert fused.get(k), k
    for fam in (1, (2, 3), (4, 5), 6, 72, 82):
        cases = set().union(*(hess.get(k, set()) for k in (fam if isinstance(fam, tuple) else (fam,))))
        assert len(cases) >= 2, (fam, cases)
    for k in (2, 3, 4, 5):
        assert hess.get(k), k
