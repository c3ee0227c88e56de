"""What the option var_compact rests on, without a GPU (layouts, cases and comparison: tests/var_compact_cases.py): the fold and the expansion
of both compact layouts on the oracle's Jacobian values, that the fold hides no wrong copy, that the GPU test's comparison sees the faults such
a launch can have, the host mirror's keyword, and the host expanders in a stand-alone program.

The oracle's own copies.  The oracle computes the lifted problem, so what the library replicates -- -B+, B- (or -E) of component 0 and of every
variation -- are separate diagonal blocks of one (1 + v) n square matrix function there, and they differ in their last bits in 15 of the 29
cases (measured: at most 2e-16 of the largest value).  `compact_of_full` refuses such values, as it must.  The round trip is therefore asked of
the oracle's values with every folded copy set to the oracle's first copy of its tile -- an array in the full layout, within ROUND x scale of
the raw values -- and the raw values must either pass bit for bit or be refused."""
import os
import subprocess

import numpy as np
import pytest

import piccolo_jl_amd as pa
import var_compact_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = 1e-14  # copy-to-copy rounding of the oracle's lifted matrix functions: a few dozen ulps (2.2e-16) of the largest value at most


def _oracle(name, order):
    case = vc.built(name)[3]
    kw = vc.of_case(case, order == "exp")
    vals, scale = vc.truth(name, order)
    return case, kw, vals, scale


def _first_copies(vals, n, C, v, m, expo):
    """The oracle's values with every folded copy replaced by the first copy of its tile (no check: that is compact_of_full's part)."""
    K, nn, ns = vals.shape[0], n * n, vc.n_segments(v, expo)
    out = vals.copy()
    seg = out[:, : ns * C * nn].reshape(K, ns, C, nn)
    first = {}
    for s in range(ns):
        t = vc.tile_of_segment(s, expo)
        first.setdefault(t, seg[:, s, 0].copy())
        seg[:, s] = first[t][:, None, :]
    return out


@pytest.mark.parametrize("name, order", vc.ALL_CASES, ids=[vc.case_id(p) for p in vc.ALL_CASES])
def test_fold_and_expansion_on_the_oracle_values(name, order):
    case, kw, vals, scale = _oracle(name, order)
    K = case.K
    assert vals.shape == (K, vc.full_per(**kw))
    n, C, v, m = kw["n"], kw["C"], kw["v"], kw["m"]
    if kw["expo"]:
        assert vc.full_per(**kw) == (1 + 2 * v) * C * n * n + case.xd * (m + 2) and vc.compact_per(**kw) == (1 + v) * n * n + case.xd * (m + 1)
    else:
        assert vc.full_per(**kw) == (2 + 4 * v) * C * n * n + case.xd * (m + 1) and vc.compact_per(**kw) == (2 + 2 * v) * n * n + case.xd * (m + 1)
    full = _first_copies(vals, **kw)
    worst = np.abs(full - vals).max()
    print("%s: the oracle's copies differ by %.2e of the largest value" % (vc.case_id((name, order)), worst / scale))
    assert worst <= ROUND * scale
    comp = vc.compact_of_full(full, **kw)
    assert comp.shape == (K, vc.compact_per(**kw))
    assert vc.same_bits(vc.expand_compact(comp, **kw), full)
    assert vc.same_bits(vc.compact_of_full(vc.expand_compact(comp, **kw), **kw), comp)
    # the raw values: the same bits, or refused -- never folded quietly
    if vc.same_bits(full, vals):
        assert vc.same_bits(vc.expand_compact(vc.compact_of_full(vals, **kw), **kw), vals)
    else:
        with pytest.raises(ValueError, match="differs from the tile"):
            vc.compact_of_full(vals, **kw)
    # what the expansion adds and what it keeps
    nt, ns, nn = vc.n_tiles(v, kw["expo"]), vc.n_segments(v, kw["expo"]), n * n
    t = vc.tail_len(n, C, v, m)
    assert vc.same_bits(full[:, -t:], comp[:, nt * nn :])
    if kw["expo"]:
        assert np.array_equal(full[:, ns * C * nn : ns * C * nn + case.xd], np.ones((K, case.xd)))


_FOLD = [("config2_v2", 4), ("config2_v2", "exp"), ("pauli_ket", 4), ("pauli_ket", "exp")]


@pytest.mark.parametrize("name, order", _FOLD, ids=[vc.case_id(p) for p in _FOLD])
def test_the_fold_hides_no_wrong_copy(name, order):
    """One bit in any one copy of any segment, or in any one of the ones, makes compact_of_full raise."""
    case, kw, vals, _ = _oracle(name, order)
    full = _first_copies(vals, **kw)
    vc.compact_of_full(full, **kw)
    n, C, v = kw["n"], kw["C"], kw["v"]
    nn = n * n
    segs = range(vc.n_segments(v, kw["expo"]))
    for s in segs:
        copies = C * sum(vc.tile_of_segment(q, kw["expo"]) == vc.tile_of_segment(s, kw["expo"]) for q in segs)
        for c in range(C):
            if copies == 1:  # (a ket's -L+_i, L-_i, -L_i: one copy, nothing is folded away)
                continue
            bad = full.copy()
            e = (s * C + c) * nn + (s + 3 * c) % nn
            bad[case.K - 1, e] = np.nextafter(bad[case.K - 1, e], np.inf)
            with pytest.raises(ValueError, match="differs from the tile"):
                vc.compact_of_full(bad, **kw)
    if kw["expo"]:
        bad = full.copy()
        bad[0, vc.n_segments(v, True) * C * nn + case.xd - 1] = np.nextafter(1.0, 2.0)
        with pytest.raises(ValueError, match="not 1.0"):
            vc.compact_of_full(bad, **kw)
        bad[0, vc.n_segments(v, True) * C * nn + case.xd - 1] = -0.0
        with pytest.raises(ValueError, match="not 1.0"):
            vc.compact_of_full(bad, **kw)
    with pytest.raises(ValueError, match="shape"):
        vc.compact_of_full(full[:, :-1], **kw)


FAULTS = {"drop_copy": vc.fault_drop_copy, "swap_L": vc.fault_swap_L, "missing_one": vc.fault_missing_one, "shift_tail": vc.fault_shift_tail}
# (the Pade layout has no ones)
_FAULT_CASES = [(nm, o, f) for nm, o in [("config2_v2", 4), ("config2_v2", "exp"), ("config3_v1", 4), ("config3_v1", "exp")] for f in FAULTS if o == "exp" or f != "missing_one"]


@pytest.mark.parametrize("name, order, fault", _FAULT_CASES, ids=["%s-%s-%s" % p for p in _FAULT_CASES])
def test_the_comparison_sees_each_fault(name, order, fault):
    """The GPU test compares bit for bit with the full launch (same_bits) and with the truth (matches): each fault fails both.  The tail shifted by
    one state column moves values by far more than the tolerance: the factor is printed."""
    case, kw, vals, scale = _oracle(name, order)
    full = _first_copies(vals, **kw)
    comp = vc.compact_of_full(full, **kw)
    good = vc.expand_compact(comp, **kw)
    assert vc.same_bits(good, full) and vc.matches(good, name, order)[0]
    bad = FAULTS[fault](comp, full, **kw)
    assert bad.shape == full.shape
    assert not vc.same_bits(bad, full)
    ok, err = vc.matches(bad, name, order)
    print("%s %s: worst error %.2e = %.1e x the tolerance" % (vc.case_id((name, order)), fault, err, err / (vc.TOL * scale)))
    assert not ok


def test_var_compact_keyword_needs_a_variational_context():
    """ValueError before any device call (no library is loaded, no context is created); the message names the option."""
    args = dict(d=2, m=2, N=4, z_dim=12, u_off=10, dt_off=8, x_offs=[0], G0=np.zeros((4, 4)), Gj=np.zeros((2, 4, 4)), batch=1)
    for order in (4, 0, 10, "exp"):
        with pytest.raises(ValueError, match="var_compact"):
            pa.integrators._PclContext(pade_order=order, var_compact=True, batch_mode=pa._lib.PCL_BATCH_MEMBERS, **args)
        with pytest.raises(ValueError, match="var_compact"):
            pa.HipPadeIntegrator(None, None, None, pade_order=order, var_compact=True)
        with pytest.raises(ValueError, match="var_compact"):
            pa.BilinearIntegrator(pa.QuantumSystem(0.5 * pa.PAULIS["Z"], [pa.PAULIS["X"]], [1.0]), None, pade_order=order, var_compact=True)
    with pytest.raises(ValueError, match="var_compact"):
        pa.integrators._PclContext(pade_order=4, var_compact=True, batch_mode=pa._lib.PCL_BATCH_TRAJ, **args)
    for mode in (pa._lib.PCL_BATCH_VARIATIONAL, pa._lib.PCL_BATCH_VARIATIONAL_EXP):
        pa.integrators._check_services(mode, var_compact=True)
    pa.integrators._check_services(var_compact=False)
    pa.integrators._check_services(pa._lib.PCL_BATCH_TRAJ, var_compact=0)


def test_host_expanders_in_a_standalone_program(tmp_path):
    """tests/var_compact_host_expand.cpp: expand_interval_var / expand_interval_var_exp, both halves, every store width of this host, four
    shapes, against a plain loop and between guard words.  ROCm's clang: the header uses clang's vector types."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    clang = os.path.join(os.path.dirname(hipcc), "amdclang++")
    exe = str(tmp_path / "var_compact_host_expand")
    r = subprocess.run([clang if os.path.exists(clang) else hipcc, "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "piccolo.jl_amd", "csrc"),
                        os.path.join(ROOT, "tests", "var_compact_host_expand.cpp"), "-o", exe], capture_output=True, text=True)  # fmt: skip
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert "FAIL" not in r.stdout and " 0 failures" in r.stdout
    assert r.stdout.count("ok   expand_interval_var ") >= 4 and r.stdout.count("ok   expand_interval_var_exp") >= 4
