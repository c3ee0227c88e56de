"""Cases that walk the order-4 kernels of the square unitary state (state_cols = 0, pade_order = 4: what bench.py measures) over the sizes at
which the launch ladders branch (piccolo.jl_amd/csrc/piccolo_hip.hip pcl_create, pcl_host_launch_pade.hpp, pcl_host_launch_hess.hpp);
importable without a GPU.

Knot [X | dt | t | u], u ~ 0.4 N(0, 1), X ~ 0.4 N(0, 1), N = 5 unless stated.  The steps are fixed per interval k from |G(u_k)|_2, cycling
through STEPS: h |G|_2 = 0.15, -0.3, 0 exactly, 0.5.  At h = 0 the d/du tails, the (u, u) entries and the (u_l, X) rows are identically zero
and must be read as exact zeros.

Systems, from fixed seeds:
    ctl    shape_cases.controlled_system: sparse exact-iso generators, what the pattern-compiled kernels take
    iso    a dense complex Hermitian drift (no pattern-compiled kernel: the union pattern is full) with sparse iso drives: every drive pairs
           the levels off (a matching) and puts one entry H[i, j] on each pair -- real or imaginary (one entry per row and column of G_l:
           width 1), complex (width 2), complex plus a second, real matching (width 3).  iso(-iH) of a Hermitian H is antisymmetric.
    real   general real n x n generators / sqrt(n) (iso_structured 0): the drives are sums of two permutation patterns (two entries per row
           and column, not antisymmetric) or fully dense

Cases (kind, d, m) and the branch each straddles -- tests/test_unitary4_shapes_cpu.py recomputes every claim with the launch code's
arithmetic restated below (props, fused_family, eval_family, hess_family and the byte formulas):
    U1   iso   4  2  width 1   n = 8: the small kernel's 8-row instance for eval_jac and eval (52); kernels 10, 20 forced; Hessian 2 (d < 12)
    U2   iso   5  2  width 1   n = 10, odd d: eval on the 16-row instance (52), eval_jac on kernel 10 (v1_auto: d <= 8)
    U3   iso   8  8  width 1   the last small size, the small kernel's most drives; m > 6: hess_v2_supported false, Hessian kernel 1
    U4   ctl   9  1            smallest pattern-compiled d.  One trajectory: 42 / 82 / Hessian 82 (2 batch K <= n_cu); forced hess_kernel 4
                               (reads 6), 7 (72), 3 (5), 1; eval_kernel 2 (70), 1 (60); kernel_version 3 (32), 2, 1.  103 seeds x N = 6
                               (515 intervals): launch_eval_sparse with nw = 3 waves per workgroup and an idle wave in the last one, the
                               Hessian rule flips to kernel 6, balanced_grid walks three intervals per workgroup
    U5   iso  10  1  width 1   128 seeds (512 intervals): kernel 10; 129 seeds (516): kernel 20, its persistent grid wraps -- the two
                               sides of d <= 16 && win_count K <= 512
    U6a  iso  11  2  width 1   Hessian auto: kernel 2 (d < 12)
    U6b  iso  12  2  width 1   Hessian auto: version 3 compiled on first use (5); hess_kernel 2 reads 3
    U7a  iso  16  4  width 2   v3_specialised holds: 31.  172 seeds x N = 4 (516 intervals): it and v1_auto stop holding: kernel 20
    U7b  iso  17  4  width 2   v3_specialised does not hold: 20
    U8   iso  25  4  width 2   the static instances: 31 and Hessian 4; odd d: lde = n in launch_eval_mfma and hess3_lds_bytes
    U9a  real 14  3  2 + 2     drives not antisymmetric: the ANTI = false instances of Hessian versions 2 and 3 (no iso system runs them)
    U9b  real 14  3            U9a with one entry moved: three entries in one column (ellt_w = 3, ell_w = 2): kernel 1; hess_kernel = 2 refused
    U10a real 16  2  dense     n_upos = 1024 exactly, uell_w = 2: wu = 2 in launch_fused_v12 and launch_eval_mfma
    U10b real 17  2  dense     n_upos = 1156: wu = -1
    U10c iso  12  3  width 1   three drives on the same positions (uell_w = 3): wu = -1 at a small n_upos
    U11  iso  32  2  width 2   hess3_lds_bytes 135,728 B fits: Hessian 5; kernel 20 with S > 1 column slices; kernel_version 3 falls back
    U12  iso  32  6  width 2   hess3_lds_bytes 204,784 B is declined: Hessian version 2 (reads 3)
    U13  iso  32  6  width 3   ell_fits_lds false (6 64 3 10 B > 8192); ell_w = 3: Hessian kernel 1, its column chunk halved to 2
    U14  ctl  31  5            hess_sparse_lds_bytes 158,608 B fits: Hessian 6
    U15  ctl  32  5            168,768 B does not: hess_kernel = 4 refused with the byte counts, auto goes on; the residual kernel 70 still runs
    U16  iso  20  2  width 1   PCL_BATCH_MEMBERS, M = 3 with per-member drifts (wu = -1 in kernel 20), member window (1, 2), the controls
                               before the state and the first state offset odd (knot [pad | u | dt | t | X_0 | X_1 | X_2])
    U17  ctl  13  2            (added to the issue's table) a second system that the whole pattern-compiled family takes -- U14 and U15 have
                               no LDS for kernel 4's tiles at m = 5 -- so that 42, 82, 72 and Hessian 82 run on two cases; m = 2: hess_split

Shapes that moved: none; the seeds of U4, U14, U15 and U17 are the first ones from their base at which the drives keep two entries per row
and column (Hessian versions 2 and 3 take them, kernel_version 3 compiles its instance) -- a property of the system, asserted by the CPU test.
One case was reseeded for a near-cancelling scalar segment (RESEED): U5's first draw has (h, h) of the h = 0 interval, 2 c_2 <M, G^2 (X_k+1 -
X_k)>, at 0.038 -- 200 products of size one cancel -- where the float64 oracle itself reads 1.1e-13 of the segment against the truth, above the
1e-13 the CPU test asks of the inputs; the next seed is taken.

The truth is vector_shape_cases.truth_values at order 4 (np.longdouble, no code shared with oracle/pade_oracle.py), rounded to float64."""
import functools

import numpy as np

import vector_shape_cases as vc
from oracle import pade_oracle as po
from shape_cases import cf_pairs, controlled_system, hess_labels, jac_labels, per_interval, union_nz

ORDER = 4
N = 5
STEPS = (0.15, -0.3, 0.0, 0.5)
LDS_BYTES = 163840
SEEN = 1e-7

# name: (kind, d, m, parameters)   ctl: (drive magnitudes, unused)   iso: (width, shared positions)   real: "two" | "col3" | "dense"
CASES = {
    "U1": ("iso", 4, 2, (1, False)), "U2": ("iso", 5, 2, (1, False)), "U3": ("iso", 8, 8, (1, False)), "U4": ("ctl", 9, 1, ([[0, 1]], 0)),
    "U5": ("iso", 10, 1, (1, False)), "U6a": ("iso", 11, 2, (1, False)), "U6b": ("iso", 12, 2, (1, False)), "U7a": ("iso", 16, 4, (2, False)),
    "U7b": ("iso", 17, 4, (2, False)), "U8": ("iso", 25, 4, (2, False)), "U9a": ("real", 14, 3, "two"), "U9b": ("real", 14, 3, "col3"),
    "U10a": ("real", 16, 2, "dense"), "U10b": ("real", 17, 2, "dense"), "U10c": ("iso", 12, 3, (1, True)), "U11": ("iso", 32, 2, (2, False)),
    "U12": ("iso", 32, 6, (2, False)), "U13": ("iso", 32, 6, (3, False)), "U14": ("ctl", 31, 5, ([[0], [1], [2], [0, 1], [3]], 0)),
    "U15": ("ctl", 32, 5, ([[0], [1], [2], [0, 1], [3]], 0)), "U16": ("iso", 20, 2, (1, False)), "U17": ("ctl", 13, 2, ([[0, 1], [2]], 0)),
}  # fmt: skip
MEMBERS = {"U16": 3}
# the launches of several trajectories: name -> (seeds, N)
BATCHES = {"U4": (103, 6), "U5a": (128, 5), "U5b": (129, 5), "U7a": (172, 4)}
# a case whose scalar segment near-cancels draws from another seed: name -> how many seeds further
RESEED = {"U5": 1}


def _seed(name):
    tail = name[1:]
    num, let = (int(tail[:-1]), "abc".index(tail[-1]) + 1) if tail[-1].isalpha() else (int(tail), 0)
    return 41000 + 37 * num + 7 * let + 5 * RESEED.get(name, 0)


# ---- systems ----------------------------------------------------------------------------------------------------------------------------------
def _herm(d, rng):
    A = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return (A + A.conj().T) / 2


def _matching_drive(d, width, rng, perm, kinds=None):
    """A Hermitian H with one entry on every pair (perm[0], perm[1]), (perm[2], perm[3]), ..: real or imaginary (kinds; width 1), complex
    (width 2); width 3: and a real entry on every pair (perm[1], perm[2]), (perm[3], perm[4]), ..  Returns (H, kinds)."""
    H = np.zeros((d, d), dtype=complex)
    kinds = rng.integers(0, 2, d // 2) if kinds is None else kinds
    for p in range(d // 2):
        i, j = perm[2 * p], perm[2 * p + 1]
        re, im = 0.5 + rng.random(), 0.5 + rng.random()
        v = (re * rng.choice([1.0, -1.0]) + 1j * im * rng.choice([1.0, -1.0])) if width >= 2 else (re if kinds[p] else 1j * im) * rng.choice([1.0, -1.0])
        H[i, j], H[j, i] = v, np.conj(v)
    if width == 3:
        for p in range((d - 1) // 2):
            i, j = perm[2 * p + 1], perm[2 * p + 2]
            H[i, j] = H[j, i] = (0.5 + rng.random()) * rng.choice([1.0, -1.0])
    return H, kinds


def _two_pattern_drive(n, rng):
    """Two entries in every row and column, on two permutation patterns without a common position."""
    p1 = rng.permutation(n)
    p2 = np.roll(p1, 1)
    G = np.zeros((n, n))
    G[np.arange(n), p1] = rng.standard_normal(n)
    G[np.arange(n), p2] = rng.standard_normal(n)
    return G


@functools.lru_cache(maxsize=None)
def system(name):
    """(G0, Gj), read-only; G0 is [M, n, n] for a case of MEMBERS."""
    kind, d, m, par = CASES[name]
    n = 2 * d
    if kind == "ctl":
        mags = par[0]
        G0, Gj = controlled_system(d, mags, np.random.default_rng(CTL_SEEDS[name]), "classes")
    elif kind == "iso":
        width, shared = par
        rng = np.random.default_rng(_seed(name))
        G0 = np.array([po.G_of_H(_herm(d, rng)) for _ in range(MEMBERS.get(name, 1))])
        G0 = G0 if name in MEMBERS else G0[0]
        perm, kinds, Hs, used = rng.permutation(d), None, [], np.zeros((d, d), dtype=int)
        for _ in range(m):
            H, k = _matching_drive(d, width, rng, perm, kinds)
            Hs.append(H)
            used += H != 0
            if shared:
                kinds = k
            else:  # the next drive's pairs: at most two drives meet in one position (uell_w <= 2) where the widths are 1 or 2
                perm = rng.permutation(d)
                while width <= 2 and len(Hs) < m and (used + (_matching_drive(d, 1, np.random.default_rng(0), perm)[0] != 0)).max() > 2:
                    perm = rng.permutation(d)
        Gj = np.array([po.G_of_H(H) for H in Hs])
    else:
        rng = np.random.default_rng(_seed("U9a" if name == "U9b" else name))
        G0 = rng.standard_normal((n, n)) / np.sqrt(n)
        if par == "dense":
            Gj = rng.standard_normal((m, n, n)) / np.sqrt(n)
        else:
            Gj = np.array([_two_pattern_drive(n, rng) for _ in range(m)])
            if par == "col3":  # one entry of the last drive's row 0 moves into a column that row 0 does not use: that column holds three
                g = Gj[-1]
                c_from = np.flatnonzero(g[0])[0]
                c_to = next(c for c in range(n) if g[0, c] == 0)
                g[0, c_to], g[0, c_from] = g[0, c_from], 0.0
    for a in (G0, Gj):
        a.setflags(write=False)
    return G0, Gj


def _widths(Gj):
    nz = np.asarray(Gj) != 0
    return int(nz.sum(axis=2).max()), int(nz.sum(axis=1).max())


def _first_ctl_seed(name, base):
    """The first seed from `base` at which controlled_system's drives keep two entries per row and column."""
    kind, d, m, (mags, _) = CASES[name]
    for s in range(base, base + 200):
        if max(_widths(controlled_system(d, mags, np.random.default_rng(s), "classes")[1])) <= 2:
            return s
    raise AssertionError(name)


# (found by _first_ctl_seed from 7100 + the case's number; tests/test_unitary4_shapes_cpu.py asserts that they still are)
CTL_BASE = {"U4": 7104, "U14": 7114, "U15": 7115, "U17": 7117}
CTL_SEEDS = {"U4": 7105, "U14": 7114, "U15": 7115, "U17": 7118}


def layout(name, n_knots=N):
    kind, d, m, par = CASES[name]
    xd = 2 * d * d
    if name in MEMBERS:  # [pad | u | dt | t | X_0 | X_1 | ..]: the controls before the state, the first state offset odd
        M = MEMBERS[name]
        return po.Layout(d=d, m=m, N=n_knots, z_dim=1 + m + 2 + M * xd, x_off=1 + m + 2, u_off=1, dt_off=1 + m)
    return po.Layout(d=d, m=m, N=n_knots, z_dim=xd + 2 + m, x_off=0, u_off=xd + 2, dt_off=xd)


def x_offs(name):
    lay = layout(name)
    return [lay.x_off + i * lay.x_dim for i in range(MEMBERS.get(name, 1))]


def g_of(lay, Z, k, G0, Gj):
    return G0 + np.tensordot(Z[k, lay.u_off : lay.u_off + lay.m], Gj, axes=1)


@functools.lru_cache(maxsize=None)
def trajectory(name, seed=0, n_knots=N):
    """Z [N, z_dim], read-only.  seed: another trajectory of the same system (a seed of a PCL_BATCH_TRAJ launch).  The members of a
    PCL_BATCH_MEMBERS launch share the knots: the steps are fixed from member 0's drift."""
    lay = layout(name, n_knots)
    G0, Gj = system(name)
    G0 = G0[0] if name in MEMBERS else G0
    rng = np.random.default_rng(_seed(name) + 1000 + seed)
    Z = 0.4 * rng.standard_normal((n_knots, lay.z_dim))
    for k in range(lay.K):
        th = STEPS[k % len(STEPS)]
        Z[k, lay.dt_off] = th / np.linalg.norm(g_of(lay, Z, k, G0, Gj), 2) if th else 0.0
    Z[n_knots - 1, lay.dt_off] = 0.1
    Z[:, lay.dt_off + 1] = np.cumsum(Z[:, lay.dt_off])
    Z.setflags(write=False)
    return Z


def rand_mu(name, seed=0, n_knots=N, member=0):
    lay = layout(name, n_knots)
    mu = np.random.default_rng(_seed(name) + 5000 + 10 * seed + member).standard_normal(lay.K * lay.x_dim)
    mu.setflags(write=False)
    return mu


def member_G0(name, member=0):
    G0 = system(name)[0]
    return G0[member] if name in MEMBERS else G0


def residual_labels(lay):
    return per_interval(np.full(lay.x_dim, "delta"), lay.K)


def labels(lay):
    return residual_labels(lay), jac_labels(lay), hess_labels(lay)


# ---- the truth -----------------------------------------------------------------------------------------------------------------------------------
def truth_of(lay, G0, Gj, Z, mu, x_off=None, **kw):
    """(delta, Jacobian values, Hessian values | None), flat, in longdouble (vector_shape_cases.truth_values at order 4)."""
    return tuple(None if a is None else a.reshape(-1) for a in vc.truth_values(lay, G0, Gj, Z, mu, ORDER, x_off=x_off, **kw))


@functools.lru_cache(maxsize=None)
def truth_ld(name, seed=0, n_knots=N, member=0):
    """(delta, Jacobian values, mu, Hessian values) of one member in longdouble; computed once and never written to."""
    lay = layout(name, n_knots)
    mu = rand_mu(name, seed, n_knots, member)
    d, j, h = truth_of(lay, member_G0(name, member), system(name)[1], trajectory(name, seed, n_knots), mu, x_off=x_offs(name)[member])
    for a in (d, j, h):
        a.setflags(write=False)
    return d, j, mu, h


@functools.lru_cache(maxsize=None)
def truth(name, seed=0, n_knots=N, member=0):
    """The same rounded to float64: what the GPU tests compare with."""
    d, j, mu, h = truth_ld(name, seed, n_knots, member)
    out = d.astype(np.float64), j.astype(np.float64), mu, h.astype(np.float64)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def flipped(name):
    """The case's trajectory with the controls at -1.7 u (the steps stay): the second launch of the controls-back-and-forth test."""
    lay = layout(name)
    Z = np.array(trajectory(name))
    Z[:, lay.u_off : lay.u_off + lay.m] *= -1.7
    Z.setflags(write=False)
    return Z


@functools.lru_cache(maxsize=None)
def flipped_truth(name):
    mu = rand_mu(name)
    d, j, h = truth_of(layout(name), member_G0(name), system(name)[1], flipped(name), mu)
    return d.astype(np.float64), j.astype(np.float64), mu, h.astype(np.float64)


@functools.lru_cache(maxsize=None)
def batch_truth(batch, hessian=False):
    """(Z [B, N, z_dim], delta [B, ..], Jacobian values [B, ..], mu [B, ..] | None, Hessian values [B, ..] | None) of a launch of BATCHES, in float64."""
    name = batch[:2] if batch[:2] == "U5" else batch
    B, n_knots = BATCHES[batch]
    lay = layout(name, n_knots)
    G0, Gj = system(name)
    Zs, ds, js, mus, hs = [], [], [], [], []
    for s in range(B):
        Z = trajectory(name, s, n_knots)
        mu = rand_mu(name, s, n_knots) if hessian else None
        d, j, h = truth_of(lay, G0, Gj, Z, mu, hessian=hessian)
        Zs.append(Z), ds.append(d.astype(np.float64)), js.append(j.astype(np.float64))
        if hessian:
            mus.append(mu), hs.append(h.astype(np.float64))
    out = np.stack(Zs), np.stack(ds), np.stack(js), (np.stack(mus) if hessian else None), (np.stack(hs) if hessian else None)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def check_segments_batch(ours, ref, layout, tol):
    """shape_cases.check_segments for every trajectory of a launch at once (ours, ref: [B, values]; layout: the labels of one trajectory): the
    same rule -- max|a - b| <= tol max|ref segment|, no floor -- per trajectory and segment.  Returns {segment: largest relative error}."""
    a, b, lab = np.asarray(ours), np.asarray(ref), np.asarray(layout).reshape(-1)
    assert a.shape == b.shape and a.ndim == 2 and a.shape[1] == lab.size, (a.shape, b.shape, lab.shape)
    assert np.all(np.isfinite(a)), "non-finite values"
    out = {}
    for s in np.unique(lab):
        sel = np.flatnonzero(lab == s)
        scale, err = np.abs(b[:, sel]).max(axis=1), np.abs(a[:, sel] - b[:, sel]).max(axis=1)
        bad = np.flatnonzero(err > tol * scale)
        assert bad.size == 0, "trajectory %d, segment %s: max err %.3e, max |ref| %.3e (> %.1e relative)" % (bad[0], s, err[bad[0]], scale[bad[0]], tol)
        out[str(s)] = float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), err)))
    return out


# ---- the launch code's arithmetic ---------------------------------------------------------------------------------------------------------------
def lds_ld(n):
    return ((n + 3) & ~3) + 2


@functools.lru_cache(maxsize=None)
def props(name):
    """What pcl_create reads off the matrices: n_upos, uell_w, ell_w, ellt_w, drives_antisym, iso, sp_plan, v4_plan (order 4), and whether the
    column-group Hessian kernel takes the drives' magnitudes."""
    kind, d, m, par = CASES[name]
    n = 2 * d
    G0, Gj = system(name)
    G0s = G0 if name in MEMBERS else G0[None]
    nz = Gj != 0
    union = nz.any(axis=0)
    ell_w, ellt_w = _widths(Gj)
    is_iso = lambda A: np.array_equal(A[d:, d:], A[:d, :d]) and np.array_equal(A[:d, d:], -A[d:, :d])
    iso = all(is_iso(A) for A in G0s) and all(is_iso(A) for A in Gj)
    sp = v4 = hc = False
    if iso and 9 <= d <= 32 and 1 <= m <= 6:
        nzu = max(union_nz(A, Gj) for A in G0s)
        mags = np.unique(np.round(np.abs(Gj[nz]), 12)).size
        sp = mags <= 8 and nzu <= 640 and nzu <= 0.45 * 2.0 * d * d
        if sp:
            cf = cf_pairs(par[0]) if kind == "ctl" else sum(np.unique(np.round(np.abs(g[g != 0]), 12)).size for g in Gj)
            v4 = cf <= 16 and v4_power_tiles(d, m, ORDER // 2) > 0
            hc = mags <= 7
    return dict(d=d, n=n, m=m, n_upos=int(union.sum()), uell_w=max(int(nz.sum(axis=0).max()), 1), ell_w=ell_w, ellt_w=ellt_w,
                anti=all(np.array_equal(g, -g.T) for g in Gj), iso=iso, sp=sp, v4=v4, hc=hc, per_member=name in MEMBERS)  # fmt: skip


def v4_lds_bytes(d, m, np_):
    return ((m + 4 + np_) * d * (2 * d + 1) + 24) * 8


def v4_power_tiles(d, m, q):
    np_ = q + 1
    while np_ > 2 and v4_lds_bytes(d, m, np_) > LDS_BYTES:
        np_ -= 1
    return np_ if v4_lds_bytes(d, m, np_) <= LDS_BYTES else 0


def ell_fits_lds(p):
    n_ell = p["m"] * p["n"] * p["ell_w"]
    return n_ell > 0 and n_ell * 10 <= 8192


def v3_specialised(p, items, specialize=1):
    if not specialize or p["ell_w"] != 2:
        return False
    return (p["d"], p["m"]) in ((27, 6), (25, 4)) or ((p["d"], p["m"]) == (16, 4) and items <= 512)


def fused3_lds_bytes(p, ncw, tab):
    LD, n, m = lds_ld(p["n"]), p["n"], p["m"]
    tile, wsz, n_ell, n_un, uw = LD * n, LD * (16 + 3 * ncw), m * n * p["ell_w"], p["n_upos"], p["uell_w"]
    b = (4 * tile + 4 * wsz + 3 * (m + 1) + 2) * 8
    if tab:
        b += (n_un * uw + n_un + n_ell) * 8 + (n_un + n_ell) * 2 + n_un * uw
    return (b + 7) // 8 * 8 + 128


def v3_fits(p):
    """launch_fused_v3's LDS test; the chunk width ncw = min(nc, 16 / (2 + m)) depends on the slice width the cost model picks, so both ends
    must agree for the answer to be a property of the shape (asserted for every case by the CPU test)."""
    ans = {fused3_lds_bytes(p, ncw, False) <= LDS_BYTES for ncw in (1, max(1, 16 // (2 + p["m"])))}
    assert len(ans) == 1, p
    return ans.pop()


def v1_auto(p, items, kernel_version=0):
    return kernel_version == 0 and (p["d"] <= 8 or (p["d"] <= 16 and items <= 512))


def fused_wu(p):
    """launch_fused_v12: the instance of pcl_fused_kernel_v2 (1 | 2 entries per union position held in registers, -1 the general loop)."""
    return p["uell_w"] if p["uell_w"] <= 2 and p["n_upos"] <= 1024 and not p["per_member"] else -1


def eval_wu(p):
    """launch_eval_mfma: the instance of pcl_eval_kernel."""
    return p["uell_w"] if p["uell_w"] <= 2 and p["n_upos"] <= 256 * 4 else -1


def eval_mfma_lds_bytes(p):
    d, n, m = p["d"], p["n"], p["m"]
    lde = n if d & 1 else lds_ld(n)
    return (lde * n + 4 * lde * 16 + 2 * (m + 1) + 2) * 8 + 128


def small_kernel(p, want_jac, kernel_version=0):
    return (kernel_version == 5 or (kernel_version == 0 and (p["n"] <= 8 or not want_jac))) and p["n"] <= 16 and p["d"] <= 8 and p["m"] <= 8


def fused_family(p, items, kernel_version=0, use_mfma=1, specialize=1, jit=1):
    """last_kernel after eval_jac at order 4 (launch_fused), or "ESHAPE"."""
    v4_auto = kernel_version == 0 and use_mfma
    if kernel_version == 4 or v4_auto:
        if p["v4"] and jit:
            return 42
        if kernel_version == 4:
            return "ESHAPE"
    if small_kernel(p, True, kernel_version):
        return 52
    if kernel_version == 5:
        return "ESHAPE"
    if (kernel_version == 3 or (kernel_version == 0 and v3_specialised(p, items, specialize))) and use_mfma and 2 + p["m"] <= 16 and v3_fits(p):
        ewr = p["ell_w"] if p["m"] <= 8 and 1 <= p["ell_w"] <= 2 else 0
        spec3 = ewr == 2 and specialize and (p["d"], p["m"]) in ((27, 6), (25, 4), (16, 4)) and 16 // (2 + p["m"]) == 2
        if spec3:
            return 31
        if jit and specialize and ewr >= 1:
            return 32
        if kernel_version == 3:
            return 30
    v2 = not v1_auto(p, items, kernel_version) and (kernel_version == 0 or kernel_version >= 2) and use_mfma
    return 20 if v2 else 10


def eval_family(p, items, n_cu, eval_kernel=0, kernel_version=0, use_mfma=1, jit=1):
    """last_kernel after eval at order 4, or "ESHAPE"."""
    if eval_kernel == 3 or (eval_kernel == 0 and kernel_version == 0):
        if p["v4"] and jit:
            return 82
        if eval_kernel == 3:
            return "ESHAPE"
    if small_kernel(p, False, kernel_version):
        return 52
    if kernel_version == 5:
        return "ESHAPE"
    if (eval_kernel == 2 or (eval_kernel == 0 and items > n_cu)) and p["sp"] and jit and (kernel_version == 0 or kernel_version >= 3):
        return 70
    if eval_kernel == 2:
        return "ESHAPE"
    if use_mfma and p["d"] >= 9 and (kernel_version == 0 or kernel_version >= 3) and eval_mfma_lds_bytes(p) <= LDS_BYTES:
        return 60
    v2 = not v1_auto(p, items, kernel_version) and (kernel_version == 0 or kernel_version >= 2) and use_mfma
    return 20 if v2 else 10


def eval_sparse_grid(items, n_cu):
    """launch_eval_sparse: (waves per workgroup, workgroups, idle waves in the last workgroup)."""
    nw = min(8, max(1, -(-items // n_cu)))
    grid = min(-(-items // nw), n_cu)
    return nw, grid, (nw * grid - items if nw * grid >= items else 0)


def balanced_grid(items, slots, grid=0):
    rounds = -(-items // slots)
    return min(items, grid) if grid > 0 else -(-items // rounds)


def hess_v2_supported(p):
    return 1 <= p["m"] <= 6 and p["ell_w"] <= 2 and p["ellt_w"] <= 2


def hess_lds_bytes(p, nc):
    LD, n, m = lds_ld(p["n"]), p["n"], p["m"]
    return (LD * n + (6 + 3 * m) * LD * nc + 8 + m + 5 * ((m + 1) * (m + 2) // 2)) * 8


def hess1_chunk(p):
    """launch_hess_v1: the state columns per chunk (half the LDS: two workgroups per CU)."""
    nc = p["d"]
    while nc > 1 and hess_lds_bytes(p, nc) > LDS_BYTES // 2:
        nc = (nc + 1) // 2
    return nc


def hess2_lds_bytes(p):
    LD, n, m = lds_ld(p["n"]), p["n"], p["m"]
    return (LD * n + 7 * LD * 16 + 4 * ((m + 1) * (m + 2) // 2) + 4 + 2) * 8


def hess3_lds_bytes(p):
    d, n, m = p["d"], p["n"], p["m"]
    lde = n if d & 1 else lds_ld(n)
    return (lde * n + (8 + 2 * m) * lde * 16 + 2 * (m + 1) + 8 * ((m + 1) * (m + 2) // 2) + 8) * 8 + 64


def hess_sparse_lds_bytes(p):
    d, n, m = p["d"], p["n"], p["m"]
    return ((5 + m) * (n + 1) * d + 2 * (m * (m + 2) + 1) * 4) * 8 + 64


def hess_family(p, items, n_cu, hess_kernel=0, use_mfma=1, specialize=1, jit=1):
    """last_hess_kernel at order 4 (launch_hess), or "ESHAPE"."""
    cols_auto = hess_kernel == 0 and 2 * items <= n_cu
    if hess_kernel == 8 or cols_auto:
        if p["v4"] and jit and p["hc"] and p["m"] >= 1:
            return 82
        if hess_kernel == 8:
            return "ESHAPE"
    if hess_kernel == 7:
        return 72 if p["v4"] and jit else "ESHAPE"
    if hess_kernel in (0, 4):
        if p["sp"] and jit and hess_sparse_lds_bytes(p) <= LDS_BYTES:
            return 6
        if hess_kernel == 4:
            return "ESHAPE"
    static = specialize and p["anti"] and (p["d"], p["m"]) in ((27, 6), (25, 4))
    if use_mfma and hess_kernel in (0, 3) and hess_v2_supported(p) and p["uell_w"] <= 2 and p["n_upos"] <= 1024 and (hess_kernel == 3 or p["d"] >= 12):
        if hess3_lds_bytes(p) <= LDS_BYTES and (static or (jit and specialize)):
            return 4 if static else 5
        if hess_kernel == 3:
            return "ESHAPE"
    if hess_kernel == 2 and not hess_v2_supported(p):
        return "ESHAPE"
    if use_mfma and hess_kernel != 1 and hess_v2_supported(p) and hess2_lds_bytes(p) <= LDS_BYTES:
        return 3 if (not static and jit and specialize and p["ell_w"] >= 1 and p["d"] >= 12) else 2
    return 1


def fused2_lds_bytes(p, nc, jac, ell):
    LD, n, m = lds_ld(p["n"]), p["n"], p["m"]
    c1 = ((2 + m) if jac else 2) * nc
    b = (LD * n * (2 if jac else 1) + 2 * LD * c1 + LD * nc + 2 * (m + 1)) * 8
    if jac and ell:
        n_ell = m * n * p["ell_w"]
        b += n_ell * 8 + (n_ell * 2 + 7) // 8 * 8
    return b + 128


def fused2_slices(p, items, n_cu):
    """choose_cols_per_slice for kernel 20 with the Jacobian: (state columns per slice, slices per interval)."""
    d, best = p["d"], 1
    for nc in range(d, 0, -1):
        if fused2_lds_bytes(p, nc, True, ell_fits_lds(p)) > LDS_BYTES // 2 and nc > 1:
            continue
        best = nc
        if items * -(-d // nc) >= 3 * n_cu:
            break
    return best, -(-d // best)


def fused2_grid(p, items, n_cu):
    """(work items, resident workgroups) of kernel 20's persistent grid: it wraps where there are more items than workgroups."""
    nc, S = fused2_slices(p, items, n_cu)
    per_cu = max(1, min(2, LDS_BYTES // fused2_lds_bytes(p, nc, True, ell_fits_lds(p))))
    return items * S, per_cu * n_cu


# ---- faults, applied to the truth alone -------------------------------------------------------------------------------------------------------
def mm_last_row(A, B):
    C = A @ B
    C[-1, :] = 0
    return C


def mm_last_col(A, B):
    C = A @ B
    C[:, -1] = 0
    return C


def mm_last_inner(A, B):
    return A[:, :-1] @ B[:-1]


def seen(good, bad, lab):
    """The largest relative change of a segment, against the segment's own maximum."""
    out = 0.0
    for s in np.unique(lab):
        sel = lab == s
        scale = np.abs(good[sel]).max()
        if scale > 0:
            out = max(out, float(np.abs(bad[sel] - good[sel]).max() / scale))
    return out
