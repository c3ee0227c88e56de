"""Case definitions shared by the general-shape tests (importable without a GPU): random systems whose sparsity pattern, (drive,
magnitude) coefficients, distinct drive magnitudes and drift value classes straddle the limits the code generator specialises on, and a
per-segment comparison of values against the oracle.

Limits (piccolo.jl_amd/csrc/pcl_codegen.hpp, pcl_codegen_v4.hpp, piccolo_hip.hip pcl_create):
    pattern-compiled kernels: sparse exact-iso generators of a unitary problem, 9 <= d <= 32, 1 <= m <= 6, at most kMaxMags = 8
    distinct drive magnitudes, and a union pattern of nz <= 640 entries and nz <= 0.45 * 2 d^2 in the left column block;
    kernel 4 family (fused 40+q, residual 80+q, Hessian 70+q / 80+q): also at most kV4MaxCf = 16 (drive, magnitude) pairs."""
import numpy as np

from oracle import pade_oracle as po

MAGS = (1.0, np.sqrt(2.0), 0.37, 0.61, 1.3, 0.83, 1.9, 0.45, 1.13, 0.27)  # distinct drive magnitudes
DRIFT_MAGS = (0.3, 0.55, 0.8)  # value classes of a "classes" drift (off-diagonal entries)
DRIFT_DIAG = (0.2, -0.4, 0.9, 1.5)
KV4_MAX_CF = 16
K_MAX_MAGS = 8
SP_MAX_NZ = 640


# ---- the generators of tests/test_parity_gpu.py (moved here unchanged) ------------------------------------------------------------------
def random_case(d, m, N, rng, x_off=0, pad=3):
    n = 2 * d
    xd = 2 * d * d
    z_dim = x_off + xd + pad + m + 1
    lay = po.Layout(d=d, m=m, N=N, z_dim=z_dim, x_off=x_off, u_off=x_off + xd + 1, dt_off=x_off + xd)
    G0 = rng.standard_normal((n, n))
    Gj = rng.standard_normal((m, n, n)) * (rng.random((m, n, n)) < 0.3) if m else np.zeros((0, n, n))
    Z = rng.standard_normal((N, z_dim))
    Z[:, lay.dt_off] = 0.05 + 0.1 * rng.random(N)
    return lay, G0, Gj, Z


def random_sparse_iso_system(d, m, rng, n_mags=3):
    """Sparse Hermitian drift and drives (complex entries: the A and the B block of iso(-iH) are both populated), drive
    entries drawn from a few magnitudes with random signs / phases in {1, i}: what the pattern-compiled kernels specialise on."""
    def herm(mask_density, vals):
        H = np.zeros((d, d), dtype=complex)
        for i in range(d):
            for j in range(i, d):
                if rng.random() < mask_density:
                    v = vals()
                    if i == j:
                        H[i, i] = v.real if v.real != 0 else abs(v)
                    else:
                        H[i, j] = v
                        H[j, i] = np.conj(v)
        return H
    density = min(0.18, 2.5 / d)  # (a few hundred entries in the union pattern at every size)
    H0 = herm(density, lambda: complex(rng.standard_normal(), rng.standard_normal()))
    H0 += np.diag(rng.standard_normal(d))
    mags = [1.0, np.sqrt(2.0), 0.37][:n_mags]
    Hd = [herm(density * 0.5, lambda: rng.choice(mags) * rng.choice([1.0, -1.0]) * rng.choice([1.0, 1j])) for _ in range(m)]
    for H in Hd:  # every drive has entries in both blocks
        i, j = rng.choice(d, 2, replace=False)
        H[i, j] += 1j * mags[0]
        H[j, i] -= 1j * mags[0]
        H[i, i] += mags[0]
    return po.G_of_H(H0), np.array([po.G_of_H(H) for H in Hd])


# ---- systems with the generator's limits under control ------------------------------------------------------------------------------
def controlled_hermitians(d, drive_mags, rng, drift="classes", density=None, extra=1):
    """Hermitian drift H0 and drives Hd[l] (complex d x d).  Drive l holds the magnitudes MAGS[g] for g in drive_mags[l], each as one
    real and one imaginary off-diagonal entry (both blocks of iso(-iH)) plus `extra` more entries, at distinct positions: so the
    (drive, magnitude) pairs are exactly sum_l len(drive_mags[l]) and the distinct magnitudes exactly the union of drive_mags.
    drift: "classes" (entries from a few magnitudes: every class resident) | "continuous" (every entry its own value class: the
    classes beyond the resident ones are streamed) | "dense" (every entry set, continuous values)."""
    offd = [(i, j) for i in range(d) for j in range(i + 1, d)]
    if density is None:
        density = min(0.18, 2.5 / d)
    H0 = np.zeros((d, d), dtype=complex)
    for i, j in offd:
        if drift == "dense" or rng.random() < density:
            if drift == "classes":
                v = rng.choice(DRIFT_MAGS) * rng.choice([1.0, -1.0]) * rng.choice([1.0, 1j])
            else:
                v = complex(rng.standard_normal(), rng.standard_normal())
            H0[i, j], H0[j, i] = v, np.conj(v)
    H0 += np.diag(rng.choice(DRIFT_DIAG, d) if drift == "classes" else rng.standard_normal(d))
    Hd = []
    for mags in drive_mags:
        H = np.zeros((d, d), dtype=complex)
        pos = rng.permutation(len(offd))
        p = 0
        for g in list(mags) + [mags[k % len(mags)] for k in range(extra)]:
            for ph in (1.0, 1j):
                i, j = offd[pos[p]]
                p += 1
                v = MAGS[g] * rng.choice([1.0, -1.0]) * ph
                H[i, j], H[j, i] = v, np.conj(v)
        Hd.append(H)
    return H0, Hd


def controlled_system(d, drive_mags, rng, drift="classes", density=None):
    H0, Hd = controlled_hermitians(d, drive_mags, rng, drift, density)
    m = len(Hd)
    Gj = np.array([po.G_of_H(H) for H in Hd]) if m else np.zeros((0, 2 * d, 2 * d))
    return po.G_of_H(H0), Gj


def cf_pairs(drive_mags):
    return sum(len(set(g)) for g in drive_mags)


def n_mags(drive_mags):
    return len(set(g for gs in drive_mags for g in gs))


def union_nz(G0, Gj):
    """Entries of the union pattern in the left column block (what pcl_codegen::make_plan counts)."""
    d = G0.shape[0] // 2
    u = G0[:, :d] != 0
    for g in Gj:
        u |= g[:, :d] != 0
    return int(u.sum())


def sp_rule_admits(G0, Gj):
    """piccolo_hip.hip pcl_create: the pattern-compiled kernels take a system with nz <= 640 and nz <= 0.45 * 2 d^2."""
    d = G0.shape[0] // 2
    nz = union_nz(G0, Gj)
    return nz <= SP_MAX_NZ and nz <= 0.45 * 2.0 * d * d


def std_layout(d, m, N):
    xd = 2 * d * d
    return po.Layout(d=d, m=m, N=N, z_dim=xd + 2 + m, x_off=0, u_off=xd + 1, dt_off=xd)


def trajectory(lay, rng, dt=(0.05, 0.15), u_scale=0.4):
    Z = u_scale * rng.standard_normal((lay.N, lay.z_dim))
    Z[:, lay.dt_off] = dt[0] + (dt[1] - dt[0]) * rng.random(lay.N)
    return Z


def g_norm(lay, Z, k, G0, Gj):
    G = G0 + np.tensordot(Z[k, lay.u_off : lay.u_off + lay.m], Gj, axes=1) if lay.m else G0
    return np.linalg.norm(G, 2)


# ---- per-segment comparison -----------------------------------------------------------------------------------------------------------
def jac_labels(lay):
    """Segment of every Jacobian value of one context (po.jac_structure order): the -B+ block, the B- block, the d/du tails, the d/dh tail,
    per interval."""
    C, n, m = lay.C, lay.n, lay.m
    nb = C * n * n
    tail = np.tile(np.repeat(np.array(["du"] * m + ["dh"]), n), C)
    per = np.concatenate([np.full(nb, "B+"), np.full(nb, "B-"), tail])
    return per_interval(per, lay.K)


def hess_labels(lay):
    """Segment of every Hessian value (po.hess_structure order): (u,u), (h,u), (h,h), then the X rows: (u_l, X_k), (h, X_k),
    (X_k+1, u_l), (X_k+1, h), per interval."""
    m, xd = lay.m, lay.x_dim
    per = ["uu"] * (m * (m + 1) // 2) + ["hu"] * m + ["hh"]
    for l in range(m):
        per += ["u%d.Xk" % l] * xd
    per += ["h.Xk"] * xd
    for l in range(m):
        per += ["Xk1.u%d" % l] * xd
    per += ["Xk1.h"] * xd
    return per_interval(np.array(per), lay.K)


def per_interval(per, K):
    """The labels of one interval, repeated for K intervals with the interval's index: every interval's segment is held to its own size
    (a step of zero beside a large step)."""
    return np.concatenate([np.char.add(per, "@%d" % k) for k in range(K)])


def check_segments(ours, ref, layout, tol):
    """max|a - b| <= tol * max|ref segment| for every segment of `layout` (one label per value), with no floor at 1: a small segment is
    held to its own size, not to the largest block's.  Returns {segment: relative error}."""
    a, b = np.asarray(ours).reshape(-1), np.asarray(ref).reshape(-1)
    labels = np.asarray(layout).reshape(-1)
    assert a.shape == b.shape == labels.shape, (a.shape, b.shape, labels.shape)
    assert np.all(np.isfinite(a)), "non-finite values in segments %s" % sorted(set(labels[~np.isfinite(a)]))
    out = {}
    for s in np.unique(labels):
        sel = labels == s
        scale = np.abs(b[sel]).max()
        err = np.abs(a[sel] - b[sel]).max()
        out[str(s)] = err / scale if scale > 0 else err
        assert err <= tol * scale, "segment %s: max err %.3e, max |ref| %.3e (rel %.3e > %.1e)" % (s, err, scale, out[str(s)], tol)
    return out


def assert_sensitive(f_q, f_lower, tol, factor=1e4):
    """The case must be able to see a broken top term: the oracle at order q differs from the oracle at the neighbouring order by at
    least factor x tol, relative."""
    f_q, f_lower = np.asarray(f_q).reshape(-1), np.asarray(f_lower).reshape(-1)
    rel = np.abs(f_q - f_lower).max() / np.abs(f_q).max()
    assert rel >= factor * tol, "case too insensitive to the top Pade term: relative change %.2e < %.1e" % (rel, factor * tol)
    return rel


def lower_order(order):
    return order - 2 if order > 2 else 4


# ---- the plain cases of tests/test_general_shapes_*.py ----------------------------------------------------------------------------------
# name: (d, drive magnitudes per drive | m of a dense non-iso system, drift kind, density, seed)
PLAIN_CASES = {
    "S1": (9, [[0, 1]], "classes", None, 1),  # smallest pattern-compiled d, one drive
    "S2": (13, [[0, 1, 2, 3], [4, 5, 6, 7], [0, 2, 4, 6], [1, 3, 5, 7]], "classes", None, 2),  # exactly kV4MaxCf = 16 pairs, 8 magnitudes
    "S3": (20, [[0, 1], [2], [0, 3]], "continuous", None, 3),  # drift classes streamed
    "S4": (31, [[0], [1], [2], [0, 1]], "classes", None, 4),  # odd d, the most drives whose tiles fit the LDS at d = 31
    "S5": (32, [[0, 1], [2]], "classes", None, 5),  # every lane of a half wave
    "S6": (32, [[0], [1], [2], [3], [0], [1]], "classes", None, 6),  # tightest LDS
    "F1": (13, [[0, 1, 2, 3, 4], [4, 5, 6, 7], [0, 2, 4, 6], [1, 3, 5, 7]], "classes", None, 2),  # 17 pairs
    "F2": (12, [[0, 1, 2], [3, 4, 5], [6, 7, 8]], "classes", None, 7),  # 9 distinct magnitudes
    "F3": (12, [[g % 4] for g in range(7)], "classes", None, 8),  # 7 drives
    "F4a": (16, 2, "dense", None, 9),  # dense non-iso generators
    "F4b": (32, 2, "dense", None, 10),
    "F5": (8, [[0], [1]], "classes", None, 11),  # d below the pattern-compiled range
    "F6": (32, [[0], [1]], "continuous", 0.45, 12),  # union pattern too dense
}
DT = (0.05, 0.15)  # the Delta t of a case's knots, scaled per case to h |G(u)|_2 of about 0.15 .. 0.45 (see plain_case)


def plain_system(name):
    d, dm, drift, density, seed = PLAIN_CASES[name]
    rng = np.random.default_rng(7000 + seed)
    if drift == "dense":
        n = 2 * d
        G0 = rng.standard_normal((n, n)) / np.sqrt(n)
        Gj = rng.standard_normal((dm, n, n)) * (rng.random((dm, n, n)) < 0.3) / np.sqrt(n)
        return G0, Gj
    return controlled_system(d, dm, rng, drift, density)


def plain_case(name, N=4, seed=0):
    """(layout, G0, Gj, Z) of a plain case: standard knot [X | dt | t | u], u ~ 0.4 N(0, 1), Delta t such that h |G(u)|_2 lies in
    0.15 .. 0.45 (the top term of order 10 then moves the values by ~1e-7 relative, 1e4 x the tolerance)."""
    G0, Gj = plain_system(name)
    d, m = G0.shape[0] // 2, len(Gj)
    lay = std_layout(d, m, N)
    rng = np.random.default_rng(100 + seed)
    Z = trajectory(lay, rng)
    for k in range(N - 1):
        Z[k, lay.dt_off] = (0.15 + 0.3 * rng.random()) / g_norm(lay, Z, k, G0, Gj)
    return lay, G0, Gj, Z
