"""CPU tests of the Hessian of the Lagrangian of the variational integrators on the exponential constraint (option ``var_exp_hess``): the
adjoint formulas the kernel evaluates (pcl_kernel_var_exp_hess.hpp; a quadruple chain on W_0 and an octuple chain per (variation, drive)),
restated in numpy, against the lifted truth of tests/var_exp_hess_truth.py -- once with every tile from a block ``expm``, once with the
kernel's scaled Taylor recurrence -- the condition on the GPU parity cases that a dropped term shows, and the constructors' keyword.

``model(case, mu, tiles)`` is the statement of what the kernels compute; ``tiles`` is how the chain T_S = L_|S|(A'; directions in S) is had."""
import dataclasses
import itertools

import numpy as np
import pytest
import scipy.linalg

import piccolo_jl_amd as pa
import var_exp_cases as cases
import var_exp_hess_truth as truth

GPU_TOL = 1e-11


def close(a, b, tol):
    """max|a - b| <= tol max(1, |b|_inf); returns the deviation relative to that scale."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() / max(1.0, np.abs(b).max())
    assert err <= tol, err
    return err


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def _subsets(S):
    return [frozenset(c) for r in range(len(S) + 1) for c in itertools.combinations(sorted(S), r)]


def tiles_expm(Gt, h, dirs):
    """{subset: T_S}: T_S = L_|S|(h Gt; the directions of S), read off exp of the 2^k n block matrix that carries direction x from block R to
    block R + {x}.  dirs: {name: (matrix, scaled_by_h)}."""
    n, names = Gt.shape[0], sorted(dirs)
    subs = _subsets(names)
    pos = {S: i for i, S in enumerate(subs)}
    B = np.zeros((len(subs) * n, len(subs) * n))
    for S in subs:
        i = pos[S]
        B[i * n : (i + 1) * n, i * n : (i + 1) * n] = h * Gt
        for x in names:
            if x not in S:
                j = pos[S | {x}]
                D, by_h = dirs[x]
                B[i * n : (i + 1) * n, j * n : (j + 1) * n] = (h if by_h else 1.0) * D
    E = scipy.linalg.expm(B)
    return {S: E[:n, pos[S] * n : (pos[S] + 1) * n] for S in subs}


def tiles_recurrence(Gt, h, dirs, norm1=None):
    """The kernel's recurrence: theta = |h| |G|_1 <= 1/4 after s halvings, Taylor degree 14 by Horner with a_h = h 2^-s / j on G' and the
    directions scaled by h, a_p = 2^-s / j on the others; then s squarings T_S <- sum_{R in S} T_R T_{S - R}."""
    n, names = Gt.shape[0], sorted(dirs)
    subs = sorted(_subsets(names), key=len, reverse=True)  # the highest tile first; every right-hand side reads the old tiles
    theta = abs(h) * (np.abs(Gt.T).sum(axis=0).max() if norm1 is None else norm1)
    s = 0
    while theta > 0.25 and s < 60:
        theta *= 0.5
        s += 1
    hs, ps = np.ldexp(h, -s), np.ldexp(1.0, -s)
    T = {S: (np.eye(n) if not S else np.zeros((n, n))) for S in subs}
    for j in range(14, 0, -1):
        ah, ap = hs / j, ps / j
        new = {}
        for S in subs:
            acc = ah * (Gt @ T[S])
            for x in sorted(S):
                D, by_h = dirs[x]
                acc = acc + (ah if by_h else ap) * (D @ T[S - {x}])
            new[S] = acc + (np.eye(n) if not S else 0.0)
        T = new
    for _ in range(s):
        T = {S: sum(T[R] @ T[S - R] for R in _subsets(S)) for S in subs}
    return T


# ---- the adjoint formulas ----------------------------------------------------------------------------------------------------------------
def model(case, mu, tiles=tiles_expm, drop=()):
    """[K, nnz_per_interval].  drop: terms left out (the mutation test)."""
    n, C, v, m, xdc = case.n, case.C, case.v, case.m, case.xdc
    nsc = (m + 1) * (m + 2) // 2
    mu = np.asarray(mu).reshape(case.K, case.xd)
    e = frozenset
    out = []
    for k in range(case.K):
        z = case.Z[k]
        h = z[case.dt_off]
        G = case.G0 + (np.tensordot(z[case.u_off : case.u_off + m], case.Gj, axes=1) if m else 0.0)
        X = [z[o : o + xdc].reshape(C, n).T for o in case.xo]
        M = [mu[k, b * xdc : (b + 1) * xdc].reshape(C, n).T for b in range(v + 1)]
        W0 = M[0] @ X[0].T + (0.0 if "W0var" in drop else sum(M[i] @ X[i].T for i in range(1, v + 1)))
        Wi = [None] + [M[i] @ X[0].T for i in range(1, v + 1)]
        a_by_h = "ap" in drop  # the mutation: W_i scaled by a_h like a generator
        uu, dtu = np.zeros((m, m)), np.zeros(m)
        uX = np.zeros((m, v + 1, n, C))
        T0 = None
        Tb = [None] * (v + 1)
        for l in range(max(m, 1)):
            dq = {"a": (W0, False)}
            if m:
                dq["c"] = (case.Gj[l].T, True)
            Q = tiles(G.T, h, dq)
            T0 = Q[e()]
            if m:
                Ta, Tc, Tac = Q[e("a")], Q[e("c")], Q[e("ac")]
                for j in range(l + 1):
                    uu[l, j] += -h * np.sum(Tac * case.Gj[j])
                dtu[l] += -np.sum(Ta * case.Gj[l]) - np.sum(Tac * G)
                for b in range(v + 1):
                    uX[l, b] += -Tc @ M[b]
            for i in range(1, v + 1):
                do = {"a": (Wi[i], a_by_h), "b": (case.Gv[i - 1].T, True)}
                if m:
                    do["c"] = (case.Gj[l].T, True)
                O = tiles(G.T, h, do)
                Tb[i] = O[e("b")]
                if m:
                    for j in range(l + 1):
                        uu[l, j] += -h * np.sum(O[e("abc")] * case.Gj[j])
                    t = 0.0
                    if "abGl" not in drop:
                        t += np.sum(O[e("ab")] * case.Gj[l])
                    if "abcG" not in drop:
                        t += np.sum(O[e("abc")] * G)
                    if "acGv" not in drop:
                        t += np.sum(O[e("ac")] * case.Gv[i - 1])
                    dtu[l] -= t
                    if "bcM" not in drop:
                        uX[l, 0] += -O[e("bc")] @ M[i]
        N = [G.T @ M[0] + sum(case.Gv[i - 1].T @ M[i] for i in range(1, v + 1))] + [G.T @ M[i] for i in range(1, v + 1)]
        R = [G.T @ N[0] + sum(case.Gv[i - 1].T @ N[i] for i in range(1, v + 1))] + [G.T @ N[i] for i in range(1, v + 1)]
        dX = [-(T0 @ N[0] + sum(Tb[i] @ N[i] for i in range(1, v + 1)))] + [-(T0 @ N[i]) for i in range(1, v + 1)]
        dd = -np.sum((T0 @ R[0] + sum(Tb[i] @ R[i] for i in range(1, v + 1))) * X[0]) - sum(np.sum((T0 @ R[i]) * X[i]) for i in range(1, v + 1))
        vals = [uu[np.tril_indices(m)], dtu, [dd]]
        for l in range(m):
            vals += [uX[l, b].T.reshape(-1) for b in range(v + 1)]
        vals += [dX[b].T.reshape(-1) for b in range(v + 1)]
        out.append(np.concatenate(vals))
    out = np.array(out)
    assert out.shape[1] == truth.nnz_per_interval(case) and nsc <= out.shape[1]
    return out


def rand_mu(case, seed):
    return np.random.default_rng(seed).standard_normal(case.K * case.xd)


def random_gv_case():
    """config 2 with a random, not antisymmetric variation generator and a random state: no structure for a transposed term to hide in."""
    case = cases.config2(1, N=3, dt=0.3)[3]
    rng = np.random.default_rng(77)
    case = dataclasses.replace(case, Gv=[0.4 * rng.standard_normal(case.G0.shape)])
    case.Z[:, : case.xd] = 0.5 * rng.standard_normal((case.N, case.xd))
    return case


def one_drive(case):
    return dataclasses.replace(case, m=1, Gj=case.Gj[:1])


def no_drives(case):
    return dataclasses.replace(case, m=0, Gj=np.zeros((0, case.n, case.n)))


PARITY_CASES = {
    "pauli_ket": lambda: cases.pauli(True)[3],
    "pauli": lambda: cases.pauli(False)[3],
    "config2_v1": lambda: cases.config2(1)[3],
    "config2_v2": lambda: cases.config2(2)[3],
    "config2_v1_ket": lambda: cases.config2(1, ket=True)[3],
    "transmon3": lambda: cases.transmon(3)[3],
    "transmon17": lambda: cases.transmon(17, N=3)[3],
    "transmon22": lambda: cases.transmon(22, N=3)[3],
    "no_drives": lambda: no_drives(cases.config2(2)[3]),
    "one_drive": lambda: one_drive(cases.config2(2)[3]),
}


# ---- tests -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["pauli", "pauli_ket", "config2_v1", "config2_v2", "random_gv", "no_drives", "one_drive"])
def test_adjoint_formulas_equal_the_lifted_truth(which):
    """Quadruple and octuple by block expm: the formulas alone, without the recurrence."""
    case = random_gv_case() if which == "random_gv" else PARITY_CASES[which]()
    mu = rand_mu(case, 1)
    t = truth.values(case, mu)
    err = close(model(case, mu, tiles_expm), t, 1e-12)
    print("%s: max|model - truth| / max(1, |truth|) %.2e  (|truth|_inf %.2e)" % (which, err, np.abs(t).max()))


@pytest.mark.parametrize("which", ["config2_dt0.1", "config2_dt4", "transmon22"])
def test_scaled_recurrence_equals_the_lifted_truth(which):
    """The kernel's scaled Taylor recurrence in numpy.  Worst deviation read, relative to max(1, |truth|_inf): config 2 at dt = 0.1 1.6e-16, at
    dt = 4 (five squarings, |truth|_inf 1.4e4) 2.8e-15, transmon(22) (n = 44, four squarings) 1.6e-15 -- four orders below the GPU tolerance."""
    case = {"config2_dt0.1": lambda: cases.config2(2)[3], "config2_dt4": lambda: cases.config2(1, dt=4.0)[3],
            "transmon22": lambda: cases.transmon(22, N=3)[3]}[which]()  # fmt: skip
    mu = rand_mu(case, 2)
    t = truth.values(case, mu)
    err = close(model(case, mu, tiles_recurrence), t, 1e-12)
    print("%s: max|recurrence - truth| / max(1, |truth|) %.2e  (|truth|_inf %.2e)" % (which, err, np.abs(t).max()))


MUTATIONS = ["abcG", "acGv", "abGl", "bcM", "W0var", "ap"]


@pytest.mark.parametrize("which", [k for k in PARITY_CASES if k != "no_drives"])
def test_a_dropped_term_shows_on_the_gpu_parity_cases(which):
    """A condition on the inputs of tests/test_var_exp_hess_gpu.py: leaving out <Tabc, G>, <Tac, Gv_i>, <Tab, G_l>, sum_i Tbc M_i, the
    sum_i M_i Xv_i' part of W_0, or scaling W_i by a_h instead of a_p moves the values by at least 1e4 x the GPU tolerance."""
    case = PARITY_CASES[which]()
    mu = rand_mu(case, 3)
    good = model(case, mu, tiles_recurrence)
    scale = max(1.0, np.abs(good).max())
    for mut in MUTATIONS:
        moved = np.abs(model(case, mu, tiles_recurrence, drop=(mut,)) - good).max() / scale
        print("%s without %s: moved by %.2e" % (which, mut, moved))
        assert moved >= 1e4 * GPU_TOL, (which, mut, moved)


@pytest.mark.parametrize("ket", [True, False])
def test_exp_hessian_keyword_needs_the_exponential_constraint(ket):
    """``exp_hessian=True`` with a Pade order: ValueError in the plain constructor's words, before any device call."""
    sysv = pa.VariationalQuantumSystem(pa.PAULIS["Z"] / 2, [pa.PAULIS["X"], pa.PAULIS["Y"]], [pa.PAULIS["Z"] / 2], [1.0, 1.0])
    case = cases.pauli(ket)[3]
    names = ["ψ̃", "ψ̃_var"] if ket else ["Ũ⃗", "Ũ⃗_var"]
    comps = {nm: case.Z[:, o : o + case.xdc].T for nm, o in zip(names, case.xo)}
    comps["Δt"] = case.Z[:, case.dt_off][None]
    comps["t"] = case.Z[:, case.dt_off + 1][None]
    comps["u"] = case.Z[:, case.u_off : case.u_off + case.m].T
    traj = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
    ctor = pa.VariationalKetIntegrator if ket else pa.VariationalUnitaryIntegrator
    with pytest.raises(ValueError, match="exp_hessian=True is the Hessian of the Lagrangian of the exponential constraint"):
        ctor(sysv, traj, names[0], names[1:], "u", pade_order=4, exp_hessian=True)
