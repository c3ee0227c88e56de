"""Case table of tests/test_objective_shapes_{cpu,gpu}.py (importable without a GPU): seeded random layouts, states, goals, forms and
regularisers at the sizes where the objective-side kernels' loops wrap -- sums of more than 256 elements, Gram triangles beyond 4096 x 256
and 8192 x 256 entries, subspaces of more than 256 entries, eight regularisers, knots whose rows are not 16-byte aligned -- with terms on
both sides of the kink of |1 - F|, and the longdouble truth of each case (objective_truth) with its mutants."""
import numpy as np

import objective_truth as ot

LD = ot.LD
TOL = 1e-12  # value: TOL max(1, |ref|); gradient, Hessian, payload: TOL max|ref| per segment
MUTANTS = ("drop256", "wave1", "flip", "noweights", "overlap_once", "drop_last_reg")


def _unitary(d, rng):
    return np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0]


def _iso_vec(U):
    U = np.asarray(U)
    return np.concatenate([np.concatenate([U[:, c].real, U[:, c].imag]) for c in range(U.shape[0])])


def _near(G, scale, rng, eps=0.05):
    """A terminal state near the goal, scaled: F about scale^4 (1 - O(eps^2)) -- 1.1 puts it beyond the kink (F > 1), 0.9 before it."""
    d = G.shape[0]
    return scale * G @ (np.eye(d) + eps * (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))) / np.sqrt(d))


def _system(n, m, rng):
    return rng.standard_normal((n, n)) / np.sqrt(n), rng.standard_normal((m, n, n)) * (rng.random((m, n, n)) < 0.3) / np.sqrt(n)


def make(name, *, d, m, N, x_offs, z_dim, dt_off, u_off, seed, traj=0, state_cols=0, goal=None, weights=None, Q=100.0, regs=(), launches=None,
         states=None, mutants=(), hess=False, index_base=0, sigma=1.0):  # fmt: skip
    """states: per term's member / seed the terminal state vector (None: the random knot stays).  traj: number of seeds (PCL_BATCH_TRAJ), 0:
    PCL_BATCH_MEMBERS with len(x_offs) members."""
    rng = np.random.default_rng(seed)
    n = 2 * d
    x_dim = n * (d if state_cols == 0 else 1)
    nbuf = traj or 1
    Z = 0.4 * rng.standard_normal((nbuf, N, z_dim))
    Z[:, :, dt_off] = 0.05 + 0.1 * rng.random((nbuf, N))
    batch = traj or len(x_offs)
    for b, x in enumerate(states or ()):
        if x is not None:
            o = x_offs[0] if traj else x_offs[b]
            Z[b if traj else 0, -1, o : o + x_dim] = x
    G0, Gj = _system(n, m, rng)
    return dict(name=name, d=d, m=m, N=N, x_offs=list(x_offs), z_dim=z_dim, dt_off=dt_off, u_off=u_off, traj=traj, batch=batch, state_cols=state_cols,
                x_dim=x_dim, Z=Z, G0=G0, Gj=Gj, goal=goal, weights=None if weights is None else np.asarray(weights, float), Q=Q, regs=list(regs),
                launches=launches, mutants=tuple(mutants), hess=hess, index_base=index_base, sigma=sigma)  # fmt: skip


# ---- builders ------------------------------------------------------------------------------------------------------------------------------------
def unitary_case(name, d, seed, *, members=0, traj=0, order=None, gap=0, x0=3, weights=None, regs_u=True, pad=2, **kw):
    """A unitary goal on M members of one knot (order: the members' positions, gap doubles between them) or on `traj` seeds; the knot is
    [x0 pad | states | dt | t | u (2)] + pad, z_dim odd; member / seed 0 lies beyond the kink (x 1.1), 1 before it (x 0.9), the others are random."""
    rng = np.random.default_rng(1000 + seed)
    xd, M = 2 * d * d, members or 1
    order = list(range(M)) if order is None else order
    x_offs = [x0 + p * (xd + gap) for p in order]
    dt_off = x0 + M * (xd + gap)
    z_dim = dt_off + 2 + 2 + pad
    z_dim += 1 - z_dim % 2
    G = _unitary(d, rng)
    states = [_iso_vec(_near(G, s, rng)) if s else None for s in ([1.1, 0.9] + [0] * 8)[: traj or M]]
    regs = ([(dt_off + 2, 2, [0.3, 0.7], 2)] if regs_u else []) + list(kw.pop("regs", ()))
    N = kw.pop("N", 4)
    return make(name, d=d, m=2, N=N, x_offs=x_offs[:1] if traj else x_offs, z_dim=z_dim, dt_off=dt_off, u_off=dt_off + 2, seed=seed, traj=traj,
                goal=("unitary", G), weights=weights, regs=regs, states=states, **kw)  # fmt: skip


def subspace_case(name, d, sub, seed, scale, **kw):
    rng = np.random.default_rng(2000 + seed)
    ns, xd = len(sub), 2 * d * d
    Gs = _unitary(ns, rng)
    U = 0.3 * (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
    if scale:
        U[np.ix_(sub, sub)] = _near(Gs, scale, rng)
    return make(name, d=d, m=2, N=3, x_offs=[1], z_dim=xd + 6, dt_off=xd + 1, u_off=xd + 3, seed=seed, goal=("subspace", Gs, list(sub)),
                states=[_iso_vec(U)], regs=[(xd + 3, 2, 0.5, 1)], launches=1, **kw)  # fmt: skip


def form_case(name, d, seed, R, with_c, *, members=0, traj=0, weights=None, target=(0.4, 1.6), **kw):
    """A random general form on a unitary context (L = x_dim = 2 d^2): rows ~ N(0, 1 / L), scaled so that F of term b is target[b % 2]."""
    rng = np.random.default_rng(3000 + seed)
    L, M = 2 * d * d, members or 1
    A = rng.standard_normal((R, L)) / np.sqrt(L) if R else None
    c = rng.standard_normal(L) / np.sqrt(L) if with_c else None
    states = []
    for b in range(traj or M):
        x = 0.4 * rng.standard_normal(L)
        lin = float(c @ x) if with_c else 0.0  # F(s x) = s lin + s^2 q: the s that gives the target
        q = float(((A @ x) ** 2).sum()) if R else 0.0
        tg = target[b % len(target)]
        states.append(x * ((-lin + np.sqrt(lin * lin + 4 * q * tg)) / (2 * q) if R else tg / lin))
    x_offs = [2 + b * L for b in range(M)]
    dt_off = 2 + M * L
    return make(name, d=d, m=1, N=3, x_offs=x_offs[:1] if traj else x_offs, z_dim=dt_off + 4, dt_off=dt_off, u_off=dt_off + 2, seed=seed, traj=traj,
                goal=("form", 0, A, c), weights=weights, states=states, launches=3, **kw)  # fmt: skip


def ket_case(name, d, n_kets, seed, joint, weights=None, coherent_weights=None, scales=(1.1, 0.9), **kw):
    """Ket context (x_dim = 2 d) with n_kets members.  joint: ONE coherent term over all kets (L = 2 d n_kets), else a term per ket."""
    rng = np.random.default_rng(4000 + seed)
    goals = [(lambda v: v / np.linalg.norm(v))(rng.standard_normal(d) + 1j * rng.standard_normal(d)) for _ in range(n_kets)]
    if joint:
        s = scales[0]
        states = [np.concatenate([(s * g + 0.02 * rng.standard_normal(d)).real, (s * g).imag]) for g in goals]
        rows = ot.coherent_ket_rows(goals, coherent_weights)
        goal = ("form", 1, np.asarray(rows, float), None)
        kw["coherent"] = (goals, coherent_weights)
    else:
        goals = [goals[0]] * n_kets
        states = [np.concatenate([(s * goals[0]).real, (s * goals[0]).imag + 0.02 * rng.standard_normal(d)]) if s else None
                  for s in (list(scales) + [0] * n_kets)[:n_kets]]  # fmt: skip
        goal = ("form", 0, np.asarray(ot.ket_rows(goals[0]), float), None)
        kw["ket_goal"] = goals[0]
    xd = 2 * d
    extra = {k: kw.pop(k) for k in ("coherent", "ket_goal") if k in kw}
    c = make(name, d=d, m=1, N=3, x_offs=[b * xd for b in range(n_kets)], z_dim=n_kets * xd + 3, dt_off=n_kets * xd, u_off=n_kets * xd + 2, seed=seed,
             state_cols=1, goal=goal, weights=weights, states=states, launches=3, **kw)  # fmt: skip
    c.update(extra)
    return c


def reg_case(name, N, seed, regs_of, **kw):
    """d = 27 unitary knot [x (1458) | dt | t | u (2) | du (2) | ddu (2)]; regs_of(x_dim, dt_off) -> the regularisers."""
    d = 27
    xd = 2 * d * d
    return unitary_case(name, d, seed, N=N, x0=0, regs_u=False, regs=regs_of(xd, xd), pad=4, **kw)


def _R(dim, seed):
    return 0.2 + np.random.default_rng(seed).random(dim)


CASES = {}


def _add(c):
    CASES[c["name"]] = c


# A: plain unitary goal
_add(unitary_case("A16", 16, 1, members=3, weights=[0.5, 0.3, 0.2], launches=1, mutants=("wave1", "flip", "noweights"), hess=True))
_add(unitary_case("A17", 17, 2, members=3, order=[2, 0, 1], gap=5, launches=2, mutants=("drop256", "wave1", "flip")))
_add(unitary_case("A27", 27, 3, traj=5, weights=[0.3, 0.1, 0.25, 0.15, 0.2], launches=1, mutants=("drop256", "wave1", "flip", "noweights")))
_add(unitary_case("A32", 32, 4, members=1, launches=1, mutants=("drop256", "wave1", "flip")))
_add(unitary_case("A27m", 27, 5, members=3, launches=1, mutants=("drop256", "flip"), x0=0, pad=1))
# B: subspace goal
_add(subspace_case("B1", 16, [5], 1, 1.1, mutants=("flip",)))
_add(subspace_case("B8", 27, [0, 3, 4, 9, 13, 20, 25, 26], 2, 0.9, mutants=("flip",)))
_add(subspace_case("B17", 20, list(range(2, 19)), 3, 1.1, mutants=("drop256", "wave1", "flip")))
_add(subspace_case("B32", 32, list(np.random.default_rng(9).permutation(32)), 4, 0.9, mutants=("drop256", "wave1", "flip")))
# C: general forms
_add(form_case("C1458_R1", 27, 1, 1, False, members=2, mutants=("drop256", "wave1", "flip")))
_add(form_case("C1458_R7c", 27, 2, 7, True, traj=2, weights=[0.6, 0.4], mutants=("drop256", "wave1", "flip", "noweights")))
_add(form_case("C2048_R2c", 32, 3, 2, True, members=2, weights=[0.7, 0.3], mutants=("drop256", "wave1", "flip", "noweights")))
_add(form_case("C2048_R0c", 32, 4, 0, True, traj=2, mutants=("drop256", "wave1", "flip")))
_add(form_case("C2048_R7", 32, 5, 7, False, members=1, target=(1.6,), mutants=("drop256", "wave1", "flip")))
_add(ket_case("Cket", 32, 5, 1, False, weights=[0.3, 0.1, 0.2, 0.25, 0.15], mutants=("flip", "noweights")))
_add(ket_case("Ccoh5", 32, 5, 2, True, coherent_weights=[0.9, 0.1, 0.4, 0.7, 0.2], mutants=("drop256", "wave1", "flip"), hess=True))
_add(ket_case("Ccoh5b", 32, 5, 3, True, scales=(0.9,), mutants=("drop256", "wave1", "flip")))
_add(ket_case("Ccoh40", 32, 40, 4, True, mutants=("drop256", "wave1", "flip"), hess=True))
# D: regularisers (d = 27: a state component of 1458 entries)
_add(reg_case("Dstate", 2, 1, lambda xd, dt: [(0, xd, _R(xd, 1), 0), (0, xd, _R(xd, 2), 1), (0, xd, _R(xd, 3), 2)], launches=2,
              mutants=("drop256", "wave1", "overlap_once"), hess=True))  # fmt: skip
_add(reg_case("Doverlap", 65, 2, lambda xd, dt: [(dt + 2, 6, _R(6, 4), 2), (dt + 2, 6, _R(6, 5), 1), (dt + 4, 4, _R(4, 6), 0), (100, 700, _R(700, 7), 2),
                                                  (500, 600, _R(600, 8), 1)], launches=2, mutants=("drop256", "wave1", "overlap_once"), hess=True))  # fmt: skip
_add(reg_case("Ddt", 100, 3, lambda xd, dt: [(dt - 300, 303, _R(303, 9), 2), (dt, 3, _R(3, 10), 1), (dt - 1, 2, _R(2, 11), 0)], launches=2,
              mutants=("drop256", "wave1", "overlap_once"), hess=True))  # fmt: skip
_add(reg_case("Deight", 65, 4, lambda xd, dt: [(dt + 2 + i % 3, 2 + i % 4, _R(2 + i % 4, 20 + i), i % 3) for i in range(7)] + [(7, 900, _R(900, 30), 2)],
              traj=3, launches=2, mutants=("drop256", "wave1", "overlap_once", "drop_last_reg"), hess=True))  # fmt: skip
# E: Hessian cases beyond the ones flagged above (hess=True): d = 16 / 27 goals with regularisers, sigma != 1, index_base 1, TRAJ with 3 seeds
_add(unitary_case("E27", 27, 6, traj=3, weights=[0.5, 0.2, 0.3], launches=1, mutants=("drop256", "flip", "noweights"), hess=True, index_base=1, sigma=0.37))
_add(form_case("E1458_R7c", 27, 7, 7, True, members=1, target=(1.6,), mutants=("drop256", "flip"), hess=True, sigma=2.5, regs=[(5, 40, 0.8, 2)]))
_add(subspace_case("E8", 27, [1, 2, 6, 8, 11, 19, 22, 24], 5, 1.1, mutants=("flip",), hess=True, index_base=1))


# ---- the truth of a case ----------------------------------------------------------------------------------------------------------------------------
def _keep(mut, n):
    e = np.arange(n)
    return e < 256 if mut == "drop256" else ~((e >= 64) & (e < 256)) if mut == "wave1" else None


def terms(case, mut=None):
    """Per terminal term (A, c, x, weight, variable indices of x, keep mask over the form's sum)."""
    g, d, xd, N, zd = case["goal"], case["d"], case["x_dim"], case["N"], case["z_dim"]
    if g is None:
        return []
    keep_e = lambda n: _keep(mut, n)
    scope, keepL = 0, None
    if g[0] == "unitary":
        A, c = ot.unitary_rows(g[1], keep_e(d * d)), None
    elif g[0] == "subspace":
        A, c = ot.subspace_rows(g[1], g[2], d, keep_e(len(g[2]) ** 2)), None
    else:
        scope, A, c = g[1], g[2], g[3]
        keepL = keep_e(A.shape[1] if A is not None else len(c))
    Z, out = case["Z"], []
    var = lambda b: (b * N * zd + case["x_offs"][0] if case["traj"] else case["x_offs"][b]) + (N - 1) * zd + np.arange(xd)
    if scope:
        idx = np.concatenate([var(b) for b in range(case["batch"])])
        return [(A, c, Z.reshape(-1)[idx], 1.0, idx, keepL)]
    for b in range(case["batch"]):
        w = 1.0 if case["weights"] is None or mut == "noweights" else case["weights"][b]
        out.append((A, c, Z.reshape(-1)[var(b)], w, var(b), keepL))
    return out


def case_regs(case, mut=None):
    return case["regs"][:-1] if mut == "drop_last_reg" else case["regs"]


def objective_truth(case, mut=None):
    """(values [1 | nbuf], gradient [nbuf, N, z_dim], member terms, (s, F) per term) in longdouble."""
    nbuf, N, zd = case["Z"].shape
    grad = np.zeros((nbuf, N, zd), dtype=LD)
    regval = np.zeros(nbuf, dtype=LD)
    for b in range(nbuf):
        v, g, _ = ot.reg_terms(case["Z"][b], case_regs(case, mut), case["dt_off"], (lambda n: _keep(mut, n)) if mut in ("drop256", "wave1") else None,
                               mut == "overlap_once")  # fmt: skip
        regval[b], grad[b] = v.sum(), g
    member, sF = [], []
    gf = grad.reshape(-1)
    for A, c, x, w, idx, keep in terms(case, mut):
        val, g, s, F = ot.form_loss(A, c, x, LD(w) * LD(case["Q"]), keep, mut == "flip")
        member.append(val), sF.append((s, F))
        gf[idx] += g
    member = np.array(member, dtype=LD)
    if case["traj"]:
        value = regval + (member if len(member) else 0)
    else:
        value = np.array([regval[0] + member.sum()])
    return value, grad, member, sF


def hessian_truth(case):
    """(keys, values, labels) of sigma grad^2 f: lower triangle, key = row * nvar + col (0-based), duplicates summed, sorted by key; label "tri@t"
    for the entries of term t's dense triangle, "reg@b.k" for the other entries of knot k of buffer b."""
    nbuf, N, zd = case["Z"].shape
    nvar = nbuf * N * zd
    keys, vals, tri = [], [], []
    for t, (A, c, x, w, idx, _) in enumerate(terms(case)):
        if A is None:
            continue
        _, _, s, _ = ot.form_loss(A, c, x, LD(1))
        i, j = np.tril_indices(len(idx))
        keys.append(np.maximum(idx[i], idx[j]) * nvar + np.minimum(idx[i], idx[j]))
        vals.append(-s * LD(w) * LD(case["Q"]) * LD(case["sigma"]) * ot.gram_tril(A))
        tri.append(np.full(len(i), t + 1))
    for b in range(nbuf):
        _, _, (k, r, cc, v) = ot.reg_terms(case["Z"][b], case["regs"], case["dt_off"])
        z0 = b * N * zd + k * zd
        keys.append((z0 + r) * nvar + z0 + cc)
        vals.append(LD(case["sigma"]) * v)
        tri.append(np.zeros(len(k), dtype=int))
    keys, vals, tri = np.concatenate(keys), np.concatenate(vals), np.concatenate(tri)
    ukeys, uvals = sum_duplicates(keys, vals)
    term_of = np.zeros(len(ukeys), dtype=int)
    np.maximum.at(term_of, np.searchsorted(ukeys, keys), tri)
    knot = (ukeys // nvar) // zd
    labels = np.where(term_of > 0, np.char.add("tri@", (term_of - 1).astype(str)), np.char.add("reg@", knot.astype(str)))
    return ukeys, uvals, labels


def sum_duplicates(keys, vals):
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    first = np.concatenate([[True], keys[1:] != keys[:-1]])
    return keys[first], np.add.reduceat(vals, np.flatnonzero(first))


def grad_labels(case):
    """Segment of every gradient entry: the terminal states' entries of a buffer ("x@b"), every other entry by knot and buffer ("k@b")."""
    nbuf, N, zd = case["Z"].shape
    lab = np.empty((nbuf, N, zd), dtype="U12")
    for b in range(nbuf):
        for k in range(N):
            lab[b, k] = "k%d@%d" % (k, b)
        for o in case["x_offs"]:
            if case["goal"] is not None:
                lab[b, N - 1, o : o + case["x_dim"]] = "x@%d" % b
    return lab


# ---- F, G: derivative rows and the reduce payload ---------------------------------------------------------------------------------------------
def payload_case(name):
    """(oracle layout, G0, Gj, Z [nbuf, N, z_dim], x_offs, weights, traj, state_cols) of a payload case: knot [states | dt | t | u (m) | du (m)]."""
    from oracle import pade_oracle as po
    from shape_cases import random_sparse_iso_system

    d, m, N, M, traj, vec = PAYLOAD_CASES[name]
    rng = np.random.default_rng(5000 + sum(map(ord, name)))
    n = d if vec else 2 * d
    xd = n if vec else n * d
    z_dim = M * xd + 2 + 2 * m
    lay = po.Layout(d=0 if vec else d, m=m, N=N, z_dim=z_dim, x_off=0, u_off=M * xd + 2, dt_off=M * xd, cols=1 if vec else None, gen=n if vec else None)
    if name == "Ptraj6":
        G0, Gj = random_sparse_iso_system(d, m, rng)
    else:
        G0, Gj = _system(n, m, rng)
    Z = 0.4 * rng.standard_normal((traj or 1, N, z_dim))
    Z[:, :, lay.dt_off] = 0.05 + 0.1 * rng.random((traj or 1, N))
    batch = traj or M
    weights = 0.5 + rng.random(batch)
    return lay, G0, Gj, Z, [b * xd for b in range(M)], weights, traj, (-1 if vec else 0)


# name: (d, m, N, members, TRAJ seeds, compact-density vector state)
PAYLOAD_CASES = {
    "P7": (4, 7, 5, 2, 0, False),  # m + 2 = 9 jobs: wave 0 runs a second pass
    "P9": (4, 9, 4, 1, 0, False),
    "P24": (4, 24, 4, 2, 0, False),  # the ABI's most drives: 26 jobs, four passes for waves 0 and 1
    "Podd": (9, 8, 5, 1, 6, True),  # levels = 3: n = 9 odd, the scalar loads; six output sets
    "Ptraj6": (9, 2, 5, 1, 6, False),  # a pattern-compiled system: the fused carrier where it applies; six output sets
}
