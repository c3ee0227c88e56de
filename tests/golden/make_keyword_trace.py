"""The keyword trace of the Python mirror: what the constructors of piccolo_jl_amd.integrators answer to every combination of their service
keywords before any device call, and what a context's attributes hold after construction, after every gate option and after a member window.
tests/test_keyword_trace_cpu.py and tests/test_keyword_trace_gpu.py run `run_case` on the cases of `CASES` and compare with
tests/golden/keyword_trace.json for equality; this file run as a script writes that table:

    python tests/golden/make_keyword_trace.py checks [out.json]     (any machine)
    python tests/golden/make_keyword_trace.py state [out.json]      (on an MI355X; keeps the other part of an existing table)

Two groups of cases (make_service_trace.py, beside this file, has the C library's side: its contexts are created with none of these keywords):

checks    one case per constructor of CTORS, no GPU.  `_lib.load` -- the name integrators calls -- is replaced by a function that raises a
          sentinel, so the outcome is the same with and without a device: the ValueError's full text; "reached" (every keyword check passed,
          the library would have been loaded); else the exception's class name.  The grid of a constructor (`grid`): pade_order of ORDERS x
          exp_hessian of False, True, "workspace" x every subset of up to three of the boolean keywords it accepts; then the invalid
          exp_hessian values 2 and "tiles" alone at every order; then each boolean keyword it does not accept, alone (its TypeError).
          _PclContext gets placeholder shapes (the loader comes before they are looked at); the public constructors a two-level system and
          a 4-knot trajectory.
state     one case per kind of KINDS, on the GPU; no kernel is launched.  A FRESH CONTEXT PER ROW keeps the rows independent:
          construct  the snapshot after construction through the mirror under every keyword state of `keyword_states` (none; each service
                     keyword by itself, exp_hessian as True and as "workspace"; large_full beside the kind's reduce keyword on the kinds
                     created with large_generator) -- or the error the constructor raises;
          options    per key of GATE_KEYS on a context without keywords: set_option(key, 1), (key, 0), (key, 1), the snapshot or the PclError
                     after each;
          window     on the two-member kinds, per keyword state that constructs: set_member_window(1, 1), then set_member_window().
          The kinds: make_service_trace.py's (same shapes, same systems); plain_lg and exp_lg, the d = 4 contexts created with
          large_generator=True (and large_exp=True): the large keywords at n <= 64, where no option is set; plain2, exp2 and large2, two
          members of one system under PCL_BATCH_MEMBERS.

In the table every distinct text is stored once (`texts`) and every distinct snapshot once (`snaps`, values in the order of SNAP), both
referred to by index; a checks row is the list of its grid's outcomes in the grid's order."""
import importlib.util
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_service_trace", os.path.join(HERE, "make_service_trace.py"))
svc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(svc)  # (puts the repository's root and tests/ on sys.path)

import piccolo_jl_amd as pa  # noqa: E402

LIB = pa._lib
PI = pa.integrators

# ---- checks ---------------------------------------------------------------------------------------------------------------------------------
ORDERS = [0, 4, 10, "exp", -1]
EXP_HESSIAN = [False, True, "workspace"]
EXP_HESSIAN_INVALID = [2, "tiles"]
BOOLS = ["exp_full", "var_compact", "large_generator", "large_hessian", "large_full", "large_reduce", "large_exp", "large_exp_hessian", "large_exp_reduce",
         "large_variational"]  # fmt: skip
_PLAIN = [k for k in BOOLS if k != "large_variational"]
_VAR = [k for k in _PLAIN if k != "exp_full"]
# constructor -> the boolean keywords it accepts
CTORS = {"ctx-members": BOOLS, "ctx-traj": BOOLS, "ctx-variational": BOOLS, "ctx-variational_exp": BOOLS, "pade": _PLAIN, "bilinear-one": _PLAIN,
         "bilinear-list": _PLAIN, "variational-ket": _VAR, "variational-unitary": _VAR}  # fmt: skip
_MODES = {"ctx-members": LIB.PCL_BATCH_MEMBERS, "ctx-traj": LIB.PCL_BATCH_TRAJ, "ctx-variational": LIB.PCL_BATCH_VARIATIONAL,
          "ctx-variational_exp": LIB.PCL_BATCH_VARIATIONAL_EXP}  # fmt: skip


def grid(ctor):
    """[(pade_order, exp_hessian, keywords switched on)] of a constructor, in the table's order."""
    subsets = [s for r in range(4) for s in itertools.combinations(CTORS[ctor], r)]
    return ([(o, eh, s) for o in ORDERS for eh in EXP_HESSIAN for s in subsets] + [(o, eh, ()) for o in ORDERS for eh in EXP_HESSIAN_INVALID]
            + [(4, False, (k,)) for k in BOOLS if k not in CTORS[ctor]])  # fmt: skip


class _Reached(Exception):
    pass


def _no_library():
    raise _Reached()


_PUBLIC = {}


def _public():
    """The two-level system and the 4-knot trajectory of the public constructors."""
    if not _PUBLIC:
        N, P = 4, pa.PAULIS
        U = np.zeros((8, N))
        U[:, 0] = pa.operator_to_iso_vec(np.eye(2))
        comps = {"u": np.zeros((2, N)), "Δt": np.full((1, N), 0.1)}
        for name in ("U1", "U2", "Uv"):
            comps[name] = U.copy()
        psi = np.zeros((4, N))
        psi[0, 0] = 1.0
        comps["psi"], comps["psiv"] = psi, np.zeros((4, N))
        _PUBLIC["traj"] = pa.NamedTrajectory(comps, controls=("u", "Δt"), timestep="Δt")
        _PUBLIC["sys"] = pa.QuantumSystem(P["Z"] / 2, [P["X"], P["Y"]], [1.0, 1.0])
        _PUBLIC["sys2"] = pa.QuantumSystem(P["Z"] / 3, [P["X"], P["Y"]], [1.0, 1.0])
        _PUBLIC["var"] = pa.VariationalQuantumSystem(P["Z"] / 2, [P["X"], P["Y"]], [P["Z"] / 2], [1.0, 1.0])
    return _PUBLIC


def _construct(ctor, kw):
    if ctor in _MODES:
        return PI._PclContext(d=2, m=2, N=4, z_dim=11, u_off=9, dt_off=8, x_offs=[0], G0=None, Gj=None, batch=1, batch_mode=_MODES[ctor], **kw)
    p = _public()
    if ctor == "pade":
        return pa.HipPadeIntegrator(p["sys"].G_drift, p["sys"].G_drives_array(), p["traj"], "U1", "u", **kw)
    if ctor == "bilinear-one":
        return pa.BilinearIntegrator(p["sys"], p["traj"], "U1", "u", **kw)
    if ctor == "bilinear-list":
        return pa.BilinearIntegrator([p["sys"], p["sys2"]], p["traj"], ["U1", "U2"], "u", **kw)
    if ctor == "variational-ket":
        return pa.VariationalKetIntegrator(p["var"], p["traj"], "psi", ["psiv"], "u", **kw)
    return pa.VariationalUnitaryIntegrator(p["var"], p["traj"], "U1", ["Uv"], "u", **kw)


def run_checks(case):
    out = []
    load = LIB.load
    LIB.load = _no_library
    try:
        for order, eh, on in grid(case["ctor"]):
            try:
                _construct(case["ctor"], dict({k: True for k in on}, pade_order=order, exp_hessian=eh))
                out.append("constructed")  # (never: the loader raises)
            except _Reached:
                out.append("reached")
            except ValueError as e:
                out.append(str(e))
            except Exception as e:
                out.append(type(e).__name__)
    finally:
        LIB.load = load
    return out


# ---- state ----------------------------------------------------------------------------------------------------------------------------------
SNAP = ["exponential", "large", "large_exp", "large_variational", "variational", "exp_hessian", "exp_full", "var_compact", "large_hessian", "large_full",
        "large_reduce", "large_exp_hessian", "large_exp_reduce", "hess_nnz", "hess_per", "compact_nnz", "compact_per", "jac_nnz", "jac_per", "n_rows", "window"]  # fmt: skip
GATE_KEYS = svc.GATES + ["var_exp_hess_tiles"]
M = svc.M
# kind -> (d, state_cols (0: unitary), variations, pade_order, N, large, members)
KINDS = {k: v + (1,) for k, v in svc.KINDS.items()}
KINDS.update({"plain_lg": (4, 0, 0, 4, 4, True, 1), "exp_lg": (4, 0, 0, "exp", 4, True, 1), "plain2": (4, 0, 0, 4, 4, False, 2),
              "exp2": (4, 0, 0, "exp", 4, False, 2), "large2": (33, 1, 0, 4, 3, True, 2)})  # fmt: skip
SINGLE = ["exp_full", "var_compact", "large_hessian", "large_full", "large_reduce", "large_exp_hessian", "large_exp_reduce"]


def keyword_states(kind):
    d, cols, v, order, N, large, members = KINDS[kind]
    states = [("none", {}), ("exp_hessian", {"exp_hessian": True}), ("exp_hessian-workspace", {"exp_hessian": "workspace"})] + [(k, {k: True}) for k in SINGLE]
    if large:
        reduce = "large_exp_reduce" if order == "exp" else "large_reduce"
        states.append(("large_full+" + reduce, {"large_full": True, reduce: True}))
    return states


def make_ctx(kind, **kw):
    d, cols, v, order, N, large, members = KINDS[kind]
    G0, Gj, Gv = svc.system(d)
    xdc = 2 * d * (cols or d)
    exp = order == "exp"
    if v:
        return PI._PclContext(d=d, m=M, N=N, z_dim=(v + 1) * xdc + 1 + M, u_off=(v + 1) * xdc + 1, dt_off=(v + 1) * xdc, x_offs=[b * xdc for b in range(v + 1)],
                              G0=np.concatenate([G0[None], Gv[None]]), Gj=Gj, batch=1 + v, per_member_G0=True, pade_order=order, state_cols=cols,
                              batch_mode=LIB.PCL_BATCH_VARIATIONAL_EXP if exp else LIB.PCL_BATCH_VARIATIONAL, large_generator=large, large_variational=large, **kw)  # fmt: skip
    return PI._PclContext(d=d, m=M, N=N, z_dim=members * xdc + 1 + M, u_off=members * xdc + 1, dt_off=members * xdc, x_offs=[b * xdc for b in range(members)],
                          G0=G0, Gj=Gj, batch=members, batch_mode=LIB.PCL_BATCH_MEMBERS, pade_order=order, state_cols=cols, large_generator=large,
                          large_exp=large and exp, **kw)  # fmt: skip


def _snap(c):
    return {"snap": {k: (list(getattr(c, k)) if k == "window" else getattr(c, k)) for k in SNAP}}


def _error(e):
    return {"error": [type(e).__name__, getattr(e, "code", None), str(e)]}


def _after(c, f, *args):
    try:
        f(*args)
    except pa.PclError as e:
        return _error(e)
    return _snap(c)


def run_state(case):
    kind = case["kind"]
    out = dict(construct={}, options={}, window={})
    for name, kw in keyword_states(kind):
        try:
            c = make_ctx(kind, **kw)
        except (ValueError, pa.PclError) as e:
            out["construct"][name] = _error(e)
            continue
        try:
            out["construct"][name] = _snap(c)
            if KINDS[kind][6] > 1:
                out["window"][name] = [_after(c, c.set_member_window, 1, 1), _after(c, c.set_member_window)]
        finally:
            c.close()
    for key in GATE_KEYS:
        c = make_ctx(kind)
        try:
            out["options"][key] = [_after(c, c.set_option, key, v) for v in (1, 0, 1)]
        finally:
            c.close()
    return out


CASES = [dict(id="checks-%s" % c, group="checks", ctor=c) for c in CTORS] + [dict(id="state-%s" % k, group="state", kind=k) for k in KINDS]


def run_case(case):
    return dict(checks=run_checks, state=run_state)[case["group"]](case)


# ---- the table's compact form: texts and snapshots by index ---------------------------------------------------------------------------------------
def _index(table, x):
    if x not in table:
        table.append(x)
    return table.index(x)


def _pack(r, texts, snaps):
    if isinstance(r, str):
        return _index(texts, r)
    if isinstance(r, list):
        return [_pack(x, texts, snaps) for x in r]
    if "snap" in r:
        return {"snap": _index(snaps, [r["snap"][k] for k in SNAP])}
    if "error" in r:
        return {"error": r["error"][:2] + [_index(texts, r["error"][2])]}
    return {k: _pack(x, texts, snaps) for k, x in r.items()}


def unpack(p, texts, snaps):
    """The inverse of _pack: what run_case returns."""
    if isinstance(p, int):
        return texts[p]
    if isinstance(p, list):
        return [unpack(x, texts, snaps) for x in p]
    if "snap" in p:
        return {"snap": dict(zip(SNAP, snaps[p["snap"]]))}
    if "error" in p:
        return {"error": p["error"][:2] + [texts[p["error"][2]]]}
    return {k: unpack(x, texts, snaps) for k, x in p.items()}


def header():
    return dict(orders=ORDERS, exp_hessian=EXP_HESSIAN + EXP_HESSIAN_INVALID, ctors=CTORS, snap=SNAP, gate_keys=GATE_KEYS,
                kinds={k: list(v) for k, v in KINDS.items()}, states={k: [s for s, _ in keyword_states(k)] for k in KINDS})


def main(group, path):
    table = dict(texts=[], snaps=[], cases=[])
    if os.path.exists(path):
        with open(path) as f:
            table = json.load(f)
    kept = {row["id"]: row for row in table["cases"] if row["group"] != group}
    rows = []
    for case in CASES:
        if case["group"] == group:
            rows.append(dict(case, expect=_pack(json.loads(json.dumps(run_case(case))), table["texts"], table["snaps"])))
            print(case["id"], "ok", flush=True)
        elif case["id"] in kept:
            rows.append(kept[case["id"]])
    table.update(header(), cases=rows)
    with open(path, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "keyword_trace.json"))
