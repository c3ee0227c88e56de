"""The service trace of the context kinds: which entry point each kind of context serves under which gate option, the code and the text it is
refused with otherwise, and what every option key accepts, stores and reads back.  tests/test_service_trace_gpu.py runs `run_case` on every
case of `CASES` and compares with tests/golden/service_trace.json for equality; this file run as a script (on an MI355X) writes that table:

    python tests/golden/make_service_trace.py [out.json]

Everything goes through the C ABI itself (ctypes on the library the Python mirror loads; the mirror only creates the contexts, with none of
its option keywords), one fresh context per case.  Four groups of cases:

service   one context per kind and option state (every gate option off; each of GATES on by itself; large_full with the kind's reduce option):
          the gate options are set, their codes and texts recorded, and -- where every set was accepted -- each entry point of CALLS is called
          once, in that order, on valid buffers (device arrays of CAP doubles, checked against the context's own sizes before anything is
          launched): code and pcl_last_error text of each, then pcl_sync and the context's last_* values.
host      the host-pointer pcl_eval_jac on the kinds with more than one state column, under host_path 0 and 2, for each reduce / compact option
          state: code, text and last_kernel (the compact route or the full one).
options   per kind and key of KEYS (every key either chain of pcl_host_options.hpp names, the PCL_LAB / PCL_PROFILE ones included: the shipped
          library refuses them as unknown): pcl_set_option with each of VALUES, pcl_get_option of the same key after each.  A FRESH CONTEXT PER
          KEY keeps the rows independent (within a key the values follow each other on one context, in the order of VALUES).
readonly  per kind: every key read once on a fresh context, and once more after every key has been set to 1 in the order of KEYS.

Values that depend on the machine or the process are recorded as null: n_cu, occupancy_v2, jit_*, cgroup_quota_cpus_x100, host_expand_MBps,
and host_threads while it is at auto (after a set of a value <= 0, and on a fresh context).

Shapes: the smallest each kind accepts.  plain, exp, var (v = 1) and var_exp (v = 1) at d = 4, m = 2, N = 4, unitary states; the large kets
(large, large_exp, large_var with v = 1) at d = 33 (n = 66), one state column, m = 2, N = 3; large_u and large_exp_u the same as unitary
problems (33 state columns: pcl_eval_jac_merit_objective_dev needs a unitary goal, the host route's compact path more than one column).
No launch here has more than three intervals.

In the table every distinct text is stored once (`texts`) and referred to by index, every distinct block of option rows once (`patterns`);
per-key entries are lists in the order of KEYS, per-call entries in the order of CALLS, the last_* values in the order of LAST."""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import piccolo_jl_amd as pa  # noqa: E402
from oracle import pade_oracle as po  # noqa: E402

LIB = pa._lib
CAP = 1 << 21  # doubles per buffer; every size a call needs is checked against it first
VALUES = [-2, -1, 0, 1, 2, 3, 4, 5, 8, 9, 16, 256, 512, 3000000]
GATES = ["exp_hess", "exp_full", "var_full", "var_compact", "var_exp_hess", "large_hess", "large_full", "large_reduce", "large_exp_hess", "large_exp_reduce"]
# kind -> (d, state_cols (0: unitary), variations, pade_order, N, large)
KINDS = {
    "plain": (4, 0, 0, 4, 4, False),
    "exp": (4, 0, 0, "exp", 4, False),
    "var": (4, 0, 1, 4, 4, False),
    "var_exp": (4, 0, 1, "exp", 4, False),
    "large": (33, 1, 0, 4, 3, True),
    "large_exp": (33, 1, 0, "exp", 3, True),
    "large_var": (33, 1, 1, 4, 3, True),
    "large_u": (33, 0, 0, 4, 3, True),
    "large_exp_u": (33, 0, 0, "exp", 3, True),
}
SEVEN = ["plain", "exp", "var", "var_exp", "large", "large_exp", "large_var"]
LARGE_KINDS = ["large", "large_exp", "large_var", "large_u", "large_exp_u"]
REDUCE = {"exp": "exp_full", "var": "var_compact", "var_exp": "var_compact", "large": "large_reduce", "large_exp": "large_exp_reduce", "large_var": "large_reduce",
          "large_u": "large_reduce", "large_exp_u": "large_exp_reduce"}  # fmt: skip
HOST_KINDS = ["plain", "exp", "var", "var_exp", "large_u", "large_exp_u"]  # more than one state column
M = 2

# every key of pcl_set_option's chain, in its order ...
SET_KEYS = ["cols_per_slice", "use_mfma", "nt_stores", "grid", "var_block_wgs", "var_col_wgs", "var_full", "exp_hess", "exp_full", "var_compact", "var_large_drives",
            "var_exp_hess", "large_hess", "large_hess_drives", "large_exp_drives", "large_exp_hess", "large_exp_hess_drives", "large_exp_reduce", "large_full",
            "large_reduce", "large_rollout_stage", "var_exp_hess_tiles", "profile_flags", "v4_variant", "host_threads", "host_path", "host_chunks", "specialize", "jit",
            "require_jit", "general_threads", "general_kernel_version", "general_slices", "general_pade_kernel", "stream_workgroups", "contiguous",
            "objective_launches", "v4_flags", "v4_ticket", "v4_one_item", "v4_ticket_cols", "v4_ticket_ahead", "v4_group", "v4_power_tiles", "v4_tail_mode", "v4_tune",
            "host_store_bytes", "resident_idle_us", "hess_xcd", "hess_rpre", "hess_pair", "hess_split", "eval_coop", "eval_kernel", "hess_kernel", "debug_timing",
            "kernel_version"]  # fmt: skip
# ... and the keys pcl_get_option's chain names beside them
GET_ONLY_KEYS = ["effective_cols_per_slice", "n_cu", "variations", "large_variational", "host_expand_MBps", "last_kernel", "last_hess_rpre", "last_hess_pair",
                 "resident_launches", "last_v4_tune_choice", "last_v4_tune_static_ns", "last_v4_tune_ticket_ns", "cgroup_quota_cpus_x100", "last_hess_split",
                 "last_eval_coop", "last_objective_launches", "last_step_launches", "last_merit_fused", "jit_compiles", "jit_cache_hits", "jit_fallbacks", "pade_order",
                 "order_tol_met", "order_theta_1e9", "last_stream_workgroups", "last_v4_ticket", "last_v4_one_item", "last_hess_kernel", "ell_width_t",
                 "drives_antisymmetric", "occupancy_v2", "iso_structured", "ell_width", "union_width"]  # fmt: skip
KEYS = SET_KEYS + GET_ONLY_KEYS
MACHINE = {"n_cu", "occupancy_v2", "jit_compiles", "jit_cache_hits", "jit_fallbacks", "cgroup_quota_cpus_x100", "host_expand_MBps"}  # values recorded as null
LAST = ["last_kernel", "last_hess_kernel", "last_step_launches", "last_objective_launches", "last_merit_fused"]

# the entry points of the service part, in calling order
CALLS = ["add_regularizer", "objective_hess_nnz", "objective_hess_structure", "objective_hess_dev", "objective_hess", "objective_dev", "objective", "set_weights",
         "set_goal", "infidelity_dev", "objective_dev_goal", "eval_jac_merit_objective_dev", "set_goal_subspace", "set_goal_form", "clear_regularizers",
         "rollout_dev", "rollout", "hess_nnz", "hess_structure_i64", "hess_dev", "hess", "jac_compact_nnz", "eval_jac_compact_dev", "jac_expand_dev",
         "merit_grad_len", "eval_jac_merit_dev", "merit_grad_dev", "comm_init", "reduce_sum_dev", "reduce_sum", "set_member_window", "sync"]  # fmt: skip


def service_states(kind):
    states = [("off", [])] + [(g, [g]) for g in GATES]
    if kind in LARGE_KINDS:
        states.append(("large_full+" + REDUCE[kind], ["large_full", REDUCE[kind]]))
    return states


def host_states(kind):
    return [("off", [])] + ([(REDUCE[kind], [REDUCE[kind]])] if kind in REDUCE else [])


CASES = (
    [dict(id="service-%s-%s" % (k, s), group="service", kind=k, set=opts) for k in KINDS for s, opts in service_states(k)]
    + [dict(id="host-%s-%s-path%d" % (k, s, hp), group="host", kind=k, set=opts, host_path=hp) for k in HOST_KINDS for s, opts in host_states(k) for hp in (0, 2)]
    + [dict(id="options-%s" % k, group="options", kind=k) for k in SEVEN]
    + [dict(id="readonly-%s" % k, group="readonly", kind=k) for k in SEVEN]
)


def _herm(d, rng, scale):
    A = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return scale * (A + A.conj().T)


_SYSTEMS = {}


def system(d):
    """(G0, Gj, Gv) of dimension n = 2 d from a fixed seed: dense Hermitian drift, drives and one variation generator."""
    if d not in _SYSTEMS:
        rng = np.random.default_rng(4100 + d)
        s = 0.5 / d
        _SYSTEMS[d] = (po.G_of_H(_herm(d, rng, s)), np.array([po.G_of_H(_herm(d, rng, s)) for _ in range(M)]), po.G_of_H(_herm(d, rng, s)))
    return _SYSTEMS[d]


def make_ctx(kind):
    d, cols, v, order, N, large = KINDS[kind]
    G0, Gj, Gv = system(d)
    C = cols or d
    xdc = 2 * d * C
    z_dim = (v + 1) * xdc + 1 + M
    exp = order == "exp"
    if v:
        return pa.integrators._PclContext(d=d, m=M, N=N, z_dim=z_dim, u_off=(v + 1) * xdc + 1, dt_off=(v + 1) * xdc, x_offs=[b * xdc for b in range(v + 1)],
                                          G0=np.concatenate([G0[None], Gv[None]]), Gj=Gj, batch=1 + v, per_member_G0=True, pade_order=order, state_cols=cols,
                                          batch_mode=LIB.PCL_BATCH_VARIATIONAL_EXP if exp else LIB.PCL_BATCH_VARIATIONAL, large_generator=large, large_variational=large)  # fmt: skip
    return pa.integrators._PclContext(d=d, m=M, N=N, z_dim=z_dim, u_off=xdc + 1, dt_off=xdc, x_offs=[0], G0=G0, Gj=Gj, batch=1, batch_mode=LIB.PCL_BATCH_MEMBERS,
                                      pade_order=order, state_cols=cols, large_generator=large, large_exp=large and exp)  # fmt: skip


_BUF = {}


def buffers():
    """Device and host arrays of CAP doubles each, made once: inputs (z, lam) random, outputs apart from them and from each other."""
    if not _BUF:
        import torch

        rng = np.random.default_rng(77)
        _BUF["hz"] = 0.1 * rng.standard_normal(CAP)
        _BUF["hlam"] = rng.standard_normal(CAP)
        for name in ("hout", "hval", "hgrad", "hx"):
            _BUF[name] = np.zeros(CAP)
        for name in ("hrows", "hcols"):
            _BUF[name] = np.zeros(CAP, dtype=np.int64)
        _BUF["dz"] = torch.from_numpy(_BUF["hz"]).cuda()
        _BUF["dlam"] = torch.from_numpy(_BUF["hlam"]).cuda()
        for name in ("ddelta", "dvals", "dcomp", "dout", "dval", "dgrad", "dx"):
            _BUF[name] = torch.zeros(CAP, dtype=torch.float64, device="cuda")
        L = LIB.load()
        vp, i32, f64, i64p = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.POINTER(ctypes.c_int64)
        L.pcl_set_goal_form.argtypes = [vp, i32, i32, vp, vp]
        L.pcl_objective_hess_nnz.argtypes = [vp, i64p]
        L.pcl_objective_hess_structure.argtypes = [vp, vp, vp]
        L.pcl_objective_hess.argtypes = [vp, vp, f64, f64, vp]
        L.pcl_objective_hess_dev.argtypes = [vp, vp, f64, f64, vp]
    return _BUF


def _p(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def _err(c):
    return (c._L.pcl_last_error(c._h) or b"").decode()


def _set(c, key, v):
    rc = c._L.pcl_set_option(c._h, key.encode(), v)
    return [rc, _err(c) if rc else ""]


def _get(c, key):
    out = ctypes.c_int64()
    rc = c._L.pcl_get_option(c._h, key.encode(), ctypes.byref(out))
    return rc, (out.value if rc == 0 else None)


def run_service(case):
    B = buffers()
    c = make_ctx(case["kind"])
    try:
        L, h = c._L, c._h
        assert c.z_len <= CAP and c.jac_nnz <= CAP and c.n_rows <= CAP and c.N * c.x_dim * c.batch <= CAP, "a buffer of CAP doubles is too small"
        out = dict(set=[_set(c, key, 1) for key in case["set"]], calls=None, last=None)
        if any(rc for rc, _ in out["set"]):
            return out
        a, b = ctypes.c_int64(), ctypes.c_int64()
        sub = (ctypes.c_int32 * 2)(0, 1)
        comm_id = ctypes.create_string_buffer(256)
        dz, dlam, hz, hlam = _p(B["dz"]), _p(B["dlam"]), _p(B["hz"]), _p(B["hlam"])
        ddelta, dvals, dcomp, dout, dval, dgrad, dx = (_p(B[k]) for k in ("ddelta", "dvals", "dcomp", "dout", "dval", "dgrad", "dx"))
        hout, hval, hgrad, hx, hrows, hcols = (_p(B[k]) for k in ("hout", "hval", "hgrad", "hx", "hrows", "hcols"))

        def counted(f, *args):  # a count that a later call sizes its output by: it must fit the buffers
            rc = f(h, *args)
            assert rc != 0 or a.value <= CAP, "a buffer of CAP doubles is too small for %d values" % a.value
            return rc

        calls = {
            "add_regularizer": lambda: L.pcl_add_regularizer(h, c.z_dim - M, M, hlam, 1),
            "objective_hess_nnz": lambda: counted(L.pcl_objective_hess_nnz, ctypes.byref(a)),
            "objective_hess_structure": lambda: L.pcl_objective_hess_structure(h, hrows, hcols),
            "objective_hess_dev": lambda: L.pcl_objective_hess_dev(h, dz, 1.0, 1.0, dvals),
            "objective_hess": lambda: L.pcl_objective_hess(h, hz, 1.0, 1.0, hout),
            "objective_dev": lambda: L.pcl_objective_dev(h, dz, 1.0, dval, dgrad),
            "objective": lambda: L.pcl_objective(h, hz, 1.0, hval, hgrad),
            "set_weights": lambda: L.pcl_set_weights(h, hlam),
            "set_goal": lambda: L.pcl_set_goal(h, hlam),
            "infidelity_dev": lambda: L.pcl_infidelity_dev(h, dz, 1.0, dval, dgrad),
            "objective_dev_goal": lambda: L.pcl_objective_dev(h, dz, 1.0, dval, dgrad),
            "eval_jac_merit_objective_dev": lambda: L.pcl_eval_jac_merit_objective_dev(h, dz, dlam, ddelta, dvals, dout, 1.0, dval, dgrad),
            "set_goal_subspace": lambda: L.pcl_set_goal_subspace(h, hlam, sub, 2),
            "set_goal_form": lambda: L.pcl_set_goal_form(h, 0, 1, hlam, None),
            "clear_regularizers": lambda: L.pcl_clear_regularizers(h),
            "rollout_dev": lambda: L.pcl_rollout_dev(h, dz, dx),
            "rollout": lambda: L.pcl_rollout(h, hz, hx),
            "hess_nnz": lambda: counted(L.pcl_hess_nnz, ctypes.byref(a), ctypes.byref(b)),
            "hess_structure_i64": lambda: L.pcl_hess_structure_i64(h, ctypes.cast(hrows, ctypes.POINTER(ctypes.c_int64)), ctypes.cast(hcols, ctypes.POINTER(ctypes.c_int64))),
            "hess_dev": lambda: L.pcl_hess_dev(h, dz, dlam, dvals),
            "hess": lambda: L.pcl_hess(h, hz, hlam, hout),
            "jac_compact_nnz": lambda: counted(L.pcl_jac_compact_nnz, ctypes.byref(a), ctypes.byref(b)),
            "eval_jac_compact_dev": lambda: L.pcl_eval_jac_compact_dev(h, dz, ddelta, dcomp),
            "jac_expand_dev": lambda: L.pcl_jac_expand_dev(h, dcomp, dvals),
            "merit_grad_len": lambda: counted(L.pcl_merit_grad_len, ctypes.byref(a), ctypes.byref(b)),
            "eval_jac_merit_dev": lambda: L.pcl_eval_jac_merit_dev(h, dz, dlam, ddelta, dvals, dout),
            "merit_grad_dev": lambda: L.pcl_merit_grad_dev(h, ddelta, dlam, dvals, dout),
            "comm_init": lambda: L.pcl_comm_init(h, comm_id, 1, 1),  # (rank 1 of 1: refused by its argument check, behind the gate)
            "reduce_sum_dev": lambda: L.pcl_reduce_sum_dev(h, dout, 4),  # (no communicator: refused, behind the gate)
            "reduce_sum": lambda: L.pcl_reduce_sum(h, hout, 4),
            "set_member_window": lambda: L.pcl_set_member_window(h, 0, 1),
            "sync": lambda: L.pcl_sync(h),
        }
        out["calls"] = []
        for name in CALLS:
            rc = calls[name]()
            out["calls"].append([rc, _err(c) if rc else ""])
        out["last"] = {key: _get(c, key)[1] for key in LAST}
        return out
    finally:
        c.close()


def run_host(case):
    B = buffers()
    c = make_ctx(case["kind"])
    try:
        assert c.z_len <= CAP and c.jac_nnz <= CAP and c.n_rows <= CAP, "a buffer of CAP doubles is too small"
        out = dict(set=[_set(c, key, 1) for key in case["set"]] + [_set(c, "host_path", case["host_path"])])
        rc = c._L.pcl_eval_jac(c._h, _p(B["hz"]), _p(B["hout"]), _p(B["hx"]))
        out["eval_jac"] = [rc, _err(c) if rc else ""]
        out["last_kernel"] = _get(c, "last_kernel")[1]
        return out
    finally:
        c.close()


def _value(key, v, auto):
    return None if key in MACHINE or (key == "host_threads" and auto) else v


def run_options(case):
    out = {}
    for key in KEYS:
        c = make_ctx(case["kind"])
        try:
            rows = []
            for v in VALUES:
                s = _set(c, key, v)
                rc, got = _get(c, key)
                rows.append(s + [rc, _value(key, got, v <= 0 or s[0] != 0)])
            out[key] = rows
        finally:
            c.close()
    return out


def run_readonly(case):
    c = make_ctx(case["kind"])
    try:
        def read():
            return {key: [rc, _value(key, got, True)] for key in KEYS for rc, got in [_get(c, key)]}

        fresh = read()
        for key in KEYS:
            _set(c, key, 1)
        after = {key: [rc, None if key in MACHINE else got] for key in KEYS for rc, got in [_get(c, key)]}  # (host_threads = 1: no longer at auto)
        return dict(fresh=fresh, after=after)
    finally:
        c.close()


def run_case(case):
    return dict(service=run_service, host=run_host, options=run_options, readonly=run_readonly)[case["group"]](case)


# ---- the table's compact form: texts and blocks of option rows by index ------------------------------------------------------------------
def _pack(result, group, texts, patterns):
    def t(s):
        if s not in texts:
            texts.append(s)
        return texts.index(s)

    def pair(p):
        return [p[0], t(p[1])]

    if group == "service":
        return dict(set=[pair(p) for p in result["set"]], calls=None if result["calls"] is None else [pair(p) for p in result["calls"]],
                    last=None if result["last"] is None else [result["last"][key] for key in LAST])
    if group == "host":
        return dict(set=[pair(p) for p in result["set"]], eval_jac=pair(result["eval_jac"]), last_kernel=result["last_kernel"])
    if group == "options":
        packed = []
        for key in KEYS:
            block = [[r[0], t(r[1]), r[2], r[3]] for r in result[key]]
            if block not in patterns:
                patterns.append(block)
            packed.append(patterns.index(block))
        return packed
    return dict(fresh=[result["fresh"][key] for key in KEYS], after=[result["after"][key] for key in KEYS])


def unpack(packed, group, texts, patterns):
    """The inverse of _pack: what run_case returns."""
    def pair(p):
        return [p[0], texts[p[1]]]

    if group == "service":
        return dict(set=[pair(p) for p in packed["set"]], calls=None if packed["calls"] is None else [pair(p) for p in packed["calls"]],
                    last=None if packed["last"] is None else dict(zip(LAST, packed["last"])))
    if group == "host":
        return dict(set=[pair(p) for p in packed["set"]], eval_jac=pair(packed["eval_jac"]), last_kernel=packed["last_kernel"])
    if group == "options":
        return {key: [[r[0], texts[r[1]], r[2], r[3]] for r in patterns[i]] for key, i in zip(KEYS, packed)}
    return dict(fresh=dict(zip(KEYS, packed["fresh"])), after=dict(zip(KEYS, packed["after"])))


def main(path):
    texts, patterns, rows = [""], [], []
    for case in CASES:
        r = run_case(case)
        rows.append(dict(case, expect=_pack(r, case["group"], texts, patterns)))
        print(case["id"], "ok", flush=True)
    with open(path, "w") as f:
        json.dump(dict(calls=CALLS, values=VALUES, keys=KEYS, last=LAST, texts=texts, patterns=patterns, cases=rows), f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "service_trace.json"))
