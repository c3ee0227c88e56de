"""Host-side mirror of the reference's integrator plug-in surface for the unitary
Pade collocation constraint, backed by libpiccolo_hip.so (HIP kernels, gfx950).

What the reference calls (Piccolo.jl v2.0.2; [EXT] = DirectTrajOpt.jl):

  BilinearIntegrator(qtraj::UnitaryTrajectory, N)          src/control/integrators.jl:35-51
  BilinearIntegrator(qtraj::SamplingTrajectory, N)         src/control/integrators.jl:134-162
  B.dim, B.x_dim, B.x_name / B.x_names, B.f(x', x, u, dt)  src/control/integrators.jl:307-309,525,552
  evaluate!(delta, B, traj) [EXT]                          src/control/integrators.jl:311,777
  eval_jacobian(B, traj) [EXT]  -> (B.dim, traj.dim*traj.N + traj.global_dim)   :780-783
  hessian_structure / Hessian of the Lagrangian [EXT]      test/aqua.jl:6-9

Here the same names exist as Python callables (``evaluate_`` for ``evaluate!``).
All arithmetic happens on the GPU through the C ABI; nothing in this module
computes a residual or a Jacobian on the host, and nothing falls back to a CPU
implementation when the library or the device is missing.
"""
import collections
import ctypes

import numpy as np

from . import _lib
from ._lib import PCL_BATCH_MEMBERS, PCL_BATCH_TRAJ, PCL_BATCH_VARIATIONAL, PCL_BATCH_VARIATIONAL_EXP, PCL_LARGE_VAR_EXP, PclError
from .trajectory import STATE, TIMESTEP, NamedTrajectory

__all__ = [
    "HipPadeIntegrator", "HipPadeMemberIntegrator", "HipPadeMultistart", "DerivativeIntegrator", "BilinearIntegrator", "evaluate_", "eval_jacobian",
    "jacobian_structure", "hessian_structure", "eval_hessian_of_lagrangian", "PclError", "HipVariationalIntegrator", "VariationalUnitaryIntegrator",
    "VariationalKetIntegrator", "variational_rollout",
]  # fmt: skip


def _colmajor(A):
    """numpy [i, j] matrix (or stack of matrices) -> flat column-major float64 buffer."""
    A = np.asarray(A, dtype=np.float64)
    return np.ascontiguousarray(np.swapaxes(A, -1, -2)).reshape(-1)


def _ptr(a):
    """Address of a host numpy array or a torch (device) tensor."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if a.dtype != np.float64 or not a.flags.c_contiguous:
            raise TypeError("expected a C-contiguous float64 array")
        return a.ctypes.data
    if hasattr(a, "data_ptr"):  # torch tensor
        if str(a.dtype) != "torch.float64" or not a.is_contiguous():
            raise TypeError("expected a contiguous float64 tensor")
        return a.data_ptr()
    raise TypeError("unsupported buffer type %r" % type(a))


# ---------------------------------------------------------------------------
# The service keywords: what each means, stated once.  The constructors below name the ones they accept and point here.
#
# exp_hessian        ``False`` | ``True`` | ``"workspace"`` (anything else: ``ValueError``).  ``True``, with ``pade_order="exp"`` only: the Hessian of
#                    the Lagrangian of the exponential constraint is served (second Frechet derivatives of exp; the library's option ``exp_hess``,
#                    generator dimensions up to 62).  On a variational context the option is ``var_exp_hess`` (third Frechet derivatives, nine LDS
#                    tiles: dimensions up to 44, beyond that the constructor raises the library's PCL_ESHAPE message); ``"workspace"`` sets
#                    ``var_exp_hess_tiles`` = 1 first: where nine tiles exceed the LDS (dimensions 46 .. 62) four of them live in a device
#                    workspace, elsewhere nothing changes.  ``"workspace"`` is the variational constructors' only.
# exp_full           with ``pade_order="exp"`` on a plain context only: the compact Jacobian, the host-pointer calls' compact path and the merit /
#                    reduce payload are served on that constraint too (option ``exp_full``).
# var_compact        on a variational context only (any Pade order, or ``"exp"``): the compact Jacobian of the stacked state -- every distinct tile
#                    once, ``ctx.compact_per`` values per interval -- its device expansion and the host-pointer calls' compact path.
# large_generator    the flag ``PCL_LARGE_N``: generator dimensions 66 .. 128 (a transmon with a cavity, density vectors of 9 .. 11 levels) on the Pade
#                    constraint, residual and Jacobian only -- the Hessian of the Lagrangian, the rollout, the objective, the compact Jacobian and
#                    the payload raise the library's message unless the keywords below switch them on; solve with a quasi-Newton Hessian.  Without it
#                    such a system is refused as before; at a dimension up to 64 it changes nothing and none of the large options is set (the
#                    ordinary context serves everything as always).  With ``pade_order="exp"`` the library refuses it unless ``large_exp=True``.
#                    On a variational constructor it sets ``PCL_LARGE_N | PCL_LARGE_VAR`` (``large_variational`` on the context): residual and
#                    Jacobian of the Pade constraint, nothing else unless ``large_var_full`` is on; with ``pade_order="exp"`` a ``ValueError``.
# large_var_full     beside ``large_generator=True`` on a variational constructor (Pade constraint): the robust-control objective family -- goals,
#                    weights, regularisers, value, gradient, the objective's Hessian -- and the rollout of the stacked state at dimensions
#                    66 .. 128 (option ``large_var_full``): ``Objective.bind``, ``rollout``, ``rollout_dev``, ``variational_rollout`` work.  The
#                    compact Jacobian stays refused there.  At a dimension up to 64 it sets nothing (``var_full``, which
#                    ``enable_objective_and_rollout`` switches on, is that context's option).
# large_var_exp      beside ``large_generator=True`` with ``pade_order="exp"`` on a variational constructor: the fourth flag ``PCL_LARGE_VAR_EXP``, the
#                    exact exponential constraint on the lifted generator at dimensions 66 .. 128 (``large_variational_exp`` on the context):
#                    residual and exact Jacobian with the value order of ``pade_order="exp"`` at dimensions up to 62.  ``large_var_full`` is
#                    allowed beside it (objective and rollout: the kernels of the Pade kind, the same bits); ``exp_hessian``, ``var_compact`` and
#                    ``large_var_hessian`` are not (this kind's Hessian keyword is ``large_var_exp_hessian``, next).  At a dimension up to 64 the
#                    ordinary variational exponential context serves.
# large_var_exp_hessian  beside ``large_var_exp=True``: the Hessian of the Lagrangian of that constraint at dimensions 66 .. 128 (option
#                    ``large_var_exp_hess``: the adjoint of the Jacobian's substepped recurrence on the lifted generator, one pass per component;
#                    values, order and structure are ``exp_hessian``'s on a variational context at dimensions up to 62): ``hess``, ``hess_dev``,
#                    ``hess_structure``, ``hessian_structure``, ``eval_hessian_of_lagrangian`` work.  At a dimension up to 64 it sets nothing
#                    (``exp_hessian`` is that context's switch).
# large_var_hessian  beside ``large_generator=True`` on a variational constructor (Pade constraint): the Hessian of the Lagrangian at dimensions
#                    66 .. 128 (option ``large_var_hess``; values, order and structure are the variational context's at dimensions up to 64):
#                    ``hess``, ``hess_dev``, ``hess_structure``, ``hessian_structure``, ``eval_hessian_of_lagrangian`` work.  At a dimension up to
#                    64 it sets nothing (the ordinary variational context serves its Hessian always).
# large_hessian      beside ``large_generator=True`` on the plain Pade constraint: the Hessian of the Lagrangian there (option ``large_hess``).
# large_full         the same conditions, or beside ``large_exp=True``: the objective family -- goals, weights, regularisers, value, gradient, the
#                    objective's Hessian -- and the rollout there (option ``large_full``): ``rollout``, ``rollout_dev``, ``Objective.bind`` work.
# large_reduce       the same conditions as ``large_hessian``: the compact Jacobian (``ctx.compact_nnz`` / ``compact_per``, ``eval_jac_compact_dev``,
#                    ``jac_expand_dev``), the host-pointer calls' compact route and the merit / reduce payload (``merit_grad_dev``,
#                    ``eval_jac_merit_dev`` -- with ``vals=None`` the payload alone -- and, with ``large_full``, ``eval_jac_merit_objective_dev``)
#                    there (option ``large_reduce``).  The three are independent of each other.
# large_exp          beside ``large_generator=True`` with ``pade_order="exp"`` on a plain context: the second flag ``PCL_LARGE_EXP``, the exponential
#                    constraint at dimensions 66 .. 128, residual and exact Jacobian (a substepped Taylor polynomial, ``ceil(|dt| |G|_1)`` substeps:
#                    the cost is linear in the step).  ``large_full`` is allowed beside it; ``large_hessian`` and ``large_reduce`` are not, and the
#                    library refuses ``exp_hessian`` and ``exp_full`` there.  At a dimension up to 64 the ordinary exponential context serves.
# large_exp_hessian  beside ``large_exp=True``: the Hessian of the Lagrangian of that constraint there (option ``large_exp_hess``: the adjoint of the
#                    Jacobian's substepped recurrence with the second derivative carried; values, order and structure are ``exp_hessian``'s).  At
#                    a dimension up to 64 it sets nothing (``exp_hessian`` is that context's switch).
# large_exp_reduce   beside ``large_exp=True``: the compact Jacobian (layout ``[-E | tails]`` per interval), the host-pointer calls' compact route
#                    and the merit / reduce payload there (option ``large_exp_reduce``).  At a dimension up to 64 it sets nothing (``exp_full``).
#
# All are off by default and none is ever switched on by itself.  One row of _SERVICES per rule: `when` -- the values of the keyword the row speaks
# about ("on": any true one); what it sets -- a `flag` of pcl_desc.batch_mode or a library `option`; the keyword it stands `beside`; the `constraint`
# it needs; the `family` of contexts it belongs to; the `sizes` on the context that follow its option (hess_nnz / hess_per, compact_nnz /
# compact_per); `at`, the kind of context (an attribute of _PclContext) on which the constructor sets the option and set_option stores it, unless
# the context is of the kind `yields`, which has a switch of its own; `refuse`, question -> sentence, in the order the questions are asked.
# ROW ORDER IS PRECEDENCE: _check_services raises the first sentence that applies (tests/golden/keyword_trace.json has every combination).
# ---------------------------------------------------------------------------
_Service = collections.namedtuple("_Service", "keyword refuse when flag option beside constraint family sizes at yields without", defaults=("on",) + (None,) * 9)
_SERVICES = (
    _Service("large_generator", {}, flag="PCL_LARGE_N"),
    # (`without`: the keywords that must be off beside this one)
    _Service("large_var_exp", flag="PCL_LARGE_VAR_EXP", beside="large_generator", constraint="exp", family="variational",
             without=("exp_hessian", "var_compact", "large_var_hessian"), refuse={
        "family": "large_var_exp=True is the flag PCL_LARGE_VAR_EXP of a variational context (VariationalUnitaryIntegrator / "
                  "VariationalKetIntegrator with large_generator=True, pade_order=\"exp\"): a plain context takes large_exp=True",
        "beside": "large_var_exp=True is the exponential constraint of a variational context created with large_generator=True "
                  "(the flags PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP): it needs that keyword",
        "constraint": "large_var_exp=True is the variational exponential constraint at generator dimensions 66 .. 128: it needs pade_order=\"exp\" (got %(order)r)",
        "without": "large_var_exp=True serves residual and Jacobian, and with large_var_full=True the objective and the rollout: the Hessian of the "
                   "Lagrangian and the compact Jacobian are not implemented for a large variational exponential context (PCL_LARGE_VAR_EXP), "
                   "so exp_hessian, var_compact and large_var_hessian stay off"}),
    _Service("large_var_exp_hessian", option="large_var_exp_hess", beside="large_var_exp", family="variational", sizes="hess", at="large_variational_exp", refuse={
        "family": "large_var_exp_hessian=True is the Hessian of the Lagrangian of a large variational exponential context (VariationalUnitaryIntegrator / "
                  "VariationalKetIntegrator with large_generator=True, large_var_exp=True, pade_order=\"exp\"): a plain context takes large_exp_hessian=True",
        "beside": "large_var_exp_hessian=True is the Hessian of the Lagrangian of a variational context created with large_var_exp=True "
                  "(large_generator=True, pade_order=\"exp\"): it needs that keyword"}),
    _Service("large_variational", flag="PCL_LARGE_VAR", beside="large_generator", constraint="pade context, or exp beside large_var_exp", family="variational", refuse={
        "constraint": "large_generator=True on a variational integrator serves the diagonal Pade orders 2 .. 10: pade_order=\"exp\" "
                      "(PCL_BATCH_VARIATIONAL_EXP) has no large variational contexts",
        "family": "large_variational=True is the flag PCL_LARGE_VAR of a variational context (VariationalUnitaryIntegrator / "
                  "VariationalKetIntegrator with large_generator=True): a plain context takes large_generator=True alone",
        "beside": "large_variational=True goes with large_generator=True (the flags PCL_LARGE_N | PCL_LARGE_VAR): it needs that keyword"}),
    _Service("large_var_full", option="large_var_full", beside="large_generator", constraint="pade context, or exp beside large_var_exp", family="variational", at="large_variational", refuse={
        "family": "large_var_full=True is the objective and the rollout of a large variational context (VariationalUnitaryIntegrator / "
                  "VariationalKetIntegrator with large_generator=True): a plain context takes large_full=True",
        "beside": "large_var_full=True is the objective and the rollout of a variational context created with large_generator=True: it needs that keyword",
        "constraint": "large_var_full=True serves the diagonal Pade orders 2 .. 10: pade_order=\"exp\" (PCL_BATCH_VARIATIONAL_EXP) has no large variational contexts"}),
    _Service("large_var_hessian", option="large_var_hess", beside="large_generator", constraint="pade context", family="variational", sizes="hess", at="large_variational", refuse={
        "family": "large_var_hessian=True is the Hessian of the Lagrangian of a large variational context (VariationalUnitaryIntegrator / "
                  "VariationalKetIntegrator with large_generator=True): a plain context takes large_hessian=True",
        "beside": "large_var_hessian=True is the Hessian of the Lagrangian of a variational context created with large_generator=True: it needs that keyword",
        "constraint": "large_var_hessian=True serves the diagonal Pade orders 2 .. 10: pade_order=\"exp\" (PCL_BATCH_VARIATIONAL_EXP) has no large variational contexts"}),
    _Service("large_exp_hessian", option="large_exp_hess", beside="large_exp", family="plain", sizes="hess", at="large_exp", refuse={
        "family": "large_exp_hessian=True is not served on a variational context (the flags PCL_LARGE_N and PCL_LARGE_EXP go with a plain context)",
        "beside": "large_exp_hessian=True is the Hessian of the Lagrangian of a context created with large_exp=True "
                  "(large_generator=True, pade_order=\"exp\"): it needs that keyword"}),
    _Service("large_exp_reduce", option="large_exp_reduce", beside="large_exp", family="plain", sizes="compact", at="large_exp", refuse={
        "family": "large_exp_reduce=True is not served on a variational context (the flags PCL_LARGE_N and PCL_LARGE_EXP go with a plain context; var_compact is its option)",
        "beside": "large_exp_reduce=True is the compact Jacobian and the reduce payload of a context created with large_exp=True "
                  "(large_generator=True, pade_order=\"exp\"): it needs that keyword"}),
    _Service("large_exp", flag="PCL_LARGE_EXP", beside="large_generator", constraint="exp", family="plain", refuse={
        "family": "large_exp=True is not served on a variational context (the flags PCL_LARGE_N and PCL_LARGE_EXP go with a plain context)",
        "beside": "large_exp=True is the exponential constraint of a context created with large_generator=True: it needs that keyword",
        "constraint": "large_exp=True is the exponential constraint at generator dimensions 66 .. 128: it needs pade_order=\"exp\" (got %(order)r)"}),
    _Service("large_hessian", option="large_hess", beside="large_generator", constraint="pade", family="plain", sizes="hess", at="large", refuse={
        "family": "large_hessian=True is not served on a variational context (the flag PCL_LARGE_N goes with the plain Pade constraint)",
        "beside": "large_hessian=True is the Hessian of the Lagrangian of a context created with large_generator=True: it needs that keyword",
        "constraint": "large_hessian=True serves the diagonal Pade orders 2 .. 10: pade_order=\"exp\" has no large contexts"}),
    _Service("large_full", option="large_full", beside="large_generator", constraint="pade, or exp beside large_exp", family="plain", at="large", refuse={
        "family": "large_full=True is not served on a variational context (the flag PCL_LARGE_N goes with the plain Pade constraint; var_full is its option)",
        "beside": "large_full=True is the objective and the rollout of a context created with large_generator=True: it needs that keyword",
        "constraint": "large_full=True serves the diagonal Pade orders 2 .. 10: pade_order=\"exp\" has no large contexts"}),
    _Service("large_reduce", option="large_reduce", beside="large_generator", constraint="pade", family="plain", sizes="compact", at="large", yields="large_exp", refuse={
        "family": "large_reduce=True is not served on a variational context (the flag PCL_LARGE_N goes with the plain Pade constraint; var_compact is its option)",
        "beside": "large_reduce=True is the compact Jacobian and the reduce payload of a context created with large_generator=True: it needs that keyword",
        "constraint": "large_reduce=True serves the diagonal Pade orders 2 .. 10: pade_order=\"exp\" has no large contexts"}),
    _Service("exp_hessian", when="any", refuse={"value": "exp_hessian must be False, True or \"workspace\" (got %(value)r)"}),
    _Service("exp_full", option="exp_full", constraint="exp", family="plain", sizes="compact", at="exponential", yields="large_exp", refuse={
        "constraint": "exp_full=True serves the compact Jacobian and the merit / reduce payload of the exponential constraint: it needs pade_order=\"exp\" (got %(order)r)",
        "family": "exp_full=True is not served on a variational context"}),
    _Service("var_compact", option="var_compact", family="variational", sizes="compact", at="variational", refuse={
        "family": "var_compact=True serves the compact Jacobian of a variational context (VariationalUnitaryIntegrator / "
                  "VariationalKetIntegrator): a plain context has its compact Jacobian without it"}),
    # (HipPadeIntegrator's own answer to "workspace", at any order: _PclContext answers it by the two rows below)
    _Service("exp_hessian", when="workspace", family="no plain integrator", refuse={
        "family": "exp_hessian=\"workspace\" is the tile plan of the variational exponential constraint: a plain integrator takes False or True"}),
    # (the option is exp_hess on a plain context, var_exp_hess on a variational one: _PclContext._key)
    _Service("exp_hessian", option="exp_hess", constraint="exp", sizes="hess", at="exponential", refuse={
        "constraint": "exp_hessian=True is the Hessian of the Lagrangian of the exponential constraint: it needs pade_order=\"exp\" (got %(order)r)"}),
    _Service("exp_hessian", when="workspace", option="var_exp_hess_tiles", family="variational exp", at="variational", refuse={
        "family": "exp_hessian=\"workspace\" is the tile plan of the variational exponential constraint (option var_exp_hess_tiles): "
                  "it needs a variational context with pade_order=\"exp\""}),
)
_BY_OPTION = {row.option: row for row in _SERVICES if row.option}
# the order in which a constructor switches the options on (the tile plan before the Hessian that reads it)
_OPTION_ORDER = ("var_exp_hess_tiles", "exp_hess", "large_hess", "large_exp_hess", "exp_full", "large_full", "large_reduce", "large_exp_reduce", "large_var_full", "large_var_hess", "large_var_exp_hess", "var_compact")
_VARIATIONAL_MODES = (PCL_BATCH_VARIATIONAL, PCL_BATCH_VARIATIONAL_EXP)


def _check_services(batch_mode=PCL_BATCH_MEMBERS, pade_order=4, *, plain_integrator=False, **keywords):
    """Every service keyword against _SERVICES, before any device call: the first sentence that applies is a ``ValueError``.  ``keywords``: the
    ones switched on (a missing one is off); ``plain_integrator``: the caller is HipPadeIntegrator.  Returns ``exp_hessian`` as ``False`` |
    ``True`` | ``"workspace"``."""
    variational = batch_mode in _VARIATIONAL_MODES
    for row in _SERVICES:
        value = keywords.get(row.keyword, False)
        if (row.when == "on" and not value) or (row.when == "workspace" and not (isinstance(value, str) and value == "workspace")):
            continue
        for question, sentence in row.refuse.items():
            if question == "value":
                refused = not (isinstance(value, (bool, np.bool_)) or (isinstance(value, (int, np.integer)) and value in (0, 1))
                               or (isinstance(value, str) and value == "workspace"))  # fmt: skip
            elif question == "family":
                refused = {"plain": variational, "variational": not variational, "variational exp": batch_mode != PCL_BATCH_VARIATIONAL_EXP,
                           "no plain integrator": plain_integrator}[row.family]  # fmt: skip
            elif question == "beside":
                refused = not keywords.get(row.beside, False)
            elif question == "without":
                refused = any(keywords.get(other, False) for other in row.without)
            else:
                exp = _lib.order_code(pade_order) == _lib.PCL_ORDER_EXP
                pade_context = exp or batch_mode == PCL_BATCH_VARIATIONAL_EXP
                refused = {"exp": not exp, "pade": exp, "pade, or exp beside large_exp": exp and not keywords.get("large_exp", False),
                           "pade context": pade_context,
                           "pade context, or exp beside large_var_exp": pade_context and not keywords.get("large_var_exp", False)}[row.constraint]  # fmt: skip
            if refused:
                raise ValueError(sentence % dict(order=pade_order, value=value))
    value = keywords.get("exp_hessian", False)
    return value if isinstance(value, str) else bool(value)


class _PclContext:
    """Owns one ``pcl_ctx`` (one GPU, one stream)."""

    def __init__(self, *, d, m, N, z_dim, u_off, dt_off, x_offs, G0, Gj, batch, batch_mode, per_member_G0=False,
                 global_dim=0, device=0, index_base=0, pade_order=4, state_cols=0, exp_hessian=False, exp_full=False, var_compact=False,
                 large_generator=False, large_hessian=False, large_full=False, large_reduce=False, large_exp=False, large_exp_hessian=False,
                 large_exp_reduce=False, large_variational=False, large_var_full=False, large_var_hessian=False, large_var_exp=False, large_var_exp_hessian=False):  # fmt: skip
        keywords = dict(exp_hessian=exp_hessian, exp_full=exp_full, var_compact=var_compact, large_generator=large_generator, large_hessian=large_hessian,
                        large_full=large_full, large_reduce=large_reduce, large_exp=large_exp, large_exp_hessian=large_exp_hessian,
                        large_exp_reduce=large_exp_reduce, large_variational=large_variational, large_var_full=large_var_full,
                        large_var_hessian=large_var_hessian, large_var_exp=large_var_exp, large_var_exp_hessian=large_var_exp_hessian)  # fmt: skip
        keywords["exp_hessian"] = _check_services(batch_mode, pade_order, **keywords)
        pade_order = _lib.order_code(pade_order)  # ("exp": the exponential constraint, PCL_ORDER_EXP)
        self._L = _lib.load()
        self._h = None
        n = d if state_cols == _lib.PCL_STATE_VECTOR else 2 * d  # PCL_STATE_VECTOR: general d x d generator, one column
        g0 = _colmajor(G0)
        gj = _colmajor(Gj) if m else np.zeros(1)
        if g0.size != n * n * (batch if per_member_G0 else 1):
            raise ValueError("G0 has %d entries, expected %d" % (g0.size, n * n * (batch if per_member_G0 else 1)))
        if m and gj.size != m * n * n:
            raise ValueError("Gj has %d entries, expected %d" % (gj.size, m * n * n))
        xo = np.ascontiguousarray(np.asarray(x_offs, dtype=np.int32).reshape(-1))
        desc = _lib.pcl_desc(
            struct_size=ctypes.sizeof(_lib.pcl_desc), d=d, n_drives=m, N=N, z_dim=z_dim, u_off=u_off, dt_off=dt_off,
            batch=batch, batch_mode=batch_mode | (_lib.PCL_LARGE_N if large_generator else 0) | (_lib.PCL_LARGE_EXP if large_exp else 0) | (_lib.PCL_LARGE_VAR if large_variational else 0) | (PCL_LARGE_VAR_EXP if large_var_exp else 0), pade_order=pade_order, device_id=device,
            index_base=index_base, per_member_G0=int(bool(per_member_G0)), state_cols=state_cols, global_dim=global_dim,
            G0=g0.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            Gj=gj.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            x_offs=xo.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
        )  # fmt: skip
        h = ctypes.c_void_p()
        rc = self._L.pcl_create(ctypes.byref(desc), ctypes.byref(h))
        if rc != 0:
            raise PclError(rc, (self._L.pcl_last_error(None) or b"").decode())
        self._h = h
        self.d, self.n, self.m, self.N, self.K, self.z_dim = d, n, m, N, N - 1, z_dim
        self.batch, self.batch_mode = batch, batch_mode
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._chk(self._L.pcl_constraint_dim(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        self.x_dim, self.n_rows, self.n_cols = a.value, b.value, c.value
        self._chk(self._L.pcl_jac_nnz(h, ctypes.byref(a), ctypes.byref(b)))
        self.jac_nnz, self.jac_per = a.value, b.value
        # the kind of context (what each kind serves, and by which keyword: the table above).  The three flags change nothing at a generator
        # dimension up to 64: the context is then an ordinary one of its constraint
        self.exponential = pade_order == _lib.PCL_ORDER_EXP
        self.large = bool(large_generator) and n > 64
        self.large_exp = bool(large_exp) and self.large
        self.large_variational = bool(large_variational) and self.large
        self.large_variational_exp = bool(large_var_exp) and self.large_variational
        # a variational context: x_dim is the stacked state; goals and forms speak of component 0, the rollout returns one stacked trajectory
        self.variational = batch_mode in _VARIATIONAL_MODES
        # one attribute per option keyword, named like it: it follows the library's option (set_option), and so do the sizes the option governs
        # (_refresh_sizes).  _switches: option key -> attribute, of the rows that apply to this kind of context
        self._switches, self._governs = {}, {"hess": [], "compact": []}
        for row in _BY_OPTION.values():
            if row.when == "on":
                setattr(self, row.keyword, False)
                if getattr(self, row.at) and not (row.yields and getattr(self, row.yields)):
                    self._switches[self._key(row)] = row.keyword
                    if row.sizes:
                        self._governs[row.sizes].append(row.keyword)
        for option in _OPTION_ORDER:  # (a large option only on a large context: at n <= 64 the ordinary context serves as always, nothing is set)
            row = _BY_OPTION[option]
            value = keywords[row.keyword]
            if (value == "workspace" if row.when == "workspace" else value) and getattr(self, row.at):
                self.set_option(self._key(row), 1)
        self._refresh_sizes()
        self.z_len = z_dim * N * (batch if batch_mode == PCL_BATCH_TRAJ else 1)
        self.window = (0, batch)
        self.goal_dim = self.x_dim // batch if self.variational else self.x_dim

    def _key(self, row):
        return "var_exp_hess" if row.option == "exp_hess" and self.batch_mode == PCL_BATCH_VARIATIONAL_EXP else row.option

    def _refresh_sizes(self):
        """hess_nnz / hess_per and compact_nnz / compact_per of the member window: current when no option of _SERVICES governs them on this kind
        of context (a plain Pade context at n <= 64; the Hessian of a variational Pade one) or one that does is on; else 0."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        for sizes, count in (("hess", self._L.pcl_hess_nnz), ("compact", self._L.pcl_jac_compact_nnz)):
            a.value = b.value = 0
            if not self._governs[sizes] or any(getattr(self, keyword) for keyword in self._governs[sizes]):
                self._chk(count(self._h, ctypes.byref(a), ctypes.byref(b)))
            setattr(self, sizes + "_nnz", a.value)
            setattr(self, sizes + "_per", b.value)

    def _chk(self, rc):
        if rc != 0:
            raise PclError(rc, (self._L.pcl_last_error(self._h) or b"").decode())

    def set_order_policy(self, dt_max, u_max, tol=1e-10):
        """The smallest diagonal Pade order whose deviation from the reference's exp constraint, ``kappa_q theta^(2q+1)`` with
        ``theta = dt_max max_{|u_l| <= u_max_l} |G_drift + sum_l u_l G_l|_2`` (the maximum over the box of controls), is below ``tol``; becomes the context's order.  Returns it."""
        um = np.ascontiguousarray(np.broadcast_to(np.abs(np.asarray(u_max, dtype=np.float64)), (max(self.m, 1),)))
        out = ctypes.c_int32()
        self._L.pcl_set_order_policy.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int32)]
        self._chk(self._L.pcl_set_order_policy(self._h, float(dt_max), um.ctypes.data, float(tol), ctypes.byref(out)))
        return out.value

    def set_order_from_trajectory(self, Z, tol=1e-10):
        """The same decision from a trajectory on the host (``theta = 1.5 max_k |dt_k G(u_k)|``): what a constructor calls when the
        trajectory carries no bounds on the drives and the timestep.  Returns the order."""
        Z = self._z(Z)
        out = ctypes.c_int32()
        self._L.pcl_set_order_from_trajectory.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int32)]
        self._chk(self._L.pcl_set_order_from_trajectory(self._h, _ptr(Z), float(tol), ctypes.byref(out)))
        return out.value

    @property
    def order_tol_met(self):
        """False when the order policy had to settle for order 10 with its bound above the tolerance."""
        return bool(self.get_option("order_tol_met"))

    @property
    def pade_order(self):
        """The order in use (0: a context created with ``pade_order=0`` that has not seen a policy or a trajectory yet; -1: the exponential constraint)."""
        return self.get_option("pade_order")

    def close(self):
        if getattr(self, "_h", None):
            self._L.pcl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- structure ----------------------------------------------------------------------------
    def jac_structure(self, dtype=np.int64):
        rows, cols = np.empty(self.jac_nnz, dtype), np.empty(self.jac_nnz, dtype)
        if dtype == np.int32:
            p = ctypes.POINTER(ctypes.c_int32)
            self._chk(self._L.pcl_jac_structure(self._h, rows.ctypes.data_as(p), cols.ctypes.data_as(p)))
        else:
            p = ctypes.POINTER(ctypes.c_int64)
            self._chk(self._L.pcl_jac_structure_i64(self._h, rows.ctypes.data_as(p), cols.ctypes.data_as(p)))
        return rows, cols

    def hess_structure(self, dtype=np.int64):
        rows, cols = np.empty(self.hess_nnz, dtype), np.empty(self.hess_nnz, dtype)
        if dtype == np.int32:
            p = ctypes.POINTER(ctypes.c_int32)
            self._chk(self._L.pcl_hess_structure(self._h, rows.ctypes.data_as(p), cols.ctypes.data_as(p)))
        else:
            p = ctypes.POINTER(ctypes.c_int64)
            self._chk(self._L.pcl_hess_structure_i64(self._h, rows.ctypes.data_as(p), cols.ctypes.data_as(p)))
        return rows, cols

    # -- host-pointer calls ---------------------------------------------------------------------
    def _z(self, Z):
        Z = np.ascontiguousarray(Z, dtype=np.float64).reshape(-1)
        if Z.size != self.z_len:
            raise ValueError("trajectory buffer has %d entries, expected %d" % (Z.size, self.z_len))
        return Z

    def eval(self, Z, delta=None):
        Z = self._z(Z)
        delta = np.empty(self.n_rows) if delta is None else delta
        self._chk(self._L.pcl_eval(self._h, _ptr(Z), _ptr(delta)))
        return delta

    def eval_jac(self, Z, delta=None, vals=None):
        Z = self._z(Z)
        delta = np.empty(self.n_rows) if delta is None else delta
        vals = np.empty(self.jac_nnz) if vals is None else vals
        self._chk(self._L.pcl_eval_jac(self._h, _ptr(Z), _ptr(delta), _ptr(vals)))
        return delta, vals

    def jac(self, Z, vals=None):
        Z = self._z(Z)
        vals = np.empty(self.jac_nnz) if vals is None else vals
        self._chk(self._L.pcl_jac(self._h, _ptr(Z), _ptr(vals)))
        return vals

    def hess(self, Z, mu, vals=None):
        Z = self._z(Z)
        mu = np.ascontiguousarray(mu, dtype=np.float64).reshape(-1)
        if mu.size != self.n_rows:
            raise ValueError("mu has %d entries, expected %d" % (mu.size, self.n_rows))
        vals = np.empty(self.hess_nnz) if vals is None else vals
        self._chk(self._L.pcl_hess(self._h, _ptr(Z), _ptr(mu), _ptr(vals)))
        return vals

    # -- device-pointer calls (torch tensors on this context's GPU; asynchronous) ----------------
    def set_stream(self, stream_handle):
        """Launch on this hipStream_t handle (0 = the legacy default stream); ``None`` restores
        the context's own stream."""
        if stream_handle is None:
            self._chk(self._L.pcl_reset_stream(self._h))
        else:
            self._chk(self._L.pcl_set_stream(self._h, ctypes.c_void_p(int(stream_handle))))

    def sync(self):
        self._chk(self._L.pcl_sync(self._h))

    def eval_dev(self, Z, delta):
        self._chk(self._L.pcl_eval_dev(self._h, _ptr(Z), _ptr(delta)))

    def eval_jac_dev(self, Z, delta, vals):
        self._chk(self._L.pcl_eval_jac_dev(self._h, _ptr(Z), _ptr(delta), _ptr(vals)))

    def eval_jac_compact_dev(self, Z, delta, compact):
        self._chk(self._L.pcl_eval_jac_compact_dev(self._h, _ptr(Z), _ptr(delta), _ptr(compact)))

    def jac_expand_dev(self, compact, vals):
        self._chk(self._L.pcl_jac_expand_dev(self._h, _ptr(compact), _ptr(vals)))

    def hess_dev(self, Z, mu, vals):
        self._chk(self._L.pcl_hess_dev(self._h, _ptr(Z), _ptr(mu), _ptr(vals)))

    def jac_dev(self, Z, vals):
        self._chk(self._L.pcl_jac_dev(self._h, _ptr(Z), _ptr(vals)))

    # -- member window: the evaluator calls cover members [first, first+count) (one member of the reference's integrator vector)
    def set_member_window(self, first=0, count=None):
        count = self.batch - first if count is None else count
        self._chk(self._L.pcl_set_member_window(self._h, int(first), int(count)))
        self.window = (int(first), int(count))
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._chk(self._L.pcl_constraint_dim(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        self.n_rows = b.value
        self._chk(self._L.pcl_jac_nnz(self._h, ctypes.byref(a), ctypes.byref(b)))
        self.jac_nnz = a.value
        self._refresh_sizes()

    # -- DerivativeIntegrator / time-consistency rows on this context's trajectory layout -----------------
    def deriv_dims(self, dx_off, dim):
        a, b = ctypes.c_int64(), ctypes.c_int64()
        self._chk(self._L.pcl_deriv_nnz(self._h, dx_off, dim, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def deriv_structure(self, x_off, dx_off, dim):
        _, nnz = self.deriv_dims(dx_off, dim)
        rows, cols = np.empty(nnz, np.int64), np.empty(nnz, np.int64)
        p = ctypes.POINTER(ctypes.c_int64)
        self._chk(self._L.pcl_deriv_structure(self._h, x_off, dx_off, dim, rows.ctypes.data_as(p), cols.ctypes.data_as(p)))
        return rows, cols

    def deriv_eval_jac(self, x_off, dx_off, dim, Z):
        Z = self._z(Z)
        nr, nnz = self.deriv_dims(dx_off, dim)
        delta, vals = np.empty(nr), np.empty(nnz)
        self._chk(self._L.pcl_deriv_eval_jac(self._h, x_off, dx_off, dim, _ptr(Z), _ptr(delta), _ptr(vals)))
        return delta, vals

    def deriv_eval_jac_dev(self, x_off, dx_off, dim, Z, delta, vals):
        self._chk(self._L.pcl_deriv_eval_jac_dev(self._h, x_off, dx_off, dim, _ptr(Z), _ptr(delta), _ptr(vals)))

    # -- terminal infidelity objective on device ----------------------------------------------------------------
    def set_goal(self, goal_iso_vec):
        g = np.ascontiguousarray(goal_iso_vec, dtype=np.float64).reshape(-1)
        if g.size != self.goal_dim:
            raise ValueError("goal iso-vec has %d entries, expected %d" % (g.size, self.goal_dim))
        self._chk(self._L.pcl_set_goal(self._h, _ptr(g)))

    def set_goal_subspace(self, goal_sub_iso_vec, subspace):
        """Embedded goal: iso-vec of the ns x ns block ``unembed(op)`` and its 0-based subspace indices."""
        sub = np.ascontiguousarray(subspace, dtype=np.int32).reshape(-1)
        g = np.ascontiguousarray(goal_sub_iso_vec, dtype=np.float64).reshape(-1)
        if g.size != 2 * sub.size * sub.size:
            raise ValueError("subspace goal iso-vec has %d entries, expected %d" % (g.size, 2 * sub.size * sub.size))
        self._chk(self._L.pcl_set_goal_subspace(self._h, _ptr(g), sub.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), sub.size))

    def set_goal_form(self, scope, A, c):
        """Terminal loss ``Q w |1 - F(x)|``, ``F = c'x + sum_r (A_r'x)^2`` (``pcl_set_goal_form``): scope 0 per member, 1 joint."""
        L = self.goal_dim * (self.batch if scope and not self.variational else 1)
        A = None if A is None else np.ascontiguousarray(A, dtype=np.float64).reshape(-1, L)
        c = None if c is None else np.ascontiguousarray(c, dtype=np.float64).reshape(L)
        self._L.pcl_set_goal_form.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self._L.pcl_set_goal_form(self._h, int(scope), 0 if A is None else A.shape[0], None if A is None else A.ctypes.data, None if c is None else c.ctypes.data))

    def objective_hess_structure(self):
        n = ctypes.c_int64()
        self._chk(self._L.pcl_objective_hess_nnz(self._h, ctypes.byref(n)))
        rows, cols = np.empty(n.value, dtype=np.int64), np.empty(n.value, dtype=np.int64)
        self._L.pcl_objective_hess_structure.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self._L.pcl_objective_hess_structure(self._h, rows.ctypes.data, cols.ctypes.data))
        return rows, cols

    def objective_hess(self, Z, Q, sigma=1.0):
        Z = self._z(Z)
        n = ctypes.c_int64()
        self._chk(self._L.pcl_objective_hess_nnz(self._h, ctypes.byref(n)))
        vals = np.empty(n.value)
        self._L.pcl_objective_hess.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
        self._chk(self._L.pcl_objective_hess(self._h, Z.ctypes.data, float(Q), float(sigma), vals.ctypes.data))
        return vals

    def objective_hess_dev(self, Z, Q, sigma, vals):
        self._L.pcl_objective_hess_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
        self._chk(self._L.pcl_objective_hess_dev(self._h, _ptr(Z), float(Q), float(sigma), _ptr(vals)))

    def set_weights(self, weights):
        if weights is None:
            self._chk(self._L.pcl_set_weights(self._h, None))
            return
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.size != self.batch:
            raise ValueError("expected %d weights, got %d" % (self.batch, w.size))
        self._chk(self._L.pcl_set_weights(self._h, _ptr(w)))

    def infidelity_dev(self, Z, Q, value=None, grad=None):
        self._chk(self._L.pcl_infidelity_dev(self._h, _ptr(Z), float(Q), _ptr(value), _ptr(grad)))

    def add_regularizer(self, off, dim, R, dt_power=2):
        R = np.ascontiguousarray(np.broadcast_to(np.asarray(R, dtype=np.float64), (dim,)))
        self._chk(self._L.pcl_add_regularizer(self._h, int(off), int(dim), _ptr(R), int(dt_power)))

    def clear_regularizers(self):
        self._chk(self._L.pcl_clear_regularizers(self._h))

    def objective_dev(self, Z, Q, value, grad=None):
        self._chk(self._L.pcl_objective_dev(self._h, _ptr(Z), float(Q), _ptr(value), _ptr(grad)))

    def objective(self, Z, Q, want_grad=True):
        """(value [1 or batch], gradient [z_len] or None) of the whole objective, host buffers."""
        Z = self._z(Z)
        value = np.empty(self.batch if self.batch_mode == PCL_BATCH_TRAJ else 1)
        grad = np.empty(self.z_len) if want_grad else None
        self._chk(self._L.pcl_objective(self._h, _ptr(Z), float(Q), _ptr(value), _ptr(grad)))
        return value, grad

    def merit_grad_len(self):
        a, b = ctypes.c_int64(), ctypes.c_int64()
        self._chk(self._L.pcl_merit_grad_len(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def merit_grad_dev(self, delta, lam, vals, out):
        """out <- [phi | J^T lam on the shared u_k | ... on dt_k] (lam None: lam = delta, phi = the constraint merit)."""
        self._chk(self._L.pcl_merit_grad_dev(self._h, _ptr(delta), _ptr(lam), _ptr(vals), _ptr(out)))

    def eval_jac_merit_dev(self, Z, lam, delta, vals, out):
        """``eval_jac_dev`` + ``merit_grad_dev`` in one pass over the state columns (pcl_eval_jac_merit_dev): the fused kernel
        forms the payload's dot products while a column's vectors are in LDS; same outputs as the two calls.  ``vals=None`` (an exponential
        context with ``exp_full``: the residual and the payload without the Jacobian, one adjoint chain per interval; a large context with
        ``large_reduce``: chain units only, no Jacobian value formed or written)."""
        self._chk(self._L.pcl_eval_jac_merit_dev(self._h, _ptr(Z), _ptr(lam), _ptr(delta), _ptr(vals), _ptr(out)))

    def eval_jac_merit_objective_dev(self, Z, lam, delta, vals, out, Q, value, grad):
        """``objective_dev`` + ``eval_jac_merit_dev`` -- a rank's whole step of a sharded ensemble -- in two launches instead of four
        (pcl_eval_jac_merit_objective_dev); the same bits."""
        self._chk(self._L.pcl_eval_jac_merit_objective_dev(self._h, _ptr(Z), _ptr(lam), _ptr(delta), _ptr(vals), _ptr(out), float(Q), _ptr(value), _ptr(grad)))

    # -- rollout (exact piecewise-constant propagation from the knot-0 state) ----------------------------------------
    def rollout(self, Z, out=None):
        """[batch, N, x_dim] iso-vec states: X_{k+1} = exp(dt_k G(u_k)) X_k."""
        Z = self._z(Z)
        out = np.empty((1 if self.variational else self.window[1], self.N, self.x_dim)) if out is None else out
        self._chk(self._L.pcl_rollout(self._h, _ptr(Z), _ptr(out)))
        return out

    def rollout_dev(self, Z, out):
        self._chk(self._L.pcl_rollout_dev(self._h, _ptr(Z), _ptr(out)))

    # -- RCCL (C-ABI path; torch.distributed is the alternative plumbing, see distributed.py) ----------------
    def comm_unique_id(self):
        buf = ctypes.create_string_buffer(128)
        rc = self._L.pcl_comm_get_unique_id(buf)
        if rc != 0:
            raise PclError(rc, (self._L.pcl_last_error(None) or b"").decode())
        return buf.raw

    def comm_init(self, unique_id, rank, nranks):
        self._chk(self._L.pcl_comm_init(self._h, ctypes.create_string_buffer(unique_id, 128), rank, nranks))

    def reduce_sum_dev(self, buf):
        self._chk(self._L.pcl_reduce_sum_dev(self._h, _ptr(buf), buf.numel()))

    def reduce_sum(self, buf):
        """In-place sum over the ranks of a host (numpy, float64, contiguous) buffer."""
        self._chk(self._L.pcl_reduce_sum(self._h, _ptr(buf), buf.size))
        return buf

    def set_option(self, key, value):
        self._chk(self._L.pcl_set_option(self._h, key.encode(), int(value)))
        if key in self._switches:  # an option of _SERVICES that applies to this kind of context: its attribute and the sizes follow it
            setattr(self, self._switches[key], bool(value))
            self._refresh_sizes()

    def get_option(self, key):
        v = ctypes.c_int64()
        self._chk(self._L.pcl_get_option(self._h, key.encode(), ctypes.byref(v)))
        return v.value


def _abs_bound(b, n):
    """max(|lower|, |upper|) per component of a bounds entry, in the shapes the mirror and the reference use: ``(lower_vec, upper_vec)`` (NamedTrajectory
    [REF named_trajectory_conversion.jl:331-332]), a list of ``(lo, hi)`` pairs per component (``system.drive_bounds``), one ``(lo, hi)`` pair, a symmetric
    bound per component, or a scalar."""
    if isinstance(b, tuple) and len(b) == 2 and all(np.ndim(x) <= 1 for x in b):  # (lower, upper): vectors or scalars
        lo, hi = (np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)) for x in b)
        return np.maximum(np.abs(lo), np.abs(hi))
    a = np.asarray(b, dtype=np.float64)
    if a.ndim == 0:
        return np.full(n, abs(float(a)))
    if a.shape == (n, 2):  # pairs per component
        return np.max(np.abs(a), axis=1)
    if a.shape == (2, n):
        return np.max(np.abs(a), axis=0)
    if a.shape == (n,):
        return np.abs(a)
    if a.shape == (2,):
        return np.full(n, np.max(np.abs(a)))
    raise ValueError("bounds of shape %r for a component of dimension %d" % (a.shape, n))


def _decide_order(ctx, traj, u_name, m, tol, copies=1):
    """``pade_order = 0`` at construction: the order policy over the trajectory's bounds, else over the trajectory itself."""
    ub, tb = traj.bounds.get(u_name), traj.bounds.get(traj.timestep)
    if ub is not None and tb is not None and m:
        umax = _abs_bound(ub, len(traj.components[u_name]))[:m]
        return ctx.set_order_policy(float(np.max(_abs_bound(tb, len(traj.components[traj.timestep])))), umax, tol)
    Z = np.ascontiguousarray(traj.datavec, dtype=np.float64).reshape(-1)
    return ctx.set_order_from_trajectory(np.tile(Z, copies) if copies > 1 else Z, tol)


def _resolved_order(ctx):
    """The order a secondary context (the scalar form ``f``) must be created with: the main context's, never 0."""
    order = ctx.pade_order
    if order == 0:
        raise PclError(-1, "the Pade order of this integrator is not decided yet (pade_order = 0 and no policy / trajectory seen)")
    return order


class HipPadeIntegrator:
    """Drop-in for ``DirectTrajOpt.BilinearIntegrator`` on the unitary path.

    One integrator object covers one state component (``x_name``) or, for a
    ``SamplingTrajectory``, the M member components at once (the reference builds
    a ``Vector{BilinearIntegrator}``, one per member, whose rows are concatenated
    in order -- the row order here is identical: member-major).
    """

    def __init__(self, G_drift, G_drives, traj, x_name=STATE, u_name="u", *, device=0, index_base=0, pade_order=0, order_tol=1e-10, exp_hessian=False,
                 exp_full=False, var_compact=False, large_generator=False, large_hessian=False, large_full=False, large_reduce=False, large_exp=False,
                 large_exp_hessian=False, large_exp_reduce=False):
        """``pade_order=0`` (the default): the smallest diagonal Pade order whose deviation from the reference's exp constraint
        [REF docs/src/concepts/index.md:21] stays below ``order_tol`` over the trajectory's bounds on ``u`` and the timestep
        (``traj.bounds``); without bounds, over ``traj`` itself (x 1.5).  Decided HERE, so every entry point -- host or device
        pointers, the scalar form ``f`` -- evaluates one order from the first call on.  ``pade_order=2..10`` pins the order
        (BASELINE.json's metric is quoted on 4, which deviates from the exp constraint by 1.6e-5 at config 3).  ``pade_order="exp"`` (or -1):
        the exponential constraint itself, ``x_{k+1} - exp(dt_k G(u_k)) x_k`` -- for steps too large for order 10 (``order_tol_met`` False); residual
        and Jacobian only: ``hessian_structure`` / ``eval_hessian_of_lagrangian`` raise, solve with a quasi-Newton Hessian.  Never chosen on its own.

        The service keywords ``exp_hessian`` (``False`` or ``True`` here), ``exp_full``, ``large_generator``, ``large_hessian``, ``large_full``,
        ``large_reduce``, ``large_exp``, ``large_exp_hessian`` and ``large_exp_reduce``: what each serves and what it must stand beside is said
        once, above ``_SERVICES`` in this module; a combination the table refuses is a ``ValueError`` before any device call.  ``var_compact``
        belongs to the variational constructors: ``True`` here is a ``ValueError``."""
        exp_hessian = _check_services(PCL_BATCH_MEMBERS, pade_order, plain_integrator=True, exp_hessian=exp_hessian, exp_full=exp_full, var_compact=var_compact,
                                      large_generator=large_generator, large_hessian=large_hessian, large_full=large_full, large_reduce=large_reduce,
                                      large_exp=large_exp, large_exp_hessian=large_exp_hessian, large_exp_reduce=large_exp_reduce)  # fmt: skip
        x_names = [x_name] if isinstance(x_name, str) else list(x_name)
        G_drives = np.asarray(G_drives, dtype=np.float64)
        G_drift = np.asarray(G_drift, dtype=np.float64)
        per_member = G_drift.ndim == 3
        n = G_drift.shape[-1]
        d = n // 2
        m = G_drives.shape[0] if G_drives.size else 0
        if per_member and G_drift.shape[0] != len(x_names):
            raise ValueError("one G_drift per member expected (%d != %d)" % (G_drift.shape[0], len(x_names)))
        for nm in x_names:
            if nm not in traj.components:
                raise KeyError("trajectory has no component %r" % (nm,))
        xlen = len(traj.components[x_names[0]])
        vec = n % 2 == 1  # odd generator dimension: a compact density vector (levels^2) under a compact Lindbladian
        if vec:
            if xlen != n or any(len(traj.components[nm]) != xlen for nm in x_names):
                raise ValueError("an odd generator dimension (%d) takes state components of that length; got %d" % (n, xlen))
            d, cols = n, 1
        else:
            if xlen % n or not (1 <= xlen // n <= d) or any(len(traj.components[nm]) != xlen for nm in x_names):
                raise ValueError("state components must all have dim n*C with n = %d, 1 <= C <= d (unitary: C = d = %d, ket: C = 1); got %d"
                                 % (n, d, xlen))  # fmt: skip
            cols = xlen // n
        if m and len(traj.components[u_name]) < m:
            raise ValueError("drive component %r has dim %d < n_drives = %d" % (u_name, len(traj.components[u_name]), m))
        self.x_names = x_names
        self.x_name = x_names[0] if len(x_names) == 1 else tuple(x_names)
        self.u_name = u_name
        self.G_drift, self.G_drives = G_drift, G_drives.reshape(m, n, n)
        self._sig = (traj.dim, traj.N)
        self._ctx = _PclContext(
            d=d, m=m, N=traj.N, z_dim=traj.dim, u_off=traj.components[u_name].start,
            dt_off=traj.components[traj.timestep].start, x_offs=[traj.components[nm].start for nm in x_names],
            G0=G_drift, Gj=self.G_drives, batch=len(x_names), batch_mode=PCL_BATCH_MEMBERS, per_member_G0=per_member,
            global_dim=traj.global_dim, device=device, index_base=index_base, pade_order=pade_order,
            state_cols=_lib.PCL_STATE_VECTOR if vec else cols, exp_hessian=exp_hessian, exp_full=exp_full, large_generator=large_generator,
            large_hessian=large_hessian, large_full=large_full, large_reduce=large_reduce, large_exp=large_exp, large_exp_hessian=large_exp_hessian, large_exp_reduce=large_exp_reduce,
        )  # fmt: skip
        self._large_generator = bool(large_generator)
        self._large_exp = bool(large_exp)
        if pade_order == 0:
            _decide_order(self._ctx, traj, u_name, m, order_tol)
        self._state_cols = _lib.PCL_STATE_VECTOR if vec else cols
        self.x_dim = self._ctx.x_dim * len(x_names) if len(x_names) > 1 else self._ctx.x_dim
        self.dim = self._ctx.n_rows
        self._f_ctx = None

    # ---- reference-style properties ------------------------------------------------------------
    @property
    def ctx(self):
        return self._ctx

    @property
    def pade_order(self):
        return self._ctx.pade_order

    def _check(self, traj):
        if (traj.dim, traj.N) != self._sig:
            raise ValueError("trajectory shape (dim=%d, N=%d) differs from the one this integrator was built for %r"
                             % (traj.dim, traj.N, self._sig))  # fmt: skip

    def f(self, x_next, x, u, dt):
        """Scalar (one-interval) form ``B.f(x_next, x, u, dt)`` [REF integrators.jl:525]."""
        c = self._ctx
        if len(self.x_names) != 1:
            raise NotImplementedError("f is defined for single-state integrators")
        if self._f_ctx is None:
            self._f_ctx = _PclContext(d=c.d, m=c.m, N=2, z_dim=c.x_dim + 1 + c.m, u_off=c.x_dim + 1, dt_off=c.x_dim,
                                      x_offs=[0], G0=self.G_drift, Gj=self.G_drives, batch=1, large_generator=self._large_generator, large_exp=self._large_exp,
                                      batch_mode=PCL_BATCH_MEMBERS, state_cols=self._state_cols, pade_order=_resolved_order(c))  # fmt: skip
        z = np.zeros((2, c.x_dim + 1 + c.m))
        z[0, : c.x_dim], z[0, c.x_dim], z[0, c.x_dim + 1 :] = x, dt, np.asarray(u)[: c.m]
        z[1, : c.x_dim] = x_next
        return self._f_ctx.eval(z)

    def close(self):
        self._ctx.close()
        if self._f_ctx is not None:
            self._f_ctx.close()


class HipVariationalIntegrator:
    """Drop-in for the ``BilinearIntegrator`` the reference's variational constructors build [REF src/control/integrators.jl:234-264]: the state
    ``vcat(x, x_var_1, ..., x_var_v)`` evolved by ``var_G(G(u), [Gv_i])`` per state column, ``Gv_i = G(H_var_i) / scale_i``.  One context of
    batch_mode PCL_BATCH_VARIATIONAL; rows are knot-major over the stacked state (``B.dim = B.x_dim * (N - 1)``).  Build it with
    ``VariationalUnitaryIntegrator`` or ``VariationalKetIntegrator``.

    ``pade_order="exp"`` (or -1): the reference's own constraint ``x'_{k+1} = exp(dt_k var_G(..)) x'_k`` instead of a Pade discretisation of
    it -- a context of batch_mode PCL_BATCH_VARIATIONAL_EXP, for the steps whose lifted ``theta`` no Pade order follows.  Residual, Jacobian,
    objective and rollout are served; ``hessian_structure`` / ``eval_hessian_of_lagrangian`` raise the library's message (third Frechet
    derivatives: solve with a quasi-Newton Hessian) unless ``exp_hessian`` switches them on.

    The service keywords ``exp_hessian`` (``False``, ``True`` or ``"workspace"``), ``var_compact``, ``large_generator``, ``large_var_full``, ``large_var_hessian``, ``large_var_exp`` and ``large_var_exp_hessian``: what each serves is
    said once, above ``_SERVICES`` in this module.  The other large keywords are accepted and, switched on, refused in the table's words."""

    def __init__(self, sys, traj, x_name, x_variations, u_name, Gv, *, ket, device=0, index_base=0, pade_order=0, order_tol=1e-10, exp_hessian=False,
                 var_compact=False, large_generator=False, large_hessian=False, large_full=False, large_reduce=False, large_exp=False,
                 large_exp_hessian=False, large_exp_reduce=False, large_var_full=False, large_var_hessian=False, large_var_exp=False,
                 large_var_exp_hessian=False):
        pade_order = _lib.order_code(pade_order)
        self.exponential = pade_order == _lib.PCL_ORDER_EXP
        batch_mode = PCL_BATCH_VARIATIONAL_EXP if self.exponential else PCL_BATCH_VARIATIONAL
        exp_hessian = _check_services(batch_mode, pade_order, exp_hessian=exp_hessian, var_compact=var_compact, large_generator=large_generator,
                                      large_variational=large_generator, large_hessian=large_hessian, large_full=large_full, large_reduce=large_reduce,
                                      large_exp=large_exp, large_exp_hessian=large_exp_hessian, large_exp_reduce=large_exp_reduce,
                                      large_var_full=large_var_full, large_var_hessian=large_var_hessian, large_var_exp=large_var_exp,
                                      large_var_exp_hessian=large_var_exp_hessian)  # fmt: skip
        x_variations = [x_variations] if isinstance(x_variations, str) else list(x_variations)
        names = [x_name] + x_variations
        n = 2 * sys.levels
        cols = 1 if ket else sys.levels
        if not x_variations:
            raise ValueError("at least one variation component is required")
        if len(x_variations) != len(Gv):
            raise ValueError("%d variation components for %d variational generators" % (len(x_variations), len(Gv)))
        for nm in names + [u_name]:
            if nm not in traj.components:
                raise KeyError("trajectory has no component %r" % (nm,))
        for nm in names:
            if len(traj.components[nm]) != n * cols:
                raise ValueError("component %r has dim %d; a %s of %d levels takes %d" % (nm, len(traj.components[nm]), "ket" if ket else "unitary",
                                                                                        sys.levels, n * cols))  # fmt: skip
        m = sys.n_drives
        if m and len(traj.components[u_name]) < m:
            raise ValueError("drive component %r has dim %d < n_drives = %d" % (u_name, len(traj.components[u_name]), m))
        self.x_names = names
        self.x_name = tuple(names)
        self.u_name = u_name
        self.G_drift = np.asarray(sys.G_drift, dtype=np.float64)
        self.G_drives = np.asarray(sys.G_drives_array(), dtype=np.float64).reshape(m, n, n)
        self.G_vars = np.asarray(Gv, dtype=np.float64).reshape(len(Gv), n, n)
        self._sig = (traj.dim, traj.N)
        self._ctx = _PclContext(
            d=sys.levels, m=m, N=traj.N, z_dim=traj.dim, u_off=traj.components[u_name].start, dt_off=traj.components[traj.timestep].start,
            x_offs=[traj.components[nm].start for nm in names], G0=np.concatenate([self.G_drift[None], self.G_vars]), Gj=self.G_drives,
            batch=len(names), batch_mode=batch_mode, per_member_G0=True, global_dim=traj.global_dim, device=device,
            index_base=index_base, pade_order=pade_order, state_cols=cols, exp_hessian=exp_hessian, var_compact=var_compact,
            large_generator=bool(large_generator), large_variational=bool(large_generator), large_var_full=bool(large_var_full),
            large_var_hessian=bool(large_var_hessian), large_var_exp=bool(large_var_exp), large_var_exp_hessian=bool(large_var_exp_hessian),
        )  # fmt: skip
        if pade_order == 0:
            _decide_order(self._ctx, traj, u_name, m, order_tol)
        self.x_dim = self._ctx.x_dim
        self.dim = self._ctx.n_rows

    @property
    def ctx(self):
        return self._ctx

    @property
    def pade_order(self):
        return self._ctx.pade_order

    def _check(self, traj):
        if (traj.dim, traj.N) != self._sig:
            raise ValueError("trajectory shape (dim=%d, N=%d) differs from the one this integrator was built for %r" % (traj.dim, traj.N, self._sig))

    def close(self):
        self._ctx.close()

    def enable_objective_and_rollout(self):
        """Switch the context's ``var_full`` option on: the objective entry points and the rollout then serve it (a freshly built integrator
        refuses them).  ``Objective.bind``, ``rollout`` and ``variational_rollout`` call this themselves.  A large variational context whose
        ``large_var_full`` is on serves them already: nothing is done there."""
        if self._ctx.large_variational and self._ctx.large_var_full:
            return
        if not self._ctx.get_option("var_full"):
            self._ctx.set_option("var_full", 1)

    def rollout(self, traj_or_Z):
        """``[N, x_dim]``: the stacked states ``vcat(x, x_var_1, ..)`` at every knot by exact propagation under the lifted generator
        (``x <- E x``, ``x_var_i <- E x_var_i + L_i x``), from the knot-0 state."""
        self.enable_objective_and_rollout()
        Z = traj_or_Z.datavec if hasattr(traj_or_Z, "datavec") else traj_or_Z
        return self._ctx.rollout(Z)[0]

    def rollout_dev(self, Z_dev, out_dev):
        """Device buffers: ``Z_dev`` the variable vector, ``out_dev`` ``N * x_dim`` doubles."""
        self.enable_objective_and_rollout()
        self._ctx.rollout_dev(Z_dev, out_dev)


def variational_rollout(B, traj):
    """The stacked iso-vec states ``vcat(x, x_var_1, ..)`` at every knot, ``x_dim x N`` (next to ``unitary_rollout``): exact propagation of the
    state and its sensitivities on the GPU.  ``B``: a ``VariationalUnitaryIntegrator`` / ``VariationalKetIntegrator``."""
    if not isinstance(B, HipVariationalIntegrator):
        raise TypeError("variational_rollout takes a variational integrator, got %s" % type(B).__name__)
    B._check(traj)
    return B.rollout(traj).T.copy()


def _variational_generators(sys, scales):
    from .quantum import VariationalQuantumSystem

    if not isinstance(sys, VariationalQuantumSystem):
        raise TypeError("a VariationalQuantumSystem is required, got %s" % type(sys).__name__)
    Gv = sys.G_vars_array()
    scales = np.broadcast_to(np.asarray(scales, dtype=np.float64), (len(Gv),))
    if np.any(scales == 0):
        raise ValueError("scales must be non-zero")
    return [Gv[i] / scales[i] for i in range(len(Gv))]


def VariationalUnitaryIntegrator(sys, traj, x_name, x_variations, u_name="u", *, scales=None, **kw):
    """``VariationalUnitaryIntegrator(sys, traj, :U, [:U_var, ...], :u; scales)`` [REF src/control/integrators.jl:247-264]: generator
    ``var_G(I (x) G(u), [I (x) G_var_i / scales[i]])`` on ``vcat(U, U_var_1, ...)``; ``scales`` defaults to ones.  Keyword arguments as for
    ``HipPadeIntegrator`` (``pade_order``, ``order_tol``, ``device``, ``index_base``, ``exp_hessian``: ``False`` | ``True`` | ``"workspace"``, ``var_compact``)."""
    Gv = _variational_generators(sys, 1.0 if scales is None else scales)
    return HipVariationalIntegrator(sys, traj, x_name, x_variations, u_name, Gv, ket=False, **kw)


def VariationalKetIntegrator(sys, traj, x_name, x_variations, u_name="u", *, scale=1.0, **kw):
    """``VariationalKetIntegrator(sys, traj, :psi, [:psi_var, ...], :u; scale)`` [REF src/control/integrators.jl:234-245]: generator
    ``var_G(G(u), [G_var_i / scale])`` on ``vcat(psi, psi_var_1, ...)``."""
    Gv = _variational_generators(sys, float(scale))
    return HipVariationalIntegrator(sys, traj, x_name, x_variations, u_name, Gv, ket=True, **kw)


class _EnsembleCore:
    """What the M per-member integrators of a SamplingTrajectory share: ONE batched ``pcl_ctx`` (all members, per-member
    drift tiles, one launch) and the results of the last fused evaluation.

    The reference evaluates its integrators one after the other on the same trajectory
    (``evaluate!(delta_i, B_i, traj)`` for i = 1..M [REF src/control/integrators.jl:316-317]); here the first member asked
    about a trajectory launches the fused kernel for ALL members and the others slice their rows out of the cached
    result.  The cache key is the trajectory buffer itself (byte comparison with the copy the results were computed from),
    so a stale result can never be served.  Hessian calls carry a per-member multiplier slice and run on a one-member
    window of the same context (``pcl_set_member_window``)."""

    def __init__(self, fused, n_members):
        self.fused = fused  # HipPadeIntegrator over all members
        self.ctx = fused.ctx
        self.M = n_members
        self.per_rows = self.ctx.x_dim * self.ctx.K
        self.per_jac = self.ctx.jac_per * self.ctx.K
        self.per_hess = self.ctx.hess_per * self.ctx.K
        self._Z = None
        self._delta = None
        self._vals = None
        self.launches = 0  # fused launches so far (tests check the sharing)

    def _fresh(self, Z):
        Z = np.ascontiguousarray(Z, dtype=np.float64).reshape(-1)
        if self._Z is None or self._Z.shape != Z.shape or not np.array_equal(self._Z, Z):
            self._Z = Z.copy()
            self._delta = self._vals = None
        return self._Z

    def delta(self, Z):
        Z = self._fresh(Z)
        if self._delta is None:
            self.ctx.set_member_window(0, self.M)
            self._delta = self.ctx.eval(Z)
            self.launches += 1
        return self._delta

    def delta_and_vals(self, Z):
        Z = self._fresh(Z)
        if self._vals is None:
            self.ctx.set_member_window(0, self.M)
            self._delta, self._vals = self.ctx.eval_jac(Z)
            self.launches += 1
        return self._delta, self._vals

    def close(self):
        self.fused.close()


class _MemberView:
    """The ``ctx``-like object of one member integrator: the generic functions (``evaluate_``, ``eval_jacobian`` ...) call
    ``eval / jac / hess / *_structure`` on it exactly as on a whole context; rows are numbered inside the member's block
    (the reference's integrators are separate objects; the problem adds each block's row offset)."""

    def __init__(self, core, i):
        self._core, self._i = core, i
        c = core.ctx
        self.x_dim, self.K, self.N, self.z_dim, self.z_len = c.x_dim, c.K, c.N, c.z_dim, c.z_len
        self.n_rows, self.jac_nnz, self.hess_nnz = core.per_rows, core.per_jac, core.per_hess

    def eval(self, Z, delta=None):
        i, r = self._i, self._core.per_rows
        d = self._core.delta(Z)[i * r : (i + 1) * r]
        if delta is not None:
            delta[:] = d
            return delta
        return d.copy()

    def jac(self, Z, vals=None):
        i, r = self._i, self._core.per_jac
        v = self._core.delta_and_vals(Z)[1][i * r : (i + 1) * r]
        if vals is not None:
            vals[:] = v
            return vals
        return v.copy()

    def eval_jac(self, Z, delta=None, vals=None):
        return self.eval(Z, delta), self.jac(Z, vals)

    def _windowed(self, fn):
        c = self._core.ctx
        c.set_member_window(self._i, 1)
        try:
            return fn(c)
        finally:
            c.set_member_window(0, self._core.M)

    def jac_structure(self, dtype=np.int64):
        return self._windowed(lambda c: c.jac_structure(dtype))

    def hess_structure(self, dtype=np.int64):
        return self._windowed(lambda c: c.hess_structure(dtype))

    def hess(self, Z, mu, vals=None):
        return self._windowed(lambda c: c.hess(Z, mu, vals))

    def rollout(self, Z):
        return self._windowed(lambda c: c.rollout(Z))


class HipPadeMemberIntegrator:
    """One element of ``BilinearIntegrator(qtraj::SamplingTrajectory, N)``'s ``Vector{BilinearIntegrator}``
    [REF src/control/integrators.jl:134-162]: the dynamics rows of ONE ensemble member (state component ``x_name``, the
    member's own system), with the reference's properties ``dim == x_dim*(N-1)``, ``x_dim``, ``x_name``, ``f``.  All members
    of one vector evaluate through a shared batched context (``ensemble``)."""

    def __init__(self, core, i, x_name, G_drift, G_drives, u_name, sig):
        self.ensemble, self.member = core, i
        self.x_name, self.x_names, self.u_name = x_name, [x_name], u_name
        self.G_drift, self.G_drives = G_drift, G_drives
        self._sig = sig
        self._view = _MemberView(core, i)
        self.x_dim = core.ctx.x_dim
        self.dim = core.per_rows
        self._f_ctx = None

    @property
    def ctx(self):
        return self._view

    @property
    def pade_order(self):  # (read from the shared context: never a stale copy of the constructor's argument)
        return self.ensemble.ctx.pade_order

    _check = HipPadeIntegrator._check

    def f(self, x_next, x, u, dt):
        """``B.f(x_next, x, u, dt)`` of this member's system [REF integrators.jl:518-525]."""
        c = self.ensemble.ctx
        if self._f_ctx is None:
            self._f_ctx = _PclContext(d=c.d, m=c.m, N=2, z_dim=c.x_dim + 1 + c.m, u_off=c.x_dim + 1, dt_off=c.x_dim, x_offs=[0],
                                      G0=self.G_drift, Gj=self.G_drives, batch=1, batch_mode=PCL_BATCH_MEMBERS,
                                      state_cols=self.ensemble.fused._state_cols, pade_order=_resolved_order(c))  # fmt: skip
        z = np.zeros((2, c.x_dim + 1 + c.m))
        z[0, : c.x_dim], z[0, c.x_dim], z[0, c.x_dim + 1 :] = x, dt, np.asarray(u)[: c.m]
        z[1, : c.x_dim] = x_next
        return self._f_ctx.eval(z)

    def close(self):
        if self._f_ctx is not None:
            self._f_ctx.close()
            self._f_ctx = None
        if self.member == 0:
            self.ensemble.close()


class HipPadeMultistart:
    """B independent trajectories of identical shape evaluated in one launch (multistart
    seeds; BASELINE.json config 5).  Not a reference type: the reference has no multistart
    facility; each seed is its own NLP and owns rows/columns ``b``-major."""

    def __init__(self, G_drift, G_drives, traj, batch, x_name=STATE, u_name="u", *, device=0, index_base=0, pade_order=0, order_tol=1e-10):
        G_drives = np.asarray(G_drives, dtype=np.float64)
        n = np.asarray(G_drift).shape[-1]
        m = G_drives.shape[0] if G_drives.size else 0
        xlen = len(traj.components[x_name])
        if xlen % n or not (1 <= xlen // n <= n // 2):
            raise ValueError("state component %r has dim %d, expected n*C with n = %d" % (x_name, xlen, n))
        self._ctx = _PclContext(
            d=n // 2, m=m, N=traj.N, z_dim=traj.dim, u_off=traj.components[u_name].start,
            dt_off=traj.components[traj.timestep].start, x_offs=[traj.components[x_name].start], G0=G_drift,
            Gj=G_drives.reshape(m, n, n), batch=batch, batch_mode=PCL_BATCH_TRAJ, device=device, index_base=index_base,
            state_cols=xlen // n, pade_order=pade_order,
        )  # fmt: skip
        if pade_order == 0:  # (decided from the bounds, else from `traj` -- the shape-defining seed -- as HipPadeIntegrator does)
            _decide_order(self._ctx, traj, u_name, m, order_tol, batch)
        self.batch = batch
        self.x_name = x_name
        self.x_dim = self._ctx.x_dim
        self.dim = self._ctx.n_rows

    @property
    def ctx(self):
        return self._ctx

    def close(self):
        self._ctx.close()


class DerivativeIntegrator:
    """``DerivativeIntegrator(x, dx, traj)``: rows ``x_{k+1} - x_k - dt_k dx_k`` of the problem templates' integrator
    list ``[dynamics, DerivativeIntegrator(u, du), DerivativeIntegrator(du, ddu)]``
    [REF src/control/templates/smooth_pulse_problem.jl:264-275].  ``dx_name=None`` gives the time-consistency rows
    ``t_{k+1} - t_k - dt_k`` [REF :277].  Evaluated on the GPU through the dynamics integrator's context (same
    trajectory layout, same stream)."""

    def __init__(self, x_name, dx_name, traj, like):
        self._ctx = like.ctx
        self._sig = (traj.dim, traj.N)
        self.x_name, self.dx_name = x_name, dx_name
        self.x_off = traj.components[x_name].start
        self.dx_off = -1 if dx_name is None else traj.components[dx_name].start
        self.x_dim = len(traj.components[x_name])
        if dx_name is not None and len(traj.components[dx_name]) != self.x_dim:
            raise ValueError("components %r and %r differ in length" % (x_name, dx_name))
        self.dim, self.nnz = self._ctx.deriv_dims(self.dx_off, self.x_dim)

    @property
    def ctx(self):
        return self

    def _check(self, traj):
        if (traj.dim, traj.N) != self._sig:
            raise ValueError("trajectory shape differs from the one this integrator was built for")

    # the generic functions below dispatch on these three
    def eval(self, Z, delta=None):
        d, _ = self._ctx.deriv_eval_jac(self.x_off, self.dx_off, self.x_dim, Z)
        if delta is not None:
            delta[:] = d
            return delta
        return d

    def jac(self, Z):
        return self._ctx.deriv_eval_jac(self.x_off, self.dx_off, self.x_dim, Z)[1]

    def jac_structure(self, dtype=np.int64):
        r, c = self._ctx.deriv_structure(self.x_off, self.dx_off, self.x_dim)
        return r.astype(dtype), c.astype(dtype)


# ---------------------------------------------------------------------------
# reference-style generic functions
# ---------------------------------------------------------------------------
def BilinearIntegrator(system, traj, x_name=None, u_name="u", **kw):
    """``BilinearIntegrator(qtraj, N)`` for the time-independent unitary path.

    ``system`` is one system (UnitaryTrajectory) -> one integrator, or a list of systems
    (``BilinearIntegrator(qtraj::SamplingTrajectory, N)`` [REF integrators.jl:134-146]) -> a LIST with one integrator per
    member, in member order, as the reference returns and as ``SamplingProblem`` requires
    [REF src/control/templates/sampling_problem.jl:190-223].  Members that share the drive generators (per-member
    ``H_drift`` only -- BASELINE config 4) evaluate through one batched context; an ensemble whose members differ in
    their drive generators too (each member uses its full ``sys.G`` [REF integrators.jl:149-162]) gets one context per
    member.

    The keywords are ``HipPadeIntegrator``'s (the service keywords among them: above ``_SERVICES`` in this module)."""
    if isinstance(system, (list, tuple)):
        from .quantum import OpenQuantumSystem
        from .trajectory import DENSITY

        systems = list(system)
        if any(getattr(s, "time_dependent", False) for s in systems):
            raise NotImplementedError("time-dependent systems use TimeDependentBilinearIntegrator (out of scope)")
        # Every base the reference samples [REF integrators.jl:149-226 (_sampling_integrator)]: unitary and ket members carry one
        # state each, MultiKet / MultiDensity members a LIST of sub-states (one integrator per sub-state, all on the member's
        # system), density members their compact Lindbladian generators.  `x_name`: one entry per member, a name or a list of
        # sub-state names; the result is flat, member-major, sub-states in order -- what the reference's reduce(vcat, ...) returns.
        default = DENSITY if isinstance(systems[0], OpenQuantumSystem) else STATE
        names = x_name or ["%s%d" % (default, i) for i in range(1, len(systems) + 1)]
        if len(names) != len(systems):
            raise ValueError("%d state names for %d systems" % (len(names), len(systems)))
        per = [[nm] if isinstance(nm, str) else list(nm) for nm in names]
        flat = [nm for p_ in per for nm in p_]
        owner = [i for i, p_ in enumerate(per) for _ in p_]
        Gd = [s.G_drives_array() for s in systems]

        def fused_members(idx):  # one batched context over the (member, sub-state) pairs `idx` that share drive generators
            fused = HipPadeIntegrator(np.array([systems[owner[j]].G_drift for j in idx]), Gd[owner[idx[0]]], traj, [flat[j] for j in idx], u_name, **kw)
            core = _EnsembleCore(fused, len(idx))
            return [HipPadeMemberIntegrator(core, a, flat[j], systems[owner[j]].G_drift, fused.G_drives, u_name, fused._sig)
                    for a, j in enumerate(idx)]  # fmt: skip

        if all(np.array_equal(Gd[0], g) for g in Gd[1:]):
            return fused_members(list(range(len(flat))))
        out = []  # members that differ in their drive generators too: a context per member (shared by its sub-states)
        for i, s in enumerate(systems):
            idx = [j for j in range(len(flat)) if owner[j] == i]
            out += [HipPadeIntegrator(s.G_drift, Gd[i], traj, flat[idx[0]], u_name, **kw)] if len(idx) == 1 else fused_members(idx)
        return out
    if getattr(system, "time_dependent", False):
        raise NotImplementedError("time-dependent systems use TimeDependentBilinearIntegrator (out of scope)")
    from .quantum import OpenQuantumSystem
    from .trajectory import DENSITY

    if isinstance(system, OpenQuantumSystem):  # BilinearIntegrator(qtraj::DensityTrajectory, N) [REF integrators.jl:82-95]
        return HipPadeIntegrator(system.G_drift, system.G_drives_array(), traj, x_name or DENSITY, u_name, **kw)
    return HipPadeIntegrator(system.G_drift, system.G_drives_array(), traj, x_name or STATE, u_name, **kw)


def evaluate_(delta, B, traj):
    """``evaluate!(delta, B, traj)``: fills ``delta`` (length ``B.dim``) in place."""
    B._check(traj)
    if delta.shape != (B.dim,):
        raise ValueError("delta must have length B.dim = %d" % B.dim)
    B.ctx.eval(traj.datavec, delta)
    return delta


def jacobian_structure(B, dtype=np.int64):
    return B.ctx.jac_structure(dtype)


def hessian_structure(B, dtype=np.int64):
    return B.ctx.hess_structure(dtype)


def eval_jacobian(B, traj):
    """``eval_jacobian(B, traj)`` -> scipy.sparse CSR of shape
    ``(B.dim, traj.dim*traj.N + traj.global_dim)``."""
    import scipy.sparse as sp

    B._check(traj)
    vals = B.ctx.jac(traj.datavec)
    rows, cols = B.ctx.jac_structure()
    return sp.csr_matrix((vals, (rows, cols)), shape=(B.dim, traj.dim * traj.N + traj.global_dim))


def eval_hessian_of_lagrangian(B, traj, mu):
    """Symmetric ``sum_k mu_k^T grad^2 delta_k`` as scipy.sparse CSR (full, both triangles)."""
    import scipy.sparse as sp

    B._check(traj)
    vals = B.ctx.hess(traj.datavec, mu)
    rows, cols = B.ctx.hess_structure()
    nv = traj.dim * traj.N + traj.global_dim
    L = sp.coo_matrix((vals, (rows, cols)), shape=(nv, nv)).tocsr()
    return L + sp.tril(L, -1).T


def unitary_rollout(B, traj):
    """``unitary_rollout(traj, sys; interpolation = :constant)`` [REF src/quantum/dynamics.jl:631-667]: the iso-vec
    states at every knot, ``x_dim x N`` (a list of such arrays for an ensemble integrator), by exact propagation
    ``exp(dt_k G(u_k))`` on the GPU instead of an ODE solve.  Starts from the trajectory's knot-0 state."""
    B._check(traj)
    X = B.ctx.rollout(traj.datavec)
    outs = [X[i].T.copy() for i in range(X.shape[0])]
    return outs[0] if len(outs) == 1 else outs


def unitary_rollout_fidelity(B, traj, U_goal=None):
    """``unitary_rollout_fidelity`` [REF src/quantum/dynamics.jl:594-629]: ``|tr(U_goal' U_N)|^2 / d^2`` of the rolled-out
    terminal state(s); ``U_goal`` defaults to the trajectory's goal for the integrator's state."""
    from .quantum import iso_vec_to_operator

    X = unitary_rollout(B, traj)
    Xs = X if isinstance(X, list) else [X]
    fids = []
    for name, Xi in zip(B.x_names, Xs):
        Ug = np.asarray(U_goal) if U_goal is not None else iso_vec_to_operator(traj.goal[name])
        Uf = iso_vec_to_operator(Xi[:, -1])
        fids.append(abs(np.trace(Ug.conj().T @ Uf)) ** 2 / Ug.shape[0] ** 2)
    return fids[0] if len(fids) == 1 else fids
