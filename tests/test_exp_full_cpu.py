"""What the option exp_full of the exponential constraint rests on, without a GPU (cases, truth and tolerance: tests/exp_full_cases.py):
the adjoint identity behind the payload-only launch, that the comparison sees the faults such a launch can have, the bookkeeping of the
compact layout, and the host mirror's keyword and offsets."""
import numpy as np
import pytest

import exp_full_cases as xc
import piccolo_jl_amd as pa
from exp_full_cases import TOL


@pytest.mark.parametrize("with_lam", [True, False], ids=["lam", "merit"])
@pytest.mark.parametrize("name", sorted(xc.CASES))
def test_adjoint_payload_is_the_payload_of_the_jacobian(name, with_lam):
    """[phi | -h <V, G_l> | -<V, G>] with V = L(A'; Lam X_k') against J'(w lam) in np.longdouble from the truth's Jacobian values."""
    want, scale = xc.payload_truth(name, with_lam)
    w = xc.worst(xc.adjoint_payload(name, with_lam), want, scale)
    print("%s: worst |adjoint - truth| / (|w lam| |column|) = %.2e" % (name, w))
    assert w <= TOL


@pytest.mark.parametrize("fault", ["drop_col", "drop_drive", "ignore_weight", "no_h", "no_g0"])
def test_the_comparison_sees_each_fault(fault):
    """Case i (three members, their own drifts, unequal weights, two drives): every fault moves the comparison by at least 1e4 x the tolerance."""
    for with_lam in (True, False):
        want, scale = xc.payload_truth("i", with_lam)
        assert xc.worst(xc.adjoint_payload("i", with_lam), want, scale) <= TOL
        w = xc.worst(xc.adjoint_payload("i", with_lam, **{fault: True}), want, scale)
        print("%s (%s): %.2e" % (fault, "lam" if with_lam else "merit", w))
        assert w >= 1e4 * TOL


@pytest.mark.parametrize("name", sorted(xc.CASES))
def test_compact_layout_expands_to_the_full_layout(name):
    c = xc.case(name)
    n, C, m, K = c.n, c.cols, c.m, c.lay.K
    vals = xc.truth(name)[1].reshape(c.batch * K, -1)
    per, cper = xc.full_per(n, C, m), xc.compact_per(n, C, m)
    assert vals.shape[1] == per == C * n * n + c.lay.x_dim * (m + 2) and cper == n * n + c.lay.x_dim * (m + 1)
    comp = xc.compact_of_full(vals, n, C, m)
    assert comp.shape == (c.batch * K, cper)
    full = xc.expand_compact(comp, n, C, m)
    assert np.array_equal(full, vals)
    o1, ot = C * n * n, C * n * n + C * n  # the ones, the tail
    assert np.array_equal(full[:, o1:ot], np.ones((c.batch * K, C * n)))
    for cc in range(C):
        assert np.array_equal(full[:, cc * n * n : (cc + 1) * n * n], comp[:, : n * n])
    assert np.array_equal(full[:, ot:], comp[:, n * n :])


def test_exp_full_keyword_needs_the_exponential_constraint():
    """ValueError before any device call (no library is loaded, no context is created)."""
    args = xc.ctx_args("a")
    for order in (4, 0, 10):
        with pytest.raises(ValueError, match="exp_full"):
            pa.integrators._PclContext(pade_order=order, exp_full=True, **args)
        with pytest.raises(ValueError, match="exp_full"):
            pa.HipPadeIntegrator(None, None, None, pade_order=order, exp_full=True)
    for mode in (pa._lib.PCL_BATCH_VARIATIONAL, pa._lib.PCL_BATCH_VARIATIONAL_EXP):
        with pytest.raises(ValueError, match="variational"):
            pa.integrators._PclContext(pade_order="exp", exp_full=True, **dict(args, batch_mode=mode))
    pa.integrators._check_services(pade_order="exp", exp_full=True)
    pa.integrators._check_services(pade_order=-1, exp_full=True)
    pa.integrators._check_services(pade_order=4, exp_full=False)


def test_jacobian_views_with_the_exponential_offsets():
    import torch

    from piccolo_jl_amd import distributed as dist

    batch, K, d, m, C = 2, 3, 3, 2, 2
    n = 2 * d
    per = C * n * n + n * C * (m + 2)
    buf = torch.arange(batch * K * per, dtype=torch.float64)
    tail = dist.jacobian_views(buf, batch, K, d, m, cols=C, exponential=True)
    assert tuple(tail.shape) == (batch, K, C, m + 1, n) and tail.data_ptr() == buf.data_ptr() + 8 * (C * n * n + C * n)
    for b, k, c, l, i in ((0, 0, 0, 0, 0), (1, 2, 1, 2, 5), (0, 1, 1, 0, 3)):
        assert tail[b, k, c, l, i].item() == (b * K + k) * per + C * n * n + C * n + (c * (m + 1) + l) * n + i
    # the merit and its shared gradient from an exponential buffer: the values of case a's truth
    cs = xc.case("a")
    ds, vs = xc.truth("a")
    phi, gu, gdt = dist.constraint_merit_and_shared_gradient(torch.from_numpy(ds.reshape(-1).copy()), torch.from_numpy(vs.reshape(-1).copy()), 1, cs.lay.K, cs.n // 2,
                                                           cs.m, exponential=True)
    want, scale = xc.payload_truth("a", False)
    got = np.concatenate([[phi.item()], gu.numpy().reshape(-1), gdt.numpy()])[None]
    assert xc.worst(got, want, scale) <= TOL
    # the default path is the Pade layout, untouched
    pper = 2 * C * n * n + n * C * (m + 1)
    pt = dist.jacobian_views(torch.arange(batch * K * pper, dtype=torch.float64), batch, K, d, m, cols=C)
    assert pt[0, 0, 0, 0, 0].item() == 2 * C * n * n
