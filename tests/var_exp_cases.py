"""Cases shared by the CPU and GPU tests of the variational integrators on the exponential constraint: (oracle system, H_vars, scales, VarCase)."""
import numpy as np

from oracle import pade_oracle as po
from variational_truth import VarCase, h_var_drift, make_case

P = po.PAULIS


def pauli(ket, N=5, seed=1):
    """The system of the reference's variational test item (H = Z / 2, drives X and Y, variation Z / 2), on a trajectory with motion."""
    s = po.quantum_system(P["Z"] / 2, [P["X"], P["Y"]], [1.0, 1.0])
    Hv, scales = [P["Z"] / 2], np.array([1.0])
    return s, Hv, scales, make_case(s, [po.G_of_H(Hv[0])], N=N, seed=seed, ket=ket, dt=0.1, u_scale=0.3)


def config2(nv, N=4, seed=3, ket=False, dt=0.1, **kw):
    s = po.config_system(2)  # d = 4, m = 4
    Hv = [h_var_drift(2, 2), np.kron(P["X"], P["I"])][:nv]
    scales = np.array([10.0, 3.0])[:nv]
    return s, Hv, scales, make_case(s, [po.G_of_H(h) / sc for h, sc in zip(Hv, scales)], N=N, seed=seed, ket=ket, dt=dt, **kw)


def config3(nv, N=4, seed=11, ket=False, dt=0.1, **kw):
    s = po.config_system(3)  # d = 27, m = 6
    Hv = [h_var_drift(3, 3), po.lift_operator(po.annihilate(3) + po.annihilate(3).conj().T, 2, [3, 3, 3])][:nv]
    scales = np.full(nv, 10.0)
    return s, Hv, scales, make_case(s, [po.G_of_H(h) / sc for h, sc in zip(Hv, scales)], N=N, seed=seed, ket=ket, dt=dt, **kw)


def d25(N=4, seed=2):
    s = po.multi_transmon_system([4.0, 4.1], [0.2, 0.21], [[0, 0.01], [0.01, 0]], levels_per_transmon=5, drive_bounds=0.1)
    Hv, scales = [h_var_drift(5, 2)], np.array([10.0])
    return s, Hv, scales, make_case(s, [po.G_of_H(Hv[0]) / 10], N=N, seed=seed)


def transmon(levels, N=4, seed=4, ket=False):
    """One transmon with `levels` levels (n = 2 levels), two drives: the sizes at the LDS boundary."""
    s = po.transmon_system(levels=levels, delta=0.02)
    a = po.annihilate(levels)
    Hv, scales = [2 * np.pi * (a.conj().T @ a)], np.array([10.0])
    return s, Hv, scales, make_case(s, [po.G_of_H(Hv[0]) / 10], N=N, seed=seed, ket=ket)


def with_Z(case, Z):
    return VarCase(**{**case.__dict__, "Z": Z})
