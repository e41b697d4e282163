"""Inputs and models of the steady-state gain tests (tests/test_gains.py,
tests/test_gpu_gains.py): the 64 seeded cases per plant (the
cases of tests/equilibrium_cases.py with both recycle valves opened as
tests/target_cases.py opens them, each at its own equilibrium), the gains from
the oracle's linearisation in numpy's float64 and in long double, and the
gains by central differences of the nonlinear plant's equilibria.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import cmpc
import equilibrium_cases as EC
import target_cases as TC

ALL = (0, 1, 2, 3)
H_P = 2.0 ** -21          # the pressure step of E (gains_body.h)
H_U = 1e-5                # the step of the nonlinear differences, inputs and pressures
NAN_BITS = np.uint64(0x7ff8000000000000)
# (outputs, inputs) of the selections under test
SELECTIONS = (((0,), (0,)), ((0, 1), (0, 2)), (ALL, ALL), (ALL, (0, 2)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def cases(plant, B=64):
    """(pressures (B, 2), u_full (B, ni), x_eq (B, ns)): pressures uniform in
    [0.95, 1.05]^2, input offsets within 0.02, both recycle valves opened to
    [0.05, 0.2], every scenario at its own equilibrium (solved by
    cmpc.plant_equilibrium).  Computed once; read-only."""
    return TC.cases(plant, ALL, B=B, recycle=True)[:3]


def scaled_diff(a, b):
    """max |a - b| over max |b|: the error scaled by the matrix's largest entry."""
    a = np.asarray(a, dtype=np.longdouble)
    b = np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def or_pressure_matrix(plant, x, u, p_in, p_out, h=H_P):
    """E = df/dp (ns x 2) by central differences of the oracle's derivative."""
    d = lambda pi, po: EC.or_derivative(plant, x, u, pi, po)
    return np.stack([(d(p_in + h, p_out) - d(p_in - h, p_out)) / (2 * h),
                     (d(p_in, p_out + h) - d(p_in, p_out - h)) / (2 * h)], axis=1)


def _solve_ld(A, Bm):
    """A^-1 Bm in long double, column by column."""
    return np.stack([EC.solve_longdouble(A, Bm[:, j]) for j in range(Bm.shape[1])], axis=1)


def gain_models(plant, x, u, p_in, p_out, outputs=ALL, inputs=ALL):
    """G, Gp, RGA and K_ff from the oracle's A, B, C and its differenced E:
    (numpy float64, long double), each a dict; RGA and K_ff only for a square
    selection."""
    A, Bm, C, _ = TC.or_linearize_full(plant, x, u, p_in, p_out)
    E = or_pressure_matrix(plant, x, u, p_in, p_out)
    Bs, Cs = Bm[:, list(inputs)], C[list(outputs)]
    m64 = {"G": -Cs @ np.linalg.solve(A, Bs), "Gp": -Cs @ np.linalg.solve(A, E)}
    Cl = np.asarray(Cs, dtype=np.longdouble)
    mld = {"G": -Cl @ _solve_ld(A, Bs), "Gp": -Cl @ _solve_ld(A, E)}
    if len(outputs) == len(inputs):
        n = len(outputs)
        m64["rga"] = m64["G"] * np.linalg.inv(m64["G"]).T
        m64["k_ff"] = -np.linalg.solve(m64["G"], m64["Gp"])
        mld["rga"] = mld["G"] * _solve_ld(mld["G"], np.eye(n)).T
        mld["k_ff"] = -_solve_ld(mld["G"], mld["Gp"])
    return m64, mld


_fd = {}


def nonlinear_gains(plant):
    """(G (B, 4, 4), Gp (B, 4, 2)) of cases(plant) by central differences of
    host-solved equilibria: +-H_U on each control input and on each pressure.
    Computed once; read-only."""
    if plant not in _fd:
        p, u, x = cases(plant)

        def rest(pp, uu):
            xe, st, _, _ = cmpc.plant_equilibrium(plant, pp, uu, x)
            assert (st == cmpc.CMPC_EQ_OK).all()
            return TC.outputs(plant, xe)

        G, Gp = np.zeros((len(x), 4, 4)), np.zeros((len(x), 4, 2))
        for c, col in enumerate(TC.PLANT_INPUT):
            d = np.zeros_like(u)
            d[:, col] = H_U
            G[:, :, c] = (rest(p, u + d) - rest(p, u - d)) / (2 * H_U)
        for k in range(2):
            d = np.zeros_like(p)
            d[:, k] = H_U
            Gp[:, :, k] = (rest(p + d, u) - rest(p - d, u)) / (2 * H_U)
        G.setflags(write=False)
        Gp.setflags(write=False)
        _fd[plant] = (G, Gp)
    return _fd[plant]
