"""Inputs and models of the steady-state target tests (tests/test_target.py,
tests/test_gpu_target.py): the rows of held outputs and free
inputs, their seeded cases on top of tests/equilibrium_cases.py, the oracle's
full linearisation and one bordered Newton step in numpy's float64 and in long
double.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import _oracle as O
import cmpc
import equilibrium_cases as EC

PLANT_INPUT = (0, 3, 4, 7)      # plant input of control input c (both plants)
# outputs that are pressures (moved by 0.02); the others are surge distances (0.3)
PRESSURE_OUTPUTS = {0: (2, 3), 1: (0, 2)}
# (plant, held outputs, free control inputs): the torque-only rows
TORQUE_ROWS = (
    (0, (0, 1), (0, 2)),
    (0, (2, 3), (0, 2)),
    (0, (0, 3), (0, 2)),
    (0, (3,), (0,)),
    (1, (1, 3), (0, 2)),
    (1, (0, 2), (0, 2)),
    (1, (3,), (2,)),
)
ALL_FOUR = ((0, 1, 2, 3), (0, 1, 2, 3))
RECYCLE_OFFSETS = (0.05, 0.2)


def outputs(plant, x):
    return np.stack([cmpc.plant_output(plant, r) for r in np.atleast_2d(x)])


def or_linearize_full(plant, x, u, p_in=1.0, p_out=1.0):
    """(A ns x ns, B ns x 4, C 4 x ns, f ns) of the oracle's continuous linearisation."""
    ns = EC.NS[plant]
    A, B, C, f = np.zeros(ns * ns), np.zeros(ns * 4), np.zeros(4 * ns), np.zeros(ns)
    EC.oracle().or_plant_linearize(plant, p_in, p_out, O.dptr(np.ascontiguousarray(x, np.float64)),
                                   O.dptr(np.ascontiguousarray(u, np.float64)), O.dptr(A), O.dptr(B), O.dptr(C),
                                   O.dptr(f))
    return A.reshape(ns, ns), B.reshape(ns, 4), C.reshape(4, ns), f


_memo = {}


def cases(plant, hold, B=64, recycle=False, seed=EC.SEED):
    """(pressures (B, 2), u_full (B, ni), x_eq (B, ns), targets (B, nh)): the
    seeded cases of equilibrium_cases (recycle: both recycle valves opened to
    an offset in RECYCLE_OFFSETS), each at its own equilibrium, and targets
    that move the held outputs from there by up to 0.3 (surge distance) or
    0.02 (pressure).  Computed once per argument set; treat as read-only."""
    key = (plant, tuple(hold), B, recycle, seed)
    if key not in _memo:
        p, u, x0 = EC.cases(plant, B=B, seed=seed)
        rng = np.random.default_rng([seed, plant, int(recycle)] + list(hold))
        if recycle:
            u = u.copy()
            u[:, [3, 7]] = rng.uniform(*RECYCLE_OFFSETS, (B, 2))
        x, st, _, _ = cmpc.plant_equilibrium(plant, p, u, x0)
        assert (st == cmpc.CMPC_EQ_OK).all()
        step = np.array([0.02 if h in PRESSURE_OUTPUTS[plant] else 0.3 for h in hold])
        t = outputs(plant, x)[:, list(hold)] + rng.uniform(-1, 1, (B, len(hold))) * step
        for a in (p, u, x, t):
            a.setflags(write=False)
        _memo[key] = (p, u, x, t)
    return _memo[key]


def bordered(plant, hold, free, t, x, u, p_in, p_out):
    """The Newton system [[A, B_free], [C_hold, 0]] d = [-f; t - y] from the oracle."""
    A, B, C, f = or_linearize_full(plant, x, u, p_in, p_out)
    nh = len(hold)
    M = np.block([[A, B[:, list(free)]], [C[list(hold)], np.zeros((nh, nh))]])
    r = np.concatenate([-f, np.asarray(t) - O.plant_output(plant, np.ascontiguousarray(x))[list(hold)]])
    return M, r


def newton_step_models(plant, hold, free, t, x, u, p_in, p_out):
    """(x, u_free) after one bordered step: (numpy float64, long double), each
    as one vector [x; u_free]."""
    M, r = bordered(plant, hold, free, t, x, u, p_in, p_out)
    z = np.concatenate([x, np.asarray(u)[[PLANT_INPUT[c] for c in free]]])
    return z + np.linalg.solve(M, r), np.asarray(z, dtype=np.longdouble) + EC.solve_longdouble(M, r)
