"""The reference's rule for ONE attempt of one trajectory, restated in plain
Python from pddp/controllers/ilqr.py - the yardstick of the decision-table
tests (test_accept_table.py, test_accept_fused_table.py), itself held to the
C oracle's fit traces and to a recording of the reference's own schedule
methods (test_accept_model.py).

  ilqr.py:140-145   a backward pass that raised: _increase_reg, NOT_PD / MAX_REG
  ilqr.py:161-181   argmin, `J_new < J_opt`, _decrease_reg, CONVERGED / ACCEPTED,
                    else _increase_reg, REJECTED / MAX_REG
  ilqr.py:298-314   the fit loop: a retry state repeats the step, ACCEPTED
                    starts the next of `n_iterations` steps, a terminal state
                    (CONVERGED, MAX_REG) leaves
  ilqr.py:364-390   _reset_reg / _decrease_reg / _increase_reg

`mu` and `delta` are Python floats (the reference's `self._mu`, `self._delta`);
costs, the `<` test and `|J_opt - J_new| / J_opt < tol` are numpy scalars of
the run's dtype, `tol` cast to it (a Python number compared with a tensor takes
the tensor's dtype).  Not a test and not a conftest: imported by the tests.
"""
import collections

import numpy as np

# iLQRState (ilqr.py:35-55)
UNDEFINED, ACCEPTED, REJECTED, NOT_PD, MAX_REG, CONVERGED = 0, 1, 2, 3, 4, 5

MU_MIN = 1e-6   # ilqr.py:94
DELTA_0 = 2.0   # ilqr.py:95

Attempt = collections.namedtuple(
    "Attempt", "state J_opt mu delta iter active fresh amin")


def reset_reg():
    """ilqr.py:364-367 -> (mu, delta)."""
    return 0.0, DELTA_0


def decrease_reg(mu, delta):
    """ilqr.py:369-374 -> (mu, delta)."""
    delta = min(1.0, delta) / DELTA_0
    mu *= delta
    if mu <= MU_MIN:
        mu = 0.0
    return mu, delta


def increase_reg(mu, delta, max_reg):
    """ilqr.py:376-390 -> (mu, delta, ok); ok False: max_reg reached."""
    delta = max(1.0, delta) * DELTA_0
    mu = max(MU_MIN, mu * delta)
    return mu, delta, not (mu >= max_reg)


def argmin(Jc):
    """torch.argmin (ilqr.py:161): the first NaN if there is one, the first
    of the smallest entries otherwise."""
    Jc = np.asarray(Jc)
    nan = np.isnan(Jc)
    if nan.any():
        return int(np.flatnonzero(nan)[0])
    return int(np.flatnonzero(Jc == Jc.min())[0])


def attempt(J_opt, Jc, bwd_status, mu, delta, iter, tol, max_reg,
            n_iterations, dtype):
    """One attempt.  `iter`: the number of step() calls started, this one
    included (1 .. n_iterations).  `amin` of the result: the candidate that
    became the nominal, -1 when the nominal stays."""
    dt = np.dtype(dtype).type
    mu, delta, iter = float(mu), float(delta), int(iter)
    J_opt = dt(J_opt)
    won = -1
    if int(bwd_status) != 0:
        mu, delta, ok = increase_reg(mu, delta, max_reg)
        state = NOT_PD if ok else MAX_REG
    else:
        a = argmin(np.asarray(Jc, dtype=dt))
        J_new = dt(np.asarray(Jc, dtype=dt)[a])
        if J_new < J_opt:
            won = a
            mu, delta = decrease_reg(mu, delta)
            with np.errstate(all="ignore"):
                rel = dt(abs(dt(J_opt - J_new))) / J_opt
            state = CONVERGED if dt(rel) < dt(tol) else ACCEPTED
            J_opt = J_new
        else:
            mu, delta, ok = increase_reg(mu, delta, max_reg)
            state = REJECTED if ok else MAX_REG
    active = fresh = 0
    if state in (NOT_PD, REJECTED):
        active = 1
    elif state == ACCEPTED and iter < int(n_iterations):
        iter, active, fresh = iter + 1, 1, 1
    return Attempt(state, J_opt, mu, delta, iter, active, fresh, won)
