"""What the tests of the softmin-weighted update share (tests/test_mppi.py;
pddp_mppi_*, csrc/mppi.hip, ILQRSolver.mppi): the numpy model of the update in
float64 - the softmin of GIVEN costs, the weighted mean of `shoot_util`'s
AR(1) values, the clamp - and the entry points called directly.  The
candidates, their costs and the oracle's rollouts are `shoot_util`'s.

pytest rewrites `assert` in test modules only: every assert here carries its
own message."""
import ctypes
import types

import numpy as np
import torch

from golden_util import np_dtype
from shoot_util import STREAM, model_ar1, std_vec
from solver_util import SENTINEL, model_draws, to_device


# ---- the numpy model of the update (include/pddp_hip.h) ---------------------
def model_weights(J, lam):
    """W [B][S] float64: exp(-(J - min finite J) / lam) over the finite costs
    of every row, 0 for the others, normalised; a row without a finite cost,
    or with a temperature that is not positive, is zeros."""
    J = np.asarray(J, np.float64)
    lam = np.broadcast_to(np.asarray(lam, np.float64), J.shape[:1])
    W = np.zeros_like(J)
    for b in range(J.shape[0]):
        fin = np.isfinite(J[b])
        if not fin.any() or not lam[b] > 0:
            continue
        w = np.zeros(J.shape[1])
        w[fin] = np.exp(-(J[b, fin] - J[b, fin].min()) / lam[b])
        W[b] = w / w.sum()
    return W


def model_e(B, N, S, m, smooth, seed, offset, dtype):
    """e [B][N][S][m] float64: the raw AR(1) values of the candidates."""
    return model_ar1(model_draws(B, N, S, m, STREAM, seed, offset, dtype),
                     smooth, dtype)


def weighted_actions(U, W, e, std, u_min=None, u_max=None):
    """Uw [B][N][m] float64 = clip(U + std sum_{s>=1} W[b][s] e[b][t][s]):
    candidate 0 has a weight and no perturbation."""
    U = np.asarray(U, np.float64)
    std = np.broadcast_to(np.asarray(std, np.float64), (U.shape[2],))
    ebar = np.einsum("bs,btsj->btj", W[:, 1:], e[:, :, 1:])
    raw = U + std * ebar
    return raw if u_min is None else np.clip(raw, u_min, u_max)


def model_update(U, J, lam, e, std, u_min=None, u_max=None):
    """(W, Uw) of given costs J [B][S]: `model_weights`, `weighted_actions`."""
    W = model_weights(J, lam)
    return W, weighted_actions(U, W, e, std, u_min, u_max)


# ---- the entry points themselves --------------------------------------------
def mppi_call(s, S, std, lam, smooth=0.0, seed=0, offset=0, active=None, b0=0,
              z0=None, U=None, rows=True, weights=True, bounded=True):
    """pddp_mppi[_batch]_* itself on trajectories b0.. of the solver's z0 and
    U (or the device tensors given, all B trajectories'), with the solver's
    table if one is set; lam: a float or [B] numpy, all B trajectories';
    every output pre-filled with SENTINEL (best: -9)."""
    from pddp_amd import _native
    B, N, n, m = s.B - b0, s.N, s.n, s.m
    opts = dict(dtype=s.dtype, device="cuda")
    z0 = (s.z0 if z0 is None else z0)[b0:].contiguous()
    U = (s.U if U is None else U)[b0:].contiguous()
    out = types.SimpleNamespace(
        J=torch.full((B, S), SENTINEL, **opts),
        best=torch.full((B,), -9, dtype=torch.int32, device="cuda"),
        J_best=torch.full((B,), SENTINEL, **opts),
        W=torch.full((B, S), SENTINEL, **opts) if weights else None,
        J_w=torch.full((B,), SENTINEL, **opts),
        Z=torch.full((B, N + 1, n), SENTINEL, **opts) if rows else None,
        U=torch.full((B, N, m), SENTINEL, **opts) if rows else None)
    p = _native.ptr
    # (every tensor the launch reads is held by a name until it has run)
    a_std = std_vec(s, std)
    lam_t = to_device(np.broadcast_to(np.asarray(lam, np.float64),
                                      (s.B,))[b0:].copy(), s.dtype)
    mask = None if active is None else active[b0:].contiguous()
    table = None if s.batch_table is None else s.batch_table[b0:].contiguous()
    name, lead = "pddp_mppi", (ctypes.addressof(s.problem),)
    if table is not None:
        name, lead = name + "_batch", lead + (p(table),)
    _native.call(name, s.dtype, *lead, B, N, S, p(z0), p(U),
                 p(s.u_min if bounded else None),
                 p(s.u_max if bounded else None), p(a_std), p(lam_t),
                 float(smooth), seed, offset, p(mask), p(out.J), p(out.best),
                 p(out.J_best), p(out.W), p(out.J_w), p(out.Z), p(out.U),
                 s._s())
    torch.cuda.synchronize()
    return out


def rounded(lam, dtype):
    """lam as the launch sees it: rounded to the run's type, in float64."""
    return np.asarray(lam, np.float64).astype(np_dtype(dtype)).astype(
        np.float64)


def wide_solver(problem, dtype, B, N, table=False, wide=True):
    """(solver, the oracle's problem of every trajectory, z0, U, u_min,
    u_max): make_solver's, bounded - tests/test_shoot.py's `_solver`.  `wide`:
    base actions U(-0.8, 0.8) BOUND, so that a perturbation of 0.3 BOUND meets
    the clamp on many steps.  `table`: the per-trajectory problems of
    `perturbed`."""
    from solver_util import BOUND, make_solver, perturbed, set_table
    s, op, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    if wide:
        rng = np.random.RandomState(5)
        U = (BOUND[problem] * rng.uniform(-0.8, 0.8, U.shape)).astype(U.dtype)
        s.U.copy_(torch.from_numpy(U))
    ops = [op] * B
    if table:
        par, xg, ug, ops = perturbed(problem, B, seed=41)
        set_table(s, par, xg, ug)
    return s, ops, z0, U, u_min, u_max
