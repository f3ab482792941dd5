"""What the tests of sampled shooting share (tests/test_shoot.py; pddp_shoot_*,
csrc/shoot.hip, ILQRSolver.shoot): the numpy model of the candidates - the
stream-2 normals of `solver_util.model_draws`, the AR(1) over them in float64,
the clamp - the oracle's dynamics and cost stepped candidate by candidate, and
the entry points called directly.

pytest rewrites `assert` in test modules only: every assert here carries its
own message."""
import ctypes
import types

import numpy as np
import torch

import oracle as orc
from golden_util import np_dtype
from solver_util import SENTINEL, TDT, model_draws, to_device

STREAM = 2  # (0 process noise, 1 measurement noise: closed_loop.hip)


# ---- the numpy model of the candidates (include/pddp_hip.h) -----------------
def model_ar1(xi, smooth, dtype):
    """e [B][N][S][m] float64: e_0 = xi_0, e_t = beta e_{t-1} + gamma xi_t
    along axis 1, beta and gamma rounded to the run's type as the entry point
    rounds them."""
    d = np_dtype(dtype)
    beta = float(d(smooth))
    gamma = float(d(np.sqrt(1.0 - float(smooth) ** 2)))
    e = np.empty_like(xi)
    e[:, 0] = xi[:, 0]
    for t in range(1, xi.shape[1]):
        e[:, t] = beta * e[:, t - 1] + gamma * xi[:, t]
    return e


def model_candidates(U, S, std, smooth, seed, offset, dtype, u_min=None,
                     u_max=None):
    """(Uc [B][S][N][m], hit [B][S][N][m]): the applied actions of every
    candidate of the base sequences U [B][N][m] in float64 - candidate 0 the
    base - and where the clamp changed one."""
    U = np.asarray(U, np.float64)
    B, N, m = U.shape
    std = np.broadcast_to(np.asarray(std, np.float64), (m,))
    xi = model_draws(B, N, S, m, STREAM, seed, offset, dtype)
    e = model_ar1(xi, smooth, dtype)
    raw = U[:, :, None, :] + std * e          # [B][N][S][m]
    raw[:, :, 0, :] = U
    raw = raw.transpose(0, 2, 1, 3)           # [B][S][N][m]
    Uc = raw if u_min is None else np.clip(raw, u_min, u_max)
    return np.ascontiguousarray(Uc), Uc != raw


def oracle_rollouts(ops, z0, Uc, dtype):
    """(X [B][S][N+1][n], J [B][S]) in the given dtype: the oracle's dynamics
    and cost stepped along every candidate's applied actions; ops[b]: the
    oracle's problem of trajectory b."""
    o = orc.load(np_dtype(dtype))
    d = np_dtype(dtype)
    B, S, N, _ = Uc.shape
    n = z0.shape[1]
    X = np.empty((B, S, N + 1, n), d)
    J = np.zeros((B, S), d)
    for b in range(B):
        for s in range(S):
            x = z0[b].astype(d)
            for t in range(N):
                u = Uc[b, s, t].astype(d)
                X[b, s, t] = x
                J[b, s] += o.cost(ops[b], x, u)[0]
                x = o.dynamics(ops[b], x, u, jac=False)[0]
            X[b, s, N] = x
            J[b, s] += o.cost(ops[b], x, None, terminal=True)[0]
    return X, J


def first_argmin(J):
    """[B]: the index of the lowest finite cost of every row, the first one on
    ties; -1 where none is finite."""
    J = np.asarray(J, np.float64)
    masked = np.where(np.isfinite(J), J, np.inf)
    best = masked.argmin(axis=1)
    return np.where(np.isfinite(masked).any(axis=1), best, -1).astype(np.int32)


# ---- the entry points themselves --------------------------------------------
def std_vec(s, std):
    """[m] device vector of a level given as a float or a sequence."""
    v = np.broadcast_to(np.asarray(std, np.float64), (s.m,))
    return to_device(v.copy(), s.dtype)


def shoot_call(s, S, std, smooth=0.0, seed=0, offset=0, active=None, b0=0,
               z0=None, U=None, rows=True, bounded=True):
    """pddp_shoot[_batch]_* itself on trajectories b0.. of the solver's z0 and
    U (or the device tensors given, all B trajectories'), with the solver's
    table if one is set; every output pre-filled with SENTINEL (best: -9)."""
    from pddp_amd import _native
    B, N, n, m = s.B - b0, s.N, s.n, s.m
    opts = dict(dtype=s.dtype, device="cuda")
    z0 = (s.z0 if z0 is None else z0)[b0:].contiguous()
    U = (s.U if U is None else U)[b0:].contiguous()
    out = types.SimpleNamespace(
        J=torch.full((B, S), SENTINEL, **opts),
        best=torch.full((B,), -9, dtype=torch.int32, device="cuda"),
        J_best=torch.full((B,), SENTINEL, **opts),
        Z=torch.full((B, N + 1, n), SENTINEL, **opts) if rows else None,
        U=torch.full((B, N, m), SENTINEL, **opts) if rows else None)
    p = _native.ptr
    # (every tensor the launch reads is held by a name until it has run)
    a_std = std_vec(s, std)
    mask = None if active is None else active[b0:].contiguous()
    table = None if s.batch_table is None else s.batch_table[b0:].contiguous()
    name, lead = "pddp_shoot", (ctypes.addressof(s.problem),)
    if table is not None:
        name, lead = name + "_batch", lead + (p(table),)
    _native.call(name, s.dtype, *lead, B, N, S, p(z0), p(U),
                 p(s.u_min if bounded else None),
                 p(s.u_max if bounded else None), p(a_std), float(smooth),
                 seed, offset, p(mask), p(out.J), p(out.best), p(out.J_best),
                 p(out.Z), p(out.U), s._s())
    torch.cuda.synchronize()
    return out


def shoot_draws_call(B, N, S, m, seed, offset, dtype):
    from pddp_amd import _native
    td = TDT[dtype]
    E = torch.full((B, N, S, m), float("nan"), dtype=td, device="cuda")
    _native.call("pddp_shoot_draws", td, B, N, S, m, seed, offset,
                 _native.ptr(E), _native.stream_handle())
    torch.cuda.synchronize()
    return E
