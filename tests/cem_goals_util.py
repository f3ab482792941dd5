"""What the tests of the cross-entropy refit under the line search's objective
share (tests/test_cem_goals.py; pddp_cem_{track,weighted,track_weighted}_*,
the cem_goals_kernel of csrc/cem.hip, ILQRSolver.cem with
objective="search"): the entry points called directly - the form chosen by
what the solver has set, `sampled_goals_util.goal_lead` - and, without a
device, the inputs and the oracle's costs of a case, for the searches on the
CPU that the test module notes.  The model of the law is `cem_util`'s, the
objective and the oracle's rollouts under it `sampled_goals_util`'s.

pytest rewrites `assert` in test modules only: every assert here carries its
own message."""
import ctypes
import types

import numpy as np
import torch

from cem_util import (host_inputs, model_candidates, model_rank, model_refit,
                      random_sigma)
from mppi_util import model_e
from sampled_goals_util import goal_lead, oracle_rollouts, weights
from shoot_util import std_vec
from solver_util import (BOUND, SENTINEL, fresh_ops, perturbed,
                         reference_rows, to_device)

ROWS = ("J", "rank", "best", "J_best", "n_elite", "J_m", "Z", "U", "S")


def floor_of(problem, m):
    """std_min [m]: another floor for every component (tests/test_cem.py's)."""
    return 0.02 * BOUND[problem] * (1.0 + np.arange(m))


def cem_call(s, S, K, sigma, smooth=0.0, mix=0.0, seed=0, offset=0,
             std_min=None, active=None, b0=0, z0=None, U=None, rows=True,
             ranks=True, J_best=True, **goal):
    """pddp_cem_{track,weighted,track_weighted}_* itself on trajectories b0..
    (`cem_util.cem_call`'s conventions; `goal`: goal_lead's)."""
    from pddp_amd import _native
    B, N, n, m = s.B - b0, s.N, s.n, s.m
    opts = dict(dtype=s.dtype, device="cuda")
    iopt = dict(dtype=torch.int32, device="cuda")
    z0 = (s.z0 if z0 is None else z0)[b0:].contiguous()
    U = (s.U if U is None else U)[b0:].contiguous()
    if torch.is_tensor(sigma):
        sg = sigma.to(**opts)[b0:].contiguous()
    else:
        sg = to_device(np.broadcast_to(np.asarray(sigma, np.float64),
                                       (s.B, N, m))[b0:].copy(), s.dtype)
    out = types.SimpleNamespace(
        J=torch.full((B, S), SENTINEL, **opts),
        rank=torch.full((B, S), -9, **iopt) if ranks else None,
        best=torch.full((B,), -9, **iopt),
        J_best=torch.full((B,), SENTINEL, **opts) if J_best else None,
        n_elite=torch.full((B,), -9, **iopt),
        J_m=torch.full((B,), SENTINEL, **opts),
        Z=torch.full((B, N + 1, n), SENTINEL, **opts) if rows else None,
        U=torch.full((B, N, m), SENTINEL, **opts) if rows else None,
        S=torch.full((B, N, m), SENTINEL, **opts) if rows else None)
    p = _native.ptr
    # (every tensor the launch reads is held by a name until it has run)
    floor = None if std_min is None else std_vec(s, std_min)
    mask = None if active is None else active[b0:].contiguous()
    suffix, lead, keep = goal_lead(s, b0, **goal)
    _native.call("pddp_cem" + suffix, s.dtype, ctypes.addressof(s.problem),
                 *lead, B, N, S, K, p(z0), p(U), p(s.u_min), p(s.u_max),
                 p(sg), p(floor), float(smooth), float(mix), seed, offset,
                 p(mask), p(out.J), p(out.rank), p(out.best), p(out.J_best),
                 p(out.n_elite), p(out.J_m), p(out.Z), p(out.U), p(out.S),
                 s._s())
    torch.cuda.synchronize()
    return out


# ---- without a device: the searches the test module notes --------------------
def host_objective(problem, dtype, B, N, form, table, L, t0):
    """`sampled_goals_util.objective_solver`'s inputs without a solver: the
    same seeds, the same order.  form None: no objective (the table only)."""
    z0, U = host_inputs(problem, dtype, B, N)
    m = U.shape[2]
    o = types.SimpleNamespace(z0=z0, U=U, xr=None, ur=None, t0=t0,
                              u_min=np.full(m, -BOUND[problem]),
                              u_max=np.full(m, BOUND[problem]))
    ops = perturbed(problem, B, seed=41)[3] if table else None
    if form in ("ref", "both"):
        o.xr, o.ur = reference_rows(problem, B, L, seed=42)
    if form in ("weights", "both"):
        ops = weights(problem, B, seed=43, ops=ops)[3]
    o.ops = fresh_ops(problem, B) if ops is None else ops
    return o


def host_costs(problem, dtype, B, N, form, table, L, t0, S, smooth, seed):
    """(o, sigma, e, J): the oracle's costs under the objective along the
    model's candidates of `seed`, drawn with test_cem_goals' widths."""
    o = host_objective(problem, dtype, B, N, form, table, L, t0)
    m = o.U.shape[2]
    sigma = random_sigma(problem, B, N, m, 13, dtype)
    e = model_e(B, N, S, m, smooth, seed, 0, dtype)
    Uc, _ = model_candidates(o.U, sigma, e, o.u_min, o.u_max)
    _, J = oracle_rollouts(o.ops, o.z0, Uc, dtype, o.xr, o.ur, t0)
    return o, sigma, e, J


def host_smallest_V(problem, dtype, B, N, form, table, L, t0, S, smooth, seed,
                    K, mix=0.25):
    """The smallest entry of the model's V under the ORACLE's ranking."""
    o, sigma, e, J = host_costs(problem, dtype, B, N, form, table, L, t0, S,
                                smooth, seed)
    rank, _, _ = model_rank(J, K)
    _, _, V = model_refit(o.U, sigma, e, rank, K, mix, dtype)
    return float(V.min())


def clear_pairs(J, tol):
    """[B][S] bool: the (b, s) whose cost is further than 4 tol |J| from both
    of its neighbours in the order of the costs - `_check_selection`'s rule,
    for every rank."""
    J = np.asarray(J, np.float64)
    B, S = J.shape
    clear = np.ones((B, S), bool)
    for b in range(B):
        order = np.argsort(J[b], kind="stable")
        v = J[b, order]
        near = np.diff(v) <= 4 * tol * np.abs(v[:-1])
        bad = np.zeros(S, bool)
        bad[:-1] |= near
        bad[1:] |= near
        clear[b, order] = ~bad
    return clear
