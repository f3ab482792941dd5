"""What the tests of the one-launch MPPI trial share (tests/test_mppi_trial.py;
pddp_mppi_trial_*, csrc/mppi_trial.hip, ILQRSolver.mppi_closed_loop): the entry
point called directly - in one launch or in several, on all trajectories or on
a tail of them - and the numpy / oracle model of a trial in the run's type:
`shoot_util`'s candidates and rollouts, `mppi_util`'s update, the oracle's plant
step under `solver_util`'s model of the device's normals.

pytest rewrites `assert` in test modules only: every assert here carries its
own message."""
import ctypes
import types

import numpy as np
import torch

import oracle as orc
from golden_util import np_dtype
from mppi_util import model_e, model_update
from shoot_util import model_candidates, oracle_rollouts, std_vec
from solver_util import SENTINEL, model_draws, to_device

# every output and log of a launch, in the order the tests compare them
NAMES = ("z0", "U", "Z", "X", "Ulog", "J", "J0", "Jw", "ess", "plans", "Jc")


def shift(plan):
    """The next step's base: row i + 1 at row i, the last row repeated."""
    return np.concatenate([plan[:, 1:], plan[:, -1:]], axis=1)


def trial_call(s, S, K, T, std, lam, smooth=0.0, seed=0, cand=0, stride=None,
               chunks=None, plant=None, dist=None, w_std=None, v_std=None,
               roll=0, step_offset=0, active=None, b0=0, z0=None, U=None,
               log_costs=True, logs=True):
    """pddp_mppi_trial_* itself on trajectories b0.. of the solver's z0 and U
    (or of the device tensors given, all B trajectories'), with the solver's
    table if one is set: control steps 0 .. T-1 in the launches of `chunks`
    (counts; default one launch), every launch on the buffers the one before
    left.  `stride`: iter_stride, default the FULL batch's B S; the caller of
    a tail passes `cand` + b0 S and `roll` + b0.  With `v_std` the true start
    is z0 and so is the first observation.  plant [B][ROW], dist [B][T][n]
    device tensors of all B trajectories; lam a float or [B] numpy; w_std,
    v_std floats.  Every output pre-filled with SENTINEL."""
    from pddp_amd import _native
    B, N, n, m = s.B - b0, s.N, s.n, s.m
    opts = dict(dtype=s.dtype, device="cuda")

    def full(*shape):
        return torch.full(shape, SENTINEL, **opts)

    def tail(t):
        return None if t is None else t[b0:].contiguous()

    out = types.SimpleNamespace(
        z0=(s.z0 if z0 is None else z0)[b0:].clone().contiguous(),
        U=(s.U if U is None else U)[b0:].clone().contiguous(),
        Z=full(B, N + 1, n), X=full(B, T + 1, n), Ulog=full(B, T, m),
        J=full(B), Y=None, x_true=None,
        J0=full(B, T, K) if logs else None, Jw=full(B, T, K) if logs else None,
        ess=full(B, T) if logs else None,
        plans=full(B, T, N, m) if logs else None,
        Jc=full(B, T, K, S) if log_costs else full(B, S))
    if v_std is not None:
        out.x_true = out.z0.clone()
        out.Y = full(B, T + 1, n)
        out.Y[:, 0] = out.z0
    p = _native.ptr
    # (every tensor the launches read is held by a name until they have run)
    U_work = full(B, N, m)
    a_std = std_vec(s, std)
    lam_t = to_device(np.broadcast_to(np.asarray(lam, np.float64),
                                      (s.B,))[b0:].copy(), s.dtype)
    w_t = None if w_std is None else torch.full((n,), w_std, **opts)
    v_t = None if v_std is None else torch.full((n,), v_std, **opts)
    mask, table = tail(active), tail(s.batch_table)
    plant_t, dist_t = tail(plant), tail(dist)
    t0 = 0
    for count in chunks or [T]:
        _native.call(
            "pddp_mppi_trial", s.dtype, ctypes.addressof(s.problem), p(table),
            p(plant_t), B, N, S, K, T, t0, count, p(out.z0), p(out.U),
            p(out.Z), p(U_work), p(s.u_min), p(s.u_max), p(a_std), p(lam_t),
            float(smooth), seed, cand, s.B * S if stride is None else stride,
            p(dist_t), p(w_t), p(v_t), roll, step_offset, p(out.x_true),
            p(mask), p(out.Jc), int(log_costs), p(out.X), p(out.Ulog),
            p(out.J), p(out.Y), p(out.J0), p(out.Jw), p(out.ess),
            p(out.plans), s._s())
        t0 += count
    torch.cuda.synchronize()
    assert t0 == T, "chunks %r do not add up to %d steps" % (chunks, T)
    return out


def trial_names(out):
    """The names of `out` that hold a tensor: NAMES, and Y / x_true under
    measurement noise."""
    return [nm for nm in NAMES + ("Y", "x_true")
            if getattr(out, nm) is not None]


# ---- the plant step ---------------------------------------------------------
def noise_rows(B, T, n, which, seed, roll, step_offset, dtype):
    """[B][T + 1][n] float64: the unit normals of stream `which` (0 process,
    1 measurement) of trials roll .. roll + B - 1 at steps step_offset .. +T."""
    d = model_draws(B, step_offset + T + 1, 1, n, which, seed, roll, dtype)
    return d[:, step_offset:, 0]


def plant_step(plant_ops, x, u, dtype):
    """(x' [B][n], l(x, u) [B]) in the run's type: the oracle's step and stage
    cost of every trajectory's plant."""
    o, d = orc.load(np_dtype(dtype)), np_dtype(dtype)
    xn, cost = np.empty(x.shape, d), np.empty(x.shape[0], d)
    for b in range(x.shape[0]):
        xb, ub = x[b].astype(d), u[b].astype(d)
        cost[b] = o.cost(plant_ops[b], xb, ub)[0]
        xn[b] = o.dynamics(plant_ops[b], xb, ub, jac=False)[0]
    return xn, cost


def terminal_cost(plant_ops, x, dtype):
    o, d = orc.load(np_dtype(dtype)), np_dtype(dtype)
    return np.array([o.cost(plant_ops[b], x[b].astype(d), None,
                            terminal=True)[0] for b in range(x.shape[0])], d)


# ---- the whole trial --------------------------------------------------------
def model_trial(ops, plant_ops, z0, U, T, K, S, std, lam, smooth, seed, cand,
                u_min, u_max, dist=None, w_std=None, v_std=None, roll=0,
                step_offset=0, dtype="f64"):
    """The trial from the ORACLE's costs: candidates -> oracle costs ->
    `model_update` -> oracle rollout -> took -> plant step, in float64 on
    draws of the run's type.  Returns the logs under trial_call's names (the
    true start is z0, and so is the first observation) and `gap`: the smallest
    |J_w - J_0| / |J_0| the trial met - where that is large against the
    device's cost error, `took` cannot differ."""
    B, N, m = U.shape
    n = z0.shape[1]
    U = np.asarray(U, np.float64).copy()
    lam = np.broadcast_to(np.asarray(lam, np.float64), (B,))
    x, y = (np.asarray(z0, np.float64).copy() for _ in range(2))
    w = noise_rows(B, T, n, 0, seed, roll, step_offset, dtype)
    v = noise_rows(B, T, n, 1, seed, roll, step_offset, dtype)
    r = types.SimpleNamespace(
        X=np.empty((B, T + 1, n)), Ulog=np.empty((B, T, m)), J=np.zeros(B),
        Y=np.empty((B, T + 1, n)), J0=np.empty((B, T, K)),
        Jw=np.empty((B, T, K)), took=np.empty((B, T, K), bool),
        plans=np.empty((B, T, N, m)), gap=np.inf)
    r.Y[:, 0] = y
    for c in range(T):
        for k in range(K):
            off = cand + (c * K + k) * B * S
            Uc, _ = model_candidates(U, S, std, smooth, seed, off, dtype,
                                     u_min, u_max)
            _, J = oracle_rollouts(ops, y, Uc, dtype)
            e = model_e(B, N, S, m, smooth, seed, off, dtype)
            _, Uw = model_update(U, J, lam, e, std, u_min, u_max)
            _, Jw = oracle_rollouts(ops, y, Uw[:, None], dtype)
            J0, Jw = J[:, 0].astype(np.float64), Jw[:, 0].astype(np.float64)
            took = np.isfinite(Jw) & (Jw <= J0)
            r.gap = min(r.gap, (np.abs(Jw - J0) / np.abs(J0)).min())
            r.J0[:, c, k], r.Jw[:, c, k], r.took[:, c, k] = J0, Jw, took
            U = np.where(took[:, None, None], Uw, U)
        r.plans[:, c] = U
        u = np.clip(U[:, 0], u_min, u_max)
        r.X[:, c], r.Ulog[:, c] = x, u
        xn, cost = plant_step(plant_ops, x, u, dtype)
        r.J += cost
        x = xn.astype(np.float64)
        if dist is not None:
            x = x + dist[:, c]
        if w_std is not None:
            x = x + w_std * w[:, c]
        y = x if v_std is None else x + v_std * v[:, c + 1]
        r.Y[:, c + 1] = y
        U = shift(U)
    r.X[:, T] = x
    r.J += terminal_cost(plant_ops, x, dtype)
    r.z0, r.U, r.x_true = y, U, x
    Uc = np.clip(U, u_min, u_max)
    r.Z = oracle_rollouts(ops, y, Uc[:, None], dtype)[0][:, 0]
    return r
