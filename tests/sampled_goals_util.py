"""What the tests of the sampling planners under the line search's objective
share (tests/test_sampled_goals.py; pddp_shoot_* / pddp_mppi_* with the
suffixes _track, _weighted, _track_weighted, pddp_mppi_trial_goals_*,
the *_goals_kernel of csrc/shoot.hip, mppi.hip and mppi_trial.hip;
ILQRSolver.shoot / mppi / mppi_closed_loop with
objective="search"): the per-trajectory weights, the oracle's rollouts with
every step under its reference row, the entry points called directly - the
form chosen by what the solver has set - and the numpy / oracle model of a
tracked trial.  The candidates, the update and the draws are `shoot_util`'s,
`mppi_util`'s and `solver_util`'s.

pytest rewrites `assert` in test modules only: every assert here carries its
own message."""
import ctypes
import types

import numpy as np
import torch

import oracle as orc
from golden_util import DT, np_dtype
from mppi_trial_util import noise_rows, shift
from mppi_util import model_e, model_update
from shoot_util import model_candidates, std_vec
from solver_util import (BOUND, SENTINEL, fresh_ops, make_solver, perturbed,
                         ref_row, reference_rows, set_ref, set_table,
                         to_device, under_row)

FORMS = ("ref", "weights", "both")


# ---- the objective ------------------------------------------------------------
def weights(problem, B, seed, ops=None):
    """tests/test_track_weights.py's `_weights`: (q [B][na], q_term [B][na],
    r [B][m]) as float64 arrays of float32 values, and the oracle's problem of
    every trajectory: `ops` (default: the shared problem B times) with the
    three diagonals overwritten.  q = shared diagonal x U(1, 2) + U(0, 0.5),
    q_term and r = shared diagonal x U(0.5, 2); a Q_term with off-diagonal
    entries (the rendezvous') is drawn upward only, as q."""
    rng = np.random.RandomState(seed)
    base = orc.make_problem(problem, DT[problem])
    na, m = base.aug_size, base.action_size
    dq = np.array([base.Q[i * 8 + i] for i in range(na)])
    dqt = np.array([base.Q_term[i * 8 + i] for i in range(na)])
    dr = np.array([base.R[i * 4 + i] for i in range(m)])
    q = dq * rng.uniform(1.0, 2.0, (B, na)) + rng.uniform(0.0, 0.5, (B, na))
    qt = dqt * rng.uniform(0.5, 2.0, (B, na))
    Qt = np.array(base.Q_term).reshape(8, 8)[:na, :na]
    if np.any(Qt - np.diag(np.diag(Qt))):
        qt = dqt * rng.uniform(1.0, 2.0, (B, na)) + \
            rng.uniform(0.0, 0.5, (B, na))
    r = dr * rng.uniform(0.5, 2.0, (B, m))
    q, qt, r = (a.astype(np.float32).astype(np.float64) for a in (q, qt, r))
    if ops is None:
        ops = fresh_ops(problem, B)
    write_diagonals(ops, q, qt, r)
    return q, qt, r, ops


def write_diagonals(ops, q, qt, r):
    for b, op in enumerate(ops):
        for i in range(q.shape[1]):
            op.Q[i * 8 + i] = q[b, i]
            op.Q_term[i * 8 + i] = qt[b, i]
        for i in range(r.shape[1]):
            op.R[i * 4 + i] = r[b, i]


def set_weights(s, q, qt, r):
    s.set_batch_weights(q=torch.from_numpy(q), q_term=torch.from_numpy(qt),
                        r=torch.from_numpy(r),
                        keep_reference=s.reference is not None)


def objective_solver(problem, dtype, B, N, form, table=False, L=None, t0=0,
                     seeds=(41, 42, 43), wide=True):
    """A bounded solver (`mppi_util.wide_solver`'s start: base actions
    U(-0.8, 0.8) BOUND) with the objective of `form` ("ref", "weights",
    "both") set through the solver's own setters, with or without a table.
    Returns a namespace: s, ops (the oracle's problem of every trajectory:
    table parameters and goals, weights' diagonals), xr / ur (None without a
    reference), t0, z0, U, u_min, u_max, q / qt / r (None without weights)."""
    s, op, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    if wide:
        rng = np.random.RandomState(5)
        U = (BOUND[problem] * rng.uniform(-0.8, 0.8, U.shape)).astype(U.dtype)
        s.U.copy_(torch.from_numpy(U))
    ops = None
    if table:
        par, xg, ug, ops = perturbed(problem, B, seed=seeds[0])
        set_table(s, par, xg, ug)
    o = types.SimpleNamespace(s=s, xr=None, ur=None, t0=t0, z0=z0, U=U,
                              u_min=u_min, u_max=u_max, q=None, qt=None,
                              r=None, problem=problem, dtype=dtype)
    if form in ("ref", "both"):
        o.xr, o.ur = reference_rows(problem, B, N + 1 if L is None else L,
                                    seed=seeds[1])
        set_ref(s, o.xr, o.ur, t0)
    if form in ("weights", "both"):
        o.q, o.qt, o.r, ops = weights(problem, B, seed=seeds[2], ops=ops)
        set_weights(s, o.q, o.qt, o.r)
    o.ops = fresh_ops(problem, B) if ops is None else ops
    return o


def oracle_rollouts(ops, z0, Uc, dtype, xr=None, ur=None, t0=0):
    """`shoot_util.oracle_rollouts` with step t under reference row
    min(t0 + t, L - 1) of its trajectory (`under_row`), the terminal step
    under row min(t0 + N, L - 1): (X [B][S][N+1][n], J [B][S]) in the given
    dtype.  Without a reference (xr None) the goals are ops[b]'s own."""
    o = orc.load(np_dtype(dtype))
    d = np_dtype(dtype)
    B, S, N, _ = Uc.shape
    n = z0.shape[1]
    X = np.empty((B, S, N + 1, n), d)
    J = np.zeros((B, S), d)
    for b in range(B):
        L = None if xr is None else xr.shape[1]
        for s in range(S):
            x = z0[b].astype(d)
            for t in range(N):
                if xr is not None:
                    under_row(ops[b], xr[b], ur[b], ref_row(L, t0, t))
                u = Uc[b, s, t].astype(d)
                X[b, s, t] = x
                J[b, s] += o.cost(ops[b], x, u)[0]
                x = o.dynamics(ops[b], x, u, jac=False)[0]
            X[b, s, N] = x
            if xr is not None:
                under_row(ops[b], xr[b], ur[b], ref_row(L, t0, N))
            J[b, s] += o.cost(ops[b], x, None, terminal=True)[0]
    return X, J


# ---- the entry points themselves ------------------------------------------------
def goal_lead(s, b0=0, ref=None, t0=None, wts=None, table="solver",
              form=None):
    """(suffix, leading arguments after the problem, the tensors to keep
    alive): the form by what the solver has set (or `form`), rows b0.. of the
    table, of the reference (`ref`: another device tensor [B][L][12]; `t0`:
    another first row) and of the weights (`wts`: another tensor)."""
    from pddp_amd import _native
    p = _native.ptr
    if form is None:
        form = "both" if s.reference is not None and \
            s.batch_weights is not None else \
            "ref" if s.reference is not None else "weights"
    tab = s.batch_table if isinstance(table, str) else table
    tab = None if tab is None else tab[b0:].contiguous()
    ref = (s.reference if ref is None else ref)
    wts = (s.batch_weights if wts is None else wts)
    keep = [tab]
    lead = (p(tab),)
    if form in ("ref", "both"):
        ref = ref[b0:].contiguous()
        keep.append(ref)
        lead += (p(ref), ref.shape[1], s.ref_start if t0 is None else t0)
    if form in ("weights", "both"):
        wts = wts[b0:].contiguous()
        keep.append(wts)
        lead += (p(wts),)
    suffix = {"ref": "_track", "weights": "_weighted",
              "both": "_track_weighted"}[form]
    return suffix, lead, keep


def shoot_call(s, S, std, smooth=0.0, seed=0, offset=0, active=None, b0=0,
               z0=None, U=None, rows=True, best=True, **goal):
    """pddp_shoot_{track,weighted,track_weighted}_* itself on trajectories
    b0.. (`shoot_util.shoot_call`'s conventions; `goal`: goal_lead's)."""
    from pddp_amd import _native
    B, N, n, m = s.B - b0, s.N, s.n, s.m
    opts = dict(dtype=s.dtype, device="cuda")
    z0 = (s.z0 if z0 is None else z0)[b0:].contiguous()
    U = (s.U if U is None else U)[b0:].contiguous()
    out = types.SimpleNamespace(
        J=torch.full((B, S), SENTINEL, **opts),
        best=torch.full((B,), -9, dtype=torch.int32, device="cuda"),
        J_best=torch.full((B,), SENTINEL, **opts) if best else None,
        Z=torch.full((B, N + 1, n), SENTINEL, **opts) if rows else None,
        U=torch.full((B, N, m), SENTINEL, **opts) if rows else None)
    p = _native.ptr
    a_std = std_vec(s, std)
    mask = None if active is None else active[b0:].contiguous()
    suffix, lead, keep = goal_lead(s, b0, **goal)
    _native.call("pddp_shoot" + suffix, s.dtype, ctypes.addressof(s.problem),
                 *lead, B, N, S, p(z0), p(U), p(s.u_min), p(s.u_max),
                 p(a_std), float(smooth), seed, offset, p(mask), p(out.J),
                 p(out.best), p(out.J_best), p(out.Z), p(out.U), s._s())
    torch.cuda.synchronize()
    return out


def mppi_call(s, S, std, lam, smooth=0.0, seed=0, offset=0, active=None, b0=0,
              z0=None, U=None, rows=True, W=True, **goal):
    """pddp_mppi_{track,weighted,track_weighted}_* itself
    (`mppi_util.mppi_call`'s conventions; `goal`: goal_lead's)."""
    from pddp_amd import _native
    B, N, n, m = s.B - b0, s.N, s.n, s.m
    opts = dict(dtype=s.dtype, device="cuda")
    z0 = (s.z0 if z0 is None else z0)[b0:].contiguous()
    U = (s.U if U is None else U)[b0:].contiguous()
    out = types.SimpleNamespace(
        J=torch.full((B, S), SENTINEL, **opts),
        best=torch.full((B,), -9, dtype=torch.int32, device="cuda"),
        J_best=torch.full((B,), SENTINEL, **opts),
        W=torch.full((B, S), SENTINEL, **opts) if W else None,
        J_w=torch.full((B,), SENTINEL, **opts),
        Z=torch.full((B, N + 1, n), SENTINEL, **opts) if rows else None,
        U=torch.full((B, N, m), SENTINEL, **opts) if rows else None)
    p = _native.ptr
    a_std = std_vec(s, std)
    lam_t = to_device(np.broadcast_to(np.asarray(lam, np.float64),
                                      (s.B,))[b0:].copy(), s.dtype)
    mask = None if active is None else active[b0:].contiguous()
    suffix, lead, keep = goal_lead(s, b0, **goal)
    _native.call("pddp_mppi" + suffix, s.dtype, ctypes.addressof(s.problem),
                 *lead, B, N, S, p(z0), p(U), p(s.u_min), p(s.u_max),
                 p(a_std), p(lam_t), float(smooth), seed, offset, p(mask),
                 p(out.J), p(out.best), p(out.J_best), p(out.W), p(out.J_w),
                 p(out.Z), p(out.U), s._s())
    torch.cuda.synchronize()
    return out


def trial_call(s, S, K, T, std, lam, smooth=0.0, seed=0, cand=0, stride=None,
               chunks=None, plant=None, dist=None, w_std=None, v_std=None,
               roll=0, step_offset=0, active=None, b0=0, z0=None, U=None,
               log_costs=True, logs=True, ref=None, t0=None, wts="solver"):
    """pddp_mppi_trial_goals_* itself (`mppi_trial_util.trial_call`'s
    conventions) with the solver's reference (or `ref`, read from row `t0`,
    default the solver's ref_start) and weights (`wts`: a tensor, or None for
    none), rows b0.. of each."""
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
    U_work = full(B, N, m)
    a_std = std_vec(s, std)
    lam_t = to_device(np.broadcast_to(np.asarray(lam, np.float64),
                                      (s.B,))[b0:].copy(), s.dtype)
    w_t = None if w_std is None else torch.full((n,), w_std, **opts)
    v_t = None if v_std is None else torch.full((n,), v_std, **opts)
    mask, table = tail(active), tail(s.batch_table)
    plant_t, dist_t = tail(plant), tail(dist)
    ref_t = tail(s.reference if ref is None else ref)
    wts_t = tail(s.batch_weights if isinstance(wts, str) else wts)
    window = (None, 0, 0) if ref_t is None else (
        p(ref_t), ref_t.shape[1], s.ref_start if t0 is None else t0)
    c0 = 0
    for count in chunks or [T]:
        _native.call(
            "pddp_mppi_trial_goals", s.dtype, ctypes.addressof(s.problem),
            p(table), p(plant_t), *window, p(wts_t), B, N, S, K, T, c0, count,
            p(out.z0), p(out.U), p(out.Z), p(U_work), p(s.u_min), p(s.u_max),
            p(a_std), p(lam_t), float(smooth), seed, cand,
            s.B * S if stride is None else stride, p(dist_t), p(w_t), p(v_t),
            roll, step_offset, p(out.x_true), p(mask), p(out.Jc),
            int(log_costs), p(out.X), p(out.Ulog), p(out.J), p(out.Y),
            p(out.J0), p(out.Jw), p(out.ess), p(out.plans), s._s())
        c0 += count
    torch.cuda.synchronize()
    assert c0 == T, "chunks %r do not add up to %d steps" % (chunks, T)
    return out


# ---- the whole trial --------------------------------------------------------
def chain_case(problem, B=5, N=6, T=3):
    """The inputs of the float64 whole-trial test, without a device (the seed
    of its candidates is searched on the CPU): make_solver's start with wide
    base actions, a reference of N + 4 rows read from row 2 on (the trial
    moves into the hold), weights, the plants' parameters of `perturbed(.,
    11)` and a disturbance."""
    from solver_util import mpc_inputs
    z0, _ = mpc_inputs(problem, B, N, False)
    m = orc.make_problem(problem, DT[problem]).action_size
    U = BOUND[problem] * np.random.RandomState(5).uniform(-0.8, 0.8,
                                                          (B, N, m))
    c = types.SimpleNamespace(z0=z0, U=U, t0=2, T=T,
                              u_min=np.full(m, -BOUND[problem]),
                              u_max=np.full(m, BOUND[problem]))
    c.xr, c.ur = reference_rows(problem, B, N + 4, seed=52)
    c.q, c.qt, c.r, c.ops = weights(problem, B, seed=53)
    c.par, _, _, c.log_ops = perturbed(problem, B, 11)
    c.dist = 0.01 * np.random.RandomState(3).randn(B, T, z0.shape[1])
    return c


def chain_lam(c, S, std, smooth, seed):
    """The spread (max - min per trajectory) of the first iteration's costs
    under the objective: the chain test's temperature."""
    Uc, _ = model_candidates(c.U, S, std, smooth, seed, 0, "f64", c.u_min,
                             c.u_max)
    _, J = oracle_rollouts(c.ops, c.z0, Uc, "f64", c.xr, c.ur, c.t0)
    return J.max(axis=1) - J.min(axis=1)


def chain_model(c, K, S, std, smooth, seed):
    return model_trial(c.ops, c.log_ops, c.z0, c.U, c.T, K, S, std,
                       chain_lam(c, S, std, smooth, seed), smooth, seed, 0,
                       c.u_min, c.u_max, c.xr, c.ur, c.t0, dist=c.dist,
                       w_std=0.02, v_std=0.01, roll=40, step_offset=2)

def model_trial(ops, log_ops, z0, U, T, K, S, std, lam, smooth, seed, cand,
                u_min, u_max, xr=None, ur=None, t0=0, dist=None, w_std=None,
                v_std=None, roll=0, step_offset=0, dtype="f64"):
    """`mppi_trial_util.model_trial` under the objective: control step c plans
    with `ops` (table parameters, weights' diagonals) under the window that
    starts at row min(t0 + c, L - 1); the applied step is logged with
    `log_ops` (the plant's parameters, the shared matrices) under that
    window's row 0, the terminal cost at c == T - 1 under its row 1.  `gap`:
    the smallest |J_w - J_0| / |J_0| the trial met."""
    o, d = orc.load(np_dtype(dtype)), np_dtype(dtype)
    B, N, m = U.shape
    n = z0.shape[1]
    L = None if xr is None else xr.shape[1]
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
        first = 0 if xr is None else ref_row(L, t0, c)
        for k in range(K):
            off = cand + (c * K + k) * B * S
            Uc, _ = model_candidates(U, S, std, smooth, seed, off, dtype,
                                     u_min, u_max)
            _, J = oracle_rollouts(ops, y, Uc, dtype, xr, ur, first)
            e = model_e(B, N, S, m, smooth, seed, off, dtype)
            _, Uw = model_update(U, J, lam, e, std, u_min, u_max)
            _, Jw = oracle_rollouts(ops, y, Uw[:, None], dtype, xr, ur, first)
            J0, Jw = J[:, 0].astype(np.float64), Jw[:, 0].astype(np.float64)
            took = np.isfinite(Jw) & (Jw <= J0)
            r.gap = min(r.gap, (np.abs(Jw - J0) / np.abs(J0)).min())
            r.J0[:, c, k], r.Jw[:, c, k], r.took[:, c, k] = J0, Jw, took
            U = np.where(took[:, None, None], Uw, U)
        r.plans[:, c] = U
        u = np.clip(U[:, 0], u_min, u_max)
        r.X[:, c], r.Ulog[:, c] = x, u
        xn = np.empty((B, n), d)
        for b in range(B):
            if xr is not None:
                under_row(log_ops[b], xr[b], ur[b], first)
            xb, ub = x[b].astype(d), u[b].astype(d)
            r.J[b] += o.cost(log_ops[b], xb, ub)[0]
            xn[b] = o.dynamics(log_ops[b], xb, ub, jac=False)[0]
        x = xn.astype(np.float64)
        if dist is not None:
            x = x + dist[:, c]
        if w_std is not None:
            x = x + w_std * w[:, c]
        y = x if v_std is None else x + v_std * v[:, c + 1]
        r.Y[:, c + 1] = y
        U = shift(U)
    r.X[:, T] = x
    for b in range(B):
        if xr is not None:
            under_row(log_ops[b], xr[b], ur[b], ref_row(L, t0, T))
        r.J[b] += o.cost(log_ops[b], x[b].astype(d), None, terminal=True)[0]
    r.z0, r.U, r.x_true = y, U, x
    Ucl = np.clip(U, u_min, u_max)
    r.Z = oracle_rollouts(ops, y, Ucl[:, None], dtype)[0][:, 0]
    return r
