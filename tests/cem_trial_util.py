"""What the tests of the one-launch CEM trial share (tests/test_cem_trial.py;
pddp_cem_trial_*, csrc/cem_trial.hip, ILQRSolver.cem_closed_loop): the entry
point called directly - in one launch or in several, on all trajectories or on
a tail of them - and the numpy / oracle model of a trial in the run's type:
`cem_util`'s candidates, ranks and refit, `shoot_util`'s rollouts,
`mppi_trial_util`'s plant step, normals and shift.

pytest rewrites `assert` in test modules only: every assert here carries its
own message."""
import ctypes
import types

import numpy as np
import torch

from cem_util import model_candidates, model_rank, model_refit
from mppi_trial_util import noise_rows, plant_step, shift, terminal_cost
from mppi_util import model_e
from shoot_util import oracle_rollouts, std_vec
from solver_util import SENTINEL, to_device

# every output and log of a launch, in the order the tests compare them
NAMES = ("z0", "U", "sigma", "Z", "X", "Ulog", "J", "Jtrace", "Jm", "nelite",
         "plans", "stds", "Jc")
OPTIONAL = ("Jtrace", "Jm", "nelite", "plans", "stds")


def trial_call(s, S, K, I, T, sigma, smooth=0.0, mix=0.0, seed=0, cand=0,
               stride=None, chunks=None, keep_std=False, std_min=None,
               plant=None, dist=None, w_std=None, v_std=None, roll=0,
               step_offset=0, active=None, b0=0, z0=None, U=None,
               log_costs=True, logs=True, bounded=True):
    """pddp_cem_trial_* itself on trajectories b0.. of the solver's z0 and U
    (or of the device tensors given, all B trajectories'), with the solver's
    table if one is set: control steps 0 .. T-1 in the launches of `chunks`
    (counts; default one launch), every launch on the buffers the one before
    left - the work buffers filled with SENTINEL again before each, they carry
    nothing.  sigma: a float, [m] or [B][N][m] numpy or device tensor, all B
    trajectories'; it is the call's `sigma` and, without `keep_std`, its
    `sigma0` too.  `stride`, `cand`, `roll`, plant, dist, w_std, v_std: as
    mppi_trial_util.trial_call.  Every output pre-filled with SENTINEL (the
    int32 one: -9); `out.work`: the four work buffers after the last launch."""
    from pddp_amd import _native
    B, N, n, m = s.B - b0, s.N, s.n, s.m
    opts = dict(dtype=s.dtype, device="cuda")

    def full(*shape):
        return torch.full(shape, SENTINEL, **opts)

    def tail(t):
        return None if t is None else t[b0:].contiguous()

    if torch.is_tensor(sigma):
        sg = sigma.to(**opts)[b0:].clone().contiguous()
    else:
        sg = to_device(np.broadcast_to(np.asarray(sigma, np.float64),
                                       (s.B, N, m))[b0:].copy(), s.dtype)
    out = types.SimpleNamespace(
        z0=(s.z0 if z0 is None else z0)[b0:].clone().contiguous(),
        U=(s.U if U is None else U)[b0:].clone().contiguous(), sigma=sg,
        Z=full(B, N + 1, n), X=full(B, T + 1, n), Ulog=full(B, T, m),
        J=full(B), Y=None, x_true=None,
        Jtrace=full(B, T, I + 1) if logs else None,
        Jm=full(B, T, I) if logs else None,
        nelite=torch.full((B, T, I), -9, dtype=torch.int32, device="cuda")
        if logs else None,
        plans=full(B, T, N, m) if logs else None,
        stds=full(B, T, N, m) if logs else None,
        Jc=full(B, T, I, S) if log_costs else full(B, S))
    if v_std is not None:
        out.x_true = out.z0.clone()
        out.Y = full(B, T + 1, n)
        out.Y[:, 0] = out.z0
    p = _native.ptr
    # (every tensor the launches read is held by a name until they have run)
    sigma0 = None if keep_std else sg.clone()
    floor = None if std_min is None else std_vec(s, std_min)
    w_t = None if w_std is None else torch.full((n,), w_std, **opts)
    v_t = None if v_std is None else torch.full((n,), v_std, **opts)
    mask, table = tail(active), tail(s.batch_table)
    plant_t, dist_t = tail(plant), tail(dist)
    t0 = 0
    for count in chunks or [T]:
        out.work = [full(B, N, m) for _ in range(4)]
        _native.call(
            "pddp_cem_trial", s.dtype, ctypes.addressof(s.problem), p(table),
            p(plant_t), B, N, S, K, I, T, t0, count, p(out.z0), p(out.U),
            p(out.Z), *[p(w) for w in out.work],
            p(s.u_min if bounded else None), p(s.u_max if bounded else None),
            p(out.sigma), p(sigma0), p(floor), float(smooth), float(mix), seed,
            cand, s.B * S if stride is None else stride, p(dist_t), p(w_t),
            p(v_t), roll, step_offset, p(out.x_true), p(mask), p(out.Jc),
            int(log_costs), p(out.X), p(out.Ulog), p(out.J), p(out.Y),
            p(out.Jtrace), p(out.Jm), p(out.nelite), p(out.plans),
            p(out.stds), s._s())
        t0 += count
    torch.cuda.synchronize()
    assert t0 == T, "chunks %r do not add up to %d steps" % (chunks, T)
    return out


def trial_names(out):
    """The names of `out` that hold a tensor: NAMES, and Y / x_true under
    measurement noise."""
    return [nm for nm in NAMES + ("Y", "x_true")
            if getattr(out, nm) is not None]


def selects(Jtrace, Jm, nelite):
    """(better, moved) [B][T][I] bool of a trial's logs (numpy): the law's two
    selects, `better` from J_m against the incumbent's cost BEFORE the
    iteration."""
    better = np.isfinite(Jm) & (Jm <= Jtrace[..., :-1])
    return better, nelite > 0


def cut_gap(J, K):
    """The smallest relative cost gap at the elite cut over the rows of J
    [B][S]: between the last elite and the first finite cost behind it (inf
    where every finite cost is an elite)."""
    gap = np.inf
    for row in np.asarray(J, np.float64):
        f = np.sort(row[np.isfinite(row)])
        if len(f) > K:
            gap = min(gap, (f[K] - f[K - 1]) / abs(f[K - 1]))
    return gap


# ---- the whole trial --------------------------------------------------------
def oracle_costs(ops, dtype):
    """costs(y, Uc [B][S][N][m]) -> J [B][S] float64 of the oracle's rollouts
    in the run's type."""
    def costs(y, Uc):
        return oracle_rollouts(ops, y, Uc, dtype)[1].astype(np.float64)
    return costs


def model_trial(costs, plant_ops, z0, U, sigma, T, K, I, S, smooth, mix, seed,
                cand, u_min, u_max, std_min=None, keep_std=False, dist=None,
                w_std=None, v_std=None, roll=0, step_offset=0, dtype="f64",
                min_gap=None, plant=None):
    """The trial from GIVEN costs (`costs(y, Uc) -> J [B][S]` float64, e.g.
    `oracle_costs`): candidates -> costs -> `model_rank` -> `model_refit` ->
    the cost of the refitted mean -> better / moved -> plant step, in float64
    on draws of the run's type.  sigma [B][N][m].  `plant(x, u) -> (x', l)`
    and its terminal cost default to the oracle's under `plant_ops`
    (`plant=(step, terminal)` replaces both).  Returns the logs under
    trial_call's names (the true start is z0, and so is the first
    observation), `better`, `moved`, and the two gaps at the chain's only
    discontinuities: `gap_inc`, the smallest |J_m - J_inc| / |J_inc| over the
    iterations with a finite J_m and J_inc, and `gap_cut`, the smallest
    `cut_gap`.  `min_gap`: both are asserted to exceed it."""
    B, N, m = U.shape
    n = z0.shape[1]
    U = np.asarray(U, np.float64).copy()
    sigma0 = np.asarray(sigma, np.float64).copy()
    sigma = sigma0.copy()
    step_fn, term_fn = plant or (
        lambda x, u: plant_step(plant_ops, x, u, dtype),
        lambda x: terminal_cost(plant_ops, x, dtype))
    x, y = (np.asarray(z0, np.float64).copy() for _ in range(2))
    w = noise_rows(B, T, n, 0, seed, roll, step_offset, dtype)
    v = noise_rows(B, T, n, 1, seed, roll, step_offset, dtype)
    r = types.SimpleNamespace(
        X=np.empty((B, T + 1, n)), Ulog=np.empty((B, T, m)), J=np.zeros(B),
        Y=np.empty((B, T + 1, n)), Jtrace=np.empty((B, T, I + 1)),
        Jm=np.empty((B, T, I)), nelite=np.empty((B, T, I), np.int32),
        better=np.empty((B, T, I), bool), moved=np.empty((B, T, I), bool),
        plans=np.empty((B, T, N, m)), stds=np.empty((B, T, N, m)),
        Jc=np.empty((B, T, I, S)), gap_inc=np.inf, gap_cut=np.inf)
    r.Y[:, 0] = y
    for c in range(T):
        mean, width, inc = U.copy(), sigma.copy(), U.copy()
        for k in range(I):
            off = cand + (c * I + k) * B * S
            e = model_e(B, N, S, m, smooth, seed, off, dtype)
            Uc, _ = model_candidates(mean, width, e, u_min, u_max)
            J = costs(y, Uc)
            rank, _, Ke = model_rank(J, K)
            Um, Sm, _ = model_refit(mean, width, e, rank, K, mix, dtype,
                                    std_min, u_min, u_max)
            moved = Ke > 0
            Um = np.where(moved[:, None, None], Um, mean)  # (no NaN rollouts)
            Jm = np.where(moved, costs(y, Um[:, None])[:, 0], np.inf)
            if k == 0:
                Jinc = J[:, 0].copy()
                r.Jtrace[:, c, 0] = Jinc
            better = np.isfinite(Jm) & (Jm <= Jinc)
            fin = np.isfinite(Jm) & np.isfinite(Jinc)
            if fin.any():
                r.gap_inc = min(r.gap_inc, (np.abs(Jm[fin] - Jinc[fin]) /
                                            np.abs(Jinc[fin])).min())
            r.gap_cut = min(r.gap_cut, cut_gap(J, K))
            inc = np.where(better[:, None, None], Um, inc)
            Jinc = np.where(better, Jm, Jinc)
            mean = np.where(moved[:, None, None], Um, mean)
            width = np.where(moved[:, None, None], Sm, width)
            r.Jc[:, c, k], r.Jm[:, c, k], r.nelite[:, c, k] = J, Jm, Ke
            r.better[:, c, k], r.moved[:, c, k] = better, moved
            r.Jtrace[:, c, k + 1] = Jinc
        r.plans[:, c], r.stds[:, c] = inc, width
        u = inc[:, 0] if u_min is None else np.clip(inc[:, 0], u_min, u_max)
        r.X[:, c], r.Ulog[:, c] = x, u
        xn, cost = step_fn(x, u)
        r.J += cost
        x = np.asarray(xn, np.float64)
        if dist is not None:
            x = x + dist[:, c]
        if w_std is not None:
            x = x + w_std * w[:, c]
        y = x if v_std is None else x + v_std * v[:, c + 1]
        r.Y[:, c + 1] = y
        U = shift(inc)
        sigma = shift(width) if keep_std else sigma0.copy()
    r.X[:, T] = x
    r.J += term_fn(x)
    r.z0, r.U, r.sigma, r.x_true = y, U, sigma, x
    if min_gap is not None:
        assert r.gap_inc > min_gap, \
            "|J_m - J_inc| / |J_inc| as small as %g" % r.gap_inc
        assert r.gap_cut > min_gap, \
            "a cost gap at the elite cut as small as %g" % r.gap_cut
    return r


def model_Z(ops, r, u_min, u_max, dtype):
    """Z [B][N+1][n] of a model trial: the oracle's rollout of clip(U) from
    z0."""
    Uc = r.U if u_min is None else np.clip(r.U, u_min, u_max)
    return oracle_rollouts(ops, r.z0, Uc[:, None], dtype)[0][:, 0]
