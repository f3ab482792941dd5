"""What the tests of the cross-entropy refit share (tests/test_cem.py;
pddp_cem_*, csrc/cem.hip, ILQRSolver.cem): the numpy model of the law in
float64 - candidates with a width per time step and component over
`shoot_util`'s AR(1) values, the ranks of GIVEN costs, the refit of the mean
and the width to the elites of GIVEN ranks - and the entry points called
directly.  The oracle's rollouts are `shoot_util`'s.

pytest rewrites `assert` in test modules only: every assert here carries its
own message."""
import ctypes
import types

import numpy as np
import torch

from golden_util import np_dtype
from shoot_util import std_vec
from solver_util import SENTINEL, to_device


# ---- the numpy model of the law (include/pddp_hip.h) ------------------------
def model_candidates(U, sigma, e, u_min=None, u_max=None):
    """(Uc [B][S][N][m], hit [B][S][N][m]): the applied actions of every
    candidate in float64 - u = clip(U[b][t] + sigma[b][t] e[b][t][s]),
    candidate 0 the mean itself - and where the clamp changed one."""
    U = np.asarray(U, np.float64)
    sigma = np.asarray(sigma, np.float64)
    raw = U[:, :, None, :] + sigma[:, :, None, :] * e   # [B][N][S][m]
    raw[:, :, 0, :] = U
    raw = raw.transpose(0, 2, 1, 3)
    Uc = raw if u_min is None else np.clip(raw, u_min, u_max)
    return np.ascontiguousarray(Uc), Uc != raw


def model_rank(J, K):
    """(rank [B][S] int32, best [B] int32, n_elite [B] int32) of given costs:
    the rank of a finite cost is the number of finite (J, s') lexicographically
    below (J, s), of another one -1; best the s of rank 0 or -1; n_elite =
    min(K, finite costs)."""
    J = np.asarray(J)
    B, S = J.shape
    rank = np.full((B, S), -1, np.int32)
    best = np.full(B, -1, np.int32)
    for b in range(B):
        f = np.flatnonzero(np.isfinite(J[b]))
        order = f[np.lexsort((f, J[b, f]))]   # by J, then by s
        rank[b, order] = np.arange(len(order))
        if len(order):
            best[b] = order[0]
    n_elite = np.minimum(K, (rank >= 0).sum(axis=1)).astype(np.int32)
    return rank, best, n_elite


def model_refit(U, sigma, e, rank, K, mix, dtype, std_min=None, u_min=None,
                u_max=None):
    """(Um [B][N][m], Sm [B][N][m], V [B][N][m]) in float64: the mean and the
    width refitted to the elites (0 <= rank < K) of given ranks.  Candidate 0
    counts in Ke and adds nothing to the sums; step = 1 - mix rounded to the
    run's type as the entry point rounds it; rows without a finite cost NaN."""
    U = np.asarray(U, np.float64)
    sigma = np.asarray(sigma, np.float64)
    B, N, m = U.shape
    step = float(np_dtype(dtype)(1.0 - float(mix)))
    floor = np.zeros(m) if std_min is None else np.broadcast_to(
        np.asarray(std_min, np.float64), (m,))
    Um, Sm, V = (np.full((B, N, m), np.nan) for _ in range(3))
    for b in range(B):
        elite = (rank[b] >= 0) & (rank[b] < K)
        Ke = int(elite.sum())
        if Ke == 0:
            continue
        elite[0] = False
        es = e[b][:, elite]                       # [N][elites s >= 1][m]
        ebar = es.sum(axis=1) / Ke
        V[b] = np.maximum((es * es).sum(axis=1) / Ke - ebar * ebar, 0.0) \
            if Ke > 1 else 0.0
        raw = U[b] + step * sigma[b] * ebar
        Um[b] = raw if u_min is None else np.clip(raw, u_min, u_max)
        sd = sigma[b] * np.sqrt(V[b])
        Sm[b] = np.maximum(sigma[b] + step * (sd - sigma[b]), floor)
    return Um, Sm, V


def random_sigma(problem, B, N, m, seed, dtype, lo=0.1, hi=0.5):
    """[B][N][m] float64 of the run's type's values: BOUND U(lo, hi), another
    width for every row and component."""
    from solver_util import BOUND
    rng = np.random.RandomState(seed)
    return (BOUND[problem] * rng.uniform(lo, hi, (B, N, m))).astype(
        np_dtype(dtype)).astype(np.float64)


# ---- the entry points themselves --------------------------------------------
ROWS = ("J", "rank", "best", "J_best", "n_elite", "J_m", "Z", "U", "S")
FILL = {"rank": -9, "best": -9, "n_elite": -9}


def cem_call(s, S, K, sigma, smooth=0.0, mix=0.0, seed=0, offset=0,
             std_min=None, active=None, b0=0, z0=None, U=None, rows=True,
             ranks=True, bounded=True):
    """pddp_cem[_batch]_* itself on trajectories b0.. of the solver's z0 and U
    (or the device tensors given, all B trajectories'), with the solver's
    table if one is set; sigma: a float, [m] or [B][N][m] numpy or device
    tensor, all B trajectories'; every output pre-filled with SENTINEL (the
    int32 ones: -9)."""
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
        J_best=torch.full((B,), SENTINEL, **opts),
        n_elite=torch.full((B,), -9, **iopt),
        J_m=torch.full((B,), SENTINEL, **opts),
        Z=torch.full((B, N + 1, n), SENTINEL, **opts) if rows else None,
        U=torch.full((B, N, m), SENTINEL, **opts) if rows else None,
        S=torch.full((B, N, m), SENTINEL, **opts) if rows else None)
    p = _native.ptr
    # (every tensor the launch reads is held by a name until it has run)
    floor = None if std_min is None else std_vec(s, std_min)
    mask = None if active is None else active[b0:].contiguous()
    table = None if s.batch_table is None else s.batch_table[b0:].contiguous()
    name, lead = "pddp_cem", (ctypes.addressof(s.problem),)
    if table is not None:
        name, lead = name + "_batch", lead + (p(table),)
    _native.call(name, s.dtype, *lead, B, N, S, K, p(z0), p(U),
                 p(s.u_min if bounded else None),
                 p(s.u_max if bounded else None), p(sg), p(floor),
                 float(smooth), float(mix), seed, offset, p(mask), p(out.J),
                 p(out.rank), p(out.best), p(out.J_best), p(out.n_elite),
                 p(out.J_m), p(out.Z), p(out.U), p(out.S), s._s())
    torch.cuda.synchronize()
    return out


def host_inputs(problem, dtype, B, N, wide=True):
    """(z0, U) of `mppi_util.wide_solver` without a device, in the run's
    type: for the searches on the CPU that the test module notes."""
    from solver_util import BOUND, mpc_inputs
    z0, U = mpc_inputs(problem, B, N, False)
    if wide:
        U = BOUND[problem] * np.random.RandomState(5).uniform(-0.8, 0.8,
                                                             U.shape)
    d = np_dtype(dtype)
    return z0.astype(d), U.astype(d)
