"""Sampled shooting with a cross-entropy (CEM) refit on the device
(pddp_cem_*, pddp_cem_batch_*, csrc/cem.hip, ILQRSolver.cem).

include/pddp_hip.h is the definition.  As in tests/test_mppi.py each stage is
held against a model fed with the DEVICE's previous stage, so a cost error can
neither flip an elite and fail a right kernel nor hide a wrong one: the costs
against the CPU oracle along `cem_util`'s candidates; the ranks EXACTLY against
the model's ranking of the device's own costs; the refitted mean and width
against the float64 refit of the model's AR(1) values under the device's own
ranks; the mean's rollout against the oracle stepped along the device's own
actions."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from abi_util import assert_entry_points, caller, cartpole_pointers
from cem_util import (ROWS, cem_call, model_candidates, model_rank,
                      model_refit, random_sigma)
from golden_util import rel_err
from mppi_util import model_e, wide_solver
from shoot_util import oracle_rollouts, shoot_call
from solver_util import (BOUND, CONTROLLER, PROBLEMS, REARMED, SENTINEL,
                         record_tol)

gpu = pytest.mark.gpu
SYMBOLS = ["pddp_cem_f32", "pddp_cem_f64", "pddp_cem_batch_f32",
           "pddp_cem_batch_f64"]
B, N = 3, 12
# The seeds of the refit tests with K >= 8, searched on the CPU (seeds 1, 2,
# ... in turn, the first that holds) with the ORACLE's costs along the model's
# candidates under `_case`'s widths, so that every entry of the model's V is
# >= 0.03 - a margin over the 0.01 the tests assert under the device's own
# ranks: seed 1 holds for all 32 cases of the grid (S = 12, K = 8, B = 3; the
# smallest V is 0.0515), and for cartpole at S = 70 (0.078), S = 300 (0.071)
# and rendezvous at S = 70 (0.147), B = 2, both types.
GRID_SEED = WIDE_SEED = 1
V_FLOOR = 0.01
# The width of the overflow case, searched on the CPU with the float32 oracle
# (cartpole, unbounded, S = 70, smooth = 0.7, seed 31, make_solver's inputs):
# at 100 the costs of 22, 18 and 22 candidates of the three trajectories are
# not finite; at 1000, 68, 67 and 68; at 10000 all but the mean's.
OVERFLOW_WIDTH, OVERFLOW_SEED = 100.0, 31


# ---- CPU -------------------------------------------------------------------
def test_cem_entry_points_are_declared_exported_and_bound():
    """CPU: the four symbols in the header, the built library,
    exported_symbols() and _native._SIGS; where the four ints (B, N, S, K),
    the two doubles (smooth, mix, after the six input pointers z0, U, u_min,
    u_max, sigma, std_min) and the two 64-bit integers sit; the ABI version
    as it was."""
    from pddp_amd import _native
    assert_entry_points(SYMBOLS)
    want = {"pddp_cem": (26, 1), "pddp_cem_batch": (27, 2)}
    for name, (count, at) in want.items():
        sig = _native._SIGS[name]
        assert len(sig) == count, name
        assert [i for i, c in enumerate(sig) if c is ctypes.c_int] == \
            [at, at + 1, at + 2, at + 3], name
        assert [i for i, c in enumerate(sig) if c is ctypes.c_double] == \
            [at + 10, at + 11], name
        assert [i for i, c in enumerate(sig) if c is ctypes.c_uint64] == \
            [at + 12, at + 13], name
    assert _native.lib().pddp_hip_abi_version() == 1


def test_cem_entry_points_refuse_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call), both dtypes, both forms.  PDDP_E_BADARG: pddp_shoot_*'s list with
    sigma in a_std's place - each null required pointer, B, N, S of 0 and
    negative, B S > 0x7fffffff, smooth of 1.0, -0.1 and NaN, a NULL table on
    _batch - and a NULL n_elite, a NULL J_m, K of 0, -1 and S + 1, mix of 1.0,
    -0.1 and NaN, every way of giving some but not all of Z_out / U_out /
    S_out, U_out == U, S_out == sigma, Z_out == z0, S = 257 without rows;
    PDDP_E_UNSUPPORTED: a DEFAULT-encoding problem.  The non-null pointers are
    host words nobody reads (q and r: two of them, for the aliasing tests)."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    r = q + 8
    lib = _native.lib()
    for t in ("f32", "f64"):
        #       0  1  2  3  4   5  6     7     8      9        10      11
        #       B  N  S  K  z0  U  umin  umax  sigma  std_min  smooth  mix
        good = [2, 3, 4, 2, q, q, None, None, q, None, 0.5, 0.25,
                #  12    13   14   15  16    17    18      19       20
                #  seed  off  act  Jc  rank  best  J_best  n_elite  J_m
                7, 0, None, q, q, q, q, q, q,
                #  21     22     23
                #  Z_out  U_out  S_out
                r, r, r]
        plain = caller(getattr(lib, "pddp_cem_" + t), good)
        batch = caller(getattr(lib, "pddp_cem_batch_" + t), good)
        forms = ((plain, (pp,), (ppd,), (None,)),
                 (batch, (pp, q), (ppd, q), (None, q)))
        for call, ok, gaussian, no_problem in forms:
            for i in (4, 5, 8, 15, 17, 19, 20):        # required pointers
                assert call(*ok, **{"_%d" % i: None}) == -1, (t, i)
            assert call(*no_problem) == -1, t
            for i in (0, 1, 2):                        # B, N, S
                assert call(*ok, **{"_%d" % i: 0}) == -1, (t, i)
                assert call(*ok, **{"_%d" % i: -3}) == -1, (t, i)
            assert call(*ok, _0=1 << 16, _2=1 << 15) == -1, t   # B S = 2^31
            for K in (0, -1, 5):                       # K < 1, K > S
                assert call(*ok, _3=K) == -1, (t, K)
            for some in ((21,), (22,), (23,), (21, 22), (21, 23), (22, 23)):
                assert call(*ok, **{"_%d" % i: None for i in some}) == -1, \
                    (t, some)
            assert call(*ok, _22=q) == -1, t           # U_out == U
            assert call(*ok, _23=q) == -1, t           # S_out == sigma
            assert call(*ok, _4=r) == -1, t            # Z_out == z0
            assert call(*ok, _2=257, _21=None, _22=None, _23=None) == -1, t
            for smooth in (1.0, -0.1, float("nan")):
                assert call(*ok, _10=smooth) == -1, (t, smooth)
            for mix in (1.0, -0.1, float("nan")):
                assert call(*ok, _11=mix) == -1, (t, mix)
            assert call(*gaussian) == _native.E_UNSUPPORTED, t
            assert call(*gaussian, _9=q, _16=None, _18=None, _21=None,
                        _22=None, _23=None) == _native.E_UNSUPPORTED, t
        assert batch(pp, None) == -1, t                # no table


def test_numpy_model_of_the_refit():
    """CPU: the model itself.  K = S with equal costs: ebar is the sum of e
    over s >= 1 divided by S (the mean counts and adds nothing) and V the
    second moment about it; K = 1: V = 0 and Sm = max(sigma + step (0 -
    sigma), std_min), Um the clamped mean where the elite is candidate 0;
    ranks with ties (to the lower s) and with entries that are not finite;
    mix and std_min."""
    rng = np.random.RandomState(4)
    U = rng.randn(2, 6, 2)
    sigma = rng.uniform(0.5, 1.5, (2, 6, 2))
    for dtype in ("f32", "f64"):
        S = 4
        e = model_e(2, 6, S, 2, 0.7, 9, 0, dtype)
        rank, best, ne = model_rank(np.full((2, S), 7.0), S)
        assert (rank == np.arange(S)).all() and (best == 0).all()
        assert (ne == S).all()
        Um, Sm, V = model_refit(U, sigma, e, rank, S, 0.0, dtype)
        ebar = e[:, :, 1:].sum(axis=2) / S
        assert np.abs(Um - (U + sigma * ebar)).max() < 1e-14, dtype
        var = (e[:, :, 1:] ** 2).sum(axis=2) / S - ebar ** 2
        assert np.abs(V - var).max() < 1e-14 and (V > 0).all(), dtype
        assert np.abs(Sm - sigma * np.sqrt(var)).max() < 1e-14, dtype
        # the clamp; mix = 0.5 halves the step of both; the floor
        Uc, _, _ = model_refit(U, sigma, e, rank, S, 0.0, dtype, None, -1.0,
                               1.0)
        assert (Uc == np.clip(Um, -1.0, 1.0)).all() and (Uc != Um).any()
        Uh, Sh, _ = model_refit(U, sigma, e, rank, S, 0.5, dtype)
        assert np.abs(Uh - (U + 0.5 * sigma * ebar)).max() < 1e-14, dtype
        assert np.abs(Sh - 0.5 * (sigma + Sm)).max() < 1e-14, dtype
        _, Sf, _ = model_refit(U, sigma, e, rank, S, 0.0, dtype, [0.0, 50.0])
        assert (Sf[:, :, 0] == Sm[:, :, 0]).all(), dtype
        assert (Sf[:, :, 1] == 50.0).all(), dtype
        # K = 1: the elite is candidate 2, then candidate 0
        J = np.array([[3.0, 2.0, 1.0, 5.0], [1.0, 2.0, 3.0, 4.0]])
        rank, best, ne = model_rank(J, 1)
        assert best.tolist() == [2, 0] and ne.tolist() == [1, 1]
        Um, Sm, V = model_refit(U, sigma, e, rank, 1, 0.25, dtype, 0.3,
                                -1.0, 1.0)
        assert (V == 0).all(), dtype
        assert np.abs(Sm - np.maximum(0.25 * sigma, 0.3)).max() < 1e-15, dtype
        want0 = np.clip(U[0] + 0.75 * sigma[0] * e[0][:, 2], -1.0, 1.0)
        assert np.abs(Um[0] - want0).max() < 1e-15, dtype
        assert (Um[1] == np.clip(U[1], -1.0, 1.0)).all(), dtype
    # ties go to the lower s; what is not finite has no rank and is no elite
    J = np.array([[1.0, np.inf, 1.0, np.nan, 0.5, -np.inf, 1.0],
                  [np.nan] * 7, [2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])
    rank, best, ne = model_rank(J, 3)
    assert rank[0].tolist() == [1, -1, 2, -1, 0, -1, 3]
    assert (rank[1] == -1).all() and (rank[2] == np.arange(7)).all()
    assert best.tolist() == [4, -1, 0] and ne.tolist() == [3, 0, 3]
    assert model_rank(J, 7)[2].tolist() == [4, 0, 7]
    e = model_e(3, 6, 7, 2, 0.0, 9, 0, "f64")
    U3, s3 = rng.randn(3, 6, 2), rng.uniform(0.5, 1.5, (3, 6, 2))
    Um, Sm, V = model_refit(U3, s3, e, rank, 3, 0.0, "f64")
    assert np.isnan(Um[1]).all() and np.isnan(Sm[1]).all()
    # (row 0: elites 4, 0, 2 - candidate 0 counts in Ke = 3 and adds nothing)
    ebar = (e[0][:, 4] + e[0][:, 2]) / 3
    assert np.abs(Um[0] - (U3[0] + s3[0] * ebar)).max() < 1e-15


# ---- GPU: what the tests share ------------------------------------------------
def _np(t):
    return t.cpu().numpy()


def _floor(problem, m):
    """std_min [m]: another floor for every component."""
    return 0.02 * BOUND[problem] * (1.0 + np.arange(m))


@functools.lru_cache(maxsize=None)
def _case(problem, dtype, smooth, table, S=12, K=8, B_=B, seed=GRID_SEED,
          mix=0.25):
    """One launch and its references, shared by the stage tests: a random
    positive width per row, step and component, the oracle's costs along the
    model's candidates, the device's outputs."""
    s, ops, z0, U, u_min, u_max = wide_solver(problem, dtype, B_, N,
                                              table=table)
    sigma = random_sigma(problem, B_, N, s.m, 13, dtype)
    floor = _floor(problem, s.m)
    e = model_e(B_, N, S, s.m, smooth, seed, 0, dtype)
    Uc, hit = model_candidates(U, sigma, e, u_min, u_max)
    _, J = oracle_rollouts(ops, z0, Uc, dtype)
    out = cem_call(s, S, K, sigma, smooth, mix, seed, std_min=floor)
    return types.SimpleNamespace(
        s=s, ops=ops, z0=z0, U=U, u_min=u_min, u_max=u_max, dtype=dtype, S=S,
        K=K, sigma=sigma, floor=floor, smooth=smooth, mix=mix, seed=seed,
        hit=hit, J_orc=J, out=out, e=e,
        tag=(problem, dtype, smooth, table, S, K))


def _check_costs(c):
    """Stage 1: Jc against the oracle within record_tol."""
    J = _np(c.out.J)
    for b in range(J.shape[0]):
        e = rel_err(J[b], c.J_orc[b])
        print(c.tag, b, "J off by", e)
        assert e < record_tol(c.dtype), (c.tag, b, e)


def _check_ranks(out, K, tag):
    """Stage 2: rank, best, J_best and n_elite EXACTLY against the model's
    ranking of the device's own costs."""
    J = _np(out.J)
    rank, best, n_elite = model_rank(J, K)
    assert (_np(out.rank) == rank).all(), (tag, _np(out.rank), rank)
    assert (_np(out.best) == best).all(), (tag, _np(out.best), best)
    assert (_np(out.n_elite) == n_elite).all(), (tag, out.n_elite, n_elite)
    for b in range(J.shape[0]):
        want = J[b, best[b]] if best[b] >= 0 else J.dtype.type(np.inf)
        assert _np(out.J_best[b]).tobytes() == want.tobytes(), (tag, b)
    return rank


def _check_refit(c):
    """Stage 3: U_out and S_out against the float64 refit of the model's e
    under the device's own ranks, rel_err within record_tol; with K >= 8
    every entry of the model's V is at least V_FLOOR (none is excluded)."""
    Um, Sm, V = model_refit(c.U, c.sigma, c.e, _np(c.out.rank), c.K, c.mix,
                            c.dtype, c.floor, c.u_min, c.u_max)
    print(c.tag, "smallest V", V.min())
    if c.K >= 8:
        assert V.min() >= V_FLOOR, (c.tag, V.min())
    else:
        assert c.K == 1 and (V == 0).all(), c.tag
    Ud, Sd = _np(c.out.U), _np(c.out.S)
    for b in range(Ud.shape[0]):
        e = (rel_err(Ud[b], Um[b]), rel_err(Sd[b], Sm[b]))
        print(c.tag, b, "U_out, S_out off by", e)
        assert max(e) < record_tol(c.dtype), (c.tag, b, e)


def _check_rollout(c):
    """Stage 4: Z_out and J_m against the oracle stepped along the device's
    own U_out."""
    Ud = _np(c.out.U)
    X, J = oracle_rollouts(c.ops, c.z0, Ud[:, None], c.dtype)
    for b in range(Ud.shape[0]):
        e = (rel_err(_np(c.out.Z[b]), X[b, 0]),
             rel_err(_np(c.out.J_m[b]), J[b, 0]))
        print(c.tag, b, "Z_out, J_m off by", e)
        assert max(e) < record_tol(c.dtype), (c.tag, b, e)


_cases = [pytest.mark.parametrize("table", [False, True],
                                  ids=["shared", "table"]),
          pytest.mark.parametrize("smooth", [0.0, 0.7]),
          pytest.mark.parametrize("dtype", ["f64", "f32"]),
          pytest.mark.parametrize("problem", PROBLEMS)]


def _all_cases(fn):
    for mark in _cases:
        fn = mark(fn)
    return gpu(fn)


# ---- GPU -------------------------------------------------------------------
@_all_cases
def test_costs_vs_oracle(problem, dtype, smooth, table):
    """B = 3, N = 12, S = 12, K = 8, bounded, sigma = BOUND U(0.1, 0.5) per
    row, step and component (a wrong row or component index shows) around
    base actions spread over 0.8 BOUND: the clamp is met on some steps and
    not on others (asserted from the model).  J within record_tol of the
    oracle along the model's candidates - tests/test_shoot.py's bars."""
    c = _case(problem, dtype, smooth, table)
    assert c.hit[:, 1:].any() and not c.hit[:, 1:].all(), c.hit.mean()
    _check_costs(c)


@_all_cases
def test_ranks_of_device_costs(problem, dtype, smooth, table):
    c = _case(problem, dtype, smooth, table)
    _check_ranks(c.out, c.K, c.tag)
    assert bool((c.out.J_best <= c.out.J[:, 0]).all())


@_all_cases
def test_refit_vs_model_under_device_ranks(problem, dtype, smooth, table):
    """mix = 0.25, std_min = 0.02 BOUND (1 + j)."""
    _check_refit(_case(problem, dtype, smooth, table))


@_all_cases
def test_mean_rollout_vs_oracle(problem, dtype, smooth, table):
    _check_rollout(_case(problem, dtype, smooth, table))


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [1, 5, 70, 300])
def test_ranks_exact(S, dtype):
    """Cartpole, B = 2.  S = 1: one lane; 5: part of a wavefront, several
    trajectories to it; 70: two wavefronts; 300: two turns per lane.  K = 1,
    8 (where S >= 8) and S: rank, best, J_best and n_elite exactly the
    model's on the device's own costs, with and without the rank output."""
    s, _, _, _, _, _ = wide_solver("cartpole", dtype, 2, N)
    sigma = random_sigma("cartpole", 2, N, s.m, 13, dtype)
    for K in sorted({1, 8, S} if S >= 8 else {1, S}):
        out = cem_call(s, S, K, sigma, 0.7, 0.0, 22)
        rank = _check_ranks(out, K, (dtype, S, K))
        assert (np.sort(rank, axis=1) == np.arange(S)).all(), (S, K)
        lean = cem_call(s, S, K, sigma, 0.7, 0.0, 22, ranks=False)
        for nm in ROWS:
            if nm != "rank":
                assert torch.equal(getattr(lean, nm), getattr(out, nm)), nm


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("K", [8, 1])
@pytest.mark.parametrize("problem,S", [("cartpole", 70), ("cartpole", 300),
                                       ("rendezvous", 70)])
def test_wider_shapes(problem, S, K, dtype):
    """B = 2.  S = 70: a trajectory over two wavefronts, the sums through
    LDS; S = 300: a lane runs two candidates, the sums across turns kept in
    U_out and S_out; rendezvous at S = 70: m = 4, so 2m = 8 sums per step go
    through the group.  Every stage as above, K = 8 and K = 1."""
    c = _case(problem, dtype, 0.7, False, S=S, K=K, B_=2, seed=WIDE_SEED)
    _check_costs(c)
    _check_ranks(c.out, K, c.tag)
    _check_refit(c)
    _check_rollout(c)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_candidate(dtype):
    """S = K = 1: only the mean - rank 0, U_out == clamp(U) bit for bit,
    S_out = max(mix sigma, std_min) and J_m is J[:, 0]'s law."""
    c = _case("cartpole", dtype, 0.7, False, S=1, K=1, B_=2, seed=WIDE_SEED)
    _check_costs(c)
    _check_ranks(c.out, 1, c.tag)
    _check_refit(c)
    _check_rollout(c)
    assert torch.equal(c.out.U, torch.minimum(torch.maximum(
        c.s.U, c.s.u_min), c.s.u_max))
    e = rel_err(_np(c.out.J_m), _np(c.out.J[:, 0]))
    assert e < record_tol(dtype), e


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S,K", [(5, 3), (70, 8), (300, 40)])
def test_ties(S, K, dtype):
    """sigma = 0 everywhere: every candidate has the bits of candidate 0, so
    rank[b][s] == s, the elites are 0 .. K-1, U_out == clamp(U) and S_out ==
    std_min, bit for bit."""
    s, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N)
    floor = _floor("cartpole", s.m)
    out = cem_call(s, S, K, 0.0, 0.7, 0.25, 5, std_min=floor)
    assert bool((out.J == out.J[:, :1]).all())
    want = torch.arange(S, dtype=torch.int32, device="cuda").expand(B, S)
    assert torch.equal(out.rank, want), out.rank
    assert out.best.tolist() == [0] * B and out.n_elite.tolist() == [K] * B
    assert torch.equal(out.J_best, out.J[:, 0])
    assert torch.equal(out.U, torch.minimum(torch.maximum(s.U, s.u_min),
                                            s.u_max))
    fl = torch.from_numpy(floor).to(out.S)
    assert torch.equal(out.S, fl.expand(B, N, s.m)), out.S


def _same_rows(a, b, rows, names=ROWS):
    for nm in names:
        x, y = getattr(a, nm), getattr(b, nm)
        for r in rows:
            assert torch.equal(x[r], y[r]), (nm, r)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_no_finite_cost(S, dtype):
    """Trajectory 1 starts at NaN: best -1, J_best and J_m +inf, n_elite 0,
    its ranks -1, its rows of Z_out / U_out / S_out keep the sentinel; the
    costs are written all the same.  The others are what they are without it,
    bit for bit."""
    s, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N, wide=False)
    clean = cem_call(s, S, 3, 3.0, 0.7, 0.25, 23)
    assert bool((clean.best >= 0).all())
    z0 = s.z0.clone()
    z0[1] = float("nan")
    out = cem_call(s, S, 3, 3.0, 0.7, 0.25, 23, z0=z0)
    assert out.best[1].item() == -1 and out.n_elite[1].item() == 0
    assert out.J_best[1].item() == float("inf")
    assert out.J_m[1].item() == float("inf")
    assert bool((out.rank[1] == -1).all())
    assert bool(torch.isnan(out.J[1]).all())
    for nm in ("Z", "U", "S"):
        assert bool((getattr(out, nm)[1] == SENTINEL).all()), nm
    _same_rows(out, clean, (0, 2))


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_masked_trajectory_is_not_touched(S, dtype):
    """active = [1, 0, 1]: nothing of trajectory 1 is read (its z0, U and
    sigma are NaN) or written (every output keeps its fill); the others as
    without the mask, bit for bit."""
    s, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N, wide=False)
    sigma = torch.full((B, N, s.m), 3.0, dtype=s.dtype, device="cuda")
    clean = cem_call(s, S, 3, sigma, 0.7, 0.25, 24)
    z0, U, sg = s.z0.clone(), s.U.clone(), sigma.clone()
    z0[1], U[1], sg[1] = float("nan"), float("nan"), float("nan")
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    out = cem_call(s, S, 3, sg, 0.7, 0.25, 24, active=active, z0=z0, U=U)
    for nm in ROWS:
        fill = -9 if nm in ("rank", "best", "n_elite") else SENTINEL
        assert bool((getattr(out, nm)[1] == fill).all()), nm
    _same_rows(out, clean, (0, 2))


@gpu
def test_some_costs_not_finite():
    """Cartpole, float32, unbounded, S = 70, K = 60, sigma = OVERFLOW_WIDTH:
    the rollouts of some candidates overflow and those of others do not - on
    every trajectory between 1 and S - 1 costs are not finite (the oracle's
    counts: the note at OVERFLOW_WIDTH).  Those get rank -1, n_elite counts
    the rest (fewer than K), and the refit is the model's under the device's
    ranks."""
    S, K = 70, 60
    s, _, z0, U, _, _ = wide_solver("cartpole", "f32", B, N, wide=False)
    out = cem_call(s, S, K, OVERFLOW_WIDTH, 0.7, 0.0, OVERFLOW_SEED,
                   bounded=False)
    bad = (~torch.isfinite(out.J)).sum(dim=1)
    print("costs that are not finite:", bad.tolist())
    assert bool(((bad >= 1) & (bad <= S - 1)).all()), bad
    rank = _check_ranks(out, K, "overflow")
    assert ((rank == -1).sum(axis=1) == _np(bad)).all()
    assert (_np(out.n_elite) == np.minimum(K, S - _np(bad))).all()
    assert bool((out.n_elite < K).any())
    sigma = np.full((B, N, s.m), OVERFLOW_WIDTH)
    e = model_e(B, N, S, s.m, 0.7, OVERFLOW_SEED, 0, "f32")
    Um, Sm, V = model_refit(U, sigma, e, rank, K, 0.0, "f32")
    assert V.min() >= V_FLOOR, V.min()
    for b in range(B):
        err = (rel_err(_np(out.U[b]), Um[b]), rel_err(_np(out.S[b]), Sm[b]))
        print("overflow", b, "U_out, S_out off by", err)
        assert max(err) < record_tol("f32"), (b, err)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [70, 300])
def test_reproducible_and_placeable(S, dtype):
    """The same call twice gives the same bits, with or without the optional
    outputs (S = 70; at S = 300 the rows are required); another seed gives
    other ranks; trajectories 1.. alone with sample_offset + S are what they
    were in the batch with offset 3, bit for bit, and without the shift they
    are not."""
    s, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N, wide=False)
    sigma = random_sigma("cartpole", B, N, s.m, 14, dtype)
    kw = dict(smooth=0.7, mix=0.25, std_min=0.1)
    a = cem_call(s, S, 8, sigma, seed=7, offset=3, **kw)
    b = cem_call(s, S, 8, sigma, seed=7, offset=3, **kw)
    _same_rows(a, b, range(B))
    if S <= 256:
        lean = cem_call(s, S, 8, sigma, seed=7, offset=3, rows=False,
                        ranks=False, **kw)
        _same_rows(a, lean, range(B), ("J", "best", "J_best", "n_elite",
                                       "J_m"))
    other = cem_call(s, S, 8, sigma, seed=8, offset=3, **kw)
    assert torch.equal(other.J[:, 0], a.J[:, 0])
    assert not torch.equal(other.rank, a.rank)
    tail = cem_call(s, S, 8, sigma, seed=7, offset=3 + S, b0=1, **kw)
    for nm in ROWS:
        assert torch.equal(getattr(tail, nm), getattr(a, nm)[1:]), nm
    moved = cem_call(s, S, 8, sigma, seed=7, offset=3, b0=1, **kw)
    assert torch.equal(moved.J[:, 0], a.J[1:, 0])
    assert not torch.equal(moved.rank, a.rank[1:])


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("table", [False, True], ids=["shared", "table"])
@pytest.mark.parametrize("S", [5, 70, 300])
def test_agrees_with_shoot(S, table, dtype):
    """K = 1 and mix = 0 with a_std broadcast to sigma: Jc, best and J_best
    have the bits of pddp_shoot_* on the same arguments - the two units agree
    on draws and costs - and so has U_out: ebar = e_best / 1 and
    g = 1 sigma, the final fma is shoot's."""
    s, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N, table=table)
    std = 0.3 * BOUND["cartpole"]
    shot = shoot_call(s, S, std, 0.7, 11, offset=6)
    out = cem_call(s, S, 1, std, 0.7, 0.0, 11, offset=6)
    assert torch.equal(out.J, shot.J)
    assert torch.equal(out.best, shot.best)
    assert torch.equal(out.J_best, shot.J_best)
    assert bool((out.best > 0).any())
    assert torch.equal(out.U, shot.U)


# ---- the solver's method ------------------------------------------------------
class _Calls(object):
    """The names `_native.call` is asked for (test_round_plan's recorder, the
    part this module needs)."""

    def __init__(self, monkeypatch):
        from pddp_amd import _native
        self.names = []
        real = _native.call

        def wrapped(name, dtype, *args):
            self.names.append("%s_%s" % (name, _native.suffix(dtype)))
            return real(name, dtype, *args)
        monkeypatch.setattr(_native, "call", wrapped)


def _controller(s):
    return {k: getattr(s, k).clone() for k in CONTROLLER}


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("table", [False, True], ids=["shared", "table"])
def test_solver_cem(table, dtype, monkeypatch):
    """ILQRSolver.cem against the entry point called directly.  Three
    iterations are three single launches chained by hand - the distribution
    moves where there is an elite, the incumbent where J_m is finite and not
    above the carried cost - bit for bit; J_trace is non-increasing;
    adopt=False touches nothing; the returned std is accepted as the next
    call's std; adopt=True puts the incumbent into U / Z in place, re-arms
    the controller, a rollout reproduces Z and a round runs."""
    s, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N, table=table)
    S, K = 12, 4
    m = s.m
    sigma0 = random_sigma("cartpole", B, N, m, 15, dtype)
    floor = _floor("cartpole", m)
    kw = dict(smooth=0.7, seed=9, sample_offset=4, mix=0.25)
    s.nominal_rollout()
    s.round()  # (a controller state that is not the re-armed one)
    torch.cuda.synchronize()
    Z0, U0, before = s.Z.clone(), s.U.clone(), _controller(s)
    addr = (s.Z.data_ptr(), s.U.data_ptr(), s.z0.data_ptr())
    std0 = torch.from_numpy(sigma0).to(s.U)
    fl = torch.from_numpy(floor)

    calls = _Calls(monkeypatch)
    r3 = s.cem(S, std0, K, iterations=3, std_min=fl, adopt=False, **kw)
    monkeypatch.undo()
    assert calls.names == ["pddp_cem%s_%s" % ("_batch" if table else "",
                                              dtype)] * 3, calls.names
    assert torch.equal(s.Z, Z0) and torch.equal(s.U, U0)
    for k, v in _controller(s).items():
        assert torch.equal(v, before[k]), k
    assert torch.equal(std0, torch.from_numpy(sigma0).to(s.U))

    mean, std, Ui, Zi = U0, std0, U0, Z0
    trace = []
    for k in range(3):
        o = cem_call(s, S, K, std, 0.7, 0.25, 9, offset=4 + k * B * S,
                     std_min=floor, U=mean)
        if k == 0:
            trace.append(o.J[:, 0])
        better = torch.isfinite(o.J_m) & (o.J_m <= trace[-1])
        take = better.reshape(B, 1, 1)
        Ui, Zi = torch.where(take, o.U, Ui), torch.where(take, o.Z, Zi)
        trace.append(torch.where(better, o.J_m, trace[-1]))
        moved = (o.n_elite > 0).reshape(B, 1, 1)
        mean, std = torch.where(moved, o.U, mean), torch.where(moved, o.S, std)
    for nm in ("J", "rank", "best", "J_best", "n_elite", "J_m"):
        assert torch.equal(getattr(r3, nm), getattr(o, nm)), nm
    assert r3.rank.dtype == r3.n_elite.dtype == torch.int32
    assert torch.equal(r3.mean, mean) and torch.equal(r3.std, std)
    assert torch.equal(r3.U, Ui) and torch.equal(r3.Z, Zi)
    assert torch.equal(r3.J_trace, torch.stack(trace))
    assert bool((r3.J_trace[1:] <= r3.J_trace[:-1]).all()), r3.J_trace
    assert not torch.equal(r3.std, std0) and bool((r3.std >= fl.to(std)).all())
    print(dtype, table, "J_trace", r3.J_trace.tolist())

    # a float and an [m] vector are the tensor; the returned std goes back in
    flat = s.cem(S, 3.0, K, adopt=False, **kw)
    vec = s.cem(S, torch.full((m,), 3.0), K, adopt=False, **kw)
    full = s.cem(S, torch.full((B, N, m), 3.0), K, adopt=False, **kw)
    for nm in ("J", "rank", "J_m", "mean", "std", "U", "Z", "J_trace"):
        assert torch.equal(getattr(flat, nm), getattr(vec, nm)), nm
        assert torch.equal(getattr(flat, nm), getattr(full, nm)), nm
    again = s.cem(S, flat.std, K, adopt=False, **kw)
    assert tuple(again.std.shape) == (B, N, m)
    assert torch.equal(s.Z, Z0) and torch.equal(s.U, U0)

    # adopt=True
    one = s.cem(S, std0, K, std_min=fl, adopt=False, **kw)
    r = s.cem(S, std0, K, std_min=fl, **kw)
    assert not hasattr(r, "Z")
    for nm in ("J", "rank", "best", "J_best", "n_elite", "J_m", "mean",
               "std", "J_trace"):
        assert torch.equal(getattr(r, nm), getattr(one, nm)), nm
    assert torch.equal(s.U, one.U) and torch.equal(s.Z, one.Z)
    keep = ~(r.J_trace[1] < r.J_trace[0])
    assert torch.equal(s.U[keep], U0[keep])
    assert addr == (s.Z.data_ptr(), s.U.data_ptr(), s.z0.data_ptr())
    for k, v in REARMED.items():
        assert bool((getattr(s, k) == v).all()), k
    assert s._derivs_due
    Z = s.Z.clone()
    s.nominal_rollout()
    e = rel_err(s.Z.cpu().numpy(), Z.cpu().numpy())
    print(dtype, table, "nominal_rollout() off the adopted Z by", e)
    assert e < record_tol(dtype), e
    s.Z.copy_(Z)
    s.round()
    assert bool(torch.isfinite(s.J_opt).all()), s.J_opt


@gpu
def test_solver_cem_keeps_rows_without_a_refit():
    """adopt=True: a masked trajectory and one without a finite candidate keep
    their U and Z, and their distribution stays; the masked outputs are NaN /
    -1 / 0."""
    s, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    s.nominal_rollout()
    s.z0[2] = float("nan")
    Z0, U0 = s.Z.clone(), s.U.clone()
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    r = s.cem(12, 3.0, 4, iterations=2, seed=3, active=active)
    assert r.best.tolist()[1:] == [-1, -1] and r.best[0].item() >= 0
    assert r.n_elite.tolist() == [4, 0, 0]
    assert bool(torch.isnan(r.J[1]).all() and torch.isnan(r.J_m[1]))
    assert bool((r.rank[1:] == -1).all())
    assert r.J_m[2].item() == float("inf")
    for b in (1, 2):
        assert torch.equal(s.Z[b], Z0[b]) and torch.equal(s.U[b], U0[b]), b
        assert torch.equal(r.mean[b], U0[b]) and bool((r.std[b] == 3.0).all())


@gpu
def test_solver_cem_refusals():
    from pddp_amd import _native
    from pddp_amd.controllers.solver import ILQRSolver
    s, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    with pytest.raises(_native.NativeError, match="std"):
        s.cem(5, torch.ones(3), 2)
    with pytest.raises(_native.NativeError, match="std"):
        s.cem(5, torch.ones(B, N + 1, s.m), 2)
    with pytest.raises(_native.NativeError, match="std"):
        s.cem(5, 1.0, 2, std_min=torch.ones(3))
    with pytest.raises(_native.NativeError, match="samples"):
        s.cem(0, 1.0, 1)
    for K in (0, 6):
        with pytest.raises(_native.NativeError, match="elites"):
            s.cem(5, 1.0, K)
    with pytest.raises(_native.NativeError, match="iterations"):
        s.cem(5, 1.0, 2, iterations=0)
    with pytest.raises(_native.NativeError, match="events"):
        s.cem(5, 1.0, 2, iterations=2, events=(None, None))
    with pytest.raises(_native.NativeError):
        s.cem(5, 1.0, 2, smooth=1.0)
    with pytest.raises(_native.NativeError):
        s.cem(5, 1.0, 2, mix=1.0)
    with pytest.raises(_native.NativeError, match="active"):
        s.cem(5, 1.0, 2, active=torch.ones(B, device="cuda"))
    s.set_batch_weights()
    with pytest.raises(_native.NativeError, match="weights"):
        s.cem(5, 1.0, 2)
    s.clear_batch_weights()
    s.set_reference(torch.zeros(B, N + 1, s.problem.aug_size))
    with pytest.raises(_native.NativeError, match="reference"):
        s.cem(5, 1.0, 2)
    plug = ILQRSolver(None, B, N, torch.float64, "cuda", plugin=object(),
                      n=4, m=1)
    with pytest.raises(_native.NativeError, match="sample problem"):
        plug.cem(5, 1.0, 2)
