"""Closed-loop evaluation under process and measurement noise drawn on the
device (pddp_closed_loop_noisy_*, pddp_closed_loop_draws_*,
csrc/closed_loop.hip, ILQRSolver.closed_loop(process_std=, obs_std=),
ILQRSolver.closed_loop_draws).

The draws are defined in include/pddp_hip.h; `solver_util.model_draws` restates
them in numpy (Philox4x32-10 on a counter, Box-Muller on its words, everything
past the exact uniforms in float64).  The rollouts are checked against the CPU
oracle stepped rollout by rollout under the noisy law with the MODEL's normals,
so a device draw that differs from the model shows in two places."""
import ctypes

import numpy as np
import pytest
import torch

import oracle as orc
from abi_util import assert_entry_points, caller, cartpole_pointers
from golden_util import np_dtype, rel_err
from solver_util import (check_stats, closed_loop_call, draws_call,
                         model_draws, noisy_call, perturbed_starts,
                         philox4x32_10, plant_rows, policy_solver, PROBLEMS,
                         record_tol)

gpu = pytest.mark.gpu
SYMBOLS = ["pddp_closed_loop_noisy_f32", "pddp_closed_loop_noisy_f64",
           "pddp_closed_loop_draws_f32", "pddp_closed_loop_draws_f64"]
STD = 0.02
VARIANTS = {"process": (STD, None), "obs": (None, STD), "both": (STD, STD)}


# ---- what the rollouts should give ------------------------------------------
def _oracle_noisy_rollouts(s, dtype, ops, z0s, u_min, u_max, w_std, v_std,
                           seed, offset=0):
    """(X [B][N+1][S][n], U [B][N][S][m], J [B][S]): the oracle's dynamics and
    cost stepped under the noisy law, in the run's dtype, with the model's
    normals."""
    o = orc.load(np_dtype(dtype))
    B, N, n, m = s.B, s.N, s.n, s.m
    S = z0s.shape[1]
    d = np_dtype(dtype)
    Z, U = s.Z.cpu().numpy(), s.U.cpu().numpy()
    K = s.gain_views()[1].cpu().numpy()
    Wn = None if w_std is None else \
        (w_std * model_draws(B, N, S, n, 0, seed, offset, dtype)).astype(d)
    Vn = None if v_std is None else \
        (v_std * model_draws(B, N, S, n, 1, seed, offset, dtype)).astype(d)
    X = np.empty((B, N + 1, S, n), d)
    Uo = np.empty((B, N, S, m), d)
    J = np.zeros((B, S), d)
    for b in range(B):
        for i in range(S):
            p, x = ops[b][i], z0s[b, i].astype(d)
            for t in range(N):
                y = x if Vn is None else x + Vn[b, t, i]
                u = np.clip(U[b, t] + K[b, t] @ (y - Z[b, t]), u_min, u_max)
                u = u.astype(d)
                X[b, t, i], Uo[b, t, i] = x, u
                J[b, i] += o.cost(p, x, u)[0]
                x = o.dynamics(p, x, u, jac=False)[0]
                if Wn is not None:
                    x = x + Wn[b, t, i]
            X[b, N, i] = x
            J[b, i] += o.cost(p, x, None, terminal=True)[0]
    return X, Uo, J


# ---- CPU -------------------------------------------------------------------
def test_noisy_entry_points_are_declared_exported_and_bound():
    """CPU: the four symbols in the header, the built library,
    exported_symbols() and _native._SIGS; the ABI version and
    pddp_closed_loop's 17 arguments as they were."""
    from pddp_amd import _native
    assert_entry_points(SYMBOLS)
    assert len(_native._SIGS["pddp_closed_loop"]) == 17
    assert len(_native._SIGS["pddp_closed_loop_noisy"]) == 21
    assert len(_native._SIGS["pddp_closed_loop_draws"]) == 9
    for name in ("pddp_closed_loop_noisy", "pddp_closed_loop_draws"):
        sig = _native._SIGS[name]
        assert [i for i, c in enumerate(sig) if c is ctypes.c_uint64] == \
            ([13, 14] if name.endswith("noisy") else [5, 6]), name
    assert _native.lib().pddp_hip_abi_version() == 1


def test_noisy_entry_points_refuse_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call), both dtypes.  Rollouts: PDDP_E_BADARG for everything
    pddp_closed_loop_* refuses and for w_std == v_std == NULL;
    PDDP_E_UNSUPPORTED for a DEFAULT-encoding problem.  Draws: PDDP_E_BADARG
    for a null W, a non-positive size, which outside {0, 1} and
    n > PDDP_MAX_STATE (8).  The non-null pointers are host words nobody
    reads."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    lib = _native.lib()
    for t in ("f32", "f64"):
        #       0  1  2  3  4  5  6     7     8     9     10 11 12 13
        #       B  N  S  Z  U  K  z0s   plant umin  umax  w  v  seed off
        good = [2, 3, 1, q, q, q, None, None, None, None, q, q, 7, 0,
                #  14   15 16 17 18
                #  act  Xc Uc Jc st
                None, q, q, q, q]
        call = caller(getattr(lib, "pddp_closed_loop_noisy_" + t), good)

        assert call(pp, _17=None) == -1, t             # Jc
        assert call(pp, _0=0) == -1, t                 # B
        assert call(pp, _1=0) == -1, t                 # N
        assert call(pp, _2=0) == -1, t                 # S
        assert call(pp, _2=-3) == -1, t
        assert call(pp, _16=None) == -1, t             # Xc without Uc
        assert call(pp, _15=None) == -1, t             # Uc without Xc
        assert call(pp, _3=None) == -1, t              # Z
        assert call(pp, _4=None) == -1, t              # U
        assert call(None) == -1, t
        assert call(pp, _10=None, _11=None) == -1, t   # no noise at all
        assert call(ppd) == _native.E_UNSUPPORTED, t
        assert call(ppd, _10=None) == _native.E_UNSUPPORTED, t
        assert call(ppd, _11=None) == _native.E_UNSUPPORTED, t
        assert call(ppd, _15=None, _16=None) == _native.E_UNSUPPORTED, t

        #        B  N  S  n  which seed off W
        dgood = [2, 3, 4, 4, 0, 7, 0, q]
        draws = caller(getattr(lib, "pddp_closed_loop_draws_" + t), dgood)

        assert draws(_7=None) == -1, t                 # W
        for i in range(4):                             # B, N, S, n
            assert draws(**{"_%d" % i: 0}) == -1, (t, i)
            assert draws(**{"_%d" % i: -1}) == -1, (t, i)
        assert draws(_4=2) == -1 and draws(_4=-1) == -1, t
        assert draws(_3=9) == -1, t                    # n > PDDP_MAX_STATE


def test_numpy_model_known_answers():
    """The model against the published Philox4x32-10 vectors, the anchors of
    seed 2026 and 5-sigma bounds on the first two moments of M = 65 536 draws
    (|mean| < 5 / sqrt(M), |var - 1| < 5 sqrt(2 / M))."""
    kat = [((0, 0, 0, 0), (0, 0),
            (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2,
            (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
            (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        got = philox4x32_10([np.array([c], np.uint64) for c in counter], key)
        assert tuple(int(g[0]) for g in got) == want, (counter, got)
    a32 = model_draws(1, 1, 1, 4, 0, 2026, 0, "f32").ravel()
    a64 = model_draws(1, 1, 1, 2, 0, 2026, 0, "f64").ravel()
    assert np.allclose(a32, [-1.28452472, -0.18145641, -0.24229188,
                             0.8049075], rtol=0, atol=5e-8), a32
    assert np.allclose(a64, [-0.38244172, -1.23962435], rtol=0,
                       atol=5e-9), a64
    B, N, S, n = 4, 16, 256, 4
    M = B * N * S * n
    assert M == 65536
    for dtype in ("f32", "f64"):
        w = [model_draws(B, N, S, n, which, 2026, 0, dtype)
             for which in (0, 1)]
        for z in w:
            print(dtype, "mean", z.mean(), "var", z.var())
            assert abs(z.mean()) < 5 / np.sqrt(M)
            assert abs(z.var() - 1) < 5 * np.sqrt(2.0 / M)
        print(dtype, "correlation of the streams",
              np.corrcoef(w[0].ravel(), w[1].ravel())[0, 1])


# ---- GPU -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(3, 5, 5, 2), (3, 5, 5, 4), (3, 5, 5, 6),
                                   (3, 5, 5, 8), (2, 5, 70, 4)])
def test_draws_match_the_model(shape, dtype):
    """pddp_closed_loop_draws_* against the model: both streams, sample
    offsets 0, 5 and 2^32 - 3 (c1 turns non-zero inside the batch).
    Bar: |W - model| <= 32 eps max(1, |model|) - the uniforms are exact, the
    model is float64, what is left is a few ulp of ln, sqrt, cos, sin on
    values below 8."""
    B, N, S, n = shape
    eps = 2.0 ** -23 if dtype == "f32" else 2.0 ** -52
    worst = 0.0
    for which in (0, 1):
        for offset in (0, 5, 2 ** 32 - 3):
            W = draws_call(B, N, S, n, which, 2026, offset,
                           dtype).cpu().numpy().astype(np.float64)
            want = model_draws(B, N, S, n, which, 2026, offset, dtype)
            dev = (np.abs(W - want) / np.maximum(1.0, np.abs(want))).max()
            worst = max(worst, dev / eps)
            assert np.isfinite(W).all()
            assert dev <= 32 * eps, (which, offset, dev / eps)
    print(shape, dtype, "largest deviation: %.2f eps (bar 32)" % worst)


def _check_noisy_vs_oracle(problem, dtype, B, N, S, seed):
    s, _, u_min, u_max = policy_solver(problem, dtype, B, N)
    rows, ops = plant_rows(problem, B, S, seed, dtype)
    z0s = perturbed_starts(s, S, seed + 100)
    tol = record_tol(dtype)
    for name, (w_std, v_std) in VARIANTS.items():
        out = noisy_call(s, S, z0s=z0s, plant=rows, w_std=w_std, v_std=v_std,
                         seed=11)
        X, U, J = _oracle_noisy_rollouts(s, dtype, ops, z0s, u_min, u_max,
                                         w_std, v_std, seed=11)
        for b in range(B):
            e = (rel_err(out.X[b].cpu().numpy(), X[b]),
                 rel_err(out.U[b].cpu().numpy(), U[b]),
                 rel_err(out.J[b].cpu().numpy(), J[b]))
            print(problem, dtype, S, name, b, e)
            assert max(e) < tol, (name, b, e)
        check_stats(out, dtype, S)
        # (the bar tells the noise from none: 0.02 per step on states of
        # order 1 to 10 is far above it, as the plain launch's states show)
        if name == "both":
            plain = closed_loop_call(s, S, z0s=z0s, plant=rows)
            d = rel_err(plain.X.cpu().numpy(), X)
            print(problem, dtype, S, "plain rollout off by", d)
            assert d > 5 * tol, d


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_noisy_rollouts_vs_oracle(problem, dtype):
    """B = 3, N = 12, S = 5 (5 of 8 lanes, several trajectories to a
    wavefront), w_std = v_std = 0.02: process only, measurement only, both."""
    _check_noisy_vs_oracle(problem, dtype, B=3, N=12, S=5, seed=31)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_noisy_rollouts_wider_than_a_wavefront(dtype):
    """Cartpole at S = 70: a trajectory over two wavefronts."""
    _check_noisy_vs_oracle("cartpole", dtype, B=2, N=12, S=70, seed=32)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_noise_is_reproducible_and_offsets_shift_it(S, dtype):
    B, N = 3, 12
    s, _, _, _ = policy_solver("cartpole", dtype, B, N)
    rows, _ = plant_rows("cartpole", B, S, 35, dtype)
    z0s = perturbed_starts(s, S, 135)
    kw = dict(z0s=z0s, plant=rows, w_std=STD, v_std=STD)
    a = noisy_call(s, S, seed=7, **kw)
    b = noisy_call(s, S, seed=7, **kw)
    for nm in ("J", "X", "U", "stats"):
        assert torch.equal(getattr(a, nm), getattr(b, nm)), nm
    lean = noisy_call(s, S, seed=7, keep=False, **kw)
    assert torch.equal(lean.J, a.J) and torch.equal(lean.stats, a.stats)
    other = noisy_call(s, S, seed=8, **kw)
    assert not torch.equal(other.J, a.J)
    assert not bool((other.J == a.J).any())
    # trajectories 1 .. B-1 alone, placed where they were in the batch
    tail = noisy_call(s, S, seed=7, offset=S, b0=1, **kw)
    for nm in ("J", "X", "U", "stats"):
        assert torch.equal(getattr(tail, nm), getattr(a, nm)[1:]), nm
    # (and without the offset they see trajectory 0's noise instead)
    moved = noisy_call(s, S, seed=7, offset=0, b0=1, **kw)
    assert not torch.equal(moved.J, a.J[1:])


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_zero_noise_is_the_plain_rollout(dtype):
    B, N, S = 3, 12, 5
    s, _, _, _ = policy_solver("cartpole", dtype, B, N)
    rows, _ = plant_rows("cartpole", B, S, 36, dtype)
    z0s = perturbed_starts(s, S, 136)
    plain = closed_loop_call(s, S, z0s=z0s, plant=rows)
    zero = noisy_call(s, S, z0s=z0s, plant=rows, w_std=0.0, v_std=0.0,
                      seed=3)
    tol = record_tol(dtype)
    for nm in ("X", "U", "J", "stats"):
        a, b = getattr(zero, nm), getattr(plain, nm)
        print(dtype, nm, "zero noise == plain, bit for bit:",
              torch.equal(a, b))
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < tol, nm


@gpu
def test_solver_closed_loop_keywords():
    """ILQRSolver.closed_loop(process_std=, obs_std=, seed=, sample_offset=)
    and closed_loop_draws against the entry points themselves.  (The gains of
    the last sweep, accepted=False: the accepted ones of a solver that has
    accepted nothing are zero.)"""
    from pddp_amd import _native
    B, N, S = 3, 12, 5
    s, _, _, _ = policy_solver("cartpole", "f64", B, N)
    same = lambda a, b: all(
        torch.equal(getattr(a, nm), getattr(b, nm)) for nm in ("J", "stats"))
    r = s.closed_loop(samples=S, process_std=STD, seed=7, accepted=False)
    want = noisy_call(s, S, w_std=STD, seed=7, keep=False)
    assert r.X is None and same(r, want)
    # a scalar and an [n] vector agree; obs_std, sample_offset and keep go
    # through
    vec = torch.full((s.n,), STD, dtype=torch.float64)
    assert same(s.closed_loop(samples=S, process_std=vec, seed=7,
                              accepted=False), want)
    levels = torch.tensor([0.01, 0.02, 0.03, 0.04], dtype=torch.float64)
    r = s.closed_loop(samples=S, process_std=levels, obs_std=0.5 * levels,
                      seed=9, sample_offset=40, accepted=False, keep=True)
    want = noisy_call(s, S, w_std=levels.cuda(), v_std=(0.5 * levels).cuda(),
                      seed=9, offset=40)
    assert same(r, want) and torch.equal(r.X, want.X) and \
        torch.equal(r.U, want.U)
    r = s.closed_loop(samples=S, obs_std=STD, seed=7, accepted=False)
    assert same(r, noisy_call(s, S, v_std=STD, seed=7, keep=False))
    with pytest.raises(_native.NativeError):
        s.closed_loop(samples=S, process_std=torch.ones(3), accepted=False)
    # without the keywords: the plain entry point, as before
    r = s.closed_loop(samples=S, accepted=False, keep=True)
    want = closed_loop_call(s, S)
    assert same(r, want) and torch.equal(r.X, want.X)
    # the draws
    for which, w in (("process", 0), ("obs", 1)):
        W = s.closed_loop_draws(S, which=which, seed=7, sample_offset=3)
        assert tuple(W.shape) == (B, N, S, s.n)
        assert torch.equal(W, draws_call(B, N, S, s.n, w, 7, 3, "f64"))
    with pytest.raises(_native.NativeError):
        s.closed_loop_draws(S, which="both")
    # under a reference closed_loop refuses, with or without noise
    s.set_reference(torch.zeros(B, N + 1, s.problem.aug_size))
    with pytest.raises(_native.NativeError, match="reference"):
        s.closed_loop(samples=S, process_std=STD)
