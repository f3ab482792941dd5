"""Sampled shooting with a softmin-weighted (MPPI) update on the device
(pddp_mppi_*, pddp_mppi_batch_*, csrc/mppi.hip, ILQRSolver.mppi).

include/pddp_hip.h is the definition.  Each stage is held against a model fed
with the DEVICE's previous stage, so the amplification of a cost error through
exp(. / lam) can neither hide a wrong kernel nor fail a right one: the costs
against the CPU oracle along `shoot_util`'s candidates; the weights against
the float64 softmin of the device's own costs; the weighted actions against
the float64 mean of the model's AR(1) values under the device's own weights;
the weighted rollout against the oracle stepped along the device's own
actions.  One float64 test takes the whole chain from the oracle's costs."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from abi_util import assert_entry_points, caller, cartpole_pointers
from golden_util import np_dtype, rel_err
from mppi_util import (model_e, model_update, model_weights, mppi_call,
                       rounded, weighted_actions, wide_solver)
from shoot_util import (first_argmin, model_candidates, oracle_rollouts,
                        shoot_call)
from solver_util import (BOUND, CONTROLLER, PROBLEMS, REARMED, SENTINEL,
                         record_tol)

gpu = pytest.mark.gpu
SYMBOLS = ["pddp_mppi_f32", "pddp_mppi_f64", "pddp_mppi_batch_f32",
           "pddp_mppi_batch_f64"]
B, N = 3, 12
EPS = {"f32": 2.0 ** -23, "f64": 2.0 ** -52}
# tests/test_shoot.py's test_selection_vs_oracle's seeds, searched on the CPU
SELECTION_SEED = {("f64", 5): 4, ("f32", 5): 22, ("f64", 70): 1,
                  ("f32", 70): 1}


# ---- CPU -------------------------------------------------------------------
def test_mppi_entry_points_are_declared_exported_and_bound():
    """CPU: the four symbols in the header, the built library,
    exported_symbols() and _native._SIGS; where the double and the 64-bit
    integers sit (after the six input pointers: z0, U, u_min, u_max, a_std,
    lam); the ABI version as it was."""
    from pddp_amd import _native
    assert_entry_points(SYMBOLS)
    want = {"pddp_mppi": (22, 10), "pddp_mppi_batch": (23, 11)}
    for name, (count, at) in want.items():
        sig = _native._SIGS[name]
        assert len(sig) == count, name
        assert [i for i, c in enumerate(sig) if c is ctypes.c_double] == \
            [at], name
        assert [i for i, c in enumerate(sig) if c is ctypes.c_uint64] == \
            [at + 1, at + 2], name
        assert [i for i, c in enumerate(sig) if c is ctypes.c_int] == \
            [at - 9, at - 8, at - 7], name
    assert _native.lib().pddp_hip_abi_version() == 1


def test_mppi_entry_points_refuse_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call), both dtypes, both forms.  PDDP_E_BADARG: pddp_shoot_*'s list - each
    null required pointer, B, N, S of 0 and negative, B S > 0x7fffffff, one of
    Z_out / U_out, U_out == U, Z_out == z0, smooth of 1.0, -0.1 and NaN, a NULL
    table on _batch - and a NULL lam, a NULL J_w, S = 257 without rows;
    PDDP_E_UNSUPPORTED: a DEFAULT-encoding problem.  The non-null pointers are
    host words nobody reads (q and r: two of them, for the aliasing tests)."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    r = q + 8
    lib = _native.lib()
    for t in ("f32", "f64"):
        #       0  1  2  3   4  5     6     7     8    9       10    11
        #       B  N  S  z0  U  umin  umax  astd  lam  smooth  seed  off
        good = [2, 3, 4, q, q, None, None, q, q, 0.5, 7, 0,
                #  12   13  14    15      16  17   18     19
                #  act  Jc  best  J_best  W   J_w  Z_out  U_out
                None, q, q, q, q, q, r, r]
        plain = caller(getattr(lib, "pddp_mppi_" + t), good)
        batch = caller(getattr(lib, "pddp_mppi_batch_" + t), good)
        forms = ((plain, (pp,), (ppd,), (None,)),
                 (batch, (pp, q), (ppd, q), (None, q)))
        for call, ok, gaussian, no_problem in forms:
            for i in (3, 4, 7, 8, 13, 14, 17):         # required pointers
                assert call(*ok, **{"_%d" % i: None}) == -1, (t, i)
            assert call(*no_problem) == -1, t
            for i in (0, 1, 2):                        # B, N, S
                assert call(*ok, **{"_%d" % i: 0}) == -1, (t, i)
                assert call(*ok, **{"_%d" % i: -3}) == -1, (t, i)
            assert call(*ok, _0=1 << 16, _2=1 << 15) == -1, t   # B S = 2^31
            assert call(*ok, _18=None) == -1, t        # U_out without Z_out
            assert call(*ok, _19=None) == -1, t        # Z_out without U_out
            assert call(*ok, _19=q) == -1, t           # U_out == U
            assert call(*ok, _3=r) == -1, t            # Z_out == z0
            assert call(*ok, _2=257, _18=None, _19=None) == -1, t
            for smooth in (1.0, -0.1, float("nan")):
                assert call(*ok, _9=smooth) == -1, (t, smooth)
            assert call(*gaussian) == _native.E_UNSUPPORTED, t
            assert call(*gaussian, _15=None, _16=None, _18=None, _19=None) \
                == _native.E_UNSUPPORTED, t
        assert batch(pp, None) == -1, t                # no table


def test_numpy_model_of_the_update():
    """CPU: the model itself.  S = 1 gives weight 1 and the clamped base;
    equal costs give weights 1 / S and the sum of e over s >= 1 divided by S
    (candidate 0 has a weight and no perturbation); a cost that is not finite
    gets weight 0 and the others share the rest; no finite cost, or a
    temperature that is not positive: zeros."""
    rng = np.random.RandomState(4)
    U = rng.randn(2, 6, 2)
    for dtype in ("f32", "f64"):
        e1 = model_e(2, 6, 1, 2, 0.7, 9, 0, dtype)
        W, Uw = model_update(U, np.array([[3.0], [5.0]]), 2.0, e1, 0.5, -1.0,
                             1.0)
        assert (W == 1.0).all() and (Uw == np.clip(U, -1.0, 1.0)).all(), dtype
        S = 4
        e = model_e(2, 6, S, 2, 0.7, 9, 0, dtype)
        W, Uw = model_update(U, np.full((2, S), 7.0), [2.0, 3.0], e, 0.5)
        assert (W == 1.0 / S).all(), dtype
        want = U + 0.5 * e[:, :, 1:].sum(axis=2) / S
        assert np.abs(Uw - want).max() < 1e-15, dtype
        _, Uc = model_update(U, np.full((2, S), 7.0), 2.0, e, 0.5, -1.0, 1.0)
        assert (Uc == np.clip(Uw, -1.0, 1.0)).all() and (Uc != Uw).any(), dtype
        J = np.array([[1.0, np.inf, 1.0, np.nan], [2.0, 2.0 + np.log(2.0),
                                                   -np.inf, 2.0]])
        W = model_weights(J, 1.0)
        assert (W[0] == [0.5, 0.0, 0.5, 0.0]).all(), W[0]
        assert np.abs(W[1] - [0.4, 0.2, 0.0, 0.4]).max() < 1e-15, W[1]
        assert (model_weights(np.full((1, S), np.nan), 1.0) == 0).all()
        assert (model_weights(J, [0.0, np.nan]) == 0).all()
        assert (model_weights(J, -1.0) == 0).all()


# ---- GPU: what the tests share ------------------------------------------------
def _lam_of(J):
    """0.5 (median_s J - min_s J) per trajectory: another one each, so the [B]
    argument is exercised; 1 where that is 0 (S = 1)."""
    J = np.asarray(J, np.float64)
    lam = 0.5 * (np.median(J, axis=1) - J.min(axis=1))
    return np.where(lam > 0, lam, 1.0)


@functools.lru_cache(maxsize=None)
def _case(problem, dtype, smooth, table, S=5, B_=B, seed=21):
    """One launch and its references, shared by the stage tests: the oracle's
    costs along the model's candidates, lam from them, the device's outputs."""
    s, ops, z0, U, u_min, u_max = wide_solver(problem, dtype, B_, N,
                                              table=table)
    std = 0.3 * BOUND[problem]
    Uc, hit = model_candidates(U, S, std, smooth, seed, 0, dtype, u_min,
                               u_max)
    _, J = oracle_rollouts(ops, z0, Uc, dtype)
    lam = rounded(_lam_of(J), dtype)
    out = mppi_call(s, S, std, lam, smooth, seed)
    return types.SimpleNamespace(
        s=s, ops=ops, z0=z0, U=U, u_min=u_min, u_max=u_max, dtype=dtype, S=S,
        std=std, smooth=smooth, seed=seed, hit=hit, J_orc=J, lam=lam, out=out,
        e=model_e(B_, N, S, s.m, smooth, seed, 0, dtype),
        tag=(problem, dtype, smooth, table, S))


def _np(t):
    return t.cpu().numpy()


def _check_costs(c):
    """Stage 1: Jc against the oracle within record_tol; best and J_best
    exactly, on the device's own costs."""
    J = _np(c.out.J)
    tol = record_tol(c.dtype)
    for b in range(J.shape[0]):
        e = rel_err(J[b], c.J_orc[b])
        print(c.tag, b, "J off by", e)
        assert e < tol, (c.tag, b, e)
    best = _np(c.out.best)
    assert (best == first_argmin(J)).all(), (best, first_argmin(J))
    for b in range(J.shape[0]):
        assert 0 <= best[b] < c.S, (c.tag, b, best[b])
        assert _np(c.out.J_best[b]).tobytes() == J[b, best[b]].tobytes(), b


def _check_weights(c):
    """Stage 2: W against the float64 softmin of the device's own costs,
    |W - model| <= 32 eps absolute; rows sum to 1 within the same bar."""
    Wm = model_weights(_np(c.out.J), c.lam)
    Wd = _np(c.out.W).astype(np.float64)
    dev = np.abs(Wd - Wm).max() / EPS[c.dtype]
    rows = np.abs(Wd.sum(axis=1) - 1.0).max() / EPS[c.dtype]
    print(c.tag, "W off by %.2f eps, rows off 1 by %.2f eps (bar 32)" %
          (dev, rows))
    assert dev <= 32 and rows <= 32, (c.tag, dev, rows)


def _check_update(c):
    """Stage 3: U_out against clip(U + std sum_s W_dev[s] e_model[s, t]) in
    float64, rel_err within record_tol."""
    Um = weighted_actions(c.U, _np(c.out.W).astype(np.float64), c.e, c.std,
                          c.u_min, c.u_max)
    Ud = _np(c.out.U)
    for b in range(Ud.shape[0]):
        e = rel_err(Ud[b], Um[b])
        print(c.tag, b, "U_out off by", e)
        assert e < record_tol(c.dtype), (c.tag, b, e)
    return Um


def _check_rollout(c):
    """Stage 4: Z_out and J_w against the oracle stepped along the device's
    own U_out."""
    Ud = _np(c.out.U)
    X, J = oracle_rollouts(c.ops, c.z0, Ud[:, None], c.dtype)
    tol = record_tol(c.dtype)
    for b in range(Ud.shape[0]):
        e = (rel_err(_np(c.out.Z[b]), X[b, 0]),
             rel_err(_np(c.out.J_w[b]), J[b, 0]))
        print(c.tag, b, "Z_out, J_w off by", e)
        assert max(e) < tol, (c.tag, b, e)


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
    """B = 3, N = 12, S = 5, bounded, std = 0.3 BOUND around base actions
    spread over 0.8 BOUND: the clamp is met on some steps and not on others
    (asserted from the model).  J within record_tol of the oracle along the
    model's candidates; best and J_best exact on the device's own costs - as
    tests/test_shoot.py's test_candidates_vs_oracle."""
    c = _case(problem, dtype, smooth, table)
    assert c.hit[:, 1:].any() and not c.hit[:, 1:].all(), c.hit.mean()
    _check_costs(c)
    assert bool((c.out.J_best <= c.out.J[:, 0]).all())


@_all_cases
def test_weights_vs_softmin_of_device_costs(problem, dtype, smooth, table):
    """lam[b] = 0.5 (median_s J - min_s J) of the oracle's costs, rounded to
    the run's type.  The bar, 32 eps absolute: the exponent's rounding moves
    w_s by at most a_s exp(-a_s) eps <= eps / e, exp by a few ulp, eta by about
    log2 S ulp."""
    c = _case(problem, dtype, smooth, table)
    assert len(set(c.lam)) == B, c.lam
    _check_weights(c)


@_all_cases
def test_update_vs_model_under_device_weights(problem, dtype, smooth, table):
    _check_update(_case(problem, dtype, smooth, table))


@_all_cases
def test_weighted_rollout_vs_oracle(problem, dtype, smooth, table):
    _check_rollout(_case(problem, dtype, smooth, table))


@gpu
@pytest.mark.parametrize("table", [False, True], ids=["shared", "table"])
@pytest.mark.parametrize("smooth", [0.0, 0.7])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_end_to_end_f64(problem, smooth, table):
    """The whole chain from the ORACLE's costs in float64: U_out against
    clip(U + std sum_s softmin(J_orc / lam)[s] e_model[s, t]).  A cost error d
    moves the softmin by at most 2 d / lam in the 1-norm, so the bar is
    2 std max|e| max_s|J_dev - J_orc| / lam per trajectory, plus stage 3's
    (record_tol relative to the row's largest action); every term comes from
    the model and the oracle."""
    c = _case(problem, "f64", smooth, table)
    Um = weighted_actions(c.U, model_weights(c.J_orc, c.lam), c.e, c.std,
                          c.u_min, c.u_max)
    Ud, Jd = _np(c.out.U), _np(c.out.J)
    for b in range(B):
        bar = 2 * c.std * np.abs(c.e[b]).max() * \
            np.abs(Jd[b] - c.J_orc[b]).max() / c.lam[b] + \
            record_tol("f64") * np.abs(Um[b]).max()
        dev = np.abs(Ud[b] - Um[b]).max()
        print(c.tag, b, "U_out off the oracle's chain by", dev, "bar", bar)
        assert dev <= bar, (c.tag, b, dev, bar)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem,S", [("cartpole", 1), ("cartpole", 70),
                                       ("cartpole", 300), ("rendezvous", 70)])
def test_wider_shapes(problem, S, dtype):
    """B = 2.  S = 1: only the base - W == 1, U_out == clamp(U) bit for bit
    and J_w is J[:, 0]'s law (within record_tol of it); S = 70: a trajectory
    over two wavefronts, the sums through LDS; S = 300: a lane runs two
    candidates, the sum across turns kept in U_out; rendezvous at S = 70:
    m = 4 sums per step through LDS.  Every stage as above."""
    c = _case(problem, dtype, 0.7, False, S=S, B_=2, seed=22)
    _check_costs(c)
    _check_weights(c)
    _check_update(c)
    _check_rollout(c)
    if S == 1:
        assert bool((c.out.W == 1).all())
        assert torch.equal(c.out.U, torch.minimum(torch.maximum(
            c.s.U, c.s.u_min), c.s.u_max))
        e = rel_err(_np(c.out.J_w), _np(c.out.J[:, 0]))
        assert e < record_tol(dtype), e


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_flat_weights_at_a_huge_temperature(dtype):
    """lam = 1e30 (1 + max J): every exponent rounds to -0 or a value whose
    exp is 1, so W is exactly 1 / (number of finite candidates) rounded
    once."""
    c = _case("cartpole", dtype, 0.7, False)
    lam = 1e30 * (1.0 + np.abs(c.J_orc).max())
    out = mppi_call(c.s, c.S, c.std, lam, c.smooth, c.seed)
    assert bool(torch.isfinite(out.J).all())
    d = np_dtype(dtype)
    assert (_np(out.W) == d(1) / d(c.S)).all(), out.W
    c2 = types.SimpleNamespace(**vars(c))
    c2.out, c2.lam = out, np.full(B, rounded(lam, dtype))
    _check_update(c2)
    _check_rollout(c2)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_one_hot_weights_give_shoots_winner(S, dtype):
    """tests/test_shoot.py's test_selection_vs_oracle's configuration and
    seeds: the ORACLE's gap between its best and second-best cost exceeds
    4 record_tol |J_best| on every trajectory (asserted from the oracle
    alone), so the device's best is the oracle's.  With lam = g / 1000, g the
    smallest gap between the best and the second-best DEVICE cost over the
    batch, every other exponent is below -1000 and its exp is 0 in both
    types: W is one-hot at best, and U_out has the bits of pddp_shoot_*'s
    U_out on the same arguments - the e chain and the final fma are the same
    explicit operations and ebar = e_best 1 / 1."""
    s, ops, z0, U, u_min, u_max = wide_solver("cartpole", dtype, B, N)
    std, seed = 0.3 * BOUND["cartpole"], SELECTION_SEED[dtype, S]
    Uc, _ = model_candidates(U, S, std, 0.7, seed, 0, dtype, u_min, u_max)
    _, J = oracle_rollouts(ops, z0, Uc, dtype)
    J = J.astype(np.float64)
    order = np.sort(J, axis=1)
    gap = order[:, 1] - order[:, 0]
    need = 4 * record_tol(dtype) * np.abs(order[:, 0])
    assert (gap > need).all(), (gap, need)
    first = mppi_call(s, S, std, 1.0, 0.7, seed)
    Jd = np.sort(_np(first.J).astype(np.float64), axis=1)
    g = (Jd[:, 1] - Jd[:, 0]).min()
    assert g > 0, g
    out = mppi_call(s, S, std, g / 1000, 0.7, seed)
    best = _np(out.best)
    assert (best == J.argmin(axis=1)).all(), (best, J.argmin(axis=1))
    hot = np.zeros((B, S))
    hot[np.arange(B), best] = 1.0
    assert (_np(out.W) == hot).all(), out.W
    shot = shoot_call(s, S, std, 0.7, seed)
    assert torch.equal(shot.best, out.best)
    assert torch.equal(out.U, shot.U)


def _same_rows(a, b, rows, names):
    for nm in names:
        x, y = getattr(a, nm), getattr(b, nm)
        for r in rows:
            assert torch.equal(x[r], y[r]), (nm, r)


NAMES = ("J", "best", "J_best", "W", "J_w", "Z", "U")


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_no_weighted_sequence(S, dtype):
    """Trajectory 1 without a finite candidate (a NaN start), and with a
    temperature of 0, of NaN and below 0: best -1, J_best and J_w +inf, its
    row of W zeros, its rows of Z_out / U_out keep the sentinel; the costs are
    written all the same.  The others are what they are without it, bit for
    bit."""
    s, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N, wide=False)
    clean = mppi_call(s, S, 3.0, 40.0, 0.7, 23)
    assert bool((clean.best >= 0).all())
    z0 = s.z0.clone()
    z0[1] = float("nan")
    runs = [("nan start", mppi_call(s, S, 3.0, 40.0, 0.7, 23, z0=z0))]
    for bad in (0.0, float("nan"), -1.0):
        runs.append((bad, mppi_call(s, S, 3.0, np.array([40.0, bad, 40.0]),
                                    0.7, 23)))
    for what, out in runs:
        assert out.best[1].item() == -1, what
        assert out.J_best[1].item() == float("inf"), what
        assert out.J_w[1].item() == float("inf"), what
        assert bool((out.W[1] == 0).all()), what
        assert bool((out.Z[1] == SENTINEL).all() and
                    (out.U[1] == SENTINEL).all()), what
        if what == "nan start":
            assert bool(torch.isnan(out.J[1]).all())
        else:
            assert torch.equal(out.J[1], clean.J[1]), what
        _same_rows(out, clean, (0, 2), NAMES)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_masked_trajectory_is_not_touched(S, dtype):
    """active = [1, 0, 1]: nothing of trajectory 1 is read (its z0, U and lam
    are NaN) or written (every output keeps its fill); the others as without
    the mask, bit for bit."""
    s, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N, wide=False)
    clean = mppi_call(s, S, 3.0, 40.0, 0.7, 24)
    z0, U = s.z0.clone(), s.U.clone()
    z0[1], U[1] = float("nan"), float("nan")
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    out = mppi_call(s, S, 3.0, np.array([40.0, np.nan, 40.0]), 0.7, 24,
                    active=active, z0=z0, U=U)
    for nm in NAMES:
        fill = -9 if nm == "best" else SENTINEL
        assert bool((getattr(out, nm)[1] == fill).all()), nm
    _same_rows(out, clean, (0, 2), NAMES)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_reproducible_and_placeable(S, dtype):
    """The same call twice gives the same bits, with or without the optional
    outputs; another seed gives other weights; trajectories 1.. alone with
    sample_offset + S are what they were in the batch, bit for bit, and
    without the offset they are not."""
    s, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N, wide=False)
    lam = np.array([40.0, 25.0, 60.0])
    a = mppi_call(s, S, 3.0, lam, 0.7, 7)
    b = mppi_call(s, S, 3.0, lam, 0.7, 7)
    _same_rows(a, b, range(B), NAMES)
    lean = mppi_call(s, S, 3.0, lam, 0.7, 7, rows=False, weights=False)
    _same_rows(a, lean, range(B), ("J", "best", "J_best", "J_w"))
    other = mppi_call(s, S, 3.0, lam, 0.7, 8)
    assert torch.equal(other.J[:, 0], a.J[:, 0])
    assert not torch.equal(other.W, a.W)
    tail = mppi_call(s, S, 3.0, lam, 0.7, 7, offset=S, b0=1)
    for nm in NAMES:
        assert torch.equal(getattr(tail, nm), getattr(a, nm)[1:]), nm
    moved = mppi_call(s, S, 3.0, lam, 0.7, 7, offset=0, b0=1)
    assert torch.equal(moved.J[:, 0], a.J[1:, 0])
    assert not torch.equal(moved.W, a.W[1:])


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


def _improved(o):
    return torch.isfinite(o.J_w) & (o.J_w <= o.J[:, 0])


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("table", [False, True], ids=["shared", "table"])
def test_solver_mppi(table, dtype, monkeypatch):
    """ILQRSolver.mppi against the entry point called directly.  adopt=False
    touches nothing and returns the carried rows; three iterations are three
    one-iteration calls with offsets k B S, bit for bit, J_trace
    non-increasing; adopt=True puts the carried rows into U / Z in place,
    re-arms the controller, a rollout reproduces Z and a round runs."""
    s, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N, table=table)
    S, std, lam = 5, 0.3 * BOUND["cartpole"], np.array([300.0, 200.0, 400.0])
    kw = dict(smooth=0.7, seed=9, sample_offset=4)
    s.nominal_rollout()
    s.round()  # (a controller state that is not the re-armed one)
    torch.cuda.synchronize()
    want = mppi_call(s, S, std, lam, 0.7, 9, offset=4)
    imp = _improved(want)
    Z0, U0, before = s.Z.clone(), s.U.clone(), _controller(s)
    addr = (s.Z.data_ptr(), s.U.data_ptr(), s.z0.data_ptr())
    lam_t = torch.from_numpy(lam)

    calls = _Calls(monkeypatch)
    r = s.mppi(S, std, lam_t, adopt=False, **kw)
    monkeypatch.undo()
    assert calls.names == ["pddp_mppi%s_%s" % ("_batch" if table else "",
                                               dtype)], calls.names
    assert r.best.dtype == torch.int32 and r.improved.dtype == torch.bool
    for nm in ("J", "best", "J_best", "W", "J_w"):
        assert torch.equal(getattr(r, nm), getattr(want, nm)), nm
    assert torch.equal(r.improved, imp)
    take = imp.reshape(B, 1, 1)
    assert torch.equal(r.U, torch.where(take, want.U, U0))
    assert torch.equal(r.Z, torch.where(take, want.Z, Z0))
    assert tuple(r.J_trace.shape) == (2, B)
    assert torch.equal(r.J_trace[0], want.J[:, 0])
    assert torch.equal(r.J_trace[1], torch.where(imp, want.J_w, want.J[:, 0]))
    # (1 / sum W^2 lies in [1, S] up to the rounding of W)
    assert bool(((r.ess >= 1 - 1e-6) & (r.ess <= S * (1 + 1e-6))).all()), r.ess
    assert torch.equal(s.Z, Z0) and torch.equal(s.U, U0)
    for k, v in _controller(s).items():
        assert torch.equal(v, before[k]), k

    # three iterations: three one-iteration calls on a second solver
    r3 = s.mppi(S, std, lam_t, iterations=3, adopt=False, **kw)
    assert torch.equal(s.Z, Z0) and torch.equal(s.U, U0)
    t, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N, table=table)
    t.U.copy_(U0)
    t.Z.copy_(Z0)
    trace = [r.J_trace[0]]
    for k in range(3):
        rk = t.mppi(S, std, lam_t, smooth=0.7, seed=9,
                    sample_offset=4 + k * B * S)
        assert not hasattr(rk, "Z")
        trace.append(torch.where(rk.improved, rk.J_w, trace[-1]))
    assert torch.equal(r3.U, t.U) and torch.equal(r3.Z, t.Z)
    for nm in ("J", "best", "J_best", "W", "J_w", "improved", "ess"):
        assert torch.equal(getattr(r3, nm), getattr(rk, nm)), nm
    assert torch.equal(r3.J_trace, torch.stack(trace))
    assert bool((r3.J_trace[1:] <= r3.J_trace[:-1]).all()), r3.J_trace
    print(dtype, table, "J_trace", r3.J_trace.tolist())

    # a scalar temperature is the vector; adopt=True
    one = s.mppi(S, std, torch.full((B,), 300.0), adopt=False, **kw)
    r = s.mppi(S, torch.full((s.m,), std, dtype=torch.float64), 300.0, **kw)
    assert not hasattr(r, "Z")
    for nm in ("J", "best", "J_best", "W", "J_w", "improved"):
        assert torch.equal(getattr(r, nm), getattr(one, nm)), nm
    assert torch.equal(s.U, one.U) and torch.equal(s.Z, one.Z)
    keep = ~r.improved
    assert torch.equal(s.U[keep], U0[keep]) and torch.equal(s.Z[keep],
                                                            Z0[keep])
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
def test_solver_mppi_keeps_rows_without_a_weighted_sequence():
    """adopt=True: a masked trajectory and one without a finite candidate keep
    their U and Z; the masked outputs are NaN / -1 / False."""
    s, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    s.nominal_rollout()
    s.z0[2] = float("nan")
    Z0, U0 = s.Z.clone(), s.U.clone()
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    r = s.mppi(5, 3.0, 300.0, seed=3, active=active)
    assert r.best.tolist()[1:] == [-1, -1] and r.best[0].item() >= 0
    assert bool(torch.isnan(r.J[1]).all() and torch.isnan(r.J_w[1]) and
                torch.isnan(r.W[1]).all())
    assert r.J_w[2].item() == float("inf")
    assert r.improved.tolist()[1:] == [False, False]
    for b in (1, 2):
        assert torch.equal(s.Z[b], Z0[b]) and torch.equal(s.U[b], U0[b]), b


@gpu
def test_solver_mppi_refusals():
    from pddp_amd import _native
    from pddp_amd.controllers.solver import ILQRSolver
    s, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    with pytest.raises(_native.NativeError, match="std"):
        s.mppi(5, torch.ones(3), 1.0)
    with pytest.raises(_native.NativeError, match="temperature"):
        s.mppi(5, 1.0, torch.ones(B + 1))
    with pytest.raises(_native.NativeError, match="samples"):
        s.mppi(0, 1.0, 1.0)
    with pytest.raises(_native.NativeError, match="iterations"):
        s.mppi(5, 1.0, 1.0, iterations=0)
    with pytest.raises(_native.NativeError, match="events"):
        s.mppi(5, 1.0, 1.0, iterations=2, events=(None, None))
    with pytest.raises(_native.NativeError):
        s.mppi(5, 1.0, 1.0, smooth=1.0)
    with pytest.raises(_native.NativeError, match="active"):
        s.mppi(5, 1.0, 1.0, active=torch.ones(B, device="cuda"))
    s.set_batch_weights()
    with pytest.raises(_native.NativeError, match="weights"):
        s.mppi(5, 1.0, 1.0)
    s.clear_batch_weights()
    s.set_reference(torch.zeros(B, N + 1, s.problem.aug_size))
    with pytest.raises(_native.NativeError, match="reference"):
        s.mppi(5, 1.0, 1.0)
    plug = ILQRSolver(None, B, N, torch.float64, "cuda", plugin=object(),
                      n=4, m=1)
    with pytest.raises(_native.NativeError, match="sample problem"):
        plug.mppi(5, 1.0, 1.0)
