"""Sampled shooting on the device (pddp_shoot_*, pddp_shoot_batch_*,
pddp_shoot_draws_*, csrc/shoot.hip, ILQRSolver.shoot, ILQRSolver.shoot_draws).

include/pddp_hip.h is the definition; `shoot_util` restates the candidates in
numpy (the stream-2 normals of `solver_util.model_draws`, the AR(1) in float64,
the clamp) and steps the CPU oracle's dynamics and cost along each, in the
run's dtype.  The device's costs, its winner's rows and its choice are checked
against that; the choice also exactly, on the device's own costs."""
import ctypes

import numpy as np
import pytest
import torch

from abi_util import assert_entry_points, caller, cartpole_pointers
from golden_util import rel_err
from shoot_util import (first_argmin, model_ar1, model_candidates,
                        oracle_rollouts, shoot_call, shoot_draws_call)
from solver_util import (BOUND, CONTROLLER, PROBLEMS, REARMED, SENTINEL,
                         make_solver, model_draws, perturbed, record_tol,
                         set_table)

gpu = pytest.mark.gpu
SYMBOLS = ["pddp_shoot_f32", "pddp_shoot_f64", "pddp_shoot_batch_f32",
           "pddp_shoot_batch_f64", "pddp_shoot_draws_f32",
           "pddp_shoot_draws_f64"]
B, N = 3, 12
# test_selection_vs_oracle's seeds, searched on the CPU (its docstring)
SELECTION_SEED = {("f64", 5): 4, ("f32", 5): 22, ("f64", 70): 1,
                  ("f32", 70): 1}


# ---- CPU -------------------------------------------------------------------
def test_shoot_entry_points_are_declared_exported_and_bound():
    """CPU: the six symbols in the header, the built library,
    exported_symbols() and _native._SIGS; where the 64-bit integers sit; the
    ABI version as it was."""
    from pddp_amd import _native
    assert_entry_points(SYMBOLS)
    want = {"pddp_shoot": (19, [10, 11]), "pddp_shoot_batch": (20, [11, 12]),
            "pddp_shoot_draws": (8, [4, 5])}
    for name, (count, at) in want.items():
        sig = _native._SIGS[name]
        assert len(sig) == count, name
        assert [i for i, c in enumerate(sig) if c is ctypes.c_uint64] == at, \
            name
        assert [i for i, c in enumerate(sig) if c is ctypes.c_double] == \
            ([] if name.endswith("draws") else [at[0] - 1]), name
    assert _native.lib().pddp_hip_abi_version() == 1


def test_shoot_entry_points_refuse_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call), both dtypes, both forms.  PDDP_E_BADARG: each null required pointer,
    B, N, S of 0 and negative, B S > 0x7fffffff, one of Z_out / U_out,
    U_out == U, Z_out == z0, smooth of 1.0, -0.1 and NaN, a NULL table on
    _batch; PDDP_E_UNSUPPORTED: a DEFAULT-encoding problem.  Draws: a null E,
    a non-positive size, m > PDDP_MAX_ACTION (4).  The non-null pointers are
    host words nobody reads (q and r: two of them, for the aliasing tests)."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    r = q + 8
    lib = _native.lib()
    for t in ("f32", "f64"):
        #       0  1  2  3   4  5     6     7     8       9     10
        #       B  N  S  z0  U  umin  umax  astd  smooth  seed  off
        good = [2, 3, 4, q, q, None, None, q, 0.5, 7, 0,
                #  11   12  13    14      15     16
                #  act  Jc  best  J_best  Z_out  U_out
                None, q, q, q, r, r]
        plain = caller(getattr(lib, "pddp_shoot_" + t), good)
        batch = caller(getattr(lib, "pddp_shoot_batch_" + t), good)
        forms = ((plain, (pp,), (ppd,), (None,)),
                 (batch, (pp, q), (ppd, q), (None, q)))
        for call, ok, gaussian, no_problem in forms:
            for i in (3, 4, 7, 12, 13):                # required pointers
                assert call(*ok, **{"_%d" % i: None}) == -1, (t, i)
            assert call(*no_problem) == -1, t
            for i in (0, 1, 2):                        # B, N, S
                assert call(*ok, **{"_%d" % i: 0}) == -1, (t, i)
                assert call(*ok, **{"_%d" % i: -3}) == -1, (t, i)
            assert call(*ok, _0=1 << 16, _2=1 << 15) == -1, t   # B S = 2^31
            assert call(*ok, _15=None) == -1, t        # U_out without Z_out
            assert call(*ok, _16=None) == -1, t        # Z_out without U_out
            assert call(*ok, _16=q) == -1, t           # U_out == U
            assert call(*ok, _3=r) == -1, t            # Z_out == z0
            for smooth in (1.0, -0.1, float("nan")):
                assert call(*ok, _8=smooth) == -1, (t, smooth)
            assert call(*gaussian) == _native.E_UNSUPPORTED, t
            assert call(*gaussian, _14=None, _15=None, _16=None) == \
                _native.E_UNSUPPORTED, t
        assert batch(pp, None) == -1, t                # no table

        #        B  N  S  m  seed off E
        dgood = [2, 3, 4, 1, 7, 0, q]
        draws = caller(getattr(lib, "pddp_shoot_draws_" + t), dgood)
        assert draws(_6=None) == -1, t                 # E
        for i in range(4):                             # B, N, S, m
            assert draws(**{"_%d" % i: 0}) == -1, (t, i)
            assert draws(**{"_%d" % i: -1}) == -1, (t, i)
        assert draws(_3=5) == -1, t                    # m > PDDP_MAX_ACTION


def test_numpy_model_of_the_candidates():
    """CPU: the model itself.  With smooth = 0 and std = 0 every candidate is
    the base; candidate 0 is the base at any std; stream 2 is neither stream 0
    nor stream 1; with smooth = 0 e is xi; the AR(1) keeps unit variance: at
    EVERY step t the M = 65 536 values of e_t (independent over b, s and the
    component) have |mean| < 5 / sqrt(M) and |var - 1| < 5 sqrt(2 / M), the
    bounds of test_numpy_model_known_answers, while the lag-1 correlation is
    beta to 5 / sqrt(M)."""
    rng = np.random.RandomState(3)
    U = rng.randn(2, 6, 2)
    for dtype in ("f32", "f64"):
        Uc, hit = model_candidates(U, 5, 0.0, 0.0, 9, 0, dtype)
        assert (Uc == U[:, None]).all() and not hit.any(), dtype
        Uc, hit = model_candidates(U, 5, 0.5, 0.7, 9, 0, dtype, -1.0, 1.0)
        assert (Uc[:, 0] == np.clip(U, -1.0, 1.0)).all(), dtype
        assert (Uc[:, 1:] != np.clip(U, -1.0, 1.0)[:, None]).any(), dtype
        assert hit.any() and not hit.all(), dtype
        w = [model_draws(2, 6, 5, 2, which, 9, 0, dtype) for which in range(3)]
        assert not (w[2] == w[0]).any() and not (w[2] == w[1]).any(), dtype
        assert (model_ar1(w[2], 0.0, dtype) == w[2]).all(), dtype
        Bm, Nm, S, m = 4, 8, 4096, 4
        M = Bm * S * m
        assert M == 65536
        xi = model_draws(Bm, Nm, S, m, 2, 2026, 0, dtype)
        for beta in (0.7, 0.95):
            e = model_ar1(xi, beta, dtype)
            for t in range(Nm):
                print(dtype, beta, t, "mean", e[:, t].mean(), "var",
                      e[:, t].var())
                assert abs(e[:, t].mean()) < 5 / np.sqrt(M), (dtype, beta, t)
                assert abs(e[:, t].var() - 1) < 5 * np.sqrt(2.0 / M), \
                    (dtype, beta, t)
            rho = np.corrcoef(e[:, 1].ravel(), e[:, 2].ravel())[0, 1]
            assert abs(rho - beta) < 5 / np.sqrt(M), (dtype, beta, rho)


# ---- GPU: what the tests share ------------------------------------------------
def _solver(problem, dtype, B_=B, table=False, wide=False):
    """(solver, the oracle's problem of every trajectory, z0, U, u_min,
    u_max): make_solver's, bounded.  `wide`: base actions U(-0.8, 0.8) BOUND,
    so that a perturbation of 0.3 BOUND meets the clamp on many steps.
    `table`: the per-trajectory problems of `perturbed`."""
    s, op, z0, U, u_min, u_max = make_solver(problem, dtype, B_, N)
    if wide:
        rng = np.random.RandomState(5)
        U = (BOUND[problem] * rng.uniform(-0.8, 0.8, U.shape)).astype(U.dtype)
        s.U.copy_(torch.from_numpy(U))
    ops = [op] * B_
    if table:
        par, xg, ug, ops = perturbed(problem, B_, seed=41)
        set_table(s, par, xg, ug)
    return s, ops, z0, U, u_min, u_max


def _check_vs_oracle(s, ops, z0, U, u_min, u_max, dtype, S, std, smooth,
                     seed, tag):
    out = shoot_call(s, S, std, smooth, seed)
    Uc, hit = model_candidates(U, S, std, smooth, seed, 0, dtype, u_min,
                               u_max)
    X, J = oracle_rollouts(ops, z0, Uc, dtype)
    tol = record_tol(dtype)
    best = out.best.cpu().numpy()
    for b in range(s.B):
        assert 0 <= best[b] < S, (tag, b, best[b])
        e = (rel_err(out.J[b].cpu().numpy(), J[b]),
             rel_err(out.Z[b].cpu().numpy(), X[b, best[b]]),
             rel_err(out.U[b].cpu().numpy(), Uc[b, best[b]]))
        print(tag, b, "best", best[b], "J, Z, U off by", e)
        assert max(e) < tol, (tag, b, e)
    return out, hit, J


def _check_selection(out):
    """The choice on the device's own costs: exact."""
    J = out.J.cpu().numpy()
    best = out.best.cpu().numpy()
    assert (best == first_argmin(J)).all(), (best, first_argmin(J))
    for b in range(J.shape[0]):
        if best[b] >= 0:
            assert out.J_best[b].cpu().numpy().tobytes() == \
                J[b, best[b]].tobytes(), b
    assert bool((out.J_best <= out.J[:, 0]).all())


# ---- GPU -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(3, 5, 5, 1), (3, 5, 5, 2), (2, 5, 70, 1)])
def test_shoot_draws_match_the_model(shape, dtype):
    """pddp_shoot_draws_* against the model's stream 2: sample offsets 0, 5
    and 2^32 - 3 (c1 turns non-zero inside the batch).  The bar of
    test_draws_match_the_model: |E - model| <= 32 eps max(1, |model|)."""
    Bd, Nd, S, m = shape
    eps = 2.0 ** -23 if dtype == "f32" else 2.0 ** -52
    for offset in (0, 5, 2 ** 32 - 3):
        E = shoot_draws_call(Bd, Nd, S, m, 2026, offset,
                             dtype).cpu().numpy().astype(np.float64)
        want = model_draws(Bd, Nd, S, m, 2, 2026, offset, dtype)
        dev = (np.abs(E - want) / np.maximum(1.0, np.abs(want))).max()
        print(shape, dtype, offset, "largest deviation: %.2f eps (bar 32)" %
              (dev / eps))
        assert np.isfinite(E).all()
        assert dev <= 32 * eps, (offset, dev / eps)


@gpu
@pytest.mark.parametrize("table", [False, True], ids=["shared", "table"])
@pytest.mark.parametrize("smooth", [0.0, 0.7])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_candidates_vs_oracle(problem, dtype, smooth, table):
    """B = 3, N = 12, S = 5 (5 of 8 lanes, several trajectories to a
    wavefront), bounded, std = 0.3 BOUND around base actions spread over
    0.8 BOUND: the clamp is met on some steps and not on others (asserted from
    the model).  Jc of every candidate, and Z_out / U_out against the model's
    rollout of the device's `best`, within record_tol - the bars of
    test_line_search_vs_oracle for these rollouts at this N.  (The oracle in
    float32 against the oracle in float64 on these candidates, measured on the
    CPU, all four problems, both forms: at most 1.1e-6 relative in J and
    9.7e-7 in the states, so the float32 bar of 2e-4 holds as it stands.)"""
    s, ops, z0, U, u_min, u_max = _solver(problem, dtype, table=table,
                                          wide=True)
    out, hit, _ = _check_vs_oracle(
        s, ops, z0, U, u_min, u_max, dtype, 5, 0.3 * BOUND[problem], smooth,
        21, (problem, dtype, smooth, table))
    assert hit[:, 1:].any() and not hit[:, 1:].all(), hit.mean()
    _check_selection(out)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [1, 70, 300])
def test_wider_shapes(S, dtype):
    """Cartpole.  S = 1: only the base, best == 0 and U_out == clamp(U) bit
    for bit; S = 70: a trajectory over two wavefronts, the argmin through LDS;
    S = 300: a lane runs two rollouts.  All costs and the winner's rows
    against the oracle, the choice exact on the device's costs."""
    s, ops, z0, U, u_min, u_max = _solver("cartpole", dtype, B_=2, wide=True)
    out, _, _ = _check_vs_oracle(s, ops, z0, U, u_min, u_max, dtype, S,
                                 0.3 * BOUND["cartpole"], 0.7, 22,
                                 ("cartpole", dtype, S))
    _check_selection(out)
    if S == 1:
        assert out.best.tolist() == [0, 0]
        assert torch.equal(out.U, torch.minimum(torch.maximum(
            s.U, s.u_min), s.u_max))


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_selection_vs_oracle(S, dtype):
    """Cartpole, B = 3, base actions spread over 0.8 BOUND (a base that a
    perturbation can beat), std = 0.3 BOUND, smooth = 0.7.  The seed
    (SELECTION_SEED) was searched on the CPU so that on EVERY trajectory the
    ORACLE's gap between its best and second-best cost exceeds
    4 record_tol |J_best| - asserted here from the oracle alone - and the
    three winners are three different candidates, none the base.  Then the
    device's `best` is the oracle's argmin, every trajectory."""
    s, ops, z0, U, u_min, u_max = _solver("cartpole", dtype, wide=True)
    std, seed = 0.3 * BOUND["cartpole"], SELECTION_SEED[dtype, S]
    Uc, _ = model_candidates(U, S, std, 0.7, seed, 0, dtype, u_min, u_max)
    _, J = oracle_rollouts(ops, z0, Uc, dtype)
    J = J.astype(np.float64)
    order = np.sort(J, axis=1)
    gap = order[:, 1] - order[:, 0]
    need = 4 * record_tol(dtype) * np.abs(order[:, 0])
    print(dtype, S, "oracle gaps", gap, "needed", need)
    assert (gap > need).all(), (gap, need)
    assert len(set(J.argmin(axis=1))) == B and (J.argmin(axis=1) > 0).all()
    out = shoot_call(s, S, std, 0.7, seed)
    assert (out.best.cpu().numpy() == J.argmin(axis=1)).all(), \
        (out.best.tolist(), J.argmin(axis=1))


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_no_finite_candidate(dtype):
    """Trajectory 1 starts at NaN: best -1, J_best +inf, its rows of Z_out /
    U_out keep the sentinel; the others are what they are without it, bit for
    bit."""
    s, _, _, _, _, _ = _solver("cartpole", dtype)
    clean = shoot_call(s, 5, 3.0, 0.7, 23)
    z0 = s.z0.clone()
    z0[1] = float("nan")
    out = shoot_call(s, 5, 3.0, 0.7, 23, z0=z0)
    assert out.best[1].item() == -1
    assert out.J_best[1].item() == float("inf")
    assert bool(torch.isnan(out.J[1]).all())
    assert bool((out.Z[1] == SENTINEL).all() and (out.U[1] == SENTINEL).all())
    for nm in ("J", "best", "J_best", "Z", "U"):
        a, b = getattr(out, nm), getattr(clean, nm)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), nm
    assert bool((clean.best >= 0).all())


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_masked_trajectory_is_not_touched(S, dtype):
    """active = [1, 0, 1]: nothing of trajectory 1 is read (its z0 and U are
    NaN) or written (every output keeps its fill); the others as without the
    mask, bit for bit."""
    s, _, _, _, _, _ = _solver("cartpole", dtype)
    clean = shoot_call(s, S, 3.0, 0.7, 24)
    z0, U = s.z0.clone(), s.U.clone()
    z0[1], U[1] = float("nan"), float("nan")
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    out = shoot_call(s, S, 3.0, 0.7, 24, active=active, z0=z0, U=U)
    for nm in ("J", "J_best", "Z", "U"):
        assert bool((getattr(out, nm)[1] == SENTINEL).all()), nm
    assert out.best[1].item() == -9
    for nm in ("J", "best", "J_best", "Z", "U"):
        a, b = getattr(out, nm), getattr(clean, nm)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), nm


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_reproducible_and_placeable(S, dtype):
    """The same seed gives the same bits; another seed other candidates but
    the same base; trajectories 1.. alone with sample_offset + S are what they
    were in the batch, bit for bit, and without the offset they are not."""
    s, _, _, _, _, _ = _solver("cartpole", dtype)
    names = ("J", "best", "J_best", "Z", "U")
    a = shoot_call(s, S, 3.0, 0.7, 7)
    b = shoot_call(s, S, 3.0, 0.7, 7)
    for nm in names:
        assert torch.equal(getattr(a, nm), getattr(b, nm)), nm
    lean = shoot_call(s, S, 3.0, 0.7, 7, rows=False)
    for nm in names[:3]:
        assert torch.equal(getattr(a, nm), getattr(lean, nm)), nm
    other = shoot_call(s, S, 3.0, 0.7, 8)
    assert torch.equal(other.J[:, 0], a.J[:, 0])
    assert not bool((other.J[:, 1:] == a.J[:, 1:]).any())
    tail = shoot_call(s, S, 3.0, 0.7, 7, offset=S, b0=1)
    for nm in names:
        assert torch.equal(getattr(tail, nm), getattr(a, nm)[1:]), nm
    moved = shoot_call(s, S, 3.0, 0.7, 7, offset=0, b0=1)
    assert torch.equal(moved.J[:, 0], a.J[1:, 0])
    assert not bool((moved.J[:, 1:] == a.J[1:, 1:]).any())


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
def test_solver_shoot(table, dtype, monkeypatch):
    """ILQRSolver.shoot against the entry point called directly; adopt=False
    touches nothing; adopt=True puts the winners into U / Z in place, re-arms
    the controller, and the nominal it leaves is consistent: a rollout
    reproduces Z, and a round starts from J_best."""
    s, _, _, _, _, _ = _solver("cartpole", dtype, table=table)
    S, std = 5, 3.0
    s.nominal_rollout()
    s.round()  # (a controller state that is not the re-armed one)
    torch.cuda.synchronize()
    want = shoot_call(s, S, std, 0.7, 9, offset=4)
    Z0, U0, before = s.Z.clone(), s.U.clone(), _controller(s)
    addr = (s.Z.data_ptr(), s.U.data_ptr(), s.z0.data_ptr())

    calls = _Calls(monkeypatch)
    r = s.shoot(S, std, smooth=0.7, seed=9, sample_offset=4, adopt=False)
    monkeypatch.undo()
    assert calls.names == ["pddp_shoot%s_%s" % ("_batch" if table else "",
                                                dtype)], calls.names
    assert r.best.dtype == torch.int32
    for nm in ("J", "best", "J_best", "Z", "U"):
        assert torch.equal(getattr(r, nm), getattr(want, nm)), nm
    assert torch.equal(s.Z, Z0) and torch.equal(s.U, U0)
    for k, v in _controller(s).items():
        assert torch.equal(v, before[k]), k

    # a vector std is the scalar; adopt=True
    r = s.shoot(S, torch.full((s.m,), std), smooth=0.7, seed=9,
                sample_offset=4)
    assert not hasattr(r, "Z")
    for nm in ("J", "best", "J_best"):
        assert torch.equal(getattr(r, nm), getattr(want, nm)), nm
    assert torch.equal(s.U, want.U) and torch.equal(s.Z, want.Z)
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
    over = ((s.J_opt - r.J_best) / r.J_best.abs()).max().item()
    print(dtype, table, "J_opt over the adopted J_best by", over)
    assert over <= record_tol(dtype), over


@gpu
def test_solver_shoot_keeps_rows_without_a_winner():
    """adopt=True: a masked trajectory and one without a finite candidate keep
    their U and Z (a device-side select on `best`); the masked outputs are
    NaN / -1."""
    s, _, _, _, _, _ = _solver("cartpole", "f64")
    s.nominal_rollout()
    s.z0[2] = float("nan")
    Z0, U0 = s.Z.clone(), s.U.clone()
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    r = s.shoot(5, 3.0, seed=3, active=active)
    assert r.best.tolist()[1:] == [-1, -1] and r.best[0].item() >= 0
    assert bool(torch.isnan(r.J[1]).all() and torch.isnan(r.J_best[1]))
    assert r.J_best[2].item() == float("inf")
    for b in (1, 2):
        assert torch.equal(s.Z[b], Z0[b]) and torch.equal(s.U[b], U0[b]), b
    assert not torch.equal(s.U[0], U0[0]) or r.best[0].item() == 0
    r = s.shoot(5, 3.0, seed=3, active=active, adopt=False)
    assert bool(torch.isnan(r.Z[1:]).all() and torch.isnan(r.U[1:]).all())


@gpu
def test_solver_shoot_refusals_and_draws():
    from pddp_amd import _native
    from pddp_amd.controllers.solver import ILQRSolver
    s, _, _, _, _, _ = _solver("cartpole", "f64")
    E = s.shoot_draws(5, seed=7, sample_offset=3)
    assert tuple(E.shape) == (B, N, 5, s.m)
    assert torch.equal(E, shoot_draws_call(B, N, 5, s.m, 7, 3, "f64"))
    with pytest.raises(_native.NativeError, match="std"):
        s.shoot(5, torch.ones(3))
    with pytest.raises(_native.NativeError):
        s.shoot(0, 1.0)
    with pytest.raises(_native.NativeError):
        s.shoot(5, 1.0, smooth=1.0)
    with pytest.raises(_native.NativeError, match="active"):
        s.shoot(5, 1.0, active=torch.ones(B, device="cuda"))
    s.set_batch_weights()
    with pytest.raises(_native.NativeError, match="weights"):
        s.shoot(5, 1.0)
    s.clear_batch_weights()
    s.set_reference(torch.zeros(B, N + 1, s.problem.aug_size))
    with pytest.raises(_native.NativeError, match="reference"):
        s.shoot(5, 1.0)
    plug = ILQRSolver(None, B, N, torch.float64, "cuda", plugin=object(),
                      n=4, m=1)
    with pytest.raises(_native.NativeError, match="sample problem"):
        plug.shoot(5, 1.0)
