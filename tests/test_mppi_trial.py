"""A receding-horizon MPPI trial in one launch (pddp_mppi_trial_*,
csrc/mppi_trial.hip, ILQRSolver.mppi_closed_loop).

include/pddp_hip.h is the definition.  Three kinds of test: the kernel against
itself bit for bit (one launch against one launch per control step - the test
of the hand-over inside the launch, where a stale read shows as a bit - a tail
of the batch alone, repetition, masks); every stage against a model fed with
the DEVICE's previous stage, as tests/test_mppi.py does; and the whole chain in
float64 against the oracle and against the same trial composed from
ILQRSolver.mppi and pddp_mpc_advance_*."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from abi_util import assert_entry_points, caller, cartpole_pointers
from golden_util import rel_err
from mppi_trial_util import (model_trial, noise_rows, plant_step, shift,
                             terminal_cost, trial_call, trial_names)
from mppi_util import (model_e, model_update, model_weights, rounded,
                       wide_solver)
from shoot_util import model_candidates, oracle_rollouts, shoot_call
from solver_util import (BOUND, CONTROLLER, REARMED, SENTINEL, TOL,
                         mpc_advance, perturbed, record_tol, same_bits,
                         trial_logs)

gpu = pytest.mark.gpu
SYMBOLS = ["pddp_mppi_trial_f32", "pddp_mppi_trial_f64"]
B, N, T = 5, 6, 3
SMOOTH, SEED = 0.7, 21
EPS = {"f32": 2.0 ** -23, "f64": 2.0 ** -52}
# tests/test_shoot.py's test_selection_vs_oracle's seeds (B = 3, N = 12),
# searched on the CPU: the oracle's best-to-second gap is decisive there
SELECTION_SEED = {("f64", 5): 4, ("f32", 5): 22, ("f64", 70): 1,
                  ("f32", 70): 1}


# ---- CPU -------------------------------------------------------------------
def test_trial_entry_points_are_declared_exported_and_bound():
    """CPU: the two symbols in the header, the built library,
    exported_symbols() and _native._SIGS; 40 arguments, the double at 18, the
    four 64-bit integers at 19, 20, 21 and 25, the nine ints at 3 .. 9, 26 and
    30; the ABI version as it was."""
    from pddp_amd import _native
    assert_entry_points(SYMBOLS)
    sig = _native._SIGS["pddp_mppi_trial"]
    assert len(sig) == 40
    at = lambda c: [i for i, x in enumerate(sig) if x is c]  # noqa: E731
    assert at(ctypes.c_double) == [18]
    assert at(ctypes.c_uint64) == [19, 20, 21, 25]
    assert at(ctypes.c_int) == [3, 4, 5, 6, 7, 8, 9, 26, 30]
    assert _native.lib().pddp_hip_abi_version() == 1


def test_trial_entry_points_refuse_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call), both dtypes.  PDDP_E_BADARG: pddp_mppi_*'s list - a null problem,
    z0, U, a_std, lam or Jc, B, N, S of 0 and negative, B S > 0x7fffffff,
    smooth of 1.0, -0.1 and NaN - and K < 1, TT < 1, t0 < 0, count < 1,
    t0 + count > TT, a null Z, U_work, Xlog, Ulog or Jcl, U_work == U, v_std
    without x_true, step_offset < 0, step_offset + TT beyond an int;
    PDDP_E_UNSUPPORTED: a DEFAULT-encoding problem.  The non-null pointers are
    host words nobody reads (q and r: two of them, for the aliasing test)."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    r = q + 8
    lib = _native.lib()
    for t in ("f32", "f64"):
        #       0      1      2  3  4  5  6   7   8      9   10 11 12
        #       table  plant  B  N  S  K  TT  t0  count  z0  U  Z  U_work
        good = [None, None, 2, 3, 4, 2, 5, 1, 3, q, q, q, r,
                # 13    14    15    16   17      18    19    20
                # umin  umax  astd  lam  smooth  seed  cand  stride
                None, None, q, q, 0.5, 7, 0, 8,
                # 21    22     23     24    25    26      27   28  29
                # dist  w_std  v_std  roll  step  x_true  act  Jc  log_costs
                None, None, None, 0, 0, None, None, q, 0,
                # 30    31    32   33    34  35  36   37
                # Xlog  Ulog  Jcl  Ylog  J0  Jw  ess  plans
                q, q, q, None, None, None, None, None]
        call = caller(getattr(lib, "pddp_mppi_trial_" + t), good)
        for i in (9, 10, 15, 16, 28):              # pddp_mppi_*'s pointers
            assert call(pp, **{"_%d" % i: None}) == -1, (t, i)
        assert call(None) == -1, t
        for i in (2, 3, 4):                        # B, N, S
            assert call(pp, **{"_%d" % i: 0}) == -1, (t, i)
            assert call(pp, **{"_%d" % i: -3}) == -1, (t, i)
        assert call(pp, _2=1 << 16, _4=1 << 15) == -1, t       # B S = 2^31
        for smooth in (1.0, -0.1, float("nan")):
            assert call(pp, _17=smooth) == -1, (t, smooth)
        for i, bad in ((5, 0), (5, -1), (6, 0), (6, -2), (7, -1), (8, 0),
                       (8, -1), (8, 5), (7, 3)):   # K, TT, t0, count
            assert call(pp, **{"_%d" % i: bad}) == -1, (t, i, bad)
        for i in (11, 12, 30, 31, 32):             # Z, U_work, the logs
            assert call(pp, **{"_%d" % i: None}) == -1, (t, i)
        assert call(pp, _12=q) == -1, t            # U_work == U
        assert call(pp, _23=q) == -1, t            # v_std without x_true
        assert call(pp, _25=-1) == -1, t           # step_offset
        assert call(pp, _25=(1 << 31) - 5) == -1, t
        assert call(ppd) == _native.E_UNSUPPORTED, t
        assert call(ppd, _23=q, _26=q, _33=q, _21=q, _22=q, _0=q, _1=q) \
            == _native.E_UNSUPPORTED, t


# ---- GPU: what the tests share ------------------------------------------------
def _np(t):
    return t.cpu().numpy()


def _lam_of(J):
    """0.5 (median_s J - min_s J) per trajectory, 1 where that is 0 (S = 1)."""
    J = np.asarray(J, np.float64)
    lam = 0.5 * (np.median(J, axis=1) - J.min(axis=1))
    return np.where(lam > 0, lam, 1.0)


def _noise(noise):
    return (0.02 if noise in ("proc", "both") else None,
            0.01 if noise in ("obs", "both") else None)


@functools.lru_cache(maxsize=None)
def _setup(problem, dtype, S, table, plant, B_=B, N_=N):
    """A solver, its problems, the plants and a temperature per trajectory
    from the oracle's costs of the first iteration."""
    s, ops, z0, U, u_min, u_max = wide_solver(problem, dtype, B_, N_,
                                              table=table)
    std = 0.3 * BOUND[problem]
    Uc, _ = model_candidates(U, S, std, SMOOTH, SEED, 0, dtype, u_min, u_max)
    _, J = oracle_rollouts(ops, z0, Uc, dtype)
    c = types.SimpleNamespace(
        s=s, ops=ops, z0=z0, U=U, u_min=u_min, u_max=u_max, dtype=dtype, S=S,
        std=std, lam=rounded(_lam_of(J), dtype), plant_ops=ops, plant=None)
    if plant:  # (other parameters AND other goals than the controller's)
        par, xg, ug, c.plant_ops = perturbed(problem, B_, 11)
        c.plant = s._plant_table("test", torch.from_numpy(par),
                                 torch.from_numpy(xg), torch.from_numpy(ug))
    rng = np.random.RandomState(3)
    c.dist_np = 0.01 * rng.randn(B_, T, s.n)
    c.dist = torch.from_numpy(c.dist_np).to(dtype=s.dtype, device="cuda")
    c.dist_np = _np(c.dist).astype(np.float64)
    return c


def _run(c, K, noise, **kw):
    w_std, v_std = _noise(noise)
    return trial_call(c.s, c.S, K, T, c.std, c.lam, SMOOTH, SEED, plant=c.plant,
                      dist=c.dist, w_std=w_std, v_std=v_std, roll=40,
                      step_offset=2, **kw)


def _assert_same(a, b, what, rows=slice(None), rows_b=slice(None)):
    for nm in trial_names(a):
        x, y = getattr(a, nm)[rows], getattr(b, nm)[rows_b]
        assert same_bits(x, y), (what, nm)


# ---- GPU, the same kernel bit for bit ----------------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70, 300])
def test_one_launch_is_three_launches(S, dtype):
    """K = 2, both noises, a plant table: count = 3 in one launch against
    three launches with count = 1, every output and log bit for bit.  Inside
    the one launch the lane group reads z0[b] and U[b] as their head stored
    them a control step (or an iteration) earlier; between two launches the
    launch boundary hands them over.  A stale read shows as a bit."""
    c = _setup("cartpole", dtype, S, False, True)
    one = _run(c, 2, "both")
    three = _run(c, 2, "both", chunks=[1, 1, 1])
    _assert_same(one, three, (S, dtype))
    took = torch.isfinite(one.Jw) & (one.Jw <= one.J0)
    print(S, dtype, "took", took.float().mean().item())
    assert bool(took.any()), "no iteration took: nothing was handed over"
    two = _run(c, 2, "both", chunks=[2, 1])
    _assert_same(one, two, (S, dtype, "2 + 1"))


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_tail_of_the_batch_alone(S, dtype):
    """Trajectories 2.. alone - the ORIGINAL B S as iter_stride,
    cand_offset + 2 S, rollout_offset + 2 - are their rows of the full run,
    bit for bit; without the candidate offset they are not."""
    c = _setup("cartpole", dtype, S, True, True)
    full = _run(c, 2, "both")
    w_std, v_std = _noise("both")
    kw = dict(plant=c.plant, dist=c.dist, w_std=w_std, v_std=v_std,
              step_offset=2, b0=2)
    tail = trial_call(c.s, S, 2, T, c.std, c.lam, SMOOTH, SEED, cand=2 * S,
                      roll=42, **kw)
    _assert_same(full, tail, (S, dtype), rows=slice(2, None))
    moved = trial_call(c.s, S, 2, T, c.std, c.lam, SMOOTH, SEED, cand=0,
                       roll=42, **kw)
    assert same_bits(moved.J0[:, 0, 0], full.J0[2:, 0, 0])
    if S > 1:
        assert not same_bits(moved.Jc, full.Jc[2:])


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reproducible_and_seeded(dtype):
    """The same call twice gives the same bits, with or without the optional
    logs; another seed gives other candidates and other noise."""
    c = _setup("cartpole", dtype, 5, False, False)
    a, b = _run(c, 2, "both"), _run(c, 2, "both")
    _assert_same(a, b, dtype)
    lean = _run(c, 2, "both", logs=False, log_costs=False)
    for nm in ("z0", "U", "Z", "X", "Ulog", "J", "Y", "x_true"):
        assert same_bits(getattr(a, nm), getattr(lean, nm)), nm
    w_std, v_std = _noise("both")
    other = trial_call(c.s, 5, 2, T, c.std, c.lam, SMOOTH, SEED + 1,
                       dist=c.dist, w_std=w_std, v_std=v_std, roll=40,
                       step_offset=2)
    assert same_bits(other.J0[:, 0, 0], a.J0[:, 0, 0])
    assert not same_bits(other.Jc, a.Jc)
    assert not same_bits(other.X[:, 1], a.X[:, 1])


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_masked_trajectories_are_not_touched(S, dtype):
    """active = [1, 0, 1, 0, 1]: nothing of trajectories 1 and 3 is read
    (their z0, U and lam are NaN) or written (every output row still holds
    SENTINEL, z0 and U their NaN); the others as without the mask."""
    c = _setup("cartpole", dtype, S, False, True)
    clean = _run(c, 2, "both")
    z0, U, lam = c.s.z0.clone(), c.s.U.clone(), c.lam.copy()
    off = [1, 3]
    z0[off], U[off], lam[off] = float("nan"), float("nan"), np.nan
    active = torch.tensor([1, 0, 1, 0, 1], dtype=torch.uint8, device="cuda")
    w_std, v_std = _noise("both")
    out = trial_call(c.s, S, 2, T, c.std, lam, SMOOTH, SEED, plant=c.plant,
                     dist=c.dist, w_std=w_std, v_std=v_std, roll=40,
                     step_offset=2, active=active, z0=z0, U=U)
    for nm in trial_names(out):
        x = getattr(out, nm)[off]
        if nm in ("z0", "U", "x_true"):
            assert bool(torch.isnan(x).all()), nm
        elif nm == "Y":  # (row 0 is the caller's)
            assert bool((x[:, 1:] == SENTINEL).all()), nm
        else:
            assert bool((x == SENTINEL).all()), nm
    _assert_same(out, clean, (S, dtype), rows=[0, 2, 4], rows_b=[0, 2, 4])


# ---- GPU, stage by stage ------------------------------------------------------
#         problem            dtype  S    K  table  plant  noise
STAGES = [("cartpole",        "f64", 5,   1, False, True,  "both"),
          ("cartpole",        "f32", 5,   1, True,  False, "both"),
          ("pendulum",        "f64", 5,   1, True,  True,  "proc"),
          ("pendulum",        "f32", 5,   1, False, True,  "obs"),
          ("double_cartpole", "f64", 5,   1, False, False, "none"),
          ("double_cartpole", "f32", 5,   1, True,  True,  "both"),
          ("rendezvous",      "f64", 70,  1, True,  True,  "both"),
          ("rendezvous",      "f32", 70,  1, False, False, "proc"),
          ("cartpole",        "f64", 1,   1, False, False, "none"),
          ("cartpole",        "f32", 1,   2, False, True,  "obs"),
          ("cartpole",        "f64", 70,  2, True,  True,  "both"),
          ("cartpole",        "f32", 70,  1, False, True,  "none"),
          ("cartpole",        "f64", 300, 1, False, True,  "proc"),
          ("cartpole",        "f32", 300, 2, True,  False, "both"),
          ("cartpole",        "f64", 5,   2, False, False, "obs"),
          ("cartpole",        "f32", 5,   2, False, True,  "proc")]


@gpu
@pytest.mark.parametrize("problem,dtype,S,K,table,plant,noise", STAGES)
def test_stages_vs_models(problem, dtype, S, K, table, plant, noise):
    """B = 5, N = 6, 3 steps, bounded, wide base actions (the clamp is met),
    log_costs on.  With y_c = Ylog[:, c] (Xlog[:, c] without measurement
    noise) and the base of step c U_in, then the shift of plan_log[:, c - 1]:

      K = 1: Jc[:, c, 0] against the oracle along the model's candidates from
             (y_c, base), rel_err < record_tol;
      J0_log is Jc[..., 0] exactly; took = isfinite(Jw) & (Jw <= J0);
      K = 1: plan_log[:, c] where took against model_update fed with the
             device's Jc, rel_err < record_tol, and Jw_log against the oracle
             stepped along plan_log; where no iteration took (any K)
             plan_log[:, c] is the base exactly;
      ess_log against 1 / sum W^2 of the float64 softmin of the device's Jc
             of the last iteration: the bar test_mppi.py holds W to, 32 eps
             absolute per weight, moves sum W^2 by at most 64 eps and
             sum W^2 >= 1 / S, so 64 S eps relative;
      Ulog[:, c] is clip(plan_log[:, c, 0]) exactly;
      the plant step: Xlog[:, c + 1] against the oracle's step of the plant
             from Xlog[:, c] with Ulog[:, c], plus disturbance, plus w_std
             times the model's stream-0 normals; Ylog[:, c + 1] against
             Xlog[:, c + 1] + v_std times the stream-1 normals; Jcl against
             the oracle's costs along Xlog, Ulog under the plant's goals -
             TOL["f64"] / record_tol("f32");
      the end: z0 is Ylog[:, T] (Xlog[:, T]) and U the shift of the last
             plan, exactly; Z against the oracle's rollout of clip(U) from
             z0, rel_err < record_tol."""
    c = _setup(problem, dtype, S, table, plant)
    w_std, v_std = _noise(noise)
    out = _run(c, K, noise)
    tag = (problem, dtype, S, K, table, plant, noise)
    n, m, tol = c.s.n, c.s.m, record_tol(dtype)
    bar = TOL["f64"] if dtype == "f64" else record_tol("f32")
    X, Ul, Jc = _np(out.X), _np(out.Ulog), _np(out.Jc)
    J0, Jw, plans = _np(out.J0), _np(out.Jw), _np(out.plans)
    seen = _np(out.Y) if v_std is not None else X
    assert same_bits(out.J0, out.Jc[..., 0]), tag
    took = np.isfinite(Jw) & (Jw <= J0)
    print(tag, "took", took.mean())
    wn = noise_rows(B, T, n, 0, SEED, 40, 2, dtype)
    vn = noise_rows(B, T, n, 1, SEED, 40, 2, dtype)
    Jcl = np.zeros(B)
    base = c.U
    for step in range(T):
        y = seen[:, step]
        if K == 1:
            off = step * B * S
            Uc, _ = model_candidates(base, S, c.std, SMOOTH, SEED, off, dtype,
                                     c.u_min, c.u_max)
            _, J = oracle_rollouts(c.ops, y, Uc, dtype)
            e = model_e(B, N, S, m, SMOOTH, SEED, off, dtype)
            _, Uw = model_update(base, Jc[:, step, 0], c.lam, e, c.std,
                                 c.u_min, c.u_max)
            _, Jp = oracle_rollouts(c.ops, y, plans[:, step][:, None], dtype)
            for b in range(B):
                err = rel_err(Jc[b, step, 0], J[b])
                print(tag, step, b, "Jc off by", err)
                assert err < tol, (tag, step, b, err)
                if took[b, step, 0]:
                    err = (rel_err(plans[b, step], Uw[b]),
                           rel_err(Jw[b, step, 0], Jp[b, 0]))
                    print(tag, step, b, "plan, J_w off by", err)
                    assert max(err) < tol, (tag, step, b, err)
        for b in range(B):
            if not took[b, step].any():
                assert plans[b, step].tobytes() == base[b].tobytes(), \
                    (tag, step, b)
        W = model_weights(Jc[:, step, K - 1], c.lam)
        W2 = (W * W).sum(axis=1)
        want = np.where(W2 > 0, 1.0 / np.where(W2 > 0, W2, 1.0), 0.0)
        ess = _np(out.ess)[:, step].astype(np.float64)
        err = np.abs(ess - want).max() / max(want.max(), 1.0)
        print(tag, step, "ess off by %.3g (bar %.3g)" % (
            err, 64 * S * EPS[dtype]))
        assert (np.abs(ess - want) <= 64 * S * EPS[dtype] * want).all(), \
            (tag, step, ess, want)
        assert (Ul[:, step] == np.clip(plans[:, step, 0], c.u_min,
                                       c.u_max)).all(), (tag, step)
        xn, cost = plant_step(c.plant_ops, X[:, step], Ul[:, step], dtype)
        xn = xn.astype(np.float64) + c.dist_np[:, step]
        if w_std is not None:
            xn = xn + w_std * wn[:, step]
        Jcl += cost
        err = rel_err(X[:, step + 1], xn)
        print(tag, step, "x' off by", err)
        assert err < bar, (tag, step, err)
        if v_std is not None:
            yn = X[:, step + 1].astype(np.float64) + v_std * vn[:, step + 1]
            err = rel_err(seen[:, step + 1], yn)
            print(tag, step, "y' off by", err)
            assert err < bar, (tag, step, err)
        base = shift(plans[:, step])
    if v_std is not None:
        assert same_bits(out.x_true, out.X[:, T]), tag
    Jcl += terminal_cost(c.plant_ops, X[:, T], dtype)
    err = rel_err(_np(out.J), Jcl)
    print(tag, "Jcl off by", err)
    assert err < bar, (tag, err)
    assert _np(out.z0).tobytes() == seen[:, T].tobytes(), tag
    assert _np(out.U).tobytes() == base.tobytes(), tag
    Zm, _ = oracle_rollouts(c.ops, seen[:, T],
                            np.clip(base, c.u_min, c.u_max)[:, None], dtype)
    err = rel_err(_np(out.Z), Zm[:, 0])
    print(tag, "Z off by", err)
    assert err < tol, (tag, err)


# ---- GPU, the whole chain in float64 ------------------------------------------
# The seed of the candidates, searched on the CPU model (model_trial, seeds
# 0, 1, ...): the first one under which every |J_w - J_0| the trial meets
# exceeds 1e-6 |J_0| on every trajectory, so that the device's cost error
# (1e-10 relative) cannot turn a `took` - the one discontinuity of the chain.
CHAIN_SEED = {"cartpole": 0, "pendulum": 0}


@gpu
@pytest.mark.parametrize("problem", ["cartpole", "pendulum"])
def test_whole_trial_vs_oracle_f64(problem):
    """steps = 3, K = 2, S = 5, both noises, a plant table: every log against
    the numpy / oracle model of the whole trial (candidates -> oracle costs ->
    model_update -> oracle rollout -> took -> plant step) at TOL["f64"].  The
    temperature is the spread of the first iteration's costs (max - min of
    the oracle's, per trajectory), so exp(-(J - J_best) / lam) has a slope of
    at most 1 / lam and amplifies nothing.  The model asserts that every
    |J_w - J_0| it meets exceeds 1e-6 relative (CHAIN_SEED)."""
    s, ops, z0, U, u_min, u_max = wide_solver(problem, "f64", B, N)
    S, K, std, seed = 5, 2, 0.3 * BOUND[problem], CHAIN_SEED[problem]
    par, xg, ug, plant_ops = perturbed(problem, B, 11)
    plant = s._plant_table("test", torch.from_numpy(par), torch.from_numpy(xg),
                           torch.from_numpy(ug))
    Uc, _ = model_candidates(U, S, std, SMOOTH, seed, 0, "f64", u_min, u_max)
    _, J = oracle_rollouts(ops, z0, Uc, "f64")
    lam = J.max(axis=1) - J.min(axis=1)
    dist = 0.01 * np.random.RandomState(3).randn(B, T, s.n)
    kw = dict(w_std=0.02, v_std=0.01, roll=40, step_offset=2)
    want = model_trial(ops, plant_ops, z0, U, T, K, S, std, lam, SMOOTH, seed,
                       0, u_min, u_max, dist=dist, **kw)
    print(problem, "smallest |J_w - J_0| / |J_0| of the model:", want.gap)
    assert want.gap > 1e-6, want.gap
    out = trial_call(s, S, K, T, std, lam, SMOOTH, seed, plant=plant,
                     dist=torch.from_numpy(dist).cuda(), **kw)
    took = _np(torch.isfinite(out.Jw) & (out.Jw <= out.J0))
    assert (took == want.took).all(), (took, want.took)
    assert took.any() and not took.all(), took
    for nm in ("J0", "Jw", "plans", "Ulog", "X", "Y", "J", "z0", "U", "Z",
               "x_true"):
        err = rel_err(_np(getattr(out, nm)), getattr(want, nm))
        print(problem, nm, "off by", err)
        assert err < TOL["f64"], (problem, nm, err)


# ---- GPU, against what exists ---------------------------------------------------
def _controller(s):
    return {k: getattr(s, k).clone() for k in CONTROLLER}


@gpu
@pytest.mark.parametrize("table", [False, True], ids=["shared", "table"])
def test_solver_method_vs_composed_host_loop_f64(table):
    """ILQRSolver.mppi_closed_loop(3 steps, K = 2) against the same trial
    composed from what existed: per control step mppi(iterations=2,
    sample_offset=candidate_offset + c K B S, adopt=True), then
    pddp_mpc_advance_* - at TOL["f64"] (two kernels' costs agree to rounding,
    not to the bit).  The method makes ONE pddp_mppi_trial_* call; afterwards
    the controller words are the re-armed ones, U / z0 / Z are the buffers
    they were, Z is nominal_rollout()'s within record_tol and two rounds
    run."""
    from pddp_amd import _native
    S, K, std, lam = 5, 2, 0.3 * BOUND["cartpole"], 300.0
    s, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N, table=table)
    t, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N, table=table)
    par, xg, ug, _ = perturbed("cartpole", B, 11)
    plant = dict(params=torch.from_numpy(par), x_goal=torch.from_numpy(xg),
                 u_goal=torch.from_numpy(ug))
    dist = 0.01 * torch.from_numpy(np.random.RandomState(3).randn(B, T, s.n))
    s.nominal_rollout()
    s.round()  # (a controller state that is not the re-armed one)
    addr = (s.Z.data_ptr(), s.U.data_ptr(), s.z0.data_ptr())
    names = []
    real = _native.call

    def wrapped(name, dtype, *args):
        names.append(name)
        return real(name, dtype, *args)
    _native.call = wrapped
    try:
        r = s.mppi_closed_loop(T, S, std, lam, iterations=K, smooth=SMOOTH,
                               seed=9, candidate_offset=4, disturbance=dist,
                               log_costs=True, **plant)
    finally:
        _native.call = real
    torch.cuda.synchronize()
    assert names.count("pddp_mppi_trial") == 1, names
    assert not [x for x in names if x.startswith(("pddp_mppi_f", "pddp_mppi_b",
                                                  "pddp_mpc_advance"))], names
    assert r.Y is None and r.took.dtype == torch.bool
    assert tuple(r.Jc.shape) == (B, T, K, S)
    assert torch.equal(r.took, torch.isfinite(r.J_w) & (r.J_w <= r.J0))
    assert same_bits(r.J0, r.Jc[..., 0])
    assert bool(((r.ess >= 1 - 1e-9) & (r.ess <= S * (1 + 1e-9))).all()), r.ess

    logs = trial_logs(t, T, 0.0)
    plant_t = t._plant_table("test", **plant)
    dist_t = dist.to(device="cuda").contiguous()
    t.nominal_rollout()
    for c in range(T):
        t.mppi(S, std, lam, smooth=SMOOTH, seed=9, iterations=K,
               sample_offset=4 + c * K * B * S)
        mpc_advance(t, T, c, logs, plant=plant_t, dist=dist_t)
    pairs = (("X", r.X, logs[0]), ("U", r.U, logs[1]), ("J", r.J, logs[2]),
             ("z0", s.z0, t.z0), ("plan", s.U, t.U), ("Z", s.Z, t.Z))
    for nm, a, b in pairs:
        err = rel_err(_np(a), _np(b))
        print(table, nm, "off the composed loop by", err)
        assert err < TOL["f64"], (nm, err)

    assert addr == (s.Z.data_ptr(), s.U.data_ptr(), s.z0.data_ptr())
    for k, v in REARMED.items():
        assert bool((getattr(s, k) == v).all()), k
    assert s._derivs_due
    Z = s.Z.clone()
    s.nominal_rollout()
    err = rel_err(_np(s.Z), _np(Z))
    print(table, "nominal_rollout() off the trial's Z by", err)
    assert err < record_tol("f64"), err
    s.rounds(2)
    assert bool(torch.isfinite(s.J_opt).all()), s.J_opt


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_four_steps_are_two_and_two_continued(dtype):
    """Through the solver, with obs_std and process_std: four steps in one
    call against 2 + 2 - the second call with z0=None, step_offset=2 and
    candidate_offset advanced by 2 K B S - bit for bit: the states, the
    observations, the actions, every log, and what the solver holds
    afterwards.  (J is not compared: the first call's ends with a terminal
    cost the whole trial does not have there.)"""
    S, K, std, lam = 5, 2, 0.3 * BOUND["cartpole"], 300.0
    kw = dict(iterations=K, smooth=SMOOTH, seed=9, process_std=0.02,
              obs_std=0.01, sample_offset=11)
    a, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N)
    b, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N)
    whole = a.mppi_closed_loop(4, S, std, lam, candidate_offset=3, **kw)
    first = b.mppi_closed_loop(2, S, std, lam, candidate_offset=3, **kw)
    x_true = b.x_true
    assert x_true is not None and same_bits(x_true, first.X[:, 2])
    second = b.mppi_closed_loop(2, S, std, lam, z0=None, step_offset=2,
                                candidate_offset=3 + 2 * K * B * S, **kw)
    assert b.x_true is x_true
    for nm in ("X", "Y"):
        x = getattr(whole, nm)
        assert same_bits(x[:, :3], getattr(first, nm)), nm
        assert same_bits(x[:, 2:], getattr(second, nm)), nm
    for nm in ("U", "J0", "J_w", "took", "ess", "plans"):
        x = getattr(whole, nm)
        assert torch.equal(x[:, :2], getattr(first, nm)), nm
        assert torch.equal(x[:, 2:], getattr(second, nm)), nm
    for nm in ("z0", "U", "Z", "x_true"):
        assert same_bits(getattr(a, nm), getattr(b, nm)), nm


@gpu
def test_noise_is_mpc_closed_loops():
    """f64, process noise alone, no plant table: X[:, c + 1] - f(X[:, c],
    U[:, c]) is process_std times the normals closed_loop_draws(1, "process",
    seed, sample_offset, steps=) returns at rows step_offset + c - the ones an
    mpc_closed_loop trial with the same three values runs under.  The bar:
    TOL["f64"] of the largest state."""
    s, ops, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    r = s.mppi_closed_loop(T, 5, 0.3 * BOUND["cartpole"], 300.0, seed=13,
                           process_std=0.05, sample_offset=7, step_offset=2)
    W = _np(s.closed_loop_draws(1, "process", 13, 7, steps=T + 2)[:, :, 0])
    X, U = _np(r.X), _np(r.U)
    for c in range(T):
        xn, _ = plant_step(ops, X[:, c], U[:, c], "f64")
        err = np.abs(X[:, c + 1] - xn - 0.05 * W[:, 2 + c]).max()
        print(c, "noise off by", err)
        assert err < TOL["f64"] * np.abs(X).max(), (c, err)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_one_hot_limit_gives_shoots_winner(S, dtype):
    """tests/test_mppi.py's test_one_hot_weights_give_shoots_winner, on its
    configuration (B = 3, N = 12) and seeds: with lam a thousandth of the
    smallest best-to-second gap of the device's costs the weights are one-hot,
    and plan_log[:, 0] of a one-step, one-iteration trial has the bits of
    pddp_shoot_*'s U_out on the same arguments."""
    s, ops, z0, U, u_min, u_max = wide_solver("cartpole", dtype, 3, 12)
    std, seed = 0.3 * BOUND["cartpole"], SELECTION_SEED[dtype, S]
    first = trial_call(s, S, 1, 1, std, 1.0, SMOOTH, seed)
    Jd = np.sort(_np(first.Jc[:, 0, 0]).astype(np.float64), axis=1)
    g = (Jd[:, 1] - Jd[:, 0]).min()
    assert g > 0, g
    out = trial_call(s, S, 1, 1, std, g / 1000, SMOOTH, seed)
    shot = shoot_call(s, S, std, SMOOTH, seed)
    # (two units' costs agree to rounding, not to the bit: csrc/Makefile)
    err = rel_err(_np(out.Jc[:, 0, 0]), _np(shot.J))
    assert err < record_tol(dtype), err
    assert torch.equal(out.Jc[:, 0, 0].argmin(dim=1).int(), shot.best)
    print(S, dtype, "best", shot.best.tolist(), "J_w - J_best",
          (out.Jw[:, 0, 0] - shot.J_best).tolist())
    assert bool((shot.best > 0).all()), shot.best
    assert bool((out.ess == 1).all()), out.ess
    assert torch.equal(out.plans[:, 0], shot.U)


@gpu
def test_solver_refusals():
    """The solver's own refusals: shapes, counts, the mask, the smoothing
    (the entry point's), and in mppi's words a reference and per-trajectory
    weights; a plugin solver has no sample problem."""
    from pddp_amd import _native
    from pddp_amd.controllers.solver import ILQRSolver
    s, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    bad = pytest.raises
    with bad(_native.NativeError, match="std"):
        s.mppi_closed_loop(2, 5, torch.ones(3), 1.0)
    with bad(_native.NativeError, match="temperature"):
        s.mppi_closed_loop(2, 5, 1.0, torch.ones(B + 1))
    with bad(_native.NativeError, match="samples"):
        s.mppi_closed_loop(2, 0, 1.0, 1.0)
    with bad(_native.NativeError, match="iterations"):
        s.mppi_closed_loop(2, 5, 1.0, 1.0, iterations=0)
    with bad(_native.NativeError, match="steps"):
        s.mppi_closed_loop(0, 5, 1.0, 1.0)
    with bad(_native.NativeError):
        s.mppi_closed_loop(2, 5, 1.0, 1.0, smooth=1.0)
    with bad(_native.NativeError, match="active"):
        s.mppi_closed_loop(2, 5, 1.0, 1.0, active=torch.ones(B, device="cuda"))
    with bad(_native.NativeError, match="step_offset"):
        s.mppi_closed_loop(2, 5, 1.0, 1.0, step_offset=-1)
    with bad(_native.NativeError, match="z0"):
        s.mppi_closed_loop(2, 5, 1.0, 1.0, z0=torch.zeros(B, s.n + 1))
    with bad(_native.NativeError, match="disturbance"):
        s.mppi_closed_loop(2, 5, 1.0, 1.0, disturbance=torch.zeros(B, 3, s.n))
    s.set_batch_weights()
    with bad(_native.NativeError, match="weights"):
        s.mppi_closed_loop(2, 5, 1.0, 1.0)
    s.clear_batch_weights()
    s.set_reference(torch.zeros(B, N + 1, s.problem.aug_size))
    with bad(_native.NativeError, match="reference"):
        s.mppi_closed_loop(2, 5, 1.0, 1.0)
    plug = ILQRSolver(None, B, N, torch.float64, "cuda", plugin=object(),
                      n=4, m=1)
    with bad(_native.NativeError, match="sample problem"):
        plug.mppi_closed_loop(2, 5, 1.0, 1.0)


@gpu
def test_solver_masked_rows_are_nan():
    """active through the solver: the outputs of a masked trajectory are NaN
    (took False), its z0 and U stay, the others are what they are without the
    mask."""
    a, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    b, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    active = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device="cuda")
    z0, U = b.z0.clone(), b.U.clone()
    kw = dict(iterations=2, seed=5, obs_std=0.01)
    clean = a.mppi_closed_loop(T, 5, 3.0, 300.0, **kw)
    out = b.mppi_closed_loop(T, 5, 3.0, 300.0, active=active, **kw)
    off, on = [1, 4], [0, 2, 3]
    for nm in ("X", "U", "J", "Y", "J0", "J_w", "ess", "plans"):
        assert bool(torch.isnan(getattr(out, nm)[off]).all()), nm
        assert same_bits(getattr(out, nm)[on], getattr(clean, nm)[on]), nm
    assert not bool(out.took[off].any())
    assert torch.equal(b.z0[off], z0[off]) and torch.equal(b.U[off], U[off])
