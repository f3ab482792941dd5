"""A receding-horizon CEM trial in one launch (pddp_cem_trial_*,
csrc/cem_trial.hip, ILQRSolver.cem_closed_loop).

include/pddp_hip.h is the definition.  Three kinds of test, as
tests/test_mppi_trial.py has them: the kernel against itself bit for bit (one
launch against one launch per control step - the test of the hand-overs of the
mean, the width, the incumbent and z0 inside the launch, where a stale read
shows as a bit - a tail of the batch alone, repetition, masks, continuation);
every stage against a model fed with the DEVICE's previous stage, as
tests/test_cem.py does; and the whole chain in float64 against the oracle and
against the same trial composed from ILQRSolver.cem and pddp_mpc_advance_*."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from abi_util import assert_entry_points, caller, cartpole_pointers
from cem_trial_util import (OPTIONAL, model_trial, model_Z, oracle_costs,
                            selects, trial_call, trial_names)
from cem_util import (model_candidates, model_rank, model_refit,
                      random_sigma)
from golden_util import rel_err
from mppi_trial_util import noise_rows, plant_step, shift, terminal_cost
from mppi_util import model_e, wide_solver
from shoot_util import oracle_rollouts
from solver_util import (BOUND, REARMED, SENTINEL, TOL, mpc_advance, perturbed,
                         record_tol, same_bits, trial_logs)

gpu = pytest.mark.gpu
SYMBOLS = ["pddp_cem_trial_f32", "pddp_cem_trial_f64"]
B, N, T = 5, 6, 3
SMOOTH, MIX = 0.7, 0.25
# tests/test_cem.py's: the smallest elite variance a refitted width is compared
# at (below it sqrt(V) amplifies the sums' rounding), and the width under which
# some float32 cartpole rollouts overflow and others do not
V_FLOOR = 0.01
OVERFLOW_WIDTH = 100.0

# The seeds below were searched on the CPU with `model_trial` under the
# ORACLE's costs, on `_setup`'s configuration (host_inputs' z0 and wide U,
# random_sigma(.., 13, ..), the floor of `_floor`, both noises, the plant of
# perturbed(.., 11), disturbance RandomState(3)); seeds 1, 2, ... in turn, the
# first that holds.
#
# test_one_launch_is_three_launches, I = 2, (S, K) = (5, 3), (70, 8), (300, 32),
# both types, both keep_std settings: some iteration is `better`, and some
# iteration `moved` without being `better`.  Under `_setup`'s widths the
# refit of 8 of 70 or 32 of 300 candidates around these far-from-optimal plans
# is all but always `better`: no seed of 1 .. 79 holds at S = 300, or at S = 70
# with keep_std, where the width narrows from step to step.  With the widths
# three times as large and the floor at BOUND (1 + j) - so that a kept width
# stays as wide as a restarted one - a wide refit around an already improved
# plan is often worse than the plan: seed 1 holds for all twelve cases (2 to
# 21 such iterations of 30 in each; every deciding cost gap of the model above
# 5e-5 relative, the device's cost error being 1e-6 in f32).
HANDOVER_SEED, HANDOVER_WIDTH, HANDOVER_FLOOR = 1, 3.0, 50.0
# test_stages_vs_models, per row of STAGES with I = 1 and K > 1: at most 5 %
# of the model's V entries of the case (all control steps) are below V_FLOOR.
# (Searched with half the cap, 2.5 %; every row not listed: seed 1.  The
# model's counts of entries below V_FLOOR at the seeds taken: 0 .. 2 of 90,
# 0 of 360 for rendezvous.)
STAGE_SEED = {("cartpole", "f64", 5, 3, 1): 5, ("pendulum", "f64", 5, 3, 1): 3,
              ("double_cartpole", "f64", 5, 3, 1): 2}
# test_whole_trial_vs_oracle_f64 (S = 12, K = 4, I = 2): every
# |J_m - J_inc| / |J_inc| and every cost gap at the elite cut exceeds 1e-6
# under both keep_std settings, and some but not every iteration is `better`
# (the smallest gaps at seed 1: 8.3e-5 for cartpole, 5.0e-6 for pendulum).
CHAIN_SEED = {"cartpole": 1, "pendulum": 1}
# test_costs_that_overflow: the horizon and seed at which, with the float32
# oracle on make_solver's inputs, unbounded, S = 70, step 0 / iteration 0 has
# between 1 and S - 1 costs that are not finite on every one of the 5
# trajectories: 25, 20, 18, 18 and 16 at N = 12 (tests/test_cem.py's horizon
# and seed); at N = 6 no rollout overflows yet.
OVERFLOW_N, OVERFLOW_SEED = 12, 31


def _floor(problem, m):
    """std_min [m]: another floor for every component."""
    return 0.02 * BOUND[problem] * (1.0 + np.arange(m))


# ---- CPU -------------------------------------------------------------------
def test_trial_entry_points_are_declared_exported_and_bound():
    """CPU: the two symbols in the header, the built library,
    exported_symbols() and _native._SIGS; 47 arguments, the two doubles at 23
    and 24, the four 64-bit integers at 25, 26, 27 and 31, the ten ints at
    3 .. 10, 32 and 36; the ABI version as it was."""
    from pddp_amd import _native
    assert_entry_points(SYMBOLS)
    sig = _native._SIGS["pddp_cem_trial"]
    assert len(sig) == 47
    at = lambda c: [i for i, x in enumerate(sig) if x is c]  # noqa: E731
    assert at(ctypes.c_double) == [23, 24]
    assert at(ctypes.c_uint64) == [25, 26, 27, 31]
    assert at(ctypes.c_int) == [3, 4, 5, 6, 7, 8, 9, 10, 32, 36]
    assert _native.lib().pddp_hip_abi_version() == 1


def test_trial_entry_points_refuse_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call), both dtypes.  PDDP_E_BADARG: what pddp_mppi_trial_* refuses - a
    null problem, z0, U or Jc, B, N, S of 0 and negative, B S > 0x7fffffff,
    smooth of 1.0, -0.1 and NaN, TT < 1, t0 < 0, count < 1, t0 + count > TT,
    a null Z, Xlog, Ulog or Jcl, v_std without x_true, step_offset < 0,
    step_offset + TT beyond an int; cem's own - K < 1, K > S, mix of 1.0,
    -0.1 and NaN, a null sigma; I < 1; every work buffer null, equal to
    another work buffer and equal to every other pointer of the call.
    PDDP_E_UNSUPPORTED: a DEFAULT-encoding problem.  The non-null pointers are
    host words nobody reads, a word of its own for every work buffer."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    words = (ctypes.c_double * 8)()
    w = [ctypes.addressof(words) + 8 * i for i in range(8)]
    lib = _native.lib()
    for t in ("f32", "f64"):
        #       0      1      2  3  4  5  6  7   8   9      10  11 12
        #       table  plant  B  N  S  K  I  TT  t0  count  z0  U  Z
        good = [None, None, 2, 3, 4, 2, 2, 5, 1, 3, q, q, q,
                # 13    14     15  16  17    18    19     20      21
                # mean  width  Um  Sm  umin  umax  sigma  sigma0  std_min
                w[0], w[1], w[2], w[3], None, None, q, None, None,
                # 22      23   24    25    26      27    28     29
                # smooth  mix  seed  cand  stride  dist  w_std  v_std
                0.5, 0.25, 7, 0, 8, None, None, None,
                # 30    31    32      33   34  35
                # roll  step  x_true  act  Jc  log_costs
                0, 0, None, None, q, 0,
                # 36    37    38   39    40      41  42      43     44
                # Xlog  Ulog  Jcl  Ylog  Jtrace  Jm  nelite  plans  stds
                q, q, q, None, None, None, None, None, None]
        call = caller(getattr(lib, "pddp_cem_trial_" + t), good)
        for i in (10, 11, 19, 34):                 # z0, U, sigma, Jc
            assert call(pp, **{"_%d" % i: None}) == -1, (t, i)
        assert call(None) == -1, t
        for i in (2, 3, 4):                        # B, N, S
            assert call(pp, **{"_%d" % i: 0}) == -1, (t, i)
            assert call(pp, **{"_%d" % i: -3}) == -1, (t, i)
        assert call(pp, _2=1 << 16, _4=1 << 15, _5=1) == -1, t   # B S = 2^31
        for i in (22, 23):                         # smooth, mix
            for bad in (1.0, -0.1, float("nan")):
                assert call(pp, **{"_%d" % i: bad}) == -1, (t, i, bad)
        for i, bad in ((5, 0), (5, -1), (5, 5), (6, 0), (6, -1), (7, 0),
                       (7, -2), (8, -1), (9, 0), (9, -1), (9, 5), (8, 3)):
            assert call(pp, **{"_%d" % i: bad}) == -1, (t, i, bad)
        for i in (12, 36, 37, 38):                 # Z, the logs
            assert call(pp, **{"_%d" % i: None}) == -1, (t, i)
        assert call(pp, _29=q) == -1, t            # v_std without x_true
        assert call(pp, _31=-1) == -1, t           # step_offset
        assert call(pp, _31=(1 << 31) - 5) == -1, t
        # the work buffers: null, each other, every other pointer of the call
        pointers = [0, 1, 10, 11, 12, 17, 18, 19, 20, 21, 27, 28, 29, 32, 33,
                    34, 36, 37, 38, 39, 40, 41, 42, 43, 44]
        for i in (13, 14, 15, 16):
            assert call(pp, **{"_%d" % i: None}) == -1, (t, i)
            for j in (13, 14, 15, 16):
                if j != i:
                    assert call(pp, **{"_%d" % i: good[j]}) == -1, (t, i, j)
            for j in pointers:
                # (x_true next to v_std: the alias is the only fault)
                kw = {"_%d" % i: w[5], "_%d" % j: w[5]}
                if j == 29:
                    kw["_32"] = w[6]
                assert call(pp, **kw) == -1, (t, i, j)
                kw["_%d" % i] = good[i]
                assert call(ppd, **kw) == _native.E_UNSUPPORTED, (t, i, j)
        assert call(ppd) == _native.E_UNSUPPORTED, t
        assert call(ppd, _29=q, _32=q, _39=q, _27=q, _28=q, _0=q, _1=q,
                    _20=q, _21=q) == _native.E_UNSUPPORTED, t


# A tiny problem with costs in closed form for the CPU test of the model: one
# state, one action; a candidate's cost is the squared distance of its actions
# from a target plus y^2, +inf where an action lies inside the HOLE - the
# finite set is not convex, so the mean of finite elites can cost +inf.
TINY = types.SimpleNamespace(B=4, N=2, S=5, K=2, I=3, T=2, target=0.6,
                             hole=(0.25, 0.45), seed=5)


def _in_hole(u):
    return (u > TINY.hole[0]) & (u < TINY.hole[1])


def _tiny_costs(y, Uc):
    J = ((Uc[..., 0] - TINY.target) ** 2).sum(axis=2) + y[:, :1] ** 2
    return np.where(_in_hole(Uc[..., 0]).any(axis=2), np.inf, J)


_TINY_PLANT = (lambda x, u: (0.9 * x + u, (x * x + u * u)[:, 0]),
               lambda x: (2.0 * x * x)[:, 0])


def _restated_trial(keep_std, z0, U, sigma):
    """The law of include/pddp_hip.h once more, trajectory by trajectory in
    plain loops (no cem_util): returns plans, stds, Jtrace, Jm, nelite, z0, U,
    sigma, J."""
    c_ = TINY
    B_, N_, S_, K_, I_, T_ = c_.B, c_.N, c_.S, c_.K, c_.I, c_.T
    step = 1.0 - MIX
    res = types.SimpleNamespace(
        plans=np.empty((B_, T_, N_, 1)), stds=np.empty((B_, T_, N_, 1)),
        Jtrace=np.empty((B_, T_, I_ + 1)), Jm=np.empty((B_, T_, I_)),
        nelite=np.empty((B_, T_, I_), np.int32), z0=np.empty((B_, 1)),
        U=np.empty((B_, N_, 1)), sigma=np.empty((B_, N_, 1)), J=np.empty(B_))

    def cost(y, u):
        if _in_hole(u).any():
            return np.inf
        return float(((u - c_.target) ** 2).sum() + y * y)

    for b in range(B_):
        x, plan, sig, total = float(z0[b, 0]), U[b, :, 0].copy(), \
            sigma[b, :, 0].copy(), 0.0
        for c in range(T_):
            mean, width, inc = plan.copy(), sig.copy(), plan.copy()
            for k in range(I_):
                off = (c * I_ + k) * B_ * S_
                e = model_e(B_, N_, S_, 1, SMOOTH, c_.seed, off, "f64")[b, :, :, 0]
                cands = [mean.copy()] + [mean + width * e[:, s]
                                         for s in range(1, S_)]
                Js = [cost(x, u) for u in cands]
                order = sorted((J, s) for s, J in enumerate(Js)
                               if np.isfinite(J))
                elites = [s for _, s in order[:K_]]
                Ke = len(elites)
                if k == 0:
                    Jinc = Js[0]
                    res.Jtrace[b, c, 0] = Jinc
                Jm = np.inf
                if Ke > 0:
                    s1 = sum(e[:, s] for s in elites if s >= 1) + np.zeros(N_)
                    s2 = sum(e[:, s] ** 2 for s in elites if s >= 1) + \
                        np.zeros(N_)
                    ebar = s1 / Ke
                    V = np.maximum(s2 / Ke - ebar ** 2, 0.0) if Ke > 1 else \
                        np.zeros(N_)
                    Um = mean + step * width * ebar
                    Sm = np.maximum(width + step * (width * np.sqrt(V) -
                                                    width), 0.0)
                    Jm = cost(x, Um)
                    if np.isfinite(Jm) and Jm <= Jinc:
                        inc, Jinc = Um.copy(), Jm
                    mean, width = Um, Sm
                res.Jm[b, c, k], res.nelite[b, c, k] = Jm, Ke
                res.Jtrace[b, c, k + 1] = Jinc
            res.plans[b, c, :, 0], res.stds[b, c, :, 0] = inc, width
            u = inc[0]
            total += x * x + u * u
            x = 0.9 * x + u
            plan = np.append(inc[1:], inc[-1])
            sig = np.append(width[1:], width[-1]) if keep_std else \
                sigma[b, :, 0].copy()
        res.z0[b, 0], res.U[b, :, 0], res.sigma[b, :, 0] = x, plan, sig
        res.J[b] = total + 2.0 * x * x
    return res


@pytest.mark.parametrize("keep_std", [False, True], ids=["restart", "keep"])
def test_numpy_model_of_the_trial(keep_std):
    """CPU: `model_trial` on TINY against `_restated_trial`, every log to
    1e-12 - the integer ones exactly.  The case (its seed searched, 1, 2, ...:
    the first under which all four occur in both modes) has an iteration that
    is `better`, one that `moved` with a finite J_m without being `better`,
    one that `moved` with a J_m that is not finite - so `better` is false
    there whatever J_inc is - and one without a finite cost, which moves
    nothing; with `keep_std` the width a step starts from is the shifted
    refit, without it the caller's."""
    c_ = TINY
    rng = np.random.RandomState(2)
    z0 = rng.uniform(-1, 1, (c_.B, 1))
    U = rng.uniform(-0.3, 0.9, (c_.B, c_.N, 1))
    sigma = rng.uniform(0.2, 0.6, (c_.B, c_.N, 1))
    got = model_trial(_tiny_costs, None, z0, U, sigma, c_.T, c_.K, c_.I, c_.S,
                      SMOOTH, MIX, c_.seed, 0, None, None, keep_std=keep_std,
                      plant=_TINY_PLANT)
    want = _restated_trial(keep_std, z0, U, sigma)
    fin = np.isfinite(got.Jm)
    print("better", got.better.sum(), "moved, finite, not better",
          (got.moved & fin & ~got.better).sum(), "moved, J_m not finite",
          (got.moved & ~fin).sum())
    assert got.better.any()
    assert (got.moved & fin & ~got.better).any()
    assert (got.moved & ~fin).any()
    assert (~got.moved).any()
    assert (got.nelite == want.nelite).all()
    assert (np.isfinite(got.Jm) == np.isfinite(want.Jm)).all()
    for nm in ("plans", "stds", "Jtrace", "Jm", "z0", "U", "sigma", "J"):
        a, b = getattr(got, nm), getattr(want, nm)
        ok = np.isfinite(b)
        assert (a[~ok] == b[~ok]).all(), nm
        assert np.abs(a[ok] - b[ok]).max() < 1e-12, nm
    if keep_std:
        assert np.abs(got.sigma - shift(got.stds[:, -1])).max() == 0
        assert np.abs(got.sigma - sigma).max() > 0
    else:
        assert np.abs(got.sigma - sigma).max() == 0


# ---- GPU: what the tests share ------------------------------------------------
def _np(t):
    return t.cpu().numpy()


def _noise(noise):
    return (0.02 if noise in ("proc", "both") else None,
            0.01 if noise in ("obs", "both") else None)


@functools.lru_cache(maxsize=None)
def _setup(problem, dtype, table, plant, B_=B, N_=N):
    """A solver, its problems, the plants, a width per row, step and component
    and a floor per component."""
    s, ops, z0, U, u_min, u_max = wide_solver(problem, dtype, B_, N_,
                                              table=table)
    c = types.SimpleNamespace(
        s=s, ops=ops, z0=z0, U=U, u_min=u_min, u_max=u_max, dtype=dtype,
        sigma=random_sigma(problem, B_, N_, s.m, 13, dtype),
        floor=_floor(problem, s.m), plant_ops=ops, plant=None)
    if plant:  # (other parameters AND other goals than the controller's)
        par, xg, ug, c.plant_ops = perturbed(problem, B_, 11)
        c.plant = s._plant_table("test", torch.from_numpy(par),
                                 torch.from_numpy(xg), torch.from_numpy(ug))
    rng = np.random.RandomState(3)
    c.dist = torch.from_numpy(0.01 * rng.randn(B_, T, s.n)).to(
        dtype=s.dtype, device="cuda")
    c.dist_np = _np(c.dist).astype(np.float64)
    return c


def _run(c, S, K, I, noise, seed, mix=MIX, wider=1.0, higher=1.0, **kw):
    """The trial on `_setup`'s inputs; `wider`, `higher`: factors on its
    widths and on its floor."""
    w_std, v_std = _noise(noise)
    kw.setdefault("roll", 40)
    return trial_call(c.s, S, K, I, T, wider * c.sigma, SMOOTH, mix, seed,
                      std_min=higher * c.floor, plant=c.plant, dist=c.dist,
                      w_std=w_std, v_std=v_std, step_offset=2, **kw)


def _assert_same(a, b, what, rows=slice(None), rows_b=slice(None)):
    for nm in trial_names(a):
        x, y = getattr(a, nm)[rows], getattr(b, nm)[rows_b]
        assert same_bits(x, y), (what, nm)


def _selects(out):
    return selects(_np(out.Jtrace), _np(out.Jm), _np(out.nelite))


# ---- GPU, the same kernel bit for bit ----------------------------------------
@gpu
@pytest.mark.parametrize("keep_std", [False, True], ids=["restart", "keep"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S,K", [(5, 3), (70, 8), (300, 32)])
def test_one_launch_is_three_launches(S, K, dtype, keep_std):
    """I = 2, both noises, a plant table: count = 3 in one launch against
    three launches with count = 1 and against 2 + 1, every output and log bit
    for bit.  Inside the one launch the lane group reads the mean, the width
    and z0[b] as their head stored them an iteration or a control step
    earlier, and the head the incumbent; between two launches the launch
    boundary hands U, sigma and z0 over.  A stale read shows as a bit.  S = 70
    spans wavefronts; S = 300 takes two turns and carries sums in Um / Sm.
    From the logs: some iteration was `better` and some `moved` without being
    `better` (HANDOVER_SEED and its widths), or the hand-overs were not
    exercised."""
    c = _setup("cartpole", dtype, False, True)
    kw = dict(keep_std=keep_std, wider=HANDOVER_WIDTH, higher=HANDOVER_FLOOR)
    one = _run(c, S, K, 2, "both", HANDOVER_SEED, **kw)
    three = _run(c, S, K, 2, "both", HANDOVER_SEED, chunks=[1, 1, 1], **kw)
    _assert_same(one, three, (S, dtype, keep_std))
    better, moved = _selects(one)
    print(S, K, dtype, keep_std, "better", better.sum(), "moved, not better",
          (moved & ~better).sum(), "of", better.size)
    assert better.any(), "no iteration was better: no incumbent handed over"
    assert (moved & ~better).any(), "the mean never left the incumbent"
    two = _run(c, S, K, 2, "both", HANDOVER_SEED, chunks=[2, 1], **kw)
    _assert_same(one, two, (S, dtype, keep_std, "2 + 1"))


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S,K", [(5, 3), (70, 8)])
def test_tail_of_the_batch_alone(S, K, dtype):
    """Trajectories 2.. alone - the ORIGINAL B S as iter_stride,
    cand_offset + 2 S, rollout_offset + 2 - are their rows of the full run,
    bit for bit; without the candidate offset they are not."""
    c = _setup("cartpole", dtype, True, True)
    full = _run(c, S, K, 2, "both", 5, keep_std=True)
    tail = _run(c, S, K, 2, "both", 5, keep_std=True, b0=2, cand=2 * S,
                roll=42)
    _assert_same(full, tail, (S, dtype), rows=slice(2, None))
    moved = _run(c, S, K, 2, "both", 5, keep_std=True, b0=2, cand=0, roll=42)
    assert same_bits(moved.Jtrace[:, 0, 0], full.Jtrace[2:, 0, 0])
    assert not same_bits(moved.Jc, full.Jc[2:])


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reproducible_and_seeded(dtype):
    """The same call twice gives the same bits, with or without the optional
    logs; another seed gives other candidates and other noise."""
    c = _setup("cartpole", dtype, False, False)
    a, b = (_run(c, 5, 3, 2, "both", 5) for _ in range(2))
    _assert_same(a, b, dtype)
    lean = _run(c, 5, 3, 2, "both", 5, logs=False, log_costs=False)
    for nm in OPTIONAL:
        assert getattr(lean, nm) is None
    for nm in ("z0", "U", "sigma", "Z", "X", "Ulog", "J", "Y", "x_true"):
        assert same_bits(getattr(a, nm), getattr(lean, nm)), nm
    other = _run(c, 5, 3, 2, "both", 6)
    assert same_bits(other.Jtrace[:, 0, 0], a.Jtrace[:, 0, 0])
    assert not same_bits(other.Jc, a.Jc)
    assert not same_bits(other.X[:, 1], a.X[:, 1])


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S,K", [(5, 3), (70, 8)])
def test_masked_trajectories_are_not_touched(S, K, dtype):
    """active = [1, 0, 1, 0, 1]: nothing of trajectories 1 and 3 is read
    (their z0, U and sigma are NaN) or written (every output row, and every
    work buffer's, still holds SENTINEL, z0, U and sigma their NaN); the others
    as without the mask."""
    c = _setup("cartpole", dtype, False, True)
    clean = _run(c, S, K, 2, "both", 5, keep_std=True)
    z0, U = c.s.z0.clone(), c.s.U.clone()
    sigma = torch.from_numpy(c.sigma).to(U)
    off = [1, 3]
    z0[off], U[off], sigma[off] = float("nan"), float("nan"), float("nan")
    active = torch.tensor([1, 0, 1, 0, 1], dtype=torch.uint8, device="cuda")
    w_std, v_std = _noise("both")
    out = trial_call(c.s, S, K, 2, T, sigma, SMOOTH, MIX, 5, keep_std=True,
                     std_min=c.floor, plant=c.plant, dist=c.dist, w_std=w_std,
                     v_std=v_std, roll=40, step_offset=2, active=active, z0=z0,
                     U=U)
    for nm in trial_names(out):
        x = getattr(out, nm)[off]
        if nm in ("z0", "U", "sigma", "x_true"):
            assert bool(torch.isnan(x).all()), nm
        elif nm == "Y":  # (row 0 is the caller's)
            assert bool((x[:, 1:] == SENTINEL).all()), nm
        elif nm == "nelite":
            assert bool((x == -9).all()), nm
        else:
            assert bool((x == SENTINEL).all()), nm
    for wk in out.work:
        assert bool((wk[off] == SENTINEL).all())
    _assert_same(out, clean, (S, dtype), rows=[0, 2, 4], rows_b=[0, 2, 4])


@gpu
@pytest.mark.parametrize("keep_std", [False, True], ids=["restart", "keep"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_four_steps_are_two_and_two_continued(dtype, keep_std):
    """Through the solver, with obs_std and process_std: four steps in one
    call against 2 + 2 - the second call with the first's `std`, z0=None,
    step_offset=2 and candidate_offset advanced by 2 I B S - bit for bit: the
    states, the observations, the actions, every log, and what the solver
    holds afterwards.  (J is not compared: the first call's ends with a
    terminal cost the whole trial does not have there.)"""
    S, K, I = 5, 3, 2
    a, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N)
    b, _, _, _, _, _ = wide_solver("cartpole", dtype, B, N)
    std = torch.from_numpy(random_sigma("cartpole", B, N, a.m, 13, dtype))
    kw = dict(iterations=I, std_min=torch.from_numpy(_floor("cartpole", a.m)),
              mix=MIX, keep_std=keep_std, smooth=SMOOTH, seed=9,
              process_std=0.02, obs_std=0.01, sample_offset=11)
    whole = a.cem_closed_loop(4, S, std, K, candidate_offset=3, **kw)
    first = b.cem_closed_loop(2, S, std, K, candidate_offset=3, **kw)
    x_true = b.x_true
    assert x_true is not None and same_bits(x_true, first.X[:, 2])
    if keep_std:
        assert same_bits(first.std, torch.cat(
            [first.std_steps[:, -1, 1:], first.std_steps[:, -1, -1:]], dim=1))
        assert not same_bits(first.std, std.to(first.std))
    else:
        assert same_bits(first.std, std.to(first.std))
    second = b.cem_closed_loop(2, S, first.std, K, z0=None, step_offset=2,
                               candidate_offset=3 + 2 * I * B * S, **kw)
    assert b.x_true is x_true
    for nm in ("X", "Y"):
        x = getattr(whole, nm)
        assert same_bits(x[:, :3], getattr(first, nm)), nm
        assert same_bits(x[:, 2:], getattr(second, nm)), nm
    for nm in ("U", "J_trace", "J_m", "n_elite", "plans", "std_steps"):
        x = getattr(whole, nm)
        assert same_bits(x[:, :2], getattr(first, nm)), nm
        assert same_bits(x[:, 2:], getattr(second, nm)), nm
    assert same_bits(whole.std, second.std)
    for nm in ("z0", "U", "Z", "x_true"):
        assert same_bits(getattr(a, nm), getattr(b, nm)), nm


# ---- GPU, stage by stage ------------------------------------------------------
#         problem            dtype  S    K   I  table  plant  noise   keep
STAGES = [("cartpole",        "f64", 5,   3,  1, False, True,  "both", False),
          ("cartpole",        "f32", 5,   3,  1, True,  False, "both", True),
          ("pendulum",        "f64", 5,   3,  1, True,  True,  "proc", True),
          ("pendulum",        "f32", 5,   3,  1, False, True,  "obs",  False),
          ("double_cartpole", "f64", 5,   3,  1, False, False, "none", True),
          ("double_cartpole", "f32", 5,   3,  1, True,  True,  "both", False),
          ("rendezvous",      "f64", 70,  8,  1, True,  True,  "both", True),
          ("rendezvous",      "f32", 70,  8,  1, False, False, "proc", False),
          ("cartpole",        "f64", 1,   1,  1, False, False, "none", True),
          ("cartpole",        "f32", 1,   1,  2, False, True,  "obs",  True),
          ("cartpole",        "f64", 70,  8,  2, True,  True,  "both", True),
          ("cartpole",        "f32", 70,  8,  1, False, True,  "none", True),
          ("cartpole",        "f64", 300, 32, 1, False, True,  "proc", False),
          ("cartpole",        "f32", 300, 32, 2, True,  False, "both", True),
          ("cartpole",        "f64", 5,   3,  2, False, False, "obs",  False),
          ("cartpole",        "f32", 5,   3,  2, False, True,  "proc", True)]


@gpu
@pytest.mark.parametrize("problem,dtype,S,K,I,table,plant,noise,keep", STAGES)
def test_stages_vs_models(problem, dtype, S, K, I, table, plant, noise, keep):
    """B = 5, N = 6, 3 steps, bounded, wide base actions (the clamp is met),
    log_costs on.  With y_c = Ylog[:, c] (Xlog[:, c] without measurement
    noise), the mean of step c U_in, then the shift of plan_log[:, c - 1], and
    its width sigma_in, then sigma_in again (restart) or the shift of
    std_log[:, c - 1] (keep):

      Jc[:, c, 0] against the oracle along the model's candidates from (y_c,
             mean, width), rel_err < record_tol;
      nelite_log[:, c, k] exactly, from model_rank of the device's own costs;
      Jtrace_log[..., 0] is Jc[..., 0, 0] exactly; Jtrace_log is monotone
             non-increasing per step where finite; with better =
             isfinite(Jm) & (Jm <= Jtrace before):
      where iteration 0 is the step's last `better` one, plan_log[:, c]
             against model_refit fed with the device's ranks, and Jm_log
             against the oracle stepped along plan_log: rel_err < record_tol;
             where no iteration was `better` plan_log[:, c] is the mean of the
             step exactly;
      I = 1: std_log[:, c] against model_refit under the device's ranks at the
             entries whose model V >= V_FLOOR, rel_err < record_tol; the
             entries below are left out, at most 5 % of the case's
             (STAGE_SEED); exactly the width where nothing `moved`; with K = 1
             (S = 1, mix 0) V is 0 and std_log is std_min exactly;
      Ulog[:, c] is clip(plan_log[:, c, 0]) exactly;
      the plant step, Ylog and Jcl as tests/test_mppi_trial.py holds them -
             TOL["f64"] / record_tol("f32");
      the end: z0 is Ylog[:, T] (Xlog[:, T]), U the shift of the last plan and
             sigma sigma_in (restart) or the shift of the last std_log (keep),
             exactly; Z against the oracle's rollout of clip(U) from z0,
             rel_err < record_tol."""
    c = _setup(problem, dtype, table, plant)
    w_std, v_std = _noise(noise)
    tag = (problem, dtype, S, K, I, table, plant, noise, keep)
    seed = STAGE_SEED.get(tag[:5], 1)
    mix = 0.0 if K == 1 else MIX
    out = _run(c, S, K, I, noise, seed, mix=mix, keep_std=keep)
    n, m, tol = c.s.n, c.s.m, record_tol(dtype)
    bar = TOL["f64"] if dtype == "f64" else record_tol("f32")
    X, Ul, Jc = _np(out.X), _np(out.Ulog), _np(out.Jc)
    Jt, Jm, ne = _np(out.Jtrace), _np(out.Jm), _np(out.nelite)
    plans, stds = _np(out.plans), _np(out.stds)
    seen = _np(out.Y) if v_std is not None else X
    assert same_bits(out.Jtrace[..., 0], out.Jc[:, :, 0, 0]), tag
    better, moved = selects(Jt, Jm, ne)
    print(tag, "better", better.mean(), "moved", moved.mean())
    d = np.diff(Jt, axis=2)
    assert (d[np.isfinite(d)] <= 0).all(), (tag, Jt)
    wn = noise_rows(B, T, n, 0, seed, 40, 2, dtype)
    vn = noise_rows(B, T, n, 1, seed, 40, 2, dtype)
    Jcl = np.zeros(B)
    mean, width = c.U, c.sigma
    left_out, entries = 0, 0
    for step in range(T):
        y = seen[:, step]
        off = step * I * B * S
        e = model_e(B, N, S, m, SMOOTH, seed, off, dtype)
        Uc, _ = model_candidates(mean, width, e, c.u_min, c.u_max)
        _, J = oracle_rollouts(c.ops, y, Uc, dtype)
        for k in range(I):
            rank, _, Ke = model_rank(Jc[:, step, k], K)
            assert (ne[:, step, k] == Ke).all(), (tag, step, k, ne, Ke)
            if k == 0:
                rank0 = rank
        Um, Sm, V = model_refit(mean, width, e, rank0, K, mix, dtype, c.floor,
                                c.u_min, c.u_max)
        _, Jp = oracle_rollouts(c.ops, y, plans[:, step][:, None], dtype)
        for b in range(B):
            err = rel_err(Jc[b, step, 0], J[b])
            print(tag, step, b, "Jc off by", err)
            assert err < tol, (tag, step, b, err)
            if not better[b, step].any():
                assert plans[b, step].tobytes() == \
                    mean[b].astype(plans.dtype).tobytes(), (tag, step, b)
            elif better[b, step, 0] and not better[b, step, 1:].any():
                err = (rel_err(plans[b, step], Um[b]),
                       rel_err(Jm[b, step, 0], Jp[b, 0]))
                print(tag, step, b, "plan, J_m off by", err)
                assert max(err) < tol, (tag, step, b, err)
        if I == 1:
            for b in range(B):
                if not moved[b, step, 0]:
                    assert stds[b, step].tobytes() == \
                        width[b].astype(stds.dtype).tobytes(), (tag, step, b)
                elif K == 1:
                    assert (V[b] == 0).all(), (tag, step, b)
                    assert (stds[b, step] == c.floor.astype(stds.dtype)).all(), \
                        (tag, step, b, stds[b, step])
                else:
                    ok = V[b] >= V_FLOOR
                    left_out += (~ok).sum()
                    entries += ok.size
                    err = rel_err(stds[b, step][ok], Sm[b][ok])
                    print(tag, step, b, "std_log off by", err)
                    assert err < tol, (tag, step, b, err)
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
        mean = shift(plans[:, step]).astype(np.float64)
        width = shift(stds[:, step]).astype(np.float64) if keep else c.sigma
    if entries:
        print(tag, "std_log entries left out:", left_out, "of", entries)
        assert left_out <= 0.05 * entries, (tag, left_out, entries)
    if S == 1:  # the mean is the only candidate: the plan never changes
        want = c.U
        for step in range(T):
            assert (plans[:, step] == want.astype(plans.dtype)).all(), tag
            want = shift(want)
    if v_std is not None:
        assert same_bits(out.x_true, out.X[:, T]), tag
    Jcl += terminal_cost(c.plant_ops, X[:, T], dtype)
    err = rel_err(_np(out.J), Jcl)
    print(tag, "Jcl off by", err)
    assert err < bar, (tag, err)
    assert _np(out.z0).tobytes() == seen[:, T].tobytes(), tag
    assert _np(out.U).tobytes() == mean.astype(plans.dtype).tobytes(), tag
    assert _np(out.sigma).tobytes() == width.astype(stds.dtype).tobytes(), tag
    Zm, _ = oracle_rollouts(c.ops, seen[:, T],
                            np.clip(mean, c.u_min, c.u_max)[:, None], dtype)
    err = rel_err(_np(out.Z), Zm[:, 0])
    print(tag, "Z off by", err)
    assert err < tol, (tag, err)


@gpu
def test_costs_that_overflow():
    """Cartpole, float32, unbounded, S = 70, K = 60, I = 2, every width
    OVERFLOW_WIDTH, make_solver's inputs at N = OVERFLOW_N: from the device's
    Jc, step 0 / iteration 0 has both finite and non-finite costs on every
    trajectory; n_elite = min(K, finite costs) in every iteration; the
    incumbent is never worse than the step's start, so the trial's X and J
    stay finite."""
    S, K, I = 70, 60, 2
    s, _, _, _, _, _ = wide_solver("cartpole", "f32", B, OVERFLOW_N,
                                   wide=False)
    out = trial_call(s, S, K, I, T, OVERFLOW_WIDTH, SMOOTH, 0.0,
                     OVERFLOW_SEED, keep_std=True, bounded=False)
    Jc = _np(out.Jc)
    bad = (~np.isfinite(Jc[:, 0, 0])).sum(axis=1)
    print("costs that are not finite:", bad.tolist())
    assert ((bad >= 1) & (bad <= S - 1)).all(), bad
    fin = np.isfinite(Jc).sum(axis=3)
    assert (_np(out.nelite) == np.minimum(K, fin)).all(), (out.nelite, fin)
    assert (_np(out.nelite) < K).any()
    assert bool(torch.isfinite(out.X).all()) and \
        bool(torch.isfinite(out.J).all()), (out.X, out.J)


# ---- GPU, the whole chain in float64 ------------------------------------------
@gpu
@pytest.mark.parametrize("keep_std", [False, True], ids=["restart", "keep"])
@pytest.mark.parametrize("problem", ["cartpole", "pendulum"])
def test_whole_trial_vs_oracle_f64(problem, keep_std):
    """steps = 3, S = 12, K = 4, I = 2, both noises, a plant table: every log
    against `model_trial` under the oracle's costs at TOL["f64"].  The model
    asserts that every |J_m - J_inc| and every cost gap at the elite cut it
    meets exceeds 1e-6 relative (CHAIN_SEED) - the chain's only
    discontinuities, which the device's cost error (1e-10 relative) then
    cannot turn."""
    s, ops, z0, U, u_min, u_max = wide_solver(problem, "f64", B, N)
    S, K, I, seed = 12, 4, 2, CHAIN_SEED[problem]
    sigma = random_sigma(problem, B, N, s.m, 13, "f64")
    floor = _floor(problem, s.m)
    par, xg, ug, plant_ops = perturbed(problem, B, 11)
    plant = s._plant_table("test", torch.from_numpy(par), torch.from_numpy(xg),
                           torch.from_numpy(ug))
    dist = 0.01 * np.random.RandomState(3).randn(B, T, s.n)
    kw = dict(w_std=0.02, v_std=0.01, roll=40, step_offset=2,
              keep_std=keep_std, std_min=floor)
    want = model_trial(oracle_costs(ops, "f64"), plant_ops, z0, U, sigma, T,
                       K, I, S, SMOOTH, MIX, seed, 0, u_min, u_max, dist=dist,
                       min_gap=1e-6, **kw)
    print(problem, "smallest gaps of the model:", want.gap_inc, want.gap_cut)
    out = trial_call(s, S, K, I, T, sigma, SMOOTH, MIX, seed, plant=plant,
                     dist=torch.from_numpy(dist).cuda(), **kw)
    better, moved = _selects(out)
    assert (better == want.better).all(), (better, want.better)
    assert (_np(out.nelite) == want.nelite).all()
    assert better.any() and not better.all(), better
    want.Z = model_Z(ops, want, u_min, u_max, "f64")
    for nm in ("Jc", "Jtrace", "Jm", "plans", "stds", "Ulog", "X", "Y", "J",
               "z0", "U", "sigma", "Z", "x_true"):
        err = rel_err(_np(getattr(out, nm)), getattr(want, nm))
        print(problem, keep_std, nm, "off by", err)
        assert err < TOL["f64"], (problem, nm, err)


# ---- GPU, against what exists ---------------------------------------------------
@gpu
@pytest.mark.parametrize("table", [False, True], ids=["shared", "table"])
def test_solver_method_vs_composed_host_loop_f64(table):
    """ILQRSolver.cem_closed_loop(3 steps, I = 2, keep_std=False) against the
    same trial composed from what existed: per control step cem(iterations=2,
    sample_offset=candidate_offset + c I B S, adopt=True), then
    pddp_mpc_advance_* - at TOL["f64"] (two kernels' costs agree to rounding,
    not to the bit).  The method makes ONE pddp_cem_trial_* call and no
    pddp_cem_f* or pddp_mpc_advance* call; afterwards the controller words are
    the re-armed ones, U / z0 / Z are the buffers they were, Z is
    nominal_rollout()'s within record_tol and two rounds run."""
    from pddp_amd import _native
    S, K, I = 12, 4, 2
    s, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N, table=table)
    t, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N, table=table)
    std = torch.from_numpy(random_sigma("cartpole", B, N, s.m, 13, "f64"))
    fl = torch.from_numpy(_floor("cartpole", s.m))
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
        r = s.cem_closed_loop(T, S, std, K, iterations=I, std_min=fl, mix=MIX,
                              smooth=SMOOTH, seed=9, candidate_offset=4,
                              disturbance=dist, log_costs=True, **plant)
    finally:
        _native.call = real
    torch.cuda.synchronize()
    assert names.count("pddp_cem_trial") == 1, names
    assert not [x for x in names if x in ("pddp_cem", "pddp_cem_batch") or
                x.startswith("pddp_mpc_advance")], names
    assert r.Y is None and r.n_elite.dtype == torch.int32
    assert tuple(r.Jc.shape) == (B, T, I, S)
    assert tuple(r.J_trace.shape) == (B, T, I + 1)
    assert same_bits(r.J_trace[..., 0], r.Jc[:, :, 0, 0])
    assert same_bits(r.std, std.to(r.std))
    assert bool((r.n_elite == K).all()), r.n_elite

    logs = trial_logs(t, T, 0.0)
    plant_t = t._plant_table("test", **plant)
    dist_t = dist.to(device="cuda").contiguous()
    t.nominal_rollout()
    for c in range(T):
        o = t.cem(S, std, K, iterations=I, std_min=fl, mix=MIX, smooth=SMOOTH,
                  seed=9, sample_offset=4 + c * I * B * S, adopt=True)
        err = rel_err(_np(r.J_trace[:, c]), _np(o.J_trace.T))
        print(table, c, "J_trace off the composed loop by", err)
        assert err < TOL["f64"], (c, err)
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
def test_noise_is_mpc_closed_loops():
    """f64, process noise alone, no plant table: X[:, c + 1] - f(X[:, c],
    U[:, c]) is process_std times the normals closed_loop_draws(1, "process",
    seed, sample_offset, steps=) returns at rows step_offset + c - the ones an
    mpc_closed_loop trial with the same three values runs under.  The bar:
    TOL["f64"] of the largest state."""
    s, ops, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    r = s.cem_closed_loop(T, 5, 0.3 * BOUND["cartpole"], 3, seed=13,
                          process_std=0.05, sample_offset=7, step_offset=2)
    W = _np(s.closed_loop_draws(1, "process", 13, 7, steps=T + 2)[:, :, 0])
    X, U = _np(r.X), _np(r.U)
    for c in range(T):
        xn, _ = plant_step(ops, X[:, c], U[:, c], "f64")
        err = np.abs(X[:, c + 1] - xn - 0.05 * W[:, 2 + c]).max()
        print(c, "noise off by", err)
        assert err < TOL["f64"] * np.abs(X).max(), (c, err)


@gpu
def test_solver_refusals():
    """The solver's own refusals: shapes, counts, the mask, smooth and mix
    (the entry point's), a reference and per-trajectory weights under both
    objectives; objective="search" with neither set is the call "shared"
    makes; a plugin solver has no sample problem."""
    from pddp_amd import _native
    from pddp_amd.controllers.solver import ILQRSolver
    s, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    bad = pytest.raises
    with bad(_native.NativeError, match="std"):
        s.cem_closed_loop(2, 5, torch.ones(3), 2)
    with bad(_native.NativeError, match="std"):
        s.cem_closed_loop(2, 5, torch.ones(B, N + 1, s.m), 2)
    with bad(_native.NativeError, match="std"):
        s.cem_closed_loop(2, 5, 1.0, 2, std_min=torch.ones(3))
    with bad(_native.NativeError, match="samples"):
        s.cem_closed_loop(2, 0, 1.0, 1)
    for K in (0, 6):
        with bad(_native.NativeError, match="elites"):
            s.cem_closed_loop(2, 5, 1.0, K)
    with bad(_native.NativeError, match="iterations"):
        s.cem_closed_loop(2, 5, 1.0, 2, iterations=0)
    with bad(_native.NativeError, match="steps"):
        s.cem_closed_loop(0, 5, 1.0, 2)
    with bad(_native.NativeError):
        s.cem_closed_loop(2, 5, 1.0, 2, smooth=1.0)
    with bad(_native.NativeError):
        s.cem_closed_loop(2, 5, 1.0, 2, mix=1.0)
    with bad(_native.NativeError, match="objective"):
        s.cem_closed_loop(2, 5, 1.0, 2, objective="other")
    with bad(_native.NativeError, match="active"):
        s.cem_closed_loop(2, 5, 1.0, 2, active=torch.ones(B, device="cuda"))
    with bad(_native.NativeError, match="step_offset"):
        s.cem_closed_loop(2, 5, 1.0, 2, step_offset=-1)
    with bad(_native.NativeError, match="z0"):
        s.cem_closed_loop(2, 5, 1.0, 2, z0=torch.zeros(B, s.n + 1))
    with bad(_native.NativeError, match="disturbance"):
        s.cem_closed_loop(2, 5, 1.0, 2, disturbance=torch.zeros(B, 3, s.n))
    z0, U = s.z0.clone(), s.U.clone()
    a = s.cem_closed_loop(2, 5, 1.0, 2, seed=4)
    s.set_nominal(z0, U)
    b = s.cem_closed_loop(2, 5, 1.0, 2, seed=4, objective="search")
    for nm in ("X", "U", "J", "J_trace", "J_m", "plans", "std_steps", "std"):
        assert same_bits(getattr(a, nm), getattr(b, nm)), nm
    s.set_batch_weights()
    with bad(_native.NativeError, match="weights"):
        s.cem_closed_loop(2, 5, 1.0, 2)
    with bad(_native.NativeError, match="not built yet"):
        s.cem_closed_loop(2, 5, 1.0, 2, objective="search")
    s.clear_batch_weights()
    s.set_reference(torch.zeros(B, N + 1, s.problem.aug_size))
    with bad(_native.NativeError, match="reference"):
        s.cem_closed_loop(2, 5, 1.0, 2)
    with bad(_native.NativeError, match="not built yet"):
        s.cem_closed_loop(2, 5, 1.0, 2, objective="search")
    plug = ILQRSolver(None, B, N, torch.float64, "cuda", plugin=object(),
                      n=4, m=1)
    with bad(_native.NativeError, match="sample problem"):
        plug.cem_closed_loop(2, 5, 1.0, 2)


@gpu
def test_solver_masked_rows_are_nan():
    """active through the solver: the outputs of a masked trajectory are NaN
    (n_elite 0, std the width given), its z0 and U stay, the others are what
    they are without the mask."""
    a, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    b, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
    active = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device="cuda")
    z0, U = b.z0.clone(), b.U.clone()
    kw = dict(iterations=2, seed=5, obs_std=0.01, keep_std=True)
    clean = a.cem_closed_loop(T, 5, 3.0, 3, **kw)
    out = b.cem_closed_loop(T, 5, 3.0, 3, active=active, **kw)
    off, on = [1, 4], [0, 2, 3]
    for nm in ("X", "U", "J", "Y", "J_trace", "J_m", "plans", "std_steps"):
        assert bool(torch.isnan(getattr(out, nm)[off]).all()), nm
        assert same_bits(getattr(out, nm)[on], getattr(clean, nm)[on]), nm
    assert bool((out.n_elite[off] == 0).all())
    assert torch.equal(out.n_elite[on], clean.n_elite[on])
    assert bool((out.std[off] == 3.0).all())
    assert same_bits(out.std[on], clean.std[on])
    assert torch.equal(b.z0[off], z0[off]) and torch.equal(b.U[off], U[off])
