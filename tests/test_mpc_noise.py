"""Receding-horizon trials under process and measurement noise drawn on the
device (pddp_mpc_advance_noisy_*, pddp_mpc_observe_*,
csrc/mpc_advance_noise.hip, ILQRSolver.mpc_closed_loop(process_std=, obs_std=)).

The law (include/pddp_hip.h): trial b is rollout rollout_offset + b of
pddp_closed_loop_noisy_*'s generator with S = 1, control step t its step
step_offset + t, stream 0 the process and stream 1 the measurement noise.  With
measurement noise the plant's state is `x_true`; z0 / Z[:, 0] hold what the
controller sees.  Every expected value is the CPU oracle stepped under that
law with the numpy model of the draws (solver_util.model_draws), so
a device draw that differs from the model, a draw of the wrong (rollout, step,
stream), or a controller that re-plans from the true state fails here.

Bounds: `record_tol` (1e-10 / 2e-4) where test_closed_loop_noise.py holds the
same draws and dynamics to it; the noise-free trial's own bounds
(test_mpc_closed_loop.py) for the trials."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import oracle as orc
from abi_util import assert_entry_points, caller, cartpole_pointers
from golden_util import DT, np_dtype, rel_err
from solver_util import (BOUND, CONTROLLER, draws_call, loop_solver,
                         make_solver, model_draws, mpc_alphas_np, mpc_inputs,
                         mpc_solver, perturbed, plant_rows, REARMED,
                         record_tol, reference_rows, SENTINEL, set_ref,
                         std_vec, to_device, trial_logs, UNDEFINED)

gpu = pytest.mark.gpu
SYMBOLS = ["pddp_mpc_advance_noisy_f32", "pddp_mpc_advance_noisy_f64",
           "pddp_mpc_observe_f32", "pddp_mpc_observe_f64"]
STD = 0.02
VARIANTS = {"process": (STD, None), "obs": (None, STD), "both": (STD, STD)}
MODELS = ["cartpole", "pendulum", "double_cartpole"]


# ---------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------

def test_mpc_noise_entry_points_are_declared_exported_and_bound():
    """CPU: the four symbols in the header, the built library,
    exported_symbols() and _native._SIGS; the noisy advance takes the tracked
    one's arguments and (w_std, v_std, seed, rollout_offset, step_offset,
    x_true, Ylog) behind `disturbance`."""
    from pddp_amd import _native
    assert_entry_points(SYMBOLS)
    sig = _native._SIGS["pddp_mpc_advance_noisy"]
    assert len(sig) == len(_native._SIGS["pddp_mpc_advance_track"]) + 7 == 37
    assert [i for i, c in enumerate(sig) if c is ctypes.c_uint64] == [18, 19]
    assert sig[20] is ctypes.c_int
    obs = _native._SIGS["pddp_mpc_observe"]
    assert len(obs) == 10
    assert [i for i, c in enumerate(obs) if c is ctypes.c_uint64] == [4, 5]
    assert len(_native._SIGS["pddp_mpc_advance"]) == 27
    assert _native.lib().pddp_hip_abi_version() == 1


def test_mpc_noise_entry_points_refuse_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call), both dtypes.  PDDP_E_BADARG: both stds NULL, v_std with a NULL
    x_true, ref with ref_len = 0 / ref_t0 = -1, a negative step_offset, a null
    required pointer, a non-positive size, t outside [0, T), a null problem;
    PDDP_E_UNSUPPORTED for a DEFAULT-encoding problem.  Observe:
    PDDP_E_BADARG for a null x, v_std or y, B or n < 1, n > PDDP_MAX_STATE (8),
    step < 0.  The non-null pointers are host words nobody reads."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    lib = _native.lib()
    for ty in ("f32", "f64"):
        #       0     1    2    3   4  5  6  7  8   9  10 11    12    13
        #       table ref  len  t0  B  N  T  t  z0  U  Z  u_min u_max plant
        good = [None, None, 0, 0, 2, 3, 4, 0, q, q, q, None, None, None,
                # 14   15 16 17   18  19    20     21   22
                # dist w  v  seed off step0 x_true Ylog mask
                None, q, q, 7, 0, 0, q, None, None,
                # 23   24   25  26        27       28 29    30    31   32
                # Xlog Ulog Jcl state_log live_log mu delta state iter active
                q, q, q, q, q, q, q, q, q, q,
                # 33    34
                # fresh n_live
                q, None]
        call = caller(getattr(lib, "pddp_mpc_advance_noisy_" + ty), good)

        assert call(pp, _15=None, _16=None) == -1, ty   # no noise at all
        assert call(pp, _20=None) == -1, ty             # v_std, no x_true
        assert call(pp, _15=None, _20=None) == -1, ty
        assert call(pp, _1=q, _2=0) == -1, ty           # ref_len
        assert call(pp, _1=q, _2=5, _3=-1) == -1, ty    # ref_t0
        assert call(pp, _19=-1) == -1, ty               # step_offset
        assert call(pp, _19=2 ** 31 - 2) == -1, ty      # (+ T: not an int)
        for required in (8, 9, 10, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,
                         33):
            assert call(pp, **{"_%d" % required: None}) == -1, (ty, required)
        for size in (4, 5, 6):
            assert call(pp, **{"_%d" % size: 0}) == -1, (ty, size)
        assert call(pp, _7=-1) == -1 and call(pp, _7=4) == -1, ty  # t
        assert call(None) == -1, ty
        for change in (dict(), dict(_15=None), dict(_16=None, _20=None),
                       dict(_1=q, _2=5)):
            assert call(ppd, **change) == _native.E_UNSUPPORTED, (ty, change)

        #        B  n  x  v  seed off step mask y
        ogood = [2, 4, q, q, 7, 0, 0, None, q]
        observe = caller(getattr(lib, "pddp_mpc_observe_" + ty), ogood)

        for i in (2, 3, 8):
            assert observe(**{"_%d" % i: None}) == -1, (ty, i)
        for i in (0, 1):
            assert observe(**{"_%d" % i: 0}) == -1, (ty, i)
            assert observe(**{"_%d" % i: -1}) == -1, (ty, i)
        assert observe(_1=9) == -1, ty
        assert observe(_6=-1) == -1, ty


# ---------------------------------------------------------------------------
# the entry points themselves
# ---------------------------------------------------------------------------

def _noisy_advance(s, T, t, logs, w=None, v=None, seed=7, off=0, step0=0,
                   x_true=None, Ylog=None, plant=None, dist=None, mask=None,
                   ref=None, ref_t0=0, b0=0):
    """pddp_mpc_advance_noisy_* on trajectories b0.. of the solver's buffers;
    `logs` as solver_util.trial_logs; w / v: a float for every component
    or None."""
    from pddp_amd import _native
    p = _native.ptr

    def sl(x):
        return None if x is None else x[b0:]

    w_t, v_t = std_vec(s, w), std_vec(s, v)
    ref_args = (None, 0, 0) if ref is None else \
        (p(sl(ref)), ref.shape[1], ref_t0)
    _native.call("pddp_mpc_advance_noisy", s.dtype,
                 ctypes.addressof(s.problem), p(sl(s.batch_table)), *ref_args,
                 s.B - b0, s.N, T, t, p(sl(s.z0)), p(sl(s.U)), p(sl(s.Z)),
                 p(s.u_min), p(s.u_max), p(sl(plant)), p(sl(dist)), p(w_t),
                 p(v_t), seed, off, step0, p(sl(x_true)), p(sl(Ylog)),
                 p(sl(mask)), *[p(sl(x)) for x in logs], p(sl(s.mu)),
                 p(sl(s.delta)), p(sl(s.state)), p(sl(s.iter)),
                 p(sl(s.active)), p(sl(s.fresh)), p(s.n_live), s._s())
    torch.cuda.synchronize()


def _observe(x, v, seed, off, step, mask=None):
    from pddp_amd import _native
    p = _native.ptr
    B, n = x.shape
    v_t = torch.full((n,), v, dtype=x.dtype, device="cuda")
    y = torch.full_like(x, SENTINEL)
    _native.call("pddp_mpc_observe", x.dtype, B, n, p(x), p(v_t), seed, off,
                 step, p(mask), p(y), _native.stream_handle())
    torch.cuda.synchronize()
    return y


def _unit_draws(B, rows, n, which, seed, off, dtype):
    """[B][rows][n] float64: the model's normals of rollouts off .. off+B-1."""
    return model_draws(B, rows, 1, n, which, seed, off, dtype)[:, :, 0]


STATE = CONTROLLER + ("z0", "U", "Z")


def _prepare(s, z0, U):
    """A nominal and two rounds behind it; some trajectories left live."""
    s.set_nominal(torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda())
    s.round(n_iterations=1)
    s.round(n_iterations=1)
    s.active.copy_(torch.arange(s.B, device="cuda") % 2)
    torch.cuda.synchronize()


def _check_noisy_advance(problem, dtype, variant, B=5, N=12, T=3, off=0,
                         step0=0, masked=False, seed=7):
    from pddp_amd import _native
    w, v = VARIANTS[variant]
    d = np_dtype(dtype)
    s, op, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    n = s.n
    rows, plant_ops = plant_rows(problem, B, 1, 11, dtype)
    rows, plant_ops = rows[:, 0], [o[0] for o in plant_ops]
    rng = np.random.RandomState(5)
    dist = rng.uniform(-0.01, 0.01, (B, T, n)).astype(d)
    # (the plant is NOT where the controller believes it to be)
    xt0 = (z0 + rng.uniform(-0.05, 0.05, (B, n))).astype(d)
    mask = None
    if masked:
        mask = np.ones(B, np.uint8)
        mask[B // 2] = 0
    on = np.ones(B, bool) if mask is None else mask.astype(bool)
    Wn = _unit_draws(B, step0 + T + 1, n, 0, seed, off, dtype)
    Vn = _unit_draws(B, step0 + T + 1, n, 1, seed, off, dtype)
    o = orc.load(d)
    tol = record_tol(dtype)
    plant_t, dist_t = to_device(rows, dtype), to_device(dist, dtype)
    mask_t = None if mask is None else torch.from_numpy(mask).cuda()
    t_on = torch.from_numpy(on).cuda()
    for t in (0, T - 1):
        _prepare(s, z0, U)
        assert bool((s.state != UNDEFINED).any())
        s.n_live.fill_(7)
        x_true = to_device(xt0, dtype) if v is not None else None
        Ylog = torch.full((B, T + 1, n), SENTINEL, dtype=s.dtype,
                          device="cuda") if v is not None else None
        pre = {k: getattr(s, k).clone() for k in STATE}
        J0 = 1.5 if t > 0 else SENTINEL
        logs = trial_logs(s, T, J0)
        logs0 = [x.clone() for x in logs]
        _noisy_advance(s, T, t, logs, w, v, seed, off, step0, x_true, Ylog,
                       plant_t, dist_t, mask_t)
        Xlog, Ulog, Jcl, state_log, live_log = (x.cpu().numpy() for x in logs)
        z_pre, U_pre = pre["z0"].cpu().numpy(), pre["U"].cpu().numpy()
        x_pre = xt0 if v is not None else z_pre
        u = np.clip(U_pre[:, 0], u_min, u_max)
        # exact: the logs (of the TRUE state), the shift, the re-armed words
        assert np.array_equal(Ulog[on, t], u[on])
        assert np.array_equal(Xlog[on, t], x_pre[on])
        shifted = np.concatenate([U_pre[:, 1:], U_pre[:, -1:]], 1)
        assert np.array_equal(s.U.cpu().numpy()[on], shifted[on])
        assert np.array_equal(state_log[on, t], pre["state"].cpu().numpy()[on])
        assert np.array_equal(live_log[on, t],
                              (pre["active"].cpu().numpy() != 0)[on])
        for k, val in REARMED.items():
            assert bool((getattr(s, k)[t_on] == val).all()), k
        assert int(s.n_live.abs().sum()) == 0
        other = [i for i in range(T) if i != t]
        assert (Ulog[:, other] == SENTINEL).all()
        keep = [i for i in range(T + 1) if i != t and not
                (i == T and t == T - 1)]
        assert (Xlog[:, keep] == SENTINEL).all()
        z_new = s.z0.cpu().numpy()
        xt_new = x_true.cpu().numpy() if v is not None else z_new
        if v is not None:
            Y = Ylog.cpu().numpy()
            assert np.array_equal(Y[on, t + 1], z_new[on])
            assert (Y[:, [i for i in range(T + 1) if i != t + 1]]
                    == SENTINEL).all()
        # to rounding: the plant step from the true state, the observation,
        # the cost of the true states
        for b in np.nonzero(on)[0]:
            xn = o.dynamics(plant_ops[b], x_pre[b], u[b], jac=False)[0] + \
                dist[b, t]
            if w is not None:
                xn = xn + (w * Wn[b, step0 + t]).astype(d)
            y = xn if v is None else xn + (v * Vn[b, step0 + t + 1]).astype(d)
            L = o.cost(plant_ops[b], x_pre[b], u[b])[0]
            J = L if t == 0 else d(J0) + L
            e = [rel_err(xt_new[b], xn), rel_err(z_new[b], y)]
            if t == T - 1:
                J = J + o.cost(plant_ops[b], xn, None, terminal=True)[0]
                assert np.array_equal(Xlog[b, T], xt_new[b])
            e.append(abs(float(Jcl[b]) - float(J)) / abs(float(J)))
            print(problem, dtype, variant, t, b, e)
            assert max(e) < tol, (t, b, e)
        if v is not None:  # (the noise is there: y is not x)
            assert not np.array_equal(z_new[on], xt_new[on])
        # Z: the rollout from the OBSERVATION under the controller's model
        Z2 = torch.full_like(s.Z, SENTINEL)
        p = _native.ptr
        s._problem_call("pddp_nominal_rollout", B, N, p(s.z0), p(s.U),
                        p(s.u_min), p(s.u_max), None, p(Z2), s._s())
        torch.cuda.synchronize()
        e = rel_err(s.Z[t_on].cpu().numpy(), Z2[t_on].cpu().numpy())
        assert e < tol, (t, e)
        assert torch.equal(s.Z[:, 0], s.z0)
        # a masked trajectory: every word as before the launch
        if (~on).any():
            t_off = ~t_on
            for k in STATE:
                assert torch.equal(getattr(s, k)[t_off], pre[k][t_off]), k
            for x, x0 in zip(logs, logs0):
                assert torch.equal(x[t_off], x0[t_off])
            if v is not None:
                assert torch.equal(x_true[t_off], to_device(xt0, dtype)[t_off])
                assert bool((Ylog[t_off] == SENTINEL).all())


@gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", MODELS)
def test_noisy_advance_vs_oracle(problem, dtype, variant):
    """B = 5, N = 12, T = 3, t in {0, T-1}, perturbed plant rows and a
    disturbance of +-0.01, a true state +-0.05 away from the observed one:
    Xlog, Ulog, Jcl, x_true, z0, Ylog and the rolled-out Z against the oracle
    stepped with model_draws.  n = 2: a partly used draw block; n = 6: more
    than one block."""
    _check_noisy_advance(problem, dtype, variant)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_noisy_advance_second_partial_wavefront(dtype):
    _check_noisy_advance("cartpole", dtype, "both", B=70, off=3, step0=2)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", MODELS)
def test_noisy_advance_leaves_masked_trajectories_untouched(problem, dtype):
    """Skipped trajectories keep every word of z0, x_true, U, Z, the
    controller state, the logs and Ylog."""
    _check_noisy_advance(problem, dtype, "both", masked=True)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_noisy_advance_of_a_part_of_the_batch_is_bit_equal(dtype):
    """rollout_offset = 3, step_offset = 2: the launch on trajectories 1..
    with rollout_offset 4 writes, bit for bit, rows 1.. of the full launch."""
    B, N, T, t = 5, 12, 3, 1
    s, _, z0, U, _, _ = make_solver("cartpole", dtype, B, N)
    xt0 = to_device(z0 + 0.03, dtype)
    got = []
    for b0, off in ((0, 3), (1, 4)):
        _prepare(s, z0, U)
        x_true = xt0.clone()
        Ylog = torch.full((B, T + 1, s.n), SENTINEL, dtype=s.dtype,
                          device="cuda")
        logs = trial_logs(s, T, 1.5)
        _noisy_advance(s, T, t, logs, STD, STD, 7, off, 2, x_true, Ylog,
                       b0=b0)
        got.append([x.clone() for x in
                    [getattr(s, k) for k in STATE] + [x_true, Ylog] +
                    list(logs)])
    for full, part in zip(*got):
        assert torch.equal(full[1:], part[1:])


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", MODELS)
def test_observe_vs_model_and_bit_equal_to_the_advance(problem, dtype):
    """pddp_mpc_observe_* is x + v_std * model_draws within record_tol, leaves a
    masked row alone, and is bit-equal to the y the advance wrote for the same
    (rollout, step) from the same x."""
    B, N, T, t, off, step0 = 70, 6, 3, 1, 5, 2
    s, _, z0, U, _, _ = make_solver(problem, dtype, B, N)
    n = s.n
    x = to_device(z0, dtype)
    mask = torch.ones(B, dtype=torch.uint8, device="cuda")
    mask[3] = 0
    y = _observe(x, STD, 7, off, 4, mask)
    want = z0 + STD * _unit_draws(B, 5, n, 1, 7, off, dtype)[:, 4]
    on = mask.bool().cpu().numpy()
    e = rel_err(y.cpu().numpy()[on], want[on])
    print(problem, dtype, e)
    assert e < record_tol(dtype), e
    assert bool((y[3] == SENTINEL).all())
    assert not torch.equal(y[mask.bool()], x[mask.bool()])
    s.set_nominal(x, torch.from_numpy(U).cuda())
    x_true = x.clone()
    logs = trial_logs(s, T, 1.5)
    _noisy_advance(s, T, t, logs, None, STD, 7, off, step0, x_true)
    assert torch.equal(_observe(x_true, STD, 7, off, step0 + t + 1), s.z0)


# ---------------------------------------------------------------------------
# the trial
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_noisy_trial(problem, B, N, T, w, v, seed):
    """The oracle's MPC loop per trajectory under the noisy law, f64: (X, Y, U,
    states, attempts) - `fit` from y_t, the plant step from x_t, the model's
    normals scaled by the stds; the shared problem as every controller's
    model, the plants `perturbed(problem, B, 11)`'s."""
    o = orc.load(np.float64)
    z0, U0 = mpc_inputs(problem, B, N, False)
    plant_ops = perturbed(problem, B, 11)[3]
    model = orc.make_problem(problem, DT[problem])
    n, m = z0.shape[1], U0.shape[2]
    u_min, u_max = np.full(m, -BOUND[problem]), np.full(m, BOUND[problem])
    alphas = mpc_alphas_np()
    Wn = _unit_draws(B, T + 1, n, 0, seed, 0, "f64")
    Vn = _unit_draws(B, T + 1, n, 1, seed, 0, "f64")
    X, Y = np.empty((B, T + 1, n)), np.empty((B, T + 1, n))
    Ul = np.empty((B, T, m))
    states = np.empty((B, T), np.int32)
    attempts = np.empty((B, T), np.int32)
    for b in range(B):
        x, Uo = z0[b], U0[b]
        y = x if v is None else x + v * Vn[b, 0]
        for t in range(T):
            _, Uo, _, st, trace = o.fit(model, y, Uo, alphas, n_iterations=1,
                                        u_min=u_min, u_max=u_max)
            states[b, t], attempts[b, t] = st, len(trace)
            u = np.clip(Uo[0], u_min, u_max)
            X[b, t], Y[b, t], Ul[b, t] = x, y, u
            x = o.dynamics(plant_ops[b], x, u, jac=False)[0]
            if w is not None:
                x = x + w * Wn[b, t]
            y = x if v is None else x + v * Vn[b, t + 1]
            Uo = np.concatenate([Uo[1:], Uo[-1:]], 0)
        X[b, T], Y[b, T] = x, y
    for a in (X, Y, Ul, states, attempts):
        a.setflags(write=False)
    return X, Y, Ul, states, attempts


TRIAL_SEED, TRIAL_R = 7, 3


@gpu
@pytest.mark.parametrize("problem", ["cartpole", "pendulum"])
def test_noisy_mpc_loop_f64_vs_oracle(problem):
    """B = 5, N = 20, T = 6, std 0.02, both noises: X, U, Y at rtol 1e-8 /
    atol 1e-10 and J at 1e-10 relative against the oracle's trajectory_cost on
    the TRUE states - the noise-free trial's bounds.  A condition of the
    test: the oracle decides every control step within TRIAL_R attempts (it
    takes one for each, under seed 7)."""
    B, N, T = 5, 20, 6
    Xo, Yo, Uo, states, attempts = _oracle_noisy_trial(
        problem, B, N, T, STD, STD, TRIAL_SEED)
    assert (attempts <= TRIAL_R).all(), attempts
    s, kw, plant_ops = mpc_solver(problem, "f64", B, N)
    r = s.mpc_closed_loop(T, TRIAL_R, process_std=STD, obs_std=STD,
                          seed=TRIAL_SEED, **kw)
    torch.cuda.synchronize()
    X, U, Y, J = (a.cpu().numpy() for a in (r.X, r.U, r.Y, r.J))
    assert X.shape == Xo.shape and U.shape == Uo.shape and Y.shape == Yo.shape
    assert int(r.unfinished.sum()) == 0
    assert np.array_equal(r.states.cpu().numpy(), states)
    print("X", np.abs(X - Xo).max(), "Y", np.abs(Y - Yo).max(), "U",
          np.abs(U - Uo).max())
    assert np.allclose(X, Xo, rtol=1e-8, atol=1e-10)
    assert np.allclose(Y, Yo, rtol=1e-8, atol=1e-10)
    assert np.allclose(U, Uo, rtol=1e-8, atol=1e-10)
    o = orc.load(np.float64)
    for b in range(B):
        Jb = o.trajectory_cost(plant_ops[b], X[b][:, None, :],
                               U[b][:, None, :])[0]
        assert abs(J[b] - Jb) <= 1e-10 * abs(Jb), (b, J[b], Jb)
    # the solver afterwards: the plant's state and the last observation
    assert torch.equal(s.x_true, r.X[:, T]) and torch.equal(s.z0, r.Y[:, T])
    assert torch.equal(s.Z[:, 0], s.z0)


@gpu
def test_noisy_mpc_loop_f32_vs_the_composed_trial():
    """cartpole f32, B = 64, N = 25, T = 5, two rounds per step, both noises,
    against the trial composed on a second solver: set_nominal(y_t), round()
    x 2, the plant step from x_t by pddp_nominal_rollout_batch at N = 1, the
    scaled draws of closed_loop_draws(steps=), a torch shift."""
    from pddp_amd import _native
    B, N, T, R, seed = 64, 25, 5, 2, 11
    s, _, z0, U, u_min, u_max = make_solver("cartpole", "f32", B, N)
    s2 = make_solver("cartpole", "f32", B, N)[0]
    par, xg, ug, plant_ops = perturbed("cartpole", B, 11)
    r = s.mpc_closed_loop(T, R, params=torch.from_numpy(par),
                          x_goal=torch.from_numpy(xg),
                          u_goal=torch.from_numpy(ug), process_std=STD,
                          obs_std=STD, seed=seed)
    torch.cuda.synchronize()
    assert s._one_launch is True, "the one-launch round did not apply"
    W = STD * s2.closed_loop_draws(1, "process", seed=seed,
                                   steps=T + 1)[:, :, 0]
    V = STD * s2.closed_loop_draws(1, "obs", seed=seed, steps=T + 1)[:, :, 0]
    rows = to_device(plant_rows("cartpole", B, 1, 11, "f32")[0][:, 0], "f32")
    x = torch.from_numpy(z0).to(dtype=torch.float32, device="cuda")
    Un = torch.from_numpy(U).to(dtype=torch.float32, device="cuda")
    y = x + V[:, 0]
    Xc = torch.empty(B, T + 1, s.n, device="cuda")
    Yc = torch.empty(B, T + 1, s.n, device="cuda")
    Uc = torch.empty(B, T, s.m, device="cuda")
    states = torch.empty(B, T, dtype=torch.int32, device="cuda")
    unfinished = torch.empty(B, T, dtype=torch.uint8, device="cuda")
    step = torch.empty(B, 2, s.n, device="cuda")
    p = _native.ptr
    for t in range(T):
        s2.set_nominal(y, Un)
        for _ in range(R):
            s2.round(n_iterations=1)
        states[:, t], unfinished[:, t] = s2.state, s2.active
        u0 = s2.U[:, :1].contiguous()
        x = x.contiguous()
        _native.call("pddp_nominal_rollout_batch", s2.dtype,
                     ctypes.addressof(s2.problem), p(rows), B, 1, p(x),
                     p(u0), p(s2.u_min), p(s2.u_max), None, p(step), s2._s())
        Xc[:, t], Yc[:, t] = x, y
        Uc[:, t] = torch.minimum(torch.maximum(u0[:, 0], s2.u_min), s2.u_max)
        x = step[:, 1] + W[:, t]
        y = x + V[:, t + 1]
        Un = torch.cat([s2.U[:, 1:], s2.U[:, -1:]], 1)
    Xc[:, T], Yc[:, T] = x, y
    torch.cuda.synchronize()
    same = ((r.states == states) & (r.unfinished == unfinished)).cpu().numpy()
    share = same.mean()
    print("decisions identical on %.1f %% of the (b, t) pairs" % (
        100 * share))
    assert share >= 0.95, share
    agree = same.all(axis=1)
    assert agree.any()
    o = orc.load(np.float64)
    X, Ua, Y, J = (a.cpu().numpy() for a in (r.X, r.U, r.Y, r.J))
    Xc, Uc, Yc = Xc.cpu().numpy(), Uc.cpu().numpy(), Yc.cpu().numpy()
    worst = 0.0
    for b in np.nonzero(agree)[0]:
        Jb = o.trajectory_cost(plant_ops[b],
                               Xc[b][:, None, :].astype(np.float64),
                               Uc[b][:, None, :].astype(np.float64))[0]
        e = (rel_err(X[b], Xc[b]), rel_err(Ua[b], Uc[b]),
             abs(J[b] - Jb) / abs(Jb), rel_err(Y[b], Yc[b]))
        worst = max(worst, max(e))
        assert max(e) < 2e-4, (b, e)
    print("worst of X, U, J, Y on the agreeing trajectories:", worst)


def _trial_outputs(r):
    return [getattr(r, k) for k in ("X", "U", "J", "states", "unfinished")] + \
        ([] if r.Y is None else [r.Y])


@gpu
@pytest.mark.parametrize("problem", ["cartpole", "pendulum"])
def test_noisy_mpc_loop_sees_the_noise_of_closed_loop_draws(problem):
    """f64, process noise only: mpc_closed_loop(process_std=s, seed=7) agrees
    with mpc_closed_loop(disturbance = s * closed_loop_draws(1, "process",
    seed=7, steps=T)[:, :, 0]) at the f64 trial's bounds (two kernels: to
    rounding, not bit for bit)."""
    B, N, T, R = 5, 20, 6, 3
    a, kw, _ = mpc_solver(problem, "f64", B, N)
    ra = a.mpc_closed_loop(T, R, process_std=STD, seed=7, **kw)
    b = mpc_solver(problem, "f64", B, N)[0]
    D = STD * b.closed_loop_draws(1, "process", seed=7, steps=T)[:, :, 0]
    assert tuple(D.shape) == (B, T, a.n)
    rb = b.mpc_closed_loop(T, R, disturbance=D.contiguous(), **kw)
    torch.cuda.synchronize()
    assert ra.Y is None and a.x_true is None
    assert torch.equal(ra.states, rb.states)
    assert torch.equal(ra.unfinished, rb.unfinished)
    for nm in ("X", "U"):
        x, y = getattr(ra, nm).cpu().numpy(), getattr(rb, nm).cpu().numpy()
        print(problem, nm, np.abs(x - y).max())
        assert np.allclose(x, y, rtol=1e-8, atol=1e-10), nm
    Ja, Jb = ra.J.cpu().numpy(), rb.J.cpu().numpy()
    assert (np.abs(Ja - Jb) <= 1e-10 * np.abs(Jb)).all(), (Ja, Jb)
    # (the noise is there)
    c = mpc_solver(problem, "f64", B, N)[0]
    rc = c.mpc_closed_loop(T, R, **kw)
    assert not np.allclose(rc.X.cpu().numpy(), ra.X.cpu().numpy(), rtol=1e-3,
                           atol=1e-5)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_noisy_mpc_loop_is_reproducible(dtype):
    """The same call twice: every output bit for bit; another seed: another X;
    stds of exactly 0: the plain trial within record_tol; both stds None: bit for
    bit the call without the keywords."""
    B, N, T, R = 5, 20, 4, 2
    noise = dict(process_std=STD, obs_std=STD, seed=7)

    def run(**more):
        s, kw, _ = mpc_solver("cartpole", dtype, B, N)
        r = s.mpc_closed_loop(T, R, **dict(kw, **more))
        torch.cuda.synchronize()
        return s, r

    (s1, r1), (s2, r2) = run(**noise), run(**noise)
    for x, y in zip(_trial_outputs(r1), _trial_outputs(r2)):
        assert torch.equal(x, y)
    for nm in STATE + ("x_true",):
        assert torch.equal(getattr(s1, nm), getattr(s2, nm)), nm
    r3 = run(**dict(noise, seed=8))[1]
    assert not torch.equal(r3.X[:, 1:], r1.X[:, 1:])
    assert not torch.equal(r3.Y, r1.Y)
    s0, plain = run()
    sk, keyed = run(process_std=None, obs_std=None, seed=5, sample_offset=2,
                    step_offset=3)
    for x, y in zip(_trial_outputs(plain), _trial_outputs(keyed)):
        assert torch.equal(x, y)
    for nm in STATE:
        assert torch.equal(getattr(s0, nm), getattr(sk, nm)), nm
    assert plain.Y is None and keyed.Y is None and sk.x_true is None
    zero = run(process_std=0.0, obs_std=0.0, seed=7)[1]
    for nm in ("X", "U", "J"):
        e = rel_err(getattr(zero, nm).cpu().numpy(),
                    getattr(plain, nm).cpu().numpy())
        print(dtype, nm, e)
        assert e < record_tol(dtype), (nm, e)
    assert torch.equal(zero.Y, zero.X)


@gpu
def test_noisy_mpc_loop_continues_bit_for_bit():
    """f64, both noises and a disturbance: mpc_closed_loop(3) then
    mpc_closed_loop(3, step_offset=3) with z0 = None is mpc_closed_loop(6)."""
    B, N, T, R = 5, 20, 6, 2
    noise = dict(process_std=STD, obs_std=[0.01, 0.02, 0.03, 0.04], seed=9,
                 sample_offset=4)
    rng = np.random.RandomState(6)
    dist = torch.from_numpy(rng.uniform(-0.01, 0.01, (B, T, 4)))
    whole, kw, _ = mpc_solver("cartpole", "f64", B, N)
    kw = dict(kw, **noise)
    z0 = whole.z0.clone()
    a = whole.mpc_closed_loop(T, R, z0=z0, disturbance=dist, **kw)
    halves = mpc_solver("cartpole", "f64", B, N)[0]
    h1 = halves.mpc_closed_loop(3, R, z0=z0, disturbance=dist[:, :3], **kw)
    assert halves.x_true is not None
    h2 = halves.mpc_closed_loop(3, R, disturbance=dist[:, 3:], step_offset=3,
                                **kw)
    torch.cuda.synchronize()
    for nm in ("X", "Y"):
        x1, x2 = getattr(h1, nm), getattr(h2, nm)
        assert torch.equal(torch.cat([x1[:, :3], x2], 1), getattr(a, nm)), nm
        assert torch.equal(x1[:, 3], x2[:, 0]), nm
    for nm in ("U", "states", "unfinished"):
        assert torch.equal(torch.cat([getattr(h1, nm), getattr(h2, nm)], 1),
                           getattr(a, nm)), nm
    for nm in STATE + ("x_true",):
        assert torch.equal(getattr(halves, nm), getattr(whole, nm)), nm
    assert torch.equal(whole.x_true, a.X[:, T])
    assert torch.equal(whole.z0, a.Y[:, T])
    # the first half's cost holds a terminal cost the whole trial's does not
    o = orc.load(np.float64)
    plant_ops = perturbed("cartpole", B, 11)[3]
    x3 = h1.X[:, 3].cpu().numpy()
    for b in range(B):
        term = o.cost(plant_ops[b], x3[b], None, terminal=True)[0]
        want = float(h1.J[b]) - term + float(h2.J[b])
        assert abs(float(a.J[b]) - want) <= 1e-12 * abs(want), b
    # set_nominal from outside, or a trial without obs_std, drops x_true
    whole.set_nominal(whole.z0, whole.U)
    assert whole.x_true is None
    halves.mpc_closed_loop(1, 1, process_std=STD)
    assert halves.x_true is None


@gpu
def test_noisy_mpc_loop_on_a_constant_reference_is_the_untracked_one():
    """f64, both noises: every reference row the problem's own goals - the
    noisy tracked trial agrees with the noisy untracked one within record_tol."""
    B, N, T, R = 3, 8, 6, 2
    noise = dict(process_std=STD, obs_std=STD, seed=7)
    s = loop_solver("cartpole", "f64", B, N)
    base = orc.make_problem("cartpole", DT["cartpole"])
    xr = np.tile(np.array(base.x_goal[:base.aug_size]), (B, 4, 1))
    ur = np.tile(np.array(base.u_goal[:base.action_size]), (B, 4, 1))
    set_ref(s, xr, ur, 1)
    r = s.mpc_closed_loop(T, R, **noise)
    u = loop_solver("cartpole", "f64", B, N)
    ru = u.mpc_closed_loop(T, R, **noise)
    torch.cuda.synchronize()
    assert s.ref_start == 1 + T
    assert torch.equal(r.states, ru.states)
    for nm in ("X", "Y", "U", "J"):
        e = rel_err(getattr(r, nm).cpu().numpy(), getattr(ru, nm).cpu().numpy())
        print(nm, e)
        assert e < record_tol("f64"), (nm, e)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_noisy_mpc_loop_with_a_moving_reference_equals_the_composed_trial(
        dtype):
    """T = 6, N = 8, R = 2, a reference of 10 rows from row 1 on (shorter than
    1 + T + N: the held row is reached), both noises: mpc_closed_loop against
    pddp_mpc_observe, set_reference_start(1 + t), rounds(R, n_iterations=1)
    and the noisy advance, bit for bit."""
    B, N, T, R, L, seed = 3, 8, 6, 2, 10, 7
    problem = "cartpole"
    xr, ur = reference_rows(problem, B, L, seed=41)
    s = loop_solver(problem, dtype, B, N)
    set_ref(s, xr, ur, 1)
    r = s.mpc_closed_loop(T, R, process_std=STD, obs_std=STD, seed=seed)
    torch.cuda.synchronize()
    assert s.ref_start == 1 + T
    assert bool(torch.isfinite(r.J).all())
    # the reference matters: the same trial under the problem's one goal
    s1 = loop_solver(problem, dtype, B, N)
    r1 = s1.mpc_closed_loop(T, R, process_std=STD, obs_std=STD, seed=seed)
    assert not torch.equal(r1.J, r.J)
    c = loop_solver(problem, dtype, B, N)
    set_ref(c, xr, ur, 0)
    x_true = c.z0.clone()
    c.set_nominal(_observe(x_true, STD, seed, 0, 0), c.U)
    logs = trial_logs(c, T, SENTINEL)
    Y = torch.full((B, T + 1, c.n), SENTINEL, dtype=c.dtype, device="cuda")
    Y[:, 0] = c.z0
    for t in range(T):
        c.set_reference_start(1 + t)
        c.rounds(R, n_iterations=1)
        _noisy_advance(c, T, t, logs, STD, STD, seed, 0, 0, x_true, Y,
                       ref=c.reference, ref_t0=1 + t)
        c._derivs_due = True
    for got, want in zip(_trial_outputs(r), list(logs) + [Y]):
        assert torch.equal(got, want)
    for nm in STATE:
        assert torch.equal(getattr(s, nm), getattr(c, nm)), nm
    assert torch.equal(s.x_true, x_true)


@gpu
def test_noisy_mpc_loop_keywords():
    """Y's shape, Y is None without obs_std, Y[:, 0] - X[:, 0] = obs_std times
    the stream-1 normals of step step_offset, the refusals, and
    closed_loop_draws(steps=)."""
    import pddp_amd
    from pddp_amd import _native
    from pddp_amd.controllers.solver import ILQRSolver
    from pddp_amd.examples import cartpole
    B, N, T = 3, 8, 4
    s = loop_solver("cartpole", "f64", B, N)
    z0, U0 = s.z0.clone(), s.U.clone()
    v = torch.tensor([0.01, 0.02, 0.03, 0.04], dtype=torch.float64)
    r = s.mpc_closed_loop(T, 2, z0=z0, obs_std=v, seed=5, sample_offset=2,
                          step_offset=3)
    torch.cuda.synchronize()
    assert tuple(r.Y.shape) == (B, T + 1, 4) and tuple(r.X.shape) == r.Y.shape
    assert torch.equal(r.X[:, 0], z0)
    want = v.numpy() * _unit_draws(B, 4, 4, 1, 5, 2, "f64")[:, 3]
    got = (r.Y[:, 0] - r.X[:, 0]).cpu().numpy()
    assert np.allclose(got, want, rtol=1e-9, atol=1e-14), (got, want)
    s.U.copy_(U0)
    rp = s.mpc_closed_loop(T, 2, z0=z0, process_std=0.01)
    assert rp.Y is None and s.x_true is None
    # a skipped trajectory: NaN / 0, its start and nominal left alone
    s.U.copy_(U0)
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    part = s.mpc_closed_loop(T, 2, z0=z0, obs_std=v, seed=5, sample_offset=2,
                             step_offset=3, active=active)
    torch.cuda.synchronize()
    on = active.bool()
    for x, y in zip(_trial_outputs(part), _trial_outputs(r)):
        assert torch.equal(x[on], y[on])
    assert bool(torch.isnan(part.Y[1]).all() and torch.isnan(part.X[1]).all())
    assert torch.equal(s.z0[1], z0[1]) and torch.equal(s.x_true[1], z0[1])
    assert torch.equal(s.U[1], U0[1])
    ok = dict(steps=2, rounds_per_step=1)
    bad = [dict(process_std=torch.zeros(3)), dict(obs_std=torch.zeros(5)),
           dict(obs_std=torch.zeros(1, 4)), dict(step_offset=-1),
           dict(step_offset=1.5), dict(obs_std=0.1, step_offset=2.0)]
    for kw in bad:
        with pytest.raises(_native.NativeError) as err:
            s.mpc_closed_loop(**dict(ok, **kw))
        for name in ("process_std", "obs_std"):
            if name in kw and "step_offset" not in kw:
                assert name in str(err.value), (kw, str(err.value))
    sp = ILQRSolver(None, 2, 3, torch.float32, "cuda",
                    plugin=types.SimpleNamespace(), n=4, m=1)
    with pytest.raises(_native.NativeError):
        sp.mpc_closed_loop(2, 1, obs_std=0.1)
    prob_d = cartpole.CartpoleDynamicsModel(0.1).native_problem(
        pddp_amd.StateEncoding.DEFAULT, cartpole.CartpoleCost())
    sd = ILQRSolver(prob_d, 2, 3, torch.float32, "cuda")
    with pytest.raises(_native.NativeError):
        sd.mpc_closed_loop(2, 1, process_std=0.1)
    # closed_loop_draws(steps=)
    for which, w in (("process", 0), ("obs", 1)):
        got = s.closed_loop_draws(2, which, seed=7, sample_offset=3, steps=T)
        assert tuple(got.shape) == (B, T, 2, 4)
        assert torch.equal(got, draws_call(B, T, 2, 4, w, 7, 3, "f64"))
        assert torch.equal(s.closed_loop_draws(2, which, seed=7,
                                               sample_offset=3),
                           draws_call(B, N, 2, 4, w, 7, 3, "f64"))
    with pytest.raises(_native.NativeError):
        s.closed_loop_draws(1, steps=0)
