"""Receding-horizon trials on the device (pddp_mpc_advance_*,
csrc/mpc_advance.hip, ILQRSolver.mpc_closed_loop): the hand-over between two
control steps against the CPU oracle and against the same work composed from
pddp_nominal_rollout[_batch]_*, and the whole loop against the oracle's MPC
loop (the loop of test_mpc_steps_vs_oracle, per trajectory, on that
trajectory's own plant)."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import oracle as orc
from abi_util import assert_entry_points, caller, cartpole_pointers, ROOT
from golden_util import DT, np_dtype, rel_err
from solver_util import (BOUND, CONTROLLER, make_solver, mpc_advance,
                         mpc_alphas_np, mpc_inputs, mpc_solver, perturbed,
                         plant_rows, PROBLEMS, REARMED, record_tol, SENTINEL,
                         set_table, to_device, trial_logs, UNDEFINED)

gpu = pytest.mark.gpu
SYMBOLS = ["pddp_mpc_advance_f32", "pddp_mpc_advance_f64"]
MAX_REG = 4  # pddp_problem.h: iLQRState


def test_mpc_entry_points_are_declared_exported_and_bound():
    """CPU: both symbols in the header, the built library and _native._SIGS."""
    from pddp_amd import _native
    assert_entry_points(SYMBOLS)
    assert len(_native._SIGS["pddp_mpc_advance"]) == 27
    assert _native.lib().pddp_hip_abi_version() == 1


def test_model_parameter_counts_agree():
    """CPU: csrc/model_params.hpp == ILQRSolver._PARAM_COUNT, model by model
    (the ids of include/pddp_problem.h)."""
    from pddp_amd.controllers.solver import ILQRSolver
    ids = dict(re.findall(r"(PDDP_MODEL_\w+)\s*=\s*(\d+)", open(os.path.join(
        ROOT, "include", "pddp_problem.h")).read()))
    txt = open(os.path.join(ROOT, "pddp_amd", "csrc", "model_params.hpp")).read()
    txt = txt[txt.index("constexpr int kModelParamCount"):]
    got = {int(ids[k]): int(v) for k, v in
           re.findall(r"MODEL == (PDDP_MODEL_\w+)\s*\?\s*(\d+)", txt)}
    last = int(re.search(r":\s*(\d+);", txt).group(1))
    want = dict(ILQRSolver._PARAM_COUNT)
    for model, count in got.items():
        assert want.pop(model) == count, model
    assert list(want.values()) == [last], want


def test_mpc_advance_refuses_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call): PDDP_E_BADARG for a null required pointer, a non-positive size and
    t outside [0, T); PDDP_E_UNSUPPORTED for a DEFAULT-encoding problem, both
    dtypes.  The non-null pointers are host words nobody reads."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    lib = _native.lib()
    for ty in ("f32", "f64"):
        #       0     1  2  3  4  5   6  7  8     9     10    11    12    13
        #       table B  N  T  t  z0  U  Z  u_min u_max plant dist  mask  Xlog
        good = [None, 2, 3, 4, 0, q, q, q, None, None, None, None, None, q,
                # 14   15   16         17        18  19     20     21    22
                # Ulog Jcl  state_log  live_log  mu  delta  state  iter  active
                q, q, q, q, q, q, q, q, q,
                # 23    24
                # fresh n_live
                q, None]
        call = caller(getattr(lib, "pddp_mpc_advance_" + ty), good)

        for required in (5, 6, 7, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23):
            assert call(pp, **{"_%d" % required: None}) == -1, (ty, required)
        for size in (1, 2, 3):
            assert call(pp, **{"_%d" % size: 0}) == -1, (ty, size)
        assert call(pp, _4=-1) == -1 and call(pp, _4=4) == -1, ty  # t
        assert call(None) == -1, ty
        assert call(ppd) == _native.E_UNSUPPORTED, ty


# ---------------------------------------------------------------------------
# one advance
# ---------------------------------------------------------------------------

def _check_advance(problem, dtype, variant, B=5, N=12, T=3):
    from pddp_amd import _native
    s, op, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    model_ops = [op] * B
    if variant in ("table", "table_own_model"):
        # (the controllers' models: other rows than the plants')
        par, xg, ug, model_ops = perturbed(problem, B, 12)
        set_table(s, par, xg, ug)
    rows, plant_ops = plant_rows(problem, B, 1, 11, dtype)
    rows, plant_ops = rows[:, 0], [o[0] for o in plant_ops]
    if variant in ("table_own_model", "own_model"):
        rows, plant_ops = None, model_ops
    bounded = variant != "unbounded"
    rng = np.random.RandomState(5)
    dist = rng.uniform(-0.01, 0.01, (B, T, s.n)).astype(np_dtype(dtype))
    mask = None
    if variant == "masked":
        mask = np.ones(B, np.uint8)
        mask[B // 2] = 0
    on = np.ones(B, bool) if mask is None else mask.astype(bool)
    o = orc.load(np_dtype(dtype))
    tol = record_tol(dtype)
    plant_t, dist_t = to_device(rows, dtype), to_device(dist, dtype)
    mask_t = None if mask is None else torch.from_numpy(mask).cuda()
    for t in (0, T - 1):
        # a nominal and two rounds behind it; some trajectories left live
        s.set_nominal(torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda())
        s.round(n_iterations=1)
        s.round(n_iterations=1)
        s.active.copy_(torch.arange(B, device="cuda") % 2)
        torch.cuda.synchronize()
        assert bool((s.state != UNDEFINED).any())
        assert bool((s.delta != 2.0).any())
        s.n_live.fill_(7)
        pre = {k: getattr(s, k).clone() for k in
               CONTROLLER + ("z0", "U", "Z", "n_live")}
        J0 = 1.5 if t > 0 else SENTINEL
        logs = trial_logs(s, T, J0)
        logs0 = [x.clone() for x in logs]
        mpc_advance(s, T, t, logs, plant=plant_t, dist=dist_t, mask=mask_t,
                    bounded=bounded)
        Xlog, Ulog, Jcl, state_log, live_log = (x.cpu().numpy() for x in logs)
        z_pre, U_pre = pre["z0"].cpu().numpy(), pre["U"].cpu().numpy()
        u = U_pre[:, 0]
        if bounded:
            u = np.clip(u, u_min, u_max)
        # exact: the logs, the shift, the re-armed words
        assert np.array_equal(Ulog[on, t], u[on])
        assert np.array_equal(Xlog[on, t], z_pre[on])
        shifted = np.concatenate([U_pre[:, 1:], U_pre[:, -1:]], 1)
        assert np.array_equal(s.U.cpu().numpy()[on], shifted[on])
        assert np.array_equal(state_log[on, t], pre["state"].cpu().numpy()[on])
        assert np.array_equal(live_log[on, t],
                              (pre["active"].cpu().numpy() != 0)[on])
        for k, v in REARMED.items():
            assert bool((getattr(s, k)[torch.from_numpy(on).cuda()] == v)
                        .all()), k
        assert int(s.n_live.abs().sum()) == 0
        # (the other steps' columns of the logs are not written)
        other = [i for i in range(T) if i != t]
        assert (Ulog[:, other] == SENTINEL).all()
        assert (state_log[:, other] == -9).all()
        assert (live_log[:, other] == 9).all()
        keep = [i for i in range(T + 1) if i != t and not
                (i == T and t == T - 1)]
        assert (Xlog[:, keep] == SENTINEL).all()
        # to rounding: the plant step, the terminal state, the cost
        z_new = s.z0.cpu().numpy()
        for b in np.nonzero(on)[0]:
            xn = o.dynamics(plant_ops[b], z_pre[b], u[b], jac=False)[0] + \
                dist[b, t]
            L = o.cost(plant_ops[b], z_pre[b], u[b])[0]
            J = L if t == 0 else np_dtype(dtype)(J0) + L
            e = [rel_err(z_new[b], xn)]
            if t == T - 1:
                J = J + o.cost(plant_ops[b], xn, None, terminal=True)[0]
                e.append(rel_err(Xlog[b, T], xn))
                assert np.array_equal(Xlog[b, T], z_new[b])
            e.append(abs(float(Jcl[b]) - float(J)) / abs(float(J)))
            print(problem, dtype, variant, t, b, e)
            assert max(e) < tol, (t, b, e)
        # Z: the rollout of pddp_nominal_rollout[_batch] from the device's own
        # z0 and shifted U, on a second buffer
        Z2 = torch.full_like(s.Z, SENTINEL)
        p = _native.ptr
        s._problem_call("pddp_nominal_rollout", B, N, p(s.z0), p(s.U),
                        p(s.u_min if bounded else None),
                        p(s.u_max if bounded else None), None, p(Z2), s._s())
        torch.cuda.synchronize()
        t_on = torch.from_numpy(on).cuda()
        print(problem, dtype, variant, t, "Z == the composed rollout, bit for "
              "bit:", torch.equal(s.Z[t_on], Z2[t_on]))
        e = rel_err(s.Z[t_on].cpu().numpy(), Z2[t_on].cpu().numpy())
        assert e < tol, (t, e)
        assert torch.equal(s.Z[:, 0], s.z0)
        # a masked trajectory: every buffer byte for byte as before the launch
        off = ~on
        if off.any():
            t_off = torch.from_numpy(off).cuda()
            for k in CONTROLLER + ("z0", "U", "Z"):
                assert torch.equal(getattr(s, k)[t_off], pre[k][t_off]), k
            for x, x0 in zip(logs, logs0):
                assert torch.equal(x[t_off], x0[t_off])


@gpu
@pytest.mark.parametrize("variant", ["plant", "table", "table_own_model",
                                     "own_model", "unbounded", "masked"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_mpc_advance_vs_composed_path_and_oracle(problem, dtype, variant):
    """B = 5, N = 12, T = 3, t in {0, T-1}, a disturbance of +-0.01, plants
    from perturbed(problem, B, 11): with plant rows alone, with a model table
    whose rows differ from the plants', with plant = NULL (the plant is the
    controller's model: the table's row, and without a table the shared
    problem), unbounded, and with one trajectory masked out."""
    _check_advance(problem, dtype, variant)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mpc_advance_second_partial_wavefront(dtype):
    _check_advance("cartpole", dtype, "masked", B=70)


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_trial(problem, B, N, T, big_U, table):
    """The oracle's MPC loop per trajectory, f64: (X, U, states, attempts),
    the model of trajectory b `perturbed(problem, B, 12)`'s row with `table`
    (else the shared problem), its plant `perturbed(problem, B, 11)`'s."""
    o = orc.load(np.float64)
    z0, U0 = mpc_inputs(problem, B, N, big_U)
    plant_ops = perturbed(problem, B, 11)[3]
    model_ops = perturbed(problem, B, 12)[3] if table else \
        [orc.make_problem(problem, DT[problem])] * B
    n, m = z0.shape[1], U0.shape[2]
    u_min, u_max = np.full(m, -BOUND[problem]), np.full(m, BOUND[problem])
    alphas = mpc_alphas_np()
    X, Ul = np.empty((B, T + 1, n)), np.empty((B, T, m))
    states = np.empty((B, T), np.int32)
    attempts = np.empty((B, T), np.int32)
    for b in range(B):
        z, Uo = z0[b], U0[b]
        for t in range(T):
            _, Uo, _, st, trace = o.fit(model_ops[b], z, Uo, alphas,
                                        n_iterations=1, u_min=u_min,
                                        u_max=u_max)
            states[b, t], attempts[b, t] = st, len(trace)
            u = np.clip(Uo[0], u_min, u_max)
            X[b, t], Ul[b, t] = z, u
            z = o.dynamics(plant_ops[b], z, u, jac=False)[0]
            Uo = np.concatenate([Uo[1:], Uo[-1:]], 0)
        X[b, T] = z
    for a in (X, Ul, states, attempts):
        a.setflags(write=False)
    return X, Ul, states, attempts


def _check_trial_vs_oracle(problem, big_U, R, table=False, B=5, N=20, T=6):
    Xo, Uo, states, attempts = _oracle_trial(problem, B, N, T, big_U, table)
    s, kw, plant_ops = mpc_solver(problem, "f64", B, N, big_U, table)
    r = s.mpc_closed_loop(T, R, **kw)
    torch.cuda.synchronize()
    X, U, J = r.X.cpu().numpy(), r.U.cpu().numpy(), r.J.cpu().numpy()
    assert X.shape == Xo.shape and U.shape == Uo.shape and J.shape == (B,)
    assert r.states.dtype == torch.int32 and r.unfinished.dtype == torch.uint8
    print(problem, "big U" if big_U else "", "R", R, "attempts",
          attempts.tolist())
    assert np.array_equal(r.unfinished.cpu().numpy(),
                          (attempts > R).astype(np.uint8))
    done = attempts <= R
    assert np.array_equal(r.states.cpu().numpy()[done], states[done])
    print("X", np.abs(X - Xo).max(), "U", np.abs(U - Uo).max())
    assert np.allclose(X, Xo, rtol=1e-8, atol=1e-10)
    assert np.allclose(U, Uo, rtol=1e-8, atol=1e-10)
    o = orc.load(np.float64)
    for b in range(B):
        Jb = o.trajectory_cost(plant_ops[b], X[b][:, None, :],
                               U[b][:, None, :])[0]
        assert abs(J[b] - Jb) <= 1e-10 * abs(Jb), (b, J[b], Jb)
    return s, r


@gpu
@pytest.mark.parametrize("problem", ["cartpole", "pendulum"])
def test_mpc_loop_vs_oracle_first_attempts(problem):
    """B = 5, N = 20, T = 6, z0 and U as in make_solver: every control step of
    every trajectory is accepted at its first attempt; one round per step."""
    attempts = _oracle_trial(problem, 5, 20, 6, False, False)[3]
    assert (attempts == 1).all(), attempts
    _check_trial_vs_oracle(problem, False, R=1)


@gpu
@pytest.mark.parametrize("R", [10, 4])
def test_mpc_loop_vs_oracle_with_rejected_steps(R):
    """The pendulum with U = 10 randn: 28 of the 30 control steps take one
    attempt, 2 take 10 and end in MAX_REG - decided within 10 rounds per step,
    unfinished (and the nominal unchanged either way) within 4."""
    _, _, states, attempts = _oracle_trial("pendulum", 5, 20, 6, True, False)
    # (a condition of the test: the rejected path is exercised)
    assert (attempts > 4).any(), attempts
    assert (attempts <= 10).all(), attempts
    assert (states[attempts > 4] == MAX_REG).all()
    s, r = _check_trial_vs_oracle("pendulum", True, R=R)
    assert bool(r.unfinished.any()) == (R == 4)


@gpu
def test_mpc_loop_vs_oracle_with_a_model_table():
    """Every controller with its own identified model, different from its
    plant: the rounds are records+separate."""
    from pddp_amd.controllers.solver import RECORDS_SEPARATE
    s, _ = _check_trial_vs_oracle("cartpole", False, R=10, table=True)
    assert s.batch_table is not None
    assert s._plan(s.kernel_variant) == RECORDS_SEPARATE


@gpu
def test_mpc_loop_f32_vs_the_composed_trial():
    """cartpole f32, B = 64, N = 25, T = 5, two rounds per step in the
    one-launch round, against the same trial composed from existing calls on
    a second solver: set_nominal, round() x 2, the plant step by
    pddp_nominal_rollout_batch at N = 1 on the plant rows, a torch shift."""
    from pddp_amd import _native
    B, N, T, R = 64, 25, 5, 2
    s, _, z0, U, u_min, u_max = make_solver("cartpole", "f32", B, N)
    s2 = make_solver("cartpole", "f32", B, N)[0]
    par, xg, ug, plant_ops = perturbed("cartpole", B, 11)
    r = s.mpc_closed_loop(T, R, params=torch.from_numpy(par),
                          x_goal=torch.from_numpy(xg),
                          u_goal=torch.from_numpy(ug))
    torch.cuda.synchronize()
    assert s._one_launch is True, "the one-launch round did not apply"
    rows = to_device(plant_rows("cartpole", B, 1, 11, "f32")[0][:, 0], "f32")
    z, Un = torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda()
    Xc = torch.empty(B, T + 1, s.n, device="cuda")
    Uc = torch.empty(B, T, s.m, device="cuda")
    states = torch.empty(B, T, dtype=torch.int32, device="cuda")
    unfinished = torch.empty(B, T, dtype=torch.uint8, device="cuda")
    step = torch.empty(B, 2, s.n, device="cuda")
    p = _native.ptr
    for t in range(T):
        s2.set_nominal(z, Un)
        for _ in range(R):
            s2.round(n_iterations=1)
        states[:, t], unfinished[:, t] = s2.state, s2.active
        u0 = s2.U[:, :1].contiguous()
        _native.call("pddp_nominal_rollout_batch", s2.dtype,
                     ctypes.addressof(s2.problem), p(rows), B, 1, p(s2.z0),
                     p(u0), p(s2.u_min), p(s2.u_max), None, p(step), s2._s())
        Xc[:, t] = s2.z0
        Uc[:, t] = torch.minimum(torch.maximum(u0[:, 0], s2.u_min), s2.u_max)
        z = step[:, 1].clone()
        Un = torch.cat([s2.U[:, 1:], s2.U[:, -1:]], 1)
    Xc[:, T] = z
    torch.cuda.synchronize()
    same = ((r.states == states) & (r.unfinished == unfinished)).cpu().numpy()
    share = same.mean()
    print("decisions identical on %.1f %% of the (b, t) pairs" % (
        100 * share))
    assert share >= 0.95, share
    agree = same.all(axis=1)
    assert agree.any()
    o = orc.load(np.float64)
    X, Ua, J = r.X.cpu().numpy(), r.U.cpu().numpy(), r.J.cpu().numpy()
    Xc, Uc = Xc.cpu().numpy(), Uc.cpu().numpy()
    for b in np.nonzero(agree)[0]:
        Jb = o.trajectory_cost(plant_ops[b],
                               Xc[b][:, None, :].astype(np.float64),
                               Uc[b][:, None, :].astype(np.float64))[0]
        e = (rel_err(X[b], Xc[b]), rel_err(Ua[b], Uc[b]),
             abs(J[b] - Jb) / abs(Jb))
        assert max(e) < 2e-4, (b, e)


# ---------------------------------------------------------------------------
# continuation, arguments, the controller's method
# ---------------------------------------------------------------------------

@gpu
def test_mpc_loop_continues_bit_for_bit():
    """mpc_closed_loop(3) twice, the second with z0 = None, is
    mpc_closed_loop(6), f64, the disturbance split accordingly."""
    B, N, T = 5, 20, 6
    rng = np.random.RandomState(6)
    dist = torch.from_numpy(rng.uniform(-0.01, 0.01, (B, T, 4)))
    whole, kw, plant_ops = mpc_solver("cartpole", "f64", B, N)
    z0 = whole.z0.clone()
    a = whole.mpc_closed_loop(T, 2, z0=z0, disturbance=dist, **kw)
    halves = mpc_solver("cartpole", "f64", B, N)[0]
    h1 = halves.mpc_closed_loop(3, 2, z0=z0, disturbance=dist[:, :3], **kw)
    h2 = halves.mpc_closed_loop(3, 2, disturbance=dist[:, 3:], **kw)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([h1.X[:, :3], h2.X], 1), a.X)
    assert torch.equal(h1.X[:, 3], h2.X[:, 0])
    for nm in ("U", "states", "unfinished"):
        assert torch.equal(torch.cat([getattr(h1, nm), getattr(h2, nm)], 1),
                           getattr(a, nm)), nm
    for nm in ("z0", "Z", "U") + CONTROLLER:
        assert torch.equal(getattr(halves, nm), getattr(whole, nm)), nm
    assert torch.equal(whole.z0, a.X[:, T]) and torch.equal(whole.Z[:, 0],
                                                            whole.z0)
    # the first half's cost holds a terminal cost the whole trial's does not
    o = orc.load(np.float64)
    x3 = h1.X[:, 3].cpu().numpy()
    for b in range(B):
        term = o.cost(plant_ops[b], x3[b], None, terminal=True)[0]
        want = float(h1.J[b]) - term + float(h2.J[b])
        assert abs(float(a.J[b]) - want) <= 1e-12 * abs(want), b
    # events: a (start, stop) pair around the whole loop
    from pddp_amd import _native
    lib = _native.lib()
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        _native.check(lib.pddp_event_create(ctypes.byref(e)), "event")
    whole.mpc_closed_loop(2, 1, events=ev, **kw)
    ms = ctypes.c_float()
    _native.check(lib.pddp_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)),
                  "elapsed")
    assert ms.value > 0
    for e in ev:
        lib.pddp_event_destroy(e)


@gpu
def test_mpc_loop_refuses_wrong_arguments():
    import pddp_amd
    from pddp_amd import _native
    from pddp_amd.controllers.solver import ILQRSolver
    from pddp_amd.examples import cartpole
    B, N = 3, 8
    s = make_solver("cartpole", "f64", B, N)[0]
    ok = dict(steps=2, rounds_per_step=1)
    bad = [dict(z0=torch.zeros(B, 5)), dict(z0=torch.zeros(B + 1, 4)),
           dict(disturbance=torch.zeros(B, 3, 4)),
           dict(disturbance=torch.zeros(B, 2, 3)),
           dict(params=torch.zeros(B, 5)), dict(x_goal=torch.zeros(B, 4)),
           dict(u_goal=torch.zeros(B + 1, 1)),
           dict(active=torch.ones(B, dtype=torch.bool, device="cuda")),
           dict(active=torch.ones(B, dtype=torch.uint8)),
           dict(steps=0), dict(rounds_per_step=0)]
    for kw in bad:
        with pytest.raises(_native.NativeError):
            s.mpc_closed_loop(**dict(ok, **kw))
    sp = ILQRSolver(None, 2, 3, torch.float32, "cuda",
                    plugin=types.SimpleNamespace(), n=4, m=1)
    with pytest.raises(_native.NativeError):
        sp.mpc_closed_loop(2, 1)
    prob_d = cartpole.CartpoleDynamicsModel(0.1).native_problem(
        pddp_amd.StateEncoding.DEFAULT, cartpole.CartpoleCost())
    sd = ILQRSolver(prob_d, 2, 3, torch.float32, "cuda")
    with pytest.raises(_native.NativeError):
        sd.mpc_closed_loop(2, 1)
    # `active`: the skipped trajectory NaN / 0, the others as without it
    s.z0.copy_(torch.from_numpy(mpc_inputs("cartpole", B, N, False)[0]))
    s.U.copy_(torch.from_numpy(mpc_inputs("cartpole", B, N, False)[1]))
    z0, U0 = s.z0.clone(), s.U.clone()
    full = s.mpc_closed_loop(3, 2)
    s.U.copy_(U0)
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    part = s.mpc_closed_loop(3, 2, z0=z0, active=active)
    torch.cuda.synchronize()
    on = active.bool()
    for nm in ("X", "U", "J", "states", "unfinished"):
        assert torch.equal(getattr(part, nm)[on], getattr(full, nm)[on]), nm
    assert bool(torch.isnan(part.X[1]).all() and torch.isnan(part.U[1]).all()
                and torch.isnan(part.J[1]))
    assert int(part.states[1].abs().sum()) == 0
    assert int(part.unfinished[1].sum()) == 0
    assert torch.equal(s.z0[1], z0[1]) and torch.equal(s.U[1], U0[1])


@gpu
def test_controller_mpc_closed_loop_returns_the_trial_tuple():
    import pddp_amd
    from pddp_amd.examples import cartpole
    enc = pddp_amd.StateEncoding.IGNORE_UNCERTAINTY
    model, cost = cartpole.CartpoleDynamicsModel(0.1), cartpole.CartpoleCost()
    g = torch.Generator().manual_seed(3)
    B, N, T = 3, 20, 4
    U0 = (0.1 * torch.randn(B, N, 1, generator=g)).double().cuda()
    z0 = (1e-2 * torch.randn(B, 4, generator=g)).double().cuda()
    ctrl = pddp_amd.controllers.iLQRController(None, model, cost)
    ctrl.fit(U0, encoding=enc, n_iterations=2, z0=z0, quiet=True)
    (X, Ua, dX), J = ctrl.mpc_closed_loop(T, rounds_per_step=3)
    assert tuple(X.shape) == (B, T, 4) and tuple(dX.shape) == (B, T, 4)
    assert tuple(Ua.shape) == (B, T, 1) and tuple(J.shape) == (B,)
    assert torch.equal(X[:, 0], z0) and bool(torch.isfinite(J).all())
    assert rel_err((X + dX)[:, :-1].cpu().numpy(),
                   X[:, 1:].cpu().numpy()) < 1e-12
    # after an unbatched fit: the one trajectory's, without the B axis
    ctrl.fit(U0[0], encoding=enc, n_iterations=2, z0=z0[0], quiet=True)
    (X1, U1, dX1), J1 = ctrl.mpc_closed_loop(T, rounds_per_step=3)
    assert tuple(X1.shape) == (T, 4) and tuple(dX1.shape) == (T, 4)
    assert tuple(U1.shape) == (T, 1) and J1.dim() == 0
    assert torch.equal(X1[0], z0[0]) and bool(torch.isfinite(J1))
