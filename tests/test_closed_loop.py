"""Closed-loop policy evaluation on the device (pddp_closed_loop_*,
csrc/closed_loop.hip, ILQRSolver.closed_loop): S rollouts of every
trajectory's policy (Z, U, K), each from its own initial state on its own
plant row, against the CPU oracle.

The oracle has no entry point of that name; its `control_law` rolls out from
Z'[0] under one problem, so rollout (b, s) is control_law on the plant row's
problem with Z' = Z[b] but Z'[0] = z0s[b][s], k'[0] = K[b][0] (z0s[b][s] -
Z[b][0]), k'[t > 0] = 0 and the one step size 1: its first action is then
U[b][0] + K[b][0] (x_0 - Z[b][0]) and every later one the feedback law."""
import types

import numpy as np
import pytest
import torch

import oracle as orc
from abi_util import assert_entry_points, caller, cartpole_pointers
from golden_util import np_dtype, rel_err
from solver_util import (closed_loop_call, make_solver, perturbed,
                         perturbed_starts, plant_rows, policy_solver, PROBLEMS,
                         record_tol, SENTINEL, set_table)

gpu = pytest.mark.gpu
SYMBOLS = ["pddp_closed_loop_f32", "pddp_closed_loop_f64"]


def _oracle_rollouts(s, dtype, ops, z0s, u_min, u_max):
    """(X [B][N+1][S][n], U [B][N][S][m], J [B][S]) of the oracle, rollout by
    rollout (module docstring)."""
    o = orc.load(np_dtype(dtype))
    B, N, n, m = s.B, s.N, s.n, s.m
    S = z0s.shape[1]
    Z, U = s.Z.cpu().numpy(), s.U.cpu().numpy()
    K = s.gain_views()[1].cpu().numpy()
    X = np.empty((B, N + 1, S, n), Z.dtype)
    Uo = np.empty((B, N, S, m), Z.dtype)
    J = np.empty((B, S), Z.dtype)
    one = np.ones(1, Z.dtype)
    for b in range(B):
        for i in range(S):
            Zp = Z[b].copy()
            Zp[0] = z0s[b, i]
            k = np.zeros((N, m), Z.dtype)
            k[0] = K[b, 0] @ (z0s[b, i] - Z[b, 0])
            Zn, Un = o.control_law(ops[b][i], Zp, U[b], k, K[b], one, u_min,
                                   u_max)
            X[b, :, i], Uo[b, :, i] = Zn[:, 0], Un[:, 0]
            J[b, i] = o.trajectory_cost(ops[b][i], Zn, Un)[0]
    return X, Uo, J


def _check_vs_oracle(problem, dtype, B, N, S, seed):
    s, _, u_min, u_max = policy_solver(problem, dtype, B, N)
    rows, ops = plant_rows(problem, B, S, seed, dtype)
    z0s = perturbed_starts(s, S, seed + 100)
    out = closed_loop_call(s, S, z0s=z0s, plant=rows)
    X, U, J = _oracle_rollouts(s, dtype, ops, z0s, u_min, u_max)
    tol = record_tol(dtype)
    for b in range(B):
        e = (rel_err(out.X[b].cpu().numpy(), X[b]),
             rel_err(out.U[b].cpu().numpy(), U[b]),
             rel_err(out.J[b].cpu().numpy(), J[b]))
        print(problem, dtype, S, b, e)
        assert max(e) < tol, (b, e)
    return out


def test_closed_loop_entry_points_are_declared_exported_and_bound():
    """CPU: both symbols in the header, the built library and _native._SIGS."""
    from pddp_amd import _native
    assert_entry_points(SYMBOLS)
    assert len(_native._SIGS["pddp_closed_loop"]) == 17
    assert _native.lib().pddp_hip_abi_version() == 1


def test_closed_loop_refuses_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call): PDDP_E_BADARG for a null Jc, S = 0 and one of Xc / Uc alone;
    PDDP_E_UNSUPPORTED for a DEFAULT-encoding problem, both dtypes.  The
    non-null pointers are host words nobody reads."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    lib = _native.lib()
    for t in ("f32", "f64"):
        #         B  N  S  Z  U  K  z0s   plant umin  umax  act   Xc Uc Jc st
        good = [2, 3, 1, q, q, q, None, None, None, None, None, q, q, q, q]
        call = caller(getattr(lib, "pddp_closed_loop_" + t), good)

        assert call(pp, _13=None) == -1, t             # Jc
        assert call(pp, _2=0) == -1, t                 # S
        assert call(pp, _11=None) == -1, t             # Uc without Xc
        assert call(pp, _12=None) == -1, t             # Xc without Uc
        assert call(pp, _3=None) == -1, t              # Z
        assert call(None) == -1, t
        assert call(ppd) == _native.E_UNSUPPORTED, t
        assert call(ppd, _11=None, _12=None) == _native.E_UNSUPPORTED, t


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_closed_loop_vs_oracle(problem, dtype):
    """B = 3, S = 5: a ragged lane group (5 of 8 lanes) and several
    trajectories in one wavefront."""
    _check_vs_oracle(problem, dtype, B=3, N=12, S=5, seed=31)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_closed_loop_wider_than_a_wavefront(dtype):
    """S = 70: a trajectory over two wavefronts; the statistics against numpy
    on the returned costs - min, max and count exact, the mean within the
    rounding bound of a 70-term sum of positive numbers, S eps relative."""
    B, S = 2, 70
    out = _check_vs_oracle("cartpole", dtype, B=B, N=12, S=S, seed=32)
    J = out.J.cpu().numpy()
    st = out.stats.cpu().numpy()
    assert np.isfinite(J).all() and (J > 0).all()
    eps = 2.0 ** -23 if dtype == "f32" else 2.0 ** -52
    for b in range(B):
        assert st[b, 1] == J[b].min() and st[b, 2] == J[b].max(), b
        assert st[b, 3] == S, b
        mean = J[b].astype(np.float64).mean()
        e = abs(float(st[b, 0]) - mean) / mean
        print(dtype, b, "mean off by", e, "bound", S * eps)
        assert e <= S * eps, (b, e)


@gpu
def test_closed_loop_is_position_independent():
    """The same controller in every b, the same (z0, plant row) in every s:
    all 210 columns and all statistics rows are the same bits."""
    B, N, S = 3, 12, 70
    s, _, _, _ = policy_solver("cartpole", "f32", B, N)
    for t in (s.Z, s.U, s.gains):
        t.copy_(t[0:1].expand_as(t).clone())
    rows, _ = plant_rows("cartpole", 1, 1, 33, "f32")
    rows = np.tile(rows, (B, S, 1))
    z0s = np.tile(perturbed_starts(s, 1, 133)[0:1], (B, S, 1))
    out = closed_loop_call(s, S, z0s=z0s, plant=rows)
    X = out.X.permute(1, 0, 2, 3).reshape(N + 1, B * S, -1)
    U = out.U.permute(1, 0, 2, 3).reshape(N, B * S, -1)
    assert torch.isfinite(out.J).all()
    assert bool((X == X[:, :1]).all()) and bool((U == U[:, :1]).all())
    assert bool((out.J == out.J[0, 0]).all())
    assert bool((out.stats == out.stats[0:1]).all())
    assert float(out.stats[0, 3]) == S


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", ["cartpole", "rendezvous"])
def test_closed_loop_reproduces_the_nominal(problem, dtype):
    """z0s = plant = NULL with feedback on: every rollout is the nominal and
    costs J_opt (S = 1 and S = 5)."""
    B, N = 3, 12
    s, _, _, _ = policy_solver(problem, dtype, B, N)
    tol = record_tol(dtype)
    Z, J = s.Z.cpu().numpy(), s.J_opt.cpu().numpy()
    for S in (1, 5):
        out = closed_loop_call(s, S)
        for i in range(S):
            e = (rel_err(out.X[:, :, i].cpu().numpy(), Z),
                 rel_err(out.J[:, i].cpu().numpy(), J))
            print(problem, dtype, S, i, e)
            assert max(e) < tol, (S, i, e)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", ["cartpole", "double_cartpole"])
def test_closed_loop_open_loop_equals_the_batch_rollout(problem, dtype):
    """gains = NULL, S = 1, plant rows given: the rollout of
    pddp_nominal_rollout_batch_* with those rows."""
    B, N = 5, 12
    s, _, _, _ = policy_solver(problem, dtype, B, N)
    par, xg, ug, _ = perturbed(problem, B, seed=34)
    set_table(s, par, xg, ug)
    s.nominal_rollout()
    rows = s.batch_table.cpu().numpy().reshape(B, 1, -1)
    out = closed_loop_call(s, 1, plant=rows, gains=None)
    e = rel_err(out.X[:, :, 0].cpu().numpy(), s.Z.cpu().numpy())
    print(problem, dtype, e)
    assert e < record_tol(dtype), e


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_closed_loop_nullables_and_masks(dtype):
    B, N, S = 3, 12, 5
    s, _, _, _ = policy_solver("cartpole", dtype, B, N)
    rows, _ = plant_rows("cartpole", B, S, 35, dtype)
    z0s = perturbed_starts(s, S, 135)
    tol = record_tol(dtype)
    kept = closed_loop_call(s, S, z0s=z0s, plant=rows)
    # costs only
    lean = closed_loop_call(s, S, z0s=z0s, plant=rows, keep=False)
    for nm in ("J", "stats"):
        a, b = getattr(lean, nm), getattr(kept, nm)
        print(dtype, nm, "costs-only == kept, bit for bit:",
              torch.equal(a, b))
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < tol, nm
    # without statistics
    bare = closed_loop_call(s, S, z0s=z0s, plant=rows, stats=False)
    assert torch.equal(bare.J, kept.J) and torch.equal(bare.X, kept.X)
    # active mask: the skipped keep the sentinel, the others their bits
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    off = np.array([False, True, False])
    got = closed_loop_call(s, S, z0s=z0s, plant=rows, active=active,
                           fill=SENTINEL)
    for nm in ("X", "U", "J", "stats"):
        a, b = getattr(got, nm), getattr(kept, nm)
        assert bool((a[off] == SENTINEL).all()), nm
        assert torch.equal(a[~off], b[~off]), nm
    # one plant that diverges (a huge dt), unbounded
    wild = rows.copy()
    wild[1, 2, 0] = 1e30
    out = closed_loop_call(s, S, z0s=z0s, plant=wild, bounded=False)
    J, st = out.J.cpu().numpy(), out.stats.cpu().numpy()
    assert not np.isfinite(J[1, 2])
    fin = np.isfinite(J)
    assert fin.sum() == B * S - 1
    assert st[1, 3] == S - 1 and np.isfinite(st[1, :3]).all()
    assert st[1, 1] == J[1][fin[1]].min() and st[1, 2] == J[1][fin[1]].max()
    assert (st[[0, 2], 3] == S).all()
    # no finite cost at all: mean = min = max = +inf, count 0
    wild[1, :, 0] = 1e30
    st = closed_loop_call(s, S, z0s=z0s, plant=wild,
                          bounded=False).stats.cpu().numpy()
    assert np.array_equal(st[1], [np.inf, np.inf, np.inf, 0.0]), st[1]
    assert (st[[0, 2], 3] == S).all()


@gpu
def test_closed_loop_refuses_plugin_and_default_solvers():
    import pddp_amd
    from pddp_amd import _native
    from pddp_amd.controllers.solver import ILQRSolver
    from pddp_amd.examples import cartpole
    sp = ILQRSolver(None, 2, 3, torch.float32, "cuda",
                    plugin=types.SimpleNamespace(), n=4, m=1)
    with pytest.raises(_native.NativeError):
        sp.closed_loop()
    prob_d = cartpole.CartpoleDynamicsModel(0.1).native_problem(
        pddp_amd.StateEncoding.DEFAULT, cartpole.CartpoleCost())
    sd = ILQRSolver(prob_d, 2, 3, torch.float32, "cuda")
    with pytest.raises(_native.NativeError):
        sd.closed_loop()


@gpu
def test_closed_loop_through_the_public_interface():
    """After a fit with a table: closed_loop() with no arguments runs every
    accepted policy once on its own row - the nominal and its cost - and
    leaves the solver as it was."""
    B, N, n_it = 6, 30, 12
    s, _, z0, U, u_min, u_max = make_solver("cartpole", "f64", B, N, seed=3)
    par, xg, ug, _ = perturbed("cartpole", B, seed=24)
    set_table(s, par, xg, ug)
    s.set_nominal(torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda())
    s.fit(n_it)
    names = ("state", "mu", "delta", "Z", "U", "batch_table", "gains_acc",
             "J_opt", "active")
    before = {k: getattr(s, k).clone() for k in names}
    plan = s._plan(0)
    r = s.closed_loop(keep=True)
    assert tuple(r.J.shape) == (B, 1) and tuple(r.stats.shape) == (B, 4)
    assert tuple(r.X.shape) == (B, N + 1, 1, 4)
    assert tuple(r.U.shape) == (B, N, 1, 1)
    J, Jopt = r.J[:, 0].cpu().numpy(), s.J_opt.cpu().numpy()
    print("J", np.abs(J - Jopt) / np.abs(Jopt))
    assert np.allclose(J, Jopt, rtol=1e-7, atol=0)
    e = rel_err(r.X[:, :, 0].cpu().numpy(), s.Z.cpu().numpy())
    print("X", e)
    assert e < record_tol("f64"), e
    assert torch.equal(r.stats[:, 0], r.J[:, 0])
    assert s.closed_loop().X is None
    for k in names:
        assert torch.equal(getattr(s, k), before[k]), k
    assert s._plan(0) == plan
    # Off the nominal, where K matters: closed_loop() against the entry point
    # itself on hand-built rows.  params [B][S][P] over the table, x_goal
    # [B][na] the same for every s, u_goal left to the table.
    S = 4
    z0s = perturbed_starts(s, S, 36)
    par2, xg2, _, _ = perturbed("cartpole", B * S, seed=37)
    _, xg3, _, _ = perturbed("cartpole", B, seed=38)
    rows = s.batch_table.cpu().numpy()[:, None, :].repeat(S, 1)
    rows[:, :, 0:par2.shape[1]] = par2.reshape(B, S, -1)
    rows[:, :, 8:8 + xg3.shape[1]] = xg3[:, None, :]
    # (the last sweep's gains made different from the accepted ones)
    s.backward(reg=torch.full((B,), 1.0, dtype=torch.float64, device="cuda"))
    assert not torch.equal(s.gains, s.gains_acc)
    kw = dict(z0=torch.from_numpy(z0s).cuda(),
              params=torch.from_numpy(par2.reshape(B, S, -1)),
              x_goal=torch.from_numpy(xg3), keep=True)
    for accepted, g in ((True, s.gains_acc), (False, s.gains)):
        want = closed_loop_call(s, S, z0s=z0s, plant=rows, gains=g)
        r4 = s.closed_loop(accepted=accepted, **kw)
        for nm in ("X", "U", "J", "stats"):
            assert torch.equal(getattr(r4, nm), getattr(want, nm)), \
                (accepted, nm)
    acc, last = s.closed_loop(**kw), s.closed_loop(accepted=False, **kw)
    assert not torch.equal(acc.J, last.J)  # (the two gain sets do differ)
    open_loop = closed_loop_call(s, S, z0s=z0s, plant=rows, gains=None)
    assert torch.equal(s.closed_loop(feedback=False, **kw).J, open_loop.J)
    assert torch.equal(acc.X[:, 0], kw["z0"])
    assert bool((acc.stats[:, 3] == S).all())
    # an `active` that is not a uint8 device tensor of shape (B,) is refused
    from pddp_amd import _native
    for bad in (torch.ones(B, dtype=torch.bool, device="cuda"),
                torch.ones(B, dtype=torch.uint8),
                torch.ones(B + 1, dtype=torch.uint8, device="cuda")):
        with pytest.raises(_native.NativeError):
            s.closed_loop(active=bad)
    for k in names:
        assert torch.equal(getattr(s, k), before[k]), k


@gpu
def test_controller_closed_loop_returns_the_trial_tuple():
    import pddp_amd
    from pddp_amd.examples import cartpole
    enc = pddp_amd.StateEncoding.IGNORE_UNCERTAINTY
    model, cost = cartpole.CartpoleDynamicsModel(0.1), cartpole.CartpoleCost()
    g = torch.Generator().manual_seed(3)
    B, N, S = 3, 20, 4
    U0 = (0.1 * torch.randn(B, N, 1, generator=g)).double().cuda()
    z0 = (1e-2 * torch.randn(B, 4, generator=g)).double().cuda()
    ctrl = pddp_amd.controllers.iLQRController(None, model, cost)
    Z, U, _ = ctrl.fit(U0, encoding=enc, n_iterations=4, z0=z0, quiet=True)
    (X, Ua, dX), J = ctrl.closed_loop(samples=S)
    assert tuple(X.shape) == (B, N, S, 4) and tuple(dX.shape) == (B, N, S, 4)
    assert tuple(Ua.shape) == (B, N, S, 1) and tuple(J.shape) == (B, S)
    assert rel_err(X[:, :, 0].cpu().numpy(), Z[:, :-1].cpu().numpy()) < 1e-10
    assert rel_err((X + dX)[:, -1, 0].cpu().numpy(),
                   Z[:, -1].cpu().numpy()) < 1e-10
