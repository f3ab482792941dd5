"""Closed-loop evaluation ALONG A REFERENCE (pddp_closed_loop_track_*,
csrc/closed_loop.hip, ILQRSolver.closed_loop(track=True)): the rollouts
of pddp_closed_loop_* / pddp_closed_loop_noisy_* with the stage cost of step t
taken under reference row min(ref_t0 + t, ref_len - 1) of the trajectory and
the terminal cost under row min(ref_t0 + N, ref_len - 1).

The expectation is composed as in tests/test_reference_tracking.py and
tests/test_closed_loop_noise.py: Oracle.dynamics / Oracle.cost stepped rollout
by rollout under the noisy law with the numpy model's normals, every cost under
a problem whose goals are that step's reference row, accumulated in the run's
dtype in t order.  The references move the goals by up to 0.5 per component
and row, so a kernel that costs under the plant row's goals, under a
neighbour's row or without the clamp is orders of magnitude above the bars -
the project's own, the line search's: 1e-10 in f64, 2e-4 in f32."""
import ctypes
import types

import numpy as np
import pytest
import torch

import oracle as orc
from abi_util import assert_entry_points, caller, cartpole_pointers
from golden_util import DT, np_dtype, rel_err
from solver_util import (check_stats, closed_loop_call, fresh_ops, loop_solver,
                         model_draws, noisy_call, perturbed, perturbed_starts,
                         plant_rows, policy_solver, PROBLEMS, record_tol,
                         ref_row, ref_tensor, reference_rows, same_bits,
                         SENTINEL, set_ref, std_vec, to_device, under_row)

gpu = pytest.mark.gpu
SYMBOLS = ["pddp_closed_loop_track_f32", "pddp_closed_loop_track_f64"]
STD = 0.02
NOISE = {"none": (None, None), "process": (STD, None), "obs": (None, STD),
         "both": (STD, STD)}
OUTPUTS = ("X", "U", "J", "stats")


# ---------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------

def test_tracked_entry_points_are_declared_exported_and_bound():
    """CPU: both symbols in the header, the built library, exported_symbols()
    and _native._SIGS, with the two uint64 words where the header has them;
    the siblings' argument counts and the ABI version as they were."""
    from pddp_amd import _native
    assert_entry_points(SYMBOLS)
    sig = _native._SIGS["pddp_closed_loop_track"]
    # the noisy sibling's arguments + (ref, ref_len, ref_t0) after the problem
    assert len(sig) == len(_native._SIGS["pddp_closed_loop_noisy"]) + 3 == 24
    assert [i for i, c in enumerate(sig) if c is ctypes.c_uint64] == [16, 17]
    assert [i for i, c in enumerate(sig) if c is ctypes.c_int] == \
        [2, 3, 4, 5, 6]
    assert len(_native._SIGS["pddp_closed_loop"]) == 17
    assert len(_native._SIGS["pddp_closed_loop_noisy"]) == 21
    assert _native.lib().pddp_hip_abi_version() == 1


def test_tracked_entry_points_refuse_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call), both dtypes: PDDP_E_BADARG for ref = NULL, ref_len = 0,
    ref_t0 = -1 and for everything pddp_closed_loop_* refuses;
    PDDP_E_UNSUPPORTED for a DEFAULT-encoding problem.  The non-null pointers
    are host words nobody reads.

    w_std == v_std == NULL passes the argument stage: the argument checks come
    before the problem's, so a DEFAULT-encoding problem with no noise answers
    PDDP_E_UNSUPPORTED, where pddp_closed_loop_noisy_* answers PDDP_E_BADARG
    for the same call.  That such a launch RUNS is the GPU tests' to show."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    lib = _native.lib()
    for t in ("f32", "f64"):
        #       0    1    2   3  4  5  6  7  8  9     10    11    12
        #       ref  len  t0  B  N  S  Z  U  K  z0s   plant umin  umax
        good = [q, 5, 0, 2, 3, 1, q, q, q, None, None, None, None,
                # 13 14 15   16   17    18 19 20 21
                # w  v  seed off  act   Xc Uc Jc st
                q, q, 7, 0, None, q, q, q, q]
        call = caller(getattr(lib, "pddp_closed_loop_track_" + t), good)

        assert call(pp, _0=None) == -1, t              # ref
        assert call(pp, _1=0) == -1, t                 # ref_len
        assert call(pp, _2=-1) == -1, t                # ref_t0
        for i in (3, 4, 5):                            # B, N, S
            assert call(pp, **{"_%d" % i: 0}) == -1, (t, i)
            assert call(pp, **{"_%d" % i: -3}) == -1, (t, i)
        assert call(pp, _6=None) == -1, t              # Z
        assert call(pp, _7=None) == -1, t              # U
        assert call(pp, _20=None) == -1, t             # Jc
        assert call(pp, _19=None) == -1, t             # Xc without Uc
        assert call(pp, _18=None) == -1, t             # Uc without Xc
        assert call(None) == -1, t
        assert call(ppd) == _native.E_UNSUPPORTED, t
        assert call(ppd, _13=None) == _native.E_UNSUPPORTED, t
        assert call(ppd, _14=None) == _native.E_UNSUPPORTED, t
        assert call(ppd, _18=None, _19=None) == _native.E_UNSUPPORTED, t
        # no noise at all is past the argument stage here ...
        assert call(ppd, _13=None, _14=None) == _native.E_UNSUPPORTED, t
        # ... a bad argument is still found with it, and the noisy sibling
        # refuses the same noise-free call as a bad argument
        assert call(ppd, _13=None, _14=None, _2=-1) == -1, t
        noisy = getattr(lib, "pddp_closed_loop_noisy_" + t)
        assert noisy(ppd, *good[3:13], None, None, *good[15:], None) == -1, t


# ---------------------------------------------------------------------------
# the entry point itself, and what it should give
# ---------------------------------------------------------------------------

def _track_call(s, S, ref, t0, z0s=None, plant=None, w_std=None, v_std=None,
                seed=0, offset=0, keep=True, stats=True, b0=0, gains="sweep",
                active=None, fill=None):
    """pddp_closed_loop_track_* on trajectories b0.. of the solver's nominal
    (ref: a [B][L][12] device tensor; z0s / plant: numpy, all B trajectories'
    or None; w_std / v_std: a float for every component or None); outputs
    pre-filled with `fill`."""
    from pddp_amd import _native
    B, N, n, m = s.B - b0, s.N, s.n, s.m
    opts = dict(dtype=s.dtype, device="cuda")

    def buf(*shape):
        return torch.empty(*shape, **opts) if fill is None else \
            torch.full(shape, fill, **opts)

    z0s_t = to_device(None if z0s is None else z0s[b0:], s.dtype)
    plant_t = to_device(None if plant is None else plant[b0:], s.dtype)
    w_t, v_t = std_vec(s, w_std), std_vec(s, v_std)
    g = s.gains if isinstance(gains, str) else gains
    out = types.SimpleNamespace(
        X=buf(B, N + 1, S, n) if keep else None,
        U=buf(B, N, S, m) if keep else None, J=buf(B, S),
        stats=buf(B, 4) if stats else None)
    p = _native.ptr
    _native.call("pddp_closed_loop_track", s.dtype,
                 ctypes.addressof(s.problem), p(ref[b0:].contiguous()),
                 ref.shape[1], t0, B, N, S, p(s.Z[b0:].contiguous()),
                 p(s.U[b0:].contiguous()),
                 p(None if g is None else g[b0:].contiguous()), p(z0s_t),
                 p(plant_t), p(s.u_min), p(s.u_max), p(w_t), p(v_t), seed,
                 offset,
                 p(None if active is None else active[b0:].contiguous()),
                 p(out.X), p(out.U), p(out.J), p(out.stats), s._s())
    torch.cuda.synchronize()
    return out


def _untracked_call(s, S, z0s, plant, w_std, v_std, seed, offset=0):
    if w_std is None and v_std is None:
        return closed_loop_call(s, S, z0s=z0s, plant=plant)
    return noisy_call(s, S, z0s=z0s, plant=plant, w_std=w_std, v_std=v_std,
                      seed=seed, offset=offset)


def _oracle_tracked(s, dtype, ops, z0s, u_min, u_max, xr, ur, t0, w_std,
                    v_std, seed, offset=0):
    """(X [B][N+1][S][n], U [B][N][S][m], J [B][S]): the oracle's dynamics and
    cost stepped under DESIGN 3.4g's law with the model's normals, the cost of
    step t under reference row min(t0 + t, L - 1) of the trajectory, the
    terminal cost under row min(t0 + N, L - 1); J in the run's dtype, in t
    order.  ops[b][i]: the plant of rollout (b, i) - its goals are written
    over."""
    o = orc.load(np_dtype(dtype))
    B, N, n, m = s.B, s.N, s.n, s.m
    S, L = z0s.shape[1], xr.shape[1]
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
                J[b, i] += o.cost(under_row(p, xr[b], ur[b], ref_row(L, t0, t)),
                                  x, u)[0]
                x = o.dynamics(p, x, u, jac=False)[0]
                if Wn is not None:
                    x = x + Wn[b, t, i]
            X[b, N, i] = x
            J[b, i] += o.cost(under_row(p, xr[b], ur[b], ref_row(L, t0, N)), x,
                              None, terminal=True)[0]
    return X, Uo, J


def _assert_close(out, want, tol, what):
    X, U, J = want
    worst = 0.0
    for b in range(J.shape[0]):
        e = (rel_err(out.X[b].cpu().numpy(), X[b]),
             rel_err(out.U[b].cpu().numpy(), U[b]),
             rel_err(out.J[b].cpu().numpy(), J[b]))
        print(*what, b, e)
        assert max(e) < tol, (what, b, e)
        worst = max(worst, max(e))
    return worst


def _track_inputs(problem, dtype, B, N, S, L, seed):
    """A policy, perturbed plants (the goal fields of plant (0, 0) far off:
    they are not read) with the oracle's problem of each, perturbed starts and
    a reference of L rows."""
    from pddp_amd import _native as N_
    s, _, u_min, u_max = policy_solver(problem, dtype, B, N)
    rows, ops = plant_rows(problem, B, S, seed, dtype)
    rows[0, 0, N_.BATCH_X_GOAL:N_.BATCH_U_GOAL + N_.MAX_ACTION] = 1e3
    z0s = perturbed_starts(s, S, seed + 100)
    xr, ur = reference_rows(problem, B, L, seed + 200)
    return s, u_min, u_max, rows, ops, z0s, xr, ur


# ---------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_tracked_rollouts_vs_oracle(problem, dtype):
    """B = 3, N = 12, S = 5 (5 of 8 lanes, several trajectories to a
    wavefront), a reference of 20 rows read from row 2, perturbed starts and
    plants; no noise, process only, measurement only, both.  The untracked
    launch on the same inputs is more than 100 bars away in J: the bar tells
    tracking from none."""
    B, N, S, L, t0 = 3, 12, 5, 20, 2
    s, u_min, u_max, rows, ops, z0s, xr, ur = _track_inputs(
        problem, dtype, B, N, S, L, seed=51)
    ref = ref_tensor(xr, ur, dtype)
    tol = record_tol(dtype)
    for name, (w_std, v_std) in NOISE.items():
        out = _track_call(s, S, ref, t0, z0s=z0s, plant=rows, w_std=w_std,
                          v_std=v_std, seed=11)
        want = _oracle_tracked(s, dtype, ops, z0s, u_min, u_max, xr, ur, t0,
                               w_std, v_std, seed=11)
        _assert_close(out, want, tol, (problem, dtype, name))
        check_stats(out, dtype, S)
        plain = _untracked_call(s, S, z0s, rows, w_std, v_std, seed=11)
        far = min(rel_err(plain.J[b].cpu().numpy(), want[2][b])
                  for b in range(B))
        print(problem, dtype, name, "untracked J off by %.3g = %.3g bars" % (
            far, far / tol))
        assert far > 100 * tol, (name, far)


@gpu
@pytest.mark.parametrize("case", ["short", "clamped_on_entry", "exact_end"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", ["cartpole", "rendezvous"])
def test_tracked_rollouts_hold_the_last_row(problem, dtype, case):
    """N = 12, both noise streams.  short: L = 4 read from row 1, the last row
    held from step 2 on; clamped_on_entry: ref_t0 = 50 with L = 4, every step
    under row 3; exact_end: ref_t0 + N == L - 1, the terminal step reads the
    last row without clamping."""
    B, N, S = 3, 12, 5
    L, t0 = {"short": (4, 1), "clamped_on_entry": (4, 50),
             "exact_end": (15, 2)}[case]
    assert case != "exact_end" or t0 + N == L - 1
    s, u_min, u_max, rows, ops, z0s, xr, ur = _track_inputs(
        problem, dtype, B, N, S, L, seed=52)
    out = _track_call(s, S, ref_tensor(xr, ur, dtype), t0, z0s=z0s,
                      plant=rows, w_std=STD, v_std=STD, seed=12)
    want = _oracle_tracked(s, dtype, ops, z0s, u_min, u_max, xr, ur, t0, STD,
                           STD, seed=12)
    _assert_close(out, want, record_tol(dtype), (problem, dtype, case))
    check_stats(out, dtype, S)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_tracked_rollouts_wider_than_a_wavefront(dtype):
    """Cartpole at S = 70, B = 3, N = 12, both noise streams: a trajectory
    over two wavefronts, lanes 0 .. 5 run two rollouts one after the other
    (each from row 0 of the window again) and the statistics cross the
    wavefronts through LDS.  The goals travel in registers at every S: there
    is no second path to cover."""
    B, N, S, L, t0 = 3, 12, 70, 20, 2
    s, u_min, u_max, rows, ops, z0s, xr, ur = _track_inputs(
        "cartpole", dtype, B, N, S, L, seed=53)
    out = _track_call(s, S, ref_tensor(xr, ur, dtype), t0, z0s=z0s,
                      plant=rows, w_std=STD, v_std=STD, seed=13)
    want = _oracle_tracked(s, dtype, ops, z0s, u_min, u_max, xr, ur, t0, STD,
                           STD, seed=13)
    _assert_close(out, want, record_tol(dtype), ("cartpole", dtype, S))
    check_stats(out, dtype, S)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_constant_reference_equals_the_untracked_launches(problem, dtype):
    """Every row of the reference the shared goals, no plant rows: the
    noise-free launch against pddp_closed_loop_*, the one with both streams
    against pddp_closed_loop_noisy_* with the same seed and offset.  Held to
    the bars; whether the bits agree is printed, not asserted (the siblings of
    DESIGN 3.4e differ in the last bit for the cartpole in f64)."""
    from pddp_amd import _native as N_
    B, N, S, L = 3, 12, 5, 7
    s, _, _, _ = policy_solver(problem, dtype, B, N)
    z0s = perturbed_starts(s, S, 154)
    shared = s._shared_row().cpu().numpy().astype(np.float64)
    na, m = s.problem.aug_size, s.m
    xr = np.tile(shared[N_.BATCH_X_GOAL:N_.BATCH_X_GOAL + na], (B, L, 1))
    ur = np.tile(shared[N_.BATCH_U_GOAL:N_.BATCH_U_GOAL + m], (B, L, 1))
    ref = ref_tensor(xr, ur, dtype)
    tol = record_tol(dtype)
    for name, (w_std, v_std) in (("none", NOISE["none"]),
                                 ("both", NOISE["both"])):
        got = _track_call(s, S, ref, 3, z0s=z0s, w_std=w_std, v_std=v_std,
                          seed=14, offset=9)
        want = _untracked_call(s, S, z0s, None, w_std, v_std, seed=14,
                               offset=9)
        for nm in OUTPUTS:
            a, b = getattr(got, nm), getattr(want, nm)
            print(problem, dtype, name, nm, "tracked == untracked, bit for "
                  "bit:", torch.equal(a, b))
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < tol, (name, nm)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", ["cartpole", "rendezvous"])
def test_states_and_actions_do_not_depend_on_the_reference(problem, dtype):
    """Two references, everything else the same, both noise streams: one
    kernel on inputs that differ only in values the dynamics never read.  X
    and U are the same bits, J differs."""
    B, N, S, L = 3, 12, 5, 20
    s, _, _, rows, _, z0s, xr, ur = _track_inputs(
        problem, dtype, B, N, S, L, seed=55)
    xr2, ur2 = reference_rows(problem, B, L, seed=999)
    kw = dict(z0s=z0s, plant=rows, w_std=STD, v_std=STD, seed=15)
    a = _track_call(s, S, ref_tensor(xr, ur, dtype), 2, **kw)
    b = _track_call(s, S, ref_tensor(xr2, ur2, dtype), 2, **kw)
    assert torch.equal(a.X, b.X) and torch.equal(a.U, b.U)
    assert not bool((a.J == b.J).any())


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_tracked_launch_repeats_offsets_and_masks(S, dtype):
    """The same call twice: the same bits.  Costs only against kept: the same
    J and stats bits.  Trajectories 1.. alone, with their slice of `ref` and
    sample_offset + S: their rows of the batch, bit for bit.  An `active`
    mask: the skipped trajectory's outputs stay as the caller filled them,
    the others keep their bits."""
    B, N, L, t0 = 3, 12, 9, 2
    s, _, _, rows, _, z0s, xr, ur = _track_inputs(
        "cartpole", dtype, B, N, S, L, seed=56)
    ref = ref_tensor(xr, ur, dtype)
    kw = dict(z0s=z0s, plant=rows, w_std=STD, v_std=STD, seed=7, offset=40)
    a = _track_call(s, S, ref, t0, **kw)
    b = _track_call(s, S, ref, t0, **kw)
    for nm in OUTPUTS:
        assert torch.equal(getattr(a, nm), getattr(b, nm)), nm
    lean = _track_call(s, S, ref, t0, keep=False, **kw)
    assert torch.equal(lean.J, a.J) and torch.equal(lean.stats, a.stats)
    tail = _track_call(s, S, ref, t0, b0=1, **dict(kw, offset=40 + S))
    for nm in OUTPUTS:
        assert torch.equal(getattr(tail, nm), getattr(a, nm)[1:]), nm
    # (and without the offset they see trajectory 0's noise instead)
    moved = _track_call(s, S, ref, t0, b0=1, **kw)
    assert not torch.equal(moved.J, a.J[1:])
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    off = np.array([False, True, False])
    got = _track_call(s, S, ref, t0, active=active, fill=SENTINEL, **kw)
    for nm in OUTPUTS:
        x, y = getattr(got, nm), getattr(a, nm)
        assert bool((x[off] == SENTINEL).all()), nm
        assert torch.equal(x[~off], y[~off]), nm


@gpu
def test_solver_and_controller_follow_the_reference():
    """ILQRSolver.closed_loop(track=True) against the entry point itself, its
    refusals, what it leaves alone, the window after mpc_closed_loop, and
    iLQRController.closed_loop(track=True)."""
    import pddp_amd
    from pddp_amd import _native
    from pddp_amd.examples import cartpole
    B, N, S, L = 3, 12, 5, 20
    s, _, u_min, u_max = policy_solver("cartpole", "f64", B, N)
    with pytest.raises(_native.NativeError, match="reference"):
        s.closed_loop(samples=S, track=True)   # no reference is set
    xr, ur = reference_rows("cartpole", B, L, seed=57)
    set_ref(s, xr, ur, 2)
    with pytest.raises(_native.NativeError, match="reference"):
        s.closed_loop(samples=S)               # as before
    with pytest.raises(_native.NativeError, match="reference"):
        s.closed_loop(samples=S, process_std=STD)
    na = s.problem.aug_size
    for kw in (dict(x_goal=torch.zeros(B, na)), dict(u_goal=torch.zeros(B, 1))):
        with pytest.raises(_native.NativeError, match="goal"):
            s.closed_loop(samples=S, track=True, **kw)
    # against the entry point: plant rows = the shared row + params
    z0s = perturbed_starts(s, S, 157)
    par, _, _, _ = perturbed("cartpole", B * S, seed=58)
    par = par.reshape(B, S, -1)
    rows = np.tile(s._shared_row().cpu().numpy(), (B, S, 1))
    rows[:, :, :par.shape[2]] = par
    s._graph = graph = ("a captured round",)
    names = ("Z", "U", "gains", "gains_acc", "reference", "state", "mu",
             "delta", "iter", "active", "fresh", "J_opt")
    before = {k: getattr(s, k).clone() for k in names}
    plan = s._plan(0)
    for noise in ({}, dict(process_std=STD, obs_std=0.5 * STD, seed=9,
                           sample_offset=40)):
        r = s.closed_loop(z0=torch.from_numpy(z0s), track=True, keep=True,
                          params=torch.from_numpy(par), accepted=False,
                          **noise)
        want = _track_call(s, S, s.reference, 2, z0s=z0s, plant=rows,
                           w_std=noise.get("process_std"),
                           v_std=noise.get("obs_std"),
                           seed=noise.get("seed", 0),
                           offset=noise.get("sample_offset", 0))
        for nm in OUTPUTS:
            assert torch.equal(getattr(r, nm), getattr(want, nm)), (noise, nm)
    assert s.closed_loop(samples=S, track=True, accepted=False).X is None
    for k in names:
        assert same_bits(getattr(s, k), before[k]), k
    assert s.ref_start == 2 and s._graph is graph and s._plan(0) == plan

    # after two MPC control steps the window stands two rows further on
    m_ = loop_solver("cartpole", "f64", B, N)
    set_ref(m_, xr, ur, 1)
    m_.mpc_closed_loop(2, 2)
    assert m_.ref_start == 3
    z0m = perturbed_starts(m_, S, 158)
    r = m_.closed_loop(z0=torch.from_numpy(z0m), track=True, keep=True,
                       accepted=False)
    torch.cuda.synchronize()
    ops = [[op] * S for op in fresh_ops("cartpole", B)]
    um, uM = m_.u_min.cpu().numpy(), m_.u_max.cpu().numpy()
    want = _oracle_tracked(m_, "f64", ops, z0m, um, uM, xr, ur, 1 + 2, None,
                           None, seed=0)
    _assert_close(r, want, record_tol("f64"), ("after mpc_closed_loop",))
    stale = _oracle_tracked(m_, "f64", ops, z0m, um, uM, xr, ur, 1, None,
                            None, seed=0)
    assert rel_err(r.J.cpu().numpy(), stale[2]) > 100 * record_tol("f64")
    assert m_.ref_start == 3

    # the controller forwards the keyword and returns the trial tuple
    enc = pddp_amd.StateEncoding.IGNORE_UNCERTAINTY
    model, cost = cartpole.CartpoleDynamicsModel(0.1), cartpole.CartpoleCost()
    g = torch.Generator().manual_seed(3)
    Nc = 20
    U0 = (0.1 * torch.randn(B, Nc, 1, generator=g)).double().cuda()
    z0 = (1e-2 * torch.randn(B, 4, generator=g)).double().cuda()
    ctrl = pddp_amd.controllers.iLQRController(None, model, cost)
    ctrl.fit(U0, encoding=enc, n_iterations=4, z0=z0, quiet=True)
    with pytest.raises(_native.NativeError, match="reference"):
        ctrl.closed_loop(samples=S, track=True)
    xc, uc = reference_rows("cartpole", B, Nc + 1, seed=59)
    ctrl.set_reference(torch.from_numpy(xc), torch.from_numpy(uc))
    (X, Ua, dX), J = ctrl.closed_loop(track=True, samples=S, obs_std=STD,
                                      seed=5)
    assert tuple(X.shape) == (B, Nc, S, 4) == tuple(dX.shape)
    assert tuple(Ua.shape) == (B, Nc, S, 1) and tuple(J.shape) == (B, S)
    Js = ctrl._solver.closed_loop(track=True, samples=S, obs_std=STD,
                                  seed=5).J
    assert torch.equal(J, Js)
    free = ctrl._solver.closed_loop(track=True, samples=S).J
    assert not bool((free == J).any())
