"""Per-trajectory cost weights (ILQRSolver.set_batch_weights, the
pddp_*_weighted_* entry points of csrc/goal_kernels.hpp): every trajectory of
the batch with its own diagonals of Q, Q_term and R, against the CPU oracle run
once per trajectory on that trajectory's own problem.

The weights (q = shared diagonal x U(1, 2) + U(0, 0.5), q_term and r = shared
diagonal x U(0.5, 2), rounded to float32 like every constant of a
pddp_problem) keep every matrix positive (semi-)definite - Q's diagonal only
grows, Q_term is diagonal in three problems and drawn as Q in the fourth
(`_weights`) - so that neither the guard of set_batch_weights nor the
regularisation schedule takes part; they move records and costs by parts in
ten, orders of magnitude above the bars - those of
tests/test_batch_problem.py: a kernel that ignores the weights, reads a
neighbour's row or replaces an off-diagonal entry fails the comparisons."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import oracle as orc
from abi_util import assert_entry_points, HDR
from golden_util import DT, FWD_NAMES, np_dtype, rel_err
from solver_util import (make_solver, named_views, perturbed, PROBLEMS,
                         record_tol, run_traced, set_table, TDT)

gpu = pytest.mark.gpu
NEW_SYMBOLS = ["pddp_%s_weighted_%s" % (k, t)
               for k in ("derivs", "line_search") for t in ("f32", "f64")]


def _weights(problem, B, seed, ops=None):
    """(q [B][na], q_term [B][na], r [B][m]) as float64 arrays of float32
    values, and the oracle's problem of every trajectory: `ops` (default: the
    shared problem B times) with the three diagonals overwritten."""
    rng = np.random.RandomState(seed)
    base = orc.make_problem(problem, DT[problem])
    na, m = base.aug_size, base.action_size
    dq = np.array([base.Q[i * 8 + i] for i in range(na)])
    dqt = np.array([base.Q_term[i * 8 + i] for i in range(na)])
    dr = np.array([base.R[i * 4 + i] for i in range(m)])
    q = dq * rng.uniform(1.0, 2.0, (B, na)) + rng.uniform(0.0, 0.5, (B, na))
    qt = dqt * rng.uniform(0.5, 2.0, (B, na))
    Qt = np.array(base.Q_term).reshape(8, 8)[:na, :na]
    if np.any(Qt - np.diag(np.diag(Qt))):
        # the rendezvous: Q_term is Q, off-diagonal entries -1 against
        # diagonals of 1 - a diagonal scaled DOWN leaves it indefinite (x0.5
        # against x0.6: an eigenvalue of -0.45).  Its terminal diagonal is
        # drawn as Q's: it only grows, the matrix stays positive semi-definite
        qt = dqt * rng.uniform(1.0, 2.0, (B, na)) + \
            rng.uniform(0.0, 0.5, (B, na))
    r = dr * rng.uniform(0.5, 2.0, (B, m))
    q, qt, r = (a.astype(np.float32).astype(np.float64) for a in (q, qt, r))
    if ops is None:
        ops = [orc.make_problem(problem, DT[problem]) for _ in range(B)]
    for b, op in enumerate(ops):
        for i in range(na):
            op.Q[i * 8 + i] = q[b, i]
            op.Q_term[i * 8 + i] = qt[b, i]
        for i in range(m):
            op.R[i * 4 + i] = r[b, i]
    return q, qt, r, ops


def _set_weights(s, q, qt, r, **kw):
    s.set_batch_weights(q=torch.from_numpy(q), q_term=torch.from_numpy(qt),
                        r=torch.from_numpy(r), **kw)


def _shared_diagonals(p, dtype):
    """The shared problem's three diagonals in the row's layout, converted
    double -> the run's dtype."""
    row = np.zeros(20)
    for i in range(p.aug_size):
        row[i], row[8 + i] = p.Q[i * 8 + i], p.Q_term[i * 8 + i]
    for i in range(p.action_size):
        row[16 + i] = p.R[i * 4 + i]
    return row.astype(np_dtype(dtype)).astype(np.float64)


def test_weighted_entry_points_are_declared_exported_and_bound():
    """CPU: the four entry points in the header, the built library,
    exported_symbols() and _native._SIGS; the row layout of the header ==
    _native's constants; the ABI version stays 1."""
    from pddp_amd import _native
    assert_entry_points(NEW_SYMBOLS)
    defs = dict(re.findall(r"#define\s+(PDDP_WEIGHT_\w+)\s+(\d+)", HDR))
    assert {k: int(v) for k, v in defs.items()} == {
        "PDDP_WEIGHT_ROW": _native.WEIGHT_ROW,
        "PDDP_WEIGHT_Q": _native.WEIGHT_Q,
        "PDDP_WEIGHT_Q_TERM": _native.WEIGHT_Q_TERM,
        "PDDP_WEIGHT_R": _native.WEIGHT_R}
    assert (_native.WEIGHT_ROW, _native.WEIGHT_Q, _native.WEIGHT_Q_TERM,
            _native.WEIGHT_R) == (20, 0, 8, 16)
    assert ctypes.CDLL(_native.LIB_PATH).pddp_hip_abi_version() == 1


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_weighted_records_vs_oracle(problem, dtype):
    """Weights alone (table == NULL), then weights AND a perturbed table: both
    writers over the shared problem."""
    B, N = 6, 70  # > 64: a second, ragged chunk of the record staging
    s, _, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    o = orc.load(np_dtype(dtype))
    tol = record_tol(dtype)
    for with_table in (False, True):
        ops = None
        if with_table:
            par, xg, ug, ops = perturbed(problem, B, seed=31)
            set_table(s, par, xg, ug)
        q, qt, r, ops = _weights(problem, B, seed=32, ops=ops)
        _set_weights(s, q, qt, r)
        assert (s.batch_table is not None) == with_table
        assert tuple(s.batch_weights.shape) == (B, 20)
        assert s.batch_weights.dtype == TDT[dtype] and s.batch_weights.is_cuda
        assert s.batch_weights.is_contiguous()
        s.nominal_rollout()
        s._rec.fill_(float("nan"))
        s.derivs(set_state=False)
        views = named_views(s)
        for b in range(B):
            ref = o.forward(ops[b], z0[b], U[b], u_min, u_max)
            for nm in FWD_NAMES:
                e = rel_err(views[nm][b].cpu().numpy(), ref[nm])
                print(problem, dtype, with_table, b, nm, e)
                assert e < tol, (with_table, b, nm, e)
            assert abs(float(s.J_opt[b]) - ref["L"].sum()) <= tol * abs(
                ref["L"].sum()), (with_table, b)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_weighted_line_search_vs_oracle(problem, dtype):
    """B = 5: a ragged last wavefront; 10, 11 and 17 step sizes, weights
    alone - and the 11 once more with a table next to the weights."""
    from pddp_amd.controllers.solver import (ILQRSolver, fit_alphas,
                                             mpc_alphas)
    B, N = 5, 12
    s0, _, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    td = TDT[dtype]
    o = orc.load(np_dtype(dtype))
    tol = record_tol(dtype)
    for alphas, with_table in (
            (fit_alphas(td, "cuda"), False), (mpc_alphas(td, "cuda"), False),
            (torch.linspace(1.0, 0.01, 17).to(td), False),
            (mpc_alphas(td, "cuda"), True)):
        s = ILQRSolver(s0.problem, B, N, td, "cuda", torch.from_numpy(u_min),
                       torch.from_numpy(u_max), alphas=alphas)
        s.z0.copy_(s0.z0)
        s.U.copy_(s0.U)
        ops = None
        if with_table:
            par, xg, ug, ops = perturbed(problem, B, seed=33)
            set_table(s, par, xg, ug)
        q, qt, r, ops = _weights(problem, B, seed=34, ops=ops)
        _set_weights(s, q, qt, r)
        s.nominal_rollout()
        s.derivs(set_state=False)
        regv = torch.full((B,), 1.0, dtype=torch.float64, device="cuda")
        s.backward(reg=regv)
        assert int(s.bwd_status.abs().sum()) == 0
        s.line_search()
        k, K = s.gain_views()
        A = s.A
        assert A == alphas.numel()
        Zc = s.Zc.permute(1, 0, 2, 3).cpu().numpy()  # (N+1, B, A, n)
        Uc = s.Uc.permute(1, 0, 2, 3).cpu().numpy()
        Jc = s.Jc.cpu().numpy()
        for b in range(B):
            Zn, Un = o.control_law(ops[b], s.Z[b].cpu().numpy(), U[b],
                                   k[b].cpu().numpy(), K[b].cpu().numpy(),
                                   s.alphas.cpu().numpy(), u_min, u_max)
            J = o.trajectory_cost(ops[b], Zn, Un)
            e = (rel_err(Zc[:, b], Zn), rel_err(Uc[:, b], Un),
                 rel_err(Jc[b], J))
            print(problem, dtype, A, with_table, b, e)
            assert max(e) < tol, (A, with_table, b, e)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", ["cartpole", "double_cartpole"])
def test_replicated_weights_equal_uniform_problem(problem, dtype):
    """Every row the shared diagonals: records and candidates of the weighted
    kernels against the uniform entry points' on the same inputs and gains (to
    rounding, not bit for bit: these are other kernels, csrc/Makefile)."""
    B, N = 5, 12
    s, _, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    tol = record_tol(dtype)

    def run():
        s.derivs(set_state=False)
        out = {k: v.clone() for k, v in named_views(s).items()}
        out["J_opt"] = s.J_opt.clone()
        return out

    def search():
        s.line_search()
        return dict(Zc=s.Zc.clone(), Uc=s.Uc.clone(), Jc=s.Jc.clone())

    s.nominal_rollout()
    want = run()
    regv = torch.full((B,), 1.0, dtype=torch.float64, device="cuda")
    s.backward(reg=regv)
    assert int(s.bwd_status.abs().sum()) == 0
    want.update(search())
    s.set_batch_weights()
    row = s.batch_weights[3].cpu().double().numpy()
    assert np.array_equal(row, _shared_diagonals(s.problem, dtype))
    s._rec.fill_(float("nan"))
    got = run()
    for t in (s.Zc, s.Uc, s.Jc):
        t.fill_(float("nan"))
    got.update(search())  # (the uniform run's gains)
    for nm in want:
        e = rel_err(got[nm].cpu().numpy(), want[nm].cpu().numpy())
        print(problem, dtype, nm, e)
        assert e < tol, (nm, e)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_weighted_kernels_honour_their_masks(dtype):
    B, N = 5, 12
    s, _, z0, U, u_min, u_max = make_solver("cartpole", dtype, B, N)
    q, qt, r, _ = _weights("cartpole", B, seed=35)
    _set_weights(s, q, qt, r)
    s.nominal_rollout()
    s.derivs(set_state=False)
    regv = torch.full((B,), 1.0, dtype=torch.float64, device="cuda")
    s.backward(reg=regv)
    ref = dict(rec=s._rec.clone(), L=s.L.clone())
    mask = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device="cuda")
    off = (mask == 0).cpu().numpy()
    sentinel = -7.25
    s._rec.fill_(sentinel)
    s.L.fill_(sentinel)
    s.derivs(mask, set_state=False)
    assert bool((s._rec[off] == sentinel).all())
    assert bool((s.L[off] == sentinel).all())
    assert torch.equal(s._rec[~off], ref["rec"][~off])
    assert torch.equal(s.L[~off], ref["L"][~off])
    # line search: active[b] == 0, bwd_status[b] != 0
    s._rec.copy_(ref["rec"])
    s.L.copy_(ref["L"])
    s.line_search()
    full = dict(Zc=s.Zc.clone(), Uc=s.Uc.clone(), Jc=s.Jc.clone())
    active = torch.tensor([1, 1, 0, 1, 1], dtype=torch.uint8, device="cuda")
    s.bwd_status[4] = 2
    skipped = np.array([False, False, True, False, True])
    for t in (s.Zc, s.Uc, s.Jc):
        t.fill_(sentinel)
    s.line_search(active=active)
    for nm in ("Zc", "Uc", "Jc"):
        t = getattr(s, nm)
        assert bool((t[skipped] == sentinel).all()), nm
        assert torch.equal(t[~skipped], full[nm][~skipped]), nm


@gpu
@pytest.mark.parametrize("problem", ["cartpole", "pendulum"])
def test_weighted_fit_traces_vs_oracle(problem):
    """Whole controller, fp64, bounded: per trajectory the oracle's fit under
    THAT trajectory's weights - the same iLQRState sequence, mu / delta,
    costs, final nominal and accepted gains (test_batch_fit_traces_vs_oracle's
    shape and bars)."""
    B, N, n_it = 6, 30, 12
    s, _, z0, U, u_min, u_max = make_solver(problem, "f64", B, N, seed=3)
    q, qt, r, ops = _weights(problem, B, seed=36)
    _set_weights(s, q, qt, r)
    s.set_nominal(torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda())
    traces = run_traced(s, n_it)
    assert s._one_launch is False and s._nominal_sweep is False
    o = orc.load(np.float64)
    alphas = s.alphas.cpu().numpy()
    J_final = []
    for b in range(B):
        Z, Uo, K, state, tr = o.fit(ops[b], z0[b], U[b], alphas,
                                    n_iterations=n_it, u_min=u_min,
                                    u_max=u_max)
        got = np.array(traces[b], dtype=np.float64)
        assert got.shape[0] == tr.shape[0], (b, got.shape, tr.shape)
        assert np.array_equal(got[:, 0], tr[:, 1]), b        # states
        assert np.allclose(got[:, 2:], tr[:, 3:], rtol=1e-12), b  # mu, delta
        assert np.allclose(got[:, 1], tr[:, 2], rtol=1e-7), b     # J_opt
        assert int(s.state[b]) == state
        assert rel_err(s.U[b].cpu().numpy(), Uo) < 1e-5
        assert rel_err(s.Z[b].cpu().numpy(), Z) < 1e-5
        _, Kacc = s.gain_views(accepted=True)
        assert rel_err(Kacc[b].cpu().numpy(), K) < 1e-5
        J_final.append(got[-1, 1])
    # the batch really held different costs
    J_final = np.array(J_final)
    assert J_final.max() > 1.01 * J_final.min() > 0, J_final


@gpu
def test_weights_plan_and_lifecycle():
    from pddp_amd import _native
    from pddp_amd.controllers.solver import ILQRSolver
    B, N = 20, 10
    s, _, z0, U, u_min, u_max = make_solver("cartpole", "f32", B, N)
    z0t, Ut = torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda()
    fresh_plan = s._plan(0)
    assert fresh_plan == "one_launch"
    q, qt, r, _ = _weights("cartpole", B, seed=37)
    _set_weights(s, q, qt, r)
    assert s._plan(0) == "records+separate"
    assert s._derivs_due is True and s._rec_stale is True
    assert s._graph is None
    s.set_nominal(z0t, Ut)
    s.round()
    assert not s._one_launch_applied() and not s._nominal_sweep_applied()
    assert s._plan(0) == "records+separate"
    # the records a round sweeps are those of ITS nominal under the weights
    Z1, U1, live = s.Z.clone(), s.U.clone(), s.active.bool().clone()
    assert int(live.sum()) >= B // 2
    s.round()
    swept = s.rec.clone()
    s2 = ILQRSolver(s.problem, B, N, torch.float32, "cuda",
                    torch.from_numpy(u_min), torch.from_numpy(u_max))
    s2.Z.copy_(Z1)
    s2.U.copy_(U1)
    s2.derivs(set_state=False)
    uniform = s2.rec.clone()
    s2.batch_weights = s.batch_weights  # (its address: looked up at the call)
    s2.derivs(set_state=False)
    assert torch.equal(swept[live], s2.rec[live])
    assert not torch.equal(swept[live], uniform[live])
    # the one-problem launches refuse while weights are set
    for call in (s.sweep_nominal, lambda: s.round_nominal(5e-6, 1e10, 50)):
        with pytest.raises(_native.NativeError, match="set_batch_weights"):
            call()
    # a table cleared while the weights stay: still records+separate
    s.set_batch_problem()
    s.clear_batch_problem()
    assert s.batch_weights is not None and s._plan(0) == "records+separate"
    assert s._one_launch is False and s._fused is False
    # ... and back: the plan and the results of a solver that never had weights
    s.clear_batch_weights()
    assert s.batch_weights is None and s._plan(0) == fresh_plan
    s.set_nominal(z0t, Ut)
    s.round()
    assert s._one_launch_applied()
    s3 = ILQRSolver(s.problem, B, N, torch.float32, "cuda",
                    torch.from_numpy(u_min), torch.from_numpy(u_max))
    s3.set_nominal(z0t, Ut)
    s3.round()
    for nm in ("Z", "U", "J_opt", "state", "mu", "delta"):
        assert torch.equal(getattr(s, nm), getattr(s3, nm)), nm
    # weights and a reference refuse each other, both ways
    x_ref = torch.zeros(B, 4, s.problem.aug_size)
    _set_weights(s, q, qt, r)
    with pytest.raises(_native.NativeError, match="reference"):
        s.set_reference(x_ref)
    assert s.reference is None
    s.clear_batch_weights()
    s.set_reference(x_ref)
    with pytest.raises(_native.NativeError, match="reference"):
        _set_weights(s, q, qt, r)
    assert s.batch_weights is None
    s.clear_reference()
    # wrong shapes name the block
    with pytest.raises(_native.NativeError, match="q_term"):
        s.set_batch_weights(q_term=torch.ones(B, 3))
    with pytest.raises(_native.NativeError, match=r"\br has shape"):
        s.set_batch_weights(r=torch.ones(B + 1, 1))
    assert s.batch_weights is None
    # outside the domain: a plugin solver, a Gaussian encoding
    sp = ILQRSolver(None, 2, 3, torch.float32, "cuda",
                    plugin=types.SimpleNamespace(), n=4, m=1)
    with pytest.raises(_native.NativeError):
        sp.set_batch_weights()
    import pddp_amd
    from pddp_amd.examples import cartpole
    prob_d = cartpole.CartpoleDynamicsModel(0.1).native_problem(
        pddp_amd.StateEncoding.DEFAULT, cartpole.CartpoleCost())
    sd = ILQRSolver(prob_d, 2, 3, torch.float32, "cuda")
    with pytest.raises(_native.NativeError):
        sd.set_batch_weights()
    # the C entry points themselves
    p = _native.ptr
    lib = _native.lib()
    pp, ppd = ctypes.addressof(s.problem), ctypes.addressof(prob_d)
    s.set_batch_weights()
    wt, st = p(s.batch_weights), s._s()
    der = (B, N, p(s.Z), p(s.U), None, None, None, p(s._rec), p(s.L),
           p(s.J_opt), None, st)
    ls = (B, N, s.A, p(s.Z), p(s.U), p(s.gains), p(s.alphas), None, None,
          None, None, p(s.Zc), p(s.Uc), p(s.Jc), st)
    for t in ("f32", "f64"):  # (refused before any launch)
        for name, args in (("derivs", der), ("line_search", ls)):
            fn = getattr(lib, "pddp_%s_weighted_%s" % (name, t))
            assert fn(ppd, None, wt, *args) == _native.E_UNSUPPORTED, (name, t)
            assert fn(pp, None, None, *args) == -1, (name, t)  # PDDP_E_BADARG
    torch.cuda.synchronize()


@gpu
def test_weights_are_checked_on_the_host():
    """check=True: a Q diagonal lowered under its off-diagonal entry (cartpole
    Q[0][0] = 0.1 against Q[0][3] = 0.5) and a non-positive R are refused, the
    first offending trajectory and matrix named; check=False takes them.  (The
    device holds the tensors; nothing is launched.)"""
    from pddp_amd import _native
    B, N = 4, 5
    s = make_solver("cartpole", "f32", B, N)[0]
    q, qt, r, _ = _weights("cartpole", B, seed=38)
    low = q.copy()
    low[:, 0] = 0.1
    with pytest.raises(_native.NativeError, match=r"\bQ of trajectory 0\b"):
        _set_weights(s, low, qt, r)
    assert s.batch_weights is None and s._plan(0) == "one_launch"
    only2 = q.copy()
    only2[2, 0] = 0.1
    with pytest.raises(_native.NativeError, match=r"\bQ of trajectory 2\b"):
        _set_weights(s, only2, qt, r)
    rneg = r.copy()
    rneg[1, 0] = 0.0
    with pytest.raises(_native.NativeError, match=r"\bR of trajectory 1\b"):
        _set_weights(s, q, qt, rneg)
    rneg[1, 0] = -1.0
    with pytest.raises(_native.NativeError, match=r"\bR of trajectory 1\b"):
        _set_weights(s, q, qt, rneg)
    assert s.batch_weights is None
    _set_weights(s, low, qt, rneg, check=False)
    row = s.batch_weights.cpu().double().numpy()
    assert np.array_equal(row[:, 0], np.float32(low[:, 0]).astype(np.float64))
    assert row[1, 16] == -1.0
    assert s._plan(0) == "records+separate"
    _set_weights(s, q, qt, r)  # (the test weights themselves pass)


@gpu
def test_closed_loop_costs_are_the_shared_problems():
    """After a fit under weights, closed_loop() reports J and stats under the
    shared Q, Q_term, R: bit-equal to an un-weighted solver's that was given
    the same nominal and accepted gains by copy."""
    B, N, S = 6, 30, 3
    s, _, z0, U, u_min, u_max = make_solver("cartpole", "f64", B, N, seed=3)
    q, qt, r, _ = _weights("cartpole", B, seed=39)
    _set_weights(s, q, qt, r)
    s.set_nominal(torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda())
    s.fit(n_iterations=12)
    rng = np.random.RandomState(40)
    z0s = torch.from_numpy(
        z0[:, None, :] + 1e-2 * rng.randn(B, S, z0.shape[1])).cuda()
    got = s.closed_loop(samples=S, z0=z0s)
    s2 = make_solver("cartpole", "f64", B, N, seed=3)[0]
    for nm in ("Z", "U", "gains_acc"):
        getattr(s2, nm).copy_(getattr(s, nm))
    want = s2.closed_loop(samples=S, z0=z0s)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got.J).all())
    assert torch.equal(got.J, want.J)
    assert torch.equal(got.stats, want.stats)


@gpu
def test_mpc_trial_with_weights_is_the_composed_trial():
    """mpc_closed_loop(3, 2) with weights, f64: bit-equal to the same trial
    composed by hand on a second solver with the same weights - per control
    step rounds(2, n_iterations=1), then pddp_mpc_advance_f64."""
    from pddp_amd import _native
    B, N, T, R = 5, 20, 3, 2
    s, _, z0, U, u_min, u_max = make_solver("cartpole", "f64", B, N)
    s2 = make_solver("cartpole", "f64", B, N)[0]
    q, qt, r, _ = _weights("cartpole", B, seed=41)
    _set_weights(s, q, qt, r)
    _set_weights(s2, q, qt, r)
    got = s.mpc_closed_loop(T, R)
    assert s._plan(0) == "records+separate" and s._one_launch is False
    opts = dict(dtype=torch.float64, device="cuda")
    X = torch.empty(B, T + 1, s2.n, **opts)
    Ua = torch.empty(B, T, s2.m, **opts)
    J = torch.empty(B, **opts)
    states = torch.empty(B, T, dtype=torch.int32, device="cuda")
    unfinished = torch.empty(B, T, dtype=torch.uint8, device="cuda")
    p = _native.ptr
    s2.set_nominal(s2.z0, s2.U)
    for t in range(T):
        s2.rounds(R, n_iterations=1)
        _native.check(_native.lib().pddp_mpc_advance_f64(
            ctypes.addressof(s2.problem), None, B, N, T, t, p(s2.z0), p(s2.U),
            p(s2.Z), p(s2.u_min), p(s2.u_max), None, None, None, p(X), p(Ua),
            p(J), p(states), p(unfinished), p(s2.mu), p(s2.delta),
            p(s2.state), p(s2.iter), p(s2.active), p(s2.fresh),
            p(s2.n_live), s2._s()), "pddp_mpc_advance_f64")
        s2._derivs_due = True  # (every nominal is new)
    torch.cuda.synchronize()
    for nm, want in (("X", X), ("U", Ua), ("J", J), ("states", states),
                     ("unfinished", unfinished)):
        assert torch.equal(getattr(got, nm), want), nm
    for nm in ("z0", "Z", "U", "mu", "delta", "state"):
        assert torch.equal(getattr(s, nm), getattr(s2, nm)), nm
    # the rounds inside the trial did optimise under the weights
    s3 = make_solver("cartpole", "f64", B, N)[0]
    plain = s3.mpc_closed_loop(T, R)
    assert not torch.equal(plain.U, got.U)


@gpu
def test_captured_round_with_weights_and_the_controller_methods():
    """capture_round with weights is a records+separate round holding the
    weights' address: a replay equals an eager round (f64 cartpole); setting
    the weights again drops the graph; iLQRController forwards
    set_batch_weights / clear_batch_weights to its solver."""
    B, N = 3, 8
    q, qt, r, _ = _weights("cartpole", B, seed=42)
    out = []
    for graph in (False, True):
        s = make_solver("cartpole", "f64", B, N)[0]
        _set_weights(s, q, qt, r)
        s.set_nominal(s.z0, s.U)
        if graph:
            s.capture_round()
            assert s._graph is not None and not s._graph_nominal
            s.set_nominal(s.z0, s.U)
            s.replay_round()
        else:
            s.round()
        torch.cuda.synchronize()
        out.append(s)
    for nm in ("Z", "U", "J_opt", "state", "mu", "delta"):
        assert torch.equal(getattr(out[0], nm), getattr(out[1], nm)), nm
    plain = make_solver("cartpole", "f64", B, N)[0]
    plain.set_nominal(plain.z0, plain.U)
    plain.round()
    assert not torch.equal(plain.J_opt, out[1].J_opt)
    _set_weights(out[1], q, qt, r)
    assert out[1]._graph is None
    from pddp_amd.controllers.ilqr import iLQRController
    calls = []
    ctl = iLQRController.__new__(iLQRController)
    ctl._solver = None
    with pytest.raises(RuntimeError):
        ctl.set_batch_weights()
    with pytest.raises(RuntimeError):
        ctl.clear_batch_weights()
    ctl._solver = types.SimpleNamespace(
        set_batch_weights=lambda *a: calls.append(a),
        clear_batch_weights=lambda: calls.append("clear"))
    ctl.set_batch_weights("q", "qt", "r", False)
    ctl.clear_batch_weights()
    assert calls == [("q", "qt", "r", False), "clear"]
