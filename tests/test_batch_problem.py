"""Per-trajectory problems (ILQRSolver.set_batch_problem, the pddp_*_batch_*
entry points of csrc/problem_kernels.hip): every trajectory of the batch with
its own model parameters and goals, against the CPU oracle run once per
trajectory on that trajectory's own problem.

The perturbations (parameters x U(0.8, 1.2), dt x U(0.9, 1.1), goals
+ U(-0.5, 0.5), u_goal + U(-0.2, 0.2), all rounded to float32 like every
constant of a pddp_problem) move records and costs by parts in ten, orders of
magnitude above the bars - those of tests/test_gpu_parity.py: a kernel that
ignores the table, or reads a neighbour's row, fails the comparisons."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import oracle as orc
from abi_util import assert_entry_points, HDR
from golden_util import FWD_NAMES, np_dtype, rel_err
from solver_util import (make_solver, named_views, perturbed, PROBLEMS,
                         record_tol, run_traced, set_table, TDT)

gpu = pytest.mark.gpu
NEW_SYMBOLS = ["pddp_%s_batch_%s" % (k, t)
               for k in ("nominal_rollout", "derivs", "line_search")
               for t in ("f32", "f64")]


def test_batch_entry_points_are_declared_exported_and_bound():
    """CPU: the six entry points in the header, the built library and
    _native._SIGS; the row layout of the header == _native's constants."""
    from pddp_amd import _native
    assert_entry_points(NEW_SYMBOLS)
    defs = dict(re.findall(r"#define\s+(PDDP_BATCH_\w+)\s+(\d+)", HDR))
    assert {k: int(v) for k, v in defs.items()} == {
        "PDDP_BATCH_ROW": _native.BATCH_ROW,
        "PDDP_BATCH_PARAMS": _native.BATCH_PARAMS,
        "PDDP_BATCH_X_GOAL": _native.BATCH_X_GOAL,
        "PDDP_BATCH_U_GOAL": _native.BATCH_U_GOAL}
    assert (_native.BATCH_ROW, _native.BATCH_PARAMS, _native.BATCH_X_GOAL,
            _native.BATCH_U_GOAL) == (20, 0, 8, 16)
    assert _native.lib().pddp_hip_abi_version() == 1


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_batch_records_vs_oracle(problem, dtype):
    B, N = 6, 70  # > 64: a second, ragged chunk of the record staging
    s, _, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    par, xg, ug, ops = perturbed(problem, B, seed=21)
    set_table(s, par, xg, ug)
    assert tuple(s.batch_table.shape) == (B, 20)
    assert s.batch_table.dtype == TDT[dtype] and s.batch_table.is_cuda
    s.nominal_rollout()
    s.derivs(set_state=False)
    views = named_views(s)
    o = orc.load(np_dtype(dtype))
    tol = record_tol(dtype)
    for b in range(B):
        ref = o.forward(ops[b], z0[b], U[b], u_min, u_max)
        for nm in FWD_NAMES:
            e = rel_err(views[nm][b].cpu().numpy(), ref[nm])
            print(problem, dtype, b, nm, e)
            assert e < tol, (b, nm, e)
        assert abs(float(s.J_opt[b]) - ref["L"].sum()) <= tol * abs(
            ref["L"].sum()), b


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_batch_line_search_vs_oracle(problem, dtype):
    """B = 5: a ragged last wavefront and a ragged last 16-lane group; 10, 11
    and 17 step sizes - the last one more than a 16-lane group holds."""
    from pddp_amd.controllers.solver import (ILQRSolver, fit_alphas,
                                             mpc_alphas)
    B, N = 5, 12
    s0, _, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    par, xg, ug, ops = perturbed(problem, B, seed=22)
    td = TDT[dtype]
    o = orc.load(np_dtype(dtype))
    tol = record_tol(dtype)
    for alphas in (fit_alphas(td, "cuda"), mpc_alphas(td, "cuda"),
                   torch.linspace(1.0, 0.01, 17).to(td)):
        s = ILQRSolver(s0.problem, B, N, td, "cuda", torch.from_numpy(u_min),
                       torch.from_numpy(u_max), alphas=alphas)
        s.z0.copy_(s0.z0)
        s.U.copy_(s0.U)
        set_table(s, par, xg, ug)
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
            print(problem, dtype, A, b, e)
            assert max(e) < tol, (A, b, e)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", ["cartpole", "double_cartpole"])
def test_replicated_table_equals_uniform_problem(problem, dtype):
    """Every row the shared problem: rollout, records and candidates of the
    batch kernels against the uniform entry points' on the same inputs and
    gains (to rounding, not bit for bit: the same closed forms inlined into
    two kernels are contracted into FMAs differently, csrc/Makefile)."""
    B, N = 5, 12
    s, _, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    tol = record_tol(dtype)

    def run():
        s.nominal_rollout()
        s.derivs(set_state=False)
        out = {k: v.clone() for k, v in named_views(s).items()}
        out["J_opt"] = s.J_opt.clone()
        return out

    def search():
        s.line_search()
        return dict(Zc=s.Zc.clone(), Uc=s.Uc.clone(), Jc=s.Jc.clone())

    want = run()
    regv = torch.full((B,), 1.0, dtype=torch.float64, device="cuda")
    s.backward(reg=regv)
    assert int(s.bwd_status.abs().sum()) == 0
    want.update(search())
    s.set_batch_problem()
    p = s.problem
    row = s.batch_table[3].cpu().double().numpy()
    assert np.array_equal(row[0:8], np.array(p.params, np.float64).astype(
        np_dtype(dtype)))
    assert np.array_equal(row[8:16], np.array(p.x_goal, np.float64).astype(
        np_dtype(dtype)))
    assert np.array_equal(row[16:20], np.array(p.u_goal, np.float64).astype(
        np_dtype(dtype)))
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
def test_batch_kernels_honour_their_masks(dtype):
    B, N = 5, 12
    s, _, z0, U, u_min, u_max = make_solver("cartpole", dtype, B, N)
    par, xg, ug, _ = perturbed("cartpole", B, seed=23)
    set_table(s, par, xg, ug)
    s.nominal_rollout()
    s.derivs(set_state=False)
    regv = torch.full((B,), 1.0, dtype=torch.float64, device="cuda")
    s.backward(reg=regv)
    ref = dict(Z=s.Z.clone(), rec=s._rec.clone(), L=s.L.clone())
    mask = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device="cuda")
    off = (mask == 0).cpu().numpy()
    sentinel = -7.25
    s.Z.fill_(sentinel)
    s.nominal_rollout(mask)
    assert bool((s.Z[off] == sentinel).all())
    assert torch.equal(s.Z[~off], ref["Z"][~off])
    s.Z.copy_(ref["Z"])
    s._rec.fill_(sentinel)
    s.L.fill_(sentinel)
    s.derivs(mask, set_state=False)
    assert bool((s._rec[off] == sentinel).all())
    assert bool((s.L[off] == sentinel).all())
    assert torch.equal(s._rec[~off], ref["rec"][~off])
    assert torch.equal(s.L[~off], ref["L"][~off])
    # line search: active[b] == 0, bwd_status[b] != 0
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
def test_batch_fit_traces_vs_oracle(problem):
    """Whole controller, fp64, bounded: per trajectory the oracle's fit on
    THAT trajectory's problem - the same iLQRState sequence, mu / delta,
    costs, final nominal and accepted gains (test_fit_traces_vs_oracle's
    shape and bars)."""
    B, N, n_it = 6, 30, 12
    s, _, z0, U, u_min, u_max = make_solver(problem, "f64", B, N, seed=3)
    par, xg, ug, ops = perturbed(problem, B, seed=24)
    set_table(s, par, xg, ug)
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
    # the batch really held different problems
    J_final = np.array(J_final)
    assert J_final.max() > 1.01 * J_final.min() > 0, J_final


@gpu
def test_batch_plan_and_lifecycle():
    from pddp_amd import _native
    from pddp_amd.controllers.solver import ILQRSolver
    B, N = 20, 10
    s, _, z0, U, u_min, u_max = make_solver("cartpole", "f32", B, N)
    z0t, Ut = torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda()
    fresh_plan = s._plan(0)
    assert fresh_plan == "one_launch"
    par, xg, ug, _ = perturbed("cartpole", B, seed=25)
    set_table(s, par, xg, ug)
    assert s._plan(0) == "records+separate"
    assert s._derivs_due is True and s._graph is None
    s.set_nominal(z0t, Ut)
    s.round()
    assert not s._one_launch_applied() and not s._nominal_sweep_applied()
    assert s._plan(0) == "records+separate"
    # the records a round sweeps are those of ITS nominal under the table
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
    s2.batch_table = s.batch_table  # (the address is looked up at the call)
    s2.derivs(set_state=False)
    assert torch.equal(swept[live], s2.rec[live])
    assert not torch.equal(swept[live], uniform[live])
    # ... and back: the plan and the results of a solver that never had a table
    s.clear_batch_problem()
    assert s.batch_table is None and s._plan(0) == fresh_plan
    s.set_nominal(z0t, Ut)
    s.round()
    assert s._one_launch_applied()
    s3 = ILQRSolver(s.problem, B, N, torch.float32, "cuda",
                    torch.from_numpy(u_min), torch.from_numpy(u_max))
    s3.set_nominal(z0t, Ut)
    s3.round()
    for nm in ("Z", "U", "J_opt", "state", "mu", "delta"):
        assert torch.equal(getattr(s, nm), getattr(s3, nm)), nm
    # outside the domain: a plugin solver, a Gaussian encoding
    sp = ILQRSolver(None, 2, 3, torch.float32, "cuda",
                    plugin=types.SimpleNamespace(), n=4, m=1)
    with pytest.raises(_native.NativeError):
        sp.set_batch_problem()
    import pddp_amd
    from pddp_amd.examples import cartpole
    prob_d = cartpole.CartpoleDynamicsModel(0.1).native_problem(
        pddp_amd.StateEncoding.DEFAULT, cartpole.CartpoleCost())
    sd = ILQRSolver(prob_d, 2, 3, torch.float32, "cuda")
    with pytest.raises(_native.NativeError):
        sd.set_batch_problem()
    # the C entry points themselves
    p = _native.ptr
    lib = _native.lib()
    pp, ppd = ctypes.addressof(s.problem), ctypes.addressof(prob_d)
    s.set_batch_problem()
    tb, st = p(s.batch_table), s._s()
    roll = (B, N, p(s.z0), p(s.U), None, None, None, p(s.Z), st)
    der = (B, N, p(s.Z), p(s.U), None, None, None, p(s._rec), p(s.L),
           p(s.J_opt), None, st)
    ls = (B, N, s.A, p(s.Z), p(s.U), p(s.gains), p(s.alphas), None, None,
          None, None, p(s.Zc), p(s.Uc), p(s.Jc), st)
    for t in ("f32", "f64"):  # (refused before any launch)
        for name, args in (("nominal_rollout", roll), ("derivs", der),
                           ("line_search", ls)):
            fn = getattr(lib, "pddp_%s_batch_%s" % (name, t))
            assert fn(ppd, tb, *args) == _native.E_UNSUPPORTED, (name, t)
            assert fn(pp, None, *args) == -1, (name, t)  # PDDP_E_BADARG
    torch.cuda.synchronize()
