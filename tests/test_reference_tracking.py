"""Reference tracking (ILQRSolver.set_reference, the pddp_*_track_* entry
points of csrc/goal_kernels.hpp and csrc/mpc_advance.hip): a goal per time step
in the derivative records, the line search and the MPC hand-over.

The oracle takes one goal per pddp_problem, but Oracle.cost / Oracle.dynamics
are per step: every expected value here is composed from them with a problem
whose x_goal / u_goal are that step's reference row (tests/test_batch_problem.py
composes per-trajectory problems the same way).  Horizon index i reads row
min(ref_t0 + i, ref_len - 1).

The references (goals + U(-0.5, 0.5), u_goal + U(-0.2, 0.2) per row, rounded
to float32 like every constant of a pddp_problem) move records and costs by
parts in ten, orders of magnitude above the bars - the project's own: 1e-10 in
f64, the records' / line search's 2e-4 in f32.  A kernel that ignores the
reference, reads a neighbour's row or misses the clamp fails the comparisons."""
import re
import types

import numpy as np
import pytest
import torch

import oracle as orc
from abi_util import assert_entry_points, cartpole_pointers, HDR
from golden_util import DT, FWD_NAMES, np_dtype, rel_err
from solver_util import (BOUND, CONTROLLER, fresh_ops, loop_solver,
                         make_solver, MEAN0, mpc_advance, named_views,
                         perturbed, PROBLEMS, record_tol, ref_row, ref_tensor,
                         reference_rows, same_bits, SENTINEL, set_ref,
                         set_table, TDT, to_device, trial_logs, under_row)

gpu = pytest.mark.gpu
KINDS = ("derivs", "line_search", "mpc_advance")
NEW_SYMBOLS = ["pddp_%s_track_%s" % (k, t) for k in KINDS
               for t in ("f32", "f64")]
COST_NAMES = ("L", "L_z", "L_u", "L_zz", "L_uz", "L_uu")
# augmented row i of each model: (state column, 0 copy / 1 sin / 2 cos)
# (ModelDims of csrc/models.hpp)
AUG = {"cartpole": ((0, 1, 3, 2, 2), (0, 0, 0, 1, 2)),
       "pendulum": ((1, 0, 0), (0, 1, 2)),
       "double_cartpole": ((0, 1, 3, 5, 2, 2, 4, 4), (0, 0, 0, 0, 1, 2, 1, 2)),
       "rendezvous": (tuple(range(8)), (0,) * 8)}


def _forward_tracked(o, op, z0, U, u_min, u_max, xr_b, ur_b, t0):
    """Oracle.forward's dictionary with every cost entry taken step by step
    under that step's reference row (Z, F_z, F_u read no goal)."""
    f = o.forward(op, z0, U, u_min, u_max)
    N, L = U.shape[0], xr_b.shape[0]
    for t in range(N + 1):
        under_row(op, xr_b, ur_b, ref_row(L, t0, t))
        if t < N:
            u = U[t] if u_min is None else np.clip(U[t], u_min, u_max)
            c = o.cost(op, f["Z"][t], u)
        else:
            c = o.cost(op, f["Z"][t], None, terminal=True)
        for nm, v in zip(COST_NAMES, c):
            if v is not None:
                f[nm][t] = v
    return f


def _cost_tracked(o, op, Zn, Un, xr_b, ur_b, t0):
    """[A] trajectory costs of candidates Zn [N+1][A][n], Un [N][A][m]: the
    sum of Oracle.cost under each step's row plus the terminal cost under
    row N, accumulated in the run's dtype in t order."""
    N, A, L = Un.shape[0], Un.shape[1], xr_b.shape[0]
    J = np.zeros(A, Zn.dtype)
    for t in range(N + 1):
        under_row(op, xr_b, ur_b, ref_row(L, t0, t))
        for a in range(A):
            if t < N:
                J[a] += o.cost(op, Zn[t, a], Un[t, a])[0]
            else:
                J[a] += o.cost(op, Zn[t, a], None, terminal=True)[0]
    return J


# ---------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------

def test_track_entry_points_are_declared_exported_and_bound():
    """CPU: the six entry points in the header, the built library and
    _native._SIGS; the row layout of the header == _native's constants."""
    from pddp_amd import _native
    assert_entry_points(NEW_SYMBOLS)
    defs = dict(re.findall(r"#define\s+(PDDP_REF_\w+)\s+(\d+)", HDR))
    assert {k: int(v) for k, v in defs.items()} == {
        "PDDP_REF_ROW": _native.REF_ROW,
        "PDDP_REF_X_GOAL": _native.REF_X_GOAL,
        "PDDP_REF_U_GOAL": _native.REF_U_GOAL}
    assert (_native.REF_ROW, _native.REF_X_GOAL, _native.REF_U_GOAL) == \
        (12, 0, 8)
    # the entry points take their sibling's arguments + (ref, ref_len, ref_t0)
    assert len(_native._SIGS["pddp_derivs_track"]) == \
        len(_native._SIGS["pddp_derivs_batch"]) + 3
    assert len(_native._SIGS["pddp_line_search_track"]) == \
        len(_native._SIGS["pddp_line_search_batch"]) + 3
    assert len(_native._SIGS["pddp_mpc_advance_track"]) == \
        len(_native._SIGS["pddp_mpc_advance"]) + 3
    assert _native.lib().pddp_hip_abi_version() == 1


def test_track_entry_points_refuse_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call): PDDP_E_BADARG for ref = NULL, ref_len = 0, ref_t0 = -1 and for a
    null required pointer / a non-positive size of the siblings;
    PDDP_E_UNSUPPORTED for a Gaussian encoding.  The non-null pointers are
    host words nobody reads."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    lib = _native.lib()
    # after (problem, table): ref, ref_len, ref_t0, then the sibling's
    tails = {
        # B N Z U u_min u_max mask rec L J state
        "derivs": [2, 3, q, q, None, None, None, q, q, q, None],
        # B N A Z U gains alphas u_min u_max active bwd_status Zc Uc Jc
        "line_search": [2, 3, 4, q, q, q, q, None, None, None, None, q, q, q],
        # B N T t z0 U Z u_min u_max plant dist mask Xlog Ulog Jcl state_log
        # live_log mu delta state iter active fresh n_live
        "mpc_advance": [2, 3, 4, 0, q, q, q, None, None, None, None, None, q,
                        q, q, q, q, q, q, q, q, q, q, None]}
    for ty in ("f32", "f64"):
        for kind, tail in tails.items():
            fn = getattr(lib, "pddp_%s_track_%s" % (kind, ty))

            def call(problem, ref=q, ref_len=5, ref_t0=0, tail=tail):
                return fn(problem, None, ref, ref_len, ref_t0, *tail, None)

            assert call(pp, ref=None) == -1, (kind, ty)
            assert call(pp, ref_len=0) == -1, (kind, ty)
            assert call(pp, ref_t0=-1) == -1, (kind, ty)
            assert call(None) == -1, (kind, ty)
            assert call(ppd) == _native.E_UNSUPPORTED, (kind, ty)
            # (a table does not change the answers)
            assert fn(ppd, q, q, 5, 0, *tail, None) == _native.E_UNSUPPORTED
            for i, v in enumerate(tail):
                if v is None or (kind == "mpc_advance" and i == 3):
                    continue  # nullable; t = 0 is a valid step
                bad = list(tail)
                bad[i] = None if v == q else 0
                assert call(pp, tail=bad) == -1, (kind, ty, i)


def test_composed_oracle_equals_the_oracle_on_a_constant_reference():
    """CPU: the composition the GPU tests compare against, on a reference
    whose every row is the problem's own goals, is Oracle.forward /
    Oracle.trajectory_cost themselves (f64)."""
    o = orc.load(np.float64)
    for problem in PROBLEMS:
        op = orc.make_problem(problem, DT[problem])
        n, m, na = op.encoded_size, op.action_size, op.aug_size
        rng = np.random.RandomState(1)
        z0 = np.asarray(MEAN0[problem], np.float64) + 1e-2 * rng.randn(n)
        U = 2.0 * BOUND[problem] * rng.randn(7, m)  # (some rows clamp)
        u_min, u_max = np.full(m, -BOUND[problem]), np.full(m, BOUND[problem])
        xr = np.tile(np.array(op.x_goal[:na]), (3, 1))
        ur = np.tile(np.array(op.u_goal[:m]), (3, 1))
        want = o.forward(orc.make_problem(problem, DT[problem]), z0, U, u_min,
                         u_max)
        got = _forward_tracked(o, op, z0, U, u_min, u_max, xr, ur, 1)
        for nm in FWD_NAMES:
            assert rel_err(got[nm], want[nm]) < 1e-14, (problem, nm)
        Zn = np.stack([want["Z"], want["Z"] * 1.01], 1)
        Un = np.stack([np.clip(U, u_min, u_max)] * 2, 1)
        J = o.trajectory_cost(orc.make_problem(problem, DT[problem]), Zn, Un)
        Jt = _cost_tracked(o, op, Zn, Un, xr, ur, 2)
        assert rel_err(Jt, J) < 1e-13, problem


# ---------------------------------------------------------------------------
# 3. records
# ---------------------------------------------------------------------------

def _check_records(problem, dtype, B, N, L, t0, table):
    s, _, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    ops = fresh_ops(problem, B)
    if table:
        par, xg, ug, ops = perturbed(problem, B, seed=31)
        set_table(s, par, xg, ug)
    xr, ur = reference_rows(problem, B, L, seed=32)
    set_ref(s, xr, ur, t0)
    assert tuple(s.reference.shape) == (B, L, 12) and s.ref_start == t0
    assert s.reference.dtype == TDT[dtype] and s.reference.is_cuda
    s.nominal_rollout()
    s.derivs(set_state=False)
    views = named_views(s)
    o = orc.load(np_dtype(dtype))
    tol = record_tol(dtype)
    for b in range(B):
        ref = _forward_tracked(o, ops[b], z0[b], U[b], u_min, u_max, xr[b],
                               ur[b], t0)
        for nm in FWD_NAMES:
            e = rel_err(views[nm][b].cpu().numpy(), ref[nm])
            print(problem, dtype, N, L, t0, table, b, nm, e)
            assert e < tol, (b, nm, e)
        Jb = ref["L"].sum()
        assert abs(float(s.J_opt[b]) - Jb) <= tol * abs(Jb), b
    return s


@gpu
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_track_records_vs_oracle(problem, dtype, table):
    """B = 3, N = 12, a reference of 20 rows read from row 3 on."""
    _check_records(problem, dtype, 3, 12, 20, 3, table)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_track_records_second_chunk_and_held_row(problem, dtype):
    """N = 70: a second, ragged 64-lane chunk and the J sum across chunks;
    ref_len = 9, ref_t0 = 2, N = 12: the window runs past the reference, the
    last row is held, the terminal row included."""
    _check_records(problem, dtype, 3, 70, 80, 5, True)
    _check_records(problem, dtype, 3, 12, 9, 2, False)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_track_records_honour_the_mask(dtype):
    B, N = 5, 12
    s = _check_records("cartpole", dtype, B, N, 9, 2, True)
    want = dict(rec=s._rec.clone(), L=s.L.clone(), J=s.J_opt.clone())
    mask = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device="cuda")
    off = mask == 0
    for t in (s._rec, s.L, s.J_opt):
        t.fill_(float("nan"))
    s.derivs(mask, set_state=False)
    torch.cuda.synchronize()
    for t, nm in ((s._rec, "rec"), (s.L, "L"), (s.J_opt, "J")):
        assert bool(torch.isnan(t[off]).all()), nm
        assert torch.equal(t[~off], want[nm][~off]), nm


# ---------------------------------------------------------------------------
# 4. search
# ---------------------------------------------------------------------------

def _check_search(problem, dtype, B, N, alphas, L, t0, table):
    from pddp_amd.controllers.solver import ILQRSolver
    s0, _, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    td = TDT[dtype]
    s = s0 if alphas is None else ILQRSolver(
        s0.problem, B, N, td, "cuda", torch.from_numpy(u_min),
        torch.from_numpy(u_max), alphas=alphas.to(td))
    s.z0.copy_(s0.z0)
    s.U.copy_(s0.U)
    ops = fresh_ops(problem, B)
    if table:
        par, xg, ug, ops = perturbed(problem, B, seed=33)
        set_table(s, par, xg, ug)
    xr, ur = reference_rows(problem, B, L, seed=34)
    set_ref(s, xr, ur, t0)
    s.nominal_rollout()
    s.derivs(set_state=False)
    regv = torch.full((B,), 1.0, dtype=torch.float64, device="cuda")
    s.backward(reg=regv)
    assert int(s.bwd_status.abs().sum()) == 0
    s.line_search()
    k, K = s.gain_views()
    A = s.A
    Zc = s.Zc.permute(1, 0, 2, 3).cpu().numpy()  # (N+1, B, A, n)
    Uc = s.Uc.permute(1, 0, 2, 3).cpu().numpy()
    Jc = s.Jc.cpu().numpy()
    o = orc.load(np_dtype(dtype))
    tol = record_tol(dtype)
    for b in range(B):
        Zn, Un = o.control_law(ops[b], s.Z[b].cpu().numpy(), U[b],
                               k[b].cpu().numpy(), K[b].cpu().numpy(),
                               s.alphas.cpu().numpy(), u_min, u_max)
        J = _cost_tracked(o, ops[b], Zn, Un, xr[b], ur[b], t0)
        e = (rel_err(Zc[:, b], Zn), rel_err(Uc[:, b], Un), rel_err(Jc[b], J))
        print(problem, dtype, A, L, t0, table, b, e)
        assert max(e) < tol, (A, b, e)
    return s


@gpu
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_track_line_search_vs_oracle(problem, dtype, table):
    """B = 3, N = 12, A = 3, a reference of 20 rows read from row 3 on."""
    _check_search(problem, dtype, 3, 12, torch.tensor([1.0, 0.5, 0.1]), 20, 3,
                  table)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_track_line_search_any_A_and_held_row(problem, dtype):
    """A = 17 with B = 5: 85 lanes, a ragged second wavefront; ref_len = 9,
    ref_t0 = 2, N = 12: the held last row, the terminal cost under it."""
    _check_search(problem, dtype, 5, 12, torch.linspace(1.0, 0.01, 17), 9, 2,
                  True)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_track_line_search_leaves_skipped_rows_untouched(dtype):
    B = 5
    s = _check_search("cartpole", dtype, B, 12, None, 9, 2, False)
    full = dict(Zc=s.Zc.clone(), Uc=s.Uc.clone(), Jc=s.Jc.clone())
    active = torch.tensor([1, 1, 0, 1, 1], dtype=torch.uint8, device="cuda")
    s.bwd_status[4] = 2
    skipped = np.array([False, False, True, False, True])
    for t in (s.Zc, s.Uc, s.Jc):
        t.fill_(SENTINEL)
    s.line_search(active=active)
    torch.cuda.synchronize()
    for nm in ("Zc", "Uc", "Jc"):
        t = getattr(s, nm)
        assert bool((t[skipped] == SENTINEL).all()), nm
        assert torch.equal(t[~skipped], full[nm][~skipped]), nm


# ---------------------------------------------------------------------------
# 5. a constant reference is the per-trajectory goal
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_constant_reference_equals_the_table(problem, dtype):
    """Every row the table's goals (u_ref left to its default, the table's
    u_goal): records, candidates and costs against the _batch_ entry points'
    on the same inputs and gains, then one round() from the same nominal."""
    B, N = 3, 12
    tol = record_tol(dtype)
    par, xg, ug, _ = perturbed(problem, B, seed=35)

    def solver(tracking):
        s, _, z0, U, _, _ = make_solver(problem, dtype, B, N)
        set_table(s, par, xg, ug)
        if tracking:
            set_ref(s, np.repeat(xg[:, None], 4, 1), None, 1)
        return s, torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda()

    s, z0, U = solver(False)
    st, _, _ = solver(True)
    m = s.m
    assert torch.equal(st.reference[:, :, 8:8 + m],
                       s.batch_table[:, None, 16:16 + m].expand(-1, 4, -1))
    out = []
    gains = None
    for x in (s, st):
        x.nominal_rollout()
        x.derivs(set_state=False)
        r = {k: v.clone() for k, v in named_views(x).items()}
        r["J_opt"] = x.J_opt.clone()
        if gains is None:
            regv = torch.full((B,), 1.0, dtype=torch.float64, device="cuda")
            x.backward(reg=regv)
            assert int(x.bwd_status.abs().sum()) == 0
            gains = x.gains.clone()
        else:
            x.gains.copy_(gains)
            x.bwd_status.zero_()
        x.line_search()
        r.update(Zc=x.Zc.clone(), Uc=x.Uc.clone(), Jc=x.Jc.clone())
        out.append(r)
    for nm in out[0]:
        e = rel_err(out[1][nm].cpu().numpy(), out[0][nm].cpu().numpy())
        print(problem, dtype, nm, e, "same bits:",
              same_bits(out[1][nm], out[0][nm]))
        assert e < tol, (nm, e)
    # one round from the same nominal
    for x in (s, st):
        x.set_nominal(z0, U)
        x.round()
    torch.cuda.synchronize()
    for nm in ("state", "mu", "delta", "iter"):
        assert torch.equal(getattr(st, nm), getattr(s, nm)), nm
    for nm in ("J_opt", "Z", "U", "gains_acc"):
        e = rel_err(getattr(st, nm).cpu().numpy(),
                    getattr(s, nm).cpu().numpy())
        print(problem, dtype, "round", nm, e, "same bits:",
              same_bits(getattr(st, nm), getattr(s, nm)))
        assert e < tol, (nm, e)


# ---------------------------------------------------------------------------
# 6. the cost vanishes on a feasible reference
# ---------------------------------------------------------------------------

def _augment(problem, Z):
    col, kind = AUG[problem]
    fn = (lambda v: v, np.sin, np.cos)
    return np.stack([fn[k](Z[..., c]) for c, k in zip(col, kind)], -1)


@gpu
@pytest.mark.parametrize("problem", PROBLEMS)
def test_cost_vanishes_on_a_feasible_reference(problem):
    """f64.  Z* the model's own rollout under a bounded U*, the reference
    augment(Z*) / U*: at (Z*, U*) J <= 1e-20 and |L_z|, |L_u| < 1e-12; from
    U = U* / 2, fit(max_rounds=6) never increases any trajectory's J_opt
    (fewer rounds where every trajectory has left the fit loop by then)."""
    B, N = 3, 12
    s, _, z0, _, u_min, u_max = make_solver(problem, "f64", B, N)
    rng = np.random.RandomState(36)
    Us = rng.uniform(-0.8, 0.8, (B, N, s.m)) * BOUND[problem]
    z0t, Ust = torch.from_numpy(z0).cuda(), torch.from_numpy(Us).cuda()
    s.set_nominal(z0t, Ust)
    torch.cuda.synchronize()
    Zs = s.Z.cpu().numpy()
    xr = _augment(problem, Zs)
    ur = np.concatenate([Us, Us[:, -1:]], 1)
    set_ref(s, xr, ur)
    s.derivs(set_state=False)
    torch.cuda.synchronize()
    _, _, L_z, L_u, _, _, _ = s.record_views()
    print(problem, "J", s.J_opt.tolist(), "L_z", float(L_z.abs().max()),
          "L_u", float(L_u.abs().max()))
    assert float(s.J_opt.max()) <= 1e-20
    assert float(L_z.abs().max()) < 1e-12 and float(L_u.abs().max()) < 1e-12
    s.set_nominal(z0t, 0.5 * Ust)
    s.derivs(set_state=False)  # (J_opt of the start)
    trace = [s.J_opt.clone()]
    rounds = s.fit(max_rounds=6,
                   on_round=lambda r, x: trace.append(x.J_opt.clone()))
    torch.cuda.synchronize()
    J = torch.stack(trace).cpu().numpy()
    print(problem, "J_opt by round", J.tolist())
    assert 1 <= rounds <= 6 and J.shape == (rounds + 1, B)
    assert np.isfinite(J).all() and (J[0] > 1e-10).all()
    assert (np.diff(J, axis=0) <= 0).all(), J
    assert (J[-1] < J[0]).all(), J


# ---------------------------------------------------------------------------
# 7. the advance
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("variant", ["plain", "mask", "plant", "disturbance"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_track_advance_equals_the_advance_on_a_constant_reference(
        problem, dtype, variant):
    """B = 5, N = 12, T = 3, t in {0, T-1}, a model table: every row of the
    reference the goals pddp_mpc_advance_* costs the trial under (the plant
    row's with a plant, else the table's): z0, U, Z, the logs and the
    controller words of the two launches from the same inputs."""
    B, N, T = 5, 12, 3
    tol = record_tol(dtype)
    s, _, z0, U, _, _ = make_solver(problem, dtype, B, N)
    par, xg, ug, _ = perturbed(problem, B, seed=37)
    set_table(s, par, xg, ug)
    plant = dist = mask = None
    if variant == "plant":
        ppar, xg, ug, _ = perturbed(problem, B, seed=38)
        rows = np.zeros((B, 20))
        rows[:, :ppar.shape[1]] = ppar
        rows[:, 8:8 + xg.shape[1]] = xg
        rows[:, 16:16 + ug.shape[1]] = ug
        plant = to_device(rows, dtype)
    if variant == "disturbance":
        dist = to_device(np.random.RandomState(5).uniform(-0.01, 0.01,
                                                          (B, T, s.n)), dtype)
    if variant == "mask":
        mask = torch.tensor([1, 1, 0, 1, 1], dtype=torch.uint8, device="cuda")
    ref = ref_tensor(np.repeat(xg[:, None], 2, 1), np.repeat(ug[:, None], 2, 1),
                     dtype)
    for t in (0, T - 1):
        got = []
        for r in (None, ref):
            s.set_nominal(torch.from_numpy(z0).cuda(),
                          torch.from_numpy(U).cuda())
            s.round(n_iterations=1)
            s.active.copy_(torch.arange(B, device="cuda") % 2)
            s.n_live.fill_(7)
            logs = trial_logs(s, T, 1.5 if t > 0 else SENTINEL)
            mpc_advance(s, T, t, logs, plant, dist, mask, r, 1)
            got.append(dict(
                {k: getattr(s, k).clone() for k in
                 CONTROLLER + ("z0", "U", "Z", "n_live")},
                Xlog=logs[0], Ulog=logs[1], Jcl=logs[2], state_log=logs[3],
                live_log=logs[4]))
        a, b = got
        for nm in a:
            if a[nm].dtype in (torch.float32, torch.float64) and \
                    nm not in ("mu", "delta"):
                e = rel_err(b[nm].cpu().numpy(), a[nm].cpu().numpy())
                print(problem, dtype, variant, t, nm, e, "same bits:",
                      same_bits(a[nm], b[nm]))
                assert e < tol, (t, nm, e)
            else:
                assert torch.equal(a[nm], b[nm]), (t, nm)
        if mask is not None:  # the masked trajectory: nothing written
            assert bool((b["Xlog"][2] == SENTINEL).all())
            assert bool((b["state_log"][2] == -9).all())


@gpu
@pytest.mark.parametrize("L", [20, 4])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_track_advance_trial_cost_vs_oracle(problem, dtype, L):
    """T = 5 advances in a row under a moving window, ref_t0 = 2 + t: Jcl is
    the sum of the oracle's stage costs of (Xlog[t], Ulog[t]) under row
    2 + t plus the terminal cost of Xlog[T] under row 2 + T, rows clamped
    (L = 4: the trial runs on the held last row from t = 1 on)."""
    B, N, T = 3, 12, 5
    s, _, z0, U, _, _ = make_solver(problem, dtype, B, N)
    xr, ur = reference_rows(problem, B, L, seed=39)
    ref = ref_tensor(xr, ur, dtype)
    s.set_nominal(torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda())
    logs = trial_logs(s, T, SENTINEL)
    for t in range(T):
        mpc_advance(s, T, t, logs, ref=ref, ref_t0=2 + t)
    X, Ul, J = (x.cpu().numpy() for x in logs[:3])
    o = orc.load(np_dtype(dtype))
    ops = fresh_ops(problem, B)
    for b in range(B):
        want = np_dtype(dtype)(0)
        for t in range(T):
            under_row(ops[b], xr[b], ur[b], ref_row(L, 2 + t, 0))
            want += o.cost(ops[b], X[b, t], Ul[b, t])[0]
        under_row(ops[b], xr[b], ur[b], ref_row(L, 2 + T - 1, 1))
        want += o.cost(ops[b], X[b, T], None, terminal=True)[0]
        e = abs(float(J[b]) - float(want)) / abs(float(want))
        print(problem, dtype, L, b, e)
        assert e < record_tol(dtype), (b, e)


# ---------------------------------------------------------------------------
# 8. the loop
# ---------------------------------------------------------------------------

def _assert_same_trial(a, b, sa, sb):
    for nm in ("X", "U", "J", "states", "unfinished"):
        assert torch.equal(getattr(a, nm), getattr(b, nm)), nm
    for nm in ("z0", "Z", "U") + CONTROLLER:
        assert torch.equal(getattr(sa, nm), getattr(sb, nm)), nm


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_mpc_loop_with_a_moving_reference_equals_the_composed_trial(problem,
                                                                    dtype):
    """T = 6, N = 8, R = 2, a reference of 20 rows from row 1 on:
    mpc_closed_loop against set_reference_start(1 + t), rounds(R,
    n_iterations=1) and the track advance, bit for bit."""
    B, N, T, R = 3, 8, 6, 2
    xr, ur = reference_rows(problem, B, 20, seed=41)
    s = loop_solver(problem, dtype, B, N)
    set_ref(s, xr, ur, 1)
    r = s.mpc_closed_loop(T, R)
    torch.cuda.synchronize()
    assert s.ref_start == 1 + T
    assert bool(torch.isfinite(r.J).all())
    # the reference matters: the same trial under the problem's one goal
    s1 = loop_solver(problem, dtype, B, N)
    r1 = s1.mpc_closed_loop(T, R)
    assert not torch.equal(r1.J, r.J)
    c = loop_solver(problem, dtype, B, N)
    set_ref(c, xr, ur, 0)
    c.set_nominal(c.z0, c.U)
    logs = trial_logs(c, T, SENTINEL)
    for t in range(T):
        c.set_reference_start(1 + t)
        c.rounds(R, n_iterations=1)
        mpc_advance(c, T, t, logs, ref=c.reference, ref_t0=1 + t)
        c._derivs_due = True
    composed = types.SimpleNamespace(X=logs[0], U=logs[1], J=logs[2],
                                     states=logs[3], unfinished=logs[4])
    _assert_same_trial(r, composed, s, c)


@gpu
def test_mpc_loop_with_a_reference_continues_bit_for_bit():
    """f64, a table set: mpc_closed_loop(3) twice, the second with z0 = None,
    is mpc_closed_loop(6) - the window goes on where the first call left it."""
    B, N, T, R = 3, 8, 6, 2
    xr, ur = reference_rows("cartpole", B, 20, seed=42)
    whole = loop_solver("cartpole", "f64", B, N, table=True)
    set_ref(whole, xr, ur, 2)
    z0 = whole.z0.clone()
    a = whole.mpc_closed_loop(T, R, z0=z0)
    halves = loop_solver("cartpole", "f64", B, N, table=True)
    set_ref(halves, xr, ur, 2)
    h1 = halves.mpc_closed_loop(3, R, z0=z0)
    assert halves.ref_start == 5
    h2 = halves.mpc_closed_loop(3, R)
    torch.cuda.synchronize()
    assert whole.ref_start == halves.ref_start == 8
    assert torch.equal(torch.cat([h1.X[:, :3], h2.X], 1), a.X)
    for nm in ("U", "states", "unfinished"):
        assert torch.equal(torch.cat([getattr(h1, nm), getattr(h2, nm)], 1),
                           getattr(a, nm)), nm
    for nm in ("z0", "Z", "U") + CONTROLLER:
        assert torch.equal(getattr(halves, nm), getattr(whole, nm)), nm
    # the first half's cost holds a terminal cost (of x_3 under row 2 + 3)
    # the whole trial's does not
    o = orc.load(np.float64)
    op = orc.make_problem("cartpole", DT["cartpole"])
    x3 = h1.X[:, 3].cpu().numpy()
    for b in range(B):
        term = o.cost(under_row(op, xr[b], ur[b], 5), x3[b], None,
                      terminal=True)[0]
        want = float(h1.J[b]) - term + float(h2.J[b])
        assert abs(float(a.J[b]) - want) <= 1e-12 * abs(want), b


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mpc_loop_runs_on_the_held_last_row(dtype):
    """A reference of 4 rows under a trial of T = 6 with N = 8 equals, bit
    for bit, the trial with the last row repeated explicitly."""
    B, N, T, R = 3, 8, 6, 2
    xr, ur = reference_rows("cartpole", B, 4, seed=43)
    pad = T + N + 2
    xl = np.concatenate([xr, np.repeat(xr[:, -1:], pad, 1)], 1)
    ul = np.concatenate([ur, np.repeat(ur[:, -1:], pad, 1)], 1)
    short = loop_solver("cartpole", dtype, B, N)
    set_ref(short, xr, ur, 1)
    long_ = loop_solver("cartpole", dtype, B, N)
    set_ref(long_, xl, ul, 1)
    a, b = short.mpc_closed_loop(T, R), long_.mpc_closed_loop(T, R)
    torch.cuda.synchronize()
    _assert_same_trial(a, b, short, long_)


# ---------------------------------------------------------------------------
# 9. refusals and restoration
# ---------------------------------------------------------------------------

@gpu
def test_reference_refusals_plan_and_restoration():
    import pddp_amd
    from pddp_amd import _native
    from pddp_amd.controllers.solver import ILQRSolver
    from pddp_amd.examples import cartpole
    B, N = 20, 10
    s, _, z0, U, u_min, u_max = make_solver("cartpole", "f32", B, N)
    z0t, Ut = torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda()
    fresh_plan = s._plan(0)
    assert fresh_plan == "one_launch"
    xr, ur = reference_rows("cartpole", B, 6, seed=44)
    s._graph = ("a captured round",)
    set_ref(s, xr, ur, 2)
    assert s._plan(0) == "records+separate"
    assert s._derivs_due is True and s._rec_stale is True
    assert s._graph is None
    assert (s._one_launch, s._nominal_sweep, s._fused) == (False,) * 3
    s.set_nominal(z0t, Ut)
    for call in (lambda: s.sweep_nominal(),
                 lambda: s.round_nominal(5e-6, 1e10, 50),
                 lambda: s.search_accept(5e-6, 1e10, 50),
                 lambda: s.closed_loop()):
        with pytest.raises(_native.NativeError, match="reference"):
            call()
    s.round()
    assert not s._one_launch_applied() and not s._nominal_sweep_applied()
    assert s._plan(0) == "records+separate"
    s._graph = ("a captured round",)
    s.set_reference_start(3)
    assert s.ref_start == 3 and s._graph is None
    # wrong shapes, a negative start
    t = torch.from_numpy
    for bad in (lambda: s.set_reference(t(xr[:, :, :4]), t(ur)),
                lambda: s.set_reference(t(xr[:5]), t(ur[:5])),
                lambda: s.set_reference(t(xr[:, 0]), None),
                lambda: s.set_reference(t(xr), t(ur[:, :5])),
                lambda: s.set_reference(t(xr[:, :0]), None),
                lambda: s.set_reference(t(xr), t(ur), start=-1),
                lambda: s.set_reference_start(-1)):
        with pytest.raises(_native.NativeError):
            bad()
    assert s.ref_start == 3 and tuple(s.reference.shape) == (B, 6, 12)
    # a table still set: its plan stays after clear_reference()
    s.set_batch_problem()
    s.clear_reference()
    assert s.reference is None and s._plan(0) == "records+separate"
    set_ref(s, xr, ur)
    s.clear_batch_problem()
    assert s._plan(0) == "records+separate"
    # ... and back: the plan and the results of a solver that never had one
    s.clear_reference()
    assert s.reference is None and s.ref_start == 0
    assert s._plan(0) == fresh_plan
    with pytest.raises(_native.NativeError):
        s.set_reference_start(1)
    s.set_nominal(z0t, Ut)
    s.round()
    assert s._one_launch_applied()
    s3 = ILQRSolver(s.problem, B, N, torch.float32, "cuda",
                    torch.from_numpy(u_min), torch.from_numpy(u_max))
    s3.set_nominal(z0t, Ut)
    s3.round()
    torch.cuda.synchronize()
    for nm in ("Z", "U", "J_opt", "state", "iter", "mu", "delta", "active",
               "fresh"):
        assert torch.equal(getattr(s, nm), getattr(s3, nm)), nm
    # outside the domain: a plugin solver, a Gaussian encoding
    sp = ILQRSolver(None, 2, 3, torch.float32, "cuda",
                    plugin=types.SimpleNamespace(), n=4, m=1)
    with pytest.raises(_native.NativeError):
        sp.set_reference(torch.zeros(2, 3, 5))
    prob_d = cartpole.CartpoleDynamicsModel(0.1).native_problem(
        pddp_amd.StateEncoding.DEFAULT, cartpole.CartpoleCost())
    sd = ILQRSolver(prob_d, 2, 3, torch.float32, "cuda")
    with pytest.raises(_native.NativeError):
        sd.set_reference(torch.zeros(2, 3, 5))


@gpu
def test_captured_round_with_a_reference_and_the_controller_methods():
    """capture_round with a reference captures the window as it stands: a
    replay equals an eager round (f64 cartpole); iLQRController forwards
    set_reference / clear_reference to its solver."""
    B, N = 3, 8
    xr, ur = reference_rows("cartpole", B, 12, seed=45)
    out = []
    for graph in (False, True):
        s = loop_solver("cartpole", "f64", B, N)
        set_ref(s, xr, ur, 1)
        s.set_nominal(s.z0, s.U)
        if graph:
            s.capture_round()
            s.set_nominal(s.z0, s.U)
            s.replay_round()
        else:
            s.round()
        torch.cuda.synchronize()
        out.append(s)
    for nm in ("Z", "U", "J_opt", "state", "mu", "delta"):
        assert torch.equal(getattr(out[0], nm), getattr(out[1], nm)), nm
    out[1].set_reference_start(2)
    assert out[1]._graph is None
    from pddp_amd.controllers.ilqr import iLQRController
    calls = []
    ctl = iLQRController.__new__(iLQRController)
    ctl._solver = None
    with pytest.raises(RuntimeError):
        ctl.set_reference(torch.zeros(1, 2, 5))
    ctl._solver = types.SimpleNamespace(
        set_reference=lambda *a: calls.append(a),
        clear_reference=lambda: calls.append("clear"))
    ctl.set_reference("x", "u", 3)
    ctl.clear_reference()
    assert calls == [("x", "u", 3), "clear"]
