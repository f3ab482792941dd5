"""The fused kernels' controller - pddp_search_accept_* (csrc/
line_search_lds.hpp, FUSED: a DPP argmin over 16 lanes, accept_decide, the
tail's winner copy in its short, long, scratch-row, dropped-candidate and dense
forms) and pddp_round_nominal_f32 (csrc/round_n4.hip) - on SEEDED controller
state, against tests/accept_model.py.

These kernels form the candidate costs themselves, so the table is over the
state: a dry launch on a snapshot gives every trajectory's `Jc` (the kernels
are deterministic), every array is restored, each trajectory is seeded with
`fresh = 0` (the sweep then leaves J_opt alone), a J_opt placed against its own
smallest cost - equal, one ulp above, 10 tol above, +inf, -inf - and a (mu,
delta, iter) row of test_accept_table.py; some trajectories are inactive.  One
launch; every output equals the model applied to the kernel's own `Jc` and
`bwd_status`.  The only tolerances are the winner's states / actions against
`oracle.control_law` (2e-5 f32, 1e-9 f64, as test_benched_round_kernels_vs_
oracle).

Step sizes [1e30, 1, 1, 0.5, 0.5, 0.25, ...] on the unbounded V_zz-regularised
branch at mu = 100: the first candidate's cost is NaN (so the reference rejects,
although later candidates improve on the nominal), the duplicated step sizes
tie.  Bounded runs use the list without 1e30 (a clamp may swallow it)."""
import numpy as np
import pytest
import torch

import accept_model as am
import oracle as orc
from accept_rows import bits, ITER_ROWS, MAX_REG, N_IT, REG_ROWS, SENT, TOL
from golden_util import np_dtype, rel_err
from solver_util import make_solver, TDT, TOL as PARITY_TOL

pytestmark = pytest.mark.gpu

STEPS = [1e30, 1.0, 1.0, 0.5, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625,
         2.0 ** -7, 2.0 ** -8, 2.0 ** -9, 2.0 ** -10, 2.0 ** -11, 2.0 ** -12,
         2.0 ** -13]
MU_SWEEP = 100.0
# The sweep that feeds pddp_search_accept_*: (gain branch, regulariser).  The
# cartpole's is the one the step sizes above were checked on.  For the other
# two it is chosen where float32 can answer the winner's comparison with the
# fp64 oracle - by the oracle's own IEEE float32 run against its fp64 run on
# these inputs (every trajectory, step sizes 1, 0.5, 0.25; rel_err of the
# states / of the actions):
#   double cartpole, V_zz-regularised: 2e-6 ... 7e-6 / 6e-5 ... 1.7e-4 at
#     reg 1e4 ... 1e8 (no trajectory's sweep goes through at reg = 100, N >=
#     127).  That branch's feedback gains do not shrink with reg (K tends to
#     -(F_u' F_u)^-1 F_u' F_z), and K (z - z_nom) with angles near pi rounds at
#     1e-4 of the actions.  Eig-clamp (Q_uu regularised, K ~ 1 / reg) at reg =
#     1e4: 2.4e-6 ... 5.9e-6 / 1.5e-7 ... 3.7e-7, every sweep goes through
#     and every trajectory has an improving candidate.
#   pendulum, V_zz-regularised: at reg = 100 2e-7 / 5e-7 (N = 16), 2.0e-6 /
#     9.5e-6 (N = 127), 1.4e-6 / 3.1e-5 (N = 140: 90 % of the rows under
#     8.9e-6; its angle winds up to 28 rad); at reg = 1e4 the actions' median
#     alone is 1.7e-5 at N = 140; eig-clamp loses the STATES instead (2.6e-5
#     ... 1.5e-4 at N >= 127).  reg = 100 it is, the cartpole's.
SWEEP = {"cartpole": (1, MU_SWEEP), "pendulum": (1, MU_SWEEP),
         "double_cartpole": (0, 1e4)}
# pddp_round_nominal_f32: mu is the sweep's regulariser as well - rows where
# the sweep goes through (tests/test_cartpole_branches.py)
_M = MAX_REG / 4
ROUND_REG_ROWS = [(100.0, 2.0), (100.0, 0.25), (100.0, 8.0),
                  (float(np.nextafter(_M, 0.0)), 2.0), (_M, 2.0),
                  (float(np.nextafter(_M, 1e3)), 2.0)]
KINDS = ("equal", "ulp_above", "ten_tol", "inf", "minus_inf")
STATE_KEYS = ("state", "iter", "active", "fresh", "mu", "delta", "J_opt")
WINNER_TOL = {"f32": 2e-5, "f64": PARITY_TOL["f64"]}


def _steps(A, huge):
    return (STEPS if huge else STEPS[1:])[:A]


def _solver(problem, dtype, B, N, A, branch, bounded, huge=None, steps=None):
    """`huge`: the list that starts with 1e30 (default: the unbounded runs);
    `steps`: another list altogether."""
    huge = (not bounded) if huge is None else huge
    from pddp_amd.controllers.solver import ILQRSolver
    s0, op, z0, U, u_min, u_max = make_solver(problem, dtype, B, N, seed=4)
    td = TDT[dtype]
    s = ILQRSolver(s0.problem, B, N, td, "cuda",
                   s0.u_min if bounded else None,
                   s0.u_max if bounded else None,
                   alphas=torch.tensor(steps or _steps(A, huge), dtype=td),
                   branch=branch)
    assert s.A == A
    s.set_nominal(torch.from_numpy(z0).cuda(), torch.from_numpy(U).cuda())
    return s, op, (u_min if bounded else None), (u_max if bounded else None)


ARRAYS = ("Z", "U", "_rec", "L", "J_opt", "gains", "gains_acc", "Jc", "Zc",
          "Uc", "bwd_status", "state", "iter", "mu", "delta", "active",
          "fresh", "n_live")


def _seed_state(s, reg_rows):
    """(mu, delta, iter) rows cycled over the batch, every 11th trajectory
    inactive with sentinels in every controller array, fresh = 0."""
    B = s.B
    b = np.arange(B)
    rr = [reg_rows[(3 * i) % len(reg_rows)] for i in b]
    dead = b % 11 == 7
    h = dict(mu=np.array([r[0] for r in rr]), delta=np.array([r[1] for r in rr]),
             iter=np.array([ITER_ROWS[(i // 2) % 3] for i in b], np.int32),
             state=np.zeros(B, np.int32), active=np.ones(B, np.uint8),
             fresh=np.zeros(B, np.uint8),
             J_opt=np.zeros(B, np.float64 if s.dtype == torch.float64
                            else np.float32))
    for k, v in SENT.items():
        h[k][dead] = v
    h["active"][dead] = 0
    for k, v in h.items():
        getattr(s, k).copy_(torch.from_numpy(v))
    return h, dead


def _seed_costs(h, dead, Jc, dt):
    """J_opt of every live trajectory against its own smallest finite cost."""
    B = len(dead)
    kinds = []
    for b in range(B):
        fin = Jc[b][np.isfinite(Jc[b])]
        Jmin = dt(fin.min()) if fin.size else dt(1.0)
        kind = KINDS[b % len(KINDS)]
        kinds.append(kind)
        if dead[b]:
            continue
        h["J_opt"][b] = {
            "equal": Jmin, "ulp_above": np.nextafter(Jmin, dt(np.inf)),
            "ten_tol": dt(Jmin * dt(1.0 + 10.0 * TOL)), "inf": dt(np.inf),
            "minus_inf": dt(-np.inf)}[kind]
    return kinds


def _sum_in_order(L, dt):
    acc = dt(0)
    for v in L:
        acc = dt(acc + dt(v))
    return acc


def _run_case(s, op, u_min, u_max, dtype, launch, reg_rows, records, unbounded,
              cartpole_steps, tag, winner_bar=True):
    """`launch(s)`: the one launch under test (True when it applied).
    `winner_bar`: compare the winners with the oracle as well."""
    dt = np_dtype(dtype)
    B, N, n, A = s.B, s.N, s.n, s.A
    h, dead = _seed_state(s, reg_rows)
    s.n_live.zero_()
    snap = {k: getattr(s, k).clone() for k in ARRAYS}
    assert launch(s), tag                       # dry: the costs it forms
    torch.cuda.synchronize()
    Jc = s.Jc.cpu().numpy().copy()
    st_dry = s.bwd_status.cpu().numpy().copy()
    for k, v in snap.items():
        getattr(s, k).copy_(v)
    kinds = _seed_costs(h, dead, Jc, dt)
    s.J_opt.copy_(torch.from_numpy(h["J_opt"]))
    # whatever the launch does not write must not look like a candidate
    s.Zc.fill_(float("nan"))
    s.Uc.fill_(float("nan"))
    if not records:
        s._rec.fill_(float("nan"))
    before = {k: getattr(s, k).cpu().numpy().copy() for k in ARRAYS}
    assert launch(s), tag
    torch.cuda.synchronize()
    got = {k: getattr(s, k).cpu().numpy() for k in ARRAYS}
    live = ~dead
    st = got["bwd_status"]
    assert np.array_equal(st[live], st_dry[live]), tag
    swept = live & (st == 0)
    assert np.array_equal(bits(got["Jc"][swept]), bits(Jc[swept])), tag

    # ---- the conditions the step sizes are there to force
    nan0 = np.isnan(Jc[swept, 0]).mean() if swept.any() else 0.0
    ties = [(i, i + 1) for i in range(A - 1)
            if float(s.alphas[i]) == float(s.alphas[i + 1])]
    tie_ok = all(np.array_equal(bits(Jc[swept, i]), bits(Jc[swept, j]))
                 for i, j in ties)
    print(tag, "status 0: %.2f" % (st[live] == 0).mean(),
          "Jc[:, 0] NaN: %.2f" % nan0, "ties", ties, "bit-equal", tie_ok)
    if cartpole_steps:
        assert (st[live] == 0).mean() >= 0.75, tag
        assert tie_ok, tag
        if unbounded:
            assert nan0 >= 0.75, tag

    # ---- every output against the model, by equality
    e = {k: before[k].copy() for k in STATE_KEYS}
    amin = np.full(B, -1)
    for b in np.flatnonzero(live):
        r = am.attempt(before["J_opt"][b], Jc[b], st[b], before["mu"][b],
                       before["delta"][b], before["iter"][b], TOL, MAX_REG,
                       N_IT, dt)
        e["state"][b], e["iter"][b], e["active"][b] = r.state, r.iter, r.active
        e["mu"][b], e["delta"][b] = r.mu, r.delta
        e["fresh"][b], e["J_opt"][b], amin[b] = r.fresh, r.J_opt, r.amin
        if records and r.fresh:
            # its records were written here: fresh cleared, J_opt = L.sum()
            # of the new nominal in t order (ilqr.py:209)
            e["fresh"][b] = 0
            e["J_opt"][b] = _sum_in_order(got["L"][b], dt)
    for k in STATE_KEYS:
        bad = np.flatnonzero(bits(got[k]) != bits(e[k]))
        assert bad.size == 0, (tag, k, bad[:6], got[k][bad[:6]],
                               e[k][bad[:6]], [kinds[i] for i in bad[:6]])
    want_live = np.bincount(np.flatnonzero(e["active"] == 1) % 256,
                            minlength=256)
    assert np.array_equal(got["n_live"], want_live), tag

    # ---- the winner copy
    acc = np.flatnonzero(amin >= 0)
    rest = np.flatnonzero(amin < 0)
    for k in ("Z", "U", "gains_acc"):
        assert np.array_equal(bits(got[k][rest]), bits(before[k][rest])), (
            tag, k)
    assert np.array_equal(bits(got["gains_acc"][acc]),
                          bits(got["gains"][acc])), tag
    scratch = got["_rec"].reshape(-1)[:B * (N + 1) * n].reshape(B, N + 1, n)
    n_rows = n_scratch = n_uc = n_tied = 0
    for b in acc:
        a = amin[b]
        src = got["Zc"][b, :, a]
        if not records and (not s.candidates_kept or a == 0) and \
                not np.isnan(scratch[b]).any():
            src = scratch[b]      # the full step's / a dropped winner's rows
            n_scratch += 1
        assert np.array_equal(bits(got["Z"][b]), bits(src)), (tag, b, a)
        n_rows += 1
        # a later candidate of the same cost with OTHER rows: a winner copy
        # that took it would have been seen
        n_tied += any(Jc[b, j] == Jc[b, a] and
                      not np.isnan(got["Zc"][b, :, j]).any() and
                      not np.array_equal(bits(got["Zc"][b, :, j]), bits(src))
                      for j in range(a + 1, A))
        if not np.isnan(got["Uc"][b, :, a]).any():   # (where Uc is written)
            assert np.array_equal(bits(got["U"][b]),
                                  bits(got["Uc"][b, :, a])), (tag, b, a)
            n_uc += 1
    # against the oracle's candidate of that step size, fed the kernel's gains
    # (compared where a 1e-9 change of the gains moves the fp64 cost by less
    # than 3e-8: test_benched_round_kernels_vs_oracle's gate); next to it what
    # the oracle's own run in the kernel's dtype loses against fp64
    o64, o_dt = orc.load(np.float64), orc.load(dt)
    k_, K_ = s.gain_views()
    k_, K_ = k_.cpu().numpy(), K_.cpu().numpy()
    n_oracle, errs = 0, []
    for b in (acc[:: max(1, len(acc) // 6)] if winner_bar else ()):
        al = np.array([float(s.alphas[amin[b]])])
        args = (before["Z"][b], before["U"][b])
        Zn, Un = o64.control_law(op, *args, k_[b], K_[b], al, u_min, u_max)
        Zp, Up = o64.control_law(op, *args, k_[b].astype(np.float64) *
                                 (1 + 1e-9), K_[b], al, u_min, u_max)
        J, Jp = o64.trajectory_cost(op, Zn, Un), o64.trajectory_cost(op, Zp, Up)
        if not (abs(Jp[0] - J[0]) / abs(J[0]) / 1e-9 < 30.0):
            continue
        Zo, Uo = o_dt.control_law(op, *args, k_[b], K_[b], al, u_min, u_max)
        n_oracle += 1
        errs.append((rel_err(got["Z"][b], Zn[:, 0]),
                     rel_err(got["U"][b], Un[:, 0]),
                     rel_err(Zo[:, 0], Zn[:, 0]), rel_err(Uo[:, 0], Un[:, 0])))
    if errs:
        m = np.max(np.array(errs), axis=0)
        print(tag, "winner vs fp64 oracle: Z %.3g U %.3g (the %s oracle's own: "
              "Z %.3g U %.3g)" % (m[0], m[1], dtype, m[2], m[3]))
        assert m[0] < WINNER_TOL[dtype] and m[1] < WINNER_TOL[dtype], (tag, m)
    print(tag, "accepted", len(acc), "copies checked", n_rows, "from scratch "
          "rows", n_scratch, "actions bit for bit", n_uc, "vs oracle", n_oracle)
    return dict(accepted=len(acc), states=set(e["state"][live].tolist()),
                oracle=n_oracle, nan0=nan0, tied_distinct=n_tied)


def _search_accept_path(problem, dtype, B, N, A, records, tag,
                        winner_bar=True):
    """Both step-size lists through pddp_search_accept_*: gains of the
    sweep on records in SWEEP's branch at its reg (the schedule's mu is then
    free: REG_ROWS)."""
    seen = dict(accepted=0, states=set(), oracle=0)
    for bounded in (False, True):
        branch, sweep_reg = SWEEP[problem]
        s, op, u_min, u_max = _solver(problem, dtype, B, N, A, branch, bounded)
        s.derivs()
        reg = torch.full((B,), sweep_reg, dtype=torch.float64,
                         device="cuda")
        s.backward(reg=reg, bounded=bounded)

        def launch(s_):
            return s_.search_accept(TOL, MAX_REG, N_IT, records=records)
        r = _run_case(s, op, u_min, u_max, dtype, launch, REG_ROWS, records,
                      not bounded, problem == "cartpole",
                      (tag, problem, dtype, B, N, A,
                       "box" if bounded else "free"), winner_bar)
        seen["accepted"] += r["accepted"]
        seen["states"] |= r["states"]
        seen["oracle"] += r["oracle"]
    # rejections by the NaN, acceptances from the bounded list
    assert seen["accepted"] > 0 and seen["states"] >= {1, 2, 4, 5}, seen
    assert seen["oracle"] > 0 or A == 1 or not winner_bar, seen


SHAPES = [(61, 16), (37, 127), (37, 140)]
OTHER_PROBLEMS = [("cartpole", "f64"), ("pendulum", "f32"), ("pendulum", "f64"),
                  ("double_cartpole", "f32"), ("double_cartpole", "f64")]
COUNTS = [1, 10, 11, 16]


@pytest.mark.parametrize("A", COUNTS)
@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("records", [True, False], ids=["records", "norec"])
def test_search_accept_cartpole_f32(records, B, N, A):
    """(37, 127): the tail's short form at its limit; (37, 140): its long
    form."""
    _search_accept_path("cartpole", "f32", B, N, A, records, "search_accept")


@pytest.mark.parametrize("A", COUNTS)
@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("knob,mode", [("pddp_search_candidates", 1),
                                       ("pddp_search_candidates", 2),
                                       ("pddp_search_form", 1),
                                       ("pddp_search_form", 2)])
def test_search_accept_cartpole_f32_knobs(knob, mode, B, N, A):
    """Candidates kept / dropped (a winner other than the full step is rolled
    out a second time) and the paired / dense form."""
    from pddp_amd import _native
    lib = _native.lib()
    prev_c = lib.pddp_search_candidates(-1)
    prev_f = lib.pddp_search_form(-1)
    try:
        getattr(lib, knob)(mode)
        _search_accept_path("cartpole", "f32", B, N, A, False,
                            "%s(%d)" % (knob, mode))
    finally:
        lib.pddp_search_candidates(prev_c)
        lib.pddp_search_form(prev_f)


@pytest.mark.parametrize("A", COUNTS)
@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("problem,dtype", OTHER_PROBLEMS)
def test_search_accept_other_problems(problem, dtype, B, N, A):
    """Decisions, schedule, masks and the winner copy, all by equality."""
    _search_accept_path(problem, dtype, B, N, A, True, "search_accept",
                        winner_bar=False)


@pytest.mark.parametrize("A", COUNTS)
@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("problem,dtype", OTHER_PROBLEMS)
def test_search_accept_other_problems_winner_vs_oracle(problem, dtype, B, N, A):
    """The same launches, the accepted nominal against `oracle.control_law`
    (fp64) at the winning step size, at the cartpole test's bars: 2e-5 in f32,
    1e-9 in f64.  Each run prints its figure next to that of the oracle's own
    IEEE run in the kernel's dtype on the same rows.  Measured on the MI355X,
    largest over the compared winners (the float32 oracle's own in brackets):
    f64 Z <= 1.1e-14, U <= 2.4e-13; f32 pendulum Z 8.2e-7 (6.9e-7), U 5.4e-6
    (6.2e-6); f32 double cartpole Z 4.2e-6 (5.3e-6), U 2.1e-7 (2.5e-7).
    (Under the V_zz-regularised sweep at reg = 1e4 the double cartpole's f32
    actions are 4.8e-5 ... 1.0e-4 from fp64 and the pendulum's 2.4e-5 at N =
    140 - exactly what the float32 oracle loses there, see SWEEP.)"""
    _search_accept_path(problem, dtype, B, N, A, True, "search_accept")


# (name, ILQRSolver branch, bounded): tests/test_cartpole_branches.py's COMBOS
# and the bounded eig-clamp branch
ROUND_COMBOS = [("eig", 0, False), ("chol", 1, False), ("chol_box", 1, True),
                ("eig_box", 0, True)]


@pytest.mark.parametrize("A", COUNTS)
@pytest.mark.parametrize("B,N", SHAPES[:2])
@pytest.mark.parametrize("combo", ROUND_COMBOS, ids=[c[0] for c in ROUND_COMBOS])
def test_one_launch_round_on_seeded_state(combo, B, N, A):
    """pddp_round_nominal_f32, rounds = 1: the sweep at the seeded mu, the
    search and the controller in one launch."""
    name, branch, bounded = combo
    s, op, u_min, u_max = _solver("cartpole", "f32", B, N, A, branch, bounded)

    def launch(s_):
        s_._one_launch = None
        return s_.round_nominal(TOL, MAX_REG, N_IT)
    r = _run_case(s, op, u_min, u_max, "f32", launch, ROUND_REG_ROWS, False,
                  not bounded, name != "eig",
                  ("round_nominal", name, B, N, A))
    if bounded:
        assert r["accepted"] > 0 and r["states"] >= {1, 2, 4, 5}, r
    else:  # the NaN wins: nothing but rejections and failed sweeps
        assert 4 in r["states"] and r["states"] & {2, 3}, r


# step sizes so small that the candidates' costs differ from one another by a
# few float32 ulps at most: tied minima whose rollouts are NOT the same rows
TINY_STEPS = [2.0 ** -e for e in (17, 18, 19, 20, 21, 22, 23, 24, 25, 26)]


@pytest.mark.parametrize("path", ["search_accept", "search_accept_norec",
                                  "round_nominal"])
def test_fused_argmin_takes_the_first_of_tied_minima(path):
    """The duplicated step sizes of the lists above tie with identical rows -
    which of them is copied cannot be seen.  Ten tiny step sizes instead
    (cartpole f32, bounded V_zz-regularised): at least one accepted trajectory
    must have a later candidate of exactly the winner's cost with other rows,
    and the nominal is the FIRST one's rows bit for bit."""
    B, N = 61, 16
    s, op, u_min, u_max = _solver("cartpole", "f32", B, N, 10, 1, True,
                                  steps=TINY_STEPS)
    if path == "round_nominal":
        def launch(s_):
            s_._one_launch = None
            return s_.round_nominal(TOL, MAX_REG, N_IT)
        rows, records = ROUND_REG_ROWS, False
    else:
        s.derivs()
        s.backward(reg=torch.full((B,), MU_SWEEP, dtype=torch.float64,
                                  device="cuda"))
        records = path == "search_accept"

        def launch(s_):
            return s_.search_accept(TOL, MAX_REG, N_IT, records=records)
        rows = REG_ROWS
    r = _run_case(s, op, u_min, u_max, "f32", launch, rows, records, False,
                  False, ("tied minima", path), winner_bar=False)
    print(path, r)
    assert r["tied_distinct"] > 0, r


@pytest.mark.parametrize("combo", ROUND_COMBOS, ids=[c[0] for c in ROUND_COMBOS])
def test_rounds_in_one_launch_from_seeded_state(combo):
    """rounds(4) against four round() calls from a seeded state (n_iterations
    = 2, max_reg = 150, mu = 100), bit for bit; and, read round by round from
    the single-round run: trajectories leave by CONVERGED, by MAX_REG and by
    the iteration count before the last round, and every array of a trajectory
    that has left stays bit-frozen."""
    name, branch, bounded = combo
    B, N, R, n_it, tol = 61, 16, 4, 2, 0.5
    sa, *_ = _solver("cartpole", "f32", B, N, 10, branch, bounded, huge=False)
    sb, *_ = _solver("cartpole", "f32", B, N, 10, branch, bounded, huge=False)
    b = np.arange(B)
    for s in (sa, sb):
        s.mu.fill_(MU_SWEEP)
        # b % 4: 0 natural (fresh); 1 a cost nothing can beat -> MAX_REG;
        # 2 / 3 a cost anything beats, in the last / first iteration
        fresh = torch.from_numpy((b % 4 == 0).astype(np.uint8)).cuda()
        J = np.where(b % 4 == 1, -np.inf, 1e30).astype(np.float32)
        s.fresh.copy_(fresh)
        s.J_opt.copy_(torch.from_numpy(J))
        s.iter.copy_(torch.from_numpy(
            np.where(b % 4 == 2, n_it, 1).astype(np.int32)))
    names = ("Z", "U", "L", "J_opt", "mu", "delta", "state", "iter", "active",
             "fresh", "gains", "gains_acc", "bwd_status", "n_live")
    eq = lambda x, y: torch.equal(torch.nan_to_num(x.double(), nan=1.5),
                                  torch.nan_to_num(y.double(), nan=1.5))
    sa.rounds(R, tol, MAX_REG, n_it)
    per_round = []
    for _ in range(R):
        sb.round(tol, MAX_REG, n_it)
        per_round.append({k: getattr(sb, k).clone() for k in names})
    assert sa._one_launch is True and sb._one_launch is True
    for k in names:
        assert eq(getattr(sa, k), getattr(sb, k)), k
    # how they left, before the last round
    left_by = {am.CONVERGED: 0, am.MAX_REG: 0, am.ACCEPTED: 0}
    frozen = [k for k in names if k not in ("n_live",) and
              not (k == "gains" and name == "eig_box")]
    for r in range(R - 1):
        gone = per_round[r]["active"] == 0
        if r:
            gone &= per_round[r - 1]["active"] != 0
        st = per_round[r]["state"][gone].cpu().numpy()
        for v in st:
            left_by[int(v)] += 1
        done = per_round[r]["active"] == 0
        for later in per_round[r + 1:]:
            for k in frozen:
                assert eq(later[k][done], per_round[r][k][done]), (r, k)
    print(name, "left before the last round by", left_by)
    assert all(v > 0 for v in left_by.values()), left_by
