"""The sampling planners under the line search's objective (pddp_shoot_* and
pddp_mppi_* with the suffixes _track, _weighted, _track_weighted,
pddp_mppi_trial_goals_*, csrc/sampled_goals.hip; ILQRSolver.shoot / mppi /
mppi_closed_loop with objective="search").  include/pddp_hip.h is the
definition: the siblings' laws word for word, every rollout costed along a
reference and / or under per-trajectory weights.

Each stage is held against a model fed with the device's previous stage
(DESIGN.md 3.4n), with the oracle stepped under each step's reference row and
each trajectory's diagonals (`sampled_goals_util.oracle_rollouts`).  The bars
are the project's own: `record_tol` (2e-4 f32, 1e-10 f64), 32 eps per weight,
64 S eps for ess, TOL["f64"] = 1e-9 for the float64 chains.

Shapes: B = 5, N = 6, 3 control steps; S in {1, 5, 70, 300}: one lane, a
partial group, several wavefronts, more than one turn.  Reference geometries
(GEOM): no hold; the hold inside the horizon; an offset window that moves
into the hold during a trial; everything held."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from abi_util import assert_entry_points, caller, cartpole_pointers
from golden_util import np_dtype, rel_err
from mppi_trial_util import noise_rows, shift, trial_names
from mppi_util import (model_e, model_update, model_weights, rounded,
                       weighted_actions)
from mppi_util import mppi_call as sibling_mppi_call
from sampled_goals_util import (chain_case, chain_lam, chain_model, mppi_call,
                                objective_solver, oracle_rollouts,
                                set_weights, shoot_call, trial_call)
from shoot_util import first_argmin, model_candidates
from solver_util import (BOUND, REARMED, SENTINEL, TOL, mpc_advance,
                         perturbed, record_tol, ref_row, ref_tensor,
                         same_bits, set_ref, to_device, trial_logs,
                         under_row)

gpu = pytest.mark.gpu
B, N, T = 5, 6, 3
SMOOTH, SEED = 0.7, 31
EPS = {"f32": 2.0 ** -23, "f64": 2.0 ** -52}
# (rows, first row): no hold; the hold inside the horizon; an offset window,
# a trial moving into the hold; everything held (first row >= rows - 1)
GEOM = {"none": (N + 1 + T, 0), "short": (3, 0), "offset": (N + 4, 2),
        "held": (4, 5)}
FAMILIES = ("shoot", "mppi")
SUFFIXES = ("track", "weighted", "track_weighted")
SYMBOLS = ["pddp_%s_%s_%s" % (f, x, t) for f in FAMILIES for x in SUFFIXES
           for t in ("f32", "f64")] + \
    ["pddp_mppi_trial_goals_f32", "pddp_mppi_trial_goals_f64"]


def _np(t):
    return t.cpu().numpy()


# ---- CPU ----------------------------------------------------------------------
def test_sampled_goals_entry_points_are_declared_exported_and_bound():
    """CPU: the 14 symbols in the header, the built library,
    exported_symbols() and _native._SIGS; each suffix is its sibling's
    arguments behind (problem, table) and the window and / or the weights,
    the trial's its sibling's with four more after the plant; the ABI version
    stays 1."""
    from pddp_amd import _native
    assert len(SYMBOLS) == 14
    assert_entry_points(SYMBOLS)
    P, I = ctypes.c_void_p, ctypes.c_int
    for fam in FAMILIES:
        rest = _native._SIGS["pddp_" + fam][1:]
        sig = {x: _native._SIGS["pddp_%s_%s" % (fam, x)] for x in SUFFIXES}
        assert sig["track"] == [P, P, P, I, I] + rest, fam
        assert sig["weighted"] == [P, P, P] + rest, fam
        assert sig["track_weighted"] == [P, P, P, I, I, P] + rest, fam
    sib = _native._SIGS["pddp_mppi_trial"]
    assert _native._SIGS["pddp_mppi_trial_goals"] == \
        sib[:3] + [P, I, I, P] + sib[3:]
    assert ctypes.CDLL(_native.LIB_PATH).pddp_hip_abi_version() == 1


def test_sampled_goals_entry_points_refuse_before_any_launch():
    """CPU (no device is touched: every answer comes before the first HIP
    call), both dtypes, every suffix with and without a table.
    PDDP_E_BADARG: weights = NULL where the name promises weights; ref = NULL,
    ref_len = 0, ref_t0 = -1 where it promises a reference; and the sibling's
    list - each null required pointer, B, N, S of 0 and negative,
    B S > 0x7fffffff, one of Z_out / U_out, U_out == U, Z_out == z0, smooth of
    1.0, -0.1 and NaN, mppi's lam and J_w and S > 256 without rows.
    PDDP_E_UNSUPPORTED: a DEFAULT-encoding problem.  The non-null pointers are
    host words nobody reads."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    r = q + 8
    lib = _native.lib()
    for t in ("f32", "f64"):
        #        0  1  2  3   4  5     6     7     8       9     10
        #        B  N  S  z0  U  umin  umax  astd  smooth  seed  off
        shoot = [2, 3, 4, q, q, None, None, q, 0.5, 7, 0,
                 #  11   12  13    14      15     16
                 #  act  Jc  best  J_best  Z_out  U_out
                 None, q, q, q, r, r]
        #       0  1  2  3   4  5     6     7     8    9       10    11
        #       B  N  S  z0  U  umin  umax  astd  lam  smooth  seed  off
        mppi = [2, 3, 4, q, q, None, None, q, q, 0.5, 7, 0,
                #  12   13  14    15      16  17   18     19
                #  act  Jc  best  J_best  W   J_w  Z_out  U_out
                None, q, q, q, None, q, r, r]
        families = {
            "shoot": (shoot, (3, 4, 7, 12, 13), 8, (15, 16)),
            "mppi": (mppi, (3, 4, 7, 8, 13, 14, 17), 9, (18, 19))}
        for fam, (good, required, smooth_at, (zo, uo)) in families.items():
            leads = {
                "track": (lambda tab: (tab, q, 5, 0),
                          [lambda tab: (tab, None, 5, 0),
                           lambda tab: (tab, q, 0, 0),
                           lambda tab: (tab, q, 5, -1)]),
                "weighted": (lambda tab: (tab, q),
                             [lambda tab: (tab, None)]),
                "track_weighted": (lambda tab: (tab, q, 5, 0, q),
                                   [lambda tab: (tab, None, 5, 0, q),
                                    lambda tab: (tab, q, 0, 0, q),
                                    lambda tab: (tab, q, 5, -1, q),
                                    lambda tab: (tab, q, 5, 0, None)])}
            for suf, (ok, bad_leads) in leads.items():
                call = caller(getattr(lib, "pddp_%s_%s_%s" % (fam, suf, t)),
                              good)
                tag = (fam, suf, t)
                for tab in (None, q):
                    # (never the good call: it would launch on host words)
                    for lead in bad_leads:
                        assert call(pp, *lead(tab)) == -1, tag
                    for i in required:
                        assert call(pp, *ok(tab), **{"_%d" % i: None}) == -1, \
                            (tag, i)
                    assert call(None, *ok(tab)) == -1, tag
                    for i in (0, 1, 2):
                        assert call(pp, *ok(tab), **{"_%d" % i: 0}) == -1, tag
                        assert call(pp, *ok(tab), **{"_%d" % i: -3}) == -1, tag
                    assert call(pp, *ok(tab), _0=1 << 16, _2=1 << 15) == -1, \
                        tag
                    assert call(pp, *ok(tab), **{"_%d" % zo: None}) == -1, tag
                    assert call(pp, *ok(tab), **{"_%d" % uo: None}) == -1, tag
                    assert call(pp, *ok(tab), **{"_%d" % uo: q}) == -1, tag
                    assert call(pp, *ok(tab), _3=r) == -1, tag
                    for smooth in (1.0, -0.1, float("nan")):
                        assert call(pp, *ok(tab),
                                    **{"_%d" % smooth_at: smooth}) == -1, tag
                    if fam == "mppi":
                        assert call(pp, *ok(tab), _2=300, _18=None,
                                    _19=None) == -1, tag
                    assert call(ppd, *ok(tab)) == _native.E_UNSUPPORTED, tag
                    # (the suffix's own test comes before the encoding's)
                    assert call(ppd, *bad_leads[0](tab)) == -1, tag


def test_trial_goals_entry_points_refuse_before_any_launch():
    """CPU, both dtypes: PDDP_E_BADARG for neither a reference nor weights,
    for a reference with ref_len < 1, ref_t0 < 0 or ref_t0 + TT beyond an
    int, and for pddp_mppi_trial_*'s own list; PDDP_E_UNSUPPORTED for a
    DEFAULT-encoding problem.  A reference alone, weights alone and both get
    past the additions' tests (shown by the encoding's answer)."""
    from pddp_amd import _native
    pp, ppd, q = cartpole_pointers()
    r = q + 8
    lib = _native.lib()
    for t in ("f32", "f64"):
        #       0      1      2    3        4       5
        #       table  plant  ref  ref_len  ref_t0  weights
        good = [None, None, q, 9, 0, q,
                # 6  7  8  9  10  11  12     13  14 15 16
                # B  N  S  K  TT  t0  count  z0  U  Z  U_work
                2, 3, 4, 2, 5, 1, 3, q, q, q, r,
                # 17    18    19    20   21      22    23    24
                # umin  umax  astd  lam  smooth  seed  cand  stride
                None, None, q, q, 0.5, 7, 0, 8,
                # 25    26     27     28    29    30      31   32  33
                # dist  w_std  v_std  roll  step  x_true  act  Jc  log_costs
                None, None, None, 0, 0, None, None, q, 0,
                # 34    35    36   37    38  39  40   41
                # Xlog  Ulog  Jcl  Ylog  J0  Jw  ess  plans
                q, q, q, None, None, None, None, None]
        call = caller(getattr(lib, "pddp_mppi_trial_goals_" + t), good)
        assert call(pp, _2=None, _5=None) == -1, t      # neither
        assert call(pp, _3=0) == -1, t                  # ref_len
        assert call(pp, _4=-1) == -1, t                 # ref_t0
        assert call(pp, _4=(1 << 31) - 5) == -1, t      # ref_t0 + TT
        assert call(pp, _4=(1 << 31) - 5, _5=None) == -1, t
        for i in (13, 14, 19, 20, 32):             # pddp_mppi_*'s pointers
            assert call(pp, **{"_%d" % i: None}) == -1, (t, i)
        assert call(None) == -1, t
        for i in (6, 7, 8):                        # B, N, S
            assert call(pp, **{"_%d" % i: 0}) == -1, (t, i)
            assert call(pp, **{"_%d" % i: -3}) == -1, (t, i)
        assert call(pp, _6=1 << 16, _8=1 << 15) == -1, t
        for smooth in (1.0, -0.1, float("nan")):
            assert call(pp, _21=smooth) == -1, (t, smooth)
        for i, bad in ((9, 0), (9, -1), (10, 0), (10, -2), (11, -1), (12, 0),
                       (12, -1), (12, 5), (11, 3)):   # K, TT, t0, count
            assert call(pp, **{"_%d" % i: bad}) == -1, (t, i, bad)
        for i in (15, 16, 34, 35, 36):             # Z, U_work, the logs
            assert call(pp, **{"_%d" % i: None}) == -1, (t, i)
        assert call(pp, _16=q) == -1, t            # U_work == U
        assert call(pp, _27=q) == -1, t            # v_std without x_true
        assert call(pp, _29=-1) == -1, t           # step_offset
        assert call(pp, _29=(1 << 31) - 5) == -1, t
        assert call(ppd) == _native.E_UNSUPPORTED, t
        assert call(ppd, _2=None, _3=0) == _native.E_UNSUPPORTED, t  # weights
        assert call(ppd, _5=None) == _native.E_UNSUPPORTED, t        # ref
        assert call(ppd, _0=q, _1=q, _4=(1 << 31) - 6) == \
            _native.E_UNSUPPORTED, t
        assert call(ppd, _2=None, _5=None) == -1, t


def test_tracked_oracle_rollouts_reduce_to_the_plain_ones():
    """CPU: the composition the GPU tests compare against.  With every
    reference row the problem's own goals it is `shoot_util.oracle_rollouts`
    to the bit; a row that differs at index N alone moves the terminal term
    alone; first rows at and beyond the last row read the last row."""
    from shoot_util import oracle_rollouts as plain
    from solver_util import fresh_ops, reference_rows
    rng = np.random.RandomState(2)
    for problem in ("cartpole", "rendezvous"):
        ops = fresh_ops(problem, 2)
        na, m, n = ops[0].aug_size, ops[0].action_size, ops[0].encoded_size
        z0 = 0.1 * rng.randn(2, n)
        Uc = rng.randn(2, 3, 4, m)
        xr = np.tile(np.array(ops[0].x_goal[:na]), (2, 5, 1))
        ur = np.tile(np.array(ops[0].u_goal[:m]), (2, 5, 1))
        X0, J0 = plain(ops, z0, Uc, "f64")
        X1, J1 = oracle_rollouts(fresh_ops(problem, 2), z0, Uc, "f64", xr, ur,
                                 1)
        assert (X0 == X1).all() and (J0 == J1).all(), problem
        xr2 = xr.copy()
        xr2[:, 4] += 0.3
        o = fresh_ops(problem, 2)
        _, J2 = oracle_rollouts(o, z0, Uc, "f64", xr2, ur, 0)
        assert (J2 != J0).all(), problem
        xr3, _ = reference_rows(problem, 2, 3, seed=1)
        ur3 = np.tile(np.array(ops[0].u_goal[:m]), (2, 3, 1))
        _, Ja = oracle_rollouts(o, z0, Uc, "f64", xr3, ur3, 2)
        _, Jb = oracle_rollouts(o, z0, Uc, "f64", xr3, ur3, 7)
        _, Jc = oracle_rollouts(o, z0, Uc, "f64", xr3[:, 2:], ur3[:, 2:], 0)
        assert (Ja == Jb).all() and (Ja == Jc).all(), problem


# ---- GPU: what the tests share --------------------------------------------------
def _lam_of(J):
    """0.5 (median_s J - min_s J) per trajectory, 1 where that is 0 (S = 1)."""
    J = np.asarray(J, np.float64)
    lam = 0.5 * (np.median(J, axis=1) - J.min(axis=1))
    return np.where(lam > 0, lam, 1.0)


@functools.lru_cache(maxsize=None)
def _setup(problem, dtype, form, table, geom="offset", S=5, smooth=SMOOTH):
    """A solver with the objective set, the oracle's costs along the model's
    candidates under it (computed once, shared, left unchanged) and a
    temperature per trajectory from them."""
    L, t0 = GEOM[geom]
    c = objective_solver(problem, dtype, B, N, form, table, L, t0)
    c.S, c.smooth, c.std = S, smooth, 0.3 * BOUND[problem]
    c.Uc, c.hit = model_candidates(c.U, S, c.std, smooth, SEED, 0, dtype,
                                   c.u_min, c.u_max)
    c.X_orc, c.J_orc = oracle_rollouts(c.ops, c.z0, c.Uc, dtype, c.xr, c.ur,
                                       c.t0)
    c.lam = rounded(_lam_of(c.J_orc), dtype)
    c.e = model_e(B, N, S, c.s.m, smooth, SEED, 0, dtype)
    c.tag = (problem, dtype, form, table, geom, S, smooth)
    return c


def _check_selection(c, out):
    """best and J_best exactly on the device's own costs; against the
    oracle's choice where the oracle's gap exceeds four times the bar."""
    J = _np(out.J)
    best = _np(out.best)
    assert (best == first_argmin(J)).all(), (c.tag, best, first_argmin(J))
    for b in range(B):
        assert 0 <= best[b] < c.S, (c.tag, b, best[b])
        assert _np(out.J_best[b]).tobytes() == J[b, best[b]].tobytes(), b
    Jo = c.J_orc.astype(np.float64)
    if c.S > 1:
        order = np.sort(Jo, axis=1)
        clear = order[:, 1] - order[:, 0] > \
            4 * record_tol(c.dtype) * np.abs(order[:, 0])
        assert (best[clear] == Jo.argmin(axis=1)[clear]).all(), c.tag
    assert bool((out.J_best <= out.J[:, 0]).all())


def _check_shoot(c, out):
    """Jc of every candidate within record_tol of the oracle under the
    objective; the selection; Z_out / U_out the winner's rows."""
    tol = record_tol(c.dtype)
    J = _np(out.J)
    _check_selection(c, out)
    best = _np(out.best)
    for b in range(B):
        e = (rel_err(J[b], c.J_orc[b]),
             rel_err(_np(out.Z[b]), c.X_orc[b, best[b]]),
             rel_err(_np(out.U[b]), c.Uc[b, best[b]]))
        print(c.tag, b, "best", best[b], "J, Z, U off by", e, "bar", tol)
        assert max(e) < tol, (c.tag, b, e)


# the covering set of stage 1: every problem with "both + table" in both
# types; every other form with and without a table, every S, both smooth
#        problem            dtype  form       table  geom      S    smooth
COSTS = [(p, d, "both", True, g, 5, sm)
         for p, g, sm in (("cartpole", "offset", 0.7),
                          ("pendulum", "short", 0.0),
                          ("double_cartpole", "none", 0.7),
                          ("rendezvous", "held", 0.0))
         for d in ("f64", "f32")] + [
    ("cartpole",        "f64", "ref",     False, "short",  70,  0.0),
    ("cartpole",        "f32", "ref",     True,  "offset", 300, 0.7),
    ("cartpole",        "f32", "weights", False, "none",   70,  0.7),
    ("cartpole",        "f64", "weights", True,  "none",   1,   0.0),
    ("cartpole",        "f64", "both",    False, "held",   300, 0.7),
    ("pendulum",        "f32", "ref",     False, "held",   5,   0.7),
    ("pendulum",        "f64", "weights", False, "none",   5,   0.7),
    ("double_cartpole", "f64", "ref",     True,  "short",  5,   0.0),
    ("double_cartpole", "f32", "weights", True,  "none",   5,   0.7),
    ("rendezvous",      "f64", "weights", False, "none",   70,  0.7),
    ("rendezvous",      "f32", "ref",     False, "offset", 70,  0.7),
    ("cartpole",        "f32", "both",    False, "none",   5,   0.0),
    ("cartpole",        "f64", "both",    False, "short",  5,   0.7),
    ("cartpole",        "f32", "both",    False, "held",   5,   0.7)]


# ---- GPU, stage 1: the costs ------------------------------------------------------
@gpu
@pytest.mark.parametrize("problem,dtype,form,table,geom,S,smooth", COSTS)
def test_candidate_costs_vs_oracle(problem, dtype, form, table, geom, S,
                                   smooth):
    """pddp_shoot_{track,weighted,track_weighted}_*: bounded, std = 0.3 BOUND
    around wide base actions (the clamp is met on some steps and not on
    others where there is more than the base).  Jc against the oracle under
    the objective, best, J_best, Z_out, U_out (`_check_shoot`)."""
    c = _setup(problem, dtype, form, table, geom, S, smooth)
    if S > 1:
        assert c.hit[:, 1:].any() and not c.hit[:, 1:].all(), c.hit.mean()
    assert (c.s.reference is not None) == (form != "weights")
    assert (c.s.batch_weights is not None) == (form != "ref")
    _check_shoot(c, shoot_call(c.s, S, c.std, smooth, SEED))


# ---- GPU, stage 2: the objective is really read -----------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_table_goals_are_not_read_under_a_reference(dtype):
    """A table whose goal fields hold 1e3 gives the same bits under a
    reference, in all three families; its parameters are read (another
    parameter row moves the costs)."""
    c = _setup("cartpole", dtype, "both", True)
    s = c.s
    table = s.batch_table
    other = table.clone()
    other[:, 8:20] = 1e3
    moved = table.clone()
    moved[:, 0] *= 1.1  # (dt)
    try:
        outs = {}
        for key, tab in (("own", table), ("goals", other), ("dt", moved)):
            s.batch_table = tab
            outs[key] = (
                shoot_call(s, 5, c.std, SMOOTH, SEED),
                mppi_call(s, 5, c.std, c.lam, SMOOTH, SEED),
                trial_call(s, 5, 2, T, c.std, c.lam, SMOOTH, SEED))
    finally:
        s.batch_table = table
    for a, b in zip(outs["own"][:2], outs["goals"][:2]):
        for nm, x in vars(a).items():
            assert same_bits(x, getattr(b, nm)), nm
    for nm in trial_names(outs["own"][2]):
        assert same_bits(getattr(outs["own"][2], nm),
                         getattr(outs["goals"][2], nm)), nm
    assert not same_bits(outs["own"][0].J, outs["dt"][0].J)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("form", ["weights", "both"])
def test_another_weights_row_moves_the_costs(form, dtype):
    """Trajectory 0 costed under trajectory 1's weights row differs from its
    own by more than the bar (record_tol relative) on every candidate, the
    other trajectories keep their bits."""
    c = _setup("cartpole", dtype, form, False)
    own = shoot_call(c.s, 5, c.std, SMOOTH, SEED)
    w = c.s.batch_weights.clone()
    w[0] = w[1]
    out = shoot_call(c.s, 5, c.std, SMOOTH, SEED, wts=w)
    d = (_np(out.J[0]).astype(np.float64) - _np(own.J[0])) / _np(own.J[0])
    print(form, dtype, "relative move of trajectory 0's costs", d)
    assert (np.abs(d) > record_tol(dtype)).all(), d
    assert same_bits(out.J[1:], own.J[1:])


@gpu
@pytest.mark.parametrize("form", ["ref", "both"])
def test_row_N_moves_the_terminal_term_alone_f64(form):
    """f64, a reference of N + 1 rows read from row 0: another x_goal in row N
    alone changes every candidate's cost by what it changes in the oracle's
    (the terminal term), within record_tol of the cost; another u_goal in row
    N changes no bit - the terminal step reads x_goal only."""
    dtype = "f64"
    c = objective_solver("cartpole", dtype, B, N, form, False, N + 1, 0)
    std = 0.3 * BOUND["cartpole"]
    Uc, _ = model_candidates(c.U, 5, std, SMOOTH, SEED, 0, dtype, c.u_min,
                             c.u_max)
    own = shoot_call(c.s, 5, std, SMOOTH, SEED)
    na = c.s.problem.aug_size
    xr2 = c.xr.copy()
    xr2[:, N] += 0.3
    ur2 = c.ur.copy()
    ur2[:, N] += 0.3
    out = shoot_call(c.s, 5, std, SMOOTH, SEED,
                     ref=ref_tensor(xr2, c.ur, dtype))
    same = shoot_call(c.s, 5, std, SMOOTH, SEED,
                      ref=ref_tensor(c.xr, ur2, dtype))
    assert same_bits(same.J, own.J) and same_bits(same.U, own.U)
    _, J1 = oracle_rollouts(c.ops, c.z0, Uc, dtype, c.xr, c.ur, 0)
    _, J2 = oracle_rollouts(c.ops, c.z0, Uc, dtype, xr2, c.ur, 0)
    dev = _np(out.J) - _np(own.J)
    assert (np.abs(J2 - J1) > 1e-3).all(), (J2 - J1)
    err = np.abs(dev - (J2 - J1)).max() / np.abs(J1).max()
    print(form, "terminal term's move off the oracle's by", err, na)
    assert err < record_tol(dtype), err


# ---- GPU, stage 3: the degenerate objective ------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", ["cartpole", "rendezvous"])
def test_degenerate_objective_equals_the_batch_sibling(problem, dtype):
    """Every reference row the table's goals and every weights row the shared
    diagonals: pddp_mppi_track_weighted_* gives pddp_mppi_batch_*'s Jc, W,
    U_out and J_w within record_tol (another kernel: to rounding, not to the
    bit).  The temperature is the spread of the costs, so the softmin
    amplifies nothing."""
    from mppi_util import wide_solver
    s, ops, z0, U, u_min, u_max = wide_solver(problem, dtype, B, N,
                                              table=True)
    std = 0.3 * BOUND[problem]
    first = sibling_mppi_call(s, 5, std, 1.0, SMOOTH, SEED)
    J = _np(first.J).astype(np.float64)
    lam = rounded(J.max(axis=1) - J.min(axis=1), dtype)
    want = sibling_mppi_call(s, 5, std, lam, SMOOTH, SEED)
    _, xg, ug, _ = perturbed(problem, B, seed=41)
    set_ref(s, np.tile(xg[:, None], (1, 4, 1)), np.tile(ug[:, None],
                                                        (1, 4, 1)), 1)
    s.set_batch_weights(keep_reference=True)
    got = mppi_call(s, 5, std, lam, SMOOTH, SEED)
    tol = record_tol(dtype)
    for nm in ("J", "W", "U", "J_w", "Z"):
        e = rel_err(_np(getattr(got, nm)), _np(getattr(want, nm)))
        print(problem, dtype, nm, "off the _batch sibling by", e)
        assert e < tol, (nm, e)
    assert torch.equal(got.best, want.best)


# ---- GPU, stage 4: window algebra, bit for bit ------------------------------------------
def _all_three(c, S, **kw):
    """One launch of each family on the same arguments."""
    return (shoot_call(c.s, S, c.std, SMOOTH, SEED, **kw),
            mppi_call(c.s, S, c.std, c.lam, SMOOTH, SEED, **kw))


def _assert_same(a, b, what, rows=slice(None), rows_b=slice(None)):
    names = trial_names(a) if hasattr(a, "plans") else \
        [k for k, v in vars(a).items() if v is not None]
    for nm in names:
        x, y = getattr(a, nm)[rows], getattr(b, nm)[rows_b]
        assert same_bits(x, y), (what, nm)


def _trial(c, S, K=2, **kw):
    kw.setdefault("w_std", 0.02)
    kw.setdefault("v_std", 0.01)
    kw.setdefault("roll", 40)
    return trial_call(c.s, S, K, T, c.std, c.lam, SMOOTH, SEED, step_offset=2,
                      **kw)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_a_first_row_is_a_sliced_reference(S, dtype):
    """ref_t0 = k on `ref` equals ref_t0 = 0 on ref[:, k:], for all three
    families: the offset window (k = 2, the trial moving into the hold) and a
    first row beyond the last (k = rows + 3 against the last row alone)."""
    c = _setup("cartpole", dtype, "both", True, "offset")
    ref = c.s.reference
    L = ref.shape[1]
    for k, cut in ((2, 2), (L + 3, L - 1)):
        sliced = ref[:, cut:].contiguous()
        for a, b in zip(_all_three(c, S, t0=k),
                        _all_three(c, S, ref=sliced, t0=0)):
            _assert_same(a, b, (S, dtype, k))
        _assert_same(_trial(c, S, t0=k), _trial(c, S, ref=sliced, t0=0),
                     (S, dtype, k, "trial"))


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_tail_of_the_batch_alone(S, dtype):
    """Trajectories 2.. alone - sample_offset + 2 S, their slices of the
    table, the reference and the weights (the trial: the ORIGINAL B S as
    iter_stride, rollout_offset + 2) - are their rows of the full launch, bit
    for bit; with another trajectory's slices they are not."""
    c = _setup("cartpole", dtype, "both", True, "offset")
    for full, tail in zip(_all_three(c, S),
                          _all_three(c, S, b0=2, offset=2 * S)):
        _assert_same(full, tail, (S, dtype), rows=slice(2, None))
    full = _trial(c, S)
    tail = _trial(c, S, b0=2, cand=2 * S, roll=42)
    _assert_same(full, tail, (S, dtype, "trial"), rows=slice(2, None))
    rolled = torch.roll(c.s.reference, 1, 0).contiguous()
    moved = shoot_call(c.s, S, c.std, SMOOTH, SEED, b0=2, offset=2 * S,
                       ref=rolled)
    assert not same_bits(moved.J, _all_three(c, S)[0].J[2:])


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reproducible_lean_and_masked(dtype):
    """S = 70.  The same call twice gives the same bits; the optional outputs
    left out (shoot: J_best and the rows; mppi: W and the rows; the trial:
    the logs) change no other bit; active = [1, 0, 1, 0, 1]: nothing of
    trajectories 1 and 3 is read (their z0 and U are NaN) or written (every
    output row still holds the sentinel), the others as without the mask."""
    S = 70
    c = _setup("cartpole", dtype, "both", True, "offset")
    a, b = _all_three(c, S), _all_three(c, S)
    for x, y in zip(a, b):
        _assert_same(x, y, dtype)
    ta = _trial(c, S)
    _assert_same(ta, _trial(c, S), (dtype, "trial"))
    lean = shoot_call(c.s, S, c.std, SMOOTH, SEED, rows=False, best=False)
    assert same_bits(lean.J, a[0].J) and torch.equal(lean.best, a[0].best)
    lean = mppi_call(c.s, S, c.std, c.lam, SMOOTH, SEED, rows=False, W=False)
    for nm in ("J", "best", "J_best", "J_w"):
        assert same_bits(getattr(lean, nm), getattr(a[1], nm)), nm
    lean = _trial(c, S, logs=False, log_costs=False)
    for nm in ("z0", "U", "Z", "X", "Ulog", "J", "Y", "x_true"):
        assert same_bits(getattr(ta, nm), getattr(lean, nm)), nm
    z0, U = c.s.z0.clone(), c.s.U.clone()
    off, on = [1, 3], [0, 2, 4]
    z0[off], U[off] = float("nan"), float("nan")
    lam = c.lam.copy()
    lam[off] = np.nan
    active = torch.tensor([1, 0, 1, 0, 1], dtype=torch.uint8, device="cuda")
    shot = shoot_call(c.s, S, c.std, SMOOTH, SEED, active=active, z0=z0, U=U)
    mp = mppi_call(c.s, S, c.std, lam, SMOOTH, SEED, active=active, z0=z0,
                   U=U)
    for out, clean in ((shot, a[0]), (mp, a[1])):
        for nm, x in vars(out).items():
            want = -9 if nm == "best" else SENTINEL
            assert bool((x[off] == want).all()), nm
        _assert_same(out, clean, dtype, rows=on, rows_b=on)
    tr = trial_call(c.s, S, 2, T, c.std, lam, SMOOTH, SEED, step_offset=2,
                    w_std=0.02, v_std=0.01, roll=40, active=active, z0=z0,
                    U=U)
    for nm in trial_names(tr):
        x = getattr(tr, nm)[off]
        if nm in ("z0", "U", "x_true"):
            assert bool(torch.isnan(x).all()), nm
        elif nm == "Y":  # (row 0 is the caller's)
            assert bool((x[:, 1:] == SENTINEL).all()), nm
        else:
            assert bool((x == SENTINEL).all()), nm
    _assert_same(tr, ta, (dtype, "trial"), rows=on, rows_b=on)


# ---- GPU, stage 5: the MPPI stages ---------------------------------------------------
#         problem            dtype  form       table  geom      S    smooth
STAGES = [c for c in COSTS if c[2] == "both" and c[3]] + [
    ("cartpole",   "f64", "ref",     False, "short",  70,  0.0),
    ("cartpole",   "f32", "weights", False, "none",   70,  0.7),
    ("cartpole",   "f64", "both",    False, "held",   300, 0.7),
    ("cartpole",   "f32", "ref",     True,  "offset", 300, 0.7),
    ("cartpole",   "f64", "weights", True,  "none",   1,   0.0),
    ("rendezvous", "f64", "weights", False, "none",   70,  0.7),
    ("rendezvous", "f32", "ref",     False, "offset", 70,  0.7)]


@gpu
@pytest.mark.parametrize("problem,dtype,form,table,geom,S,smooth", STAGES)
def test_mppi_stages_vs_models(problem, dtype, form, table, geom, S, smooth):
    """pddp_mppi_{track,weighted,track_weighted}_*, as tests/test_mppi.py
    holds its siblings: Jc against the oracle under the objective and the
    selection (stage 1); W against the float64 softmin of the device's own
    costs, 32 eps absolute, rows summing to 1 (stage 2); U_out against
    clip(U + std sum_s W_dev e_model) (stage 3); Z_out and J_w against the
    oracle under the objective along the device's own U_out (stage 4) - all
    within record_tol.  The rendezvous at S = 70: m = 4 sums through LDS."""
    c = _setup(problem, dtype, form, table, geom, S, smooth)
    out = mppi_call(c.s, S, c.std, c.lam, smooth, SEED)
    tol = record_tol(dtype)
    J = _np(out.J)
    for b in range(B):
        e = rel_err(J[b], c.J_orc[b])
        print(c.tag, b, "J off by", e)
        assert e < tol, (c.tag, b, e)
    _check_selection(c, out)
    Wm = model_weights(J, c.lam)
    Wd = _np(out.W).astype(np.float64)
    dev = np.abs(Wd - Wm).max() / EPS[dtype]
    rows = np.abs(Wd.sum(axis=1) - 1.0).max() / EPS[dtype]
    print(c.tag, "W off by %.2f eps, rows off 1 by %.2f eps (bar 32)" %
          (dev, rows))
    assert dev <= 32 and rows <= 32, (c.tag, dev, rows)
    Um = weighted_actions(c.U, Wd, c.e, c.std, c.u_min, c.u_max)
    Ud = _np(out.U)
    X, Jw = oracle_rollouts(c.ops, c.z0, Ud[:, None], dtype, c.xr, c.ur, c.t0)
    for b in range(B):
        e = (rel_err(Ud[b], Um[b]), rel_err(_np(out.Z[b]), X[b, 0]),
             rel_err(_np(out.J_w[b]), Jw[b, 0]))
        print(c.tag, b, "U_out, Z_out, J_w off by", e)
        assert max(e) < tol, (c.tag, b, e)
    if S == 1:
        assert bool((out.W == 1).all())
        assert torch.equal(out.U, torch.minimum(torch.maximum(
            c.s.U, c.s.u_min), c.s.u_max))


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_no_weighted_sequence(S, dtype):
    """Trajectory 1 without a finite candidate (a NaN start), and with a
    temperature of 0, of NaN and below 0: best -1, J_best and J_w +inf, its
    row of W zeros, its rows of Z_out / U_out keep the sentinel; the costs are
    written all the same.  The others are what they are without it, bit for
    bit."""
    c = _setup("cartpole", dtype, "both", True, "offset")
    s = c.s
    clean = mppi_call(s, S, c.std, 40.0, SMOOTH, 23)
    assert bool((clean.best >= 0).all())
    z0 = s.z0.clone()
    z0[1] = float("nan")
    runs = [("nan start", mppi_call(s, S, c.std, 40.0, SMOOTH, 23, z0=z0))]
    for bad in (0.0, float("nan"), -1.0):
        lam = np.full(B, 40.0)
        lam[1] = bad
        runs.append((bad, mppi_call(s, S, c.std, lam, SMOOTH, 23)))
    for what, out in runs:
        assert out.best[1].item() == -1, what
        assert out.J_best[1].item() == float("inf"), what
        assert out.J_w[1].item() == float("inf"), what
        assert bool((out.W[1] == 0).all()), what
        assert bool((out.Z[1] == SENTINEL).all() and
                    (out.U[1] == SENTINEL).all()), what
        if what == "nan start":
            assert bool(torch.isnan(out.J[1]).all())
        else:
            assert torch.equal(out.J[1], clean.J[1]), what
        _assert_same(out, clean, what, rows=[0, 2, 3, 4], rows_b=[0, 2, 3, 4])


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70])
def test_one_hot_weights_give_shoots_winner(S, dtype):
    """With lam a thousandth of the smallest gap between the best and the
    second-best DEVICE cost over the batch, every other exponent is below
    -1000 and its exp is 0 in both types: W is one-hot at best, and
    pddp_mppi_track_weighted_*'s U_out has the BITS of
    pddp_shoot_track_weighted_*'s on the same arguments - the e chain, the
    products w_s e and the final fma are the same explicit operations."""
    c = _setup("cartpole", dtype, "both", True, "offset")
    first = mppi_call(c.s, S, c.std, 1.0, SMOOTH, SEED)
    Jd = np.sort(_np(first.J).astype(np.float64), axis=1)
    g = (Jd[:, 1] - Jd[:, 0]).min()
    assert g > 0, g
    out = mppi_call(c.s, S, c.std, g / 1000, SMOOTH, SEED)
    best = _np(out.best)
    hot = np.zeros((B, S))
    hot[np.arange(B), best] = 1.0
    assert (_np(out.W) == hot).all(), out.W
    shot = shoot_call(c.s, S, c.std, SMOOTH, SEED)
    assert torch.equal(shot.best, out.best)
    assert bool((shot.best > 0).any()), shot.best
    assert torch.equal(out.U, shot.U)


# ---- GPU, stage 6: the trial ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("S", [5, 70, 300])
def test_one_launch_is_three_launches(S, dtype):
    """K = 2, both noises, a plant table, a table, weights and the offset
    reference, whose hold is entered at control step 2: count = 3 in one
    launch against three launches with count = 1 and against 2 + 1, every
    output and log bit for bit.  A stale read of U[b] or z0[b], or a window
    that does not move inside the launch, shows as a bit; a window that does
    not move at all shows against the sliced reference of
    test_a_first_row_is_a_sliced_reference and the oracle's rows below."""
    c = _setup("cartpole", dtype, "both", True, "offset")
    par, _, _, _ = perturbed("cartpole", B, 11)
    plant = c.s._plant_table("test", torch.from_numpy(par), None, None)
    one = _trial(c, S, plant=plant)
    _assert_same(one, _trial(c, S, plant=plant, chunks=[1, 1, 1]), (S, dtype))
    _assert_same(one, _trial(c, S, plant=plant, chunks=[2, 1]),
                 (S, dtype, "2 + 1"))
    took = torch.isfinite(one.Jw) & (one.Jw <= one.J0)
    print(S, dtype, "took", took.float().mean().item())
    assert bool(took.any()), "no iteration took: nothing was handed over"


#          problem            dtype  form       table  plant  geom      S    K
TRIALS = [("cartpole",        "f64", "both",    True,  True,  "offset", 5,   1),
          ("cartpole",        "f32", "both",    True,  True,  "offset", 5,   1),
          ("pendulum",        "f64", "both",    True,  False, "short",  5,   1),
          ("pendulum",        "f32", "ref",     False, True,  "none",   5,   1),
          ("double_cartpole", "f64", "weights", False, True,  "none",   5,   1),
          ("double_cartpole", "f32", "both",    True,  True,  "held",   5,   1),
          ("rendezvous",      "f64", "both",    True,  True,  "offset", 70,  1),
          ("rendezvous",      "f32", "ref",     False, False, "short",  70,  1),
          ("cartpole",        "f64", "ref",     False, True,  "offset", 300, 1),
          ("cartpole",        "f32", "both",    False, True,  "offset", 300, 2),
          ("cartpole",        "f64", "both",    False, True,  "offset", 70,  2),
          ("cartpole",        "f32", "weights", True,  True,  "none",   1,   2)]


@gpu
@pytest.mark.parametrize("problem,dtype,form,table,plant,geom,S,K", TRIALS)
def test_trial_stages_vs_models(problem, dtype, form, table, plant, geom, S,
                                K):
    """pddp_mppi_trial_goals_*, stage by stage as tests/test_mppi_trial.py
    holds its sibling (both noises, a disturbance, log_costs on), with
    y_c = Ylog[:, c] and the base of step c the shift of plan_log[:, c - 1]:

      K = 1: Jc[:, c, 0] against the oracle under the window that starts at
             row min(ref_t0 + c, L - 1) along the model's candidates;
             plan_log where took against model_update fed with the device's
             Jc, Jw_log against the oracle along plan_log - record_tol;
      J0_log is Jc[..., 0] exactly; without a took plan_log is the base;
      ess_log against the float64 softmin of the device's Jc, 64 S eps;
      Ulog[:, c] is clip(plan_log[:, c, 0]) exactly;
      the plant step and the observation against the oracle's step of the
             plant (the plant row's PARAMETERS) plus the model's normals;
      Jcl against the oracle's costs along Xlog, Ulog under the SHARED Q,
             Q_term, R and, with a reference, row ref_t0 + c (the terminal
             cost under row ref_t0 + T) - the plant row's goals without -
             TOL["f64"] / record_tol("f32");
      the end: z0, U exactly, Z against the oracle's rollout of clip(U)."""
    import oracle as orc
    c = _setup(problem, dtype, form, table, geom, S)
    s = c.s
    tag = (problem, dtype, form, table, plant, geom, S, K)
    plant_t, log_ops = None, None
    if plant:
        par, xg, ug, log_ops = perturbed(problem, B, 11)
        tracked = form != "weights"
        plant_t = s._plant_table(
            "test", torch.from_numpy(par),
            None if tracked else torch.from_numpy(xg),
            None if tracked else torch.from_numpy(ug))
    elif table:
        _, _, _, log_ops = perturbed(problem, B, seed=41)
    else:
        from solver_util import fresh_ops
        log_ops = fresh_ops(problem, B)
    dist_np = 0.01 * np.random.RandomState(3).randn(B, T, s.n)
    dist = to_device(dist_np, dtype)
    dist_np = _np(dist).astype(np.float64)
    out = _trial(c, S, K, plant=plant_t, dist=dist)
    n, m, tol = s.n, s.m, record_tol(dtype)
    bar = TOL["f64"] if dtype == "f64" else record_tol("f32")
    o, d = orc.load(np_dtype(dtype)), np_dtype(dtype)
    X, Ul, Jc = _np(out.X), _np(out.Ulog), _np(out.Jc)
    J0, Jw, plans, seen = _np(out.J0), _np(out.Jw), _np(out.plans), _np(out.Y)
    assert same_bits(out.J0, out.Jc[..., 0]), tag
    took = np.isfinite(Jw) & (Jw <= J0)
    print(tag, "took", took.mean())
    wn = noise_rows(B, T, n, 0, SEED, 40, 2, dtype)
    vn = noise_rows(B, T, n, 1, SEED, 40, 2, dtype)
    L = None if c.xr is None else c.xr.shape[1]
    Jcl = np.zeros(B, d)
    base = c.U
    for step in range(T):
        y = seen[:, step]
        first = 0 if L is None else ref_row(L, c.t0, step)
        if K == 1:
            off = step * B * S
            Uc, _ = model_candidates(base, S, c.std, SMOOTH, SEED, off, dtype,
                                     c.u_min, c.u_max)
            _, J = oracle_rollouts(c.ops, y, Uc, dtype, c.xr, c.ur, first)
            e = model_e(B, N, S, m, SMOOTH, SEED, off, dtype)
            _, Uw = model_update(base, Jc[:, step, 0], c.lam, e, c.std,
                                 c.u_min, c.u_max)
            _, Jp = oracle_rollouts(c.ops, y, plans[:, step][:, None], dtype,
                                    c.xr, c.ur, first)
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
        assert (np.abs(ess - want) <= 64 * S * EPS[dtype] * want).all(), \
            (tag, step, ess, want)
        assert (Ul[:, step] == np.clip(plans[:, step, 0], c.u_min,
                                       c.u_max)).all(), (tag, step)
        xn = np.empty((B, n))
        for b in range(B):
            if L is not None:
                under_row(log_ops[b], c.xr[b], c.ur[b], first)
            xb, ub = X[b, step].astype(d), Ul[b, step].astype(d)
            Jcl[b] += o.cost(log_ops[b], xb, ub)[0]
            xn[b] = o.dynamics(log_ops[b], xb, ub, jac=False)[0]
        xn = xn + dist_np[:, step] + 0.02 * wn[:, step]
        err = rel_err(X[:, step + 1], xn)
        print(tag, step, "x' off by", err)
        assert err < bar, (tag, step, err)
        yn = X[:, step + 1].astype(np.float64) + 0.01 * vn[:, step + 1]
        err = rel_err(seen[:, step + 1], yn)
        print(tag, step, "y' off by", err)
        assert err < bar, (tag, step, err)
        base = shift(plans[:, step])
    assert same_bits(out.x_true, out.X[:, T]), tag
    for b in range(B):
        if L is not None:
            under_row(log_ops[b], c.xr[b], c.ur[b], ref_row(L, c.t0, T))
        Jcl[b] += o.cost(log_ops[b], X[b, T].astype(d), None,
                         terminal=True)[0]
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


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_weights_do_not_move_the_trial_cost(dtype):
    """S = 1 and std = 0: the plan never changes, so the action log is the
    same with and without weights - and so are X and Jcl, bit for bit: the
    trial reports under the SHARED matrices.  The planning costs differ."""
    c = _setup("cartpole", dtype, "both", False, "offset")
    kw = dict(w_std=None, v_std=None)
    a = trial_call(c.s, 1, 2, T, 0.0, 1.0, SMOOTH, SEED, **kw)
    b = trial_call(c.s, 1, 2, T, 0.0, 1.0, SMOOTH, SEED, wts=None, **kw)
    for nm in ("Ulog", "X", "J", "z0", "Z"):
        assert same_bits(getattr(a, nm), getattr(b, nm)), nm
    assert not same_bits(a.J0, b.J0)


# The seed of the candidates, searched on the CPU model
# (sampled_goals_util.chain_model, seeds 0, 1, ...): the first one under which
# every |J_w - J_0| the trial meets exceeds 1e-6 |J_0| on every trajectory and
# some iterations take and some do not.  Seed 0 serves both; the smallest gap
# it meets is 8.29e-3 on the cartpole and 9.53e-4 on the pendulum.
CHAIN_SEED = {"cartpole": 0, "pendulum": 0}


@gpu
@pytest.mark.parametrize("problem", ["cartpole", "pendulum"])
def test_whole_trial_vs_oracle_f64(problem):
    """3 steps, K = 2, S = 5, both noises, a plant table (parameters), the
    offset reference and weights: every log against the numpy / oracle model
    of the whole trial at TOL["f64"].  The temperature is the spread of the
    first iteration's costs under the objective.  The model asserts that
    every |J_w - J_0| it meets exceeds 1e-6 relative (CHAIN_SEED)."""
    from solver_util import make_solver
    K, S, std, seed = 2, 5, 0.3 * BOUND[problem], CHAIN_SEED[problem]
    c = chain_case(problem, B, N, T)
    s, _, _, _, _, _ = make_solver(problem, "f64", B, N)
    s.z0.copy_(torch.from_numpy(c.z0))
    s.U.copy_(torch.from_numpy(c.U))
    set_ref(s, c.xr, c.ur, c.t0)
    set_weights(s, c.q, c.qt, c.r)
    plant = s._plant_table("test", torch.from_numpy(c.par), None, None)
    lam = chain_lam(c, S, std, SMOOTH, seed)
    want = chain_model(c, K, S, std, SMOOTH, seed)
    print(problem, "smallest |J_w - J_0| / |J_0| of the model:", want.gap)
    assert want.gap > 1e-6, want.gap
    out = trial_call(s, S, K, T, std, lam, SMOOTH, seed, plant=plant,
                     dist=torch.from_numpy(c.dist).cuda(), w_std=0.02,
                     v_std=0.01, roll=40, step_offset=2)
    took = _np(torch.isfinite(out.Jw) & (out.Jw <= out.J0))
    assert (took == want.took).all(), (took, want.took)
    assert took.any() and not took.all(), took
    for nm in ("J0", "Jw", "plans", "Ulog", "X", "Y", "J", "z0", "U", "Z",
               "x_true"):
        err = rel_err(_np(getattr(out, nm)), getattr(want, nm))
        print(problem, nm, "off by", err)
        assert err < TOL["f64"], (problem, nm, err)


# ---- GPU, stage 7: the solver ---------------------------------------------------------
def _pair(form, dtype="f64", geom="offset", table=True):
    L, t0 = GEOM[geom]
    return [objective_solver("cartpole", dtype, B, N, form, table, L, t0).s
            for _ in range(2)]


@gpu
def test_solver_trial_vs_composed_host_loop_f64():
    """ILQRSolver.mppi_closed_loop(objective="search", 3 steps, K = 2) with a
    table, the offset reference and weights against the same trial composed
    from what exists: per control step mppi(objective="search", iterations=2,
    adopt=True), pddp_mpc_advance_track_* and set_reference_start(+1) - at
    TOL["f64"].  The method makes ONE pddp_mppi_trial_goals_* call.
    Afterwards ref_start has advanced by the steps, a captured round is
    dropped, the controller words are the re-armed ones and two rounds run."""
    from pddp_amd import _native
    S, K, std, lam = 5, 2, 0.3 * BOUND["cartpole"], 300.0
    s, t = _pair("both")
    par, _, _, _ = perturbed("cartpole", B, 11)
    plant = dict(params=torch.from_numpy(par))
    dist = 0.01 * torch.from_numpy(np.random.RandomState(3).randn(B, T, s.n))
    s.nominal_rollout()
    s.round()  # (a controller state that is not the re-armed one)
    s._graph = object()
    names = []
    real = _native.call

    def wrapped(name, dtype, *args):
        names.append(name)
        return real(name, dtype, *args)
    _native.call = wrapped
    try:
        r = s.mppi_closed_loop(T, S, std, lam, iterations=K, smooth=SMOOTH,
                               seed=9, candidate_offset=4, disturbance=dist,
                               log_costs=True, objective="search", **plant)
    finally:
        _native.call = real
    torch.cuda.synchronize()
    assert names.count("pddp_mppi_trial_goals") == 1, names
    assert "pddp_mppi_trial" not in names, names
    assert s.ref_start == GEOM["offset"][1] + T and s._graph is None
    assert torch.equal(r.took, torch.isfinite(r.J_w) & (r.J_w <= r.J0))
    assert same_bits(r.J0, r.Jc[..., 0])

    logs = trial_logs(t, T, 0.0)
    plant_t = t._plant_table("test", plant["params"], None, None)
    dist_t = dist.to(device="cuda").contiguous()
    t.nominal_rollout()
    for c in range(T):
        t.mppi(S, std, lam, smooth=SMOOTH, seed=9, iterations=K,
               sample_offset=4 + c * K * B * S, objective="search")
        mpc_advance(t, T, c, logs, plant=plant_t, dist=dist_t,
                    ref=t.reference, ref_t0=t.ref_start)
        t.set_reference_start(t.ref_start + 1)
    pairs = (("X", r.X, logs[0]), ("U", r.U, logs[1]), ("J", r.J, logs[2]),
             ("z0", s.z0, t.z0), ("plan", s.U, t.U), ("Z", s.Z, t.Z))
    for nm, a, b in pairs:
        err = rel_err(_np(a), _np(b))
        print(nm, "off the composed loop by", err)
        assert err < TOL["f64"], (nm, err)
    assert s.ref_start == t.ref_start
    for k, v in REARMED.items():
        assert bool((getattr(s, k) == v).all()), k
    assert s._derivs_due
    s.rounds(2)
    assert bool(torch.isfinite(s.J_opt).all()), s.J_opt


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_four_steps_are_two_and_two_continued(dtype):
    """Through the solver, with the reference, weights, obs_std and
    process_std: four steps in one call against 2 + 2 - the second call with
    z0=None, step_offset=2 and candidate_offset advanced by 2 K B S, the
    reference continued by the solver - bit for bit: the states, the
    observations, the actions, every log, and what the solver holds."""
    S, K, std, lam = 5, 2, 0.3 * BOUND["cartpole"], 300.0
    kw = dict(iterations=K, smooth=SMOOTH, seed=9, process_std=0.02,
              obs_std=0.01, sample_offset=11, objective="search")
    a, b = _pair("both", dtype)
    whole = a.mppi_closed_loop(4, S, std, lam, candidate_offset=3, **kw)
    first = b.mppi_closed_loop(2, S, std, lam, candidate_offset=3, **kw)
    assert b.ref_start == GEOM["offset"][1] + 2
    second = b.mppi_closed_loop(2, S, std, lam, z0=None, step_offset=2,
                                candidate_offset=3 + 2 * K * B * S, **kw)
    assert a.ref_start == b.ref_start == GEOM["offset"][1] + 4
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
def test_noise_is_mpc_closed_loops_under_the_reference():
    """f64, process noise alone, a reference: X[:, c + 1] - f(X[:, c],
    U[:, c]) is process_std times the normals closed_loop_draws(1, "process",
    seed, sample_offset, steps=) returns at rows step_offset + c, and an
    mpc_closed_loop trial with the same three values under the same reference
    steps under the same ones."""
    import oracle as orc
    from solver_util import fresh_ops
    a, b = _pair("ref", table=False)
    kw = dict(seed=13, process_std=0.05, sample_offset=7, step_offset=2)
    r = a.mppi_closed_loop(T, 5, 0.3 * BOUND["cartpole"], 300.0,
                           objective="search", **kw)
    q = b.mpc_closed_loop(T, 2, **kw)
    assert a.ref_start == b.ref_start == GEOM["offset"][1] + T
    W = _np(a.closed_loop_draws(1, "process", 13, 7, steps=T + 2)[:, :, 0])
    o, ops = orc.load(np.float64), fresh_ops("cartpole", B)
    for out in (r, q):
        X, U = _np(out.X), _np(out.U)
        for c in range(T):
            for i in range(B):
                xn = o.dynamics(ops[i], X[i, c], U[i, c], jac=False)[0]
                err = np.abs(X[i, c + 1] - xn - 0.05 * W[i, 2 + c]).max()
                assert err < TOL["f64"] * np.abs(X).max(), (c, i, err)


@gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_solver_shoot_shares_the_line_searchs_objective(dtype):
    """With a table, a reference and weights set, shoot(adopt=True,
    objective="search"): J_best <= J[:, 0]; nominal_rollout() reproduces Z
    within record_tol; and the cost the next round's records report for the
    nominal (pddp_derivs_track_weighted_*'s J) equals J_best within
    record_tol - the planner and the line search share one objective.
    Against the entry point called directly: the same bits."""
    (s,) = _pair("both", dtype)[:1]
    std = 0.3 * BOUND["cartpole"]
    direct = shoot_call(s, 70, std, SMOOTH, 5, offset=3)
    out = s.shoot(70, std, smooth=SMOOTH, seed=5, sample_offset=3,
                  objective="search")
    for nm in ("J", "best", "J_best"):
        assert same_bits(getattr(out, nm), getattr(direct, nm)), nm
    assert same_bits(s.U, direct.U) and same_bits(s.Z, direct.Z)
    assert bool((out.best > 0).any()) and bool((out.J_best <= out.J[:, 0]).all())
    for k, v in REARMED.items():
        assert bool((getattr(s, k) == v).all()), k
    Z = s.Z.clone()
    s.nominal_rollout()
    tol = record_tol(dtype)
    assert rel_err(_np(s.Z), _np(Z)) < tol
    s.derivs(set_state=False)
    e = np.abs(_np(s.J_opt) - _np(out.J_best)) / np.abs(_np(out.J_best))
    print(dtype, "the records' J off J_best by", e)
    assert (e < tol).all(), e


@gpu
def test_solver_mppi_iterations_and_nothing_set():
    """mppi(iterations=3, objective="search") is three single calls with
    sample_offset advanced by B S, bit for bit, J_trace non-increasing;
    objective="search" with nothing set returns the bits of the plain call,
    in all three methods, through the siblings' entry points."""
    from mppi_util import wide_solver
    from pddp_amd import _native
    S, std, lam = 5, 0.3 * BOUND["cartpole"], 300.0
    a, b = _pair("both")
    a.nominal_rollout()
    b.nominal_rollout()
    three = a.mppi(S, std, lam, smooth=SMOOTH, seed=9, sample_offset=4,
                   iterations=3, objective="search")
    Jt = _np(three.J_trace)
    assert (Jt[1:] <= Jt[:-1]).all(), Jt
    trace = [three.J_trace[0]]
    for k in range(3):
        one = b.mppi(S, std, lam, smooth=SMOOTH, seed=9,
                     sample_offset=4 + k * B * S, objective="search")
        trace.append(torch.where(one.improved, one.J_w, trace[-1]))
    assert torch.equal(three.J_trace, torch.stack(trace))
    for nm in ("J", "W", "J_w", "best", "improved", "ess"):
        assert same_bits(getattr(one, nm), getattr(three, nm)), nm
    assert same_bits(a.U, b.U) and same_bits(a.Z, b.Z)

    names = []
    real = _native.call

    def wrapped(name, dtype, *args):
        names.append(name)
        return real(name, dtype, *args)
    _native.call = wrapped
    try:
        outs = []
        for objective in ("shared", "search"):
            p, _, _, _, _, _ = wide_solver("cartpole", "f64", B, N)
            outs.append((
                p.shoot(S, std, seed=3, adopt=False, objective=objective),
                p.mppi(S, std, lam, seed=3, adopt=False, objective=objective),
                p.mppi_closed_loop(T, S, std, lam, seed=3,
                                   objective=objective)))
    finally:
        _native.call = real
    assert not [x for x in names if "track" in x or "weighted" in x or
                "goals" in x], names
    for x, y in zip(*outs):
        for nm, v in vars(x).items():
            if torch.is_tensor(v):
                assert same_bits(v, getattr(y, nm)), nm


@gpu
def test_solver_objective_refusals():
    """objective="shared" still raises in the words the siblings' tests match,
    and names objective="search"; another value is refused; x_goal / u_goal
    with a reference in the trial are refused - all before any launch."""
    from pddp_amd import _native
    (s,) = _pair("both")[:1]
    calls = []
    real = _native.call
    _native.call = lambda *a: calls.append(a[0]) or real(*a)
    bad = pytest.raises
    try:
        for fn, args in ((s.shoot, (5, 1.0)), (s.mppi, (5, 1.0, 1.0)),
                         (s.mppi_closed_loop, (2, 5, 1.0, 1.0))):
            with bad(_native.NativeError, match="reference") as e:
                fn(*args)
            assert 'objective="search"' in str(e.value)
            with bad(_native.NativeError, match="objective"):
                fn(*args, objective="line search")
            with bad(_native.NativeError, match="objective"):
                fn(*args, objective=None)
        na = s.problem.aug_size
        with bad(_native.NativeError, match="x_goal"):
            s.mppi_closed_loop(2, 5, 1.0, 1.0, objective="search",
                               x_goal=torch.zeros(B, na))
        with bad(_native.NativeError, match="u_goal"):
            s.mppi_closed_loop(2, 5, 1.0, 1.0, objective="search",
                               u_goal=torch.zeros(B, s.m))
        s.clear_reference()
        for fn, args in ((s.shoot, (5, 1.0)), (s.mppi, (5, 1.0, 1.0)),
                         (s.mppi_closed_loop, (2, 5, 1.0, 1.0))):
            with bad(_native.NativeError, match="weights") as e:
                fn(*args)
            assert 'objective="search"' in str(e.value)
    finally:
        _native.call = real
    assert not calls, calls
