"""The launch sequence of a solver round, recorded call by call.

`ILQRSolver._plan()` picks one of five sequences (the table in
pddp_amd/controllers/solver.py).  A recorder around the C ABI
(`_native.call`, `_native.call_rc` and the entry points the solver reaches
through `_native.lib()` itself, DIRECT) logs, for every call a case makes
after `set_nominal`, the entry point with its dtype suffix and the positions
of its NULL arguments; the real call goes through.  Runs of one entry are
written "count*entry".

EXPECTED is what this recorder logged, together with the solver's flags at the
end of each case, on commit e505e79 ("GP step kernels: chunked form for
training sets beyond one LDS"), the last one whose `round()` decided its
launches condition by condition: a change of solver.py that makes other calls,
in another order, or leaves other flags fails here.  (alphas17: pddp_accept
takes 16 step sizes at most, so on that commit the nominal+separate fall-back
ends in a NativeError after its launches; the record holds that too.)  The
cases with a table, a reference or weights and those of `closed_loop`,
`closed_loop_draws` and `mpc_closed_loop` (EXPECTED's second block, with
`ref_start` among the flags) were recorded on commit f5d44c3 ("Batched solver:
per-trajectory diagonals of Q, Q_term and R"), the last one whose setters and
trials each carried their own copy of the host-side plumbing."""
import ctypes

import numpy as np
import pytest
import torch

from pddp_amd import _native
from golden_util import DT
from solver_util import BOUND, MEAN0

pytestmark = pytest.mark.gpu

B, N = 32, 20
S, L_REF = 3, 8  # rollouts per trajectory, rows of a reference (< N: held)
DIRECT = ("pddp_round_nominal_f32", "pddp_attach_events",
          "pddp_search_candidates", "pddp_event_record",
          "pddp_mpc_advance_f32", "pddp_mpc_advance_f64",
          "pddp_mpc_advance_track_f32", "pddp_mpc_advance_track_f64")
FLAGS = ("_one_launch", "_nominal_sweep", "_fused", "_derivs_due",
         "_rec_stale", "candidates_kept", "last_search_timed", "ref_start")


class Recorder(object):

    def __init__(self, monkeypatch):
        self.log = []
        lib = _native.lib()
        for wrapper in ("call", "call_rc"):
            monkeypatch.setattr(_native, wrapper,
                                self._typed(getattr(_native, wrapper)))
        for name in DIRECT:
            monkeypatch.setattr(lib, name, self._direct(name,
                                                        getattr(lib, name)))

    def _note(self, name, args):
        null = [str(i) for i, a in enumerate(args) if a is None or (
            isinstance(a, ctypes.c_void_p) and not a.value)]
        entry = name + (":" + ",".join(null) if null else "")
        if self.log and self.log[-1][1] == entry:
            self.log[-1][0] += 1
        else:
            self.log.append([1, entry])

    def _typed(self, real):
        def wrapped(name, dtype, *args):
            self._note("%s_%s" % (name, _native.suffix(dtype)), args)
            return real(name, dtype, *args)
        return wrapped

    def _direct(self, name, real):
        def wrapped(*args):
            self._note(name, args)
            return real(*args)
        return wrapped

    def entries(self):
        return [e if c == 1 else "%d*%s" % (c, e) for c, e in self.log]


def _solver(problem="cartpole", dtype=torch.float32, bounded=True, branch=0,
            alphas=None):
    import pddp_amd
    from pddp_amd.controllers.solver import ILQRSolver
    from pddp_amd.utils.encoding import StateEncoding
    mod = getattr(pddp_amd.examples, problem)
    model = [getattr(mod, k) for k in dir(mod) if
             k.endswith("DynamicsModel") and k != "DynamicsModel"][0]
    cost = [getattr(mod, k) for k in dir(mod)
            if k.endswith("Cost") and k != "AugmentedQRCost"][0]
    prob = model(DT[problem]).native_problem(
        StateEncoding.IGNORE_UNCERTAINTY, cost())
    rng = np.random.RandomState(1)
    n, m = prob.encoded_size, prob.action_size
    z0 = np.asarray(MEAN0[problem], np.float64) + 1e-2 * rng.randn(B, n)
    U = 0.1 * rng.randn(B, N, m)
    bound = torch.full((m,), BOUND[problem], dtype=dtype)
    s = ILQRSolver(prob, B, N, dtype, "cuda", -bound if bounded else None,
                   bound if bounded else None, alphas=alphas, branch=branch)
    s._keep = prob
    return s, torch.from_numpy(z0).to(dtype).cuda(), \
        torch.from_numpy(U).to(dtype).cuda()


def _gp_solver():
    """The GP plugin solver of test_gp's hipGraph test."""
    from pddp_amd import GaussianVariable, StateEncoding
    from pddp_amd.controllers.ilqr import fit_alphas
    from pddp_amd.controllers.plugin import TorchProblem
    from pddp_amd.controllers.solver import ILQRSolver
    from pddp_amd.examples.cartpole import CartpoleCost, CartpoleDynamicsModel
    from pddp_amd.models.gp import gp_dynamics_model_factory
    CM = CartpoleDynamicsModel
    g = torch.Generator().manual_seed(3)
    X = torch.cat([torch.randn(40, 2, generator=g),
                   3.0 + 0.8 * torch.randn(40, 1, generator=g),
                   torch.randn(40, 1, generator=g)], -1)
    U = 3.0 * torch.randn(40, 1, generator=g)
    with torch.no_grad():
        dX = CM(0.1)(X, U, 0, StateEncoding.IGNORE_UNCERTAINTY) - X
    model = gp_dynamics_model_factory(4, 1, CM.angular_indices,
                                      CM.non_angular_indices)().cuda()
    model.fit(X.cuda(), U.cuda(), dX.cuda())
    model.eval()
    enc = StateEncoding.DEFAULT
    Bg, Ng = 8, 10
    z0 = torch.stack([GaussianVariable(
        torch.tensor([0.0, 0.0, 3.0, 0.0]) + 0.05 * torch.randn(4, generator=g),
        var=1e-2 * torch.ones(4)).encode(enc) for _ in range(Bg)]).cuda()
    U0 = (0.3 * torch.randn(Bg, Ng, 1, generator=g)).cuda()
    plugin = TorchProblem(model, CartpoleCost().cuda(), enc, {}, {})
    s = ILQRSolver(None, Bg, Ng, torch.float32, "cuda", torch.tensor([-10.0]),
                   torch.tensor([10.0]), fit_alphas(torch.float32, "cuda"),
                   plugin=plugin, n=14, m=1)
    return s, z0, U0


def _pair():
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    _native.lib().pddp_event_create(ctypes.byref(a))
    _native.lib().pddp_event_create(ctypes.byref(b))
    return a, b


def _three_rounds(s, **kw):
    for _ in range(3):
        s.round(**kw)


def _capture_and_replay(s):
    s.capture_round()
    s.replay_round(True)
    s.replay_round(True)


def _force(flag):
    def run(s):
        setattr(s, flag, False)
        _three_rounds(s)
    return run


def _params(s, *lead):
    """[*lead][P] model parameters: the shared ones, each scaled by up to 5 %."""
    P = s._PARAM_COUNT[s.problem.model]
    g = torch.Generator().manual_seed(5)
    base = torch.tensor(list(s.problem.params)[:P], dtype=torch.float64)
    scale = 1 + 0.05 * torch.rand(*lead, P, generator=g, dtype=torch.float64)
    return (base * scale).to(s.dtype)


def _x_ref(s):
    """[B][L_REF][na] goals: the shared goal, moved a little in every row."""
    na = s.problem.aug_size
    g = torch.Generator().manual_seed(6)
    goal = torch.tensor(list(s.problem.x_goal)[:na], dtype=torch.float64)
    return (goal + 0.05 * torch.randn(B, L_REF, na, generator=g,
                                      dtype=torch.float64)).to(s.dtype)


def _q(s):
    """[B][na] diagonals of Q: the shared one, each entry raised by up to 10 %
    (the matrix stays positive semi-definite)."""
    na = s.problem.aug_size
    g = torch.Generator().manual_seed(7)
    diag = torch.tensor([s.problem.Q[i * _native.MAX_AUG + i]
                         for i in range(na)], dtype=torch.float64)
    return (diag * (1 + 0.1 * torch.rand(B, na, generator=g,
                                         dtype=torch.float64))).to(s.dtype)


def _table(s):
    s.set_batch_problem(params=_params(s, B))


def _reference(s, start=0):
    s.set_reference(_x_ref(s), start=start)


def _weights(s):
    s.set_batch_weights(q=_q(s))


def _after(*setters, then=_three_rounds):
    def run(s):
        for setter in setters:
            setter(s)
        then(s)
    return run


def _reference_moved(s):
    _reference(s)
    _three_rounds(s)
    s.set_reference_start(3)
    s.round()


def _weights_cleared(s):
    _weights(s)
    s.round()
    s.clear_batch_weights()
    _three_rounds(s)


def _cleared_in_turn(s):
    from pddp_amd.controllers.solver import RECORDS_SEPARATE
    _table(s)
    _reference(s)
    s.clear_reference()
    assert s._plan(s.kernel_variant) == RECORDS_SEPARATE
    s.round()
    s.clear_batch_problem()
    assert s._plan(s.kernel_variant) != RECORDS_SEPARATE
    s.round()


def _mpc_track(s):
    _reference(s, start=1)
    s.mpc_closed_loop(steps=2, rounds_per_step=2)
    assert s.ref_start == 1 + 2


# case -> (arguments of _solver, or None for the GP plugin; what it runs)
CASES = {}
for _bounded in (True, False):
    for _branch in (0, 1):
        _kw = dict(bounded=_bounded, branch=_branch)
        _id = "%s-%s" % ("bounded" if _bounded else "unbounded",
                         "chol" if _branch else "eig")
        CASES["default-" + _id] = (_kw, _three_rounds)
        for _flag in ("_one_launch", "_nominal_sweep", "_fused"):
            CASES["%s_off-%s" % (_flag, _id)] = (_kw, _force(_flag))
CASES.update({
    "cartpole-f64": (dict(dtype=torch.float64), _three_rounds),
    "pendulum-f32": (dict(problem="pendulum"), _three_rounds),
    "pendulum-f64": (dict(problem="pendulum", dtype=torch.float64),
                     _three_rounds),
    "double_cartpole-f32": (dict(problem="double_cartpole"), _three_rounds),
    "alphas17": (dict(alphas=torch.linspace(1.0, 0.01, 17)), _three_rounds),
    "exact_variant": (dict(), lambda s: (
        setattr(s, "kernel_variant", s.exact_variant()), _three_rounds(s))),
    "rounds4": (dict(), lambda s: s.rounds(4)),
    "fit_rounds_per_launch8": (dict(), lambda s: s.fit(
        n_iterations=3, rounds_per_launch=8)),
    "search_events": (dict(), lambda s: _three_rounds(
        s, search_events=_pair())),
    "backward_events": (dict(), lambda s: _three_rounds(
        s, backward_events=_pair())),
    "capture_replay": (dict(), _capture_and_replay),
    "gp-round": (None, _three_rounds),
    "gp-capture_replay": (None, _capture_and_replay),
})
# per-trajectory data and the trials on a plant (EXPECTED's second block)
CASES.update({
    "table": (dict(), _after(_table)),
    "table-f64": (dict(dtype=torch.float64), _after(_table)),
    "reference": (dict(), _reference_moved),
    "table+reference": (dict(), _after(_table, _reference)),
    "weights": (dict(), _after(_weights)),
    "table+weights": (dict(), _after(_table, _weights)),
    "weights-cleared": (dict(), _weights_cleared),
    "table+reference-cleared-in-turn": (dict(), _cleared_in_turn),
    "table-capture_replay": (dict(), _after(_table,
                                            then=_capture_and_replay)),
    "closed_loop": (dict(), lambda s: s.closed_loop(samples=S)),
    "closed_loop-plant": (dict(), lambda s: s.closed_loop(
        samples=S, params=_params(s, B, S))),
    "closed_loop-noisy": (dict(), lambda s: s.closed_loop(
        samples=S, process_std=0.01, obs_std=None)),
    "closed_loop-track": (dict(), _after(_reference, then=lambda s: (
        s.closed_loop(samples=S, track=True, process_std=None,
                      obs_std=None)))),
    "closed_loop-track-noisy": (dict(), _after(_reference, then=lambda s: (
        s.closed_loop(samples=S, track=True, process_std=0.01,
                      obs_std=0.02)))),
    "closed_loop_draws": (dict(), lambda s: s.closed_loop_draws(S)),
    "mpc": (dict(), lambda s: s.mpc_closed_loop(
        steps=2, rounds_per_step=2, events=_pair())),
    "mpc-plant": (dict(), lambda s: s.mpc_closed_loop(
        steps=2, rounds_per_step=2, params=_params(s, B))),
    "mpc-track": (dict(), _mpc_track),
})


def record(case, monkeypatch):
    """(log, flags) of one case."""
    kw, run = CASES[case]
    s, z0, U = _gp_solver() if kw is None else _solver(**kw)
    s.set_nominal(z0, U)
    rec = Recorder(monkeypatch)
    try:
        run(s)
    except _native.NativeError as e:
        # (alphas17: pddp_accept takes 16 step sizes at most, so the
        # nominal+separate fall-back ends in this error - part of the record)
        rec.log.append([1, "NativeError: %s" % e])
    torch.cuda.synchronize()
    monkeypatch.undo()
    return rec.entries(), tuple(getattr(s, f, None) for f in FLAGS)


EXPECTED = {'_fused_off-bounded-chol': (['pddp_derivs_f32',
                              'pddp_riccati_backward_variant_f32',
                              'pddp_line_search_f32',
                              'pddp_accept_f32',
                              'pddp_derivs_f32',
                              'pddp_riccati_backward_variant_f32',
                              'pddp_line_search_f32',
                              'pddp_accept_f32',
                              'pddp_derivs_f32',
                              'pddp_riccati_backward_variant_f32',
                              'pddp_line_search_f32',
                              'pddp_accept_f32'],
                             (None, None, False, False, False, True, None)),
 '_fused_off-bounded-eig': (['pddp_derivs_f32',
                             'pddp_riccati_backward_variant_f32',
                             'pddp_line_search_f32',
                             'pddp_accept_f32',
                             'pddp_derivs_f32',
                             'pddp_riccati_backward_variant_f32',
                             'pddp_line_search_f32',
                             'pddp_accept_f32',
                             'pddp_derivs_f32',
                             'pddp_riccati_backward_variant_f32',
                             'pddp_line_search_f32',
                             'pddp_accept_f32'],
                            (None, None, False, False, False, True, None)),
 '_fused_off-unbounded-chol': (['pddp_derivs_f32:5,6',
                                'pddp_riccati_backward_variant_f32:5,6',
                                'pddp_line_search_f32:8,9',
                                'pddp_accept_f32',
                                'pddp_derivs_f32:5,6',
                                'pddp_riccati_backward_variant_f32:5,6',
                                'pddp_line_search_f32:8,9',
                                'pddp_accept_f32',
                                'pddp_derivs_f32:5,6',
                                'pddp_riccati_backward_variant_f32:5,6',
                                'pddp_line_search_f32:8,9',
                                'pddp_accept_f32'],
                               (None, None, False, False, False, True, None)),
 '_fused_off-unbounded-eig': (['pddp_derivs_f32:5,6',
                               'pddp_riccati_backward_variant_f32:5,6',
                               'pddp_line_search_f32:8,9',
                               'pddp_accept_f32',
                               'pddp_derivs_f32:5,6',
                               'pddp_riccati_backward_variant_f32:5,6',
                               'pddp_line_search_f32:8,9',
                               'pddp_accept_f32',
                               'pddp_derivs_f32:5,6',
                               'pddp_riccati_backward_variant_f32:5,6',
                               'pddp_line_search_f32:8,9',
                               'pddp_accept_f32'],
                              (None, None, False, False, False, True, None)),
 '_nominal_sweep_off-bounded-chol': (['pddp_derivs_f32',
                                      'pddp_riccati_backward_variant_f32',
                                      'pddp_search_accept_f32',
                                      'pddp_search_candidates',
                                      'pddp_riccati_backward_variant_f32',
                                      'pddp_search_accept_f32',
                                      'pddp_search_candidates',
                                      'pddp_riccati_backward_variant_f32',
                                      'pddp_search_accept_f32',
                                      'pddp_search_candidates'],
                                     (None,
                                      False,
                                      True,
                                      False,
                                      False,
                                      True,
                                      None)),
 '_nominal_sweep_off-bounded-eig': (['pddp_derivs_f32',
                                     'pddp_riccati_backward_variant_f32',
                                     'pddp_search_accept_f32',
                                     'pddp_search_candidates',
                                     'pddp_riccati_backward_variant_f32',
                                     'pddp_search_accept_f32',
                                     'pddp_search_candidates',
                                     'pddp_riccati_backward_variant_f32',
                                     'pddp_search_accept_f32',
                                     'pddp_search_candidates'],
                                    (None,
                                     False,
                                     True,
                                     False,
                                     False,
                                     True,
                                     None)),
 '_nominal_sweep_off-unbounded-chol': (['pddp_derivs_f32:5,6',
                                        'pddp_riccati_backward_variant_f32:5,6',
                                        'pddp_search_accept_f32:8,9',
                                        'pddp_search_candidates',
                                        'pddp_riccati_backward_variant_f32:5,6',
                                        'pddp_search_accept_f32:8,9',
                                        'pddp_search_candidates',
                                        'pddp_riccati_backward_variant_f32:5,6',
                                        'pddp_search_accept_f32:8,9',
                                        'pddp_search_candidates'],
                                       (None,
                                        False,
                                        True,
                                        False,
                                        False,
                                        True,
                                        None)),
 '_nominal_sweep_off-unbounded-eig': (['pddp_derivs_f32:5,6',
                                       'pddp_riccati_backward_variant_f32:5,6',
                                       'pddp_search_accept_f32:8,9',
                                       'pddp_search_candidates',
                                       'pddp_riccati_backward_variant_f32:5,6',
                                       'pddp_search_accept_f32:8,9',
                                       'pddp_search_candidates',
                                       'pddp_riccati_backward_variant_f32:5,6',
                                       'pddp_search_accept_f32:8,9',
                                       'pddp_search_candidates'],
                                      (None,
                                       False,
                                       True,
                                       False,
                                       False,
                                       True,
                                       None)),
 '_one_launch_off-bounded-chol': (['pddp_sweep_nominal_f32',
                                   'pddp_search_accept_f32:27',
                                   'pddp_search_candidates',
                                   'pddp_sweep_nominal_f32',
                                   'pddp_search_accept_f32:27',
                                   'pddp_search_candidates',
                                   'pddp_sweep_nominal_f32',
                                   'pddp_search_accept_f32:27',
                                   'pddp_search_candidates'],
                                  (False,
                                   True,
                                   True,
                                   False,
                                   True,
                                   True,
                                   None)),
 '_one_launch_off-bounded-eig': (['pddp_sweep_nominal_f32',
                                  'pddp_search_accept_f32:27',
                                  'pddp_search_candidates',
                                  'pddp_sweep_nominal_f32',
                                  'pddp_search_accept_f32:27',
                                  'pddp_search_candidates',
                                  'pddp_sweep_nominal_f32',
                                  'pddp_search_accept_f32:27',
                                  'pddp_search_candidates'],
                                 (False, True, True, False, True, True, None)),
 '_one_launch_off-unbounded-chol': (['pddp_sweep_nominal_f32:5,6',
                                     'pddp_search_accept_f32:8,9,27',
                                     'pddp_search_candidates',
                                     'pddp_sweep_nominal_f32:5,6',
                                     'pddp_search_accept_f32:8,9,27',
                                     'pddp_search_candidates',
                                     'pddp_sweep_nominal_f32:5,6',
                                     'pddp_search_accept_f32:8,9,27',
                                     'pddp_search_candidates'],
                                    (False,
                                     True,
                                     True,
                                     False,
                                     True,
                                     True,
                                     None)),
 '_one_launch_off-unbounded-eig': (['pddp_sweep_nominal_f32:5,6',
                                    'pddp_search_accept_f32:8,9,27',
                                    'pddp_search_candidates',
                                    'pddp_sweep_nominal_f32:5,6',
                                    'pddp_search_accept_f32:8,9,27',
                                    'pddp_search_candidates',
                                    'pddp_sweep_nominal_f32:5,6',
                                    'pddp_search_accept_f32:8,9,27',
                                    'pddp_search_candidates'],
                                   (False,
                                    True,
                                    True,
                                    False,
                                    True,
                                    True,
                                    None)),
 'alphas17': (['pddp_round_nominal_f32:30',
               'pddp_sweep_nominal_f32',
               'pddp_search_accept_f32:27',
               'pddp_line_search_f32',
               'pddp_accept_f32',
               'NativeError: pddp_accept failed with code -2'],
              (False, False, False, False, True, True, None)),
 'backward_events': (['pddp_attach_events',
                      'pddp_round_nominal_f32:30',
                      'pddp_attach_events',
                      'pddp_round_nominal_f32:30',
                      'pddp_attach_events',
                      'pddp_round_nominal_f32:30'],
                     (True, True, True, False, True, True, None)),
 'capture_replay': (['pddp_round_nominal_f32:30'],
                    (True, True, True, False, True, True, None)),
 'cartpole-f64': (['pddp_sweep_nominal_f64',
                   'pddp_search_accept_f64:27',
                   'pddp_search_candidates',
                   'pddp_sweep_nominal_f64',
                   'pddp_search_accept_f64:27',
                   'pddp_search_candidates',
                   'pddp_sweep_nominal_f64',
                   'pddp_search_accept_f64:27',
                   'pddp_search_candidates'],
                  (False, True, True, False, True, True, None)),
 'default-bounded-chol': (['3*pddp_round_nominal_f32:30'],
                          (True, True, True, False, True, True, None)),
 'default-bounded-eig': (['3*pddp_round_nominal_f32:30'],
                         (True, True, True, False, True, True, None)),
 'default-unbounded-chol': (['3*pddp_round_nominal_f32:7,8,30'],
                            (True, True, True, False, True, True, None)),
 'default-unbounded-eig': (['3*pddp_round_nominal_f32:7,8,30'],
                           (True, True, True, False, True, True, None)),
 'double_cartpole-f32': (['pddp_derivs_f32',
                          'pddp_riccati_backward_variant_f32',
                          'pddp_search_accept_f32',
                          'pddp_search_candidates',
                          'pddp_riccati_backward_variant_f32',
                          'pddp_search_accept_f32',
                          'pddp_search_candidates',
                          'pddp_riccati_backward_variant_f32',
                          'pddp_search_accept_f32',
                          'pddp_search_candidates'],
                         (None, False, True, False, False, True, None)),
 'exact_variant': (['pddp_derivs_f32',
                    'pddp_riccati_backward_variant_f32',
                    'pddp_search_accept_f32',
                    'pddp_search_candidates',
                    'pddp_riccati_backward_variant_f32',
                    'pddp_search_accept_f32',
                    'pddp_search_candidates',
                    'pddp_riccati_backward_variant_f32',
                    'pddp_search_accept_f32',
                    'pddp_search_candidates'],
                   (None, None, True, False, False, True, None)),
 'fit_rounds_per_launch8': (['2*pddp_round_nominal_f32:30'],
                            (True, True, True, False, True, True, None)),
 'gp-capture_replay': (['pddp_gp_step_masked_f32',
                        'pddp_qr_cost_derivs_f32',
                        'pddp_pack_records_f32',
                        'pddp_sum_stage_costs_f32',
                        'pddp_riccati_backward_variant_f32',
                        'pddp_gp_rollout_f32',
                        'pddp_accept_f32',
                        'pddp_gp_step_masked_f32',
                        'pddp_qr_cost_derivs_f32',
                        'pddp_pack_records_f32',
                        'pddp_sum_stage_costs_f32',
                        'pddp_riccati_backward_variant_f32',
                        'pddp_gp_rollout_f32',
                        'pddp_accept_f32',
                        'pddp_riccati_backward_variant_f32',
                        'pddp_gp_rollout_f32',
                        'pddp_accept_f32'],
                       (None, False, None, True, False, True, None)),
 'gp-round': (['pddp_gp_step_masked_f32',
               'pddp_qr_cost_derivs_f32',
               'pddp_pack_records_f32',
               'pddp_sum_stage_costs_f32',
               'pddp_riccati_backward_variant_f32',
               'pddp_gp_rollout_f32',
               'pddp_accept_f32',
               'pddp_gp_step_masked_f32',
               'pddp_qr_cost_derivs_f32',
               'pddp_pack_records_f32',
               'pddp_sum_stage_costs_f32',
               'pddp_riccati_backward_variant_f32',
               'pddp_gp_rollout_f32',
               'pddp_accept_f32',
               'pddp_gp_step_masked_f32',
               'pddp_qr_cost_derivs_f32',
               'pddp_pack_records_f32',
               'pddp_sum_stage_costs_f32',
               'pddp_riccati_backward_variant_f32',
               'pddp_gp_rollout_f32',
               'pddp_accept_f32'],
              (None, False, None, False, False, True, None)),
 'pendulum-f32': (['pddp_round_nominal_f32:30',
                   'pddp_sweep_nominal_f32',
                   'pddp_search_accept_f32:27',
                   'pddp_search_candidates',
                   'pddp_sweep_nominal_f32',
                   'pddp_search_accept_f32:27',
                   'pddp_search_candidates',
                   'pddp_sweep_nominal_f32',
                   'pddp_search_accept_f32:27',
                   'pddp_search_candidates'],
                  (False, True, True, False, True, True, None)),
 'pendulum-f64': (['pddp_derivs_f64',
                   'pddp_riccati_backward_variant_f64',
                   'pddp_search_accept_f64',
                   'pddp_search_candidates',
                   'pddp_riccati_backward_variant_f64',
                   'pddp_search_accept_f64',
                   'pddp_search_candidates',
                   'pddp_riccati_backward_variant_f64',
                   'pddp_search_accept_f64',
                   'pddp_search_candidates'],
                  (None, False, True, False, False, True, None)),
 'rounds4': (['pddp_round_nominal_f32:30'],
             (True, True, True, False, True, True, None)),
 'search_events': (['pddp_sweep_nominal_f32',
                    'pddp_attach_events',
                    'pddp_search_accept_f32:27',
                    'pddp_search_candidates',
                    'pddp_sweep_nominal_f32',
                    'pddp_attach_events',
                    'pddp_search_accept_f32:27',
                    'pddp_search_candidates',
                    'pddp_sweep_nominal_f32',
                    'pddp_attach_events',
                    'pddp_search_accept_f32:27',
                    'pddp_search_candidates'],
                   (None, True, True, False, True, True, 'search_accept'))}

# the second block (module docstring): `ref_start` is the last flag
EXPECTED.update(
{'closed_loop': (['pddp_closed_loop_f32:7,8,11,12,13'],
                 (None, None, None, True, False, True, None, 0)),
 'closed_loop-noisy': (['pddp_closed_loop_noisy_f32:7,8,12,15,16,17'],
                       (None, None, None, True, False, True, None, 0)),
 'closed_loop-plant': (['pddp_closed_loop_f32:7,11,12,13'],
                       (None, None, None, True, False, True, None, 0)),
 'closed_loop-track': (['pddp_closed_loop_track_f32:10,11,14,15,18,19,20'],
                       (False, False, False, True, True, True, None, 0)),
 'closed_loop-track-noisy': (['pddp_closed_loop_track_f32:10,11,18,19,20'],
                             (False, False, False, True, True, True, None, 0)),
 'closed_loop_draws': (['pddp_closed_loop_draws_f32'],
                       (None, None, None, True, False, True, None, 0)),
 'mpc': (['pddp_event_record',
          'pddp_nominal_rollout_f32:7',
          'pddp_round_nominal_f32:30',
          'pddp_mpc_advance_f32:1,11,12,13',
          'pddp_round_nominal_f32:30',
          'pddp_mpc_advance_f32:1,11,12,13',
          'pddp_event_record'],
         (True, True, True, True, True, True, None, 0)),
 'mpc-plant': (['pddp_nominal_rollout_f32:7',
                'pddp_round_nominal_f32:30',
                'pddp_mpc_advance_f32:1,12,13',
                'pddp_round_nominal_f32:30',
                'pddp_mpc_advance_f32:1,12,13'],
               (True, True, True, True, True, True, None, 0)),
 'mpc-track': (['pddp_nominal_rollout_f32:7',
                'pddp_derivs_track_f32:1,11,15',
                'pddp_derivs_track_f32:1',
                'pddp_riccati_backward_variant_f32',
                'pddp_line_search_track_f32:1',
                'pddp_accept_f32',
                'pddp_derivs_track_f32:1',
                'pddp_riccati_backward_variant_f32',
                'pddp_line_search_track_f32:1',
                'pddp_accept_f32',
                'pddp_mpc_advance_track_f32:1,14,15,16',
                'pddp_derivs_track_f32:1',
                'pddp_riccati_backward_variant_f32',
                'pddp_line_search_track_f32:1',
                'pddp_accept_f32',
                'pddp_derivs_track_f32:1',
                'pddp_riccati_backward_variant_f32',
                'pddp_line_search_track_f32:1',
                'pddp_accept_f32',
                'pddp_mpc_advance_track_f32:1,14,15,16'],
               (False, False, False, True, False, True, None, 3)),
 'reference': (['pddp_derivs_track_f32:1,11,15',
                'pddp_derivs_track_f32:1',
                'pddp_riccati_backward_variant_f32',
                'pddp_line_search_track_f32:1',
                'pddp_accept_f32',
                'pddp_derivs_track_f32:1',
                'pddp_riccati_backward_variant_f32',
                'pddp_line_search_track_f32:1',
                'pddp_accept_f32',
                'pddp_derivs_track_f32:1',
                'pddp_riccati_backward_variant_f32',
                'pddp_line_search_track_f32:1',
                'pddp_accept_f32',
                'pddp_derivs_track_f32:1,11,15',
                'pddp_derivs_track_f32:1',
                'pddp_riccati_backward_variant_f32',
                'pddp_line_search_track_f32:1',
                'pddp_accept_f32'],
               (False, False, False, False, False, True, None, 3)),
 'table': (['pddp_derivs_batch_f32:8,12',
            'pddp_derivs_batch_f32',
            'pddp_riccati_backward_variant_f32',
            'pddp_line_search_batch_f32',
            'pddp_accept_f32',
            'pddp_derivs_batch_f32',
            'pddp_riccati_backward_variant_f32',
            'pddp_line_search_batch_f32',
            'pddp_accept_f32',
            'pddp_derivs_batch_f32',
            'pddp_riccati_backward_variant_f32',
            'pddp_line_search_batch_f32',
            'pddp_accept_f32'],
           (False, False, False, False, False, True, None, 0)),
 'table+reference': (['pddp_derivs_track_f32:11,15',
                      'pddp_derivs_track_f32',
                      'pddp_riccati_backward_variant_f32',
                      'pddp_line_search_track_f32',
                      'pddp_accept_f32',
                      'pddp_derivs_track_f32',
                      'pddp_riccati_backward_variant_f32',
                      'pddp_line_search_track_f32',
                      'pddp_accept_f32',
                      'pddp_derivs_track_f32',
                      'pddp_riccati_backward_variant_f32',
                      'pddp_line_search_track_f32',
                      'pddp_accept_f32'],
                     (False, False, False, False, False, True, None, 0)),
 'table+reference-cleared-in-turn': (['pddp_derivs_batch_f32:8,12',
                                      'pddp_derivs_batch_f32',
                                      'pddp_riccati_backward_variant_f32',
                                      'pddp_line_search_batch_f32',
                                      'pddp_accept_f32',
                                      'pddp_round_nominal_f32:30'],
                                     (True,
                                      True,
                                      True,
                                      False,
                                      True,
                                      True,
                                      None,
                                      0)),
 'table+weights': (['pddp_derivs_weighted_f32:9,13',
                    'pddp_derivs_weighted_f32',
                    'pddp_riccati_backward_variant_f32',
                    'pddp_line_search_weighted_f32',
                    'pddp_accept_f32',
                    'pddp_derivs_weighted_f32',
                    'pddp_riccati_backward_variant_f32',
                    'pddp_line_search_weighted_f32',
                    'pddp_accept_f32',
                    'pddp_derivs_weighted_f32',
                    'pddp_riccati_backward_variant_f32',
                    'pddp_line_search_weighted_f32',
                    'pddp_accept_f32'],
                   (False, False, False, False, False, True, None, 0)),
 'table-capture_replay': (['pddp_derivs_batch_f32:8,12',
                           'pddp_derivs_batch_f32',
                           'pddp_riccati_backward_variant_f32',
                           'pddp_line_search_batch_f32',
                           'pddp_accept_f32'],
                          (False, False, False, False, False, True, None, 0)),
 'table-f64': (['pddp_derivs_batch_f64:8,12',
                'pddp_derivs_batch_f64',
                'pddp_riccati_backward_variant_f64',
                'pddp_line_search_batch_f64',
                'pddp_accept_f64',
                'pddp_derivs_batch_f64',
                'pddp_riccati_backward_variant_f64',
                'pddp_line_search_batch_f64',
                'pddp_accept_f64',
                'pddp_derivs_batch_f64',
                'pddp_riccati_backward_variant_f64',
                'pddp_line_search_batch_f64',
                'pddp_accept_f64'],
               (False, False, False, False, False, True, None, 0)),
 'weights': (['pddp_derivs_weighted_f32:1,9,13',
              'pddp_derivs_weighted_f32:1',
              'pddp_riccati_backward_variant_f32',
              'pddp_line_search_weighted_f32:1',
              'pddp_accept_f32',
              'pddp_derivs_weighted_f32:1',
              'pddp_riccati_backward_variant_f32',
              'pddp_line_search_weighted_f32:1',
              'pddp_accept_f32',
              'pddp_derivs_weighted_f32:1',
              'pddp_riccati_backward_variant_f32',
              'pddp_line_search_weighted_f32:1',
              'pddp_accept_f32'],
             (False, False, False, False, False, True, None, 0)),
 'weights-cleared': (['pddp_derivs_weighted_f32:1,9,13',
                      'pddp_derivs_weighted_f32:1',
                      'pddp_riccati_backward_variant_f32',
                      'pddp_line_search_weighted_f32:1',
                      'pddp_accept_f32',
                      '3*pddp_round_nominal_f32:30'],
                     (True, True, True, False, True, True, None, 0))})


@pytest.mark.parametrize("case", sorted(CASES))
def test_round_makes_the_recorded_calls(case, monkeypatch):
    log, flags = record(case, monkeypatch)
    print(case, log, flags)
    want_log, want_flags = EXPECTED[case]
    # (the first block was recorded before `ref_start` was a flag: none of its
    # cases sets a reference, so the constructor's 0 stands)
    want_flags += (0,) * (len(FLAGS) - len(want_flags))
    assert log == want_log
    assert flags == want_flags
