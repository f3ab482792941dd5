"""The launch sequence of a solver round, recorded call by call.

`ILQRSolver._plan()` picks one of five sequences (the table in
pddp_amd/controllers/solver.py).  A recorder around the C ABI
(`_native.call`, `_native.call_rc` and the three entry points the solver
reaches through `_native.lib()` itself) logs, for every call a case makes
after `set_nominal`, the entry point with its dtype suffix and the positions
of its NULL arguments; the real call goes through.  Runs of one entry are
written "count*entry".

EXPECTED is what this recorder logged, together with the solver's flags at the
end of each case, on commit e505e79 ("GP step kernels: chunked form for
training sets beyond one LDS"), the last one whose `round()` decided its
launches condition by condition: a change of solver.py that makes other calls,
in another order, or leaves other flags fails here.  (alphas17: pddp_accept
takes 16 step sizes at most, so on that commit the nominal+separate fall-back
ends in a NativeError after its launches; the record holds that too.)"""
import ctypes

import numpy as np
import pytest
import torch

from pddp_amd import _native
from test_gpu_parity import BOUND, DT, MEAN0

pytestmark = pytest.mark.gpu

B, N = 32, 20
DIRECT = ("pddp_round_nominal_f32", "pddp_attach_events",
          "pddp_search_candidates")
FLAGS = ("_one_launch", "_nominal_sweep", "_fused", "_derivs_due",
         "_rec_stale", "candidates_kept", "last_search_timed")


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


@pytest.mark.parametrize("case", sorted(CASES))
def test_round_makes_the_recorded_calls(case, monkeypatch):
    log, flags = record(case, monkeypatch)
    print(case, log, flags)
    want_log, want_flags = EXPECTED[case]
    assert log == want_log
    assert flags == want_flags
