"""Which code the plugin path runs (controllers/plugin.py TorchProblem): the
four decisions and `capture_ok` as Boolean functions of the five predicates,
on a bare TorchProblem whose predicates are stubs.  No device is needed: the
decisions are host code."""
import itertools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pddp_amd import StateEncoding  # noqa: E402
from pddp_amd.controllers.plugin import TorchProblem  # noqa: E402


class _Model(object):
    """What the GP line search's shape test reads: a cartpole's layout."""
    state_size = 4
    angular_indices = [2]
    non_angular_indices = [0, 1, 3]

    def eval(self):
        return self


def _plugin(bnn_cost, bnn_plain, jvp, gp, gp_search, qr, model=_Model):
    """A TorchProblem that answers its five predicates with the given
    Booleans; `_bnn_native_ok` by `need_cost`.  `asked` collects the grad mode
    the dynamics predicates were asked under."""
    plugin = TorchProblem(model(), None, StateEncoding.DEFAULT)
    plugin.asked = []

    def bnn(s_, need_cost=True):
        plugin.asked.append(torch.is_grad_enabled())
        return bnn_cost if need_cost else bnn_plain
    plugin._bnn_native_ok = bnn
    plugin._bnn_jvp_ok = lambda s_: jvp
    plugin._gp_native_ok = lambda s_: gp
    plugin._gp_line_search_ok = lambda s_: gp_search
    plugin._qr_cost_native_ok = lambda s_, co=None: qr
    return plugin


# (need_cost=True asks for more than need_cost=False: it implies it)
COMBINATIONS = [c for c in itertools.product((False, True), repeat=6)
                if c[1] or not c[0]]


def test_the_combinations_are_the_admissible_ones():
    assert len(COMBINATIONS) == 48


@pytest.mark.parametrize("combo", COMBINATIONS,
                         ids=lambda c: "".join("01"[v] for v in c))
def test_decisions_are_the_parents_boolean_functions(combo, monkeypatch):
    monkeypatch.delenv("PDDP_NO_GP_ROLLOUT", raising=False)
    bnn_cost, bnn_plain, jvp, gp, gp_search, qr = combo
    plugin = _plugin(*combo)
    s = types.SimpleNamespace(m=1)
    assert plugin._rollout_path(s) == ("bnn" if bnn_cost else "torch")
    with torch.enable_grad():
        plugin.asked.clear()
        assert plugin._dynamics_path(s) == (
            "bnn" if bnn_plain and jvp else "gp" if gp else "autograd")
        # (the network's own test answers differently with autograd on)
        assert plugin.asked == [False]
    assert plugin._cost_path(s) == ("hip" if qr else "autograd")
    assert plugin._line_search_path(s) == (
        "bnn" if bnn_cost else "gp_rollout" if gp_search else "generic")
    assert plugin.capture_ok(s) is bool(
        (bnn_cost and jvp and qr) or (gp_search and qr))


def test_predicates_and_switches_are_asked_at_every_call():
    """Nothing is cached: a predicate replaced on the instance, or a switch
    flipped, between two calls changes the second answer."""
    plugin = _plugin(False, False, False, True, True, True)
    s = types.SimpleNamespace(m=1)
    assert plugin._line_search_path(s) == "gp_rollout"
    plugin._gp_line_search_ok = lambda s_: False
    assert plugin._line_search_path(s) == "generic"
    assert plugin._dynamics_path(s) == "gp"
    plugin._gp_native_ok = lambda s_: False
    assert plugin._dynamics_path(s) == "autograd"
    assert plugin.capture_ok(s) is False


def test_the_switches_are_declared_and_default_to_on():
    for name in ("use_native_bnn", "use_native_bnn_jvp", "use_native_gp",
                 "use_native_cost", "use_gp_rollout"):
        assert getattr(TorchProblem, name) is True
    a = TorchProblem(None, None, StateEncoding.DEFAULT)
    b = TorchProblem(None, None, StateEncoding.DEFAULT)
    a.use_native_cost = False  # (an instance's own; the class keeps its)
    assert b.use_native_cost is True and TorchProblem.use_native_cost is True
    s = types.SimpleNamespace(m=1, dtype=torch.float32, n=14)
    assert a._qr_cost_native_ok(s) is False


class _Wide(_Model):       # more than six states
    state_size = 7
    angular_indices = []
    non_angular_indices = list(range(7))


class _Angles(_Model):     # six states, nine augmented features
    state_size = 6
    angular_indices = [1, 2, 3]
    non_angular_indices = [0, 4, 5]


@pytest.mark.parametrize("off", ["environment", "switch", "state_size",
                                 "features", "actions"])
def test_the_ways_off_the_gp_rollout_kernel(off, monkeypatch):
    monkeypatch.delenv("PDDP_NO_GP_ROLLOUT", raising=False)
    model = {"state_size": _Wide, "features": _Angles}.get(off, _Model)
    plugin = _plugin(False, False, False, True, True, True, model=model)
    s = types.SimpleNamespace(m=5 if off == "actions" else 4)
    if off == "environment":
        assert plugin._line_search_path(s) == "gp_rollout"
        monkeypatch.setenv("PDDP_NO_GP_ROLLOUT", "1")
    if off == "switch":
        assert plugin._line_search_path(s) == "gp_rollout"
        plugin.use_gp_rollout = False
    assert plugin._line_search_path(s) == "gp_step"
    # (the GP line search is asked for first: without it, the generic loop)
    plugin._gp_line_search_ok = lambda s_: False
    assert plugin._line_search_path(s) == "generic"


@pytest.mark.parametrize("path", ["bnn", "gp_rollout", "gp_step"])
def test_line_search_runs_what_the_decision_names(path):
    plugin = _plugin(False, False, False, False, False, False)
    plugin.cost = _Model()  # (anything with eval())
    plugin._line_search_path = lambda s_: path
    ran = []
    plugin._bnn_rollouts = lambda *a, **k: ran.append("bnn")
    plugin._line_search_gp = lambda *a, **k: ran.append("gp_rollout")
    plugin._line_search_gp_torch = lambda *a, **k: ran.append("gp_step")
    s = types.SimpleNamespace(A=2, alphas=None, gains=None, Zc=None, Uc=None,
                              bwd_status=None, Jc=torch.zeros(3, 2))
    plugin.line_search(s)
    assert ran == [path]
