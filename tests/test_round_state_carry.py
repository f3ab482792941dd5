"""The one-launch round with several rounds per launch keeps what a trajectory
carries from round to round - active, fresh, iter, mu, delta, J_opt - in LDS
(accept.hpp RoundState, round_n4_body.hpp) and reads it there in every round
of a launch; the global arrays are written as before.  `rounds(R)` is held here
to R calls of `round()` from the same start, byte for byte, at the smallest
shapes that exercise the record: a ragged last workgroup (B = 20: a pair with
missing trajectories), horizons around the sweep's blocks of sixteen steps and
the last one the launch serves (N = 127: no rows carried in LDS, the record
still is), trajectories that are masked from the start, that leave the fit in
the middle of a launch, that are rejected, and that converge."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

NAMES = ("Z", "U", "J_opt", "Jc", "mu", "delta", "state", "iter", "active",
         "fresh", "gains", "gains_acc")
ACCEPTED, REJECTED, NOT_PD, CONVERGED = 1, 2, 3, 5  # include/pddp_problem.h
# case (c): a start rough enough for rejected and accepted attempts side by
# side in five rounds - actions of the bound's size (10) on a 17-step horizon
ROUGH_SEED, ROUGH_U_SCALE = 3, 8.0


def _pair(B, N, seed=0, u_scale=None, bounded=True):
    """Two solvers on the same start (bench.py's synthetic inputs)."""
    import bench
    from pddp_amd.controllers.solver import ILQRSolver
    out = []
    for _ in range(2):
        s, z0, U, _b = bench.make_cartpole_solver(B, N, torch.float32, "cuda",
                                                  seed, 0)
        if not bounded:
            s = ILQRSolver(s._keep, B, N, torch.float32, "cuda", None, None,
                           kernel_variant=0)
        if u_scale is not None:
            U = U * (u_scale / 0.1)
        s.set_nominal(z0, U)
        out.append(s)
    return out


def _same(a, b, where):
    for k in NAMES:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape, (where, k)
        # byte for byte: the bit patterns, NaN payloads included
        assert torch.equal(x.contiguous().view(torch.uint8),
                           y.contiguous().view(torch.uint8)), (where, k)
    assert int(a.n_live.sum()) == int(b.n_live.sum()), (where, "n_live")


def _run(a, b, R, launches=2, **kw):
    """`launches` times: a.rounds(R) against R calls of b.round().  Returns the
    states the single-round side went through."""
    seen = []
    for trip in range(launches):
        a.rounds(R, **kw)
        for _ in range(R):
            b.round(**kw)
            seen.append(b.state.clone())
        torch.cuda.synchronize()
        assert a._one_launch is True and b._one_launch is True
        _same(a, b, trip)
    return torch.stack(seen)


@pytest.mark.parametrize("B", [16, 20])
@pytest.mark.parametrize("N", [1, 3, 17, 33, 127])
@pytest.mark.parametrize("R", [2, 5])
def test_rounds_in_one_launch_carry_the_state(B, N, R):
    a, b = _pair(B, N)
    _run(a, b, R, n_iterations=50)


def test_masked_trajectories_and_a_pair_that_never_runs():
    def mask(s):
        s.active[1::3] = 0
        s.active[0:4] = 0  # a whole (sweep, generator) pair without work
    a, b = _pair(16, 17)
    for s in (a, b):
        mask(s)
    iter0, Z0 = a.iter.clone(), a.Z.clone()
    _run(a, b, 5, n_iterations=50)
    # the pair that never ran: nothing of its trajectories moved
    assert torch.equal(a.iter[0:4], iter0[0:4])
    assert torch.equal(a.Z[0:4], Z0[0:4])
    assert not torch.equal(a.Z[4:], Z0[4:])


def test_trajectories_leave_the_fit_inside_a_launch():
    a, b = _pair(16, 17)
    _run(a, b, 5, n_iterations=2)
    # the iteration budget is spent: masks cleared in the middle of a launch
    assert int((b.active == 0).sum()) > 0


def test_rejected_and_accepted_attempts_in_one_launch():
    a, b = _pair(16, 17, seed=ROUGH_SEED, u_scale=ROUGH_U_SCALE)
    seen = _run(a, b, 5, launches=1, n_iterations=50)
    # (on the single-round side: the comparison above is not vacuous)
    assert bool(((seen == REJECTED) | (seen == NOT_PD)).any()), seen.tolist()
    assert bool((seen == ACCEPTED).any()), seen.tolist()


def test_convergence_inside_a_launch():
    a, b = _pair(16, 17)
    seen = _run(a, b, 5, tol=0.5, n_iterations=50)
    assert bool((seen == CONVERGED).any()), seen.tolist()
    assert int((b.active == 0).sum()) > 0


def test_unbounded_launch_carries_the_state():
    """The other gain branches run the same body (cartpole_branches.hip)."""
    a, b = _pair(20, 17, bounded=False)
    _run(a, b, 5, n_iterations=50)
