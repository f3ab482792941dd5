"""What costing the closed-loop rollouts along a reference costs
(ILQRSolver.closed_loop(track=True), pddp_closed_loop_track_f32 of
csrc/closed_loop.hip) next to the launches with one goal per rollout:
cartpole f32, 4096 trajectories, horizon 100, bounded, the gains of one sweep
at reg = 1, every plant row the shared problem, starts Z[b][0] +
U(-0.05, 0.05), S = 16 and 64, costs only and with the trajectories kept.

  (a) pddp_closed_loop_f32            against (A) the tracked noise-free launch;
  (c) pddp_closed_loop_noisy_f32 with process and measurement noise, std 0.02
      each                            against (C) the tracked one with both.

The reference has 160 rows, every one the shared goals, and is read from row 3
on: both legs of a pair do the same arithmetic.  The aim is each tracked launch
within 1.10 x of its sibling.

The protocol of tools/closed_loop_noise_time.py: one process, the legs
alternating launch by launch, events on the dispatch itself
(pddp_attach_events), WARM warm-up launches, median of REPS with [min, max]:
    python tools/closed_loop_track_time.py [B]"""
import ctypes
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from pddp_amd import _native
from pddp_amd.controllers.solver import ILQRSolver
from pddp_amd.examples import cartpole
from pddp_amd.utils.encoding import StateEncoding

B = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 4096
N, WARM, REPS, STD, ROWS, START = 100, 5, 20, 0.02, 160, 3
td = torch.float32
lib = _native.lib()


def event():
    e = ctypes.c_void_p()
    _native.check(lib.pddp_event_create(ctypes.byref(e)), "pddp_event_create")
    return e


def elapsed_us(e0, e1):
    ms = ctypes.c_float()
    _native.check(lib.pddp_event_elapsed_ms(e0, e1, ctypes.byref(ms)),
                  "pddp_event_elapsed_ms")
    return ms.value * 1e3


def stats(ts):
    ts = np.array(ts)
    return "%.1f us [%.1f, %.1f]" % (np.median(ts), ts.min(), ts.max())


def policy():
    """A solver with a nominal and the gains of one sweep (the same numbers
    at every call), every row of its table the shared problem."""
    prob = cartpole.CartpoleDynamicsModel(0.1).native_problem(
        StateEncoding.IGNORE_UNCERTAINTY, cartpole.CartpoleCost())
    s = ILQRSolver(prob, B, N, td, "cuda", torch.full((1,), -10.0, dtype=td),
                   torch.full((1,), 10.0, dtype=td))
    rng = np.random.RandomState(0)
    s.set_nominal(torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda(),
                  torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda())
    s.derivs(set_state=False)
    s.backward(reg=torch.full((B,), 1.0, dtype=torch.float64, device="cuda"))
    assert int(s.bwd_status.abs().sum()) == 0
    s.set_batch_problem()
    return s


plain, tracked = policy(), policy()
assert torch.equal(plain.gains, tracked.gains)
na = tracked.problem.aug_size
goals = tracked._shared_row()[_native.BATCH_X_GOAL:_native.BATCH_X_GOAL + na]
tracked.set_reference(goals.expand(B, ROWS, na), start=START)
e0, e1 = event(), event()
std = torch.full((4,), STD, dtype=td, device="cuda")
rng = np.random.RandomState(1)


def leg(s, **kw):
    def run():
        s.closed_loop(accepted=False, events=(e0, e1), **kw)
        return elapsed_us(e0, e1)
    return run


legs, pairs = {}, []
for S in (16, 64):
    z0 = (plain.Z[:, :1] + torch.from_numpy(rng.uniform(
        -0.05, 0.05, (B, S, 4))).to(td).cuda()).contiguous()
    for keep in (False, True):
        tag = "S %d, %s" % (S, "kept" if keep else "costs only")
        noise = dict(process_std=std, obs_std=std, seed=1)
        legs["(a) plain, " + tag] = leg(plain, z0=z0, keep=keep)
        legs["(A) tracked, " + tag] = leg(tracked, z0=z0, keep=keep,
                                          track=True)
        legs["(c) both streams, " + tag] = leg(plain, z0=z0, keep=keep,
                                               **noise)
        legs["(C) tracked, both streams, " + tag] = leg(
            tracked, z0=z0, keep=keep, track=True, **noise)
        pairs += [("(A) tracked, " + tag, "(a) plain, " + tag),
                  ("(C) tracked, both streams, " + tag,
                   "(c) both streams, " + tag)]

# on a constant reference the tracked launches give what their siblings give
S = 16
for noise in ({}, dict(process_std=std, obs_std=std, seed=1)):
    a = plain.closed_loop(samples=S, accepted=False, **noise)
    b = tracked.closed_loop(samples=S, accepted=False, track=True, **noise)
    assert torch.allclose(a.J, b.J, rtol=2e-4, atol=0), noise

times = {k: [] for k in legs}
for i in range(WARM + REPS):
    for name, run in legs.items():
        t = run()
        if i >= WARM:
            times[name].append(t)
print("cartpole f32, B %d, N %d, bounded, std %g, a reference of %d rows read "
      "from row %d; %d warm-up launches, median of %d [min, max]" % (
          B, N, STD, ROWS, START, WARM, REPS))
med = {k: np.median(v) for k, v in times.items()}
base = dict(pairs)
for name, ts in times.items():
    extra = ""
    if name in base:
        extra = "; %.2f x its sibling (aim 1.10)" % (med[name] /
                                                     med[base[name]])
    print("%s: %s%s" % (name, stats(ts), extra), flush=True)
