"""What per-trajectory cost weights cost next to a reference (ILQRSolver with
set_reference and set_batch_weights, the track_weighted_* kernels of
csrc/goal_kernels.hpp): cartpole f32, 4096 trajectories, horizon 100, bounded,
the fit's ten step sizes; every row of the weights holds the shared diagonals
and every row of the reference the problem's own goals, so all legs do the same
work.  The method of tools/batch_weights_time.py.

  - the two kernels: pddp_derivs_track_weighted_f32 against
    pddp_derivs_track_f32 and pddp_line_search_track_weighted_f32 against
    pddp_line_search_track_f32 on the same buffers, events attached to the
    dispatch itself (pddp_attach_events), the two alternating;
  - a whole round(), two legs alternating round by round, each on a solver of
    its own: with a reference and weights, with the reference alone - the same
    records+separate plan.  Every timed round starts from the same nominal
    (set_nominal outside the events: all B trajectories fresh and live, so a
    round is records, sweep, search and accept of the whole batch in every
    repetition); pddp_event_record on the stream around each round.

One process, WARM warm-up repetitions, median of REPS with [min, max]; under a
time limit of its own:
    timeout -k 10 300 python tools/track_weights_time.py [B]"""
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
N, WARM, REPS, L_REF = 100, 5, 20, 8
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


def overlap(a, b):
    return max(min(a), min(b)) <= min(max(a), max(b))


def solver(weights):
    """A solver tracking the constant reference, with the shared diagonals in
    every row of the weights where asked for."""
    prob = cartpole.CartpoleDynamicsModel(0.1).native_problem(
        StateEncoding.IGNORE_UNCERTAINTY, cartpole.CartpoleCost())
    s = ILQRSolver(prob, B, N, td, "cuda", torch.full((1,), -10.0, dtype=td),
                   torch.full((1,), 10.0, dtype=td))
    s._keep = prob
    goal = torch.tensor(list(prob.x_goal)[:prob.aug_size], dtype=torch.float64)
    s.set_reference(goal.repeat(B, L_REF, 1))  # (u_ref: the problem's u_goal)
    if weights:
        s.set_batch_weights(keep_reference=True)
    return s


rng = np.random.RandomState(0)
z0 = torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda()
U0 = torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda()
e0, e1 = event(), event()

# -- the two kernels, kernel time ---------------------------------------------
s = solver(False)
s.set_nominal(z0, U0)
s.derivs(set_state=False)
rec_track = s._rec.clone()
s.backward(reg=torch.full((B,), 1.0, dtype=torch.float64, device="cuda"))
assert int(s.bwd_status.abs().sum()) == 0
s.set_batch_weights(keep_reference=True)
weights = s.batch_weights
s.derivs(set_state=False)
# the same work: the records agree to rounding
dev = float((s._rec - rec_track).abs().max() / rec_track.abs().max())
print("records, track_weighted against track: largest deviation %.2e of the "
      "largest entry" % dev)
assert dev < 2e-4
for name, call in (("derivs", lambda: s.derivs(set_state=False)),
                   ("line_search", s.line_search)):
    times = {"track": [], "track_weighted": []}
    for i in range(WARM + REPS):
        for leg in ("track", "track_weighted"):
            s.batch_weights = weights if leg == "track_weighted" else None
            s._launch((e0, e1), call)
            t = elapsed_us(e0, e1)
            if i >= WARM:
                times[leg].append(t)
    tt, tw = np.median(times["track"]), np.median(times["track_weighted"])
    print("%s, B %d N %d A %d f32: pddp_%s_track_f32 %s; "
          "pddp_%s_track_weighted_f32 %s; ratio %.2f; [min, max] %s" % (
              name, B, N, s.A, name, stats(times["track"]), name,
              stats(times["track_weighted"]), tw / tt,
              "overlap" if overlap(times["track"], times["track_weighted"])
              else "do not overlap"), flush=True)

# -- a whole round ------------------------------------------------------------
LEGS = ("reference + weights", "reference")
solvers = {leg: solver(leg.endswith("weights")) for leg in LEGS}
ts = {leg: [] for leg in LEGS}
for i in range(WARM + REPS):
    for leg in LEGS:
        s = solvers[leg]
        s.set_nominal(z0, U0)
        _native.check(lib.pddp_event_record(e0, s._s()), "pddp_event_record")
        s.round(5e-6, 1e10, 1 << 30)  # (nobody leaves the loop)
        _native.check(lib.pddp_event_record(e1, s._s()), "pddp_event_record")
        t = elapsed_us(e0, e1)
        if i >= WARM:
            ts[leg].append(t)
for leg in LEGS:
    assert solvers[leg]._plan(0) == "records+separate", leg
med = {leg: np.median(ts[leg]) for leg in LEGS}
print("round, B %d N %d f32: %s" % (B, N, "; ".join(
    "%s %s (live %d)" % (leg, stats(ts[leg]), int(solvers[leg].active.sum()))
    for leg in LEGS)), flush=True)
print("(reference + weights) / reference %.2f; [min, max] %s" % (
    med[LEGS[0]] / med[LEGS[1]],
    "overlap" if overlap(ts[LEGS[0]], ts[LEGS[1]]) else "do not overlap"),
    flush=True)
