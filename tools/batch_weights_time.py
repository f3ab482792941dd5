"""What per-trajectory cost weights cost (ILQRSolver.set_batch_weights, the
weighted_* kernels of csrc/goal_kernels.hpp): cartpole f32, 4096 trajectories,
horizon 100, bounded, the fit's ten step sizes; every row of the weights (and
of the table) is the shared problem's, so all legs do the same work.

  - the two kernels: pddp_derivs_weighted_f32 against pddp_derivs_batch_f32
    and pddp_line_search_weighted_f32 against pddp_line_search_batch_f32 on
    the same buffers, events attached to the dispatch itself
    (pddp_attach_events), the two alternating;
  - a whole round(), three legs alternating round by round, each on a solver
    of its own: with weights; (a) with a replicated set_batch_problem() table
    - the same records+separate plan: what the weights themselves cost; (b)
    the uniform problem as the solver runs it by default (one launch): what
    leaving that plan costs.  Every timed round starts from the same nominal
    (set_nominal outside the events: all B trajectories fresh and live, so a
    round is records, sweep, search and accept of the whole batch in every
    repetition); pddp_event_record on the stream around each round.

One process, WARM warm-up rounds, median of REPS with [min, max]:
    python tools/batch_weights_time.py [B]"""
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
N, WARM, REPS = 100, 5, 20
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


def solver():
    prob = cartpole.CartpoleDynamicsModel(0.1).native_problem(
        StateEncoding.IGNORE_UNCERTAINTY, cartpole.CartpoleCost())
    s = ILQRSolver(prob, B, N, td, "cuda", torch.full((1,), -10.0, dtype=td),
                   torch.full((1,), 10.0, dtype=td))
    s._keep = prob
    return s


rng = np.random.RandomState(0)
z0 = torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda()
U0 = torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda()
e0, e1 = event(), event()

# -- the two kernels, kernel time ---------------------------------------------
s = solver()
s.set_nominal(z0, U0)
s.set_batch_problem()
table = s.batch_table
s.derivs(set_state=False)
rec_batch = s._rec.clone()
s.backward(reg=torch.full((B,), 1.0, dtype=torch.float64, device="cuda"))
assert int(s.bwd_status.abs().sum()) == 0
s.set_batch_weights()
weights = s.batch_weights
s.derivs(set_state=False)
# the same work: the records agree to rounding
dev = float((s._rec - rec_batch).abs().max() / rec_batch.abs().max())
print("records, weighted against batch: largest deviation %.2e of the "
      "largest entry" % dev)
assert dev < 2e-4
for name, call in (("derivs", lambda: s.derivs(set_state=False)),
                   ("line_search", s.line_search)):
    times = {"batch": [], "weighted": []}
    for i in range(WARM + REPS):
        for leg in ("batch", "weighted"):
            s.batch_weights = weights if leg == "weighted" else None
            s._launch((e0, e1), call)
            t = elapsed_us(e0, e1)
            if i >= WARM:
                times[leg].append(t)
    tb, tw = np.median(times["batch"]), np.median(times["weighted"])
    print("%s, B %d N %d A %d f32: pddp_%s_batch_f32 %s; pddp_%s_weighted_f32 "
          "(table + weights) %s; ratio %.2f" % (
              name, B, N, s.A, name, stats(times["batch"]), name,
              stats(times["weighted"]), tw / tb), flush=True)

# -- a whole round ------------------------------------------------------------
LEGS = ("records+separate, weights", "records+separate, table",
        "default (one launch)")
solvers, ts = {}, {leg: [] for leg in LEGS}
for leg in LEGS:
    solvers[leg] = s = solver()
    if leg.endswith("weights"):
        s.set_batch_weights()
    if leg.endswith("table"):
        s.set_batch_problem()
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
    assert solvers[leg]._plan(0) == (
        "one_launch" if leg.startswith("default") else "records+separate"), leg
med = {leg: np.median(ts[leg]) for leg in LEGS}
print("round, B %d N %d f32: %s" % (B, N, "; ".join(
    "%s %s (live %d)" % (leg, stats(ts[leg]), int(solvers[leg].active.sum()))
    for leg in LEGS)), flush=True)
print("weights / table (a) %.2f; weights / one launch (b) %.2f" % (
    med[LEGS[0]] / med[LEGS[1]], med[LEGS[0]] / med[LEGS[2]]), flush=True)
