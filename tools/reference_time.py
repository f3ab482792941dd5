"""What a goal per time step costs (ILQRSolver.set_reference, the track_*
kernels of csrc/goal_kernels.hpp and csrc/mpc_advance.hip): cartpole f32, 4096
trajectories, horizon 100, bounded, the fit's ten step sizes.  Every row of
the table is the shared problem and every row of the reference its goals, so
both legs of a pair do
the same work on the same buffers.  One process, the legs of a pair
alternating launch by launch, events attached to the dispatch itself
(pddp_attach_events):

  - pddp_line_search_track_f32 against pddp_line_search_batch_f32;
  - pddp_derivs_track_f32 against pddp_derivs_batch_f32;
  - pddp_mpc_advance_track_f32 against pddp_mpc_advance_f32 (z0 and U put back
    before every launch, outside the events);
  - a whole round() with a reference against round() with a table, two
    solvers taking turns, pddp_event_record around each round.

WARM warm-up launches, median of REPS [min, max]:
    python tools/reference_time.py [B]"""
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
N, WARM, REPS, REF_LEN = 100, 5, 20, 160
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


def solver(reference):
    prob = cartpole.CartpoleDynamicsModel(0.1).native_problem(
        StateEncoding.IGNORE_UNCERTAINTY, cartpole.CartpoleCost())
    s = ILQRSolver(prob, B, N, td, "cuda", torch.full((1,), -10.0, dtype=td),
                   torch.full((1,), 10.0, dtype=td))
    s._keep = prob
    s.set_batch_problem()
    if reference:
        x_goal = s.batch_table[:, None, 8:8 + prob.aug_size]
        s.set_reference(x_goal.expand(-1, REF_LEN, -1), start=3)
    return s


def report(what, a, b, ta, tb):
    print("%s, B %d N %d f32: %s %s; %s %s; ratio %.2f" % (
        what, B, N, a, stats(ta), b, stats(tb),
        np.median(tb) / np.median(ta)), flush=True)


rng = np.random.RandomState(0)
z0 = torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda()
U0 = torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda()
e0, e1 = event(), event()

# -- records and line search, kernel time -------------------------------------
s = solver(True)
ref = s.reference
s.set_nominal(z0, U0)
s.derivs(set_state=False)
s.backward(reg=torch.full((B,), 1.0, dtype=torch.float64, device="cuda"))
assert int(s.bwd_status.abs().sum()) == 0
# the same work: the records and the candidates' first steps agree to rounding
# (from these gains most 100-step rollouts leave the basin: the costs
# themselves are not comparable)
s.line_search()
rec_t, Zc_t = s._rec.clone(), s.Zc[:, :9].clone()
s.reference = None
s.derivs(set_state=False)
s.line_search()
for what, a, b in (("records", rec_t, s._rec), ("candidates, steps 0 .. 8",
                                                Zc_t, s.Zc[:, :9])):
    dev = float((a - b).abs().max() / b.abs().max())
    print("%s: largest deviation %.2e of the largest entry" % (what, dev))
    assert dev < 2e-4
for what, fn in (("line search, A %d" % s.A, s.line_search),
                 ("records", lambda: s._derivs(None, s._jscr, None))):
    times = {"batch": [], "track": []}
    for i in range(WARM + REPS):
        for leg in ("batch", "track"):
            s.reference = ref if leg == "track" else None
            s._launch((e0, e1), fn)
            t = elapsed_us(e0, e1)
            if i >= WARM:
                times[leg].append(t)
    name = "pddp_line_search" if "search" in what else "pddp_derivs"
    report(what, name + "_batch_f32", name + "_track_f32", times["batch"],
           times["track"])

# -- the hand-over, kernel time -----------------------------------------------
T = 8
p = _native.ptr
opts = dict(dtype=td, device="cuda")
logs = (torch.empty(B, T + 1, 4, **opts), torch.empty(B, T, 1, **opts),
        torch.empty(B, **opts),
        torch.empty(B, T, dtype=torch.int32, device="cuda"),
        torch.empty(B, T, dtype=torch.uint8, device="cuda"))
tail = (B, N, T, 0, p(s.z0), p(s.U), p(s.Z), p(s.u_min), p(s.u_max), None,
        None, None, *[p(x) for x in logs], p(s.mu), p(s.delta), p(s.state),
        p(s.iter), p(s.active), p(s.fresh), p(s.n_live), s._s())
head = (ctypes.addressof(s.problem), p(s.batch_table))
times = {"batch": [], "track": []}
for i in range(WARM + REPS):
    for leg in ("batch", "track"):
        s.z0.copy_(z0)
        s.U.copy_(U0)
        lib.pddp_attach_events(e0, e1)
        if leg == "track":
            rc = lib.pddp_mpc_advance_track_f32(*head, p(ref), REF_LEN, 3,
                                                *tail)
        else:
            rc = lib.pddp_mpc_advance_f32(*head, *tail)
        _native.check(rc, "pddp_mpc_advance")
        t = elapsed_us(e0, e1)
        if i >= WARM:
            times[leg].append(t)
report("hand-over", "pddp_mpc_advance_f32", "pddp_mpc_advance_track_f32",
       times["batch"], times["track"])

# -- a whole round -------------------------------------------------------------
legs = {"table": solver(False), "reference": solver(True)}
times = {k: [] for k in legs}
for x in legs.values():
    x.set_nominal(z0, U0)
for i in range(WARM + REPS):
    for leg, x in legs.items():
        _native.check(lib.pddp_event_record(e0, x._s()), "pddp_event_record")
        x.round(5e-6, 1e10, 1 << 30)  # (nobody leaves the loop)
        _native.check(lib.pddp_event_record(e1, x._s()), "pddp_event_record")
        t = elapsed_us(e0, e1)
        if i >= WARM:
            times[leg].append(t)
for leg, x in legs.items():
    assert x._plan(0) == "records+separate", leg
report("round (live %s)" % ", ".join(
    "%d" % int(x.active.sum()) for x in legs.values()),
    "records+separate, table", "records+separate, reference", times["table"],
    times["reference"])
