"""What a receding-horizon trial costs on the device
(ILQRSolver.mpc_closed_loop, pddp_mpc_advance_f32 of csrc/mpc_advance.hip)
next to the same trial composed from the entry points there were before it:
cartpole f32, 4096 trajectories, horizon 100, bounded, T = 20 control steps,
rounds_per_step 1, 2 and 4, every plant the shared problem with its parameters
x U(0.9, 1.1).

  (a) mpc_closed_loop: per control step the rounds and ONE advance launch;
  (b) the composed trial: per control step the rounds, the plant step by
      pddp_nominal_rollout_batch_f32 at N = 1 on the plant rows, a torch shift
      of U and set_nominal (two copies, the seven fills of
      reset_controller_state, the nominal rollout).  It logs nothing and sums
      no cost: less work than (a) does;
  (c) the advance launch alone against pddp_nominal_rollout_f32 alone on the
      same buffers, events attached to the dispatch (pddp_attach_events).
      The data drifts between the repetitions of (c): every advance steps z0
      through the perturbed plant and shifts U, and the rollout is timed on
      whatever that left ((a) resets z0 and U at the start of each loop).

One process, the legs alternating loop by loop; (a) and (b) between two events
recorded on the solver's stream around the whole loop (no host synchronisation
inside); WARM warm-up loops, median of REPS with [min, max]:
    python tools/mpc_loop_time.py [B]"""
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
N, T, WARM, REPS = 100, 20, 5, 20
ROUNDS = (1, 2, 4)
td = torch.float32
lib = _native.lib()
p = _native.ptr


def event():
    e = ctypes.c_void_p()
    _native.check(lib.pddp_event_create(ctypes.byref(e)), "pddp_event_create")
    return e


def elapsed_us(e0, e1):
    ms = ctypes.c_float()
    _native.check(lib.pddp_event_elapsed_ms(e0, e1, ctypes.byref(ms)),
                  "pddp_event_elapsed_ms")
    return ms.value * 1e3


def stats(ts, per=1):
    ts = np.array(ts) / per
    return "%.1f us [%.1f, %.1f]" % (np.median(ts), ts.min(), ts.max())


prob = cartpole.CartpoleDynamicsModel(0.1).native_problem(
    StateEncoding.IGNORE_UNCERTAINTY, cartpole.CartpoleCost())


def solver():
    return ILQRSolver(prob, B, N, td, "cuda", torch.full((1,), -10.0, dtype=td),
                      torch.full((1,), 10.0, dtype=td))


rng = np.random.RandomState(0)
z0 = torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda()
U0 = torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda()
sa, sb = solver(), solver()
P0, PN = _native.BATCH_PARAMS, sa._PARAM_COUNT[prob.model]
params = sa._shared_row()[P0:P0 + PN].repeat(B, 1) * torch.from_numpy(
    rng.uniform(0.9, 1.1, (B, PN))).to(td).cuda()
plant = sb._plant_table("mpc_loop_time", params, None, None)
e0, e1 = event(), event()
step = torch.empty(B, 2, 4, dtype=td, device="cuda")


def fused(R):
    sa.U.copy_(U0)
    sa.mpc_closed_loop(T, R, z0=z0, params=params, events=(e0, e1))
    return elapsed_us(e0, e1)


def composed(R):
    s = sb
    _native.check(lib.pddp_event_record(e0, s._s()), "pddp_event_record")
    s.set_nominal(z0, U0)
    for t in range(T):
        s.rounds(R, n_iterations=1)
        u0 = s.U[:, :1].contiguous()
        _native.call("pddp_nominal_rollout_batch", td, s._pp, p(plant), B, 1,
                     p(s.z0), p(u0), p(s.u_min), p(s.u_max), None, p(step),
                     s._s())
        s.set_nominal(step[:, 1], torch.cat([s.U[:, 1:], s.U[:, -1:]], 1))
    _native.check(lib.pddp_event_record(e1, s._s()), "pddp_event_record")
    return elapsed_us(e0, e1)


# (c): one launch each on sa's buffers, the trial logs of a T = 1 trial
logs = (torch.empty(B, 2, 4, dtype=td, device="cuda"),
        torch.empty(B, 1, 1, dtype=td, device="cuda"),
        torch.empty(B, dtype=td, device="cuda"),
        torch.empty(B, 1, dtype=torch.int32, device="cuda"),
        torch.empty(B, 1, dtype=torch.uint8, device="cuda"))


def advance_alone(_):
    s = sa
    lib.pddp_attach_events(e0, e1)
    _native.call("pddp_mpc_advance", td, s._pp, None, B, N, 1, 0, p(s.z0),
                 p(s.U), p(s.Z), p(s.u_min), p(s.u_max), p(plant), None, None,
                 *[p(x) for x in logs], p(s.mu), p(s.delta), p(s.state),
                 p(s.iter), p(s.active), p(s.fresh), p(s.n_live), s._s())
    return elapsed_us(e0, e1)


def rollout_alone(_):
    sa._launch((e0, e1), sa.nominal_rollout)
    return elapsed_us(e0, e1)


legs = {}
for R in ROUNDS:
    legs["(a) mpc_closed_loop, %d rounds per step" % R] = (fused, R)
    legs["(b) composed trial, %d rounds per step" % R] = (composed, R)
legs["(c) pddp_mpc_advance_f32 alone"] = (advance_alone, 0)
legs["(c) pddp_nominal_rollout_f32 alone"] = (rollout_alone, 0)

times = {k: [] for k in legs}
for i in range(WARM + REPS):
    for name, (leg, R) in legs.items():
        t = leg(R)
        if i >= WARM:
            times[name].append(t)
print("cartpole f32, B %d, N %d, bounded, T %d; %d warm-up loops, median of %d "
      "[min, max]; plan of the rounds: %s" % (
          B, N, T, WARM, REPS, sa._plan(sa.kernel_variant)))
for R in ROUNDS:
    a = times["(a) mpc_closed_loop, %d rounds per step" % R]
    b = times["(b) composed trial, %d rounds per step" % R]
    print("rounds per step %d, per control step: (a) %s; (b) %s; (a) / (b) "
          "%.2f" % (R, stats(a, T), stats(b, T), np.median(a) / np.median(b)),
          flush=True)
a = times["(c) pddp_mpc_advance_f32 alone"]
b = times["(c) pddp_nominal_rollout_f32 alone"]
print("(c) the advance alone %s; the nominal rollout alone %s; ratio %.2f" % (
    stats(a), stats(b), np.median(a) / np.median(b)), flush=True)
