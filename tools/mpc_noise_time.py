"""What noise drawn in the advance adds to a control step of a receding-horizon
trial (ILQRSolver.mpc_closed_loop(process_std=, obs_std=),
pddp_mpc_advance_noisy_f32 of csrc/mpc_advance_noise.hip): the configuration of
tools/mpc_loop_time.py - cartpole f32, 4096 trajectories, horizon 100, bounded,
T = 20 control steps, rounds_per_step 1, 2 and 4, every plant the shared
problem with its parameters x U(0.9, 1.1) - run

  (a) without noise (mpc_loop_time.py's leg (a): pddp_mpc_advance_f32);
  (b) with a `disturbance` tensor [B][T][n] built beforehand (its making is
      not timed; the same launch as (a) with one more load per step);
  (c) with process noise, std 0.02, drawn in the launch;
  (d) with measurement noise, std 0.02 (the plant's state kept in x_true; the
      first observation's launch, pddp_mpc_observe_f32, is inside the events);
  (e) with both.

One process, the legs alternating loop by loop, each between two events
recorded on the solver's stream around the whole loop (no host synchronisation
inside); WARM warm-up loops, median of REPS with [min, max], per control step:
    python tools/mpc_noise_time.py [B]"""
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
STD = 0.02
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


def stats(ts, per=1):
    ts = np.array(ts) / per
    return "%.1f us [%.1f, %.1f]" % (np.median(ts), ts.min(), ts.max())


prob = cartpole.CartpoleDynamicsModel(0.1).native_problem(
    StateEncoding.IGNORE_UNCERTAINTY, cartpole.CartpoleCost())
s = ILQRSolver(prob, B, N, td, "cuda", torch.full((1,), -10.0, dtype=td),
               torch.full((1,), 10.0, dtype=td))
rng = np.random.RandomState(0)
z0 = torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda()
U0 = torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda()
P0, PN = _native.BATCH_PARAMS, s._PARAM_COUNT[prob.model]
params = s._shared_row()[P0:P0 + PN].repeat(B, 1) * torch.from_numpy(
    rng.uniform(0.9, 1.1, (B, PN))).to(td).cuda()
# (b)'s tensor: the process noise of (c), written out once
dist = (STD * s.closed_loop_draws(1, "process", seed=7, steps=T)[:, :, 0]) \
    .contiguous()
e0, e1 = event(), event()

LEGS = {"(a) no noise": dict(),
        "(b) disturbance tensor": dict(disturbance=dist),
        "(c) process noise": dict(process_std=STD, seed=7),
        "(d) obs noise": dict(obs_std=STD, seed=7),
        "(e) both": dict(process_std=STD, obs_std=STD, seed=7)}


def trial(R, kw):
    s.U.copy_(U0)
    s.mpc_closed_loop(T, R, z0=z0, params=params, events=(e0, e1), **kw)
    return elapsed_us(e0, e1)


times = {(name, R): [] for name in LEGS for R in ROUNDS}
for i in range(WARM + REPS):
    for (name, R), ts in times.items():
        t = trial(R, LEGS[name])
        if i >= WARM:
            ts.append(t)
print("cartpole f32, B %d, N %d, bounded, T %d, std %.2f; %d warm-up loops, "
      "median of %d [min, max] per control step; plan of the rounds: %s" % (
          B, N, T, STD, WARM, REPS, s._plan(s.kernel_variant)))
for R in ROUNDS:
    base = np.median(times[("(a) no noise", R)])
    for name in LEGS:
        ts = times[(name, R)]
        print("rounds per step %d, %s: %s; x %.3f of (a)" % (
            R, name, stats(ts, T), np.median(ts) / base), flush=True)
