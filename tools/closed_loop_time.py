"""What a closed-loop evaluation costs (ILQRSolver.closed_loop,
pddp_closed_loop_f32 of csrc/closed_loop.hip) next to the line search that does
the same work per rollout: cartpole f32, 4096 trajectories, horizon 100,
bounded, the gains of one sweep at reg = 1, every plant row the shared problem,
starts Z[b][0] + U(-0.05, 0.05).

  - pddp_line_search_batch_f32 with 16 step sizes: 65 536 rollouts;
  - the closed loop with S = 16 (four trajectories to a wavefront, every lane
    reads its trajectory's row) and S = 64 (a wavefront per trajectory), costs
    only and with the trajectories kept.

One process, the legs alternating launch by launch, events attached to the
dispatch itself (pddp_attach_events); WARM warm-up launches, median of REPS
with [min, max]:
    python tools/closed_loop_time.py [B]"""
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
N, A, WARM, REPS = 100, 16, 5, 20
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


prob = cartpole.CartpoleDynamicsModel(0.1).native_problem(
    StateEncoding.IGNORE_UNCERTAINTY, cartpole.CartpoleCost())
s = ILQRSolver(prob, B, N, td, "cuda", torch.full((1,), -10.0, dtype=td),
               torch.full((1,), 10.0, dtype=td),
               alphas=torch.linspace(1.0, 0.01, A).to(td))
rng = np.random.RandomState(0)
s.set_nominal(torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda(),
              torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda())
s.derivs(set_state=False)
s.backward(reg=torch.full((B,), 1.0, dtype=torch.float64, device="cuda"))
assert int(s.bwd_status.abs().sum()) == 0
s.set_batch_problem()  # (every row the shared problem)
table = s.batch_table
e0, e1 = event(), event()

legs = {"pddp_line_search_batch_f32, A %d" % A: lambda ev: s._launch(
    ev, s.line_search)}
for S in (16, 64):
    z0 = (s.Z[:, :1] + torch.from_numpy(rng.uniform(
        -0.05, 0.05, (B, S, 4))).to(td).cuda()).contiguous()
    for keep in (False, True):
        name = "closed loop, S %d, %s" % (S, "kept" if keep else "costs only")
        legs[name] = lambda ev, z0=z0, keep=keep: s.closed_loop(
            z0=z0, accepted=False, keep=keep, events=ev)

times = {k: [] for k in legs}
for i in range(WARM + REPS):
    for name, leg in legs.items():
        leg((e0, e1))
        t = elapsed_us(e0, e1)
        if i >= WARM:
            times[name].append(t)
base = np.median(times[next(iter(legs))])
print("cartpole f32, B %d, N %d, bounded; %d warm-up launches, median of %d "
      "[min, max]" % (B, N, WARM, REPS))
for name, ts in times.items():
    extra = ""
    if name.startswith("closed loop"):
        S = int(name.split("S ")[1].split(",")[0])
        extra = "; %.2f x the line search; %.3g rollout-steps / s" % (
            np.median(ts) / base, B * S * N / (np.median(ts) * 1e-6))
    print("%s: %s%s" % (name, stats(ts), extra), flush=True)
