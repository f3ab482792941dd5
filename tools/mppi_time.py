"""What the softmin-weighted update costs (ILQRSolver.mppi, pddp_mppi_f32 of
csrc/mppi.hip) next to sampled shooting on the same candidates
(ILQRSolver.shoot, pddp_shoot_f32 of csrc/shoot.hip, a unit this one leaves
byte for byte as it was) and next to one solver round: cartpole f32, 4096
trajectories, horizon 100, bounded, base actions 0.1 randn, std 3, smooth 0.7,
temperature 100, S = 16, 64 and 256.

  (a) shoot(S, adopt=False): costs, argmin, the winner rolled out again;
  (b) mppi(S, adopt=False): the launch alone - costs, argmin, the weights, the
      draws a second time, the weighted sequence rolled out;
  (c) one round() of the solver (the one-launch round), for scale.

The protocol of tools/shoot_time.py: one process, the legs alternating launch
by launch, events on the dispatch itself (pddp_attach_events), WARM warm-up
launches, median of REPS with [min, max]:
    python tools/mppi_time.py [B]"""
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
N, WARM, REPS, STD, SMOOTH, LAM = 100, 5, 20, 3.0, 0.7, 100.0
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
bounds = (torch.full((1,), -10.0, dtype=td), torch.full((1,), 10.0, dtype=td))
rng = np.random.RandomState(0)
z0 = torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda()
U = torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda()
s = ILQRSolver(prob, B, N, td, "cuda", *bounds)
s.set_nominal(z0, U)
# (the round's solver: its nominal moves, the rollouts' does not)
r = ILQRSolver(prob, B, N, td, "cuda", *bounds)
r.set_nominal(z0, U)
lam = torch.full((B,), LAM, dtype=td, device="cuda")
e0, e1 = event(), event()
t0, t1 = torch.cuda.Event(enable_timing=True), \
    torch.cuda.Event(enable_timing=True)


def shoot_leg(S):
    def run():
        s.shoot(S, STD, smooth=SMOOTH, seed=1, adopt=False, events=(e0, e1))
        return elapsed_us(e0, e1)
    return run


def mppi_leg(S):
    def run():
        s.mppi(S, STD, lam, smooth=SMOOTH, seed=1, adopt=False,
               events=(e0, e1))
        return elapsed_us(e0, e1)
    return run


def round_leg():  # (torch events around the call: one launch, or several)
    r.set_nominal(z0, U)
    t0.record()
    r.round()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3


legs = {}
for S in (16, 64, 256):
    legs["(a) shoot, S %d" % S] = shoot_leg(S)
    legs["(b) mppi, S %d" % S] = mppi_leg(S)
legs["(c) one round"] = round_leg

times = {k: [] for k in legs}
for i in range(WARM + REPS):
    for name, leg in legs.items():
        t = leg()
        if i >= WARM:
            times[name].append(t)
print("cartpole f32, B %d, N %d, bounded, std %g, smooth %g, temperature %g; "
      "%d warm-up launches, median of %d [min, max]" % (
          B, N, STD, SMOOTH, LAM, WARM, REPS))
med = {k: np.median(v) for k, v in times.items()}
for name, ts in times.items():
    extra = ""
    if name[:3] == "(b)":
        base = med["(a) shoot, " + name.split(", ")[1]]
        extra = "; %.2f x (a), %.2f x one round" % (
            med[name] / base, med[name] / med["(c) one round"])
    print("%s: %s%s" % (name, stats(ts), extra), flush=True)
out = s.mppi(256, STD, lam, smooth=SMOOTH, seed=1, adopt=False)
print("S 256: the weighted sequence is no worse than the base on %d of %d "
      "trajectories, cheaper than shoot's winner on %d; median effective "
      "sample size %.1f" % (
          int(out.improved.sum()), B, int((out.J_w < out.J_best).sum()),
          float(out.ess.median())))
