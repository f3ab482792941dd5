"""What the cross-entropy refit costs (ILQRSolver.cem, pddp_cem_f32 of
csrc/cem.hip) next to the softmin-weighted update on the same candidates
(ILQRSolver.mppi, pddp_mppi_f32 of csrc/mppi.hip, a unit this one leaves byte
for byte as it was): cartpole f32, 4096 trajectories, horizon 100, bounded,
base actions 0.1 randn, std 3, smooth 0.7, temperature 100, S = 64, 256 and
1024.

  (a) mppi(S, adopt=False): costs, argmin, the weights, the draws a second
      time with m sums per step, the weighted sequence rolled out;
  (b) cem(S, elites=S / 8, adopt=False): costs, the ranks, the elites' draws a
      second time with 2m sums per step, the refitted mean rolled out;
  (c) cem(S, elites=S): no candidate skips its draws in pass 3;
  (d) cem(S, elites=1): nearly all do;
  (e) shoot(S, adopt=False): pass 1 and the winner rolled out once more, for
      the scale of pass 1.
(c) - (d) is what the second draws of all candidates cost.  (c) and (a) both
make every draw twice over the same pass 1, so (c) - (a) is the ranking and
the m further sums per step, less mppi's argmin and eta: the tool prints both
differences.

The protocol of tools/mppi_time.py: one process, the legs alternating launch
by launch, events on the dispatch itself (pddp_attach_events), WARM warm-up
launches, median of REPS with [min, max]; the engine clock before and after
(rocm-smi, read only) printed with the result:
    python tools/cem_time.py [B]"""
import ctypes
import os
import subprocess
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
SAMPLES = (64, 256, 1024)
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


def clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True,
                             text=True, timeout=30).stdout
        return "; ".join(l.strip() for l in out.splitlines()
                         if "sclk" in l and "GPU[0]" in l) or "sclk: n/a"
    except (OSError, subprocess.SubprocessError):
        return "sclk: n/a"


prob = cartpole.CartpoleDynamicsModel(0.1).native_problem(
    StateEncoding.IGNORE_UNCERTAINTY, cartpole.CartpoleCost())
bounds = (torch.full((1,), -10.0, dtype=td), torch.full((1,), 10.0, dtype=td))
rng = np.random.RandomState(0)
z0 = torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda()
U = torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda()
s = ILQRSolver(prob, B, N, td, "cuda", *bounds)
s.set_nominal(z0, U)
lam = torch.full((B,), LAM, dtype=td, device="cuda")
sigma = torch.full((B, N, 1), STD, dtype=td, device="cuda")
e0, e1 = event(), event()


def mppi_leg(S):
    def run():
        s.mppi(S, STD, lam, smooth=SMOOTH, seed=1, adopt=False,
               events=(e0, e1))
        return elapsed_us(e0, e1)
    return run


def shoot_leg(S):
    def run():
        s.shoot(S, STD, smooth=SMOOTH, seed=1, adopt=False, events=(e0, e1))
        return elapsed_us(e0, e1)
    return run


def cem_leg(S, K):
    def run():
        s.cem(S, sigma, K, smooth=SMOOTH, seed=1, adopt=False,
              events=(e0, e1))
        return elapsed_us(e0, e1)
    return run


legs = {}
for S in SAMPLES:
    legs["(a) mppi, S %d" % S] = mppi_leg(S)
    legs["(b) cem K = S / 8, S %d" % S] = cem_leg(S, S // 8)
    legs["(c) cem K = S, S %d" % S] = cem_leg(S, S)
    legs["(d) cem K = 1, S %d" % S] = cem_leg(S, 1)
    legs["(e) shoot, S %d" % S] = shoot_leg(S)

before = clock()
times = {k: [] for k in legs}
for i in range(WARM + REPS):
    for name, leg in legs.items():
        t = leg()
        if i >= WARM:
            times[name].append(t)
after = clock()
print("cartpole f32, B %d, N %d, bounded, std %g, smooth %g, temperature %g; "
      "%d warm-up launches, median of %d [min, max]" % (
          B, N, STD, SMOOTH, LAM, WARM, REPS))
print("engine clock before: %s; after: %s" % (before, after))
med = {k: np.median(v) for k, v in times.items()}
for name, ts in times.items():
    extra = ""
    if name[:3] != "(a)":
        extra = "; %.2f x (a)" % (
            med[name] / med["(a) mppi, " + name.split(", ")[-1]])
    print("%s: %s%s" % (name, stats(ts), extra), flush=True)
for S in SAMPLES:
    a, c, d = (med["%s, S %d" % (k, S)] for k in (
        "(a) mppi", "(c) cem K = S", "(d) cem K = 1"))
    print("S %d: (c) - (d), every candidate's second draws, %.1f us; "
          "(c) - (a), the ranking and m more sums per step less mppi's argmin "
          "and eta, %.1f us" % (S, c - d, c - a), flush=True)
out = s.cem(256, sigma, 32, iterations=4, smooth=SMOOTH, seed=1, adopt=False)
print("S 256, K 32, four iterations: the incumbent is cheaper than the start "
      "on %d of %d trajectories; median cost %.3f -> %.3f; median width "
      "%.3f -> %.3f" % (
          int((out.J_trace[-1] < out.J_trace[0]).sum()), B,
          float(out.J_trace[0].median()), float(out.J_trace[-1].median()),
          STD, float(out.std.median())))
