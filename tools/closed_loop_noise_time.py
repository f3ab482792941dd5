"""What noise drawn inside the closed-loop rollouts costs
(ILQRSolver.closed_loop(process_std=, obs_std=), pddp_closed_loop_noisy_f32 of
csrc/closed_loop.hip) next to the noise-free launch and next to merely
filling the tensor the alternative design - a disturbance argument - would have
read: cartpole f32, 4096 trajectories, horizon 100, bounded, the gains of one
sweep at reg = 1, every plant row the shared problem, starts Z[b][0] +
U(-0.05, 0.05), S = 16 and 64, costs only and with the trajectories kept.

  (a) pddp_closed_loop_f32;
  (b) process noise, std 0.02;
  (c) process and measurement noise, std 0.02 each;
  (d) torch.randn(B, S, N, n) alone, on the same stream.

The protocol of tools/closed_loop_time.py: one process, the legs alternating
launch by launch, events on the dispatch itself (pddp_attach_events; torch
events around (d), which is not the library's launch), WARM warm-up launches,
median of REPS with [min, max]:
    python tools/closed_loop_noise_time.py [B]"""
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
N, WARM, REPS, STD = 100, 5, 20, 0.02
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
               torch.full((1,), 10.0, dtype=td))
rng = np.random.RandomState(0)
s.set_nominal(torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda(),
              torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda())
s.derivs(set_state=False)
s.backward(reg=torch.full((B,), 1.0, dtype=torch.float64, device="cuda"))
assert int(s.bwd_status.abs().sum()) == 0
s.set_batch_problem()  # (every row the shared problem)
e0, e1 = event(), event()
t0, t1 = torch.cuda.Event(enable_timing=True), \
    torch.cuda.Event(enable_timing=True)
std = torch.full((4,), STD, dtype=td, device="cuda")


def library_leg(**kw):
    def run():
        s.closed_loop(accepted=False, events=(e0, e1), **kw)
        return elapsed_us(e0, e1)
    return run


def randn_leg(S):
    def run():  # (the solver's stream is torch's current one)
        t0.record()
        torch.randn(B, S, N, 4, dtype=td, device="cuda")
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3
    return run


legs = {}
for S in (16, 64):
    z0 = (s.Z[:, :1] + torch.from_numpy(rng.uniform(
        -0.05, 0.05, (B, S, 4))).to(td).cuda()).contiguous()
    for keep in (False, True):
        tag = "S %d, %s" % (S, "kept" if keep else "costs only")
        legs["(a) plain, " + tag] = library_leg(z0=z0, keep=keep)
        legs["(b) process noise, " + tag] = library_leg(
            z0=z0, keep=keep, process_std=std, seed=1)
        legs["(c) process + measurement noise, " + tag] = library_leg(
            z0=z0, keep=keep, process_std=std, obs_std=std, seed=1)
    legs["(d) torch.randn(B, S, N, n) alone, S %d" % S] = randn_leg(S)

times = {k: [] for k in legs}
for i in range(WARM + REPS):
    for name, leg in legs.items():
        t = leg()
        if i >= WARM:
            times[name].append(t)
print("cartpole f32, B %d, N %d, bounded, std %g; %d warm-up launches, median "
      "of %d [min, max]" % (B, N, STD, WARM, REPS))
med = {k: np.median(v) for k, v in times.items()}
for name, ts in times.items():
    extra = ""
    if name[:3] in ("(b)", "(c)"):
        base = med["(a) plain, " + name.split(", ", 1)[1]]
        extra = "; %+.1f us over (a), %.2f x" % (med[name] - base,
                                                med[name] / base)
    print("%s: %s%s" % (name, stats(ts), extra), flush=True)
