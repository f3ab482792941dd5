"""What a receding-horizon CEM trial costs as ONE launch
(ILQRSolver.cem_closed_loop, pddp_cem_trial_f32 of csrc/cem_trial.hip) next to
the same trial composed from the pieces that existed before it, and next to the
MPPI trial: cartpole f32, 4096 trajectories, horizon 100, bounded, base actions
0.1 randn, width 3 everywhere, smooth 0.7, mix 0, every control step restarting
from that width, 50 control steps, S = 64 and 256 candidates, K = S / 8 elites,
I = 1 and 3 iterations per control step.

  (a) cem_closed_loop(50, S, 3.0, S / 8, iterations=I): one launch for the
      whole trial;
  (b) the same trial in a host loop on preallocated buffers: per control step
      I pddp_cem_f32 launches, each followed by cem's five selects (torch.where
      on the incumbent's U and Z, on the carried cost, on the mean and on the
      width), then one pddp_mpc_advance_f32;
  (c) mppi_closed_loop(50, S, 3.0, 100.0, iterations=I), for orientation.

One process, the legs alternating trial by trial, torch events around each
leg's whole host loop (so (b) includes its dispatch gaps: they are what the
single launch removes), WARM warm-up trials, median of REPS with [min, max],
reported per control step:
    python tools/cem_trial_time.py [B]"""
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
N, T, WARM, REPS, STD, SMOOTH, LAM = 100, 50, 2, 7, 3.0, 0.7, 100.0
td = torch.float32
opts = dict(dtype=td, device="cuda")


def stats(ts):
    ts = np.array(ts) / T
    return "%.1f us [%.1f, %.1f]" % (np.median(ts), ts.min(), ts.max())


prob = cartpole.CartpoleDynamicsModel(0.1).native_problem(
    StateEncoding.IGNORE_UNCERTAINTY, cartpole.CartpoleCost())
bounds = (torch.full((1,), -10.0, dtype=td), torch.full((1,), 10.0, dtype=td))
rng = np.random.RandomState(0)
z0 = torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda()
U = torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda()
s = ILQRSolver(prob, B, N, td, "cuda", *bounds)     # (a)
c = ILQRSolver(prob, B, N, td, "cuda", *bounds)     # (b)
r = ILQRSolver(prob, B, N, td, "cuda", *bounds)     # (c)
lam = torch.full((B,), LAM, **opts)
width = torch.full((B, N, 1), STD, **opts)
t0, t1 = torch.cuda.Event(enable_timing=True), \
    torch.cuda.Event(enable_timing=True)
p = _native.ptr


def timed(fn):
    def run():
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        run.last = out
        return t0.elapsed_time(t1) * 1e3
    return run


def trial_leg(S, I):
    def run():
        return s.cem_closed_loop(T, S, width, S // 8, iterations=I,
                                 smooth=SMOOTH, seed=1).J
    return run


def composed_leg(S, I):
    K = S // 8
    J, Jm = torch.empty(B, S, **opts), torch.empty(B, **opts)
    best = torch.empty(B, dtype=torch.int32, device="cuda")
    ne = torch.empty(B, dtype=torch.int32, device="cuda")
    Zm, Um = torch.empty(B, N + 1, 4, **opts), torch.empty(B, N, 1, **opts)
    Sm, mean = torch.empty(B, N, 1, **opts), torch.empty(B, N, 1, **opts)
    sigma, Jinc = torch.empty(B, N, 1, **opts), torch.empty(B, **opts)
    X, Ul = torch.empty(B, T + 1, 4, **opts), torch.empty(B, T, 1, **opts)
    Jcl = torch.empty(B, **opts)
    st = torch.empty(B, T, dtype=torch.int32, device="cuda")
    lv = torch.empty(B, T, dtype=torch.uint8, device="cuda")

    def run():
        for step in range(T):
            mean.copy_(c.U)
            sigma.copy_(width)
            for k in range(I):
                _native.call("pddp_cem", td, c._pp, B, N, S, K, p(c.z0),
                             p(mean), p(c.u_min), p(c.u_max), p(sigma), None,
                             SMOOTH, 0.0, 1, (step * I + k) * B * S, None,
                             p(J), None, p(best), None, p(ne), p(Jm), p(Zm),
                             p(Um), p(Sm), c._s())
                if k == 0:
                    Jinc.copy_(J[:, 0])
                better = torch.isfinite(Jm) & (Jm <= Jinc)
                take = better.reshape(B, 1, 1)
                torch.where(take, Um, c.U, out=c.U)
                torch.where(take, Zm, c.Z, out=c.Z)
                torch.where(better, Jm, Jinc, out=Jinc)
                moved = (ne > 0).reshape(B, 1, 1)
                torch.where(moved, Um, mean, out=mean)
                torch.where(moved, Sm, sigma, out=sigma)
            _native.call("pddp_mpc_advance", td, c._pp, None, B, N, T, step,
                         p(c.z0), p(c.U), p(c.Z), p(c.u_min), p(c.u_max), None,
                         None, None, p(X), p(Ul), p(Jcl), p(st), p(lv),
                         p(c.mu), p(c.delta), p(c.state), p(c.iter),
                         p(c.active), p(c.fresh), p(c.n_live), c._s())
        return Jcl
    return run


def mppi_leg(S, I):
    def run():
        return r.mppi_closed_loop(T, S, STD, lam, iterations=I, smooth=SMOOTH,
                                  seed=1).J
    return run


legs = {}
for S in (64, 256):
    for I in (1, 3):
        tail = "S %d, I %d" % (S, I)
        legs["(a) one launch, " + tail] = timed(trial_leg(S, I))
        legs["(b) composed, " + tail] = timed(composed_leg(S, I))
        legs["(c) MPPI trial, " + tail] = timed(mppi_leg(S, I))

times = {k: [] for k in legs}
costs = {}
for i in range(WARM + REPS):
    for name, leg in legs.items():
        for x in (s, c, r):  # every trial from the same start
            x.z0.copy_(z0), x.U.copy_(U)
        c.nominal_rollout()
        t = leg()
        if i >= WARM:
            times[name].append(t)
        costs[name] = float(leg.last.median())
print("cartpole f32, B %d, N %d, %d control steps, bounded, width %g, smooth "
      "%g, mix 0, K = S / 8; %d warm-up trials, median of %d [min, max], per "
      "control step" % (B, N, T, STD, SMOOTH, WARM, REPS))
med = {k: np.median(v) for k, v in times.items()}
for name, ts in times.items():
    extra = ""
    if name[:3] == "(a)":
        tail = name.split(", ", 1)[1]
        extra = "; %.2f x (b), %.2f x (c); median trial cost %.4g (b: %.4g, " \
            "c: %.4g)" % (med[name] / med["(b) composed, " + tail],
                          med[name] / med["(c) MPPI trial, " + tail],
                          costs[name], costs["(b) composed, " + tail],
                          costs["(c) MPPI trial, " + tail])
    print("%s: %s%s" % (name, stats(ts), extra), flush=True)
