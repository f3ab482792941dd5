"""What a receding-horizon MPPI trial costs as ONE launch
(ILQRSolver.mppi_closed_loop, pddp_mppi_trial_f32 of csrc/mppi_trial.hip) next
to the same trial composed from the pieces that existed before it, and next to
iLQR MPC: cartpole f32, 4096 trajectories, horizon 100, bounded, base actions
0.1 randn, std 3, smooth 0.7, temperature 100, 50 control steps, S = 16, 64 and
256 candidates, K = 1 and 3 iterations per control step.

  (a) mppi_closed_loop(50, S, iterations=K): one launch for the whole trial;
  (b) the same trial in a host loop on preallocated buffers: per control step
      K pddp_mppi_f32 launches, each followed by its selects (took, and
      torch.where on U and Z), then one pddp_mpc_advance_f32;
  (c) one control step of mpc_closed_loop(1, rounds_per_step=3), for
      orientation.

One process, the legs alternating trial by trial, torch events around each
leg's whole host loop (so (b) includes its dispatch gaps: they are what the
single launch removes), WARM warm-up trials, median of REPS with [min, max],
reported per control step:
    python tools/mppi_trial_time.py [B]"""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from pddp_amd import _native
from pddp_amd.controllers.solver import ILQRSolver, mpc_alphas
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
r = ILQRSolver(prob, B, N, td, "cuda", *bounds,     # (c)
               alphas=mpc_alphas(td, "cuda"))
lam = torch.full((B,), LAM, **opts)
a_std = torch.full((1,), STD, **opts)
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


def trial_leg(S, K):
    def run():
        return s.mppi_closed_loop(T, S, STD, lam, iterations=K, smooth=SMOOTH,
                                  seed=1)
    return run


def composed_leg(S, K):
    J, Jw = torch.empty(B, S, **opts), torch.empty(B, **opts)
    best = torch.empty(B, dtype=torch.int32, device="cuda")
    Zw, Uw = torch.empty(B, N + 1, 4, **opts), torch.empty(B, N, 1, **opts)
    X, Ul = torch.empty(B, T + 1, 4, **opts), torch.empty(B, T, 1, **opts)
    Jcl = torch.empty(B, **opts)
    st = torch.empty(B, T, dtype=torch.int32, device="cuda")
    lv = torch.empty(B, T, dtype=torch.uint8, device="cuda")

    def run():
        for step in range(T):
            for k in range(K):
                _native.call("pddp_mppi", td, c._pp, B, N, S, p(c.z0), p(c.U),
                             p(c.u_min), p(c.u_max), p(a_std), p(lam), SMOOTH,
                             1, (step * K + k) * B * S, None, p(J), p(best),
                             None, None, p(Jw), p(Zw), p(Uw), c._s())
                take = (torch.isfinite(Jw) & (Jw <= J[:, 0])).reshape(B, 1, 1)
                torch.where(take, Uw, c.U, out=c.U)
                torch.where(take, Zw, c.Z, out=c.Z)
            _native.call("pddp_mpc_advance", td, c._pp, None, B, N, T, step,
                         p(c.z0), p(c.U), p(c.Z), p(c.u_min), p(c.u_max), None,
                         None, None, p(X), p(Ul), p(Jcl), p(st), p(lv),
                         p(c.mu), p(c.delta), p(c.state), p(c.iter),
                         p(c.active), p(c.fresh), p(c.n_live), c._s())
        return Jcl
    return run


def ilqr_leg():
    r.set_nominal(z0, U)
    t0.record()
    r.mpc_closed_loop(1, 3, z0=None)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 * T  # (stats() divides by T)


legs = {}
for S in (16, 64, 256):
    for K in (1, 3):
        legs["(a) one launch, S %d, K %d" % (S, K)] = timed(trial_leg(S, K))
        legs["(b) composed, S %d, K %d" % (S, K)] = timed(composed_leg(S, K))
legs["(c) iLQR MPC, 3 rounds"] = ilqr_leg

times = {k: [] for k in legs}
costs = {}
for i in range(WARM + REPS):
    for name, leg in legs.items():
        if name[1] in "ab":  # every trial from the same start
            s.z0.copy_(z0), s.U.copy_(U), c.z0.copy_(z0), c.U.copy_(U)
            c.nominal_rollout()
        t = leg()
        if i >= WARM:
            times[name].append(t)
        if name[1] == "a":
            costs[name] = float(leg.last.J.median())
        elif name[1] == "b":
            costs[name] = float(leg.last.median())
print("cartpole f32, B %d, N %d, %d control steps, bounded, std %g, smooth %g, "
      "temperature %g; %d warm-up trials, median of %d [min, max], per "
      "control step" % (B, N, T, STD, SMOOTH, LAM, WARM, REPS))
med = {k: np.median(v) for k, v in times.items()}
for name, ts in times.items():
    extra = ""
    if name[:3] == "(a)":
        other = "(b) composed, " + name.split(", ", 1)[1]
        extra = "; %.2f x (b), %.2f x (c); median trial cost %.4g (b: %.4g)" % (
            med[name] / med[other], med[name] / med["(c) iLQR MPC, 3 rounds"],
            costs[name], costs[other])
    print("%s: %s%s" % (name, stats(ts), extra), flush=True)
