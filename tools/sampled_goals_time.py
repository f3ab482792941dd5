"""What the line search's objective costs the sampling planners: each new form
(ILQRSolver.shoot / mppi / cem / mppi_closed_loop with objective="search"
along a reference, under per-trajectory weights, under both - the
*_goals_kernel of csrc/shoot.hip, csrc/mppi.hip, csrc/cem.hip,
csrc/mppi_trial.hip) next to its sibling
without either (the plain kernel of the same unit) ON THE SAME COMMIT: cartpole f32, 4096 trajectories, horizon 100,
bounded, base actions 0.1 randn, std 3, smooth 0.7, temperature 100,
S = 16, 64 and 256.  The reference has N + 1 + steps rows around the shared
goal, the weights are the shared diagonals x U(1, 2).

  shoot, mppi: one launch, adopt=False;
  cem: one launch, adopt=False, S / 4 elites, mix 0.25: the plain form, the
       _batch form (a table of the shared rows) and _track_weighted; mppi has
       a _batch row too, so that both ratios "both" / "batch" come from one run;
  trial: mppi_closed_loop(steps = 20, iterations = 3), time per control step.

The protocol of tools/mppi_time.py: one process, the legs alternating launch
by launch, events on the dispatch itself (pddp_attach_events), WARM warm-up
launches, median of REPS with [min, max]; the engine clock before and after
(rocm-smi, read only) printed with the result:
    python tools/sampled_goals_time.py [B] [shoot|mppi|cem|trial ...]"""
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
STEPS, K = 20, 3
KINDS = [a for a in sys.argv[1:] if not a.isdigit()] or \
    ["shoot", "mppi", "cem", "trial"]
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
na = prob.aug_size
x_goal = torch.tensor(list(prob.x_goal)[:na], dtype=td)
x_ref = x_goal + torch.from_numpy(
    rng.uniform(-0.5, 0.5, (B, N + 1 + STEPS, na))).to(td)
dq = torch.tensor([prob.Q[i * 8 + i] for i in range(na)], dtype=td)
dqt = torch.tensor([prob.Q_term[i * 8 + i] for i in range(na)], dtype=td)
dr = torch.tensor([prob.R[0]], dtype=td)
scale = lambda d: d * torch.from_numpy(
    rng.uniform(1.0, 2.0, (B, d.numel()))).to(td)


def solver(form):
    s = ILQRSolver(prob, B, N, td, "cuda", *bounds)
    s.set_nominal(z0, U)
    if form == "batch":
        s.set_batch_problem()
    if form in ("ref", "both"):
        s.set_reference(x_ref)
    if form in ("weights", "both"):
        s.set_batch_weights(q=scale(dq), q_term=scale(dqt), r=scale(dr),
                            keep_reference=form == "both")
    return s


FORMS = ("plain", "ref", "weights", "both")
solvers = {f: solver(f) for f in FORMS + ("batch",)}
lam = torch.full((B,), LAM, dtype=td, device="cuda")
e0, e1 = event(), event()


def leg(kind, form, S):
    s = solvers[form]
    kw = dict(smooth=SMOOTH, seed=1, events=(e0, e1), objective="search")

    def run():
        if kind == "shoot":
            s.shoot(S, STD, adopt=False, **kw)
        elif kind == "mppi":
            s.mppi(S, STD, lam, adopt=False, **kw)
        elif kind == "cem":
            s.cem(S, STD, S // 4, mix=0.25, adopt=False, **kw)
        else:
            if s.reference is not None:
                s.set_reference_start(0)
            s.mppi_closed_loop(STEPS, S, STD, lam, iterations=K, z0=z0, **kw)
            s.U.copy_(U)
            return elapsed_us(e0, e1) / STEPS
        return elapsed_us(e0, e1)
    return run


legs = {}
for kind in ("shoot", "mppi", "cem", "trial"):
    forms = {"mppi": FORMS + ("batch",), "cem": ("plain", "batch", "both")}
    for S in (16, 64, 256):
        for form in forms.get(kind, FORMS) if kind in KINDS else ():
            legs[(kind, S, form)] = leg(kind, form, S)

before = clock()
times = {k: [] for k in legs}
for i in range(WARM + REPS):
    for name, run in legs.items():
        t = run()
        if i >= WARM:
            times[name].append(t)
print("cartpole f32, B %d, N %d, bounded, std %g, smooth %g, temperature %g; "
      "trial: %d steps of %d iterations, per control step; %d warm-up "
      "launches, median of %d [min, max]" % (
          B, N, STD, SMOOTH, LAM, STEPS, K, WARM, REPS))
print("clock before: %s\nclock after:  %s" % (before, clock()))
med = {k: np.median(v) for k, v in times.items()}
for (kind, S, form), ts in times.items():
    extra = "" if form == "plain" else \
        "; %.2f x plain" % (med[kind, S, form] / med[kind, S, "plain"])
    if form == "both" and (kind, S, "batch") in med:
        extra += "; %.2f x batch" % (med[kind, S, form] / med[kind, S, "batch"])
    print("%s, S %d, %s: %s%s" % (kind, S, form, stats(ts), extra), flush=True)
