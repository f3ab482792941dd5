"""What a per-trajectory problem costs (ILQRSolver.set_batch_problem, the
batch_* kernels of csrc/problem_kernels.hip): cartpole f32, 4096 trajectories, horizon 100,
bounded, the fit's ten step sizes; every row of the table is the shared
problem, so both forms do the same work on the same buffers.

  - pddp_line_search_batch_f32 against pddp_line_search_f32 (the uniform
    entry point: nominal data staged in LDS), events attached to the dispatch
    itself (pddp_attach_events), the two alternating;
  - a whole round(): as the solver runs it by default (one launch), the
    uniform round on records with separate search and accept (the batch
    round's launch sequence with the uniform kernels), and the round with the
    table; pddp_event_record around each round.

  - with --against LIB, first of all: the six launches of the problem
    kernels (nominal rollout, records and the plain search - one lane per
    trajectory and step size -, each with one problem and with the table) in
    the loaded build (PDDP_HIP_LIB, else the tree's) and in the build LIB,
    alternating launch by launch on the same buffers, events attached to the
    dispatch itself.  A build holds its own if its median is not above the
    other's maximum over the same repetitions.

WARM warm-up launches, median of REPS:
    python tools/batch_problem_time.py [B] [--against LIB]"""
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
AGAINST = sys.argv[sys.argv.index("--against") + 1] \
    if "--against" in sys.argv else None
N, WARM, REPS = 100, 5, 20
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


def solver():
    prob = cartpole.CartpoleDynamicsModel(0.1).native_problem(
        StateEncoding.IGNORE_UNCERTAINTY, cartpole.CartpoleCost())
    s = ILQRSolver(prob, B, N, td, "cuda", torch.full((1,), -10.0, dtype=td),
                   torch.full((1,), 10.0, dtype=td))
    s._keep = prob
    return s


rng = np.random.RandomState(0)
z0 = torch.from_numpy(1e-2 * rng.randn(B, 4)).to(td).cuda()
U0 = torch.from_numpy(0.1 * rng.randn(B, N, 1)).to(td).cuda()

# -- the line search, kernel time -------------------------------------------
s = solver()
s.set_nominal(z0, U0)
s.derivs(set_state=False)
s.backward(reg=torch.full((B,), 1.0, dtype=torch.float64, device="cuda"))
assert int(s.bwd_status.abs().sum()) == 0
s.line_search()
Zc_uniform = s.Zc[:, :9].clone()
s.set_batch_problem()
s.line_search()
# the same work: the candidates' first steps agree to rounding (from these
# gains most of the 100-step rollouts leave the basin, and two roundings of a
# diverging rollout end anywhere: the costs themselves are not comparable)
dev = float((s.Zc[:, :9] - Zc_uniform).abs().max() / Zc_uniform.abs().max())
print("candidates, steps 0 .. 8: largest deviation %.2e of the largest entry"
      % dev)
assert dev < 2e-4
e0, e1 = event(), event()
table = s.batch_table

# -- the problem kernels, this build against another --------------------------
if AGAINST:
    other = ctypes.CDLL(AGAINST)
    p, st = _native.ptr, s._s()
    A17 = 17  # (above 16 step sizes the uniform entry point runs the plain kernel)
    al17 = torch.linspace(1.0, 0.01, A17).to(td).cuda()
    Zc17 = torch.empty(B, N + 1, A17, 4, dtype=td, device="cuda")
    Uc17 = torch.empty(B, N, A17, 1, dtype=td, device="cuda")
    Jc17 = torch.empty(B, A17, dtype=td, device="cuda")
    head = {"": (ctypes.addressof(s.problem),),
            "_batch": (ctypes.addressof(s.problem), p(table))}
    roll = (B, N, p(s.z0), p(s.U), p(s.u_min), p(s.u_max), None, p(s.Z), st)
    der = (B, N, p(s.Z), p(s.U), p(s.u_min), p(s.u_max), None, p(s._rec),
           p(s.L), p(s.J_opt), None, st)

    def search(A, al, Zc, Uc, Jc):
        return (B, N, A, p(s.Z), p(s.U), p(s.gains), p(al), p(s.u_min),
                p(s.u_max), None, p(s.bwd_status), p(Zc), p(Uc), p(Jc), st)

    for name, form, args in (
            ("pddp_nominal_rollout", "", roll), ("pddp_derivs", "", der),
            ("pddp_line_search", "", search(A17, al17, Zc17, Uc17, Jc17)),
            ("pddp_nominal_rollout", "_batch", roll),
            ("pddp_derivs", "_batch", der),
            ("pddp_line_search", "_batch",
             search(s.A, s.alphas, s.Zc, s.Uc, s.Jc))):
        ts = {"this": [], "other": []}
        for i in range(WARM + REPS):
            for build, l in (("this", lib), ("other", other)):
                fn = getattr(l, name + form + "_f32")
                fn.argtypes = _native._SIGS[name + form]
                l.pddp_attach_events.argtypes = [ctypes.c_void_p] * 2
                l.pddp_attach_events(e0, e1)
                _native.check(fn(*head[form], *args), name + form)
                t = elapsed_us(e0, e1)
                if i >= WARM:
                    ts[build].append(t)
        print("%s%s_f32%s, B %d N %d: this build %s; %s %s; %s" % (
            name, form, ", A %d" % args[2] if "search" in name else "", B, N,
            stats(ts["this"]), AGAINST, stats(ts["other"]),
            "holds" if np.median(ts["this"]) <= max(ts["other"])
            else "SLOWER"), flush=True)

times = {"uniform": [], "batch": []}
for i in range(WARM + REPS):
    for leg in ("uniform", "batch"):
        s.batch_table = table if leg == "batch" else None
        s._launch((e0, e1), s.line_search)
        t = elapsed_us(e0, e1)
        if i >= WARM:
            times[leg].append(t)
s.batch_table = table
tu, tb = np.median(times["uniform"]), np.median(times["batch"])
print("line search, B %d N %d A %d f32: pddp_line_search_f32 %s; "
      "pddp_line_search_batch_f32 %s; ratio %.2f" % (
          B, N, s.A, stats(times["uniform"]), stats(times["batch"]), tb / tu),
      flush=True)

# -- a whole round ------------------------------------------------------------
out = []
for leg in ("default (one launch)", "records+separate, uniform",
            "records+separate, table"):
    s = solver()
    if leg.endswith("uniform"):
        s._one_launch = s._nominal_sweep = s._fused = False
    if leg.endswith("table"):
        s.set_batch_problem()
    s.set_nominal(z0, U0)
    ts = []
    for i in range(WARM + REPS):
        _native.check(lib.pddp_event_record(e0, s._s()), "pddp_event_record")
        s.round(5e-6, 1e10, 1 << 30)  # (nobody leaves the loop)
        _native.check(lib.pddp_event_record(e1, s._s()), "pddp_event_record")
        t = elapsed_us(e0, e1)
        if i >= WARM:
            ts.append(t)
    assert s._plan(0) == ("one_launch" if leg.startswith("default")
                          else "records+separate"), leg
    out.append("%s %s (live %d)" % (leg, stats(ts), int(s.active.sum())))
print("round, B %d N %d f32: %s" % (B, N, "; ".join(out)), flush=True)
