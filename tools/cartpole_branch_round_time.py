"""A round of the cartpole's fit loop in every gain branch (eig-clamp /
V_zz-regularised, bounded or not), four ways: on records (pddp_derivs +
sweep on records + fused search), sweep from the nominal + record-free search
(two launches), the one-launch round, and ten rounds per launch.  Every
repetition starts from the same nominal and runs the same rounds, so the legs
do the same work (their decisions are identical, tests/test_cartpole_branches
.py): python tools/cartpole_branch_round_time.py [B] [reps]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import pddp_amd
from pddp_amd.controllers.solver import ILQRSolver
from pddp_amd.examples import cartpole
from pddp_amd.utils.encoding import StateEncoding

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
N, WARM, K = 100, 10, 30
prob = cartpole.CartpoleDynamicsModel(0.1).native_problem(
    StateEncoding.IGNORE_UNCERTAINTY, cartpole.CartpoleCost())
rng = np.random.RandomState(0)
z0 = 1e-2 * rng.randn(B, 4)
U0 = 0.1 * rng.randn(B, N, 1)
LEGS = ("records", "two launches", "one launch", "ten rounds / launch")
for td in (torch.float32, torch.float64):
    for name, branch, bounded in (("eig-clamp bounded", 0, True),
                                  ("eig-clamp unbounded", 0, False),
                                  ("V_zz-reg unbounded", 1, False),
                                  ("V_zz-reg bounded", 1, True)):
        out = []
        for leg in LEGS[:2] if td == torch.float64 else LEGS:
            bnd = (torch.full((1,), -10.0, dtype=td),
                   torch.full((1,), 10.0, dtype=td)) if bounded else (None, None)
            s = ILQRSolver(prob, B, N, td, "cuda", bnd[0], bnd[1], branch=branch)
            s._nominal_sweep = False if leg == "records" else None
            if leg == "two launches":
                s._one_launch = False
            ts = []
            for rep in range(REPS):
                s.set_nominal(torch.from_numpy(z0).to(td).cuda(),
                              torch.from_numpy(U0).to(td).cuda())
                step = (lambda: s.rounds(10, 5e-6, 1e10, 1 << 30)) \
                    if leg == LEGS[3] else (lambda: s.round(5e-6, 1e10, 1 << 30))
                per = 10 if leg == LEGS[3] else 1
                for _ in range(WARM // per):
                    step()
                torch.cuda.synchronize()
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(K // per):
                    step()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) / K * 1e3)
            if leg != "records":
                assert s._nominal_sweep is True, leg
            if leg in LEGS[2:]:
                assert s._one_launch is True, leg
            ts = np.array(ts[1:])  # (the first repetition: caches, attributes)
            out.append("%s %.1f us [%.1f, %.1f]" % (
                leg, np.median(ts), ts.min(), ts.max()))
        print("%-20s %s B %d N %d live %d: %s" % (
            name, str(td).split(".")[-1], B, N, int(s.active.sum()),
            "; ".join(out)), flush=True)
