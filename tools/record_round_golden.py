"""Records what the one-launch round (pddp_round_nominal_f32) computes at small
shapes, from bench.py's synthetic inputs: the fixture of
tests/test_round_rollout_golden.py, which holds later builds to it byte for
byte.  Record it from the build the change under test STARTS from (its parent
commit), on an MI355X, never from the code under test:

    python tools/record_round_golden.py [tests/golden/round_rollout_parent.npz]

(PDDP_HIP_LIB selects the library, pddp_amd/_native.py.)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "round_rollout_parent.npz")

# (B, N, rounds per launch, some trajectories inactive).  B = 20: a ragged
# second workgroup with one live pair.  N: the remainder loop of the rollout
# alone (1, 3), its four-step trip alone (4), both (5, 17), the benchmark's
# horizon (100).  One and three rounds per launch are two kernels.
CASES = [(B, N, R, False) for B in (16, 20) for N in (1, 3, 4, 5, 17, 100)
         for R in (1, 3)] + [(16, 17, 3, True)]
ARRAYS = ("Z", "U", "J_opt", "Jc", "full_step_rows", "mu", "delta", "state")


def case_name(B, N, R, inactive):
    return "B%d_N%d_R%d%s" % (B, N, R, "_inactive" if inactive else "")


def run_case(B, N, R, inactive):
    """The arrays of one case, as numpy, after R rounds in one launch."""
    import torch
    import bench
    s, z0, U, _ = bench.make_cartpole_solver(B, N, torch.float32, "cuda", 0, 0)
    s.set_nominal(z0, U)
    if inactive:
        s.active[1::3] = 0
    # (the full step's rows land in the first B (N + 1) 4 words of the record
    # buffer, which the one-launch round uses as scratch)
    s._rec.zero_()
    if R == 1:
        s.round(5e-6, 1e10, 1 << 30)
    else:
        s.rounds(R, 5e-6, 1e10, 1 << 30)
    torch.cuda.synchronize()
    assert s._one_launch is True, "the one-launch round did not apply"
    rows = s._rec.reshape(-1)[:B * (N + 1) * 4].reshape(B, N + 1, 4)
    out = {"Z": s.Z, "U": s.U, "J_opt": s.J_opt, "Jc": s.Jc,
           "full_step_rows": rows, "mu": s.mu, "delta": s.delta,
           "state": s.state}
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    blob = {}
    for case in CASES:
        got = run_case(*case)
        for k in ARRAYS:
            blob[case_name(*case) + "/" + k] = got[k]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **blob)
    print("%d cases, %d arrays, %d bytes -> %s" % (
        len(CASES), len(blob), os.path.getsize(out), out))


if __name__ == "__main__":
    main()
