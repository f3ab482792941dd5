"""Records what the one-launch round computes at the horizons around the
sweep's 16-step block - one block short by a step, exactly one, exactly two,
two and a step, three - with the sweep's own outputs (the gains) among the
arrays: the fixture of tests/test_round_block_golden.py, which holds later
builds to it byte for byte.  Record it from the build the change under test
STARTS from (its parent commit), on an MI355X, never from the code under test:

    python tools/record_round_block_golden.py [tests/golden/round_block_parent.npz]

(PDDP_HIP_LIB selects the library, pddp_amd/_native.py.)"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location(
    "record_round_golden", os.path.join(ROOT, "tools", "record_round_golden.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
case_name = base.case_name

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "round_block_parent.npz")

# (B, N, rounds per launch, some trajectories inactive).  B = 20: a ragged
# second workgroup.  One and three rounds per launch are two kernels.
CASES = [(B, N, R, False) for B in (16, 20) for N in (15, 16, 32, 33, 48)
         for R in (1, 3)] + [(16, 33, 3, True)]
ARRAYS = base.ARRAYS + ("gains_acc", "gains_k", "gains_K")


def run_case(B, N, R, inactive):
    """The existing fixture's arrays of one case and the sweep's outputs: the
    accepted gains and the API's views of the last sweep's."""
    import torch
    import bench
    made = []
    make = bench.make_cartpole_solver

    def keep(*a, **kw):
        out = make(*a, **kw)
        made.append(out[0])
        return out
    bench.make_cartpole_solver = keep
    try:
        got = base.run_case(B, N, R, inactive)
    finally:
        bench.make_cartpole_solver = make
    s = made[0]
    torch.cuda.synchronize()
    k, K = s.gain_views()
    for name, v in (("gains_acc", s.gains_acc), ("gains_k", k), ("gains_K", K)):
        got[name] = v.detach().cpu().numpy().copy()
    return got


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
