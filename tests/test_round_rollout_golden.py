"""The one-launch round against what its parent build computed (DESIGN.md
3.5b, round 9): tests/golden/round_rollout_parent.npz was recorded on an MI355X
by tools/record_round_golden.py from the build BEFORE the rollout step was
reordered, and every array of every case must still be the same bytes - the
step performs the operations it performed, with the same contractions, in
another order of issue.  The cases run the rollout's remainder loop alone, its
four-step trip alone, both, the benchmark's horizon, a ragged last workgroup,
one and three rounds per launch, and a batch with inactive trajectories."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "round_rollout_parent.npz")

_spec = importlib.util.spec_from_file_location(
    "record_round_golden", os.path.join(ROOT, "tools", "record_round_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    import torch
    # (the bytes are gfx950's: another chip's f32 contractions may differ)
    arch = torch.cuda.get_device_properties(0).gcnArchName
    if not arch.startswith("gfx950"):
        pytest.skip("recorded on gfx950, this is " + arch)
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.gpu
@pytest.mark.parametrize("case", rec.CASES, ids=lambda c: rec.case_name(*c))
def test_round_is_the_parents_byte_for_byte(golden, case):
    got = rec.run_case(*case)
    bad = []
    for k in rec.ARRAYS:
        want = golden[rec.case_name(*case) + "/" + k]
        g = got[k]
        if g.dtype != want.dtype or g.shape != want.shape or \
                g.tobytes() != want.tobytes():
            n = int((g.view(np.uint8) != want.view(np.uint8)).sum()) \
                if g.shape == want.shape and g.dtype == want.dtype else -1
            bad.append((k, n))
    assert not bad, "arrays that differ (name, bytes): %r" % bad
