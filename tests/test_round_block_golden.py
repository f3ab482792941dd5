"""The one-launch round at the horizons around the sweep's 16-step block,
against what its parent build computed:
tests/golden/round_block_parent.npz was recorded on an MI355X by
tools/record_round_block_golden.py from the build BEFORE the chains' waits and
the sweep's block boundary were touched, and every array of every case must
still be the same bytes.  The horizons give one block short by a step, exactly
one block, exactly two, two and a step, and three; the arrays are those of
tests/test_round_rollout_golden.py and the sweep's own outputs, the gains."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "round_block_parent.npz")

_spec = importlib.util.spec_from_file_location(
    "record_round_block_golden",
    os.path.join(ROOT, "tools", "record_round_block_golden.py"))
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
def test_round_blocks_are_the_parents_byte_for_byte(golden, case):
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
