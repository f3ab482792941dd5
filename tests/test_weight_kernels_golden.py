"""The records and the line search under per-trajectory cost weights, with one
goal per trajectory and along a MOVING reference, against what the parent build
computed: tests/golden/weight_kernels_parent.npz was recorded
on an MI355X by tools/record_weight_golden.py from the build in which
weights.hip and track_weights.hip were translation units of their own with
their own launchers, impls and entry points, and every array of every case must
still be the same bytes - the one unit and the one host path launch the kernels
those units launched, with the arguments they passed.  All four sample models,
f32 and f64, bounded and unbounded, with and without a table; the shapes, the
masks, the weights and the sentinel are described at the tool, which also says
which arrays are stored as digests of their bytes."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "weight_kernels_parent.npz")

_spec = importlib.util.spec_from_file_location(
    "record_weight_golden",
    os.path.join(ROOT, "tools", "record_weight_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    import torch
    # (the bytes are gfx950's: another chip's contractions may differ)
    arch = torch.cuda.get_device_properties(0).gcnArchName
    if not arch.startswith("gfx950"):
        pytest.skip("recorded on gfx950, this is " + arch)
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.gpu
@pytest.mark.parametrize("case", rec.CASES, ids=lambda c: rec.case_name(*c))
def test_weight_kernels_are_the_parents_byte_for_byte(golden, case):
    got = rec.run_case(*case)
    prefix = rec.case_name(*case) + "/"
    want = {k[len(prefix):]: v for k, v in golden.items()
            if k.startswith(prefix)}
    assert sorted(got) == sorted(want)
    bad = []
    for k, w in want.items():
        g = got[k]
        if g.dtype != w.dtype or g.shape != w.shape:
            bad.append((k, -1))
        elif g.tobytes() != w.tobytes():
            # entries that differ: values, or digests of rows
            bad.append((k, int((g.view(np.uint8).reshape(g.shape + (-1,)) !=
                                w.view(np.uint8).reshape(w.shape + (-1,)))
                               .any(axis=-1).sum())))
    assert not bad, "arrays that differ (name, entries): %r" % bad
