"""The cross-entropy planners - pddp_cem_* in all five forms and
pddp_cem_trial_* - against what the parent build computed:
tests/golden/cem_kernels_parent.npz was recorded on an MI355X by
tools/record_cem_golden.py from the build in which cem_kernel_body.inc and
cem_trial_kernel_body.inc each had their own copy of the ranking and the refit,
and the two trial bodies each their own plant section and closing rollout, and
every array of every case must still be the same bytes.  All four sample
models, f32 and f64, bounded and unbounded; the shapes, the options of each
launch, the masks and the sentinel are described at the tool, which also says
which arrays are stored as digests of their bytes."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cem_kernels_parent.npz")

_spec = importlib.util.spec_from_file_location(
    "record_cem_golden", os.path.join(ROOT, "tools", "record_cem_golden.py"))
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
def test_cem_kernels_are_the_parents_byte_for_byte(golden, case):
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
