"""The matrix-core backward sweeps - on records (riccati_mfma16.hpp,
riccati_mfma32.hpp, riccati_mfma32s.hpp) and from the nominal
(riccati_mfma16_nominal.hpp) - against what the parent build computed
(DESIGN.md 3.2b): tests/golden/matrix_sweeps_parent.npz was recorded on an
MI355X by tools/record_sweep_golden.py from the build in which each of the four
kernels carried its own copy of the gain block and of the 16 x 16 step, and
every array of every case must still be the same bytes - the shared texts
perform the operations the copies performed.  Every variant (14, 15, 26, 27),
both gain branches, bounded and unbounded, f32 and f64, N = 1, 2, 3, 7 (records)
and 1, 70 (nominal), masks partly off; the inputs (clamped steps, a NaN, a
negative L_uu), the sentinels and which arrays are stored as digests of their
bytes are described at the tool."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "matrix_sweeps_parent.npz")

_spec = importlib.util.spec_from_file_location(
    "record_sweep_golden",
    os.path.join(ROOT, "tools", "record_sweep_golden.py"))
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
def test_matrix_core_sweeps_are_the_parents_byte_for_byte(golden, case):
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
            # entries that differ: values, or digests of (trajectory, step)
            bad.append((k, int((g.view(np.uint8).reshape(g.shape + (-1,)) !=
                                w.view(np.uint8).reshape(w.shape + (-1,)))
                               .any(axis=-1).sum())))
    assert not bad, "arrays that differ (name, entries): %r" % bad
