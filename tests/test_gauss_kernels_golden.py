"""The kernels of the Gaussian state encodings - pddp_qr_cost_derivs_*, the
rollout, the records and the line search under the four Gaussian encodings,
pddp_bnn_jvp_moments_* - against what the parent build computed (DESIGN.md
3.9a): tests/golden/gauss_kernels_parent.npz was recorded on an MI355X by
tools/record_gauss_golden.py from the build in which the hyper-dual numbers
existed twice, the scalar overloads five times and the cost on the augmented
moments once per unit; every array of every case must still be the same bytes.
The shapes, the inputs, the sentinel and which arrays are stored as digests of
their bytes are described at the tool.

A CPU test holds the tool's states to what it says of them: with
tests/qr_cost_model.py's Cholesky in the run's own number format, every qr case
has a state on the first rung of the jitter ladder, and every case with two
non-angular dimensions one on a higher rung and one for which no rung
succeeds."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import qr_cost_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gauss_kernels_parent.npz")

_spec = importlib.util.spec_from_file_location(
    "record_gauss_golden",
    os.path.join(ROOT, "tools", "record_gauss_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


def rungs_of(Z, D, ang, dtype):
    """The rung of each encoded state [count, n] (None: the fall-back), the
    augmented covariance evaluated and factorised in `dtype`."""
    tdt, ndt = ((torch.float32, np.float32) if dtype == "f32"
                else (torch.float64, np.float64))
    _, Ca = qm.moments(torch.from_numpy(Z).to(tdt), D, list(ang),
                       qm.non_angular(D, ang), exact=False)
    return [qm.rung(a, ndt) for a in Ca.numpy()]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_recorded_states_reach_the_rungs_they_are_chosen_for(dtype):
    first = qm.ladder()[0]
    for idx, (D, ang) in enumerate(rec.QR_SHAPES):
        Z = rec.encoded(*rec.qr_states(D, ang, dtype, 300 + idx))
        r = rungs_of(Z, D, ang, dtype)
        assert first in r, (D, ang, r)
        if D - len(ang) >= 2:
            assert r[2] is not None and r[2] > first, (D, ang, r)
            assert r[5] is None, (D, ang, r)
    for k, problem in enumerate(rec.base.PROBLEMS):
        from pddp_amd.examples.problems import SampleProblems
        mc = SampleProblems[problem.upper()].get_model_class()
        D = mc.state_size
        ang = tuple(int(i) for i in mc.angular_indices)
        if D - len(ang) < 2:
            continue
        N = rec.PB_N
        Z = rec.encoded(*rec.problem_states(
            problem, dtype, 2 * (N + 1), 501 + 10 * k, climb=N + 2,
            fallback=N))
        r = rungs_of(Z, D, ang, dtype)
        assert r[N + 2] is not None and r[N + 2] > first, (problem, r)
        assert r[N] is None, (problem, r)


@pytest.fixture(scope="module")
def golden():
    # (the bytes are gfx950's: another chip's contractions may differ)
    arch = torch.cuda.get_device_properties(0).gcnArchName
    if not arch.startswith("gfx950"):
        pytest.skip("recorded on gfx950, this is " + arch)
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.gpu
@pytest.mark.parametrize("case", rec.CASES, ids=lambda c: rec.case_name(*c))
def test_gauss_kernels_are_the_parents_byte_for_byte(golden, case):
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
