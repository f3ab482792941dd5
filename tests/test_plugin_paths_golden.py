"""The plugin path (controllers/plugin.py TorchProblem) through every one of
its paths - BNN kernels, GP kernels, QR-cost kernel, generic autograd -
against what the parent build computed:
tests/golden/plugin_paths_parent.npz was recorded on an MI355X by
tools/record_plugin_golden.py from the build in which the path decision was
re-derived in `rollout`, `derivs`, `line_search` and `capture_ok`, the ctypes
structures were filled in four copies and the first particles drawn in two;
every array of every case must still be the same bytes, `last_derivs_path`
included.  The cases, the inputs, the sentinel and which arrays are stored as
digests of their bytes are described at the tool."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plugin_paths_parent.npz")

_spec = importlib.util.spec_from_file_location(
    "record_plugin_golden",
    os.path.join(ROOT, "tools", "record_plugin_golden.py"))
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
        blob = {k: f[k] for k in f.files}
    # (the weights, the masks and the normals are torch's draws)
    version = str(blob.pop("torch_version"))
    if version != torch.__version__:
        pytest.skip("recorded under torch %s, this is %s" % (
            version, torch.__version__))
    return blob


@pytest.mark.gpu
@pytest.mark.parametrize("case", rec.CASES, ids=lambda c: rec.case_name(*c))
def test_plugin_paths_are_the_parents_byte_for_byte(golden, case):
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
            # entries that differ: values, or digests of trajectories
            bad.append((k, int((np.atleast_1d(g) != np.atleast_1d(w)).sum())))
    assert not bad, "arrays that differ (name, entries): %r" % bad
