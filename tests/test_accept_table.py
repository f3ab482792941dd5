"""The stand-alone controller kernel (pddp_accept_f32 / _f64,
csrc/controller.hip + csrc/accept.hpp) against a decision table: one launch,
every trajectory of the batch one row of the table, every output compared
with tests/accept_model.py (the reference's rule, ilqr.py:140-181, :298-314,
:364-390) by equality - mu / delta as double bits, J_opt as bits of the run's
dtype - and the winner copy checked exactly through candidates that encode
their own index.

Axes of the table (accept_rows.py `table_rows`): sweep status x active mask x
cost pattern (where the minimum sits, ties, NaNs, +inf, J_new against J_opt to
the last bit, the convergence test on both sides of tol, J_opt <= 0) x
(mu, delta) (mu_min downward, delta on either side of 1, mu delta' against
max_reg from below / equal / above) x iter against n_iterations.
DESIGN.md 5."""

import numpy as np
import pytest
import torch

from accept_rows import bits, expected, MAX_REG, N_IT, SENT, table_rows, TOL
from golden_util import np_dtype

pytestmark = pytest.mark.gpu

TDT = {"f64": torch.float64, "f32": torch.float32}


def index_coded(shape, dt, sign=1.0, frac=0.0):
    """Every element its own flat index (+ 1 + frac), exact in float32."""
    size = int(np.prod(shape))
    assert size + 2 < 2 ** 23
    return (sign * (np.arange(size, dtype=np.float64) + 1.0 + frac)).astype(
        dt).reshape(shape)


def seed_inputs(rows, N, n, m, A, dtype):
    dt = np_dtype(dtype)
    B, gs = len(rows), m + m * n
    h = dict(
        Zc=index_coded((B, N + 1, A, n), dt),
        Uc=index_coded((B, N, A, m), dt, -1.0),
        gains=index_coded((B, N, gs), dt, 1.0, 0.5),
        Z=index_coded((B, N + 1, n), dt, -1.0, 0.25),
        U=index_coded((B, N, m), dt, 1.0, 0.25),
        gains_acc=index_coded((B, N, gs), dt, -1.0, 0.5),
        Jc=np.stack([r[3] for r in rows]).astype(dt),
        bwd_status=np.array([r[1] for r in rows], np.int32),
        active=np.array([r[0] for r in rows], np.uint8),
        J_opt=np.array([r[2] for r in rows], dt),
        mu=np.array([r[4] for r in rows], np.float64),
        delta=np.array([r[5] for r in rows], np.float64),
        iter=np.array([r[6] for r in rows], np.int32),
        state=np.zeros(B, np.int32), fresh=np.zeros(B, np.uint8))
    dead = h["active"] == 0
    for k, v in SENT.items():
        h[k][dead] = v
    h["Jc"][dead & (np.arange(B) % 2 == 0)] = np.nan
    return h


def check_outputs(got, h, e, tag):
    """Controller state against the model by equality; the copy exactly."""
    for k in ("state", "iter", "active", "fresh", "mu", "delta", "J_opt"):
        bad = np.flatnonzero(bits(got[k]) != bits(e[k]))
        assert bad.size == 0, (tag, k, bad[:8], got[k][bad[:8]], e[k][bad[:8]])
    amin = e["amin"]
    acc = np.flatnonzero(amin >= 0)
    rest = np.flatnonzero(amin < 0)
    assert acc.size and rest.size
    assert np.array_equal(got["Z"][acc], h["Zc"][acc, :, amin[acc]]), tag
    assert np.array_equal(got["U"][acc], h["Uc"][acc, :, amin[acc]]), tag
    assert np.array_equal(got["gains_acc"][acc], h["gains"][acc]), tag
    for k in ("Z", "U", "gains_acc"):
        assert np.array_equal(bits(got[k][rest]), bits(h[k][rest])), (tag, k)
    for k in ("Zc", "Uc", "Jc", "gains", "bwd_status"):   # inputs: untouched
        assert np.array_equal(bits(got[k]), bits(h[k])), (tag, k)


@pytest.mark.parametrize("N", [1, 17])
@pytest.mark.parametrize("A", [1, 10, 11, 16])
@pytest.mark.parametrize("n,m", [(4, 1), (6, 1), (8, 4)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_accept_kernel_against_the_table(dtype, n, m, A, N):
    """(4, 1): rows that divide the wavefront - the copy's whole-row path;
    (6, 1): 64 % 6 != 0 - its per-element path; (8, 4): the rendezvous'
    sizes.  Two launches on the same seeded inputs: n_live is a running
    total."""
    from pddp_amd import _native
    rows = table_rows(A, dtype)
    B = len(rows)
    h = seed_inputs(rows, N, n, m, A, dtype)
    e = expected(rows, dtype)
    dev = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
    n_live = torch.zeros(256, dtype=torch.int32, device="cuda")
    want_live = np.bincount(np.flatnonzero(e["active"] == 1) % 256,
                            minlength=256)
    p = _native.ptr
    for launch in (1, 2):
        for k, v in h.items():
            dev[k].copy_(torch.from_numpy(v))
        _native.call("pddp_accept", TDT[dtype], B, N, n, m, A, p(dev["Zc"]),
                     p(dev["Uc"]), p(dev["Jc"]), p(dev["gains"]),
                     p(dev["bwd_status"]), TOL, MAX_REG, N_IT, p(dev["Z"]),
                     p(dev["U"]), p(dev["gains_acc"]), p(dev["J_opt"]),
                     p(dev["mu"]), p(dev["delta"]), p(dev["state"]),
                     p(dev["iter"]), p(dev["active"]), p(dev["fresh"]),
                     p(n_live), _native.stream_handle())
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in dev.items()}
        check_outputs(got, h, e, (dtype, n, m, A, N, launch))
        assert np.array_equal(n_live.cpu().numpy(), launch * want_live), launch
