"""The stand-alone controller kernel (pddp_accept_f32 / _f64,
csrc/controller.hip + csrc/accept.hpp) against a decision table: one launch,
every trajectory of the batch one row of the table, every output compared
with tests/accept_model.py (the reference's rule, ilqr.py:140-181, :298-314,
:364-390) by equality - mu / delta as double bits, J_opt as bits of the run's
dtype - and the winner copy checked exactly through candidates that encode
their own index.

Axes of the table (`table_rows`): sweep status x active mask x cost pattern
(where the minimum sits, ties, NaNs, +inf, J_new against J_opt to the last
bit, the convergence test on both sides of tol, J_opt <= 0) x (mu, delta)
(mu_min downward, delta on either side of 1, mu delta' against max_reg from
below / equal / above) x iter against n_iterations.  DESIGN.md 5."""
import functools

import numpy as np
import pytest
import torch

import accept_model as am
from golden_util import np_dtype

pytestmark = pytest.mark.gpu

TDT = {"f64": torch.float64, "f32": torch.float32}
TOL, MAX_REG, N_IT = 5e-6, 150.0, 5
_M = 37.5  # 37.5 * (2 * 2) == MAX_REG exactly

# (mu, delta) before the attempt
REG_ROWS = [
    (0.0, 2.0),
    (1e-6, 4.0),
    (2e-6, 2.0),                      # a decrease lands on mu_min: mu -> 0
    (float(np.nextafter(2e-6, 1.0)), 2.0),   # ... just above it: stays
    (1.0, 0.25),                      # an increase: max(1, delta) * 2
    (1.0, 8.0),                       # a decrease: min(1, delta) / 2
    (float(np.nextafter(_M, 0.0)), 2.0),     # an increase ends below max_reg
    (_M, 2.0),                        # ... on it: MAX_REG (>=)
    (float(np.nextafter(_M, 1e3)), 2.0),     # ... above it
    (100.0, 2.0),
]
ITER_ROWS = [1, N_IT - 1, N_IT]


def tol_edge(J_opt, dt):
    """(J_under, J_over): neighbouring costs below `J_opt` whose improvement
    is just under tol (CONVERGED) and just over it (ACCEPTED) as the model
    evaluates the test in `dt`."""
    kw = dict(bwd_status=0, mu=0.0, delta=2.0, iter=1, tol=TOL, max_reg=1e10,
              n_iterations=N_IT, dtype=dt)
    J = dt(dt(J_opt) * dt(1.0 - TOL))
    conv = lambda x: am.attempt(J_opt, [x], **kw).state == am.CONVERGED
    for _ in range(4096):
        if not conv(J):
            J = np.nextafter(J, dt(np.inf))
        elif conv(np.nextafter(J, dt(-np.inf))):
            J = np.nextafter(J, dt(-np.inf))
        else:
            over = np.nextafter(J, dt(-np.inf))
            assert J < dt(J_opt) and conv(J) and not conv(over)
            return J, over
    raise AssertionError("no edge of the convergence test near %r" % J_opt)


def cost_patterns(A, dt):
    """[(name, J_opt, Jc[A])] - the nominal's cost is 10 and every candidate
    that is not part of the pattern costs 20 + its index (worse, distinct)."""
    nan, inf = dt(np.nan), dt(np.inf)
    base = lambda: (20 + np.arange(A)).astype(dt)
    out = []

    def add(name, edits, J_opt=10.0):
        Jc = base()
        for i, v in edits.items():
            Jc[i] = v
        out.append((name, dt(J_opt), Jc))

    add("min_first", {0: 5})
    add("none_better", {})
    add("all_inf", {i: inf for i in range(A)})
    add("equal", {A - 1: 10})                       # not <: REJECTED
    add("one_ulp", {A - 1: np.nextafter(dt(10), -inf)})   # CONVERGED
    under, over = tol_edge(10.0, dt)
    add("under_tol", {A // 2: under})
    add("over_tol", {A // 2: over})
    add("negative", {0: -3}, J_opt=-1.0)            # rel < 0: CONVERGED
    add("zero", {A - 1: -1}, J_opt=0.0)             # rel = inf: ACCEPTED
    add("from_inf", {0: 5}, J_opt=inf)              # rel = nan: ACCEPTED
    add("nan_only_first", {0: nan})
    if A >= 2:
        add("min_last", {A - 1: 5})
        add("tie_ends", {0: 5, A - 1: 5})
        add("nan_first", {0: nan, 1: 4})
        add("nan_last", {A - 2: 4, A - 1: nan})
    if A >= 3:
        p = A // 2
        add("min_middle", {p: 5})
        add("tie_inner", {A // 3: 5, A - 1: 5})
        add("tie_three", {1: 5, p: 5, A - 1: 5})
        add("nan_between", {p - 1: 5, p: nan, p + 1: 4})
        add("two_nans", {A // 3: nan, A // 3 + 1: 4, A - 1: nan})
    return out


@functools.lru_cache(maxsize=None)
def table_rows(A, dtype):
    """The cross product, pruned: every cost pattern with every (mu, delta),
    with every iter, with a failed sweep and as an inactive row; a failed sweep
    with every (mu, delta) x iter.  [(active, bwd_status, J_opt, Jc, mu, delta,
    iter)], then cycled up to a batch beyond 256 that is no multiple of 16."""
    dt = np_dtype(dtype)
    pats = cost_patterns(A, dt)
    rows = []
    for i, (_, J_opt, Jc) in enumerate(pats):
        for j, (mu, delta) in enumerate(REG_ROWS):
            rows.append((1, 0, J_opt, Jc, mu, delta,
                         ITER_ROWS[(i + j) % 3]))
        for k, it in enumerate(ITER_ROWS):
            mu, delta = REG_ROWS[(i + k) % len(REG_ROWS)]
            rows.append((1, 0, J_opt, Jc, mu, delta, it))
        mu, delta = REG_ROWS[i % len(REG_ROWS)]
        rows.append((1, 5, J_opt, Jc, mu, delta, ITER_ROWS[i % 3]))
        rows.append((0, 0, J_opt, Jc, mu, delta, ITER_ROWS[i % 3]))
        rows.append((0, -1, J_opt, Jc, mu, delta, ITER_ROWS[(i + 1) % 3]))
    for mu, delta in REG_ROWS:
        for it in ITER_ROWS:
            rows.append((1, -1 if it == 1 else 2,
                         pats[0][1], pats[0][2], mu, delta, it))
    # spread the kinds over the batch, then fill up
    order = np.random.RandomState(A).permutation(len(rows))
    rows = [rows[i] for i in order]
    B = max(len(rows), 257)
    B += (5 - B) % 16            # B % 16 == 5
    assert B > 256 and B % 16
    return [rows[i % len(rows)] for i in range(B)]


SENT = dict(state=-7, iter=-3, mu=123.25, delta=-0.5, J_opt=-77.5, fresh=3)


def expected(rows, dtype):
    """The model, row by row -> dict of arrays (inactive rows: the sentinels
    they were seeded with) + amin [B]."""
    dt = np_dtype(dtype)
    B = len(rows)
    e = dict(state=np.zeros(B, np.int32), iter=np.zeros(B, np.int32),
             mu=np.zeros(B, np.float64), delta=np.zeros(B, np.float64),
             J_opt=np.zeros(B, dt), active=np.zeros(B, np.uint8),
             fresh=np.zeros(B, np.uint8), amin=np.full(B, -1, np.int64))
    for b, (act, st, J_opt, Jc, mu, delta, it) in enumerate(rows):
        if not act:
            for k, v in SENT.items():
                e[k][b] = v
            continue
        r = am.attempt(J_opt, Jc, st, mu, delta, it, TOL, MAX_REG, N_IT, dt)
        e["state"][b], e["iter"][b] = r.state, r.iter
        e["mu"][b], e["delta"][b], e["J_opt"][b] = r.mu, r.delta, r.J_opt
        e["active"][b], e["fresh"][b], e["amin"][b] = r.active, r.fresh, r.amin
    return e


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.itemsize]) \
        if a.dtype.kind == "f" else a


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
