"""The decision table of the accept step: every (cost pattern, mu, delta,
iter, sweep status, mask) row the accept kernels are asked, and what
accept_model.attempt says of each.  Shared by test_accept_table.py,
test_accept_fused_table.py and test_accept_model.py."""
import functools

import numpy as np

import accept_model as am
from golden_util import np_dtype

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
            assert J < dt(J_opt) and conv(J) and not conv(over), \
                ("not the edge of the convergence test", J_opt, J, over)
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
    assert B > 256 and B % 16, ("batch of the decision table", A, dtype, B)
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
