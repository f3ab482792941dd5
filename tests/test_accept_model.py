"""tests/accept_model.py - the plain restatement of one attempt that the
decision-table tests judge the HIP controller by - held to two sources that
were not written from it:

  a. the C oracle's `fit` traces (oracle/pddp_oracle_impl.inc), replayed row by
     row through the model's schedule and masks;
  b. tests/golden/accept_schedule.npz: the reference controller's own
     `_reset_reg` / `_increase_reg` / `_decrease_reg` recorded over seeded
     random call sequences (tools/make_golden.py --accept-schedule).

Every comparison is an equality of doubles / integers.  CPU only."""
import os

import numpy as np
import pytest
import torch

import accept_model as am
import oracle as orc
from golden_util import GOLDEN_DIR

# (bounded, max_reg, n_iterations)
ORACLE_CONFIGS = [(False, 30.0, 50), (True, 1e-3, 50), (True, 0.2, 50),
                  (True, 1e10, 3)]
TOL = 5e-6


def _oracle_traces(bounded, max_reg, n_it):
    B, N = 24, 16
    rng = np.random.RandomState(4)
    z0 = (1e-2 * rng.randn(B, 4)).astype(np.float32)
    U = (0.1 * rng.randn(B, N, 1)).astype(np.float32)
    alphas = (1.025 ** (-torch.arange(10.0) ** 2).to(torch.float32)).numpy()
    o = orc.load(np.float32)
    op = orc.make_problem("cartpole", 0.1)
    kw = dict(u_min=np.float32([-10.0]), u_max=np.float32([10.0])) \
        if bounded else {}
    out = []
    for b in range(B):
        _, _, _, state, trace = o.fit(op, z0[b], U[b], alphas,
                                      n_iterations=n_it, tol=TOL,
                                      max_reg=max_reg, **kw)
        assert len(trace) and int(trace[-1][1]) == state
        out.append(trace)
    return out


@pytest.mark.parametrize("bounded,max_reg,n_it", ORACLE_CONFIGS)
def test_model_replays_the_oracle_fit_traces(bounded, max_reg, n_it):
    """Each trace row (it, state, J_opt, mu, delta) is one attempt.  Its state
    says which way the attempt went (NOT_PD: the sweep failed; REJECTED:
    J_new >= J_opt; ACCEPTED / CONVERGED: J_new < J_opt; MAX_REG: one of the
    first two, told apart by J_opt).  The model, fed a one-candidate attempt of
    that kind from the state the previous row left, must give the row's mu and
    delta bit for bit, MAX_REG exactly where the trace has it, CONVERGED /
    ACCEPTED as the trace wherever the trace holds both costs (a retry: J_opt
    is the previous row's), and masks that match how the trace goes on."""
    traces = _oracle_traces(bounded, max_reg, n_it)
    exits = {am.CONVERGED: 0, am.MAX_REG: 0, am.ACCEPTED: 0}
    attempts = checked_conv = 0
    for trace in traces:
        assert 2 <= len(trace) <= 4096
        mu, delta = am.reset_reg()
        for r, row in enumerate(trace):
            it, state, J = int(row[0]), int(row[1]), np.float32(row[2])
            same_step = r > 0 and int(trace[r - 1][0]) == it
            J_before = np.float32(trace[r - 1][2]) if same_step else None
            if state in (am.ACCEPTED, am.CONVERGED):
                # the cost before: known on a retry; at the first attempt of a
                # step it is the forward pass' sum, which the trace does not
                # hold - any larger finite cost goes the same way through the
                # schedule (the state is then not compared)
                J_opt = J_before if same_step else np.float32(J) * np.float32(2)
                assert J_opt > J > 0
                got = am.attempt(J_opt, [J], 0, mu, delta, it + 1, TOL,
                                 max_reg, n_it, np.float32)
                assert got.amin == 0 and got.J_opt == J
                if same_step:
                    assert got.state == state, (r, row)
                    checked_conv += 1
                else:
                    assert got.state in (am.ACCEPTED, am.CONVERGED)
            else:
                # rejected / failed sweep / max_reg: the nominal's cost stays
                if same_step:
                    assert J == J_before
                got = am.attempt(J, [J], int(state == am.NOT_PD), mu, delta,
                                 it + 1, TOL, max_reg, n_it, np.float32)
                assert got.amin == -1 and got.J_opt == J
                assert (got.state == am.MAX_REG) == (state == am.MAX_REG), row
                if state != am.MAX_REG:
                    assert got.state == state, row
            assert got.mu == row[3] and got.delta == row[4], (r, row, got)
            mu, delta = got.mu, got.delta
            # the masks against how the trace goes on
            last = r == len(trace) - 1
            if got.state == state:
                assert bool(got.active) == (not last), (r, row, got)
                if not last:
                    new_step = int(trace[r + 1][0]) != it
                    assert bool(got.fresh) == new_step
                    assert got.iter == int(trace[r + 1][0]) + 1
                else:
                    assert got.fresh == 0 and got.iter == it + 1
            attempts += 1
        exits[int(trace[-1][1])] += 1
    print("bounded", bounded, "max_reg", max_reg, "n_it", n_it, "attempts",
          attempts, "exits", exits, "accept states compared", checked_conv)
    assert exits[am.CONVERGED] > 0 and exits[am.MAX_REG] > 0, exits


def test_model_schedule_equals_the_reference_recording():
    """accept_schedule.npz: nine seeded sequences of 200 calls of the
    reference's own schedule methods; mu, delta and the return value after
    every call, exactly."""
    g = np.load(os.path.join(GOLDEN_DIR, "accept_schedule.npz"))
    calls, mus, deltas, rets = g["calls"], g["mu"], g["delta"], g["ret"]
    assert calls.shape == (9, 200)
    n_over = n_zeroed = 0
    for s in range(calls.shape[0]):
        max_reg = float(g["max_reg"][s])
        mu = delta = None
        for c in range(calls.shape[1]):
            call = int(calls[s, c])
            if call == 0:
                mu, delta = am.reset_reg()
                ret = -1
            elif call == 1:
                mu, delta, ok = am.increase_reg(mu, delta, max_reg)
                ret = int(ok)
                n_over += not ok
            else:
                before = mu
                mu, delta = am.decrease_reg(mu, delta)
                ret = -1
                n_zeroed += before > 0.0 and mu == 0.0
            assert mu == mus[s, c] and delta == deltas[s, c], (s, c, call)
            assert ret == int(rets[s, c]), (s, c, call)
    # the recording reaches both edges of the schedule
    assert n_over > 0 and n_zeroed > 0, (n_over, n_zeroed)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_edges(dtype):
    """The rows the table tests lean on, spelled out once."""
    dt = np.dtype(dtype).type
    nan, inf = dt(np.nan), dt(np.inf)
    kw = dict(mu=1.0, delta=2.0, iter=1, tol=TOL, max_reg=1e10,
              n_iterations=5, dtype=dtype)
    assert am.argmin([3, 1, 1, 2]) == 1
    assert am.argmin([0.5, nan, 0.1, nan]) == 1
    assert am.argmin([inf, inf]) == 0
    a = am.attempt(dt(2), [dt(1), nan, dt(0.5)], 0, **kw)
    assert (a.state, a.amin, a.mu, a.delta) == (am.REJECTED, -1, 4.0, 4.0)
    a = am.attempt(dt(2), [dt(2)], 0, **kw)           # not <
    assert a.state == am.REJECTED and a.J_opt == dt(2)
    a = am.attempt(dt(2), [np.nextafter(dt(2), dt(-inf))], 0, **kw)
    assert (a.state, a.amin, a.mu, a.delta, a.active) == (
        am.CONVERGED, 0, 0.5, 0.5, 0)
    a = am.attempt(dt(-1), [dt(-3)], 0, **kw)         # rel < 0 < tol
    assert a.state == am.CONVERGED
    a = am.attempt(dt(0), [dt(-1)], 0, **kw)          # rel = inf
    assert (a.state, a.iter, a.active, a.fresh) == (am.ACCEPTED, 2, 1, 1)
    a = am.attempt(inf, [dt(1)], 0, **kw)             # rel = nan
    assert a.state == am.ACCEPTED
    a = am.attempt(dt(2), [dt(1)], 0, **dict(kw, iter=5))
    assert (a.state, a.iter, a.active, a.fresh) == (am.ACCEPTED, 5, 0, 0)
    a = am.attempt(dt(2), [dt(1)], 7, **dict(kw, max_reg=4.0))
    assert (a.state, a.mu, a.active, a.amin) == (am.MAX_REG, 4.0, 0, -1)
    a = am.attempt(dt(2), [dt(1)], 7, **dict(kw, max_reg=np.nextafter(4.0, 5)))
    assert (a.state, a.active, a.fresh) == (am.NOT_PD, 1, 0)
    # a decrease that lands exactly on mu_min goes to 0, just above stays
    assert am.decrease_reg(2e-6, 1.0) == (0.0, 0.5)
    m, d = am.decrease_reg(np.nextafter(2e-6, 1.0), 1.0)
    assert m > am.MU_MIN and d == 0.5
    assert am.increase_reg(0.0, 0.25, 1.0) == (1e-6, 2.0, True)
    assert am.decrease_reg(1.0, 8.0) == (0.5, 0.5)


def test_decision_table_covers_every_exit():
    import accept_rows as tab
    """The table itself: every state, both masks, a winner at every kind of
    position - by the model, before any kernel is asked."""
    for dtype in ("f32", "f64"):
        for A in (1, 10, 11, 16):
            rows = tab.table_rows(A, dtype)
            e = tab.expected(rows, dtype)
            live = np.array([r[0] for r in rows]) == 1
            assert 256 < len(rows) < 600 and len(rows) % 16
            assert set(e["state"][live]) == {1, 2, 3, 4, 5}
            assert (~live).sum() >= 16
            assert set(e["amin"]) >= ({-1, 0, A // 2, A // 3, A - 1}
                                      if A >= 3 else {-1, 0})
            it_out = (e["state"] == am.ACCEPTED) & (e["active"] == 0) & live
            assert it_out.any()  # left by the iteration count
            assert ((e["mu"] == 0.0) & live).any()
            assert ((e["mu"] == tab.MAX_REG) & (e["state"] == am.MAX_REG)).any()
            assert (live[256:]).any()  # a live row in a wrapped shard
