"""Pins the CPU oracle (oracle/, plain C) to the reference: every oracle
function is compared with golden vectors captured from anassinator/pddp itself
(tools/make_golden.py).  CPU-only."""
import numpy as np
import pytest

import oracle as orc
from action_families import eig_sweep_numpy
from golden_util import (DT, FWD_NAMES, TAGS_DC150, load, load_dc150, np_dtype,
                         rel_err, tags)

PROBLEMS = ["cartpole", "pendulum", "double_cartpole", "rendezvous"]
# fp64: restatement vs reference differ only by summation order / LAPACK
# rounding.  fp32: same, at float epsilon, amplified through the horizon.
TOL = {"f64": 1e-9, "f32": 2e-3}
TOL_FWD = {"f64": 1e-11, "f32": 3e-4}


@pytest.mark.parametrize("problem", PROBLEMS)
def test_constants_match_reference(problem):
    g = load(problem)
    p = orc.make_problem(problem, DT[problem])
    na, m = p.aug_size, p.action_size
    Q = np.array(p.Q).reshape(8, 8)[:na, :na]
    Qt = np.array(p.Q_term).reshape(8, 8)[:na, :na]
    R = np.array(p.R).reshape(4, 4)[:m, :m]
    assert np.array_equal(Q, g["const/cost/Q"])
    assert np.array_equal(Qt, g["const/cost/Q_term"])
    assert np.array_equal(R, g["const/cost/R"])
    goal = np.broadcast_to(g["const/cost/x_goal"], (na,))
    assert np.allclose(np.array(p.x_goal)[:na], goal, rtol=0, atol=1e-15)
    names = {"cartpole": ["dt", "mc", "mp", "l", "mu", "g"],
             "pendulum": ["dt", "m", "l", "mu", "g"],
             "double_cartpole": ["dt", "mc", "mp1", "mp2", "l1", "l2", "mu",
                                 "g"],
             "rendezvous": ["dt", "m", "alpha"]}[problem]
    for i, nm in enumerate(names):
        assert p.params[i] == float(g["const/model/" + nm]), nm


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_forward_matches_reference(problem, dtype):
    g = load(problem, dtype=dtype)
    o = orc.load(np_dtype(dtype))
    p = orc.make_problem(problem, DT[problem])
    for tag in tags(problem):
        for sub, bounded in (("fwd", False), ("fwd_bounded", True)):
            kw = dict(u_min=g["u_min"], u_max=g["u_max"]) if bounded else {}
            out = o.forward(p, g["z0"], g[tag + "/U"], **kw)
            for nm in FWD_NAMES:
                ref = g["%s/%s/%s" % (tag, sub, nm)]
                err = rel_err(out[nm], ref)
                assert err < TOL_FWD[dtype], (tag, sub, nm, err)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_backward_matches_reference(problem, dtype):
    g = load(problem, dtype=dtype)
    o = orc.load(np_dtype(dtype))
    n_ok = n_fail = 0
    for tag in tags(problem):
        f = {nm: g["%s/fwd_bounded/%s" % (tag, nm)] for nm in FWD_NAMES}
        for branch in "ABCD":
            for reg in (0.0, 1e-6, 1.0, 100.0):
                key = "%s/bwd/%s/%g" % (tag, branch, reg)
                kw = dict(reg=reg, V_zz_reg=branch in "CD")
                if branch in "BD":
                    kw.update(u_min=g["u_min"], u_max=g["u_max"],
                              U=g[tag + "/U"])
                k, K, status = o.backward(f["F_z"], f["F_u"], f["L_z"],
                                          f["L_u"], f["L_zz"], f["L_uz"],
                                          f["L_uu"], **kw)
                ok = int(g[key + "/ok"])
                if problem == "rendezvous" and branch in "AB":
                    # Reference defect (documented in DESIGN.md): ilqr.py:631
                    # uses the NON-symmetric eig (geev); for repeated
                    # eigenvalues (rendezvous is x/y symmetric) its
                    # eigenvectors are not orthogonal, so E diag(1/e) E^T is
                    # not Q_uu^-1 and the output is LAPACK-internal.  The
                    # oracle uses the intended symmetric decomposition; it
                    # is checked against numpy eigh in
                    # test_backward_eig_branch_vs_numpy instead.
                    continue
                if dtype == "f32" and ok != (status == 0):
                    # knife-edge PD tests may flip in float; must not in f64
                    continue
                assert ok == (status == 0), (key, status)
                if ok:
                    n_ok += 1
                    ek = rel_err(k, g[key + "/k"])
                    eK = rel_err(K, g[key + "/K"])
                    assert ek < TOL[dtype] and eK < TOL[dtype], (key, ek, eK)
                else:
                    n_fail += 1
    assert n_ok >= 12


def test_boxqp_matches_reference():
    g = np.load(__import__("os").path.join(
        __import__("golden_util").GOLDEN_DIR, "boxqp.npz"))
    for case in range(int(g["n_cases"])):
        key = "case%d" % case
        dt = g[key + "/Q"].dtype
        o = orc.load(dt)
        x, result, Uf, free = o.boxqp(g[key + "/x0"], g[key + "/Q"],
                                      g[key + "/c"], g[key + "/lower"],
                                      g[key + "/upper"])
        ref = int(g[key + "/result"])
        if dt == np.float64:
            assert result == ref, (key, result)
        else:  # float: the exit test taken at the optimum is a knife edge
            assert (result >= 1) == (ref >= 1), (key, result, ref)
        if result >= 1:
            tol = 1e-10 if dt == np.float64 else 1e-4
            assert np.allclose(x, g[key + "/x"], rtol=tol, atol=tol), key
            assert np.array_equal(free, g[key + "/free"]), key


def test_boxqp_of_one_action_returns_the_clamped_newton_point():
    """What the benched sweep's lean BoxQP rests on (csrc/riccati_n4_elem.hpp
    QpLean1): for ONE action the reference's projected
    Newton loop with its Armijo back-tracking (constraint.py:150-266, restated
    in oracle/pddp_oracle.c and pinned by test_boxqp_matches_reference) returns
    the clamped warm start where its first exit tests say so, and
    clamp(newton) otherwise - whatever step sizes the back-tracking tries.
    20 000 problems of the sweep's distribution in float64 (where f(x1) - f(x0)
    is not rounding noise): warm starts inside / on / outside the box, Newton
    points inside, beyond and next to the bounds, curvature over six decades."""
    o = orc.load(np.float64)
    rng = np.random.RandomState(5)
    n = 20000
    Q = np.exp(rng.uniform(-6, 8, n))
    c = rng.randn(n) * np.exp(rng.uniform(-4, 6, n))
    un = 3.0 * rng.randn(n)
    lo, hi = -10.0 - un, 10.0 - un
    x0 = lo + (hi - lo) * rng.rand(n)
    k = n // 8
    x0[:k] = lo[:k]
    x0[k:2 * k] = hi[k:2 * k]
    x0[2 * k:3 * k] = lo[2 * k:3 * k] + 30.0 * rng.randn(k)
    # Newton point a hair inside / outside a bound: steps the clamp cuts to
    # almost nothing (theta -> 0: the back-tracking's longest runs)
    sl = slice(3 * k, 4 * k)
    c[sl] = -Q[sl] * hi[sl] * (1.0 + 1e-9 * rng.randn(k))
    sl = slice(4 * k, 5 * k)
    x0[sl] = hi[sl] - np.exp(rng.uniform(-30, 0, k))
    c[sl] = -Q[sl] * (hi[sl] + np.exp(rng.uniform(-3, 6, k)))
    worst, failed = 0.0, 0
    for i in range(n):
        x, result, _, _ = o.boxqp(np.array([x0[i]]), np.array([[Q[i]]]),
                                  np.array([c[i]]), np.array([lo[i]]),
                                  np.array([hi[i]]))
        if result < 1:
            failed += 1
            continue
        xs = min(max(x0[i], lo[i]), hi[i])
        x1 = min(max(-c[i] / Q[i], lo[i]), hi[i])
        g0 = Q[i] * xs + c[i]
        clamped0 = (xs == lo[i] and g0 > 0) or (xs == hi[i] and g0 < 0)
        want = xs if (clamped0 or abs(g0) < 1e-8) else x1
        scale = max(1.0, abs(want))
        worst = max(worst, abs(x[0] - want) / scale)
    # measured: no failure, worst deviation 3.6e-15 - the loop's answer IS the
    # closed form, to the rounding of the Newton point
    assert failed == 0, failed
    assert worst < 1e-12, worst


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_line_search_matches_reference(problem, dtype):
    g = load(problem, dtype=dtype)
    o = orc.load(np_dtype(dtype))
    p = orc.make_problem(problem, DT[problem])
    for tag in tags(problem):
        f = {nm: g["%s/fwd_bounded/%s" % (tag, nm)] for nm in FWD_NAMES}
        U = g[tag + "/U"]
        k = g[tag + "/bwd/B/1/k"]
        K = g[tag + "/bwd/B/1/K"]
        for sched in ("fit", "mpc"):
            alphas = g["%s/ls_%s/alphas" % (tag, sched)]
            Zn, Un = o.control_law(p, f["Z"], U, k, K, alphas, g["u_min"],
                                   g["u_max"])
            J = o.trajectory_cost(p, Zn, Un)
            Zr = g["%s/ls_%s/Z_new" % (tag, sched)]
            Ur = g["%s/ls_%s/U_new" % (tag, sched)]
            Jr = g["%s/ls_%s/J" % (tag, sched)]
            N = Ur.shape[0]
            if N <= 5:
                tol = 1e-12 if dtype == "f64" else 1e-5
                assert rel_err(Zn, Zr) < tol
                assert rel_err(Un, Ur) < tol
                assert rel_err(J, Jr) < tol
            else:
                # Long horizons with reg=1 gains give DIVERGING candidate
                # rollouts (|z| up to 1e246, inf, NaN): rounding differences
                # grow exponentially with t.  Check the stable prefix tightly
                # and the non-finite pattern of the costs.
                T = 12
                tol = 1e-9 if dtype == "f64" else 2e-3
                assert rel_err(Zn[:T], Zr[:T]) < tol
                assert rel_err(Un[:T], Ur[:T]) < tol
                assert np.array_equal(np.isfinite(J), np.isfinite(Jr))
                if dtype == "f64":
                    fin = np.isfinite(Jr)
                    assert np.allclose(J[fin], Jr[fin], rtol=1e-6)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_backward_eig_branch_vs_numpy(dtype):
    """m = 4 (rendezvous): the eig-clamp branch against an independent numpy
    restatement with the symmetric eigendecomposition (see the note in
    test_backward_matches_reference)."""
    g = load("rendezvous", dtype=dtype)
    o = orc.load(np_dtype(dtype))
    for tag in tags("rendezvous"):
        f = {nm: g["%s/fwd_bounded/%s" % (tag, nm)].astype(np.float64)
             for nm in FWD_NAMES}
        for reg in (0.0, 1.0):
            k, K, status = o.backward(f["F_z"], f["F_u"], f["L_z"], f["L_u"],
                                      f["L_zz"], f["L_uz"], f["L_uu"], reg=reg)
            assert status == 0
            # the float64 numpy restatement (action_families.eig_sweep_numpy)
            kn, Kn, _ = eig_sweep_numpy(f, reg)
            tol = 1e-9 if dtype == "f64" else 2e-3
            for t in range(f["F_u"].shape[0]):
                assert np.allclose(k[t], kn[t], rtol=tol, atol=tol * 10)
                assert np.allclose(K[t], Kn[t], rtol=tol, atol=tol * 10)


@pytest.mark.parametrize("mode", ["bounded", "free"])
@pytest.mark.parametrize("problem", PROBLEMS[:3])
def test_fit_trace_matches_reference(problem, mode):
    """Whole controller: same state sequence, mu/delta schedule and costs as
    iLQRController.fit (fp64)."""
    g = load(problem)
    o = orc.load(np.float64)
    p = orc.make_problem(problem, DT[problem])
    ft = "fit_" + mode
    alphas = 1.025 ** (-np.arange(10.0) ** 2)
    kw = dict(u_min=g["u_min"], u_max=g["u_max"]) if mode == "bounded" else {}
    Z, U, K, state, trace = o.fit(p, g["z0"], g[ft + "/U0"], alphas,
                                  n_iterations=int(g[ft + "/n_iterations"]),
                                  **kw)
    ref = g[ft + "/trace"]
    assert trace.shape == ref.shape
    assert np.array_equal(trace[:, :2], ref[:, :2])  # iteration, state
    assert np.allclose(trace[:, 3:], ref[:, 3:], rtol=1e-12)  # mu, delta
    assert np.allclose(trace[:, 2], ref[:, 2], rtol=1e-7)  # J_opt
    assert state == int(g[ft + "/state"])
    assert rel_err(U, g[ft + "/U"]) < 1e-5
    assert rel_err(Z, g[ft + "/Z"]) < 1e-5
    assert rel_err(K, g[ft + "/K"]) < 1e-5


def test_oracle_at_configs3_horizon_matches_reference():
    """BASELINE configs[3]'s horizon (double cartpole, N = 150) against the
    reference's own outputs (tools/make_golden.py --dc-default): bounded
    forward pass, the four backward branches x four regularisations, the fit
    schedule's line search, and the three-iteration bounded fit (11 attempts)."""
    g = load_dc150()
    o = orc.load(np.float64)
    p = orc.make_problem("double_cartpole", DT["double_cartpole"])
    kwb = dict(u_min=g["u_min"], u_max=g["u_max"])
    n_ok = 0
    for tag in TAGS_DC150:
        U = g[tag + "/U"]
        out = o.forward(p, g["z0"], U, **kwb)
        for nm in FWD_NAMES:
            err = rel_err(out[nm], g["%s/fwd_bounded/%s" % (tag, nm)])
            assert err < 1e-11, (tag, nm, err)
        f = {nm: g["%s/fwd_bounded/%s" % (tag, nm)] for nm in FWD_NAMES}
        for branch in "ABCD":
            for reg in (0.0, 1e-6, 1.0, 100.0):
                key = "%s/bwd/%s/%g" % (tag, branch, reg)
                kw = dict(reg=reg, V_zz_reg=branch in "CD")
                if branch in "BD":
                    kw.update(U=U, **kwb)
                k, K, status = o.backward(f["F_z"], f["F_u"], f["L_z"],
                                          f["L_u"], f["L_zz"], f["L_uz"],
                                          f["L_uu"], **kw)
                assert int(g[key + "/ok"]) == (status == 0), (key, status)
                if status == 0:
                    n_ok += 1
                    assert rel_err(k, g[key + "/k"]) < 1e-9, key
                    assert rel_err(K, g[key + "/K"]) < 1e-9, key
        alphas = g[tag + "/ls_fit/alphas"]
        Zn, Un = o.control_law(p, f["Z"], U, g[tag + "/bwd/B/1/k"],
                               g[tag + "/bwd/B/1/K"], alphas, g["u_min"],
                               g["u_max"])
        J = o.trajectory_cost(p, Zn, Un)
        Zr, Ur, Jr = (g["%s/ls_fit/%s" % (tag, nm)] for nm in
                      ("Z_new", "U_new", "J"))
        T = 12  # (candidates of reg = 1 gains diverge on long horizons)
        assert rel_err(Zn[:T], Zr[:T]) < 1e-9 and rel_err(Un[:T], Ur[:T]) < 1e-9
        assert np.array_equal(np.isfinite(J), np.isfinite(Jr))
        fin = np.isfinite(Jr)
        assert np.allclose(J[fin], Jr[fin], rtol=1e-6)
    assert n_ok >= 20
    ft = "fit_bounded"
    assert int(g[ft + "/N"]) == 150
    Z, U, K, state, trace = o.fit(p, g["z0"], g[ft + "/U0"],
                                  1.025 ** (-np.arange(10.0) ** 2),
                                  n_iterations=int(g[ft + "/n_iterations"]),
                                  **kwb)
    ref = g[ft + "/trace"]
    assert trace.shape == ref.shape
    assert np.array_equal(trace[:, :2], ref[:, :2])
    assert np.allclose(trace[:, 3:], ref[:, 3:], rtol=1e-12)
    assert np.allclose(trace[:, 2], ref[:, 2], rtol=1e-7)
    assert state == int(g[ft + "/state"])
    assert rel_err(U, g[ft + "/U"]) < 1e-5
    assert rel_err(K, g[ft + "/K"]) < 1e-5


# ---- the second CPU restatement: torch ops, one trajectory (oracle/torch_port.py)
def _torch_problem(problem):
    import pddp_amd
    mod = getattr(pddp_amd.examples, problem)
    model = [getattr(mod, n) for n in dir(mod) if n.endswith("DynamicsModel")
             and n != "DynamicsModel"][0](DT[problem]).double()
    cost = [getattr(mod, n) for n in dir(mod) if n.endswith("Cost")
            and n != "AugmentedQRCost"][0]().double()
    return model, cost


@pytest.mark.parametrize("problem", PROBLEMS)
def test_torch_port_matches_reference(problem):
    """oracle/torch_port.py (the op-for-op PyTorch-CPU leg of bench.py's
    cpu_baseline) against the reference's golden outputs in fp64:
    derivative rollout, the four gain branches (with the same successes and
    failures), both line-search schedules."""
    import torch
    import pddp_amd
    from oracle import torch_port as tp
    g = load(problem, dtype="f64")
    enc = pddp_amd.StateEncoding.IGNORE_UNCERTAINTY
    model, cost = _torch_problem(problem)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    u_min, u_max = t_(g["u_min"]), t_(g["u_max"])
    n_ok = 0
    for tag in tags(problem)[:2]:
        U = t_(g[tag + "/U"])
        out = tp.forward(t_(g["z0"]), U, model, cost, enc, u_min, u_max)
        for nm, t in zip(FWD_NAMES, out):
            assert rel_err(t.numpy(), g["%s/fwd_bounded/%s" % (tag, nm)]) < 1e-10, \
                (tag, nm)
        for branch in "ABCD":
            if problem == "rendezvous" and branch in "AB":
                continue  # reference's non-symmetric eig: see the C port's test
            for reg in (0.0, 1e-6, 1.0, 100.0):
                key = "%s/bwd/%s/%g" % (tag, branch, reg)
                kw = dict(reg=reg, V_zz_reg=branch in "CD")
                if branch in "BD":
                    kw.update(u_min=u_min, u_max=u_max, U=U)
                try:
                    k, K = tp.backward(*out[1:3], *out[4:], **kw)
                    ok = True
                except RuntimeError:
                    ok = False
                assert ok == bool(int(g[key + "/ok"])), key
                if ok:
                    n_ok += 1
                    assert rel_err(k.numpy(), g[key + "/k"]) < 1e-8, key
                    assert rel_err(K.numpy(), g[key + "/K"]) < 1e-8, key
        k, K = t_(g[tag + "/bwd/B/1/k"]), t_(g[tag + "/bwd/B/1/K"])
        for sched in ("fit", "mpc"):
            alphas = t_(g["%s/ls_%s/alphas" % (tag, sched)])
            Zn, Un = tp.control_law(model, out[0], U, k, K, alphas, enc, u_min,
                                    u_max)
            J = tp.trajectory_cost(cost, Zn, Un, enc)
            T = 6  # stable prefix of possibly diverging candidates
            assert rel_err(Zn[:T].numpy(),
                           g["%s/ls_%s/Z_new" % (tag, sched)][:T]) < 1e-9
            assert rel_err(Un[:T].numpy(),
                           g["%s/ls_%s/U_new" % (tag, sched)][:T]) < 1e-9
            Jr = g["%s/ls_%s/J" % (tag, sched)]
            fin = np.isfinite(Jr)
            assert np.allclose(J.numpy()[fin], Jr[fin], rtol=1e-7)
    assert n_ok >= 6


def test_torch_port_boxqp_and_iteration():
    """boxqp of the torch port on the reference's unit cases, and one whole
    iteration against the C port's (same accept decision, same costs)."""
    import os
    import torch
    import pddp_amd
    from oracle import torch_port as tp
    g = np.load(os.path.join(__import__("golden_util").GOLDEN_DIR, "boxqp.npz"))
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    for case in range(int(g["n_cases"])):
        key = "case%d" % case
        if g[key + "/Q"].dtype != np.float64:
            continue
        x, result, Uf, free = tp.boxqp(t_(g[key + "/x0"]), t_(g[key + "/Q"]),
                                       t_(g[key + "/c"]), t_(g[key + "/lower"]),
                                       t_(g[key + "/upper"]))
        assert result == int(g[key + "/result"]), key
        if result >= 1:
            assert np.allclose(x.numpy(), g[key + "/x"], rtol=1e-10, atol=1e-10)
            assert np.array_equal(free.numpy().astype(np.uint8),
                                  g[key + "/free"].astype(np.uint8)), key
    problem = "cartpole"
    gg = load(problem, dtype="f64")
    model, cost = _torch_problem(problem)
    enc = pddp_amd.StateEncoding.IGNORE_UNCERTAINTY
    tag = tags(problem)[0]
    U = t_(gg[tag + "/U"])
    alphas = t_(gg[tag + "/ls_fit/alphas"])
    U2, J0, J1, acc = tp.iteration(t_(gg["z0"]), U, model, cost, enc,
                                   t_(gg["u_min"]), t_(gg["u_max"]), alphas,
                                   reg=1.0)
    Jr = gg[tag + "/ls_fit/J"]
    assert np.isclose(J0, float(gg[tag + "/fwd_bounded/L"].sum()), rtol=1e-12)
    assert np.isclose(J1, np.nanmin(Jr), rtol=1e-7)
    assert acc == (np.nanmin(Jr) < J0)
