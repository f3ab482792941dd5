"""sweep_records.py on the CPU: its numpy model of the m = 1 sweep against the
float64 oracle, the conditions its families promise the GPU tests
(test_matrix_sweeps.py), and the comparison against broken copies of the
model."""
import numpy as np
import pytest

import oracle as orc
import sweep_records as sr
from golden_util import rel_err

SIZES = [1, 3, 7, 14, 22, 30]
HORIZONS = [1, 2, 5]


def oracle_sweep(o, rec, b, V_zz_reg, bounds, reg):
    args, kw = sr.oracle_call(rec, b, V_zz_reg, bounds, reg)
    return o.backward(*args, **kw), args, kw


def step_err(a, b):
    """Largest per-step rel_err (a NaN equal to a NaN)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    a, b = np.nan_to_num(a), np.nan_to_num(b)
    return max(rel_err(a[t], b[t]) if np.abs(b[t]).max() > 0 else
               float(np.abs(a[t]).max()) for t in range(a.shape[0]))


@pytest.mark.parametrize("N", HORIZONS)
@pytest.mark.parametrize("n", SIZES)
def test_model_equals_the_float64_oracle(n, N):
    """k, K to 1e-10 per step and the status, on every trajectory of the
    batch - the four families, the faults included - under every launch
    configuration: both gain branches, unbounded, bounded and with the wide
    bounds."""
    rec, _ = sr.launch_batch(n, N, np.float64)
    o = orc.load(np.float64)
    for V_zz_reg, bounds, reg in sr.CONFIGS:
        for b in range(len(sr.ROLES)):
            (ko, Ko, so), _, _ = oracle_sweep(o, rec, b, V_zz_reg, bounds, reg)
            m = sr.model_sweep(sr.one(rec, b), sr.reg_of(b, reg), V_zz_reg,
                               bounds, rec["U"][b])
            key = (V_zz_reg, bounds, reg, b, sr.ROLES[b])
            assert m["status"] == so, key
            assert step_err(m["k"], ko) < 1e-10, key
            assert step_err(m["K"], Ko) < 1e-10, key
            if bounds is not None and so == sr.BWD_OK and \
                    sr.ROLES[b] != "repeat":
                # the outcome is the oracle's: a clamped step has K == 0
                # (`repeat` has Q_uz == 0 on its free steps)
                assert np.array_equal(m["outcome"] != sr.FREE,
                                      (Ko == 0).all(axis=(1, 2))), key


def test_fault_statuses_by_branch():
    """What the faults are there for: a NaN in L_uu raises in `eig`, fails
    `potrf` and fails the BoxQP; -1e4 is clamped on the eig-clamp branch and
    is NOT_PD on the unbounded Cholesky branch.  The two indefinite
    trajectories are NOT_PD there as well."""
    rec, good = sr.launch_batch(7, 5, np.float64)
    nan, neg = sr.FAULTS
    assert np.isnan(rec["L_uu"][nan]).sum() == 1 and \
        (rec["L_uu"][neg] == -1e4).sum() == 1
    assert np.isfinite(good["L_uu"]).all() and (good["L_uu"][neg] > 0).all()
    for V_zz_reg, bounds, reg in sr.CONFIGS:
        res = sr.classify(rec, V_zz_reg, bounds, reg)
        want_nan = sr.BWD_NAN if not V_zz_reg else (
            sr.BWD_NOT_PD if bounds is None else sr.BWD_BOXQP_FAILED)
        assert res[nan]["status"] == want_nan
        if not V_zz_reg:
            assert res[neg]["status"] == sr.BWD_OK
        elif bounds is None:
            assert res[neg]["status"] == sr.BWD_NOT_PD
            assert res[3]["status"] == res[4]["status"] == sr.BWD_NOT_PD


@pytest.mark.parametrize("n", range(1, 31))
def test_family_conditions_hold_at_every_launched_size(n):
    """For every (n, dtype, N) of test_matrix_sweeps.py: status 0 by the
    float64 oracle on every trajectory that is not a fault, under every
    launch configuration; by the model, Q_uu < 0 exactly at the chosen steps,
    every BoxQP margin at least 1e-2, the three outcomes in every bounded
    launch, the exact-on-bound steps, nothing active under the wide
    bounds."""
    o = orc.load(np.float64)
    for N in HORIZONS:
        for npd in (np.float32,) + ((np.float64,) if n <= 14 else ()):
            rec, _ = sr.launch_batch(n, N, npd)
            assert sr.broken_conditions(rec, N) == []
            r64 = sr.rounded(rec, np.float64)
            for V_zz_reg, bounds, reg in sr.CONFIGS:
                for b in range(len(sr.ROLES)):
                    if b == sr.INACTIVE or sr.fault_like(b, V_zz_reg):
                        continue
                    (_, _, so), _, _ = oracle_sweep(o, r64, b, V_zz_reg,
                                                    bounds, reg)
                    assert so == sr.BWD_OK, (n, N, npd, V_zz_reg, bounds, b)


@pytest.mark.parametrize("npd", [np.float32, np.float64])
def test_repeat_reaches_the_outlined_boxqp(npd):
    """n4::QpClosed::solve in IEEE arithmetic (the forms without fast math) on
    the second of the two equal steps of `repeat`: the warm start is the
    Newton point -((c / U) / U) of the first, so s0 = 0 and s0 g0 = 0 - the
    Armijo test cannot pass and no bound cuts the step -, while the residual
    g0 = Q x + c is no smaller than min_grad = 1e-8, whether the compiler
    fuses it or not: iteration 0 is not done, `slow` is set."""
    from fractions import Fraction
    for V_zz_reg, _, reg in sr.CONFIGS:
        Q = npd(sr.REPEAT_QUU) if V_zz_reg else \
            npd(sr.REPEAT_QUU) + npd(reg)   # F_u = 0: Q_uu_reg = L_uu
        c = npd(sr.REPEAT_QU)
        U = np.sqrt(Q)
        newton = -((c / U) / U)
        assert type(newton) is npd and -0.31 < newton < -0.29
        g0 = Q * newton + c
        fused = float(Fraction(float(Q)) * Fraction(float(newton)) +
                      Fraction(float(c)))
        assert abs(g0) >= 1e-8 and abs(fused) >= 1e-8, (npd, V_zz_reg, reg)
        s0 = newton - newton
        assert not (s0 * g0 < 0)


def test_the_comparison_rejects_three_mutants():
    """The model broken in one place - the eig clamp dropped, K kept on a
    clamped step, V_z without Q_uz^T k - is outside 1e-10 of the oracle on
    the trajectories that meet the broken place, and only in the
    configurations that reach it; the unbroken model is inside everywhere
    (test_model_equals_the_float64_oracle)."""
    n, N = 7, 5
    rec, _ = sr.launch_batch(n, N, np.float64)
    o = orc.load(np.float64)
    hit = {"no_clamp": set(), "K_kept": set(), "Vz_short": set()}
    for V_zz_reg, bounds, reg in sr.CONFIGS:
        for b in range(len(sr.ROLES)):
            if b in sr.FAULTS:
                continue
            (ko, Ko, so), _, _ = oracle_sweep(o, rec, b, V_zz_reg, bounds, reg)
            for mut in hit:
                m = sr.model_sweep(sr.one(rec, b), sr.reg_of(b, reg), V_zz_reg,
                                   bounds, rec["U"][b], mutant=mut)
                if m["status"] != so or step_err(m["k"], ko) >= 1e-10 or \
                        step_err(m["K"], Ko) >= 1e-10:
                    hit[mut].add((V_zz_reg, bounds is not None, b))
    # the clamp: the indefinite trajectories, eig-clamp branch only
    assert hit["no_clamp"] and all(
        not V and sr.ROLES[b] in ("indef_last", "indef_t0")
        for V, _, b in hit["no_clamp"])
    assert {b for _, _, b in hit["no_clamp"]} == {3, 4, 15}
    # K of a clamped step: bounded launches only, every bounds* trajectory
    assert all(bd for _, bd, _ in hit["K_kept"])
    assert {6, 7, 8, 9} <= {b for _, _, b in hit["K_kept"]}
    # V_z: every trajectory with more than one step, in every configuration
    assert {b for _, _, b in hit["Vz_short"]} >= set(range(len(sr.ROLES))) - {
        sr.FAULTS[0], sr.FAULTS[1]}
