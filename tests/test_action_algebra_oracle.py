"""The C oracle's action-space algebra for m = 2 .. 4 (its cyclic Jacobi, eig
clamp, Cholesky and BoxQP inside `backward`) against plain float64 numpy on
the families of action_families.py - no GPU.  The HIP kernel's gains.hpp
restates the same Jacobi, so a kernel-against-oracle comparison cannot see an
error the two share; this file keeps the yardstick itself honest, and tells a
GPU failure of test_action_algebra.py in the kernel from one shared with the
port.

One step (N = 1, F_u = 0, F_z = I, L_uz = [I_m | 0], n = 5): Q_uu = sym(L_uu)
exactly, -K[0][:, :m] is the side's inverse, k[0] = -inv Q_u.

Unbounded branches: r = ||inv_o - inv||_2 / ||inv||_2 / (eps kappa) against
`eigh` (invariant to the eigenvector basis: repeated eigenvalues are well
posed), the same for k.  The oracle's worst over m = 2 .. 4 and all families:
5.7 in float64 (repeat, m = 4), 7.9 in float32 (repeat, m = 4); the bars are
four times 5.9 and 3.0.

Bounded branches: k against the minimiser found by enumerating the 3^m active
patterns, |k - x| / max(1, |x|), over every case but those with an eigenvalue
clamped at reg = 0 (action_families.boxqp_decidable) and those whose KKT
margin is below 1e-3 (at most 12 in 3920).  With cond(Q_g) <= 100 the oracle's
worst is 49 eps in float64 (138 to 294 cases) and 5.45e3 eps in float32 (2233
to 4794 cases: action_families.probe_batch says why so many); the bars are
four times 17 eps and 2.5e3 eps, and the free set never differs.  Above cond
100 the errors are taken in units of cond(Q_g) (action_families.bounded_tiers):
K at most 1.45, k at most 8.5 but for one float64 `graded` case at 1.3e3, and
the BoxQP ends beside the minimiser on 1 of 214 cases (float64, m = 3) and 2 of
3365 (float32, m = 3)."""
import collections

import numpy as np
import pytest

import action_families as af
from action_families import BRANCHES, oracle_side
from golden_util import np_dtype

R_BAR = {"f64": 4 * 5.9, "f32": 4 * 3.0}
K_BAR_EPS = {"f64": 4 * 17.0, "f32": 4 * 2.5e3}
LEFT_OUT = 0.04


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("name,V_zz_reg,bounded", BRANCHES,
                         ids=[b[0] for b in BRANCHES])
def test_oracle_one_step_probe_vs_numpy(name, V_zz_reg, bounded, m, dtype):
    (labels, A, reg, rec), k, K, st, ref = oracle_side(m, dtype, V_zz_reg,
                                                       bounded)
    eps = float(np.finfo(np_dtype(dtype)).eps)
    assert not st.any(), dict(zip(labels, st))
    assert np.isfinite(k).all() and np.isfinite(K).all()
    if not bounded:
        # the Cholesky branch regularises V_zz, which F_u = 0 keeps out of Q_uu
        worst = af.unbounded_worst(labels, A, 0 * reg if V_zz_reg else reg,
                                   rec, k, K, eps)
        print(name, m, dtype, {f: round(r, 2) for f, r in worst.items()})
        assert max(worst.values()) <= R_BAR[dtype], worst
        return
    t = af.bounded_tiers(ref, k, K)
    (ek, eK, sameA, A_), (rk, rK, sameB, B_) = t["A"], t["B"]
    print(name, m, dtype, "A: k %.3g eps, K %.3g eps, free set %d of %d;  "
          "B: k %.3g, K %.3g eps cond, free set %d of %d;  %d cases" % (
              ek / eps, eK / eps, sameA.sum(), A_.sum(), rk / eps, rK / eps,
              sameB.sum(), B_.sum(), len(ref)))
    assert len(ref) >= (2000 if dtype == "f32" else 250)
    assert A_.sum() + B_.sum() >= (1 - LEFT_OUT) * len(ref)
    # cond(Q_g) <= 100: the quoted figures
    assert ek <= K_BAR_EPS[dtype] * eps and eK <= K_BAR_EPS[dtype] * eps
    assert sameA.sum() == A_.sum()
    # above: K, a plain solve, at the float64 figure in units of cond; k at
    # the float32 one in both dtypes, for the objective test's early stop is
    # met in float64 too (1.3e3 on a `graded` case); the reference's BoxQP
    # ends beside the minimiser in at most one case, or 1 of 400
    assert rK <= K_BAR_EPS["f64"] * eps and rk <= K_BAR_EPS["f32"] * eps
    assert B_.sum() - sameB.sum() <= max(1, B_.sum() / 400.0)


def test_families_hold_their_condition():
    """The builders' own assertion, and the exact structure the names promise
    (zeros that are zeros, a subnormal that is one)."""
    for dtype in (np.float64, np.float32):
        for m in (2, 3, 4):
            for name in af.FAMILIES:
                a = af.family(name, m, 4, dtype)
                assert a.shape == (4, m, m)
                assert np.array_equal(a.astype(dtype).astype(np.float64), a)
            assert np.array_equal(af.family("cI", m, 1, dtype)[0], 3 * np.eye(m))
            d = af.family("diag", m, 3, dtype)
            assert not (d * (1 - np.eye(m))).any()
            assert ((np.diagonal(d, axis1=1, axis2=2) < 0).any(axis=1)).all()
            assert ((np.diagonal(d, axis1=1, axis2=2) > 0).any(axis=1)).all()
            p = af.family("perm", m, 1, dtype)[0]
            assert not np.diag(p).any() and p[0, m - 1] == 1
            lam = np.linalg.eigvalsh(af.family("indef", m, 5, dtype))
            assert (lam.min(axis=1) < 0).all() and (lam.max(axis=1) > 0).all()
            b = af.family("block", m, 2, dtype)
            assert not b[0][:m - m // 2, m - m // 2:].any()
            assert not b[1][:m // 2, m // 2:].any()
        t = af.family("denorm", 4, 1, dtype)[0, 0, 1]
        assert 0 < t < np.finfo(np.float32).tiny


def test_enumerated_boxqp_is_the_minimiser():
    """The reference of the bounded probes (action_families.bounded_reference,
    a batch of two) against a brute-force grid on two-dimensional problems
    with one active bound and with none."""
    Q = np.array([[2.0, 0.5], [0.5, 1.0]])
    A = np.stack([Q, Q])
    rec = dict(L_u=np.array([[[-4.0, 0.3]], [[0.4, -0.3]]]),
               U=np.zeros((2, 1, 2)),
               L_uz=np.broadcast_to(np.eye(2), (2, 1, 2, 2)).copy())
    ref = af.bounded_reference(A, np.zeros(2), rec, True)
    g = np.linspace(-1, 1, 401)
    X, Y = np.meshgrid(g, g, indexing="ij")
    P = np.stack([X.ravel(), Y.ravel()], 1)
    for b, (x, K, f, margin, cond) in enumerate(ref):
        c = rec["L_u"][b, 0]
        obj = 0.5 * np.einsum("pi,ij,pj->p", P, Q, P) + P @ c
        assert np.abs(P[obj.argmin()] - x).max() <= 5e-3
        assert margin > 0 and np.isclose(cond, np.linalg.cond(Q))
        assert not K[~f].any()
        assert np.allclose(K[np.ix_(f, f)], -np.linalg.inv(Q[np.ix_(f, f)]))
    assert ref[0][0][0] == 1.0 and list(ref[0][2]) == [False, True]
    assert list(ref[1][2]) == [True, True]
