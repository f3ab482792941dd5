"""The generic sweep's action-space algebra for m = 2 .. 4 (csrc/gains.hpp:
jacobi_eig, chol_upper_masked, chol_solve, boxqp; run in every lane by
csrc/riccati_generic.hpp) on the MI355X, against plain float64 numpy rather
than against the oracle alone - the oracle's Jacobi is the kernel's, line for
line, so the two can share an error.  The families, the one-step probe and the
references are action_families.py's; test_action_algebra_oracle.py holds the
oracle to the same references on the CPU.

Measured on the MI355X, worst ratio per family as kernel / oracle of the same
dtype (unbounded probes, r in units of eps * kappa; families not listed: 0 on
both sides in float64, equal on both sides in float32 and at most 1.0):

  eig   m  dtype  spd        indef      repeat     block      perm       graded
        2  f64    0.58/0.56  0.76/0.78  0.45/0.42  0.00/0.00  0.77/0.77  0.70/0.29
        2  f32    0.25/0.39  0.83/0.73  0.78/0.95  0.75/0.75  1.02/1.02  0.43/0.82
        3  f64    0.83/0.70  3.67/4.59  1.72/1.72  1.44/1.14  3.19/1.31  1.60/1.60
        3  f32    0.54/0.66  2.19/1.71  0.87/1.11  1.58/1.55  1.54/0.76  0.04/0.04
        4  f64    1.19/1.19  3.22/3.91  4.13/5.73  0.53/0.57  0.64/0.48  0.88/0.88
        4  f32    0.13/0.64  2.28/2.78  1.98/7.90  1.05/0.90  0.77/1.03  0.00/0.00
  chol  m  dtype  spd        cI         graded     (denorm 0.00/0.00)
        2  f64    0.40/0.40  1.46/1.46  0.70/0.70
        2  f32    0.20/0.32  0.99/0.99  0.58/0.13
        3  f64    0.71/0.65  1.27/1.27  1.60/1.60
        3  f32    0.29/0.29  0.91/0.91  0.02/0.02
        4  f64    1.57/1.53  1.06/1.06  0.88/0.88
        4  f32    0.20/0.12  0.90/0.90  0.00/0.00

Bounded probes, kernel / oracle, on the cases kept (KKT margin >= 1e-3; at
most 12 of 3920 left out; no status anywhere).  "A", cond(Q_g) <= 100: worst
|k - x| / max(1, |x|) and the same for K in eps, free sets all the
reference's on both sides.  "B", above it: the same in units of eps cond(Q_g)
(action_families.bounded_tiers).

            m  f64 A k    f64 A K    f64 B k      f64 B K    f32 A k        f32 A K    f32 B k    f32 B K
  eig_box   2  5.13/3.0   4.5/4.5    .0014/.0035  .002/.003  1.36e3/1.36e3  19.4/39.4  0.79/0.79  0.42/0.34
            3  14.9/49    39.5/39.0  0.85/0.85    1.08/1.08  1.74e3/2.44e3  28.5/44.6  1.17/2.24  0.22/0.24
            4  41/47      37.2/53.1  610/1.33e3   1.45/1.45  1.65e3/2.33e3  18.9/28.4  8.37/8.47  0.32/0.21
  chol_box  2  2.0/2.5    5.27/6.02  7e-5/7e-5    1e-4/1e-4  811/811        10.7/7.15  0.41/0.52  .007/.007
            3  3.5/3.5    5.75/5.75  .005/.005    .002/.002  258/1.03e3     18.2/18.9  0.95/0.96  0.20/0.20
            4  12.2/10.0  12.8/14.5  0.04/0.03    0.10/0.06  2.18e3/5.45e3  18.9/18.9  0.56/2.66  0.24/0.24

Cases (A + B): eig_box float64 294 + 189, 265 + 214, 275 + 213; float32 4794 +
2957, 4302 + 3365, 4457 + 3361; chol_box float64 about 150 + 150, float32
about 2500 + 2300.  In "B" the float64 oracle ends beside the minimiser on one
case (m = 3, `indef` under reg = 1e-3), and the kernel ends where it does; in
float32 the oracle does so on 2 cases for m = 3 and the kernel on 2 others for
m = 4.

(With 286 float32 cases of cond(Q_g) <= 100 instead of 4302 the same kernel
measured 56.8 eps against the oracle's 6.45 on eig_box, m = 3 - a ratio of 8.8
between two draws from the tail that action_families.probe_batch describes.)
"""
import numpy as np
import pytest
import torch

import oracle as orc
import action_families as af
from action_families import BRANCHES, oracle_side
from golden_util import np_dtype, rel_err
from solver_util import TDT
# (conftest.py dumps sys.modules["test_gpu_parity"].STATS: the fp32
# bookkeeping stays in that module - the one import from a test module)
from test_gpu_parity import _check_gains, _f32_ok, F32_RATIO

pytestmark = pytest.mark.gpu

BWD_OK, BWD_NAN, BWD_NOT_PD, BWD_BOXQP_FAILED = 0, 1, 2, 3


def _cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------
# one step: eig, clamp, inverse, Cholesky and BoxQP of the kernel


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("name,V_zz_reg,bounded", BRANCHES,
                         ids=[b[0] for b in BRANCHES])
def test_one_step_probe_vs_numpy(name, V_zz_reg, bounded, m, dtype):
    """A whole family list as the trajectories of ONE launch of the generic
    kernel (N = 1, n = 5 -> riccati_generic_kernel<T, 8, m>), reg 0, 1e-3 and
    1 riding along per trajectory.  Unbounded: the kernel's worst ratio per
    family at most F32_RATIO x max(the oracle's of the same dtype, 1) - the
    floor is one rounding of the input.  Bounded, on the cases whose KKT
    margin is at least 1e-3 (at least 95% of the batch; the only other
    exclusion is action_families.boxqp_decidable's): with cond(Q_g) <= 100 the
    kernel's worst distance from the enumerated minimiser (k) and from the
    free rows' solve (K) at most F32_RATIO x the oracle's on the same cases,
    clamped rows of K exactly 0, and the free set the reference's (float32:
    as often as the oracle's is); above that (action_families.bounded_tiers)
    the same in units of cond(Q_g) with the unbounded probes' floor, on the
    cases where the oracle ends in the minimiser, and the free set the
    reference's wherever the oracle's is (float32: see below)."""
    from pddp_amd.controllers.ilqr import backward
    (labels, A, reg, rec), ko, Ko, sto, ref = oracle_side(m, dtype, V_zz_reg,
                                                          bounded)
    assert not sto.any()
    B = len(labels)
    kw = dict(reg=_cuda(reg), V_zz_reg=V_zz_reg)
    if bounded:
        one = np.ones(m, np_dtype(dtype))
        kw.update(u_min=_cuda(-one), u_max=_cuda(one), U=_cuda(rec["U"]))
    Z = torch.zeros(B, 2, af.N_STATE, dtype=TDT[dtype], device="cuda")
    L = torch.zeros(B, 2, dtype=TDT[dtype], device="cuda")
    k, K, st = backward(Z, _cuda(rec["F_z"]), _cuda(rec["F_u"]), L,
                        _cuda(rec["L_z"]), _cuda(rec["L_u"]),
                        _cuda(rec["L_zz"]), _cuda(rec["L_uz"]),
                        _cuda(rec["L_uu"]), return_status=True,
                        kernel_variant=1, **kw)
    k, K, st = k.cpu().numpy(), K.cpu().numpy(), st.cpu().numpy()
    eps = float(np.finfo(np_dtype(dtype)).eps)
    assert not st.any(), dict(zip(labels, st))
    assert np.isfinite(k).all() and np.isfinite(K).all()
    if not bounded:
        r = 0 * reg if V_zz_reg else reg
        hip = af.unbounded_worst(labels, A, r, rec, k, K, eps)
        ora = af.unbounded_worst(labels, A, r, rec, ko, Ko, eps)
        print("PROBE", name, m, dtype, " ".join(
            "%s %.2f/%.2f" % (f, hip[f], ora[f]) for f in hip))
        for f in hip:
            assert hip[f] <= F32_RATIO * max(ora[f], 1.0), (f, hip[f], ora[f])
        return
    to = af.bounded_tiers(ref, ko, Ko)
    agree = to["same"]
    if dtype == "f32":
        # above cond 100 the float32 BoxQP ends beside the minimiser on about
        # 1 case in 1700, on rounding: the oracle on 0, 2 and 0 of 2957, 3365
        # and 3361 eig_box cases for m = 2, 3, 4, the kernel (MI355X) on 0, 0
        # and 2, never the same ones.  The errors are measured where both
        # sides end in the minimiser; the number where the kernel does not is
        # held to the bound test_action_algebra_oracle.py sets the oracle.
        agree = agree & af.bounded_tiers(ref, k, K)["same"]
        to = af.bounded_tiers(ref, ko, Ko, agree=agree)
    th = af.bounded_tiers(ref, k, K, agree=agree)
    for tier in "AB":
        (ek, eK, same, mask), (eko, eKo, sameo, _) = th[tier], to[tier]
        print("PROBE", name, m, dtype, tier, "k %.3g/%.3g  K %.3g/%.3g eps%s  "
              "free set %d/%d of %d, %d cases" % (
                  ek / eps, eko / eps, eK / eps, eKo / eps,
                  " cond" if tier == "B" else "", same.sum(), sameo.sum(),
                  mask.sum(), B))
    assert th["A"][3].sum() + th["B"][3].sum() >= 0.95 * B
    # cond(Q_g) <= 100: the issue's bars
    (ek, eK, same, mask), (eko, eKo, sameo, _) = th["A"], to["A"]
    assert ek <= F32_RATIO * eko, (ek / eps, eko / eps)
    assert eK <= F32_RATIO * eKo, (eK / eps, eKo / eps)
    assert same.sum() == mask.sum() if dtype == "f64" else \
        same.sum() >= sameo.sum()
    # above it: units of cond, floor of one rounding as in the unbounded
    # probes, on the cases where the oracle ends in the minimiser; the free
    # set the reference's wherever the oracle's is
    (rk, rK, same, mask), (rko, rKo, sameo, _) = th["B"], to["B"]
    assert rk <= F32_RATIO * max(rko, eps), (rk / eps, rko / eps)
    assert rK <= F32_RATIO * max(rKo, eps), (rK / eps, rKo / eps)
    if dtype == "f64":
        assert not (sameo & ~same).any()
        # where it is not, the kernel ends where the oracle does
        odd = mask & ~sameo
        assert np.array_equal((K[odd, 0] != 0).any(axis=-1),
                              (Ko[odd, 0] != 0).any(axis=-1))
        assert rel_err(k[odd], ko[odd]) < 1e-9 and \
            rel_err(K[odd], Ko[odd]) < 1e-9
    else:
        assert mask.sum() - same.sum() <= max(1, mask.sum() / 400.0)


# ---------------------------------------------------------------------------
# sweeps in context: every (NMAX, M) instantiation with M > 1


def _sweep(rec, dtype, reg, V_zz_reg, bounded, active):
    """pddp_riccati_backward on packed records with an `active` mask; gains
    and status pre-filled so that an untouched trajectory shows."""
    from pddp_amd import _native
    dt = TDT[dtype]
    B, N, n, m = rec["F_u"].shape
    lay = _native.record_layout(n, m)
    dev = {nm: _cuda(rec[nm]) for nm in af.ARG_NAMES + ("U",)}
    p, st = _native.ptr, _native.stream_handle(dev["U"].device)
    buf = torch.empty(B, N + 1, lay.stride, dtype=dt, device="cuda")
    _native.call("pddp_pack_records", dt, B, N, n, m,
                 *[p(dev[nm]) for nm in ("F_z", "F_u", "L_z", "L_u", "L_zz",
                                         "L_uz", "L_uu", "U")], p(buf), st)
    one = torch.ones(m, dtype=dt, device="cuda")
    lo, hi = -one, one
    regv = torch.full((B,), reg, dtype=torch.float64, device="cuda")
    gains = torch.full((B, N, lay.gain_stride), 7.0, dtype=dt, device="cuda")
    status = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    act = None if active is None else _cuda(np.asarray(active, np.uint8))
    _native.call("pddp_riccati_backward_variant", dt, B, N, n, m, p(buf),
                 p(lo) if bounded else None, p(hi) if bounded else None,
                 p(regv), int(V_zz_reg), None if act is None else p(act),
                 p(gains), p(status), st, 0)
    torch.cuda.synchronize()
    g = gains.cpu().numpy()
    return (g[..., :m], g[..., m:].reshape(B, N, m, n), status.cpu().numpy(),
            g)


ALL_BRANCHES = [(V, bd, reg) for V in (False, True) for bd in (False, True)
                for reg in (0.0, 1.0)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [2, 8, 9, 16, 17, 32, 33])
@pytest.mark.parametrize("m", [2, 3, 4])
def test_sweeps_in_context_vs_oracle_and_numpy(m, n, dtype):
    """riccati_generic_kernel<T, {8, 16, 32}, m> on both sides of every NMAX
    boundary (n = 8 / 9, 16 / 17, 32 / 33 - the last the four-wavefront
    riccati_large_kernel<T, m>) and with fewer states than actions, all four
    gain branches, reg 0 and 1, on action_families.sweep_records: status the
    oracle's everywhere, gains the oracle's (`_check_gains`) and, in float64
    on the unbounded eig-clamp branch, numpy `eigh`'s to 1e-8; the inactive
    trajectory untouched.

    Two cells of trajectory 1 (indefinite Q_uu at steps 1 and 4) at reg = 0
    are decided by rounding, and both depart from what the issue that asked
    for these tests expected (status 0 on the eig-clamp branches, equal to the
    oracle's).  Below the first clamp the unbounded sweep grows by 1e24 a
    step (sweep_records): its gains are compared from step 4 on, and its
    status over the whole horizon is the oracle's, which is PDDP_BWD_NAN (the
    overflow), not 0.  The bounded eig-clamp branch hands BoxQP a Q_g with an
    eigenvalue of 1e-12 (action_families.boxqp_decidable): its gains are not
    compared; its status is the oracle's in float64; in float32, where the
    oracle itself goes either way from one shape to the next, it is 0 or
    PDDP_BWD_BOXQP_FAILED, not necessarily the oracle's.

    float32: every row goes through `_check_gains` as it is, but the bounded
    rows of trajectory 3, the one built to meet mixed free sets.  Those use
    its collecting form: per shape at most one of them may lie outside the
    single-row bound, with K inside and k not wild (the suite's 2e-2).  The
    float32 BoxQP's early stop (action_families.probe_batch) is met by that
    trajectory at (m, n) = (3, 17): the float32 ORACLE is 4.9e-5 and 2.0e-5
    from the float64 one on its bounded eig-clamp rows (every other row of
    every shape: at most 1.3e-6), above the Cholesky floor of 3e-5, and the
    kernel meets the same stop on its bounded Cholesky row at reg = 0
    (MI355X: k 1.2e-4 from the float64 oracle with K at 2.6e-7, that is with
    the oracle's free sets and factors at every step; no other row of any
    shape outside)."""
    from pddp_amd.controllers.ilqr import BRANCH_CHOLESKY
    assert BRANCH_CHOLESKY == 1
    npd = np_dtype(dtype)
    rec = af.sweep_records(n, m, npd)
    o = orc.load(npd)
    N = rec["F_u"].shape[1]
    active = [1, 1, 0, 1]
    mixed = 0
    outside = [] if dtype == "f32" else None
    for V_zz_reg, bounded, reg in ALL_BRANCHES:
        key = (V_zz_reg, bounded, reg)
        k, K, st, raw = _sweep(rec, dtype, reg, V_zz_reg, bounded, active)
        assert st[2] == -5 and (raw[2] == 7.0).all(), key
        for b in (0, 1, 3):
            okw = dict(reg=reg, V_zz_reg=V_zz_reg)
            if bounded:
                okw.update(u_min=-np.ones(m, npd), u_max=np.ones(m, npd),
                           U=rec["U"][b])
            args = [rec[nm][b] for nm in af.ARG_NAMES]
            kr, Kr, sr = o.backward(*args, **okw)
            ill_boxqp = b == 1 and reg == 0.0 and bounded and not V_zz_reg
            if ill_boxqp and dtype == "f32":
                assert st[b] in (BWD_OK, BWD_BOXQP_FAILED), (key, st[b])
            else:
                assert st[b] == sr, (key, b, st[b], sr)
            if b != 1:
                assert sr == BWD_OK, (key, b)
            elif V_zz_reg and not bounded:
                assert sr == BWD_NOT_PD, key
            elif not V_zz_reg and not bounded and reg == 0.0:
                assert sr == BWD_NAN, key
            elif not V_zz_reg and not (ill_boxqp and dtype == "f32"):
                assert sr == BWD_OK, key
            if ill_boxqp:
                continue
            t0 = af.sweep_comparable(b, reg) if not (V_zz_reg or bounded) \
                else 0
            if t0 == 0 and sr != BWD_OK:
                continue
            if t0:
                # the steps from t0 on are the sweep over the horizon cut at t0
                cut = [a[t0:] for a in args]
                kr, Kr, sr = o.backward(*cut, **okw)
                assert sr == BWD_OK, key
                args = cut
            _check_gains(dtype, k[b, t0:], K[b, t0:], kr, Kr, args, okw,
                         soft=outside if (bounded and b == 3) else None,
                         test="action_algebra", n=n, m=m, V_zz_reg=V_zz_reg,
                         bounded=bounded, reg=reg, b=b)
            if bounded and b == 3:
                zero = (Kr == 0).all(axis=-1)  # (N, m): clamped actions
                assert np.array_equal((K[b] == 0).all(axis=-1), zero) or \
                    dtype == "f32", key
                # a step with some actions clamped and some free
                per_step = zero.sum(axis=-1)
                mixed += int(((per_step > 0) & (per_step < m)).any())
            if dtype == "f64" and not V_zz_reg and not bounded:
                kn, Kn, _ = af.eig_sweep_numpy(
                    {nm: rec[nm][b] for nm in af.ARG_NAMES}, reg)
                ek = rel_err(k[b, t0:], kn[t0:])
                eK = rel_err(K[b, t0:], Kn[t0:])
                assert ek < 1e-8 and eK < 1e-8, (key, b, ek, eK)
    # trajectory 3 met a mixed free set within a step on every bounded run
    assert mixed == 4
    if outside:
        print("OUTSIDE", outside)
        assert len(outside) <= 1, outside
        r = outside[0]
        assert r["bounded"] and r["b"] == 3 and r["k_hip"] < 2e-2 and _f32_ok(
            r["K_hip"], r["K_o32"], r["V_zz_reg"]), r


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nan_in_one_record_for_three_actions(dtype):
    """m = 3, n = 9: a NaN in one off-diagonal entry of L_uu of trajectory 1
    at step 3.  The status is the oracle's (PDDP_BWD_NAN on the eig-clamp
    branches, where `eig` raises) and the other trajectories' gains are bit
    for bit those of the run without it."""
    npd = np_dtype(dtype)
    rec = af.sweep_records(9, 3, npd)
    bad = dict(rec, L_uu=rec["L_uu"].copy())
    bad["L_uu"][1, 3, 0, 2] = np.nan
    o = orc.load(npd)
    others = [0, 2, 3]
    for V_zz_reg in (False, True):
        for bounded in (False, True):
            _, _, st_ok, g_ok = _sweep(rec, dtype, 1.0, V_zz_reg, bounded, None)
            _, _, st, g = _sweep(bad, dtype, 1.0, V_zz_reg, bounded, None)
            okw = dict(reg=1.0, V_zz_reg=V_zz_reg)
            if bounded:
                okw.update(u_min=-np.ones(3, npd), u_max=np.ones(3, npd),
                           U=bad["U"][1])
            sr = o.backward(*[bad[nm][1] for nm in af.ARG_NAMES], **okw)[2]
            assert sr != BWD_OK and st[1] == sr, (V_zz_reg, bounded, st[1], sr)
            if not V_zz_reg:
                assert sr == BWD_NAN
            assert np.array_equal(st[others], st_ok[others])
            assert np.array_equal(g[others], g_ok[others])
            # the steps above the fault are what they were
            assert np.array_equal(g[1, 4:], g_ok[1, 4:])
