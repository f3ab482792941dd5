"""Seeded record families for the m = 1 sweeps at any state size n, and a
plain numpy float64 model of that sweep (controllers/ilqr.py:489-526, 581-672
restated for one action).  The model CLASSIFIES - which steps clamp Q_uu,
which BoxQP outcome a step has and by what margin - so that a test can assert
that the cases it claims are in its batch; the yardstick for values stays the
C oracle (test_sweep_records.py holds the model to it on the CPU,
test_matrix_sweeps.py the matrix-core kernels on the GPU).

One batch (`batch`) is the trajectories of one launch; ROLES names them:

  plain       the distribution of test_backward_large_state_vs_oracle
              (F_z ~ I, L_zz SPD, L_uu > 0).  Trajectory 0 always runs at
              reg = 0; trajectory 2 is the inactive one.
  indef_last  L_uu < 0 at t = N - 1 (and t = N - 3): the first step of the
              sweep already takes the clamp e = 1e-12 (ilqr.py:633)
  indef_t0    L_uu < 0 at t = 0 only.  The second one (trajectory 15) always
              runs at reg = 0: the only place where the 1e-12 of the clamp is
              more than a 1e-9th of Q_uu_reg, k = -1e12 Q_u; nothing follows
              the step, so nothing grows
  small_quu   0 < Q_uu < reg at every step (L_uu = 2^-12)
              At the indefinite steps F_u and L_uz are scaled by 1e-4: Q_uz is
              small there, so the rank-one term c Q_uz^T Q_uz of the value
              update (c ~ -Q_uu / reg^2) stays modest and the steps below do
              not clamp in their turn (asserted: the clamped steps by the
              model are exactly the chosen ones).  On the Cholesky branch
              there is no clamp: Q_uu_reg < 0 fails `potrf` (unbounded) or the
              BoxQP, so there the two indef_* trajectories are held like
              faults - status the oracle's, gains not compared.
  bounds0..2  L_u placed step by step (by the model, at reg = 1e-3 on the
              eig-clamp branch) so that step t has outcome (t + i) % 3 of
              free / at u_min / at u_max: all three in every trajectory with
              N >= 3 and in every launch from N = 1 on
  on_umin     U[t0] == u_min exactly with Q_u > 0: the feasible step is 0
  on_umax     U[t0] == u_max exactly with Q_u > 0: free, moving inward
  repeat      steps 1 and 0 carry the same scalars (F_u = L_uz = 0, so Q_uu =
              L_uu and Q_u = L_u exactly) and are free: the warm start of step
              0 is already its Newton point (see test_matrix_sweeps.py on the
              outlined BoxQP)
  nan, neg    a NaN / a -1e4 in L_uu of an otherwise plain trajectory; FAULTS
              maps them to the records without the fault
"""
import functools

import numpy as np

ARG_NAMES = ("F_z", "F_u", "L_z", "L_u", "L_zz", "L_uz", "L_uu")
BWD_OK, BWD_NAN, BWD_NOT_PD, BWD_BOXQP_FAILED = 0, 1, 2, 3
NONE, FREE, LOWER, UPPER = -1, 0, 1, 2  # BoxQP outcome of a step
U_MIN, U_MAX = -1.0, 1.0
WIDE = 1e6  # the launch whose bounds are never active
MARGIN = 1e-2

ROLES = ("plain", "plain", "plain", "indef_last", "indef_t0", "small_quu",
         "bounds0", "bounds1", "bounds2", "on_umin", "on_umax", "repeat",
         "plain", "nan", "neg", "indef_t0", "plain")
INACTIVE = 2
REG0 = (0, 15)     # the trajectories that run at reg = 0
FAULTS = (13, 14)  # workgroups {12 .. 15} (16x16 form) / {12, 13}, {14, 15}
REGS = (1e-3, 1.0)
# (V_zz_reg, bounds, reg) of every launch of test_matrix_sweeps.py
CONFIGS = [(V, bd, reg) for V in (False, True)
           for bd in (None, (U_MIN, U_MAX)) for reg in REGS] + \
          [(V, (-WIDE, WIDE), REGS[0]) for V in (False, True)]


def reg_of(b, reg):
    return 0.0 if b in REG0 else reg


def fault_like(b, V_zz_reg):
    """Trajectories whose status is compared and whose gains are not."""
    return b in FAULTS or (V_zz_reg and ROLES[b] in ("indef_last", "indef_t0"))


# ---------------------------------------------------------------------------
# the model


def _q_terms(r, t, V, Vz):
    A, f = r["F_z"][t], r["F_u"][t][:, 0]
    Qz = r["L_z"][t] + A.T @ Vz
    Qu = r["L_u"][t, 0] + f @ Vz
    Qzz = r["L_zz"][t] + A.T @ V @ A
    Quz = r["L_uz"][t, 0] + f @ V @ A
    Quu = r["L_uu"][t, 0, 0] + f @ V @ f
    return Qz, Qu, 0.5 * (Qzz + Qzz.T), Quz, Quu


def _boxqp1(x0, Q, c, lo, hi):
    """utils/constraint.py:150-266 for one variable, as what it converges to:
    (x, free, failed).  clamp(-c / Q, lo, hi); a start already clamped with
    the gradient pointing outward stays (before the factorisation is tried),
    and so does one whose gradient is below min_grad."""
    x0 = min(max(x0, lo), hi)
    out = lambda x: (x == lo and Q * x + c > 0) or (x == hi and Q * x + c < 0)
    if out(x0):
        return x0, False, False
    if not (Q > 0 and np.isfinite(Q)):
        return x0, True, True
    if abs(Q * x0 + c) < 1e-8:
        return x0, True, False
    x = min(max(-c / Q, lo), hi)
    return x, not out(x), False


def model_sweep(records, reg=0.0, V_zz_reg=False, bounds=None, U=None,
                mutant=None):
    """One trajectory's sweep in float64: dict with k (N, 1), K (N, 1, n),
    status and, per step, Q_uu, the BoxQP outcome (NONE when unbounded or not
    reached) and its margin: the distance of the unconstrained step from the
    nearer bound over hi - lo.  `mutant`: a deliberately broken copy
    ("no_clamp", "K_kept", "Vz_short"; test_sweep_records.py)."""
    r = {nm: np.asarray(records[nm], np.float64) for nm in ARG_NAMES}
    N, n = r["F_u"].shape[:2]
    k, K = np.zeros((N, 1)), np.zeros((N, 1, n))
    Quu_t = np.full(N, np.nan)
    outcome, margin = np.full(N, NONE), np.full(N, np.inf)
    V, Vz = r["L_zz"][N].copy(), r["L_z"][N].copy()
    status = BWD_OK
    for t in reversed(range(N)):
        Qz, Qu, Qzz, Quz, Quu = _q_terms(r, t, V, Vz)
        Quu_t[t] = Quu
        if V_zz_reg:                                      # ilqr.py:588-592
            _, _, _, Quz_g, Qg = _q_terms(r, t, V + reg * np.eye(n), Vz)
        else:                                             # ilqr.py:631-634
            if not np.isfinite(Quu):
                status = BWD_NAN
                break
            e = 1e-12 if (Quu < 0 and mutant != "no_clamp") else Quu
            Qg, Quz_g = e + reg, Quz
        if bounds is None:
            if V_zz_reg and not (Qg > 0 and np.isfinite(Qg)):
                status = BWD_NOT_PD                       # ilqr.py:595
                break
            with np.errstate(all="ignore"):
                kt, Kt = -Qu / Qg, -Quz_g / Qg
            k[t], K[t] = kt, Kt
            if not V_zz_reg and (np.isnan(kt) or np.isnan(Kt).any()):
                status = BWD_NAN                          # ilqr.py:639-640
                break
        else:
            lo, hi = bounds[0] - U[t, 0], bounds[1] - U[t, 0]
            kt, free, failed = _boxqp1(k[min(t + 1, N - 1), 0], Qg, Qu, lo, hi)
            k[t] = kt
            if failed:
                status = BWD_BOXQP_FAILED
                break
            outcome[t] = FREE if free else (LOWER if kt == lo else UPPER)
            if Qg > 0:
                margin[t] = min(abs(-Qu / Qg - lo), abs(-Qu / Qg - hi)) / (hi - lo)
            Kt = -Quz_g / Qg if (free or mutant == "K_kept") else 0.0 * Quz
            K[t] = Kt
        # value update with the un-regularised terms (ilqr.py:619-625, 664-672)
        Vz = Qz + Kt * Qu + Kt * Quu * kt
        if mutant != "Vz_short":
            Vz = Vz + Quz * kt
        V = Qzz + Quu * np.outer(Kt, Kt) + np.outer(Kt, Quz) + np.outer(Quz, Kt)
        V = 0.5 * (V + V.T)
    return dict(k=k, K=K, status=status, Quu=Quu_t, outcome=outcome,
                margin=margin)


# ---------------------------------------------------------------------------
# the families: float64 masters, one trajectory each


def plain(n, N, rng):
    R = 0.2 * rng.standard_normal((N + 1, n, n))
    return dict(
        F_z=np.eye(n) + 0.05 * rng.standard_normal((N, n, n)),
        F_u=0.3 * rng.standard_normal((N, n, 1)),
        L_z=rng.standard_normal((N + 1, n)),
        L_u=rng.standard_normal((N, 1)),
        L_zz=np.eye(n) + R @ R.transpose(0, 2, 1),
        L_uz=0.05 * rng.standard_normal((N, 1, n)),
        L_uu=1.0 + 0.04 * rng.standard_normal((N, 1, 1)) ** 2,
        U=0.5 * rng.standard_normal((N, 1)))


def indefinite_steps(role, N):
    """The steps at which the model must see Q_uu < 0 (eig-clamp branch)."""
    if role == "indef_last":
        return sorted({N - 1, max(N - 3, 0)} if N >= 3 else {N - 1})
    return [0] if role == "indef_t0" else []


def indefinite(n, N, rng, role):
    r = plain(n, N, rng)
    steps = range(N) if role == "small_quu" else indefinite_steps(role, N)
    for t in steps:
        r["F_u"][t] *= 1e-4
        r["L_uz"][t] *= 1e-4
        r["L_uu"][t] = 2.0 ** -12 if role == "small_quu" else \
            -0.25 - 0.5 * rng.random()
    return r


def exact_step(N):
    return N // 2


def bounded(n, N, rng, role):
    """L_u chosen going down the sweep so that the unconstrained step lands
    where the role wants it; U within +-0.3 so that a free step stays free
    under every reg of CONFIGS."""
    r = plain(n, N, rng)
    r["U"] = 0.3 * (2.0 * rng.random((N, 1)) - 1.0)
    want = [(t + int(role[-1])) % 3 if role[:-1] == "bounds" else t % 3
            for t in range(N)]
    t0 = exact_step(N)
    if role == "on_umin":
        r["U"][t0], want[t0] = U_MIN, LOWER
    if role == "on_umax":
        r["U"][t0], want[t0] = U_MAX, FREE
    V, Vz, kprev = r["L_zz"][N].copy(), r["L_z"][N].copy(), 0.0
    for t in reversed(range(N)):
        Qz, Qu, Qzz, Quz, Quu = _q_terms(r, t, V, Vz)
        Qg = Quu + REGS[0]
        u = r["U"][t, 0]
        if role == "on_umax" and t == t0:
            x = -0.5
        else:
            x = {FREE: 0.3 * (2.0 * rng.random() - 1.0) - u,
                 LOWER: U_MIN - u - 4.0, UPPER: U_MAX - u + 4.0}[want[t]]
        r["L_u"][t, 0] += -x * Qg - Qu
        Qu = -x * Qg
        kt, free, _ = _boxqp1(kprev, Qg, Qu, U_MIN - u, U_MAX - u)
        Kt = -Quz / Qg if free else 0.0 * Quz
        Vz = Qz + Kt * Qu + Kt * Quu * kt + Quz * kt
        V = Qzz + Quu * np.outer(Kt, Kt) + np.outer(Kt, Quz) + np.outer(Quz, Kt)
        V, kprev = 0.5 * (V + V.T), kt
    return r


# (Q_u: the first of 0.9 * 2^32 + 12345.678 + 1000.123 j whose residual is not
# 0 in either type, fused or not - test_repeat_reaches_the_outlined_boxqp)
REPEAT_QUU, REPEAT_QU = 3.0 * 2.0 ** 32, 3865483912.201


def repeat(n, N, rng):
    """Steps 1 and 0 with the same scalars and free (k = -0.3).  Q_uu is no
    power of two, so that neither sqrt(Q) nor 1 / Q is exact and the Newton
    point -Q_u / Q carries a rounding; Q_u is large, so that the residual Q x +
    Q_u at that point, a rounding of Q_u, stays above the BoxQP's min_grad of
    1e-8 in float64 too."""
    r = plain(n, N, rng)
    for t in range(min(N, 2)):
        r["F_u"][t] = 0.0
        r["L_uz"][t] = 0.0
        r["L_uu"][t] = REPEAT_QUU
        r["L_u"][t] = REPEAT_QU
        r["U"][t] = 0.125
    return r


def fault(n, N, rng, role):
    """(records with the fault, records without it, the faulty step)."""
    good = plain(n, N, rng)
    bad = dict(good, L_uu=good["L_uu"].copy())
    # (-1e4 at the last step of the sweep: with reg = 1e-3 the value function
    # below a clamp of that size grows by 1e26 a step, and whether float32
    # overflows within five steps would be decided by the operation order)
    t = N // 2 if role == "nan" else 0
    bad["L_uu"][t] = np.nan if role == "nan" else -1e4
    return bad, good, t


def batch(n, N, seed):
    """The float64 masters of one launch: (records with a leading batch
    dimension, the same with the faults removed)."""
    bad, good = [], []
    for b, role in enumerate(ROLES):
        rng = np.random.default_rng([seed, n, N, b])
        if role in ("nan", "neg"):
            rb, rg, _ = fault(n, N, rng, role)
        else:
            rb = plain(n, N, rng) if role == "plain" else \
                repeat(n, N, rng) if role == "repeat" else \
                indefinite(n, N, rng, role) if role in (
                    "indef_last", "indef_t0", "small_quu") else \
                bounded(n, N, rng, role)
            rg = rb
        bad.append(rb)
        good.append(rg)
    stack = lambda rs: {nm: np.stack([r[nm] for r in rs]) for nm in rs[0]}
    return stack(bad), stack(good)


def one(rec, b):
    return {nm: v[b] for nm, v in rec.items()}


def oracle_call(rec, b, V_zz_reg, bounds, reg):
    """(args, kw) of the oracle's `backward` for trajectory b of a batch
    under one launch's configuration, in the dtype of the records."""
    kw = dict(reg=reg_of(b, reg), V_zz_reg=V_zz_reg)
    if bounds is not None:
        npd = rec["U"].dtype
        kw.update(u_min=np.full(1, bounds[0], npd),
                  u_max=np.full(1, bounds[1], npd), U=rec["U"][b])
    return [rec[nm][b] for nm in ARG_NAMES], kw


def classify(rec, V_zz_reg, bounds, reg):
    """model_sweep of every trajectory of a batch under one launch's
    configuration (None for the inactive one)."""
    return [None if b == INACTIVE else model_sweep(
        one(rec, b), reg_of(b, reg), V_zz_reg, bounds, rec["U"][b])
        for b in range(len(ROLES))]


def broken_conditions(rec, N, models=None):
    """The conditions on the inputs that a test asserts (module docstring of
    test_matrix_sweeps.py); the list of those that do not hold.  `models`: a
    dict that receives `classify` of every configuration."""
    bad = []
    for V_zz_reg, bounds, reg in CONFIGS:
        key = (V_zz_reg, bounds, reg)
        res = classify(rec, V_zz_reg, bounds, reg)
        if models is not None:
            models[key] = res
        seen = set()
        for b, m in enumerate(res):
            if m is None or fault_like(b, V_zz_reg):
                continue
            role = ROLES[b]
            if m["status"] != BWD_OK:
                bad.append((key, b, "status", m["status"]))
            if not V_zz_reg:
                want = indefinite_steps(role, N)
                if list(np.nonzero(m["Quu"] < 0)[0]) != want:
                    bad.append((key, b, "clamped Q_uu at", m["Quu"]))
                if role == "small_quu" and not (
                        (m["Quu"] > 0) & (m["Quu"] < REGS[0])).all():
                    bad.append((key, b, "small Q_uu", m["Quu"]))
            if bounds is None:
                continue
            if not (m["margin"] >= MARGIN).all():
                bad.append((key, b, "margin", m["margin"].min()))
            seen |= set(m["outcome"])
            if bounds[1] == WIDE:
                # (reg = 0 under a clamped Q_uu: a step of 1e12 Q_u)
                if (m["outcome"] != FREE).any() and b != REG0[1]:
                    bad.append((key, b, "wide bounds active"))
                continue
            t0 = exact_step(N)
            if role == "on_umin" and not (
                    m["outcome"][t0] == LOWER and m["k"][t0, 0] == 0.0):
                bad.append((key, b, "on u_min"))
            if role == "on_umax" and not (
                    m["outcome"][t0] == FREE and m["k"][t0, 0] < 0.0):
                bad.append((key, b, "on u_max"))
            if role == "repeat" and (m["outcome"][:2] != FREE).any():
                bad.append((key, b, "repeat"))
            if role[:-1] == "bounds" and list(m["outcome"]) != [
                    (t + int(role[-1])) % 3 for t in range(N)]:
                bad.append((key, b, "outcomes", m["outcome"]))
        if bounds is not None and bounds[1] != WIDE and \
                not {FREE, LOWER, UPPER} <= seen:
            bad.append((key, "outcomes of the launch", seen))
    return bad


def rounded(rec, npd):
    return {nm: v.astype(npd) for nm, v in rec.items()}


@functools.lru_cache(maxsize=None)
def chosen_seed(n, N):
    """The first seed whose batch, rounded to float32 and (n <= 14) as it
    is, meets every condition."""
    for seed in range(200):
        rec, _ = batch(n, N, seed)
        if not broken_conditions(rounded(rec, np.float32), N) and (
                n > 14 or not broken_conditions(rec, N)):
            return seed
    raise AssertionError("no seed for n = %d, N = %d" % (n, N))


def launch_batch(n, N, npd):
    """(records, records without the faults) in the run's dtype."""
    rec, good = batch(n, N, chosen_seed(n, N))
    return rounded(rec, npd), rounded(good, npd)
