"""Seeded input families for the action-space algebra of the generic sweep
(csrc/gains.hpp: jacobi_eig, chol_upper_masked, chol_solve, boxqp for
m = 2 .. 4) and the plain float64 references they are judged by - shared by
test_action_algebra_oracle.py (the C oracle alone, no GPU) and
test_action_algebra.py (the HIP kernel).  Not a test and not a conftest:
imported by the tests.

Every builder returns symmetric m x m float64 matrices whose values are
exactly representable in the dtype under test (they are cast to it and back),
so both sides and the reference see the same numbers.

  spd      A A^T + 0.1 I
  indef    Q diag(lam) Q^T, |lam| in [0.5, 3], at least one of each sign
  repeat   spectrum (2, .., 2, -1) in a random basis; m = 4 also (2, 2, 5, 5)
  cI/negI  exactly 3 I and -3 I
  diag     exactly diagonal, mixed signs
  block    exact zeros between two blocks (m = 2: two 1 x 1 blocks)
  perm     zero diagonal, a[0][m-1] = a[m-1][0] = 1 (theta = 0 in the first
           rotation that meets it).  m = 2: eigenvalues +-1; m = 4: the
           exchange matrix (+-1 twice); m = 3: every off-diagonal 1
           (eigenvalues 2, -1, -1) - with the other entries zero the matrix is
           singular for m > 2 and the clamp is not defined
  graded   diag(d) + sqrt(d) C sqrt(d), d = 10^U(-6, 6), |C| ~ 1e-3
  denorm   diag(1e6, 1, 1e-6, 1e3)[:m] and a[0][1] = a[1][0] = 1e-42
           (subnormal in float32)

A property of the inputs, asserted here: the float64 `eigh` of the cast matrix
has min |lam| >= 1e-3 max |lam| (graded, denorm: every lam > 0), so that the
discontinuous clamp `e < 0 -> 1e-12` never sits on a rounding error.
"""
import functools
import itertools

import numpy as np

import oracle as orc
from golden_util import np_dtype

FAMILIES = ("spd", "indef", "repeat", "cI", "negI", "diag", "block", "perm",
            "graded", "denorm")
# positive definite whatever the seed: the inputs of the Cholesky branches
PD_FAMILIES = ("spd", "cI", "graded", "denorm")
REGS = (0.0, 1e-3, 1.0)
N_STATE = 5  # n of the one-step probe


def _cast(a, dtype):
    return np.asarray(a, np.float64).astype(dtype).astype(np.float64)


def _basis(rng, m):
    q, r = np.linalg.qr(rng.standard_normal((m, m)))
    return q * np.sign(np.diag(r))


def _signs(rng, m):
    """Random signs, at least one of each."""
    while True:
        s = rng.choice([-1.0, 1.0], size=m)
        if abs(s.sum()) < m:
            return s


def _sym(a):
    return 0.5 * (a + a.T)


def _indef(rng, m):
    q = _basis(rng, m)
    lam = rng.uniform(0.5, 3.0, m) * _signs(rng, m)
    return _sym((q * lam) @ q.T)


def _draw(name, m, rng, i):
    if name == "spd":
        a = rng.standard_normal((m, m))
        return a @ a.T + 0.1 * np.eye(m)
    if name == "indef":
        return _indef(rng, m)
    if name == "repeat":
        lam = np.array([2.0] * (m - 1) + [-1.0])
        if m == 4 and i % 2:
            lam = np.array([2.0, 2.0, 5.0, 5.0])
        q = _basis(rng, m)
        return _sym((q * lam) @ q.T)
    if name == "cI":
        return 3.0 * np.eye(m)
    if name == "negI":
        return -3.0 * np.eye(m)
    if name == "diag":
        return np.diag(rng.uniform(0.5, 3.0, m) * _signs(rng, m))
    if name == "block":
        h = m // 2 if i % 2 else m - m // 2
        a = np.zeros((m, m))
        for lo, hi in ((0, h), (h, m)):
            w = hi - lo
            a[lo:hi, lo:hi] = (_indef(rng, w) if w > 1 else
                               rng.uniform(0.5, 3.0) * rng.choice([-1.0, 1.0]))
        return a
    if name == "perm":
        if m == 3:
            return np.ones((3, 3)) - np.eye(3)
        return np.eye(m)[::-1].copy()
    if name == "graded":
        d = 10.0 ** rng.uniform(-6.0, 6.0, m)
        c = 1e-3 * rng.standard_normal((m, m))
        c = _sym(c)
        np.fill_diagonal(c, 0.0)
        s = np.sqrt(d)
        return np.diag(d) + s[:, None] * c * s[None, :]
    if name == "denorm":
        a = np.diag([1e6, 1.0, 1e-6, 1e3][:m])
        a[0, 1] = a[1, 0] = 1e-42
        return a
    raise ValueError(name)


def _well_posed(name, a):
    lam = np.linalg.eigvalsh(a)
    if name in ("graded", "denorm"):
        return bool((lam > 0).all())
    return bool(np.abs(lam).min() >= 1e-3 * np.abs(lam).max())


def family(name, m, count, dtype, seed=0):
    """`count` matrices of one family, (count, m, m) float64 holding `dtype`
    values.  A random draw that misses the eigenvalue condition after the cast
    is drawn again (the stream stays seeded); the condition is asserted on
    everything returned."""
    rng = np.random.default_rng([seed, m, FAMILIES.index(name)])
    out = np.empty((count, m, m))
    for i in range(count):
        for _ in range(100):
            a = _cast(_sym(_draw(name, m, rng, i)), dtype)
            if _well_posed(name, a):
                break
        assert _well_posed(name, a), (name, m, i)
        assert np.array_equal(a, a.T)
        out[i] = a
    return out


def cases(names, m, dtype, per_family=10, seed=0):
    """The batch of one probe launch: every family of `names`, `per_family`
    matrices each, every matrix once per regularisation of REGS.  Returns
    (labels, A (B, m, m), reg (B,)); labels[b] is the family's name."""
    labels, mats, regs = [], [], []
    for name in names:
        for a in family(name, m, per_family, dtype, seed):
            for reg in REGS:
                labels.append(name)
                mats.append(a)
                regs.append(reg)
    return labels, np.stack(mats), np.asarray(regs)


def probe_records(A, dtype, seed=0):
    """One-step records (N = 1, n = N_STATE) around the matrices A (B, m, m):
    F_u = 0, F_z = I, L_zz = I, L_uz = [I_m | 0], so that Q_uu = sym(L_uu)
    exactly, Q_u = L_u and Q_uz = L_uz; U ~ 0.5 N(0, 1) for the bounded
    branches (bounds +-1).  Everything in `dtype`."""
    B, m, _ = A.shape
    n = N_STATE
    rng = np.random.default_rng([seed, m, 77])
    eye = np.broadcast_to(np.eye(n), (B, 1, n, n))
    L_uz = np.zeros((B, 1, m, n))
    L_uz[:, 0, :, :m] = np.eye(m)
    rec = dict(
        F_z=eye.copy(), F_u=np.zeros((B, 1, n, m)),
        L_z=0.1 * rng.standard_normal((B, 2, n)),
        L_u=rng.standard_normal((B, 1, m)),
        L_zz=np.broadcast_to(np.eye(n), (B, 2, n, n)).copy(), L_uz=L_uz,
        L_uu=A[:, None].copy(), U=0.5 * rng.standard_normal((B, 1, m)))
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in rec.items()}


ARG_NAMES = ("F_z", "F_u", "L_z", "L_u", "L_zz", "L_uz", "L_uu")


def oracle_probe(o, rec, reg, V_zz_reg, bounded):
    """The C oracle `o` on every trajectory of probe/sweep records ->
    k (B, N, m), K (B, N, m, n), status (B,)."""
    B = rec["F_z"].shape[0]
    m = rec["L_u"].shape[-1]
    ks, Ks, sts = [], [], []
    for b in range(B):
        kw = dict(reg=float(reg[b]), V_zz_reg=V_zz_reg)
        if bounded:
            kw.update(u_min=-np.ones(m), u_max=np.ones(m), U=rec["U"][b])
        k, K, st = o.backward(*[rec[nm][b] for nm in ARG_NAMES], **kw)
        ks.append(k)
        Ks.append(K)
        sts.append(st)
    return np.stack(ks), np.stack(Ks), np.asarray(sts)


# --------------------------------------------------------------------------
# float64 references


def eig_clamp_inverse(A, reg):
    """ilqr.py:631-636 in float64 numpy: (E / e) E^T with e < 0 -> 1e-12, then
    + reg.  Returns (inv, kappa of the unclamped input)."""
    lam, E = np.linalg.eigh(A)
    kappa = np.abs(lam).max() / np.abs(lam).min()
    e = np.where(lam < 0, 1e-12, lam) + reg
    return (E / e) @ E.T, kappa


def eig_clamp_matrix(A, reg):
    """ilqr.py:645: Q_uu_reg = (E * e) E^T of the bounded eig-clamp branch."""
    lam, E = np.linalg.eigh(A)
    e = np.where(lam < 0, 1e-12, lam) + reg
    return (E * e) @ E.T


def inverse_ratios(inv_got, k_got, A, reg, Q_u, eps):
    """The measure of the unbounded branches: the 2-norm error of the inverse
    and of k = -inv Q_u in units of eps * kappa (of the unclamped input),
    relative to ||inv||_2 and ||inv||_2 ||Q_u||."""
    inv, kappa = eig_clamp_inverse(A, reg)
    ninv = np.linalg.norm(inv, 2)
    r_inv = np.linalg.norm(np.asarray(inv_got, np.float64) - inv, 2) / ninv
    r_k = np.linalg.norm(np.asarray(k_got, np.float64) + inv @ Q_u) / (
        ninv * np.linalg.norm(Q_u))
    return r_inv / (eps * kappa), r_k / (eps * kappa)


@np.errstate(over="ignore", invalid="ignore", divide="ignore")
def eig_sweep_numpy(f, reg):
    """The unbounded eig-clamp sweep (ilqr.py:529-674) restated in float64
    numpy with the symmetric eigendecomposition, independent of the oracle's
    Jacobi.  `f` maps the record names to one trajectory's arrays.  Returns
    k (N, m), K (N, m, n) and the eigenvalues of every step's Q_uu (N, m)."""
    f = {nm: np.asarray(f[nm], np.float64) for nm in ARG_NAMES}
    N, n, m = f["F_u"].shape
    k, K, lams = np.empty((N, m)), np.empty((N, m, n)), np.empty((N, m))
    Vz, Vzz = f["L_z"][N], f["L_zz"][N]
    for t in range(N - 1, -1, -1):
        Fz, Fu = f["F_z"][t], f["F_u"][t]
        Qz = f["L_z"][t] + Fz.T @ Vz
        Qu = f["L_u"][t] + Fu.T @ Vz
        Qzz = f["L_zz"][t] + Fz.T @ Vzz @ Fz
        Qzz = 0.5 * (Qzz + Qzz.T)
        Quz = f["L_uz"][t] + Fu.T @ Vzz @ Fz
        Quu = f["L_uu"][t] + Fu.T @ Vzz @ Fu
        Quu = 0.5 * (Quu + Quu.T)
        if not np.isfinite(Quu).all():  # `eig` raises: nothing below t
            k[:t + 1], K[:t + 1], lams[:t + 1] = np.nan, np.nan, np.nan
            break
        e, E = np.linalg.eigh(Quu)
        lams[t] = e
        e = np.where(e < 0, 1e-12, e) + reg
        inv = (E / e) @ E.T
        kt, Kt = -inv @ Qu, -inv @ Quz
        k[t], K[t] = kt, Kt
        Vz = Qz + Kt.T @ Qu + Kt.T @ Quu @ kt + Quz.T @ kt
        Vzz = Qzz + Kt.T @ Quu @ Kt + Kt.T @ Quz + Quz.T @ Kt
        Vzz = 0.5 * (Vzz + Vzz.T)
    return k, K, lams


# --------------------------------------------------------------------------
# what a side (oracle or kernel) reached on a probe batch


def unbounded_worst(labels, A, reg, rec, k, K, eps):
    """Per family, the worst ratio (inverse and k together) of a side's
    one-step gains on an unbounded branch: -K[0][:, :m] is its inverse."""
    m = A.shape[-1]
    worst = {}
    for b, name in enumerate(labels):
        r_inv, r_k = inverse_ratios(-K[b, 0][:, :m], k[b, 0], A[b], reg[b],
                                    rec["L_u"][b, 0].astype(np.float64), eps)
        worst[name] = max(worst.get(name, 0.0), r_inv, r_k)
    return worst


def bounded_reference(A, reg, rec, V_zz_reg):
    """The float64 minimisers of a bounded probe batch (bounds +-1 around
    U), min 0.5 x Q_g x + Q_u x on [lower, upper], by enumeration of the 3^m
    active patterns (free / at lower / at upper): the free block is solved,
    and the pattern's KKT margin is the smallest of the free coordinates'
    distances to their bounds and of the clamped coordinates' gradients taken
    with the sign that keeps them clamped.  Q_g is positive definite, so
    exactly one pattern has a positive margin.  The enumeration runs over the
    whole batch at once: a clamped coordinate's row and column are replaced by
    the identity's, which leaves the free block's solve what it is.  Per
    trajectory: (k, K, free mask, margin, cond(Q_g)), with K =
    -solve(Q_g[ff], Q_uz[f]) on the free rows and 0 on the clamped ones
    (ilqr.py:602-617)."""
    B, m, _ = A.shape
    Q = np.stack([A[b] if V_zz_reg else eig_clamp_matrix(A[b], reg[b])
                  for b in range(B)])
    U = rec["U"][:, 0].astype(np.float64)
    c = rec["L_u"][:, 0].astype(np.float64)
    Quz = rec["L_uz"][:, 0].astype(np.float64)
    lower, upper = -1.0 - U, 1.0 - U
    best = np.full(B, -np.inf)
    bx, bf = np.zeros((B, m)), np.zeros((B, m), bool)
    eye = np.eye(m)
    for pat in itertools.product((0, 1, 2), repeat=m):
        pat = np.asarray(pat)
        f = pat == 0
        xc = np.where(f, 0.0, np.where(pat == 1, lower, upper))
        ff = np.outer(f, f)
        Qm = np.where(ff, Q, eye)
        rhs = np.where(f, -(c + np.einsum("bij,bj->bi", Q, xc)), xc)
        x = np.linalg.solve(Qm, rhs[..., None])[..., 0]
        g = np.einsum("bij,bj->bi", Q, x) + c
        margin = np.where(f, np.minimum(x - lower, upper - x),
                          np.where(pat == 1, g, -g)).min(axis=1)
        better = margin > best
        best = np.where(better, margin, best)
        bx[better], bf[better] = x[better], f
    out = []
    for b in range(B):
        f = bf[b]
        K = np.zeros_like(Quz[b])
        if f.any():
            K[f] = -np.linalg.solve(Q[b][np.ix_(f, f)], Quz[b][f])
        out.append((bx[b], K, f, best[b], float(np.linalg.cond(Q[b]))))
    return out


MARGIN = 1e-3  # cases whose best KKT margin is below this are left out


COND_TIER = 100.0


def bounded_errors(ref, k, K):
    """A side's one-step gains against `bounded_reference`, per case: arrays
    of |k - x| / max(1, |x|) (worst coordinate), the same for K, whether the
    free set - the rows of K that are not exactly zero - is the reference's,
    whether the case is kept (margin >= MARGIN), and cond(Q_g)."""
    B = len(ref)
    ek, eK, cond = np.zeros(B), np.zeros(B), np.zeros(B)
    same, kept = np.zeros(B, bool), np.zeros(B, bool)
    for b, (x, Kr, f, margin, c) in enumerate(ref):
        kb, Kb = k[b, 0].astype(np.float64), K[b, 0].astype(np.float64)
        ek[b] = (np.abs(kb - x) / np.maximum(1.0, np.abs(x))).max()
        eK[b] = (np.abs(Kb - Kr) / np.maximum(1.0, np.abs(Kr))).max()
        same[b] = np.array_equal((Kb != 0).any(axis=1), f)
        kept[b], cond[b] = margin >= MARGIN, c
    return ek, eK, same, kept, cond


def bounded_tiers(ref, k, K, agree=None):
    """The two readings of `bounded_errors`.
    "A", the kept cases with cond(Q_g) <= COND_TIER: worst errors of k and K
    as they are, and how many free sets are the reference's.
    "B", the kept cases above it (a clamped eigenvalue under reg = 1e-3,
    `graded`, `denorm`, the wider `spd`): the errors in units of cond(Q_g),
    the measure of the unbounded probes, over the cases in `agree` (default:
    the side's own agreeing cases).  The reference's BoxQP does not always
    end in the minimiser there: with two eigenvalues of 1e-3 under one of 2.7
    it stops on its objective test (result 4) 0.2 away along the flat
    directions with another free set, in float64 and float32 alike - on such
    a case the yardstick of a kernel is the oracle, not the minimiser, so
    the caller passes the oracle's agreeing cases (its "same") as `agree` and
    compares the free sets side by side.
    Returns {tier: (worst k, worst K, agreeing mask, tier mask), "same": the
    agreeing mask over all cases}."""
    ek, eK, same, kept, cond = bounded_errors(ref, k, K)
    out = {"same": same}
    for tier, mask, unit in (("A", kept & (cond <= COND_TIER), 1.0),
                             ("B", kept & (cond > COND_TIER), cond)):
        sel = mask & (same if agree is None else agree) if tier == "B" \
            else mask
        out[tier] = (float((ek / unit)[sel].max()) if sel.any() else 0.0,
                     float((eK / unit)[sel].max()) if sel.any() else 0.0,
                     same & mask, mask)
    return out


def boxqp_decidable(A, reg):
    """Mask of the cases a bounded eig-clamp probe keeps: all but those with
    an eigenvalue clamped at reg = 0.  There Q_g = E e E^T has an eigenvalue
    of 1e-12 next to ones of order 1, and rebuilt in floating point it carries
    an error of eps * max |e| in every entry: 1e-4 of that eigenvalue in
    float64, 1e5 times it in float32.  The float32 factorisation fails on
    about half of such Q_g, on either side, and the float64 minimiser moves
    by up to its own size; no reference can judge them.  The threshold that
    follows is cond(Q_g) * eps << 1 for the weaker format, cond(Q_g) << 1.7e7;
    every kept case with a clamped eigenvalue has cond(Q_g) <= 3 / 1e-3, and
    the clamped ones at reg = 0 have 5e11 or more.  `graded` and `denorm`
    stay at every reg: their Q_g is diagonally dominant and the rebuilt
    matrix accurate entry by entry.  (The excluded matrices stay in the
    unbounded probes.)"""
    lam_min = np.linalg.eigvalsh(A).min(axis=1)
    return ~((reg == 0.0) & (lam_min < 0))


# --------------------------------------------------------------------------
# the four probes, one batch each


def probe_batch(m, dtype, V_zz_reg, bounded):
    """(labels, A, reg, records) of the one-step probe of a gain branch: every
    family on the eig-clamp branches, the positive definite ones on the
    Cholesky branches.

    Unbounded: 300 and 120 trajectories in a launch.

    Bounded, float64: 600 (eig-clamp, less the 110 to 120 that
    `boxqp_decidable` takes out) and 300 (Cholesky).  Bounded, float32: 16
    times as many, 7800 and 4800.  The reason is that the bounded bars
    compare a side's WORST case with the oracle's, and the float32 BoxQP's
    error is heavy-tailed on both sides.  Of 2300 cases with cond(Q_g) <= 100
    per m, the float32 oracle is within 0.4 eps of the minimiser at the
    median and within 12 eps at the 99th percentile; 3 to 7 cases are beyond
    50 eps, and the worst are at 175 to 475 eps.  These are cases where the
    iteration stops on its objective test (constraint.py:172) one Newton step
    early.  In float32 that test, a decrease below 1e-8 |f|, is less than one
    ulp of f and fires on rounding.  Which cases stop early therefore depends
    on the last bit, and a batch has to be large enough for each side to meet
    several of them: at 300 cases the float32 oracle's own worst moves between
    6 and 110 eps from one m to the next.  On the Cholesky branch Q_g is exact
    and the tail thinner (1 case in 2234 for m = 4), so it takes more cases to
    meet it.  In float64 the test is far above rounding, both sides stop at
    the same iteration, and the small batch is enough."""
    big = np.dtype(dtype) == np.float32
    if bounded:
        names = PD_FAMILIES if V_zz_reg else FAMILIES
        labels, A, reg = cases(names, m, dtype,
                               per_family=(25 * (16 if big else 1)
                                           if V_zz_reg else
                                           20 * (16 if big else 1)))
        if not V_zz_reg:
            keep = boxqp_decidable(A, reg)
            labels = [l for l, kp in zip(labels, keep) if kp]
            A, reg = A[keep], reg[keep]
    elif V_zz_reg:
        labels, A, reg = cases(PD_FAMILIES, m, dtype, per_family=10)
    else:
        labels, A, reg = cases(FAMILIES, m, dtype, per_family=10)
    return labels, A, reg, probe_records(A, dtype)


BRANCHES = [("eig", False, False), ("chol", True, False),
            ("eig_box", False, True), ("chol_box", True, True)]


@functools.lru_cache(maxsize=None)
def oracle_side(m, dtype, V_zz_reg, bounded):
    """The oracle of `dtype` on a probe batch - computed once, shared by the
    CPU and the GPU tests, not to be written to."""
    batch = probe_batch(m, np_dtype(dtype), V_zz_reg, bounded)
    k, K, st = oracle_probe(orc.load(np_dtype(dtype)), batch[3], batch[2],
                            V_zz_reg, bounded)
    ref = bounded_reference(batch[1], batch[2], batch[3], V_zz_reg) \
        if bounded else None
    return batch, k, K, st, ref


# --------------------------------------------------------------------------
# sweeps in context: N = 6, B = 4

SHIFTED = (1, 4)  # steps of trajectory 1 whose L_uu gets -50 on an eigenvector


def sweep_records(n, m, dtype):
    """Synthetic records of four trajectories over N = 6 steps:
      0  positive definite throughout;
      1  L_uu - 50 v v^T (v an eigenvector of L_uu) at the steps SHIFTED, so
         that Q_uu is indefinite there;
      2  like 0 (meant to be launched inactive);
      3  positive definite, its nominal U at 0.95 of a bound of +-1 in every
         coordinate, so that the box is 0.05 away on one side and mixed free
         sets occur.
    Checked here with `eig_sweep_numpy` on trajectory 1: a negative
    eigenvalue of Q_uu at the shifted steps and min |lam| >= 1e-2 max |lam| at
    every step - at reg = 1 for all of them, at reg = 0 for the steps down to
    the first shifted one (step 4): there the clamp's 1e-12 makes gains of
    1e12 whose square enters V_zz, and no step below it is conditioned in any
    precision (`sweep_comparable` leaves those steps of that trajectory out
    of the gain comparisons; its status is compared all the same)."""
    rng = np.random.default_rng([n, m, 4])
    B, N = 4, 6
    R = 0.2 * rng.standard_normal((B, N + 1, n, n))
    Ru = 0.2 * rng.standard_normal((B, N, m, m))
    rec = dict(
        F_z=np.eye(n) + 0.05 * rng.standard_normal((B, N, n, n)),
        F_u=0.3 * rng.standard_normal((B, N, n, m)),
        L_z=rng.standard_normal((B, N + 1, n)),
        L_u=rng.standard_normal((B, N, m)),
        L_zz=np.eye(n) + R @ R.transpose(0, 1, 3, 2),
        L_uz=0.05 * rng.standard_normal((B, N, m, n)),
        L_uu=np.eye(m) + Ru @ Ru.transpose(0, 1, 3, 2),
        U=0.5 * rng.standard_normal((B, N, m)))
    rec["L_uu"] = 0.5 * (rec["L_uu"] + rec["L_uu"].transpose(0, 1, 3, 2))
    # trajectory 1: a weak coupling of the actions, or the -51 w w^T that a
    # clamped step adds to V_zz (w = Q_uz^T v) turns the next Q_uu negative in
    # turn and the sweep grows geometrically, reg = 1 included
    rec["F_u"][1] *= 0.1
    rec["L_uz"][1] *= 0.1
    for t in SHIFTED:
        lam, E = np.linalg.eigh(rec["L_uu"][1, t])
        v = E[:, t % m]
        rec["L_uu"][1, t] -= 50.0 * np.outer(v, v)
    rec["U"][3] = 0.95 * rng.choice([-1.0, 1.0], size=(N, m))
    rec = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in rec.items()}
    one = {nm: rec[nm][1] for nm in ARG_NAMES}
    for reg in (0.0, 1.0):
        lam = eig_sweep_numpy(one, reg)[2]
        steps = range(N) if reg else range(max(SHIFTED), N)
        for t in steps:
            a = np.abs(lam[t])
            assert a.min() >= 1e-2 * a.max(), (n, m, reg, t, lam[t])
        for t in SHIFTED:
            if t in steps:
                assert lam[t].min() < 0, (n, m, reg, t, lam[t])
    return rec


def sweep_comparable(b, reg):
    """First step whose gains of trajectory b are compared on the unbounded
    eig-clamp branch (see sweep_records): every step, but for trajectory 1 at
    reg = 0 those from its first clamp on."""
    return max(SHIFTED) if (b == 1 and reg == 0.0) else 0
