"""Records what the kernels of the Gaussian state encodings compute at small
shapes: pddp_qr_cost_derivs_*, the problem entry points (pddp_nominal_rollout_*,
pddp_derivs_*, pddp_line_search_*) under the four Gaussian encodings, and
pddp_bnn_jvp_moments_*.  It is the fixture of
tests/test_gauss_kernels_golden.py, which holds later builds to it byte for
byte.  Record it from the build the change under test STARTS from (its parent
commit), on an MI355X, never from the code under test:

    python tools/record_gauss_golden.py [tests/golden/gauss_kernels_parent.npz]

(PDDP_HIP_LIB selects the library, pddp_amd/_native.py; only C ABI entry points
are called.)

The cases are the smallest that reach every instantiation of the number types,
of the jittered Cholesky and of the cost on the augmented moments:

  qr       every (D, angles) of the dispatch table (tests/test_qr_cost_kernel.py
           SHAPES), m = 1 and 2, with and without bounds, B = 2, N = 2 (the
           terminal step is in).  The six states: the regimes (a) - (d) of that
           module, a state on a higher rung of the ladder and one for which no
           rung succeeds (the diagonal fall-back), see pair_state().
  problem  cartpole, pendulum, double cartpole, rendezvous under each Gaussian
           encoding, B = 2, N = 3, bounded: the rollout, the records and the
           line search (3 step sizes); trajectory 1 starts from a state on a
           higher rung, the records' trajectory 0 ends in a fall-back state.
  jvp      one (D, angles, m) per admitted (D, lanes) of
           tests/test_bnn_step_kernels.py, B = 2, P = 7, with and without
           eps_out; trajectory 1's particle cloud has rank one at a scale that
           absorbs every jitter: the ladder climbs to its end and the fall-back
           is taken.

Every input is made on the CPU in float64 from a fixed seed and rounded through
float32.  Every output buffer holds a sentinel before the launch.  Arrays of
up to 2 KB are stored whole, larger ones as 8-byte BLAKE2b digests of their
bytes, one per row of the first axis (tools/record_problem_golden.py)."""
import ctypes
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location(
    "record_problem_golden",
    os.path.join(ROOT, "tools", "record_problem_golden.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "gauss_kernels_parent.npz")
SENTINEL, STATE_SENTINEL = base.SENTINEL, base.STATE_SENTINEL
WHOLE_UP_TO = 2048  # bytes

# (D, angular indices): tests/test_qr_cost_kernel.py SHAPES
QR_SHAPES = [(2, ()), (2, (0,)), (2, (0, 1)),
             (4, ()), (4, (2,)), (4, (0, 3)),
             (6, ()), (6, (4,)), (6, (1, 2)), (6, (0, 5))]
QR_B, QR_N = 2, 2
ENCODINGS = ("UPPER_TRIANGULAR_CHOLESKY", "FULL_COVARIANCE_MATRIX",
             "VARIANCE_ONLY", "STANDARD_DEVIATION_ONLY")
PB_B, PB_N, PB_A = 2, 3, 3
# (D, angular indices, m): every (D, lanes) of tests/test_bnn_step_kernels.py
JVP_SHAPES = [(1, (0,), 1), (2, (0,), 1), (3, (1,), 2), (4, (2,), 1),
              (4, (2,), 2), (5, (0, 4), 1), (6, (1, 2), 1)]
JVP_B, JVP_P, JVP_N, JVP_T, NET_ROWS = 2, 7, 2, 1, 8
# seven particles on one line: zero sum, squares summing to 4 (P - 1)
RANK_ONE = np.array([-3.0, -2.0, -1.0, 1.0, 1.0, 2.0, 2.0])

CASES = ([("qr", t, "D%d_ang%s" % (D, "".join(map(str, a)) or "none"))
          for t in ("f32", "f64") for D, a in QR_SHAPES] +
         [("problem", t, "%s_%s" % (p, e)) for t in ("f32", "f64")
          for p in base.PROBLEMS for e in ENCODINGS] +
         [("jvp", t, "D%d_ang%s_m%d" % (D, "".join(map(str, a)), m))
          for t in ("f32", "f64") for D, a, m in JVP_SHAPES])


def case_name(family, dtype, key):
    return "%s_%s_%s" % (family, dtype, key)


def stored(a):
    a = np.ascontiguousarray(a)
    return a if a.nbytes <= WHOLE_UP_TO else base.digests(a, 1)


def r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def non_angular(D, ang):
    return [i for i in range(D) if i not in ang]


# ------------------------------------------------------------------ states --
def factors(rng, count, D, regime="a", ang=()):
    """(mean [count, D], U [count, D, D] upper) of a regime of
    tests/test_qr_cost_kernel.py: (a) diagonal^2 in [0.02, 0.07],
    off-diagonals 0.05 randn; (b) diagonal^2 in [1e-6, 1e-5], off-diagonals
    1e-3 randn; (c) a zero factor; (d) angle variances in [4, 9], angle means
    50 randn."""
    mean = rng.randn(count, D)
    d2 = rng.rand(count, D)
    off = np.triu(rng.randn(count, D, D), 1)
    if regime in "ad":
        diag, off = np.sqrt(0.02 + 0.05 * d2), 0.05 * off
    elif regime == "b":
        diag, off = np.sqrt(1e-6 + 9e-6 * d2), 1e-3 * off
    else:
        diag, off = 0.0 * d2, 0.0 * off
    U = off + diag[:, :, None] * np.eye(D)
    if regime == "d":
        for a in ang:
            target = 4.0 + 5.0 * rng.rand(count)
            U[:, :, a] *= np.sqrt(target / (U[:, :, a] ** 2).sum(-1))[:, None]
            mean[:, a] = 50.0 * rng.randn(count)
    return mean, U


def pair_state(U, p, q, a):
    """Columns p and q of one factor become (a, 0, ...): C[p][p] = C[p][q] =
    C[q][q] = a^2 and no other entry of their rows, so the second of the two
    pivots is (a^2 + jitter) - a^2 at every attempt - positive from the rung
    that a^2 does not absorb, never when a^2 absorbs 10."""
    U[:, p] = 0.0
    U[:, q] = 0.0
    U[0, :] = 0.0
    U[0, p] = U[0, q] = a
    return U


# (the rung the pair reaches: 1 + 1e-12 is 1 in f32, 2^40 + 1e-12 is 2^40 in
# f64; 2^40 + 10 is 2^40 in f32, 2^80 + 10 is 2^80 in f64)
CLIMB = {"f32": 1.0, "f64": 2.0 ** 20}
FALLBACK = {"f32": 2.0 ** 20, "f64": 2.0 ** 40}


def encoded(mean, U, enc="UPPER_TRIANGULAR_CHOLESKY"):
    """[count, n] of (mean, U^T U) under an encoding, rounded through f32."""
    D = mean.shape[-1]
    U = r32(U)
    C = np.einsum("...ki,...kj->...ij", U, U)
    dg = np.einsum("...ii->...i", C)
    if enc == "UPPER_TRIANGULAR_CHOLESKY":
        iu = np.triu_indices(D)
        oth = U[..., iu[0], iu[1]]
    elif enc == "FULL_COVARIANCE_MATRIX":
        oth = C.reshape(*C.shape[:-2], D * D)
    elif enc == "VARIANCE_ONLY":
        oth = dg
    else:
        oth = np.sqrt(dg)
    return r32(np.concatenate([mean, oth], -1))


def qr_states(D, ang, dtype, seed):
    """(mean, U) of the six states of one qr case, [B, N + 1] in row-major
    order: regimes a, b, the climbing pair, d, c, the fall-back pair (without
    two non-angular dimensions: regime b twice more)."""
    rng = np.random.RandomState(seed)
    non = non_angular(D, ang)
    means, Us = [], []
    for k, regime in enumerate("abxdcy"):
        m_, U_ = factors(rng, 1, D, {"x": "a", "y": "a"}.get(regime, regime),
                         ang)
        if regime in "xy":
            if len(non) >= 2:
                a = (CLIMB if regime == "x" else FALLBACK)[dtype]
                pair_state(U_[0], non[0], non[1], a)
            else:
                m_, U_ = factors(rng, 1, D, "b", ang)
        means.append(m_[0])
        Us.append(U_[0])
    return np.stack(means), np.stack(Us)


def qr_constants(D, ang, m, rng):
    """Q = A^T A + 0.1 I plus a skew part (asymmetric), Q_term = 3 Q^T, R with
    an off-diagonal entry, non-zero goals, bounds."""
    NA = D + len(ang)
    A = rng.randn(NA, NA)
    Q = A.T @ A + 0.1 * np.eye(NA)
    S = rng.randn(NA, NA)
    Q = r32(Q + 0.3 * (S - S.T))
    return dict(Q=Q, Q_term=r32(3.0 * Q.T),
                R=np.array([[0.75, 0.25], [0.25, 0.5]])[:m, :m],
                x_goal=r32(0.5 * rng.randn(NA)),
                u_goal=np.array([0.25, -0.125])[:m],
                u_min=np.array([-0.75, -0.5])[:m],
                u_max=np.array([0.875, 0.625])[:m])


def problem_states(problem, dtype, count, seed, climb=None, fallback=None):
    """(mean, U) of `count` states around the model's starting point, regime
    (a); state `climb` on a higher rung and state `fallback` beyond the ladder
    (a pendulum has one non-angular dimension: regime (b) there)."""
    from pddp_amd.examples.problems import SampleProblems
    mc = SampleProblems[problem.upper()].get_model_class()
    D = mc.state_size
    ang = tuple(int(i) for i in mc.angular_indices)
    non = non_angular(D, ang)
    rng = np.random.RandomState(seed)
    mean, U = factors(rng, count, D, "a", ang)
    mean = np.asarray(base.MEAN0[problem], np.float64) + 0.1 * mean
    small = factors(rng, 2, D, "b", ang)[1]
    for k, a in ((climb, CLIMB[dtype]), (fallback, FALLBACK[dtype])):
        if k is None:
            continue
        if len(non) >= 2:
            pair_state(U[k], non[0], non[1], a)
        else:
            U[k] = small[0 if k == climb else 1]
    return mean, U


# --------------------------------------------------------------- the cases --
def run_case(family, dtype, key):
    """{name: array as stored} of one case."""
    import torch
    from pddp_amd import _native as N_
    td = torch.float32 if dtype == "f32" else torch.float64
    lib, p, st = N_.lib(), N_.ptr, N_.stream_handle()

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(r32(a))).to(td).cuda()

    def full(*shape):
        return torch.full(shape, SENTINEL, dtype=td, device="cuda")

    def host(t):  # (waits for the stream)
        return stored(t.detach().cpu().numpy())

    def call(name, *args):
        fn = getattr(lib, name + "_" + dtype)
        N_.check(fn(*args), name)

    def shape_into(s, D, ang):
        non = non_angular(D, ang)
        s.D, s.n_ang, s.n_non = D, len(ang), len(non)
        for i, v in enumerate(ang):
            s.ang[i] = v
        for i, v in enumerate(non):
            s.non[i] = v

    out = {}
    idx = [c for c in CASES if c[0] == family and c[1] == "f32"].index(
        (family, "f32", key))
    if family == "qr":
        D, ang = QR_SHAPES[idx]
        B, N, n = QR_B, QR_N, D + D * (D + 1) // 2
        mean, U = qr_states(D, ang, dtype, 300 + idx)
        Z = dev(encoded(mean, U).reshape(B, N + 1, n))
        for m in (1, 2):
            rng = np.random.RandomState(400 + 10 * idx + m)
            c = {k: dev(v) for k, v in qr_constants(D, ang, m, rng).items()}
            Ua = rng.rand(B, N, m) - 0.5
            Ua[0, 1, 0], Ua[1, 0, m - 1] = -2.0, 2.0  # beyond the bounds
            Ua = dev(Ua)
            for bounds in (True, False):
                o = dict(L=full(B * (N + 1)), L_z=full(B * (N + 1), n),
                         L_zz=full(B * (N + 1), n, n), L_u=full(B * N, m),
                         L_uz=full(B * N, m, n), L_uu=full(B * N, m, m))
                s = N_.QrCost()
                s.B, s.N, s.m = B, N, m
                shape_into(s, D, ang)
                for k, t in list(c.items()) + list(o.items()):
                    if k in ("u_min", "u_max") and not bounds:
                        continue
                    setattr(s, k, p(t))
                s.Z, s.U = p(Z), p(Ua)
                call("pddp_qr_cost_derivs", ctypes.byref(s), st)
                for k, t in o.items():
                    out["m%d_%s/%s" % (m, "bounded" if bounds else "free",
                                       k)] = host(t)
    elif family == "problem":
        from pddp_amd.examples.problems import SampleProblems
        from pddp_amd.utils.encoding import StateEncoding
        problem = [q for q in base.PROBLEMS if key.startswith(q + "_")][0]
        enc = key[len(problem) + 1:]
        sp = SampleProblems[problem.upper()]
        prob = sp.get_model_class()(base.DT[problem]).native_problem(
            StateEncoding[enc], sp.get_cost_class()())
        n, m = prob.encoded_size, prob.action_size
        S, GS = N_.record_layout(n, m).stride, m + m * n
        B, N, A = PB_B, PB_N, PB_A
        pp = ctypes.addressof(prob)
        seed = 500 + 10 * base.PROBLEMS.index(problem)
        rng = np.random.RandomState(seed + 9)
        bound = base.BOUND[problem]
        u_min, u_max = dev(np.full(m, -bound)), dev(np.full(m, bound))
        # -- nominal rollout: trajectory 1 starts on a higher rung
        z0 = dev(encoded(*problem_states(problem, dtype, B, seed, climb=1),
                         enc))
        Ua = dev(0.6 * bound * rng.randn(B, N, m))
        Z = full(B, N + 1, n)
        call("pddp_nominal_rollout", pp, B, N, p(z0), p(Ua), p(u_min),
             p(u_max), None, p(Z), st)
        out["rollout/Z"] = host(Z)
        # -- records: (1, 1) on a higher rung, (0, N) beyond the ladder
        Zs = dev(encoded(*problem_states(
            problem, dtype, B * (N + 1), seed + 1, climb=(N + 1) + 1,
            fallback=N), enc).reshape(B, N + 1, n))
        rec, L, J = full(B, N + 1, S), full(B, N + 1), full(B)
        state = torch.full((B,), STATE_SENTINEL, dtype=torch.int32,
                           device="cuda")
        call("pddp_derivs", pp, B, N, p(Zs), p(Ua), p(u_min), p(u_max), None,
             p(rec), p(L), p(J), p(state), st)
        out["records/rec"] = base.digests(rec.cpu().numpy(), 2)
        out["records/L_J"] = np.concatenate(
            [L.cpu().numpy(), J.cpu().numpy()[:, None]], axis=1)
        out["records/state"] = state.cpu().numpy()
        # -- line search: trajectory 1's nominal starts on a higher rung
        Zn = dev(encoded(*problem_states(
            problem, dtype, B * (N + 1), seed + 2, climb=N + 1),
            enc).reshape(B, N + 1, n))
        gains = dev(0.1 * rng.randn(B, N, GS))
        alphas = dev(np.array([1.0, 0.5, 0.25]))
        Zc, Uc, Jc = full(B, N + 1, A, n), full(B, N, A, m), full(B, A)
        call("pddp_line_search", pp, B, N, A, p(Zn), p(Ua), p(gains),
             p(alphas), p(u_min), p(u_max), None, None, p(Zc), p(Uc), p(Jc),
             st)
        out["search/Jc"] = Jc.cpu().numpy()
        out["search/Zc"], out["search/Uc"] = host(Zc), host(Uc)
    else:
        D, ang, m = JVP_SHAPES[idx]
        B, P, N, t = JVP_B, JVP_P, JVP_N, JVP_T
        n, NA = D + D * (D + 1) // 2, D + len(ang)
        rng = np.random.RandomState(700 + idx)
        mean, U = factors(rng, B * (N + 1), D)
        Z = r32(encoded(mean, U).reshape(B, N + 1, n))
        e = rng.randn(B, P, D)
        Xp = np.zeros((B, P, D))
        iu = np.triu_indices(D)
        U0 = np.zeros((D, D))
        U0[iu] = Z[0, t, D:]
        Xp[0] = Z[0, t, :D] + e[0] @ U0
        # (every later addition - |dX_mean|, |std eps| < 1 - is absorbed)
        scale = 2.0 ** 24 if dtype == "f32" else 2.0 ** 60
        Xp[1] = scale * RANK_ONE[:, None]
        Ua = rng.rand(B, N, m) - 0.5
        Ua[1, t, m - 1] = 2.0
        c = dict(X_mean=0.1 * rng.randn(NA + m),
                 X_std_inv=0.5 + rng.rand(NA + m),
                 dX_mean=0.01 * rng.randn(D), dX_std=0.03 + 0.05 * rng.rand(D),
                 u_min=np.array([-0.75, -0.5])[:m],
                 u_max=np.array([0.875, 0.625])[:m])
        keep = {k: dev(v) for k, v in c.items()}
        keep.update(Z=dev(Z), U=dev(Ua), Xp=dev(Xp), eps=dev(e))
        for ups in (False, True):
            od = 2 * D if ups else D
            y = np.zeros((B * P, NET_ROWS, od))
            y[:, :1 + D + m, :D] = rng.randn(B * P, 1 + D + m, D)
            y[P:, 0, :D] = 0.0  # the rank-one cloud stays on its line
            if ups:
                y[:, 0, D:] = -1.0 + 0.3 * rng.randn(B * P, D)
                y[:, 1:1 + D + m, D:] = rng.randn(B * P, D + m, D)
            keep["net_out"] = dev(y)
            keep["eps_out"] = dev(rng.randn(P, D)) if ups else None
            o = dict(Xp_next=full(B, P, D), Z_next=full(B, n),
                     F_z=full(B, N, n, n), F_u=full(B, N, n, m))
            s = N_.BnnJvp()
            s.B, s.P, s.N, s.t, s.m = B, P, N, t, m
            shape_into(s, D, ang)
            s.in_dim, s.out_dim, s.independent_noise = NA + m, od, 0
            F = full(B * P, NET_ROWS, NA + m)  # (the features' output)
            for k, v in list(keep.items()) + list(o.items()) + [("F", F)]:
                setattr(s, k, p(v))
            call("pddp_bnn_jvp_moments", ctypes.byref(s), st)
            for k, v in o.items():
                out["%s/%s" % ("eps_out" if ups else "mean_only", k)] = host(v)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    blob = {}
    for case in CASES:
        for k, v in run_case(*case).items():
            blob[case_name(*case) + "/" + k] = v
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **blob)
    print("%d cases, %d arrays, %d bytes -> %s" % (
        len(CASES), len(blob), os.path.getsize(out), out))


if __name__ == "__main__":
    main()
