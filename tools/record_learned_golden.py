"""Records what the learned-model entry points compute at small shapes: the GP
step, its masked form and its rollout (pddp_gp_step_*, _masked_*,
pddp_gp_rollout_*) and the fused Bayesian network in f32 and f64 (all eight
pddp_bnn_mlp_* entry points).  It is the fixture of
tests/test_learned_kernels_golden.py, which holds later builds to it byte for
byte.  Record it from the build the change under test STARTS from (its parent
commit), on an MI355X, never from the code under test:

    python tools/record_learned_golden.py [tests/golden/learned_kernels_parent.npz]

(PDDP_HIP_LIB selects the library, pddp_amd/_native.py; only C ABI entry points
are called.)

The shapes are the ones at which the HOST code of these entry points can go
wrong: every branch of the GP's choice of form (resident; chunked with the
rows in slices of 3, 3, 1 and 4, 2 and the terminal launch in one slice), a
mask, every built (state_size, d) pair, every encoding; of the network every
H, both W1 widths, a tile remainder, a live_rows scalar, every packing of the
forward-mode groups.

Every input is made on the CPU in float64 from a fixed seed, out of additions,
multiplications and divisions alone (no library's exp or inverse, which may
differ between machines), rounded through float32 and converted.  The GP's
inverse is that of a small SPD kernel matrix (rational quadratic, noise on the
diagonal) by Gauss-Jordan elimination.  Every output buffer holds a sentinel
before the launch, so rows that are skipped are part of the bytes.  Stored
whole: arrays of up to 2 KB.  Larger arrays - the Jacobians Fz and Fu, the
rollout's Zc, the network's Y at the larger shapes - are stored as 8-byte
BLAKE2b digests of their bytes, one per row of the first axis."""
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

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden",
                           "learned_kernels_parent.npz")
SENTINEL = base.SENTINEL
WHOLE_UP_TO = 2048  # bytes

# (state_size, angles, non-angles, actions, encoding): d = n_non + 2 n_ang + m
SYSTEMS = {
    "6x9": (6, (1, 2), (0, 3, 4, 5), 1, 1),  # double cartpole, Cholesky
    "4x6": (4, (2,), (0, 1, 3), 1, 2),       # cartpole, variances
    "2x4": (2, (0,), (1,), 1, 3),            # pendulum, standard deviations
}
# name: (system, M, R, rows_per_mask or 0, (force_chunk, force_rows) or None)
GP_STEP = {
    "6x9_resident": ("6x9", 66, 7, 0, None),
    "6x9_masked": ("6x9", 66, 7, 3, None),
    "6x9_chunked": ("6x9", 66, 7, 0, (8, 3)),
    "4x6": ("4x6", 5, 2, 0, None),
    "2x4": ("2x4", 2, 1, 0, None),
}
# name: (system, M, B, N, A, bounded, (force_chunk, force_rows) or None)
GP_ROLLOUT = {
    "6x9_resident": ("6x9", 66, 2, 3, 3, True, None),
    "6x9_chunked": ("6x9", 66, 2, 3, 3, True, (8, 4)),
    "2x4": ("2x4", 2, 1, 1, 1, False, None),
}
# name: (H, in_dim, out_dim, group, live, R, live_rows or None); group 0: the
# plain network.  P = 7 throughout; H = 64 / 128 add only the switch
BNN_P = 7


def _bnn_cases(f64):
    plain_R = 17 if f64 else 33
    c = {
        "H200_plain": (200, 6, 4, 0, 0, plain_R, None),
        "H200_plain_wide": (200, 15, 16, 0, 0, plain_R, None),
        "H200_plain_rows": (200, 6, 4, 0, 0, plain_R, 12 if f64 else 20),
        "H64_plain": (64, 6, 4, 0, 0, plain_R, None),
        "H128_plain_wide": (128, 15, 16, 0, 0, plain_R, None),
        "H64_jvp_8_6": (64, 6, 4, 8, 6, 40, None),
        "H128_jvp_8_6_wide": (128, 15, 16, 8, 6, 40, None),
        "H200_jvp_8_6_wide": (200, 15, 16, 8, 6, 40, None),
        "H200_jvp_16_16_wide": (200, 15, 16, 16, 16, 80, None),
        "H200_jvp_8_6_rows": (200, 6, 4, 8, 6, 40, 24),
    }
    groups = ((8, 4), (8, 6), (8, 8), (16, 16)) + (() if f64 else ((32, 32),))
    for g, l in groups:
        c["H200_jvp_%d_%d" % (g, l)] = (200, 6, 4, g, l, 5 * g, None)
    return c


BNN = {"f32": _bnn_cases(False), "f64": _bnn_cases(True)}

CASES = ([("gp_step", t, k) for t in ("f32", "f64") for k in GP_STEP] +
         [("gp_rollout", t, k) for t in ("f32", "f64") for k in GP_ROLLOUT] +
         [("bnn", t, k) for t in ("f32", "f64") for k in BNN[t]])


def case_name(family, dtype, key):
    return "%s_%s_%s" % (family, dtype, key)


def stored(a):
    """The array as the fixture holds it (see the module's text)."""
    a = np.ascontiguousarray(a)
    return a if a.nbytes <= WHOLE_UP_TO else base.digests(a, 1)


def spd_inverse(K):
    """Gauss-Jordan without pivoting (K is SPD), elementwise operations only."""
    M = K.shape[0]
    A = np.concatenate([K.copy(), np.eye(M)], axis=1)
    for i in range(M):
        A[i] = A[i] / A[i, i]
        f = A[:, i].copy()
        f[i] = 0.0
        A = A - f[:, None] * A[i][None, :]
    return A[:, M:]


def gp_arrays(system, M, seed):
    """float64 arrays of a pddp_gp_model (include/pddp_hip.h) and its sizes."""
    E, ang, non, m, enc = SYSTEMS[system]
    d = len(non) + 2 * len(ang) + m
    rng = np.random.RandomState(seed)
    Xt = 0.8 * rng.randn(M, d)
    ell = 1.5 + rng.rand(E, d)
    sf2, sn2 = 0.5 + 0.5 * rng.rand(E), 0.01 + 0.01 * rng.rand(E)
    y = 0.3 * rng.randn(E, M)
    iL = 1.0 / (ell * ell)
    Kinv, beta = np.zeros((E, M, M)), np.zeros((E, M))
    for a in range(E):
        r2 = np.zeros((M, M))
        for p in range(d):
            diff = Xt[:, p][:, None] - Xt[:, p][None, :]
            r2 = r2 + diff * diff * iL[a, p]
        Ki = spd_inverse(sf2[a] / (1.0 + 0.5 * r2) + sn2[a] * np.eye(M))
        Kinv[a] = 0.5 * (Ki + Ki.T)
        for j in range(M):
            beta[a] = beta[a] + Kinv[a][:, j] * y[a, j]
    # the pairs of training points (models/gp.py _native_model)
    mp, ps = ((M + 3) // 4) * 2, (2 * d + 3) & ~3
    xp = np.zeros((2 * mp, d))
    xp[:M] = Xt
    pairs = np.zeros((mp, ps))
    pairs[:, :2 * d] = xp.reshape(mp, 2, d).transpose(0, 2, 1).reshape(mp, -1)
    bp = np.zeros((E, 2 * mp))
    bp[:, :M] = beta
    n = {1: E + E * (E + 1) // 2, 2: 2 * E, 3: 2 * E, 4: E}[enc]
    return dict(Xt=Xt, Xt_pairs=pairs, beta=beta, beta_pairs=bp, Kinv=Kinv,
                inv_ell2=iL, sf2=sf2, sn2=sn2), (E, ang, non, m, enc, n)


def gp_states(rng, shape, E, enc):
    """Encoded state distributions [*shape, n]: small means, and as the
    encoding holds it a positive-definite covariance."""
    mean = 0.3 * rng.randn(*shape, E)
    if enc == 1:  # the rows of an upper-triangular factor, diagonal first
        rows = []
        for r in range(E):
            row = 0.02 * rng.randn(*shape, E - r)
            row[..., 0] = 0.05 + 0.1 * rng.rand(*shape)
            rows.append(row)
        return np.concatenate([mean] + rows, axis=-1)
    if enc in (2, 3):
        return np.concatenate([mean, 0.02 + 0.05 * rng.rand(*shape, E)], -1)
    return mean


class _Forced:
    """pddp_gp_step_force_chunk / _force_rows_per_launch for one block."""

    def __init__(self, lib, force):
        self.lib, self.force = lib, force

    def __enter__(self):
        if self.force is not None:
            self.chunk = self.lib.pddp_gp_step_force_chunk(self.force[0])
            self.rows = self.lib.pddp_gp_step_force_rows_per_launch(
                self.force[1])

    def __exit__(self, *exc):
        if self.force is not None:
            self.lib.pddp_gp_step_force_chunk(self.chunk)
            self.lib.pddp_gp_step_force_rows_per_launch(self.rows)


def run_case(family, dtype, key):
    """{name: array as stored} of one case."""
    import torch
    from pddp_amd import _native as N_
    td = torch.float32 if dtype == "f32" else torch.float64
    lib, p, st = N_.lib(), N_.ptr, N_.stream_handle()

    def dev(a):
        a = np.ascontiguousarray(a).astype(np.float32).astype(np.float64)
        return torch.from_numpy(a).to(td).cuda()

    def full(*shape):
        return torch.full(shape, SENTINEL, dtype=td, device="cuda")

    def host(t):  # (waits for the stream)
        return stored(t.detach().cpu().numpy())

    def call(name, *args):
        fn = getattr(lib, name)
        N_.check(fn(*args), name)

    def model_of(system, M, seed):
        arrays, (E, ang, non, m, enc, n) = gp_arrays(system, M, seed)
        keep = {k: dev(v) for k, v in arrays.items()}
        g = N_.GpModel()
        g.state_size, g.action_size, g.M, g.encoding = E, m, M, enc
        g.n_ang, g.n_non = len(ang), len(non)
        for i, v in enumerate(ang):
            g.ang[i] = v
        for i, v in enumerate(non):
            g.non[i] = v
        for k, t in keep.items():
            setattr(g, k, p(t))
        return g, keep, (E, m, enc, n)

    out = {}
    if family == "gp_step":
        system, M, R, per, force = GP_STEP[key]
        g, keep, (E, m, enc, n) = model_of(system, M, 21)
        rng = np.random.RandomState(22)
        z, u = dev(gp_states(rng, (R,), E, enc)), dev(0.5 * rng.randn(R, m))
        mask = None
        if per:  # the middle group is skipped
            groups = (R + per - 1) // per
            mask = torch.ones(groups, dtype=torch.uint8)
            mask[groups // 2] = 0
            mask = mask.cuda()
        with _Forced(lib, force):
            for jac in (0, 1):
                zn = full(R, n)
                Fz = full(R, n, n) if jac else None
                Fu = full(R, n, m) if jac else None
                lead = (ctypes.byref(g), R, p(z), p(u), p(zn), p(Fz), p(Fu))
                if per:
                    call("pddp_gp_step_masked_" + dtype, *lead, p(mask), per,
                         st)
                else:
                    call("pddp_gp_step_" + dtype, *lead, st)
                out["jac%d/z_next" % jac] = host(zn)
                if jac:
                    out["jac1/Fz"], out["jac1/Fu"] = host(Fz), host(Fu)
    elif family == "gp_rollout":
        system, M, B, N, A, bounded, force = GP_ROLLOUT[key]
        g, keep, (E, m, enc, n) = model_of(system, M, 23)
        na = g.n_non + 2 * g.n_ang
        rng = np.random.RandomState(24)
        spd = lambda k: (lambda W: (W[:, :, None] * W[:, None, :]).sum(0) / k
                         + 0.5 * np.eye(k))(rng.randn(k, k))
        t_ = dict(
            Z=dev(gp_states(rng, (B, N + 1), E, enc)),
            U=dev(0.5 * rng.randn(B, N, m)),
            gains=dev(0.1 * rng.randn(B, N, m + m * n)),
            alphas=dev(0.5 ** np.arange(A)),
            Q=dev(spd(na)), Q_term=dev(2.0 * spd(na)), R=dev(0.1 * spd(m)),
            x_goal=dev(0.1 * rng.randn(na)), u_goal=dev(0.1 * rng.randn(m)),
            Zc=full(B, N + 1, A, n), Uc=full(B, N, A, m), Jc=full(B, A))
        if bounded:  # (a part of the actions lies beyond)
            t_["u_min"], t_["u_max"] = dev(-0.4 * np.ones(m)), dev(
                0.4 * np.ones(m))
        if B > 1:  # nobody dropped; the sweep of trajectory 1 failed
            t_["active"] = torch.ones(B, dtype=torch.uint8).cuda()
            status = torch.zeros(B, dtype=torch.int32)
            status[1] = 1
            t_["bwd_status"] = status.cuda()
        r = N_.GpRollout()
        r.B, r.N, r.A = B, N, A
        for k, t in t_.items():
            setattr(r, k, p(t))
        with _Forced(lib, force):
            call("pddp_gp_rollout_" + dtype, ctypes.byref(g), ctypes.byref(r),
                 st)
        for k in ("Zc", "Uc", "Jc"):
            out[k] = host(t_[k])
    else:
        H, in_dim, out_dim, group, live, R, live_rows = BNN[dtype][key]
        rng = np.random.RandomState(25)
        P = BNN_P
        w = [dev(a) for a in (
            rng.randn(R, in_dim),
            rng.randn(H, in_dim) / 3.0, 0.1 * rng.randn(H),
            1.25 * (rng.rand(P, H) < 0.8),
            rng.randn(H, H) / 12.0, 0.1 * rng.randn(H),
            1.25 * (rng.rand(P, H) < 0.8),
            rng.randn(out_dim, H) / 12.0, 0.1 * rng.randn(out_dim))]
        Y = full(R, out_dim)
        rows = None if live_rows is None else torch.tensor(
            [live_rows], dtype=torch.int32).cuda()
        ptrs = [p(t) for t in w] + [p(Y)]
        if group == 0:
            if rows is None:
                call("pddp_bnn_mlp_" + dtype, R, P, in_dim, H, out_dim, *ptrs,
                     st)
            else:
                call("pddp_bnn_mlp_rows_" + dtype, R, P, in_dim, H, out_dim,
                     *ptrs, p(rows), st)
        elif dtype == "f64" or rows is not None:
            call("pddp_bnn_mlp_jvp_rows_" + dtype, R, P, group, live, in_dim,
                 H, out_dim, *ptrs, p(rows), st)
        elif live == group:
            call("pddp_bnn_mlp_jvp_f32", R, P, group, in_dim, H, out_dim,
                 *ptrs, st)
        else:
            call("pddp_bnn_mlp_jvp_live_f32", R, P, group, live, in_dim, H,
                 out_dim, *ptrs, st)
        out["Y"] = host(Y)
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
