"""One call of each BNN entry point outside the network, restated in plain
torch on the CPU - the yardstick of test_bnn_step_kernels.py for
`pddp_bnn_moment_step_*` (csrc/bnn_rollout.hip) and `pddp_bnn_jvp_features_*` /
`pddp_bnn_jvp_moments_*` (csrc/bnn_jvp.hip).  Written from the header comments
of include/pddp_hip.h (`pddp_bnn_step`, `pddp_bnn_jvp`) and of the two .hip
files; the cost on the augmented moments is qr_cost_model's.  It shares no
code with pddp_amd.utils.encoding, utils.angular or models.bnn.

Every function works in the dtype of the tensors it is given (float64: the
reference value; float32: what the same formulas give in single precision, the
yardstick of the f32 bars) and takes its arguments as a dict `a` named after
the struct's fields, tensors in the struct's layouts:

  step(a, t)          Z [B, N+1, n], U [B, N, m], gains [B, N, m + m n],
                      alphas [A], Xp [B, A, P, D], J [B, A], net_out [rows,
                      out_dim] (t > 0), eps_out [P, D] or None, ...
  jvp_features(a, t)  Xp [B, P, D], ...
  jvp_moments(a, t)   net_out [rows, 8, out_dim], eps [B, P, D], ...

What a call does not write is NaN in the result.  The Cholesky differential is
not coded here: jvp_moments() builds the particle tangents per direction as
the header states them and differentiates the model's own encode() with
torch.autograd.functional.jacobian.

`mutate` breaks the model on purpose, for the test that shows the comparison
can fail: "cov_P" (covariance over P), "phi_diag" (the differential of the
factor without the halved diagonal of Phi - the one place where that
differential is written out, wrongly), "sincos_swap" (the two feature slots of
an angle exchanged), "no_alpha" (`alpha k` applied as `k`).  Not a test and
not a conftest: imported by the tests."""
import numpy as np
import torch

import qr_cost_model as qm

NET_ROWS = 8  # network rows per (trajectory, particle) of the jvp pair


def _np(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def upper_of(z, D):
    """The factor U [D, D] of z = mean | triu(U) row by row."""
    U = z.new_zeros(D, D)
    iu = torch.triu_indices(D, D)
    U[iu[0], iu[1]] = z[D:]
    return U


def encode(mean, cov):
    """mean [D], cov [D, D] -> (z [n], rung): the upper Cholesky factor of
    `cov + rung I` at the first rung of ladder() at which a sequential
    factorisation in cov's dtype succeeds; the diagonal of standard deviations
    (rung None) when none does."""
    D = mean.shape[-1]
    r = qm.rung(cov.detach().numpy(), _np(cov.dtype))
    if r is None:
        U = torch.diag(torch.diagonal(cov).sqrt())
    else:
        U = torch.linalg.cholesky(
            cov + r * torch.eye(D, dtype=cov.dtype), upper=True)
    iu = torch.triu_indices(D, D)
    return torch.cat([mean, U[iu[0], iu[1]]]), r


def particle_moments(X, mutate=None):
    """X [P, D] -> mean [D], unbiased covariance [D, D]."""
    P = X.shape[0]
    mean = X.sum(0) / P
    d = X - mean
    return mean, d.t() @ d / (P if mutate == "cov_P" else P - 1)


def _features(a, x, u, mutate=None):
    """x [P, D], u [m] -> the network's input rows [P, in_dim]: non-angular
    states in the order of `non`, (sin, cos) per angle, the action last."""
    ang, non = list(a["ang"]), list(a["non"])
    nn, m = len(non), a["m"]
    feat = x.new_zeros(x.shape[0], nn + 2 * len(ang) + m)
    for i, d in enumerate(non):
        feat[:, i] = x[:, d]
    for k, d in enumerate(ang):
        s, c = torch.sin(x[:, d]), torch.cos(x[:, d])
        if mutate == "sincos_swap":
            s, c = c, s
        feat[:, nn + 2 * k], feat[:, nn + 2 * k + 1] = s, c
    feat[:, nn + 2 * len(ang):] = u
    return (feat - a["X_mean"]) * a["X_std_inv"]


def _clamp(a, u):
    if a.get("u_min") is None or a.get("u_max") is None:
        return u
    return torch.maximum(torch.minimum(u, a["u_max"]), a["u_min"])


def _output_particles(a, x, y, eps_out):
    """x [P, D], network rows y [P, out_dim] -> (x + dx, std eps [P, D])."""
    D = x.shape[1]
    dx = y[:, :D] * a["dX_std"] + a["dX_mean"]
    stdeps = torch.zeros_like(x)
    if eps_out is not None:
        stdeps = torch.exp(y[:, D:2 * D] + torch.log(a["dX_std"])) * eps_out
        dx = dx + stdeps
    return x + dx, stdeps


def _aug_rungs(a, z):
    """z [K, n] -> the rung of the augmented covariance per row, evaluated in
    z's dtype with `q expm1(c)` and with the difference of exponentials."""
    D, ang, non = a["D"], list(a["ang"]), list(a["non"])
    out = []
    for exact in (True, False):
        _, Ca = qm.moments(z, D, ang, non, exact=exact)
        out.append([qm.rung(c, _np(z.dtype)) for c in Ca.numpy()])
    return out


def _cost(a, z, u, terminal):
    """z [K, n], u [K, m] -> (l [K], rungs as _aug_rungs gives them).  A row
    whose augmented covariance leaves the ladder keeps the variances only."""
    D, ang, non = a["D"], list(a["ang"]), list(a["non"])
    Q = a["Q_term"] if terminal else a["Q"]
    L0 = qm.value(D, ang, non, Q, a["R"], a["x_goal"], a["u_goal"], z,
                  None if terminal else u)
    exact, own = _aug_rungs(a, z)
    trQ = torch.diagonal(Q).sum()
    add = []
    for k, r in enumerate(own):
        if r is not None:
            add.append(r * trQ)
        else:
            _, Ca = qm.moments(z[k], D, ang, non)
            off = Ca - torch.diag(torch.diagonal(Ca))
            add.append(-(off * Q.t()).sum())
    return L0 + torch.stack(add).to(L0.dtype), (exact, own)


def _live(a):
    live = torch.ones(a["B"], dtype=torch.bool)
    if a.get("active") is not None:
        live &= a["active"] != 0
    if a.get("bwd_status") is not None:
        live &= a["bwd_status"] == 0
    return live


def step(a, t, mutate=None):
    """One call of the moment step.  -> dict(Xp [B, A, P, D], z [B, A, n] =
    Zc[:, t], u [B, A, m] = Uc[:, t] (t < N), J [B, A], Jc [B, A] (t = N), F
    [B A P, in_dim] (t < N), live [B], and the jitter rungs met: rung_state,
    rung_aug_exact, rung_aug - lists over the live candidates)."""
    B, A, P, D, m, N = (a[k] for k in ("B", "A", "P", "D", "m", "N"))
    n = qm.encoded_size(D)
    dt = a["Z"].dtype
    nan = lambda *s: torch.full(s, float("nan"), dtype=dt)
    live, slot = _live(a), a.get("slot")
    in_dim = len(a["non"]) + 2 * len(a["ang"]) + m
    terminal = t == N
    Xp = a["Xp"].clone()
    out = dict(Xp=Xp, z=nan(B, A, n), u=nan(B, A, m), J=a["J"].clone(),
               Jc=nan(B, A), F=nan(B * A * P, in_dim), live=live,
               rung_state=[])
    cand = [(b, ai) for b in range(B) if live[b] for ai in range(A)]

    def rows(b, ai):
        sb = b if slot is None else int(slot[b])
        return slice((sb * A + ai) * P, (sb * A + ai + 1) * P)

    for b, ai in cand:
        if t == 0:
            out["z"][b, ai] = a["Z"][b, 0]
            continue
        x, _ = _output_particles(a, Xp[b, ai], a["net_out"][rows(b, ai)],
                                 a.get("eps_out"))
        Xp[b, ai] = x
        out["z"][b, ai], r = encode(*particle_moments(x, mutate))
        out["rung_state"].append(r)
    if not cand:
        return out
    idx = tuple(torch.tensor(c) for c in zip(*cand))
    z = out["z"][idx]
    u = None
    if not terminal:
        bs = idx[0]
        g = a["gains"][bs, t]
        k, K = g[:, :m], g[:, m:].reshape(-1, m, n)
        alpha = a["alphas"][idx[1]].unsqueeze(-1)
        if mutate == "no_alpha":
            alpha = torch.ones_like(alpha)
        dz = z - a["Z"][bs, t]
        u = _clamp(a, a["U"][bs, t] + alpha * k +
                   (K @ dz.unsqueeze(-1))[..., 0])
        out["u"][idx] = u
    l, (out["rung_aug_exact"], out["rung_aug"]) = _cost(a, z, u, terminal)
    J = l if t == 0 else out["J"][idx] + l
    out["J"][idx] = J
    if terminal:
        out["Jc"][idx] = J
        return out
    for i, (b, ai) in enumerate(cand):
        out["F"][rows(b, ai)] = _features(a, Xp[b, ai], u[i], mutate)
    return out


def _jvp_slot(a, b):
    return b if a.get("slot") is None else int(a["slot"][b])


def jvp_features(a, t, mutate=None):
    """-> dict(eps [B, P, D] = (Xp - mean_t) U_t^-1, F [B P, 8, in_dim]: the
    input row, the D + m tangent rows d row / d (mean_d | u) at the clamped
    action, zero rows; packed by `slot`, a negative slot is skipped)."""
    B, P, D, m = (a[k] for k in ("B", "P", "D", "m"))
    ang, non = list(a["ang"]), list(a["non"])
    nn, na = len(non), len(non) + 2 * len(ang)
    dt = a["Z"].dtype
    out = dict(eps=torch.full((B, P, D), float("nan"), dtype=dt),
               F=torch.full((B * P, NET_ROWS, na + m), float("nan"), dtype=dt))
    si = a["X_std_inv"]
    for b in range(B):
        sb = _jvp_slot(a, b)
        if sb < 0:
            continue
        z, x = a["Z"][b, t], a["Xp"][b]
        out["eps"][b] = torch.linalg.solve_triangular(
            upper_of(z, D), x - z[:D], upper=True, left=False)
        rows = x.new_zeros(P, NET_ROWS, na + m)
        rows[:, 0] = _features(a, x, _clamp(a, a["U"][b, t]), mutate)
        for c in range(D):
            if c in non:
                o = non.index(c)
                rows[:, 1 + c, o] = si[o]
            else:
                o = nn + 2 * ang.index(c)
                ds, dc = torch.cos(x[:, c]), -torch.sin(x[:, c])
                if mutate == "sincos_swap":
                    ds, dc = dc, ds
                rows[:, 1 + c, o] = ds * si[o]
                rows[:, 1 + c, o + 1] = dc * si[o + 1]
        for r in range(m):
            rows[:, 1 + D + r, na + r] = si[na + r]
        out["F"][sb * P:(sb + 1) * P] = rows
    return out


def _wrong_factor_differential(U, dC):
    """dU = Phi(U^-T dC U^-1) U with Phi = the upper triangle INCLUDING the
    whole diagonal: the "phi_diag" mutant."""
    W = torch.linalg.solve_triangular(
        U.t(), dC, upper=False)                      # U^-T dC
    W = torch.linalg.solve_triangular(U, W, upper=True, left=False)
    return torch.triu(W) @ U


def jvp_moments(a, t, mutate=None):
    """-> dict(Xp_next [B, P, D], Z_next [B, n], F_z [B, n, n], F_u [B, n, m]:
    the blocks of time step t; rung [B], eig_ratio [B]: smallest over largest
    eigenvalue of the output particles' covariance)."""
    B, P, D, m = (a[k] for k in ("B", "P", "D", "m"))
    n = qm.encoded_size(D)
    dt = a["Z"].dtype
    nan = lambda *s: torch.full(s, float("nan"), dtype=dt)
    out = dict(Xp_next=nan(B, P, D), Z_next=nan(B, n), F_z=nan(B, n, n),
               F_u=nan(B, n, m), rung=[], eig_ratio=[])
    sd = a["dX_std"]
    eps_out = a.get("eps_out")
    pairs = [(i, j) for i in range(D) for j in range(i, D)]  # U_ab, row-major
    for b in range(B):
        sb = _jvp_slot(a, b)
        if sb < 0:
            continue
        Y = a["net_out"][sb * P:(sb + 1) * P]                # [P, 8, out_dim]
        xo, stdeps = _output_particles(a, a["Xp"][b], Y[:, 0], eps_out)
        eps = a["eps"][b]

        def dnet(row):
            d = Y[:, row, :D] * sd
            if eps_out is not None and not a.get("independent_noise"):
                d = d + stdeps * Y[:, row, D:2 * D]
            return d

        eye = torch.eye(D, dtype=dt)
        tang = [eye[k] + dnet(1 + k) for k in range(D)]                # mean_b
        tang += [eps[:, i:i + 1] * (eye[j] + dnet(1 + j)) for i, j in pairs]
        tang += [dnet(1 + D + r) for r in range(m)]                    # u
        T = torch.stack(tang)                                 # [n + m, P, D]

        def f(theta):
            x = xo + (theta.view(-1, 1, 1) * T).sum(0)
            return encode(*particle_moments(x, mutate))[0]

        theta0 = torch.zeros(n + m, dtype=dt)
        Jac = torch.autograd.functional.jacobian(f, theta0)
        mean, cov = particle_moments(xo, mutate)
        z, r = encode(mean, cov)
        if mutate == "phi_diag" and r is not None:
            dC = torch.autograd.functional.jacobian(
                lambda th: particle_moments(
                    xo + (th.view(-1, 1, 1) * T).sum(0))[1], theta0)
            iu = torch.triu_indices(D, D)
            for k in range(n + m):
                dU = _wrong_factor_differential(upper_of(z, D), dC[..., k])
                Jac[D:, k] = dU[iu[0], iu[1]]
        ev = torch.linalg.eigvalsh(cov.double())
        out["rung"].append(r)
        out["eig_ratio"].append(float(ev[0] / ev[-1]))
        out["Xp_next"][b], out["Z_next"][b] = xo, z
        out["F_z"][b], out["F_u"][b] = Jac[:, :n], Jac[:, n:]
    return out
