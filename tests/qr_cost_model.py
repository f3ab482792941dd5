"""The quadratic cost on the angle-augmented Gaussian state under the DEFAULT
encoding, restated entry by entry in plain torch on the CPU - the yardstick of
test_qr_cost_kernel.py for `pddp_qr_cost_derivs_f32 / _f64`
(csrc/qr_cost_derivs.hip).  Written from the formulas of that kernel's header
comment and DESIGN.md 3.8; it shares no code with pddp_amd.utils.angular,
utils.encoding or costs.

  z = mean[D] | triu(U) row by row,  C = U^T U
  augmented order: non-angular states ascending, then (sin, cos) per angle
  E[sin a] = exp(-v/2) sin m,  E[cos a] = exp(-v/2) cos m        (v = C[a][a])
  with q = exp(-(v_i + v_j)/2), c = C[a_i][a_j]:
    Cov(sin_i, sin_j) = [q (e^c - 1) cos(m_i - m_j) - q (e^-c - 1) cos(m_i + m_j)] / 2
    Cov(cos_i, cos_j) = [q (e^c - 1) cos(m_i - m_j) + q (e^-c - 1) cos(m_i + m_j)] / 2
    Cov(sin_i, cos_j) = [q (e^c - 1) sin(m_i - m_j) + q (e^-c - 1) sin(m_i + m_j)] / 2
    Cov(x, sin_i) = C[x][a_i] E[cos_i],   Cov(x, cos_i) = -C[x][a_i] E[sin_i]
  L0 = (Ma - g)^T Q (Ma - g) + sum_ij Ca_ij Q_ji + (u - u_g)^T R (u - u_g)
  L  = L0 + rung * tr(Q): the augmented covariance is re-encoded through a
       Cholesky factorisation of Ca + rung I, rung the first of 1e-12, 1e-11,
       ... <= 10 at which the factorisation succeeds; the terminal step reads
       Q_term and has no action term.

`q (e^c - 1)` is evaluated as `q expm1(c)` (`exact=True`, the reference value)
or as the difference of two exponentials in the tensor's own dtype
(`exact=False`: what a float32 evaluation really factorises).  Not a test and
not a conftest: imported by the tests."""
import numpy as np
import torch


def encoded_size(D):
    return D + D * (D + 1) // 2


def non_angular(D, ang):
    return [i for i in range(D) if i not in ang]


def covariance(z, D):
    """C[i][j] (nested lists of tensors) of z = mean | triu(U), C = U^T U."""
    U, k = [[None] * D for _ in range(D)], D
    for r in range(D):
        for c in range(r, D):
            U[r][c] = z[..., k]
            k += 1
    C = [[None] * D for _ in range(D)]
    for i in range(D):
        for j in range(i, D):
            s = U[0][i] * U[0][j]
            for r in range(1, i + 1):
                s = s + U[r][i] * U[r][j]
            C[i][j] = C[j][i] = s
    return C


def moments(z, D, ang, non, exact=True):
    """Ma [..., NA], Ca [..., NA, NA] of the augmented state."""
    C = covariance(z, D)
    nn = len(non)
    NA = nn + 2 * len(ang)
    Ma = [None] * NA
    Ca = [[None] * NA for _ in range(NA)]
    for r, i in enumerate(non):
        Ma[r] = z[..., i]
        for c, j in enumerate(non):
            Ca[r][c] = C[i][j]
    for a1, i1 in enumerate(ang):
        r = nn + 2 * a1
        m1, v1 = z[..., i1], C[i1][i1]
        Es = torch.exp(-0.5 * v1) * torch.sin(m1)
        Ec = torch.exp(-0.5 * v1) * torch.cos(m1)
        Ma[r], Ma[r + 1] = Es, Ec
        for a2, i2 in enumerate(ang):
            cc = nn + 2 * a2
            m2, v2, c = z[..., i2], C[i2][i2], C[i1][i2]
            lq = -0.5 * (v1 + v2)
            if exact:
                ep = torch.exp(lq) * torch.expm1(c)
                em = torch.exp(lq) * torch.expm1(-c)
            else:
                ep = torch.exp(lq + c) - torch.exp(lq)
                em = torch.exp(lq - c) - torch.exp(lq)
            cd, cs = torch.cos(m1 - m2), torch.cos(m1 + m2)
            sd, ss = torch.sin(m1 - m2), torch.sin(m1 + m2)
            Ca[r][cc] = 0.5 * (ep * cd - em * cs)
            Ca[r + 1][cc + 1] = 0.5 * (ep * cd + em * cs)
            Ca[r][cc + 1] = 0.5 * (ep * sd + em * ss)
            Ca[cc + 1][r] = Ca[r][cc + 1]
        for c, j in enumerate(non):
            Ca[c][r] = Ca[r][c] = C[j][i1] * Ec
            Ca[c][r + 1] = Ca[r + 1][c] = -(C[j][i1] * Es)
    return (torch.stack(Ma, -1),
            torch.stack([torch.stack(row, -1) for row in Ca], -2))


def value(D, ang, non, Q, R, x_goal, u_goal, z, u):
    """L0 of (z, u); u None: no action term (the terminal step, with Q =
    Q_term).  Any leading batch dimensions."""
    Ma, Ca = moments(z, D, ang, non)
    dx = Ma - x_goal
    L0 = ((dx @ Q) * dx).sum(-1) + (Ca * Q.t()).sum((-2, -1))
    if u is not None:
        du = u - u_goal
        L0 = L0 + ((du @ R) * du).sum(-1)
    return L0


def evaluate(D, ang, non, m, Q, Q_term, R, x_goal, u_goal, z, u,
             terminal=False):
    """One (z [n], u [m]) in float64, `u` the clamped action:
    dict(L0, trQ, L_z [n], L_u [m], L_zz [n][n], L_uz [m][n], L_uu [m][m]);
    the terminal form (Q_term, no action) has the z blocks only."""
    f64 = lambda t: torch.as_tensor(t, dtype=torch.float64)
    n = encoded_size(D)
    Qs = f64(Q_term if terminal else Q)
    R, x_goal, u_goal = f64(R), f64(x_goal), f64(u_goal)
    zu = f64(z) if terminal else torch.cat([f64(z), f64(u)])
    assert zu.shape == (n + (0 if terminal else m),)

    def f(x):
        return value(D, ang, non, Qs, R, x_goal, u_goal, x[:n],
                     None if terminal else x[n:])
    g = torch.autograd.functional.jacobian(f, zu)
    H = torch.autograd.functional.hessian(f, zu)
    out = dict(L0=f(zu), trQ=torch.diagonal(Qs).sum(), L_z=g[:n],
               L_zz=H[:n, :n])
    if not terminal:
        out.update(L_u=g[n:], L_uz=H[n:, :n], L_uu=H[n:, n:])
    return out


def evaluate_batch(D, ang, non, m, Q, Q_term, R, x_goal, u_goal, Z, U,
                   terminal=False):
    """evaluate() for K points at once, Z [K, n], U [K, m]: the same forward
    under torch.func (vmap of jacfwd over jacrev), thirty times faster than K
    calls of evaluate(), to which test_qr_cost_kernel.py holds it.  Every
    entry of the result has the leading dimension K."""
    f64 = lambda t: torch.as_tensor(t, dtype=torch.float64)
    n = encoded_size(D)
    Qs = f64(Q_term if terminal else Q)
    R, x_goal, u_goal = f64(R), f64(x_goal), f64(u_goal)
    ZU = f64(Z) if terminal else torch.cat([f64(Z), f64(U)], -1)
    assert ZU.shape[1:] == (n + (0 if terminal else m),)

    def f(x):
        return value(D, ang, non, Qs, R, x_goal, u_goal, x[:n],
                     None if terminal else x[n:])
    g = torch.func.vmap(torch.func.grad(f))(ZU)
    H = torch.func.vmap(torch.func.hessian(f))(ZU)
    out = dict(L0=torch.func.vmap(f)(ZU),
               trQ=torch.diagonal(Qs).sum().expand(ZU.shape[0]),
               L_z=g[:, :n], L_zz=H[:, :n, :n])
    if not terminal:
        out.update(L_u=g[:, n:], L_uz=H[:, n:, :n], L_uu=H[:, n:, n:])
    return out


def ladder():
    """1e-12, 1e-11, ... <= 10 as the repeated `*= 10.0` of a double gives
    them (not the decimal literals: 1e-12 * 10 * 10 ... drifts by an ulp)."""
    out, jit = [], 1e-12
    while jit <= 10.0:
        out.append(jit)
        jit *= 10.0
    return out


def cholesky_ok(A):
    """Sequential upper Cholesky (row by row, pivot = sqrt of the reduced
    diagonal) in A's own numpy dtype; False at the first pivot that is not
    positive."""
    A = np.asarray(A)
    NA, T = A.shape[0], A.dtype.type
    U = np.zeros((NA, NA), dtype=A.dtype)
    for i in range(NA):
        for j in range(i, NA):
            s = A[i, j]
            for q in range(i):
                s = T(s - T(U[q, i] * U[q, j]))
            if i == j:
                if not s > 0:
                    return False
                U[i, i] = np.sqrt(s)
            else:
                U[i, j] = T(s / U[i, i])
    return True


def rung(Ca, dtype):
    """The first value of ladder() at which `Ca + rung I`, formed and
    factorised in `dtype` (np.float32 / np.float64), succeeds; None when none
    does."""
    Ca = np.asarray(Ca, dtype=dtype)
    eye = np.eye(Ca.shape[0], dtype=dtype)
    for jit in ladder():
        if cholesky_ok(Ca + dtype(jit) * eye):
            return jit
    return None
