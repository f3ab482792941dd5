"""Toy GP systems shared by test_gp.py and test_gp_chunked.py: a fitted model
per example system, encoded rows to step, and the relative error both use."""
import torch

from pddp_amd.models.gp import gp_dynamics_model_factory

SYSTEMS = {"pendulum": (2, 1, [0]), "cartpole": (4, 1, [2]),
           "double_cartpole": (6, 1, [1, 2])}


def system_model(system, M, dtype, seed=0):
    D, m, ang = SYSTEMS[system]
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, D, generator=g, dtype=torch.float64)
    U = torch.randn(M, m, generator=g, dtype=torch.float64)
    dX = 0.3 * torch.sin(X @ torch.randn(D, D, generator=g,
                                          dtype=torch.float64)) + 0.2 * U
    model = gp_dynamics_model_factory(D, m, ang)().double()
    model.fit(X, U, dX)
    return model.to(dtype).cuda(), (X, U, dX)


def system_rows(system, R, encoding, dtype, seed=1, spread=0.2):
    from pddp_amd.utils.encoding import encode
    D, m, _ = SYSTEMS[system]
    g = torch.Generator().manual_seed(seed)
    mean = 0.5 * torch.randn(R, D, generator=g, dtype=torch.float64)
    A = spread * torch.randn(R, D, D, generator=g, dtype=torch.float64)
    C = A @ A.transpose(-1, -2) + 1e-3 * torch.eye(D, dtype=torch.float64)
    z = encode(mean, C=C, encoding=encoding)
    u = torch.randn(R, m, generator=g, dtype=torch.float64)
    return z.to(dtype).cuda(), u.to(dtype).cuda()


def max_rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))
