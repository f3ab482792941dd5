#!/usr/bin/env python3
"""Captures golden vectors from the reference (anassinator/pddp, imported
read-only from /root/reference through tools/ref_shims.py) into
tests/golden/*.npz.

Run in the build container only (the GPU box has no /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden.py

Each fixture holds inputs AND the reference's outputs for one
(problem, encoding, dtype): the nominal inputs (z0, U, bounds), the
float32-rounded model/cost constants the reference ended up with, the outputs of
`pddp.controllers.ilqr.forward` (ilqr.py:393), of `backward` (ilqr.py:530) for
the four gain branches x several regularisation values (including failing
ones), of `_control_law` + `_trajectory_cost` (ilqr.py:678,765) for both alpha
schedules, `boxqp` (constraint.py:150) unit cases and complete
`iLQRController.fit` traces (ilqr.py:237).  Only data is stored - no reference
source text.
"""
import math
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_shims import import_reference  # noqa: E402

warnings.simplefilter("ignore")
pddp = import_reference()

from pddp.controllers.ilqr import (  # noqa: E402
    forward, backward, _control_law, _trajectory_cost, iLQRController)
from pddp.utils.constraint import boxqp  # noqa: E402
from pddp.utils.encoding import StateEncoding  # noqa: E402
from pddp.utils.gaussian_variable import GaussianVariable  # noqa: E402
from pddp.examples import (  # noqa: E402
    cartpole, pendulum, double_cartpole, rendezvous)

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")

PROBLEMS = {
    # name: (model cls, cost cls, env cls, dt, bound, mean of z0)
    "cartpole": (cartpole.CartpoleDynamicsModel, cartpole.CartpoleCost,
                 cartpole.CartpoleEnv, 0.1, 10.0,
                 [0.01, -0.02, 0.015, 0.0]),
    "pendulum": (pendulum.PendulumDynamicsModel, pendulum.PendulumCost,
                 pendulum.PendulumEnv, 0.1, 2.5, [0.02, -0.01]),
    "double_cartpole": (double_cartpole.DoubleCartpoleDynamicsModel,
                        double_cartpole.DoubleCartpoleCost,
                        double_cartpole.DoubleCartpoleEnv, 0.05, 20.0,
                        [0.01, -0.02, math.pi - 0.015, 0.0, math.pi + 0.02,
                         0.01]),
    "rendezvous": (rendezvous.RendezvousDynamicsModel,
                   rendezvous.RendezvousCost, rendezvous.RendezvousEnv, 0.1,
                   5.0, [-10.0, -10.0, 10.0, 10.0, 0.0, -5.0, 5.0, 0.0]),
}

ENCODINGS = {
    "ignore": StateEncoding.IGNORE_UNCERTAINTY,
    "default": StateEncoding.DEFAULT,
    "variance": StateEncoding.VARIANCE_ONLY,
    "std": StateEncoding.STANDARD_DEVIATION_ONLY,
    "fullcov": StateEncoding.FULL_COVARIANCE_MATRIX,
}

# ilqr.py:282 - `.to` binds to the parenthesised EXPONENT (a trailer binds
# tighter than **): the integer exponents are cast, the power is taken in the
# run's dtype
ALPHAS_FIT = lambda dt=torch.float32: 1.025**(-torch.arange(10.0)**2).to(dt)
ALPHAS_MPC = lambda: 10.0**torch.linspace(0, -3, 11)  # ilqr.py:116


def np_(t):
    return t.detach().cpu().numpy().copy()


def nominal_controls(N, m, dtype, kind):
    t = torch.arange(N, dtype=torch.float64)
    cols = []
    for j in range(m):
        if kind == "cos":
            cols.append(0.1 * torch.cos(t + 0.7 * j))
        else:  # seeded
            g = torch.Generator().manual_seed(1234 + j)
            cols.append(0.1 * torch.randn(N, generator=g, dtype=torch.float64))
    return torch.stack(cols, -1).to(dtype)


def capture_backward(store, prefix, Z, F_z, F_u, L, L_z, L_u, L_zz, L_uz, L_uu,
                     U, u_min, u_max, regs):
    for branch in "ABCD":
        V_zz_reg = branch in "CD"
        bounded = branch in "BD"
        for reg in regs:
            key = "%s/%s/%g" % (prefix, branch, reg)
            kw = dict(reg=reg, V_zz_reg=V_zz_reg)
            if bounded:
                kw.update(u_min=u_min, u_max=u_max, U=U)
            try:
                k, K = backward(Z, F_z, F_u, L, L_z, L_u, L_zz, L_uz, L_uu,
                                **kw)
                store[key + "/ok"] = np.array(1)
                store[key + "/k"] = np_(k)
                store[key + "/K"] = np_(K)
            except RuntimeError as e:
                store[key + "/ok"] = np.array(0)
                store[key + "/err"] = np.array(str(e)[:60])


def capture_problem(name, enc_name, dtype, Ns, with_fit, fit_iters=None,
                    suffix="", lean_long=False, steps_from_mu=None):
    """`lean_long`: at the horizons after the first keep only what the tests
    read - the bounded forward pass, the four backward branches and the fit
    schedule's line search (a record of n = 27, N = 150 is 0.9 MB per tensor).
    `fit_iters`: iteration counts of the bounded fit trace; `suffix`: appended
    to the file's encoding key.  `steps_from_mu`: instead of `fit` (which
    starts at mu = 0, ilqr.py:277, 364-367) `fit_iters` calls of the
    controller's own `step` (ilqr.py:183-235) with the regularisation state
    preset to (mu, delta_0) - for starts from which `fit` RAISES in the
    reference: under a Gaussian encoding a line-search candidate that leaves
    the basin hands the cost a covariance that is not positive definite, and
    `_trajectory_cost` (ilqr.py:159) is outside `_step`'s try block."""
    model_cls, cost_cls, env_cls, dt, bound, mean0 = PROBLEMS[name]
    encoding = ENCODINGS[enc_name]
    store = {}
    model = model_cls(dt).to(dtype)
    cost = cost_cls().to(dtype)
    for pname, p in model.named_parameters():
        store["const/model/" + pname] = np_(p)
    for pname, p in cost.named_parameters():
        store["const/cost/" + pname] = np_(p)
    m = model.action_size
    u_min = torch.full((m,), -bound, dtype=dtype)
    u_max = torch.full((m,), bound, dtype=dtype)
    store["u_min"] = np_(u_min)
    store["u_max"] = np_(u_max)
    store["dt"] = np.array(dt)
    store["encoding"] = np.array(int(encoding))

    mean = torch.tensor(mean0, dtype=dtype)
    z0 = GaussianVariable(
        mean, var=1e-2 * torch.ones_like(mean)).encode(encoding).detach()
    store["z0"] = np_(z0)

    for N in Ns:
        for kind in ("cos", "seeded"):
            if kind == "seeded" and N != Ns[0]:
                continue
            tag = "N%d_%s" % (N, kind)
            U = nominal_controls(N, m, dtype, kind)
            if kind == "seeded":
                U = 30 * U  # exercises the clamp in forward() on pendulum
            store[tag + "/U"] = np_(U)
            lean = lean_long and N != Ns[0]
            for bounded in ((True,) if lean else (False, True)):
                bt = tag + ("/fwd_bounded" if bounded else "/fwd")
                kw = dict(u_min=u_min, u_max=u_max) if bounded else {}
                out = forward(z0, U.clone(), model, cost, encoding, **kw)
                names = ["Z", "F_z", "F_u", "L", "L_z", "L_u", "L_zz", "L_uz",
                         "L_uu"]
                for nm, t in zip(names, out):
                    store[bt + "/" + nm] = np_(t)
                if not bounded:
                    out_free = out
                else:
                    out_b = out
            # backward uses the bounded forward outputs when bounds are given
            # (this is what iLQRController.step does, ilqr.py:198-208).
            Z, F_z, F_u, L, L_z, L_u, L_zz, L_uz, L_uu = out_b
            regs = [0.0, 1e-6, 1.0, 100.0]
            capture_backward(store, tag + "/bwd", Z, F_z, F_u, L, L_z, L_u,
                             L_zz, L_uz, L_uu, U, u_min, u_max, regs)

            # Line search from the branch-B (controller default) gains, reg=1
            # (at the long horizons of --dc-default also from the reg = 100
            # gains, whose candidates all stay in the basin).
            for aname, alphas, ls_reg in (
                    ("fit", ALPHAS_FIT(dtype), 1.0),
                    ("mpc", ALPHAS_MPC(), 1.0),
                    ("fit100", ALPHAS_FIT(dtype), 100.0)):
                if (lean and aname == "mpc") or (not lean and
                                                 aname == "fit100"):
                    continue
                k, K = backward(Z, F_z, F_u, L, L_z, L_u, L_zz, L_uz, L_uu,
                                reg=ls_reg, u_min=u_min, u_max=u_max, U=U)
                alphas = alphas.to(dtype)
                Zb, Ub = _control_law(model, Z, U, k, K, alphas, encoding, {},
                                      u_min=u_min, u_max=u_max)
                try:
                    J = _trajectory_cost(cost, Zb, Ub, encoding, {})
                except RuntimeError:
                    # a candidate that left the basin (a covariance that is no
                    # longer positive definite, encoding.py:552-563): the
                    # reference raises for the whole batch; step size by step
                    # size, NaN where it raises
                    Js = []
                    for a in range(alphas.shape[0]):
                        try:
                            Js.append(_trajectory_cost(
                                cost, Zb[:, a:a + 1], Ub[:, a:a + 1],
                                encoding, {})[0])
                        except RuntimeError:
                            Js.append(torch.tensor(float("nan"), dtype=dtype))
                    J = torch.stack(Js)
                    print("  ", tag, aname, "candidates the reference raises "
                          "on:", int(torch.isnan(J).sum()))
                store["%s/ls_%s/alphas" % (tag, aname)] = np_(alphas)
                store["%s/ls_%s/Z_new" % (tag, aname)] = np_(Zb)
                store["%s/ls_%s/U_new" % (tag, aname)] = np_(Ub)
                store["%s/ls_%s/J" % (tag, aname)] = np_(J)

    if with_fit:
        N = with_fit
        for n_iter, bounded in (((fit_iters, True),) if fit_iters else
                                ((25, True), (8, False))
                                if enc_name == "ignore" else ((6, True),)):
            env = env_cls(dt=dt, model=model_cls(dt))
            env._state = mean.clone()
            ctrl = iLQRController(env, model, cost)
            U = nominal_controls(N, m, dtype, "cos")
            trace = []

            def on_iteration(i, state, Z, U_, J, ctrl=ctrl, trace=trace):
                trace.append((i, int(state), float(J), ctrl._mu, ctrl._delta))

            kw = dict(u_min=u_min, u_max=u_max) if bounded else {}
            if steps_from_mu is not None:
                # what `fit` itself does from here
                try:
                    ctrl.fit(U.clone(), encoding=encoding, n_iterations=1,
                             quiet=True, **kw)
                    store["steps/fit_raises"] = np.array(0)
                except RuntimeError as e:
                    store["steps/fit_raises"] = np.array(1)
                    store["steps/fit_error"] = np.array(str(e)[:60])
                del trace[:]
                ctrl._U_nominal = U.clone()
                ctrl._mu, ctrl._delta = float(steps_from_mu), ctrl._delta_0
                z0s = env.get_state().encode(encoding).detach().to(dtype)
                assert torch.equal(z0s, z0)
                alphas = ALPHAS_FIT(dtype).to(dtype)
                done = 0
                for it in range(n_iter):
                    try:
                        state = ctrl.step(z0s, U=None, i=it, encoding=encoding,
                                          alphas=alphas, quiet=True,
                                          on_iteration=on_iteration, **kw)
                    except RuntimeError as e:
                        print("   step", it, "raises:", str(e)[:60])
                        break
                    done += 1
                store["steps/mu0"] = np.array(float(steps_from_mu))
                store["steps/N"] = np.array(N)
                store["steps/n_steps"] = np.array(done)
                store["steps/alphas"] = np_(alphas)
                store["steps/U0"] = np_(U)
                store["steps/trace"] = np.array(trace, dtype=np.float64)
                store["steps/Z"] = np_(ctrl._Z_nominal)
                store["steps/U"] = np_(ctrl._U_nominal)
                store["steps/K"] = np_(ctrl._K)
                store["steps/state"] = np.array(int(state))
                print("   steps from mu = %g:" % steps_from_mu, trace)
                continue
            Zf, Uf, state = ctrl.fit(U.clone(), encoding=encoding,
                                     n_iterations=n_iter, quiet=True,
                                     on_iteration=on_iteration, **kw)
            ft = "fit_%s" % ("bounded" if bounded else "free")
            store[ft + "/N"] = np.array(N)
            store[ft + "/n_iterations"] = np.array(n_iter)
            store[ft + "/U0"] = np_(U)
            store[ft + "/trace"] = np.array(trace, dtype=np.float64)
            store[ft + "/Z"] = np_(Zf)
            store[ft + "/U"] = np_(Uf)
            store[ft + "/K"] = np_(ctrl._K)
            store[ft + "/state"] = np.array(int(state))

    dname = "f64" if dtype == torch.float64 else "f32"
    path = os.path.join(OUT, "%s_%s%s_%s.npz" % (name, enc_name, suffix,
                                                  dname))
    np.savez_compressed(path, **store)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024.0))


def capture_boxqp():
    """Unit vectors for boxqp (constraint.py:150-266), m in {1,2,4}."""
    store = {}
    g = torch.Generator().manual_seed(7)
    case = 0
    for dtype in (torch.float64, torch.float32):
        for m in (1, 2, 4):
            for trial in range(6):
                A = torch.randn(m, m, generator=g, dtype=torch.float64)
                Q = (A.t().mm(A) + 0.1 * torch.eye(m, dtype=torch.float64))
                c = 3.0 * torch.randn(m, generator=g, dtype=torch.float64)
                lower = -torch.rand(m, generator=g, dtype=torch.float64) - 0.1
                upper = torch.rand(m, generator=g, dtype=torch.float64) + 0.1
                x0 = torch.randn(m, generator=g, dtype=torch.float64)
                if trial == 0:  # interior optimum
                    lower, upper = lower * 100, upper * 100
                if trial == 1:  # warm start exactly at a bound
                    x0 = upper.clone()
                if trial == 2:  # pinned
                    upper = lower.clone()
                if trial == 3:  # indefinite Q
                    Q = Q - 2.0 * torch.eye(m, dtype=torch.float64) * Q.diag().max()
                Q, c, lower, upper, x0 = [
                    t.to(dtype) for t in (Q, c, lower, upper, x0)]
                # boxqp allocates float32 scratch under the default dtype and
                # the reference indexes with it; keep default dtype = dtype.
                torch.set_default_dtype(dtype)
                x, result, Ufree, free = boxqp(x0, Q, c, lower, upper)
                torch.set_default_dtype(torch.float32)
                key = "case%d" % case
                store[key + "/x0"] = np_(x0)
                store[key + "/Q"] = np_(Q)
                store[key + "/c"] = np_(c)
                store[key + "/lower"] = np_(lower)
                store[key + "/upper"] = np_(upper)
                store[key + "/x"] = np_(x)
                store[key + "/result"] = np.array(int(result))
                store[key + "/free"] = np_(free).astype(np.uint8)
                case += 1
    store["n_cases"] = np.array(case)
    path = os.path.join(OUT, "boxqp.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024.0))


def capture_bnn():
    """BNN moment-matched dynamics (pddp/models/bnn/modules.py): fixed weights,
    dropout noise and particle noise are stored with the outputs, so that an
    independent implementation can be fed the same randomness."""
    from pddp.models.bnn import bnn_dynamics_model_factory
    from pddp.utils.evaluation import batch_eval_dynamics
    from pddp.examples.cartpole import CartpoleDynamicsModel as CM
    torch.manual_seed(3)
    dtype = torch.float64
    P, D, m = 24, 4, 1
    enc = StateEncoding.DEFAULT
    cls = bnn_dynamics_model_factory(D, m, [32, 24], CM.angular_indices,
                                     CM.non_angular_indices)
    model = cls(n_particles=P).to(dtype).eval()
    model.X_mean.data = 0.1 * torch.randn(6, dtype=dtype)
    model.X_std.data = 0.5 + torch.rand(6, dtype=dtype)
    model.X_std_inv.data = model.X_std.reciprocal()
    model.dX_mean.data = 0.05 * torch.randn(D, dtype=dtype)
    model.dX_std.data = 0.2 + 0.3 * torch.rand(D, dtype=dtype)
    model.dX_std_inv.data = model.dX_std.reciprocal()
    store = {}
    mean = torch.tensor([0.1, -0.2, 0.3, 0.05], dtype=dtype)
    A_ = 0.2 * torch.randn(D, D, dtype=dtype)
    covar = A_.t().mm(A_) + 0.01 * torch.eye(D, dtype=dtype)
    z0 = GaussianVariable(mean, covar=covar).encode(enc).detach()
    store["z0"] = np_(z0)
    T = 6
    U = 0.3 * torch.randn(T, m, dtype=dtype)
    store["U"] = np_(U)
    opts = {"use_predicted_std": False, "infer_noise_variables": True}
    # 1. single-state moment-matched rollout i = 0..T-1 (fills the caches)
    z = z0
    Zs = [np_(z)]
    for i in range(T):
        z = model(z, U[i], i, enc, **opts).detach()
        Zs.append(np_(z))
    store["single/Z"] = np.stack(Zs)
    # everything random the model drew
    for name, mod in model.model.named_children():
        if hasattr(mod, "noise") and name.startswith("drop"):
            store["state/%s.noise" % name] = np_(mod.noise)
            store["state/%s.logit_p" % name] = np_(mod.logit_p)
            store["state/%s.temperature" % name] = np_(mod.temperature)
        if hasattr(mod, "weight"):
            store["state/%s.weight" % name] = np_(mod.weight)
            store["state/%s.bias" % name] = np_(mod.bias)
    for nm in ("X_mean", "X_std", "X_std_inv", "dX_mean", "dX_std",
               "dX_std_inv"):
        store["state/" + nm] = np_(getattr(model, nm))
    for i, e in model.eps_in.items():
        store["state/eps_in/%d" % i] = np_(e)
    # 2. Jacobians by the reference's replicated-input trick along that
    #    rollout (ilqr.py:467 calls it in time order, so output[i-1] is the
    #    cache of the previous call with the same row count)
    model.output = {}
    z = z0
    Fz, Fu, Zb = [], [], [np_(z0)]
    for i in range(T):
        zi = z.detach().requires_grad_()
        ui = U[i].detach().requires_grad_()
        zn, fz, fu = batch_eval_dynamics(model, zi, ui, i, encoding=enc,
                                         **opts)
        Fz.append(np_(fz)); Fu.append(np_(fu)); Zb.append(np_(zn))
        z = zn.detach()
    store["jac/Z"] = np.stack(Zb)
    store["jac/F_z"] = np.stack(Fz)
    store["jac/F_u"] = np.stack(Fu)
    # 3. a batch of DIFFERENT rows (what the line search feeds), time order
    model.output = {}
    rows = 5
    Zr = z0.unsqueeze(0) + 0.01 * torch.randn(rows, z0.shape[0], dtype=dtype)
    # keep the Cholesky block valid: only perturb the mean part
    Zr[:, D:] = z0[D:]
    store["rows/Z0"] = np_(Zr)
    Ur = 0.3 * torch.randn(T, rows, m, dtype=dtype)
    store["rows/U"] = np_(Ur)
    outs = []
    z = Zr
    for i in range(T):
        z = model(z, Ur[i], i, enc, **opts).detach()
        outs.append(np_(z))
    store["rows/Z"] = np.stack(outs)
    store["P"] = np.array(P)
    # 4. a whole iLQR fit on the learned model (same cached noise: eps_in and
    #    the dropout masks are reused as long as nobody calls resample())
    from pddp.examples.cartpole import CartpoleCost, CartpoleEnv
    model.output = {}
    cost = CartpoleCost().to(dtype)
    env = CartpoleEnv(dt=0.1)
    ctrl = iLQRController(env, model, cost, model_opts=opts)
    u_min = torch.tensor([-10.0], dtype=dtype)
    u_max = torch.tensor([10.0], dtype=dtype)
    trace = []

    def on_iteration(i, state, Z, U_, J):
        trace.append((i, int(state), float(J), ctrl._mu, ctrl._delta))

    class _E(object):  # env.get_state() with the stored z0
        def get_state(self_inner):
            class G(object):
                def encode(s2, enc_):
                    return z0
            return G()
    ctrl.env = _E()
    Zf, Uf, state = ctrl.fit(U.clone(), encoding=enc, n_iterations=5,
                             quiet=True, on_iteration=on_iteration,
                             u_min=u_min, u_max=u_max)
    store["fit/trace"] = np.array(trace, dtype=np.float64)
    store["fit/Z"] = np_(Zf)
    store["fit/U"] = np_(Uf)
    store["fit/K"] = np_(ctrl._K)
    store["fit/state"] = np.array(int(state))
    path = os.path.join(OUT, "bnn_cartpole_default_f64.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024.0))


def capture_bnn_real_size():
    """The BNN at the size BASELINE.json configs[2] runs it - hidden [200, 200],
    100 particles, cartpole, DEFAULT encoding (n = 14) - through the reference's
    own `forward` (ilqr.py:393-486: moment-matched nominal rollout,
    batch_eval_dynamics Jacobians evaluation.py:242-288, cost derivatives),
    `backward` (ilqr.py:529-674), `_control_law` + `_trajectory_cost`
    (ilqr.py:678-791) in float32 (the reference's default dtype, what the HIP
    BNN kernels compute in) AND in float64 with the very same weights, dropout
    noise and particle noise cast up (the yardstick for fp32 error).  A few
    trajectories, horizon 8."""
    from pddp.models.bnn import bnn_dynamics_model_factory
    from pddp.examples.cartpole import CartpoleDynamicsModel as CM
    from pddp.examples.cartpole import CartpoleCost
    torch.manual_seed(11)
    P, D, m, H, N, R = 100, 4, 1, 200, 8, 3
    enc = StateEncoding.DEFAULT
    opts = {"use_predicted_std": False, "infer_noise_variables": True}
    cls = bnn_dynamics_model_factory(D, m, [H, H], CM.angular_indices,
                                     CM.non_angular_indices)
    m32 = cls(n_particles=P).eval()
    with torch.no_grad():  # untrained network: moderate dynamics
        m32.model.fc_out.weight.mul_(0.1)
        m32.model.fc_out.bias.mul_(0.1)
    m32.X_mean.data = 0.1 * torch.randn(6)
    m32.X_std.data = 0.5 + torch.rand(6)
    m32.X_std_inv.data = m32.X_std.reciprocal()
    m32.dX_mean.data = 0.05 * torch.randn(D)
    m32.dX_std.data = 0.2 + 0.3 * torch.rand(D)
    m32.dX_std_inv.data = m32.dX_std.reciprocal()
    # inputs: R trajectories around the hanging-down start
    z0s, Us = [], []
    for r in range(R):
        mean = torch.tensor([0.0, 0.0, math.pi, 0.0]) + 0.05 * torch.randn(D)
        z0s.append(GaussianVariable(
            mean, var=1e-2 * torch.ones(D)).encode(enc).detach())
        Us.append(0.3 * torch.randn(N, m))
    # one call draws the dropout masks and eps_in[0]; they are then reused
    m32(z0s[0], Us[0][0], 0, enc, **opts)
    m32.output = {}
    store = {"P": np.array(P), "H": np.array(H), "N": np.array(N),
             "z0": np.stack([np_(z) for z in z0s]),
             "U": np.stack([np_(u) for u in Us]),
             "alphas": np_(ALPHAS_FIT()), "u_min": np.array([-10.0]),
             "u_max": np.array([10.0]), "reg": np.array(1.0)}
    for name, mod in m32.model.named_children():
        if hasattr(mod, "noise") and name.startswith("drop"):
            store["state/%s.noise" % name] = np_(mod.noise)
            store["state/%s.logit_p" % name] = np_(mod.logit_p)
            store["state/%s.temperature" % name] = np_(mod.temperature)
        if hasattr(mod, "weight"):
            store["state/%s.weight" % name] = np_(mod.weight)
            store["state/%s.bias" % name] = np_(mod.bias)
    for nm in ("X_mean", "X_std", "X_std_inv", "dX_mean", "dX_std",
               "dX_std_inv"):
        store["state/" + nm] = np_(getattr(m32, nm))
    store["state/eps_in/0"] = np_(m32.eps_in[0])
    # the float64 twin: identical parameter and noise VALUES
    m64 = cls(n_particles=P).double().eval()
    with torch.no_grad():
        for (n_a, p_a), (n_b, p_b) in zip(m32.named_parameters(),
                                          m64.named_parameters()):
            assert n_a == n_b
            p_b.data = p_a.data.double()
        for name, mod in m64.model.named_children():
            if hasattr(mod, "noise") and name.startswith("drop"):
                # same uniform draws; the concrete mask is recomputed from
                # them in float64 (CDropout.forward only redraws when it has
                # no mask of the right shape, modules.py:563-568)
                mod.noise.data = getattr(m32.model, name).noise.data.double()
                mod._update_concrete_noise(mod.noise)
    for nm in ("X_mean", "X_std", "X_std_inv", "dX_mean", "dX_std",
               "dX_std_inv"):
        getattr(m64, nm).data = getattr(m32, nm).data.double()
    m64.eps_in = {0: m32.eps_in[0].double()}
    for tag, model, dt in (("f32", m32, torch.float32),
                           ("f64", m64, torch.float64)):
        cost = CartpoleCost().to(dt)
        u_min = torch.tensor([-10.0], dtype=dt)
        u_max = torch.tensor([10.0], dtype=dt)
        for r in range(R):
            model.output = {}
            model.eps_in = {0: model.eps_in[0]}
            z0, U = z0s[r].to(dt), Us[r].to(dt)
            out = forward(z0, U.clone(), model, cost, enc, True, opts, {},
                          u_min, u_max)
            names = ("Z", "F_z", "F_u", "L", "L_z", "L_u", "L_zz", "L_uz",
                     "L_uu")
            for nm, t in zip(names, out):
                store["%s/%d/fwd/%s" % (tag, r, nm)] = np_(t)
            k, K = backward(*out, reg=1.0, u_min=u_min, u_max=u_max, U=U)
            store["%s/%d/k" % (tag, r)] = np_(k)
            store["%s/%d/K" % (tag, r)] = np_(K)
            # the line search is fed the float32 run's gains in both dtypes:
            # it is the rollout kernels that are being pinned, not the sweep
            k_in = torch.from_numpy(store["f32/%d/k" % r]).to(dt)
            K_in = torch.from_numpy(store["f32/%d/K" % r]).to(dt)
            Z_in = torch.from_numpy(store["f32/%d/fwd/Z" % r]).to(dt)
            alphas = ALPHAS_FIT().to(dt)
            model.output = {}
            Zn, Un = _control_law(model, Z_in, U, k_in, K_in, alphas, enc,
                                  opts, u_min, u_max)
            J = _trajectory_cost(cost, Zn, Un, enc, {})
            store["%s/%d/ls/Z_new" % (tag, r)] = np_(Zn)
            store["%s/%d/ls/U_new" % (tag, r)] = np_(Un)
            store["%s/%d/ls/J" % (tag, r)] = np_(J)
    path = os.path.join(OUT, "bnn_cartpole_real_size.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024.0))


def capture_round3():
    """Round-3 fixtures (one file, tests/golden/round3_extras.npz):
      train/  one fixed-noise training step of the BNN dynamics model through
              the reference's own modules (normalisation by BNN.fit with
              n_iter = 0, modules.py:170-176; model forward with held dropout
              masks, :187-188; likelihood losses.py:20-38; regulariser
              :550-583, 753-771; backward; Adam(amsgrad) :179) - loss terms,
              every parameter gradient, the parameters after 3 steps;
      pddp/   PDDPController.fit (pddp.py:61-206) on a deterministic
              environment with a model that records what it is trained on:
              exploration actions, the H = 2 N closed-loop trial, the
              keep-the-last-rows dataset rule;
      agg/    forward / backward / line search of ilqr.py under an
              AggregateCost (costs/base.py:125-181) built with the operator
              overloads."""
    from pddp.models.bnn import bnn_dynamics_model_factory
    from pddp.models.bnn.losses import gaussian_log_likelihood
    from pddp.examples.cartpole import (CartpoleCost, CartpoleDynamicsModel,
                                        CartpoleEnv)
    from pddp.controllers import PDDPController
    from pddp.utils.angular import augment_state
    store = {}
    dtype = torch.float64
    CM = CartpoleDynamicsModel

    # ------------------------------------------------------------- train/
    torch.manual_seed(21)
    D, m, Nd = 4, 1, 48
    cls = bnn_dynamics_model_factory(D, m, [32, 24], CM.angular_indices,
                                     CM.non_angular_indices)
    model = cls(n_particles=10).to(dtype)
    X = torch.randn(Nd, D, dtype=dtype)
    U = torch.randn(Nd, m, dtype=dtype)
    dX = 0.1 * torch.randn(Nd, D, dtype=dtype)
    store["train/X"], store["train/U"], store["train/dX"] = np_(X), np_(U), np_(dX)
    model.train()
    # (normalisation only: one step at learning rate 0 - n_iter = 0 never
    # ends, modules.py:394-411 counts up to `total` exactly)
    model.fit(X, U, dX, n_iter=1, learning_rate=0.0, quiet=True)
    for nm in ("X_mean", "X_std", "X_std_inv", "dX_mean", "dX_std",
               "dX_std_inv"):
        store["train/state/" + nm] = np_(getattr(model, nm))
    X_ = torch.cat([augment_state(X, CM.angular_indices,
                                  CM.non_angular_indices), U], dim=-1)
    params = [p for p in model.parameters() if p.requires_grad]
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    lr, reg_scale = 1e-3, 1.0
    # held masks drawn by the first forward below (modules.py:609-614: no
    # concrete mask yet -> uniform noise of the batch's shape, then kept)
    for name, mod in model.model.named_children():
        if name.startswith("drop"):
            mod.concrete_noise = None
    opt = torch.optim.Adam(params, lr, amsgrad=True)
    store["train/lr"], store["train/reg_scale"] = np.array(lr), np.array(reg_scale)
    first = True
    for step in range(3):
        opt.zero_grad()
        x_ = model._normalize_input(X_)
        out = model.model(x_, resample=False)
        mean, log_std = out.split([D, D], dim=-1)
        mean, log_std = model._scale_output(mean, log_std)
        nll = -gaussian_log_likelihood(dX, mean, log_std.exp()).mean()
        reg = model.model.regularization() / Nd
        loss = nll + reg_scale * reg
        if first:
            # initial weights and the masks' noise (drawn by this forward)
            for name, mod in model.model.named_children():
                if hasattr(mod, "noise") and name.startswith("drop"):
                    store["train/state/%s.noise" % name] = np_(mod.noise)
                    store["train/state/%s.temperature" % name] = np_(mod.temperature)
            first = False
        loss.backward()
        store["train/step%d/nll" % step] = np_(nll)
        store["train/step%d/reg" % step] = np_(reg)
        store["train/step%d/loss" % step] = np_(loss)
        if step == 0:
            for n_, p_ in zip(names, params):
                store["train/grad0/" + n_] = np_(p_.grad)
                store["train/init/" + n_] = np_(p_)  # (before the first step)
        opt.step()
    for n_, p_ in zip(names, params):
        store["train/after3/" + n_] = np_(p_)
    store["train/param_names"] = np.array(names)

    # -------------------------------------------------------------- pddp/
    class FlatEnv(object):
        """Deterministic cartpole plant: the true model, no noise."""

        def __init__(self, model, x0):
            self.model, self.x0 = model, x0.clone()
            self.x = x0.clone()

        def reset(self):
            self.x = self.x0.clone()

        def get_state(self):
            return GaussianVariable(self.x.clone(),
                                    var=1e-6 * torch.ones_like(self.x))

        def apply(self, u):
            z = self.x
            with torch.no_grad():
                self.x = self.model(z, u.detach().to(z), 0,
                                    StateEncoding.IGNORE_UNCERTAINTY).detach()

    class RecModel(CartpoleDynamicsModel):
        fitted = []

        def fit(self, X, U, dX, quiet=False, **kw):
            RecModel.fitted.append((np_(X), np_(U), np_(dX)))

    enc = StateEncoding.IGNORE_UNCERTAINTY
    Np = 8
    rmodel = RecModel(0.1).to(dtype)
    x0 = torch.tensor([0.0, 0.0, 0.3, 0.0], dtype=dtype)
    env = FlatEnv(CartpoleDynamicsModel(0.1).to(dtype), x0)
    cost = CartpoleCost().to(dtype)
    ctrl = PDDPController(env, rmodel, cost, training_opts={})
    torch.manual_seed(31)
    U0 = 0.2 * torch.randn(Np, 1, dtype=dtype)
    store["pddp/U0"], store["pddp/x0"] = np_(U0), np_(x0)
    u_min = torch.tensor([-3.0], dtype=dtype)
    u_max = torch.tensor([3.0], dtype=dtype)
    draws, trials = [], []
    real_rand_like = torch.rand_like

    def rec_rand_like(t, *a, **k):
        r = real_rand_like(t, *a, **k)
        draws.append(np_(r))
        return r
    torch.rand_like = rec_rand_like
    try:
        Zf, Uf, st = ctrl.fit(
            U0, encoding=enc, quiet=True, max_trials=4,
            n_initial_sample_trajectories=2, sampling_noise=0.8,
            max_dataset_size=20, u_min=u_min, u_max=u_max, n_iterations=4,
            on_trial=lambda t, X_, U_: trials.append((t, np_(X_), np_(U_))))
    finally:
        torch.rand_like = real_rand_like
    store["pddp/rand_draws"] = np.stack(draws)
    for k, (t, X_, U_) in enumerate(trials):
        store["pddp/trial%d/index" % k] = np.array(t)
        store["pddp/trial%d/X" % k], store["pddp/trial%d/U" % k] = X_, U_
    for k, (X_, U_, dX_) in enumerate(RecModel.fitted):
        store["pddp/fit%d/X" % k] = X_
        store["pddp/fit%d/U" % k] = U_
        store["pddp/fit%d/dX" % k] = dX_
    store["pddp/n_trials"] = np.array(len(trials))
    store["pddp/n_fits"] = np.array(len(RecModel.fitted))
    store["pddp/Z"], store["pddp/U"] = np_(Zf), np_(Uf)
    store["pddp/state"] = np.array(int(st))

    # --------------------------------------------------------------- agg/
    Na = 12
    agg = CartpoleCost().to(dtype) * 0.6 + CartpoleCost(
        pole_length=0.8).to(dtype) * 0.25 + 0.5
    amodel = CartpoleDynamicsModel(0.1).to(dtype)
    for ename in ("ignore", "default"):
        e = ENCODINGS[ename]
        z0 = GaussianVariable(
            torch.tensor([0.01, -0.02, 0.4, 0.0], dtype=dtype),
            var=1e-2 * torch.ones(4, dtype=dtype)).encode(e).detach()
        Ua = nominal_controls(Na, 1, dtype, "cos")
        um = torch.tensor([-10.0], dtype=dtype)
        uM = torch.tensor([10.0], dtype=dtype)
        Z, F_z, F_u, L, L_z, L_u, L_zz, L_uz, L_uu = forward(
            z0, Ua.clone(), amodel, agg, e, True, {}, {}, u_min=um, u_max=uM)
        pre = "agg/%s/" % ename
        store[pre + "z0"], store[pre + "U"] = np_(z0), np_(Ua)
        for nm, v in (("Z", Z), ("F_z", F_z), ("F_u", F_u), ("L", L),
                      ("L_z", L_z), ("L_u", L_u), ("L_zz", L_zz),
                      ("L_uz", L_uz), ("L_uu", L_uu)):
            store[pre + nm] = np_(v)
        k, K = backward(Z, F_z, F_u, L, L_z, L_u, L_zz, L_uz, L_uu, reg=1.0,
                        u_min=um, u_max=uM, U=Ua)
        store[pre + "k"], store[pre + "K"] = np_(k), np_(K)
        al = ALPHAS_FIT(dtype)
        Zn, Un = _control_law(amodel, Z, Ua, k, K, al, e, {}, u_min=um,
                              u_max=uM)
        J = _trajectory_cost(agg, Zn, Un, e, {})
        store[pre + "J"] = np_(J)
    path = os.path.join(OUT, "round3_extras.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


def capture_accept_schedule():
    """tests/golden/accept_schedule.npz: the reference controller's own
    `_reset_reg` / `_increase_reg(max_reg)` / `_decrease_reg` (ilqr.py:364-390)
    driven through seeded random call sequences - 200 calls each, for every
    pair of increase probability {0.3, 0.5, 0.7} and max_reg {1e-3, 1, 1e10},
    a reset at the start and after every `_increase_reg` that returned False.
    Stored per sequence: the calls (0 reset, 1 increase, 2 decrease), `_mu`
    and `_delta` after each call (doubles) and what the call returned (1 True,
    0 False, -1 None)."""
    n_calls = 200
    calls, mus, deltas, rets, p_incs, max_regs = [], [], [], [], [], []
    for si, (p_inc, max_reg) in enumerate(
            (p, r) for p in (0.3, 0.5, 0.7) for r in (1e-3, 1.0, 1e10)):
        rng = np.random.RandomState(100 + si)
        ctrl = iLQRController(None, None, None)
        seq, mu, delta, ret = [], [], [], []
        reset_due = True
        for _ in range(n_calls):
            if reset_due:
                call, r = 0, ctrl._reset_reg()
                reset_due = False
            elif rng.rand() < p_inc:
                call, r = 1, ctrl._increase_reg(max_reg)
                reset_due = r is False
            else:
                call, r = 2, ctrl._decrease_reg()
            seq.append(call)
            mu.append(float(ctrl._mu))
            delta.append(float(ctrl._delta))
            ret.append(-1 if r is None else int(bool(r)))
        calls.append(seq); mus.append(mu); deltas.append(delta); rets.append(ret)
        p_incs.append(p_inc); max_regs.append(max_reg)
    store = {"calls": np.array(calls, np.int8),
             "mu": np.array(mus, np.float64),
             "delta": np.array(deltas, np.float64),
             "ret": np.array(rets, np.int8),
             "p_increase": np.array(p_incs, np.float64),
             "max_reg": np.array(max_regs, np.float64)}
    path = os.path.join(OUT, "accept_schedule.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes;",
          "max_reg reached %d times" % int((store["ret"] == 0).sum()))


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    np.random.seed(0)
    if "--accept-schedule" in sys.argv:
        capture_accept_schedule()
        return
    if "--round3" in sys.argv:
        capture_round3()
        return
    if "--bnn-only" in sys.argv:
        capture_bnn()
        return
    if "--bnn-real-size" in sys.argv:
        capture_bnn_real_size()
        return
    if "--other-encodings" in sys.argv:
        # the remaining Gaussian encodings: fp64, short horizons
        for enc in ("variance", "std", "fullcov"):
            capture_problem("cartpole", enc, torch.float64, [5, 25],
                            with_fit=12)
        capture_problem("pendulum", "variance", torch.float64, [5, 25],
                        with_fit=12)
        capture_problem("pendulum", "std", torch.float64, [5, 25],
                        with_fit=12)
        capture_problem("pendulum", "fullcov", torch.float64, [5, 25],
                        with_fit=12)
        return
    if "--dc-fullcov" in sys.argv:
        # round 3: the double cartpole under the full covariance (n = 42), the
        # last (problem, encoding) pair to go native; short horizons - the
        # reference differentiates 43 replicated inputs per step
        capture_problem("double_cartpole", "fullcov", torch.float64, [5, 12],
                        with_fit=6)
        return
    if "--rendezvous-gaussian" in sys.argv:
        # round 4: rendezvous (8 states, 4 actions) carries the FULL covariance
        # through its dynamics (rendezvous/model.py:94,110): n = 44 under the
        # Cholesky encoding, 72 under the full covariance matrix
        for enc in ("default", "fullcov", "variance", "std"):
            capture_problem("rendezvous", enc, torch.float64, [5, 12],
                            with_fit=6)
        return
    if "--dc-default" in sys.argv:
        # round 5: BASELINE configs[3]'s own shape - the double cartpole under
        # DEFAULT (n = 27) at horizons 5 and 150, and under IGNORE_UNCERTAINTY
        # at horizon 150, each with a three-iteration fit at N = 150
        # (double_cartpole/model.py:100-195 through ilqr.py:393-674)
        capture_problem("double_cartpole", "default", torch.float64, [5, 150],
                        with_fit=150, fit_iters=3, lean_long=True,
                        steps_from_mu=1000.0)
        capture_problem("double_cartpole", "ignore", torch.float64, [5, 150],
                        with_fit=150, fit_iters=3, suffix="150",
                        lean_long=True)
        return
    if "--default-only" in sys.argv:
        capture_problem("cartpole", "default", torch.float64, [5, 25],
                        with_fit=12)
        capture_problem("pendulum", "default", torch.float64, [5, 25],
                        with_fit=12)
        return
    capture_boxqp()
    for dtype in (torch.float64, torch.float32):
        capture_problem("cartpole", "ignore", dtype, [5, 100], with_fit=30)
        capture_problem("pendulum", "ignore", dtype, [5, 50], with_fit=25)
        capture_problem("double_cartpole", "ignore", dtype, [5, 60],
                        with_fit=20)
        capture_problem("rendezvous", "ignore", dtype, [5, 40], with_fit=20)
    # DEFAULT (upper-triangular Cholesky) encoding: captured for the next
    # rows of SURVEY 8(f); fp64 only, short horizons (n = 14 / 5).
    capture_problem("cartpole", "default", torch.float64, [5, 25], with_fit=12)
    capture_problem("pendulum", "default", torch.float64, [5, 25], with_fit=12)
    capture_bnn()
    capture_bnn_real_size()


if __name__ == "__main__":
    main()
