"""What the GPU test modules and the scripts under tools/ share: the example
problems and their solvers, per-trajectory tables and references, the
closed-loop and MPC entry points called directly, the numpy model of the
device's normal draws, and the BNN fixtures.  Every name more than one module
uses lives here; a test module imports from here (or from golden_util,
abi_util, ...), never from another test module.

The one exception is the fp32 bookkeeping of tests/test_gpu_parity.py (STATS,
F32_RATIO, F32_FLOOR, _f32_ok, _backward64, _check_gains): tests/conftest.py
dumps sys.modules["test_gpu_parity"].STATS, so those stay there.

pytest rewrites `assert` in test modules only: every assert here carries its
own message."""
import ctypes
import types

import numpy as np
import torch

import oracle as orc
from golden_util import DT, np_dtype, rel_err

PROBLEMS = ["cartpole", "pendulum", "double_cartpole", "rendezvous"]
BOUND = {"cartpole": 10.0, "pendulum": 2.5, "double_cartpole": 20.0,
         "rendezvous": 5.0}
MEAN0 = {"cartpole": [0, 0, 0, 0], "pendulum": [0, 0],
         "double_cartpole": [0, 0, np.pi, 0, np.pi, 0],
         "rendezvous": [-10, -10, 10, 10, 0, -5, 5, 0]}
TDT = {"f64": torch.float64, "f32": torch.float32}
TOL = {"f64": 1e-9}  # fp64: 1e-9 everywhere (fp32: test_gpu_parity.py)
PARAM_COUNT = {"cartpole": 6, "pendulum": 5, "double_cartpole": 8,
               "rendezvous": 3}  # dt included (include/pddp_problem.h)
REC_NAMES = ("F_z", "F_u", "L_z", "L_u", "L_zz", "L_uz", "L_uu")
SENTINEL = -7.25
# pddp_problem.h: iLQRState
UNDEFINED = 0
CONTROLLER = ("mu", "delta", "state", "iter", "active", "fresh")
REARMED = dict(mu=0.0, delta=2.0, state=UNDEFINED, iter=1, active=1, fresh=1)


# ---- solvers on the example problems ----------------------------------------
def make_solver(problem, dtype, B, N, seed=0):
    import pddp_amd
    from pddp_amd.controllers.solver import ILQRSolver
    from pddp_amd.utils.encoding import StateEncoding
    mod = getattr(pddp_amd.examples, problem)
    model_cls = [getattr(mod, n) for n in dir(mod)
                 if n.endswith("DynamicsModel") and n != "DynamicsModel"][0]
    cost_cls = [getattr(mod, n) for n in dir(mod)
                if n.endswith("Cost") and n != "AugmentedQRCost"][0]
    model, cost = model_cls(DT[problem]), cost_cls()
    prob = model.native_problem(StateEncoding.IGNORE_UNCERTAINTY, cost)
    rng = np.random.RandomState(seed)
    n, m = prob.encoded_size, prob.action_size
    z0 = np.asarray(MEAN0[problem], np.float64) + 1e-2 * rng.randn(B, n)
    U = 0.1 * rng.randn(B, N, m)
    bound = BOUND[problem]
    td = TDT[dtype]
    u_min = torch.full((m,), -bound, dtype=td)
    u_max = torch.full((m,), bound, dtype=td)
    s = ILQRSolver(prob, B, N, td, "cuda", u_min, u_max)
    z0 = z0.astype(np_dtype(dtype))
    U = U.astype(np_dtype(dtype))
    s.z0.copy_(torch.from_numpy(z0))
    s.U.copy_(torch.from_numpy(U))
    op = orc.make_problem(problem, DT[problem])
    return s, op, z0, U, u_min.numpy(), u_max.numpy()


def run_traced(s, n_iterations, tol=5e-6, max_reg=1e10, max_rounds=400):
    traces = [[] for _ in range(s.B)]

    def on_round(r, s):
        act = s.active.cpu().numpy()
        st = s.state.cpu().numpy()
        J = s.J_opt.cpu().numpy()
        mu = s.mu.cpu().numpy()
        de = s.delta.cpu().numpy()
        for b in range(s.B):
            if on_round.attempted[b]:
                traces[b].append((st[b], J[b], mu[b], de[b]))
        on_round.attempted = act.copy()

    on_round.attempted = np.ones(s.B, np.uint8)
    s.fit(n_iterations, tol, max_reg, on_round, max_rounds=max_rounds)
    return traces


class nominal_kernel(object):
    """pddp_sweep_nominal_kernel(which) for the duration of a `with` block:
    3 / 4 the record generator of riccati_n4_elem.hpp inline / on wavefronts
    of its own, 0 auto (by batch)."""

    def __init__(self, which):
        self.which = which

    def __enter__(self):
        from pddp_amd import _native
        self.prev = _native.lib().pddp_sweep_nominal_kernel(self.which)

    def __exit__(self, *exc):
        from pddp_amd import _native
        _native.lib().pddp_sweep_nominal_kernel(self.prev)


# ---- per-trajectory problems (tests/test_batch_problem.py) ------------------
def record_tol(dtype):
    # test_derivative_records_vs_oracle's / test_line_search_vs_oracle's bars
    return 1e-10 if dtype == "f64" else 2e-4


def perturbed(problem, B, seed):
    """(params [B][P], x_goal [B][na], u_goal [B][m]) as float64 arrays of
    float32 values, and the oracle's problem of every trajectory."""
    rng = np.random.RandomState(seed)
    base = orc.make_problem(problem, DT[problem])
    P, na, m = PARAM_COUNT[problem], base.aug_size, base.action_size
    par = np.tile(np.array(base.params[:P]), (B, 1))
    par[:, 0] *= rng.uniform(0.9, 1.1, B)
    par[:, 1:] *= rng.uniform(0.8, 1.2, (B, P - 1))
    xg = np.tile(np.array(base.x_goal[:na]), (B, 1)) + \
        rng.uniform(-0.5, 0.5, (B, na))
    ug = np.tile(np.array(base.u_goal[:m]), (B, 1)) + \
        rng.uniform(-0.2, 0.2, (B, m))
    par, xg, ug = (a.astype(np.float32).astype(np.float64)
                   for a in (par, xg, ug))
    ops = []
    for b in range(B):
        op = orc.make_problem(problem, DT[problem])
        for i in range(P):
            op.params[i] = par[b, i]
        for i in range(na):
            op.x_goal[i] = xg[b, i]
        for i in range(m):
            op.u_goal[i] = ug[b, i]
        ops.append(op)
    return par, xg, ug, ops


def set_table(s, par, xg, ug):
    s.set_batch_problem(params=torch.from_numpy(par),
                        x_goal=torch.from_numpy(xg),
                        u_goal=torch.from_numpy(ug))


def named_views(s):
    v = dict(zip(REC_NAMES, s.record_views()))
    v["Z"], v["L"] = s.Z, s.L
    return v


def to_device(a, dtype):
    """numpy (or None) -> a contiguous device tensor; dtype: "f32" / "f64" or
    a torch dtype."""
    return None if a is None else torch.from_numpy(
        np.ascontiguousarray(a)).to(dtype=TDT.get(dtype, dtype), device="cuda")


# ---- closed-loop evaluation (tests/test_closed_loop.py) ---------------------
def plant_rows(problem, B, S, seed, dtype):
    """[B][S][20] plant rows (numpy, the run's dtype) from `perturbed`, and
    the oracle's problem of every (b, s)."""
    from pddp_amd import _native as N_
    par, xg, ug, ops = perturbed(problem, B * S, seed)
    rows = np.zeros((B * S, N_.BATCH_ROW))
    rows[:, N_.BATCH_PARAMS:N_.BATCH_PARAMS + par.shape[1]] = par
    rows[:, N_.BATCH_X_GOAL:N_.BATCH_X_GOAL + xg.shape[1]] = xg
    rows[:, N_.BATCH_U_GOAL:N_.BATCH_U_GOAL + ug.shape[1]] = ug
    rows = rows.reshape(B, S, N_.BATCH_ROW).astype(np_dtype(dtype))
    return rows, [ops[b * S:(b + 1) * S] for b in range(B)]


def policy_solver(problem, dtype, B, N, seed=0):
    """A solver holding a nominal and the gains of one sweep at reg = 1 (as
    test_batch_line_search_vs_oracle makes them), bounded."""
    s, op, z0, U, u_min, u_max = make_solver(problem, dtype, B, N, seed)
    s.nominal_rollout()
    s.derivs(set_state=False)
    s.backward(reg=torch.full((B,), 1.0, dtype=torch.float64, device="cuda"))
    assert int(s.bwd_status.abs().sum()) == 0, \
        ("the sweep at reg = 1 failed", problem, dtype, s.bwd_status.tolist())
    return s, op, u_min, u_max


def perturbed_starts(s, S, seed):
    """z0s = Z[b][0] + U(-0.05, 0.05), [B][S][n] in the run's dtype."""
    rng = np.random.RandomState(seed)
    Z0 = s.Z[:, 0].cpu().numpy()
    d = rng.uniform(-0.05, 0.05, (s.B, S, s.n))
    return (Z0[:, None, :] + d).astype(Z0.dtype)


def closed_loop_call(s, S, z0s=None, plant=None, gains="sweep", bounded=True,
                     active=None, keep=True, stats=True, fill=None):
    """pddp_closed_loop_* itself on the solver's nominal; outputs pre-filled
    with `fill`.  z0s / plant: numpy or None."""
    from pddp_amd import _native
    B, N, n, m = s.B, s.N, s.n, s.m
    opts = dict(dtype=s.dtype, device="cuda")

    def buf(*shape):
        return torch.empty(*shape, **opts) if fill is None else \
            torch.full(shape, fill, **opts)

    z0s_t, plant_t = to_device(z0s, s.dtype), to_device(plant, s.dtype)
    g = s.gains if isinstance(gains, str) else gains
    out = types.SimpleNamespace(
        X=buf(B, N + 1, S, n) if keep else None,
        U=buf(B, N, S, m) if keep else None, J=buf(B, S),
        stats=buf(B, 4) if stats else None)
    p = _native.ptr
    _native.call("pddp_closed_loop", s.dtype, ctypes.addressof(s.problem), B,
                 N, S, p(s.Z), p(s.U), p(g), p(z0s_t), p(plant_t),
                 p(s.u_min if bounded else None),
                 p(s.u_max if bounded else None), p(active), p(out.X),
                 p(out.U), p(out.J), p(out.stats), s._s())
    torch.cuda.synchronize()
    return out


# ---- the numpy model of the draws (include/pddp_hip.h) ----------------------
_U = np.uint64
_M0, _M1, _W0, _W1 = _U(0xD2511F53), _U(0xCD9E8D57), _U(0x9E3779B9), \
    _U(0xBB67AE85)
_LO, _32 = _U(0xffffffff), _U(32)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays of 32-bit words, key: two words."""
    c0, c1, c2, c3 = (np.asarray(c, _U) for c in counter)
    k0, k1 = _U(key[0]), _U(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # (32 x 32 bits: fits 64)
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LO, \
            (p0 >> _32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def box_muller(u1, u2):
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def model_draws(B, N, S, n, which, seed, offset, dtype):
    """[B][N][S][n] float64: the unit normals of stream `which`."""
    per = 4 if dtype == "f32" else 2
    nb = -(-n // per)
    shape = (B, N, S, nb)
    r = (np.arange(B * S, dtype=_U) + _U(offset)).reshape(B, 1, S, 1)
    t = np.arange(N, dtype=_U).reshape(1, N, 1, 1)
    k = np.arange(nb, dtype=_U).reshape(1, 1, 1, nb)
    counter = [np.broadcast_to(a, shape) for a in (
        r & _LO, r >> _32, t, (_U(which) << _U(16)) | k)]
    x = philox4x32_10(counter, (seed & 0xffffffff, seed >> 32))
    if dtype == "f32":
        u = [((w >> _U(9)).astype(np.float64) + 0.5) * 2.0 ** -23 for w in x]
        z = box_muller(u[0], u[1]) + box_muller(u[2], u[3])
    else:
        u = [(((hi << _U(20)) | (lo >> _U(12))).astype(np.float64) + 0.5) *
             2.0 ** -52 for hi, lo in ((x[0], x[1]), (x[2], x[3]))]
        z = box_muller(u[0], u[1])
    return np.stack(z, -1).reshape(B, N, S, nb * per)[..., :n]


# ---- the noisy entry points (tests/test_closed_loop_noise.py) ---------------
def std_vec(s, std):
    return None if std is None else torch.full(
        (s.n,), std, dtype=s.dtype, device="cuda")


def noisy_call(s, S, z0s=None, plant=None, w_std=None, v_std=None, seed=0,
               offset=0, keep=True, stats=True, b0=0, gains="sweep"):
    """pddp_closed_loop_noisy_* on trajectories b0.. of the solver's nominal
    (z0s / plant: numpy, all B trajectories' or None; w_std / v_std: a float
    for every component, a tensor or None)."""
    from pddp_amd import _native
    B, N, n, m = s.B - b0, s.N, s.n, s.m
    opts = dict(dtype=s.dtype, device="cuda")
    z0s_t = to_device(None if z0s is None else z0s[b0:], s.dtype)
    plant_t = to_device(None if plant is None else plant[b0:], s.dtype)
    w_t = w_std if torch.is_tensor(w_std) else std_vec(s, w_std)
    v_t = v_std if torch.is_tensor(v_std) else std_vec(s, v_std)
    g = s.gains if isinstance(gains, str) else gains
    out = types.SimpleNamespace(
        X=torch.empty(B, N + 1, S, n, **opts) if keep else None,
        U=torch.empty(B, N, S, m, **opts) if keep else None,
        J=torch.empty(B, S, **opts),
        stats=torch.empty(B, 4, **opts) if stats else None)
    p = _native.ptr
    _native.call("pddp_closed_loop_noisy", s.dtype,
                 ctypes.addressof(s.problem), B, N, S,
                 p(s.Z[b0:].contiguous()), p(s.U[b0:].contiguous()),
                 p(None if g is None else g[b0:].contiguous()), p(z0s_t),
                 p(plant_t), p(s.u_min), p(s.u_max), p(w_t), p(v_t), seed,
                 offset, None, p(out.X), p(out.U), p(out.J), p(out.stats),
                 s._s())
    torch.cuda.synchronize()
    return out


def draws_call(B, N, S, n, which, seed, offset, dtype):
    from pddp_amd import _native
    td = torch.float32 if dtype == "f32" else torch.float64
    W = torch.full((B, N, S, n), float("nan"), dtype=td, device="cuda")
    _native.call("pddp_closed_loop_draws", td, B, N, S, n, which, seed,
                 offset, _native.ptr(W), _native.stream_handle())
    torch.cuda.synchronize()
    return W


def check_stats(out, dtype, S):
    """As test_closed_loop_wider_than_a_wavefront: min, max and count exact,
    the mean within S eps of numpy's on the returned costs."""
    J, st = out.J.cpu().numpy(), out.stats.cpu().numpy()
    assert np.isfinite(J).all() and (J > 0).all(), \
        ("a cost that is not finite and positive", J.min(), J.max())
    eps = 2.0 ** -23 if dtype == "f32" else 2.0 ** -52
    for b in range(J.shape[0]):
        assert st[b, 1] == J[b].min() and st[b, 2] == J[b].max(), \
            ("min / max", b, st[b, 1:3], J[b].min(), J[b].max())
        assert st[b, 3] == S, ("count", b, st[b, 3], S)
        mean = J[b].astype(np.float64).mean()
        e = abs(float(st[b, 0]) - mean) / mean
        assert e <= S * eps, ("mean", b, e, S * eps)


# ---- references (tests/test_reference_tracking.py) --------------------------
def reference_rows(problem, B, L, seed):
    """(x_ref [B][L][na], u_ref [B][L][m]): float64 arrays of float32 values."""
    rng = np.random.RandomState(seed)
    base = orc.make_problem(problem, DT[problem])
    na, m = base.aug_size, base.action_size
    xr = np.array(base.x_goal[:na]) + rng.uniform(-0.5, 0.5, (B, L, na))
    ur = np.array(base.u_goal[:m]) + rng.uniform(-0.2, 0.2, (B, L, m))
    return (xr.astype(np.float32).astype(np.float64),
            ur.astype(np.float32).astype(np.float64))


def ref_row(L, t0, i):
    return min(t0 + i, L - 1)


def under_row(op, xr_b, ur_b, row):
    """`op` with the goals of reference row `row` of its trajectory."""
    for i in range(op.aug_size):
        op.x_goal[i] = xr_b[row, i]
    for i in range(op.action_size):
        op.u_goal[i] = ur_b[row, i]
    return op


def fresh_ops(problem, B):
    return [orc.make_problem(problem, DT[problem]) for _ in range(B)]


def set_ref(s, xr, ur, start=0):
    s.set_reference(torch.from_numpy(xr),
                    None if ur is None else torch.from_numpy(ur), start)


def ref_tensor(xr, ur, dtype):
    B, L = xr.shape[:2]
    ref = np.zeros((B, L, 12))
    ref[:, :, :xr.shape[2]] = xr
    ref[:, :, 8:8 + ur.shape[2]] = ur
    return to_device(ref, dtype)


def same_bits(a, b):
    return torch.equal(a, b) or bool(
        ((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def loop_solver(problem, dtype, B, N, table=False):
    from pddp_amd.controllers.solver import ILQRSolver, mpc_alphas
    s0, _, z0, U, u_min, u_max = make_solver(problem, dtype, B, N)
    td = TDT[dtype]
    s = ILQRSolver(s0.problem, B, N, td, "cuda", torch.from_numpy(u_min),
                   torch.from_numpy(u_max), alphas=mpc_alphas(td, "cuda"))
    s.z0.copy_(s0.z0)
    s.U.copy_(s0.U)
    if table:
        par, xg, ug, _ = perturbed(problem, B, seed=40)
        set_table(s, par, xg, ug)
    return s


# ---- MPC trials (tests/test_mpc_closed_loop.py) -----------------------------
def trial_logs(s, T, J0):
    """The five trial buffers (Xlog, Ulog, Jcl, state_log, live_log), every
    element a value no launch writes; Jcl starts at J0."""
    opts = dict(dtype=s.dtype, device="cuda")
    return (torch.full((s.B, T + 1, s.n), SENTINEL, **opts),
            torch.full((s.B, T, s.m), SENTINEL, **opts),
            torch.full((s.B,), J0, **opts),
            torch.full((s.B, T), -9, dtype=torch.int32, device="cuda"),
            torch.full((s.B, T), 9, dtype=torch.uint8, device="cuda"))


def mpc_advance(s, T, t, logs, plant=None, dist=None, mask=None, ref=None,
                ref_t0=0, bounded=True):
    """pddp_mpc_advance[_track]_* itself on the solver's buffers; `logs`: the
    five trial buffers of trial_logs."""
    from pddp_amd import _native
    p = _native.ptr
    head = (ctypes.addressof(s.problem), p(s.batch_table))
    name = "pddp_mpc_advance"
    if ref is not None:
        head += (p(ref), ref.shape[1], ref_t0)
        name += "_track"
    _native.call(name, s.dtype, *head, s.B, s.N, T, t, p(s.z0), p(s.U),
                 p(s.Z), p(s.u_min if bounded else None),
                 p(s.u_max if bounded else None), p(plant), p(dist), p(mask),
                 *[p(x) for x in logs], p(s.mu), p(s.delta), p(s.state),
                 p(s.iter), p(s.active), p(s.fresh), p(s.n_live), s._s())
    torch.cuda.synchronize()


def mpc_alphas_np():
    return (10.0 ** torch.linspace(0, -3, 11)).double().numpy()


def mpc_inputs(problem, B, N, big_U):
    """z0, U of make_solver (seed 0) without a device: `big_U`: U = 10 randn in
    place of 0.1 randn, the same draws."""
    base = orc.make_problem(problem, DT[problem])
    n, m = base.encoded_size, base.action_size
    rng = np.random.RandomState(0)
    z0 = np.asarray(MEAN0[problem], np.float64) + 1e-2 * rng.randn(B, n)
    U = (10.0 if big_U else 0.1) * rng.randn(B, N, m)
    return z0, U


def mpc_solver(problem, dtype, B, N, big_U=False, table=False):
    """A solver with the 11-alpha MPC schedule on `mpc_inputs`, the plants'
    fields of `perturbed(problem, B, 11)` as mpc_closed_loop's keywords."""
    from pddp_amd.controllers.solver import ILQRSolver, mpc_alphas
    s0, _, _, _, u_min, u_max = make_solver(problem, dtype, B, N)
    td = TDT[dtype]
    s = ILQRSolver(s0.problem, B, N, td, "cuda", torch.from_numpy(u_min),
                   torch.from_numpy(u_max), alphas=mpc_alphas(td, "cuda"))
    z0, U = mpc_inputs(problem, B, N, big_U)
    s.z0.copy_(torch.from_numpy(z0))
    s.U.copy_(torch.from_numpy(U))
    if table:
        par, xg, ug, _ = perturbed(problem, B, 12)
        set_table(s, par, xg, ug)
    par, xg, ug, plant_ops = perturbed(problem, B, 11)
    kw = dict(params=torch.from_numpy(par), x_goal=torch.from_numpy(xg),
              u_goal=torch.from_numpy(ug))
    return s, kw, plant_ops


# ---- BNN fixtures -----------------------------------------------------------
def bnn_real_size_run(dtype=torch.float32, raw=None):
    """Runs the HIP BNN path (native nominal rollout, forward-mode Jacobians,
    hyper-dual cost derivatives, moment-step line search around the fused
    network kernel) on the inputs of tests/golden/bnn_cartpole_real_size.npz and
    returns rows {what, r, hip_vs_f64, hip_vs_f32, ref32_vs_f64}."""
    import os
    import pddp_amd
    from golden_util import GOLDEN_DIR
    from pddp_amd.controllers.plugin import TorchProblem
    from pddp_amd.controllers.solver import ILQRSolver
    from pddp_amd.examples import cartpole
    from pddp_amd.models.bnn import (bnn_dynamics_model_factory,
                                     load_reference_state)
    g = np.load(os.path.join(GOLDEN_DIR, "bnn_cartpole_real_size.npz"))
    CM = cartpole.CartpoleDynamicsModel
    P, H, N = int(g["P"]), int(g["H"]), int(g["N"])
    model = bnn_dynamics_model_factory(
        4, 1, [H, H], CM.angular_indices, CM.non_angular_indices)(
            n_particles=P).float().eval()
    load_reference_state(model, {k[len("state/"):]: g[k] for k in g.files
                                 if k.startswith("state/")})
    # (float64: the same weights and noise cast up, as the fixture's f64 run)
    model = model.to(dtype).cuda()
    model.eps_in = {k: v.to(dtype).cuda() for k, v in model.eps_in.items()}
    for d in model.model.drops:
        d.noise = d.noise.to(dtype).cuda()
    cost = cartpole.CartpoleCost().to(dtype).cuda()
    enc = pddp_amd.StateEncoding.DEFAULT
    opts = {"use_predicted_std": False, "infer_noise_variables": True}
    plugin = TorchProblem(model, cost, enc, opts, {})
    R = g["z0"].shape[0]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()
    s = ILQRSolver(None, R, N, dtype, "cuda", cu(g["u_min"]),
                   cu(g["u_max"]), cu(g["alphas"]), plugin=plugin, n=14, m=1)
    s.set_nominal(cu(g["z0"]), cu(g["U"]))  # native nominal rollout
    s.derivs()
    path = dict(plugin.last_derivs_path)
    views = dict(zip(("F_z", "F_u", "L_z", "L_u", "L_zz", "L_uz", "L_uu"),
                     s.record_views()))
    views["Z"], views["L"] = s.Z, s.L
    rows = []

    def add(what, r, got, key):
        a32, a64 = g["f32/%d/%s" % (r, key)], g["f64/%d/%s" % (r, key)]
        rows.append(dict(what=what, r=r, hip_vs_f64=rel_err(got, a64),
                         hip_vs_f32=rel_err(got, a32),
                         ref32_vs_f64=rel_err(a32, a64)))
    for r in range(R):
        for nm in ("Z", "F_z", "F_u", "L", "L_z", "L_u", "L_zz", "L_uu"):
            add(nm, r, views[nm][r].cpu().numpy(), "fwd/" + nm)
        luz = float(views["L_uz"][r].abs().max())
        assert luz == 0.0 == float(np.abs(g["f64/%d/fwd/L_uz" % r]).max()), \
            ("L_uz is not zero", r, luz)
    # the line search on the reference's own gains
    for r in range(R):
        # (the fixture feeds the float32 run's gains and nominal to both dtypes)
        s.gains[r, :, :1] = cu(g["f32/%d/k" % r])
        s.gains[r, :, 1:] = cu(g["f32/%d/K" % r]).reshape(N, 14)
        s.Z[r] = cu(g["f32/%d/fwd/Z" % r])
    s.line_search(use_status=False)
    Zc = s.Zc.permute(0, 1, 2, 3).cpu().numpy()  # [R][N+1][A][n]
    Uc = s.Uc.cpu().numpy()
    Jc = s.Jc.cpu().numpy()
    if raw is not None:  # (tools/dbg: the arrays themselves)
        raw.update(Zc=Zc, Uc=Uc, Jc=Jc, g=g)
    for r in range(R):
        add("Z_new", r, Zc[r], "ls/Z_new")
        add("U_new", r, Uc[r], "ls/U_new")
        add("J", r, Jc[r], "ls/J")
    rows.append(dict(what="path", path=path))
    return rows


def bnn_mpc_controller(B, N, graph, P=100, H=200, seed=0,
                       use_predicted_std=False, dtype=torch.float32):
    import pddp_amd
    from pddp_amd.examples import cartpole
    from pddp_amd.models.bnn import bnn_dynamics_model_factory
    torch.manual_seed(seed)
    CM = cartpole.CartpoleDynamicsModel
    model = bnn_dynamics_model_factory(
        4, 1, [H, H], CM.angular_indices, CM.non_angular_indices)(
            n_particles=P).cuda().to(dtype).eval()
    with torch.no_grad():  # untrained network: keep its dynamics gentle
        model.model.out.weight.mul_(0.05)
        model.model.out.bias.mul_(0.05)
    cost = cartpole.CartpoleCost().cuda().to(dtype)
    ctrl = pddp_amd.controllers.iLQRController(
        None, model, cost, graph=graph,
        model_opts={"use_predicted_std": use_predicted_std,
                    "infer_noise_variables": True})
    g = torch.Generator().manual_seed(seed + 1)
    ctrl._U_nominal = (0.1 * torch.randn(B, N, 1, generator=g)).cuda().to(dtype)
    x = (torch.tensor([0.0, 0.0, 3.14159, 0.0]) +
         1e-2 * torch.randn(B, 4, generator=g)).cuda().to(dtype)
    return ctrl, CM(0.1).cuda().to(dtype), x


def bnn_problem(problem, B, N, seed=0):
    """The BNN workloads of bench.py (configs[2] / configs[3]'s problem):
    [200, 200] hidden, 100 particles, DEFAULT encoding, float32, bounded."""
    import pddp_amd
    from pddp_amd.controllers.ilqr import fit_alphas
    from pddp_amd.controllers.plugin import TorchProblem
    from pddp_amd.controllers.solver import ILQRSolver
    from pddp_amd.models.bnn import bnn_dynamics_model_factory
    torch.manual_seed(0)
    if problem == "cartpole":
        from pddp_amd.examples import cartpole as ex
        CM, cost_cls = ex.CartpoleDynamicsModel, ex.CartpoleCost
        mean0, bound = [0.0, 0.0, 3.14159, 0.0], 10.0
    else:
        from pddp_amd.examples import double_cartpole as ex
        CM, cost_cls = ex.DoubleCartpoleDynamicsModel, ex.DoubleCartpoleCost
        mean0, bound = [0.0, 0.0, 3.14159, 0.0, 3.14159, 0.0], 20.0
    D, m = CM.state_size, 1
    n = D + D * (D + 1) // 2
    model = bnn_dynamics_model_factory(
        D, m, [200, 200], CM.angular_indices, CM.non_angular_indices)(
            n_particles=100).cuda().eval()
    with torch.no_grad():  # untrained weights: keep the dynamics gentle
        model.model.out.weight.mul_(0.05)
        model.model.out.bias.mul_(0.05)
    cost = cost_cls().cuda()
    enc = pddp_amd.StateEncoding.DEFAULT
    opts = {"use_predicted_std": False, "infer_noise_variables": True}
    g = torch.Generator().manual_seed(seed)
    mean = torch.tensor(mean0)
    z0 = torch.stack([pddp_amd.GaussianVariable(
        mean + 1e-2 * torch.randn(D, generator=g),
        var=1e-2 * torch.ones(D)).encode(enc) for _ in range(B)]).cuda()
    U = (0.1 * torch.randn(B, N, m, generator=g)).cuda()

    def solver(model_, cost_, rows, dtype, native64=False):
        plugin = TorchProblem(model_, cost_, enc, opts, {})
        if dtype == torch.float64 and not native64:
            plugin.use_native_cost = False  # the float64 twin is the torch checker
        return ILQRSolver(None, rows, N, dtype, "cuda", torch.tensor([-bound]),
                          torch.tensor([bound]), fit_alphas(dtype, "cuda"),
                          plugin=plugin, n=n, m=m)
    return model, cost, z0, U, solver
