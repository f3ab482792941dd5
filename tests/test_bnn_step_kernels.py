"""`pddp_bnn_moment_step_f32 / _f64` (csrc/bnn_rollout.hip) and
`pddp_bnn_jvp_features_*` / `pddp_bnn_jvp_moments_*` (csrc/bnn_jvp.hip) called
directly, as controllers/plugin.py calls them, against tests/bnn_step_model.py
- the same step in plain torch float64 on the CPU - at every shape the host
admits: the runtime-D instantiations (D = 1, 3, 5, 7, 8 of the moment step,
`EXACT = false` of the Jacobian pair, D = 4 with m = 2 on the 32-lane kernel),
m = 2, no angles, the full-width bound D = 8 with two angles, the particle
counts at which a lane's `has[q]` flips or a slice owns no particle, skipped
and packed trajectories, and encode()'s diagonal fall-back.  The network
output is synthetic (increments of 1e-2 .. 1e-1): no network launch.

Bars.  f64: states, actions, costs, particles and features 1e-10, Jacobians
1e-8, each the largest difference over the largest entry of the model's block
(the bars of test_bnn_f64.py).  f32: the model itself is run in torch float32
on the CPU on the same inputs, and per block the kernel may be 8 x as far from
the float64 model as that run is, at least 16 eps32 (the yardstick of
test_qr_cost_kernel.py; DESIGN.md 5.1 holds the measured pairs).

Preconditions, asserted: every case but the fall-back's sits on jitter rung
1e-12 in the run's dtype - the state covariance, and the augmented covariance
evaluated with `q expm1(c)` and with the difference of exponentials; every
Jacobian case has P >= D + 2 (but D = 1 at P = 2, where one slice in two owns
no particle: the covariance of two particles of one dimension has full rank)
and an output covariance whose smallest eigenvalue is at least 1e-4 of its
largest."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bnn_step_model as bm
import qr_cost_model as qm

EPS32 = float(np.finfo(np.float32).eps)
SENT = 12345.0          # what every output holds before a call
GUARD = 16              # words behind every output buffer
RUNG = qm.ladder()[0]
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32],
                                 ids=["f64", "f32"])
JACOBIANS = ("F_z", "F_u")


def dtype_id(dtype):
    return "f32" if dtype == torch.float32 else "f64"


def shape_id(s):
    D, ang, m = s[:3]
    tail = "".join("-%s" % (v,) for v in s[3:])
    return "D%d-ang%s-m%d%s" % (D, "".join(map(str, ang)) or "none", m, tail)


# ------------------------------------------------------------------ inputs --
def r32(t):
    return t.float().double()


def constants(D, ang, m, idx):
    """As test_qr_cost_kernel.constants: Q = A^T A + 0.1 I (plus a skew part
    of the same size for odd `idx`), Q_term = 3 Q^T, R with an off-diagonal
    entry, non-zero goals, bounds; and the network's normalisation - float64,
    every value exactly representable in float32."""
    g = torch.Generator().manual_seed(2000 + idx)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    uni = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    NA = D + len(ang)
    A = rnd(NA, NA)
    Q = A.t() @ A + 0.1 * torch.eye(NA, dtype=torch.float64)
    if idx % 2 == 1 and NA > 1:
        S = rnd(NA, NA)
        K = S - S.t()
        Q = Q + K * (Q.norm() / K.norm())
    Q = r32(Q)
    R = torch.tensor([[0.7, 0.2], [0.2, 0.4]], dtype=torch.float64)[:m, :m]
    two = lambda a, b: r32(torch.tensor([a, b], dtype=torch.float64)[:m])
    return dict(
        Q=Q, Q_term=r32(3.0 * Q.t()), R=r32(R), x_goal=r32(0.5 * rnd(NA)),
        u_goal=two(0.3, -0.2), u_min=two(-0.8, -0.6), u_max=two(0.9, 0.7),
        X_mean=r32(0.1 * rnd(NA + m)), X_std_inv=r32(0.5 + uni(NA + m)),
        dX_mean=r32(0.01 * rnd(D)), dX_std=r32(0.03 + 0.05 * uni(D)))


def encoded_states(D, count, g):
    """[count, n]: means N(0, 1), Cholesky diagonal^2 in [0.02, 0.07],
    off-diagonals 0.05 randn."""
    mean = torch.randn(count, D, generator=g, dtype=torch.float64)
    diag = (0.02 + 0.05 * torch.rand(count, D, generator=g,
                                     dtype=torch.float64)).sqrt()
    off = 0.05 * torch.randn(count, D, D, generator=g, dtype=torch.float64)
    U = torch.triu(off, 1) + torch.diag_embed(diag)
    iu = torch.triu_indices(D, D)
    return torch.cat([mean, U[:, iu[0], iu[1]]], -1)


def standardised(P, D, g):
    e = torch.randn(P, D, generator=g, dtype=torch.float64)
    return e - e.mean(0) if P < 3 else (e - e.mean(0)) / e.std(0)


def synthetic_net(rows, D, out_dim, ups, g):
    """[*rows, out_dim]: mean increments N(0, 1) (times dX_std = 0.03 .. 0.08),
    log-std columns around -1; columns nobody may read are NaN."""
    y = torch.full((*rows, out_dim), float("nan"), dtype=torch.float64)
    y[..., :D] = torch.randn(*rows, D, generator=g, dtype=torch.float64)
    if ups:
        y[..., D:2 * D] = -1.0 + 0.3 * torch.randn(*rows, D, generator=g,
                                                   dtype=torch.float64)
    return r32(y)


@functools.lru_cache(maxsize=None)
def step_case(D, ang, m, B, A, N, P, ups, bounds=True, extra_out=0, seed=0,
              skip=False):
    """The arguments of the N + 1 calls of one moment-step case (float64,
    every value exactly representable in float32): the nominal's states stay
    within 0.05 of its first, one action per trajectory lies beyond a bound,
    the particles of step 0 are mean + eps U of z_0 for every candidate.  With
    `skip`: trajectory 1 is inactive, trajectory 2 has a failed backward
    pass, `slot` as TorchProblem._bnn_rollouts builds it, and `net_outs` hold
    the live trajectories' rows packed to the front (NaN behind them)."""
    non = tuple(qm.non_angular(D, ang))
    idx = 17 * D + 5 * len(ang) + m + sum(ang)
    g = torch.Generator().manual_seed(100 * idx + seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    n = qm.encoded_size(D)
    a = dict(constants(D, ang, m, idx), B=B, A=A, P=P, D=D, m=m, N=N, ang=ang,
             non=non, out_dim=(2 * D if ups else D) + extra_out)
    if not bounds:
        a["u_min"] = a["u_max"] = None
    Z0 = encoded_states(D, B, g)
    Z = Z0[:, None].repeat(1, N + 1, 1)
    Z[:, 1:] += 0.05 * rnd(B, N, n)
    U = torch.rand(B, N, m, generator=g, dtype=torch.float64) - 0.5
    for b in range(B if N > 1 else 1):  # (N = 1: trajectory 0's only)
        U[b, b % N, b % m] = 2.0 if b % 2 else -2.0
    a.update(Z=r32(Z), U=r32(U), gains=r32(0.1 * rnd(B, N, m + m * n)),
             alphas=r32(torch.tensor([1.0, 0.5, 0.125, 0.03125])[:A].double()))
    e0 = standardised(P, D, g)
    X0 = torch.stack([a["Z"][b, 0, :D] + e0 @ bm.upper_of(a["Z"][b, 0], D)
                      for b in range(B)])
    a["Xp"] = r32(X0[:, None].repeat(1, A, 1, 1))
    a["J"] = torch.full((B, A), float("nan"), dtype=torch.float64)
    rows = B * A * P
    nets = [None] + [synthetic_net((rows,), D, a["out_dim"], ups, g)
                     for _ in range(N)]
    a["eps_outs"] = [None] + [r32(standardised(P, D, g)) if ups else None
                              for _ in range(N)]
    if skip:
        assert B == 4
        a["active"] = torch.tensor([1, 0, 1, 1], dtype=torch.uint8)
        a["bwd_status"] = torch.tensor([0, 0, 3, 0], dtype=torch.int32)
        alive = (a["active"] != 0) & (a["bwd_status"] == 0)
        a["slot"] = (torch.cumsum(alive.to(torch.int32), 0,
                                  dtype=torch.int32) - 1)
        a["unpacked_net_outs"] = nets
        packed = [None]
        for y in nets[1:]:
            yp = torch.full_like(y, float("nan"))
            live = y.view(B, A * P, -1)[alive]
            yp[:live.shape[0] * A * P] = live.reshape(-1, y.shape[-1])
            packed.append(yp)
        nets = packed
    a["net_outs"] = nets
    return a


def in_dtype(a, dtype):
    """The case's floating tensors (lists of them too) in `dtype`."""
    conv = lambda v: v.to(dtype) if torch.is_tensor(v) and \
        v.is_floating_point() else v
    return {k: [conv(x) for x in v] if isinstance(v, list) else conv(v)
            for k, v in a.items()}


def step_args(a, t, Xp, J):
    return dict(a, Xp=Xp, J=J, net_out=a["net_outs"][t],
                eps_out=a["eps_outs"][t])


def model_rollout(a, dtype, mutate=None):
    """bm.step() for t = 0 .. N on the case in `dtype`: the list of results,
    float64."""
    a = in_dtype(a, dtype)
    outs, Xp, J = [], a["Xp"], a["J"]
    for t in range(a["N"] + 1):
        o = bm.step(step_args(a, t, Xp, J), t, mutate)
        Xp, J = o["Xp"], o["J"]
        outs.append({k: v.double() if torch.is_tensor(v) and
                     v.is_floating_point() else v for k, v in o.items()})
    return outs


@functools.lru_cache(maxsize=None)
def step_model(key, dtype):
    return model_rollout(step_case(*key), dtype)


def assert_on_first_rung(outs):
    for o in outs:
        for k in ("rung_state", "rung_aug_exact", "rung_aug"):
            assert all(r == RUNG for r in o.get(k, [])), (k, o.get(k))


# -------------------------------------------------------------- comparison --
def rel(got, ref):
    """max |got - ref| over the entries the model has (not NaN), relative to
    the block's largest model entry; None when the model has none."""
    has = ~torch.isnan(ref)
    if not bool(has.any()):
        return None
    top = float(ref[has].abs().max())
    err = float((got[has] - ref[has]).abs().max())
    if err != err:
        return float("inf")
    return err / top if top > 0 else (0.0 if err == 0 else float("inf"))


def bars_for(ref, ref32, dtype):
    """f64: the fixed bars; f32: 8 x the float32 model's own distance from
    the float64 model, at least 16 eps32, per block."""
    out = {}
    for k, v in ref.items():
        if not (torch.is_tensor(v) and v.is_floating_point()) or \
                rel(v, v) is None:
            continue
        if dtype == torch.float64:
            out[k] = 1e-8 if k in JACOBIANS else 1e-10
        else:
            out[k] = max(8 * rel(ref32[k], v), 16 * EPS32)
    return out


def failures(got, ref, bars, tag=None, ref32=None):
    """The blocks of `got` farther from `ref` than their bar: [(block, error,
    bar)].  With a tag, prints every figure first."""
    bad = []
    for k, bar in bars.items():
        e = rel(got[k], ref[k])
        if tag is not None:
            print("BNNSTEP", *tag, k, "%.3g" % e,
                  "%.3g" % rel(ref32[k], ref[k]) if ref32 is not None else "-",
                  "bar %.3g" % bar)
        if not e <= bar:
            bad.append((k, e, bar))
    return bad


# ------------------------------------------------------------ device calls --
STEP_IN = ("Z", "U", "gains", "alphas", "u_min", "u_max", "Q", "Q_term", "R",
           "x_goal", "u_goal", "X_mean", "X_std_inv", "dX_mean", "dX_std")
STEP_OUT = ("Xp", "F", "Zc", "Uc", "J", "Jc")


def fill_shape(st, D, ang, non, m):
    st.D, st.m = D, m
    st.n_ang, st.n_non = len(ang), len(non)
    for i, v in enumerate(ang):
        st.ang[i] = v
    for i, v in enumerate(non):
        st.non[i] = v
    st.in_dim = len(non) + 2 * len(ang) + m


def guarded(shape, dtype, init=None):
    """(flat buffer of SENT with GUARD words behind the data, its view)."""
    count = int(np.prod(shape))
    flat = torch.full((count + GUARD,), SENT, dtype=dtype, device="cuda")
    view = flat[:count].view(*shape)
    if init is not None:
        view.copy_(init.to(dtype))
    return flat, view


class StepRun(object):
    """The device side of one moment-step case: call(t) launches step t as
    TorchProblem._bnn_rollouts does; outputs start as SENT."""

    def __init__(self, a, dtype):
        from pddp_amd import _native
        assert sorted(a["ang"] + a["non"]) == list(range(a["D"]))
        self.a, self.dtype = a, dtype
        B, A, P, D, m, N = (a[k] for k in ("B", "A", "P", "D", "m", "N"))
        n = qm.encoded_size(D)
        dev = lambda t: None if t is None else t.to(dtype).cuda().contiguous()
        self.keep = {k: dev(a[k]) for k in STEP_IN}
        for k in ("active", "bwd_status", "slot"):
            self.keep[k] = None if a.get(k) is None else a[k].cuda()
        self.nets = [dev(y) for y in a["net_outs"]]
        self.eps = [dev(e) for e in a["eps_outs"]]
        st = self.st = _native.BnnStep()
        st.B, st.A, st.P, st.N = B, A, P, N
        fill_shape(st, D, a["ang"], a["non"], m)
        st.out_dim = a["out_dim"]
        shapes = dict(Xp=(B, A, P, D), F=(B * A * P, st.in_dim),
                      Zc=(B, N + 1, A, n), Uc=(B, N, A, m), J=(B, A),
                      Jc=(B, A))
        self.flat, self.view = {}, {}
        for k in STEP_OUT:
            self.flat[k], self.view[k] = guarded(
                shapes[k], dtype, a["Xp"] if k == "Xp" else None)
        for k, t in list(self.keep.items()) + list(self.view.items()):
            setattr(st, k, _native.ptr(t))

    def call(self, t):
        from pddp_amd import _native
        self.st.t = t
        self.st.net_out = _native.ptr(self.nets[t])
        self.st.eps_out = _native.ptr(self.eps[t])
        _native.call("pddp_bnn_moment_step", self.dtype, ctypes.byref(self.st),
                     _native.stream_handle(torch.device("cuda")))
        torch.cuda.synchronize()

    def snapshot(self):
        return {k: v.cpu().clone() for k, v in self.flat.items()}


def expected_step(a, o, t):
    """The model's result of step t laid out as the kernel's buffers: NaN
    where the call writes nothing."""
    B, A, P, D, m, N = (a[k] for k in ("B", "A", "P", "D", "m", "N"))
    n = qm.encoded_size(D)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64)
    Zc, Uc = nan(B, N + 1, A, n), nan(B, N, A, m)
    Zc[:, t] = o["z"]
    if t < N:
        Uc[:, t] = o["u"]
    Xp = nan(B, A, P, D)
    if t > 0:
        Xp[o["live"]] = o["Xp"][o["live"]]
    J = nan(B, A)
    J[o["live"]] = o["J"][o["live"]]
    return dict(Xp=Xp, F=o["F"], Zc=Zc, Uc=Uc, J=J, Jc=o["Jc"])


def assert_written_only(before, after, exp):
    """Bit for bit what it was - SENT, or an earlier step's result - wherever
    the model writes nothing, the guard words included."""
    for k, e in exp.items():
        count = e.numel()
        untouched = torch.isnan(e).reshape(-1)
        assert torch.equal(after[k][:count][untouched],
                           before[k][:count][untouched]), k
        assert torch.equal(after[k][count:], before[k][count:]), k
        assert torch.isfinite(after[k][:count][~untouched]).all(), k


def run_step_case(key, dtype, tag):
    """All N + 1 calls of a case against the model, after every call."""
    a = step_case(*key)
    ref = step_model(key, torch.float64)
    ref32 = step_model(key, torch.float32) if dtype == torch.float32 else None
    assert_on_first_rung(ref if dtype == torch.float64 else ref32)
    run = StepRun(a, dtype)
    bad = []
    for t in range(a["N"] + 1):
        before = run.snapshot()
        run.call(t)
        after = run.snapshot()
        exp = expected_step(a, ref[t], t)
        assert_written_only(before, after, exp)
        got = {k: after[k][:exp[k].numel()].view(exp[k].shape).double()
               for k in exp}
        e32 = expected_step(a, ref32[t], t) if ref32 is not None else None
        bad += [(t,) + f for f in failures(
            got, exp, bars_for(exp, e32, dtype), tag + ("t%d" % t,), e32)]
    assert not bad, bad
    return run


# --------------------------------------------------------------- GPU tests --
# (D, angular indices, m): the runtime-D instantiation, then the three
# compiled dimensions
STEP_SHAPES = [(1, (), 1), (1, (0,), 1), (3, (1,), 2), (5, (0, 4), 1),
               (7, (2,), 2), (8, (), 2), (8, (3, 7), 2),
               (2, (0,), 2), (4, (2,), 1), (6, (1, 2), 2)]
STEP_P = 20  # lanes 0 .. 3 own two particles, the others one


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("ups", [False, True], ids=["mean_only", "eps_out"])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=shape_id)
def test_moment_step_over_the_dispatch(shape, ups, dtype):
    """B = 3, A = 3, N = 2 (nine candidates: three wavefronts, the last with
    one group), bounds with one clamped action per trajectory, `eps_out` NULL
    (out_dim = D) and given (out_dim = 2 D): after each of the three calls Xp,
    Zc[:, t], Uc[:, t], J, F and at t = N Jc against the model fed the same
    network output, and nothing else written."""
    D, ang, m = shape
    key = (D, ang, m, 3, 3, 2, STEP_P, ups)
    run_step_case(key, dtype, (dtype_id(dtype), shape_id(shape),
                               "ups%d" % ups))


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("bounds,extra_out", [(False, 0), (True, 3)],
                         ids=["free", "wide_rows"])
def test_moment_step_without_bounds_and_with_wider_network_rows(
        bounds, extra_out, dtype):
    """(5, (0, 4), 1) with NULL bounds, and with out_dim = 2 D + 3 (the row
    stride of net_out; the three extra columns are NaN)."""
    key = (5, (0, 4), 1, 3, 3, 2, STEP_P, True, bounds, extra_out)
    a = step_case(*key)
    run_step_case(key, dtype, (dtype_id(dtype), "D5", "bounds%d" % bounds,
                               "extra%d" % extra_out))
    if not bounds:  # (the bounds would have bitten: the comparison saw it)
        u = torch.stack([o["u"] for o in step_model(key, torch.float64)[:-1]])
        c = constants(5, (0, 4), 1, 0)
        assert bool((u > c["u_max"]).any() or (u < c["u_min"]).any())
    assert a["out_dim"] == 10 + extra_out


EDGE_CASES = [(1, (0,), 1, P) for P in (2, 15, 16, 17, 100, 128)] + \
             [(4, (2,), 1, P) for P in (15, 16, 17, 100, 128)]


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("case", EDGE_CASES, ids=shape_id)
def test_moment_step_particle_count_edges(case, dtype):
    """A lane owns particles lane + 16 q: P = 15 / 16 / 17 and 128 are where
    `has[q]` flips, on the scalar (D = 1) and the paired (D = 4) load path;
    P = 2 with D = 1 only (two particles span one dimension).  B = 2, A = 2,
    N = 1, eps_out given."""
    D, ang, m, P = case
    run_step_case((D, ang, m, 2, 2, 1, P, True), dtype,
                  (dtype_id(dtype), shape_id(case)))


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("shape", [(3, (1,), 2), (4, (2,), 1)], ids=shape_id)
def test_moment_step_skips_and_packs(shape, dtype):
    """B = 4 with trajectory 1 inactive and trajectory 2's backward pass
    failed, `slot` as TorchProblem._bnn_rollouts builds it: the packed run
    against the model, the live candidates bit for bit what the unpacked
    launch gives them, their F rows at the packed positions, and everything of
    the skipped trajectories still SENT (assert_written_only; their particles
    as given)."""
    D, ang, m = shape
    key = (D, ang, m, 4, 3, 2, STEP_P, True, True, 0, 0, True)
    a = step_case(*key)
    packed = run_step_case(key, dtype, (dtype_id(dtype), shape_id(shape),
                                        "packed"))
    plain = dict(a, active=None, bwd_status=None, slot=None,
                 net_outs=a["unpacked_net_outs"])
    full = StepRun(plain, dtype)
    A, P, N = a["A"], a["P"], a["N"]
    live = [0, 3]
    for t in range(N + 1):
        full.call(t)
    # (F: the rows of the last stage step, in both runs)
    for rank, b in enumerate(live):
        for k in ("Xp", "Zc", "Uc", "J", "Jc"):
            assert torch.equal(packed.view[k][b], full.view[k][b]), (k, b)
        rows = lambda i: slice(i * A * P, (i + 1) * A * P)
        assert torch.equal(packed.view["F"][rows(rank)],
                           full.view["F"][rows(b)]), b
    assert bool((packed.view["F"][len(live) * A * P:] == SENT).all())
    for b in (1, 2):
        for k in ("Zc", "Uc", "J", "Jc"):
            assert bool((packed.view[k][b] == SENT).all()), (k, b)
        assert torch.equal(packed.view["Xp"][b].cpu().double(), a["Xp"][b])


# ---- the Jacobian pair
JVP_B, JVP_N, JVP_T = 3, 3, 1
# (D, angular indices, m, P): P spread so that 7, 9, 33 and 100 each meet a
# 16-lane and a 32-lane shape; B P is no multiple of eight
JVP_SHAPES = [(1, (), 1, 7), (1, (0,), 1, 9), (3, (1,), 2, 33),
              (3, (0, 2), 1, 100), (5, (0, 4), 1, 9), (5, (), 2, 33),
              (4, (2,), 2, 7), (2, (0, 1), 2, 7),
              (2, (0,), 1, 9), (4, (2,), 1, 33), (6, (1, 2), 1, 100),
              (1, (0,), 1, 2), (1, (0,), 1, 3)]
JVP_VARIANTS = [(False, False), (True, False), (True, True)]
JVP_VARIANT_IDS = ["mean_only", "eps_out", "eps_out_independent"]


def jvp_lanes(D, m):
    dirs = qm.encoded_size(D) + m
    return 16 if D <= 4 and dirs <= 15 else 32


def test_jvp_shapes_meet_both_kernels_at_every_particle_count():
    """The table above: every P of 7, 9, 33, 100 on a 16-lane and on a 32-lane
    shape, B P never a multiple of eight, P >= D + 2 (but the two-particle
    case), every `EXACT = false` kernel and D = 4 on the 32-lane one."""
    lanes = {P: set() for P in (7, 9, 33, 100)}
    for D, ang, m, P in JVP_SHAPES:
        assert D + m <= 7 and D <= 6
        assert P >= D + 2 or (D, P) == (1, 2)
        assert (JVP_B * P) % 8 != 0
        if P in lanes:
            lanes[P].add(jvp_lanes(D, m))
    assert all(v == {16, 32} for v in lanes.values()), lanes
    seen = {(D, jvp_lanes(D, m)) for D, _, m, _ in JVP_SHAPES}
    assert {(1, 16), (3, 16), (5, 32), (4, 32), (2, 16), (4, 16),
            (6, 32)} <= seen


@functools.lru_cache(maxsize=None)
def jvp_case(D, ang, m, P, ups=False, independent=False, skip=False, seed=0):
    """The arguments of the pair at t = 1 of N = 3 (float64, exactly
    representable in float32): Xp = mean_t + e U_t with e standardised per
    trajectory, the action of step t beyond a bound for trajectory 1,
    `net_out` synthetic - tangent rows N(0, 1), the rows behind the D + m
    tangents NaN (nobody may read them)."""
    non = tuple(qm.non_angular(D, ang))
    idx = 17 * D + 5 * len(ang) + m + sum(ang)
    g = torch.Generator().manual_seed(100 * idx + 7 + seed)
    B, N, t = JVP_B, JVP_N, JVP_T
    a = dict(constants(D, ang, m, idx), B=B, P=P, D=D, m=m, N=N, ang=ang,
             non=non, out_dim=2 * D if ups else D,
             independent_noise=int(independent))
    Z = encoded_states(D, B * (N + 1), g).reshape(B, N + 1, -1)
    U = torch.rand(B, N, m, generator=g, dtype=torch.float64) - 0.5
    U[1, t, m - 1] = 2.0
    a.update(Z=r32(Z), U=r32(U))
    a["Xp"] = r32(torch.stack([
        a["Z"][b, t, :D] + standardised(P, D, g) @ bm.upper_of(a["Z"][b, t], D)
        for b in range(B)]))
    a["slot"] = torch.tensor([0, -1, 1], dtype=torch.int32) if skip else None
    y = synthetic_net((B * P, bm.NET_ROWS), D, a["out_dim"], ups, g)
    if ups:  # tangent rows of the log-std columns: derivatives, not levels
        y[:, 1:, D:] = r32(torch.randn(B * P, bm.NET_ROWS - 1, D, generator=g,
                                       dtype=torch.float64))
    y[:, 1 + D + m:] = float("nan")
    if skip:
        y[2 * P:] = float("nan")
    a["net_out"] = y
    a["eps_out"] = r32(standardised(P, D, g)) if ups else None
    return a


@functools.lru_cache(maxsize=None)
def jvp_model(key, dtype):
    """(features, moments) of the model on the case in `dtype`, float64; the
    moments read the model's own eps."""
    a = in_dtype(jvp_case(*key), dtype)
    fe = bm.jvp_features(a, JVP_T)
    mo = bm.jvp_moments(dict(a, eps=fe["eps"]), JVP_T)
    dbl = lambda o: {k: v.double() if torch.is_tensor(v) else v
                     for k, v in o.items()}
    return dbl(fe), dbl(mo)


JVP_IN = ("Z", "U", "u_min", "u_max", "X_mean", "X_std_inv", "dX_mean",
          "dX_std", "net_out", "Xp", "eps_out")
JVP_OUT = ("Xp_next", "eps", "F", "Z_next", "F_z", "F_u")


class JvpRun(object):
    """The device side of one case of the pair; outputs start as SENT."""

    def __init__(self, a, dtype, eps=None, t=JVP_T):
        from pddp_amd import _native
        assert sorted(a["ang"] + a["non"]) == list(range(a["D"]))
        self.dtype = dtype
        B, P, D, m, N = (a[k] for k in ("B", "P", "D", "m", "N"))
        n = qm.encoded_size(D)
        dev = lambda v: None if v is None else v.to(dtype).cuda().contiguous()
        self.keep = {k: dev(a.get(k)) for k in JVP_IN}
        self.keep["slot"] = None if a.get("slot") is None else a["slot"].cuda()
        st = self.st = _native.BnnJvp()
        st.B, st.P, st.N, st.t = B, P, N, t
        fill_shape(st, D, a["ang"], a["non"], m)
        st.out_dim = a["out_dim"]
        st.independent_noise = a["independent_noise"]
        shapes = dict(Xp_next=(B, P, D), eps=(B, P, D),
                      F=(B * P, bm.NET_ROWS, st.in_dim), Z_next=(B, n),
                      F_z=(B, N, n, n), F_u=(B, N, n, m))
        self.flat, self.view = {}, {}
        for k in JVP_OUT:
            self.flat[k], self.view[k] = guarded(shapes[k], dtype)
        if eps is not None:  # (skipped trajectories' rows: never read)
            self.view["eps"].copy_(torch.nan_to_num(eps, nan=SENT).to(dtype))
        for k, v in list(self.keep.items()) + list(self.view.items()):
            setattr(st, k, _native.ptr(v))

    def call(self, which):
        from pddp_amd import _native
        _native.call("pddp_bnn_jvp_" + which, self.dtype,
                     ctypes.byref(self.st),
                     _native.stream_handle(torch.device("cuda")))
        torch.cuda.synchronize()

    def snapshot(self):
        return {k: v.cpu().clone() for k, v in self.flat.items()}


def jvp_expected(a, o, which):
    """The model's blocks in the kernel's layouts (the time axis of F_z / F_u
    NaN but at step t), NaN for every buffer the call does not write."""
    B, P, D, m, N = (a[k] for k in ("B", "P", "D", "m", "N"))
    n = qm.encoded_size(D)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64)
    exp = dict(Xp_next=nan(B, P, D), eps=nan(B, P, D),
               F=nan(B * P, bm.NET_ROWS,
                     len(a["non"]) + 2 * len(a["ang"]) + m),
               Z_next=nan(B, n), F_z=nan(B, N, n, n), F_u=nan(B, N, n, m))
    if which == "features":
        exp.update(eps=o["eps"], F=o["F"])
    else:
        exp.update(Xp_next=o["Xp_next"], Z_next=o["Z_next"])
        exp["F_z"][:, JVP_T] = o["F_z"]
        exp["F_u"][:, JVP_T] = o["F_u"]
    return exp


def run_jvp(key, dtype, which, tag):
    a = jvp_case(*key)
    fe, mo = jvp_model(key, torch.float64)
    fe32, mo32 = jvp_model(key, torch.float32) if dtype == torch.float32 \
        else (None, None)
    if which == "moments":
        own = mo if dtype == torch.float64 else mo32
        assert all(r == RUNG for r in own["rung"]), own["rung"]
        assert min(mo["eig_ratio"]) >= 1e-4, mo["eig_ratio"]
    run = JvpRun(a, dtype, eps=fe["eps"] if which == "moments" else None)
    before = run.snapshot()
    run.call(which)
    after = run.snapshot()
    o, o32 = (fe, fe32) if which == "features" else (mo, mo32)
    exp = jvp_expected(a, o, which)
    assert_written_only(before, after, exp)
    got = {k: after[k][:exp[k].numel()].view(exp[k].shape).double()
           for k in exp}
    e32 = jvp_expected(a, o32, which) if o32 is not None else None
    bad = failures(got, exp, bars_for(exp, e32, dtype), tag, e32)
    assert not bad, bad
    return exp


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("shape", JVP_SHAPES, ids=shape_id)
def test_jvp_features_over_the_dispatch(shape, dtype):
    """eps and all eight rows per (trajectory, particle) - the input row, the
    D + m tangent rows at the clamped action, the zero rows - against the
    model; nothing else written."""
    exp = run_jvp(shape, dtype, "features",
                  (dtype_id(dtype), shape_id(shape), "features"))
    D, _, m, _ = shape
    assert bool((exp["F"][:, 1 + D + m:] == 0).all())


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("ups,independent", JVP_VARIANTS, ids=JVP_VARIANT_IDS)
@pytest.mark.parametrize("shape", JVP_SHAPES, ids=shape_id)
def test_jvp_moments_over_the_dispatch(shape, ups, independent, dtype):
    """Xp_next, Z_next, F_z[b][1], F_u[b][1] from the model's eps and a
    synthetic network output, with `eps_out` NULL and given
    (`independent_noise` 0 and 1); F_z / F_u of the other time steps still
    SENT."""
    run_jvp(shape + (ups, independent), dtype, "moments",
            (dtype_id(dtype), shape_id(shape),
             JVP_VARIANT_IDS[JVP_VARIANTS.index((ups, independent))]))


@pytest.mark.gpu
@DTYPES
def test_jvp_pair_skips_and_packs(dtype):
    """slot = (0, -1, 1) at (3, (1,), 2), P = 33: nothing of trajectory 1 is
    read (its network rows do not exist) or written, trajectory 2's network
    rows are those of rank 1."""
    key = (3, (1,), 2, 33, True, False, True)
    tag = (dtype_id(dtype), "D3-slot")
    exp = run_jvp(key, dtype, "features", tag + ("features",))
    assert bool(torch.isnan(exp["F"][2 * 33:]).all())
    assert not bool(torch.isnan(exp["F"][:2 * 33]).any())
    exp = run_jvp(key, dtype, "moments", tag + ("moments",))
    assert bool(torch.isnan(exp["Z_next"][1]).all())
    assert not bool(torch.isnan(exp["Z_next"][[0, 2]]).any())


# ---- encode()'s diagonal fall-back
def fallback_particles(dtype):
    """(a, a), (-a, -a), (0, 0): the mean is 0 and the covariance a^2 [[1, 1],
    [1, 1]], exactly; every jitter <= 10 is absorbed by a^2 (2^80 in f64, 2^40
    in f32) and the second pivot is exactly 0 at every rung."""
    a = 2.0 ** 40 if dtype == torch.float64 else 2.0 ** 20
    X = torch.tensor([[a, a], [-a, -a], [0.0, 0.0]], dtype=torch.float64)
    return a, X, torch.tensor([0.0, 0.0, a, 0.0, a], dtype=torch.float64)


def fallback_step_case(dtype):
    a = dict(step_case(2, (), 1, 2, 1, 1, 3, False))
    _, X, _ = fallback_particles(dtype)
    zero = torch.zeros(2, 2, dtype=torch.float64)
    a.update(Q=zero, Q_term=zero, dX_mean=torch.zeros(2, dtype=torch.float64),
             Xp=X.expand(2, 1, 3, 2).contiguous(),
             net_outs=[None, torch.zeros(6, 2, dtype=torch.float64)])
    return a


@DTYPES
def test_fallback_model_and_package_encode_agree(dtype):
    """CPU: the model's encode() and the package's - encode(M, C) raises, the
    model's forward then encodes the standard deviations (models/bnn.py) -
    both give (0, 0 | a, 0, a) exactly; and so does the model's whole step."""
    from pddp_amd.utils.encoding import StateEncoding, encode
    _, X, want = fallback_particles(dtype)
    X = X.to(dtype)
    mean, cov = bm.particle_moments(X)
    z, r = bm.encode(mean, cov)
    assert r is None and torch.equal(z.double(), want)
    enc = StateEncoding.UPPER_TRIANGULAR_CHOLESKY
    with pytest.raises(RuntimeError):
        encode(mean, C=cov, encoding=enc)
    assert torch.equal(encode(mean, S=X.std(dim=-2), encoding=enc).double(),
                       want)
    outs = model_rollout(fallback_step_case(dtype), dtype)
    assert outs[1]["rung_state"] == [None, None]
    assert torch.equal(outs[1]["z"], want.expand(2, 1, 5))
    assert torch.isfinite(outs[1]["Jc"]).all()


@pytest.mark.gpu
@DTYPES
def test_fallback_moment_step_is_exact(dtype):
    """D = 2, P = 3, no angles, m = 1, zero Q, the particles fed as Xp with a
    zero network output: Zc[:, 1] = (0, 0 | a, 0, a) exactly, the particles
    unchanged, the costs finite and the model's."""
    _, X, want = fallback_particles(dtype)
    a = fallback_step_case(dtype)
    ref = model_rollout(a, torch.float64)
    run = StepRun(a, dtype)
    run.call(0)
    run.call(1)
    assert torch.equal(run.view["Zc"][:, 1].cpu().double(),
                       want.expand(2, 1, 5))
    assert torch.equal(run.view["Xp"].cpu().double(), a["Xp"])
    Jc = run.view["Jc"].cpu().double()
    assert torch.isfinite(Jc).all()
    assert rel(Jc, ref[1]["Jc"]) <= (1e-10 if dtype == torch.float64
                                     else 16 * EPS32)


@pytest.mark.gpu
@DTYPES
def test_fallback_jvp_moments_is_exact(dtype):
    """The same particles through the moments kernel: Z_next = (0, 0 | a, 0,
    a) exactly - the entry above the diagonal is zero, not what the last
    failed factorisation left there - and Xp_next the particles."""
    _, X, want = fallback_particles(dtype)
    a = dict(jvp_case(2, (), 1, 3))
    a.update(dX_mean=torch.zeros(2, dtype=torch.float64),
             Xp=X.expand(JVP_B, 3, 2).contiguous(),
             net_out=torch.zeros(JVP_B * 3, bm.NET_ROWS, 2,
                                 dtype=torch.float64))
    run = JvpRun(a, dtype, eps=torch.zeros(JVP_B, 3, 2, dtype=torch.float64))
    run.call("moments")
    assert torch.equal(run.view["Z_next"].cpu().double(),
                       want.expand(JVP_B, 5))
    assert torch.equal(run.view["Xp_next"].cpu().double(), a["Xp"])
    for k in JACOBIANS:
        assert torch.isfinite(run.view[k][:, JVP_T]).all(), k


# ---- host wiring
def made_up_problem(D, m, ang, H, P):
    """A learned problem no example has: the BNN model class and an
    AugmentedQRCost over the same index lists, float64 on the device."""
    from pddp_amd.examples._common import AugmentedQRCost
    from pddp_amd.models.bnn import bnn_dynamics_model_factory
    non = qm.non_angular(D, ang)
    cls = bnn_dynamics_model_factory(D, m, [H, H], list(ang) or None,
                                     non if ang else None)
    model = cls(n_particles=P).double().cuda().eval()
    with torch.no_grad():  # keep the learned dynamics gentle: dx ~ 1e-2
        model.model.out.weight.mul_(0.05)
        model.model.out.bias.mul_(0.05)

    class Plant(object):
        state_size = D
        action_size = m
        angular_indices = list(ang)
        non_angular_indices = non

    class Cost(AugmentedQRCost):
        model_class = Plant
    c = constants(D, ang, m, 3)
    cost = Cost(c["Q"], c["R"], Q_term=c["Q_term"], x_goal=c["x_goal"],
                u_goal=c["u_goal"]).double().cuda()
    return model, cost


def host_solver(model, cost, D, m, B, N, native, model_opts):
    import pddp_amd
    from pddp_amd.controllers.ilqr import fit_alphas
    from pddp_amd.controllers.plugin import TorchProblem
    from pddp_amd.controllers.solver import ILQRSolver
    dt = torch.float64
    enc = pddp_amd.StateEncoding.DEFAULT
    n = qm.encoded_size(D)
    plugin = TorchProblem(model, cost, enc, dict(model_opts), {})
    plugin.use_native_bnn = native
    plugin.use_native_bnn_jvp = native
    plugin.use_native_cost = native
    s = ILQRSolver(None, B, N, dt, "cuda", torch.full((m,), -1.0, dtype=dt),
                   torch.full((m,), 1.0, dtype=dt), fit_alphas(dt, "cuda"),
                   plugin=plugin, n=n, m=m)
    g = torch.Generator().manual_seed(1)
    z0 = torch.stack([pddp_amd.GaussianVariable(
        0.3 * torch.randn(D, generator=g, dtype=dt),
        var=1e-2 * torch.ones(D, dtype=dt)).encode(enc)
        for _ in range(B)]).cuda()
    U = (0.1 * torch.randn(B, N, m, generator=g, dtype=dt)).cuda()
    U[:, 2] = 2.0  # one clamped action: derivatives at the bound
    s.set_nominal(z0, U)
    gains = 1e-1 * torch.randn(s.gains.shape, generator=g, dtype=dt).cuda()
    return s, plugin, gains


def rel_dev(x, y, floor):
    return float((x - y).abs().max()) / max(float(y.abs().max()), floor)


@pytest.mark.gpu
@pytest.mark.parametrize("model_opts", [
    {"use_predicted_std": False},
    {"use_predicted_std": True, "independent_noise": False}],
    ids=["mean_only", "predicted_std"])
def test_host_wiring_at_a_shape_no_example_has(model_opts):
    """D = 3, m = 2, angle 1, P = 20, f64, B = 3, N = 5 through
    TorchProblem: the native line search against the torch path and the
    native Jacobians against autograd, at the bars of test_bnn_f64.py."""
    torch.manual_seed(7)
    D, m, B, N = 3, 2, 3, 5
    model, cost = made_up_problem(D, m, (1,), 64, 20)
    res, recs = [], []
    for native in (True, False):
        s, plugin, gains = host_solver(model, cost, D, m, B, N, native,
                                       model_opts)
        s.gains.copy_(gains)
        with torch.no_grad():
            assert plugin._bnn_native_ok(s) == native
            assert plugin._bnn_jvp_ok(s) == native
        s.line_search()
        res.append((s.Zc.clone(), s.Uc.clone(), s.Jc.clone(), s.Z.clone()))
        model.output = {}
        s.derivs()
        torch.cuda.synchronize()
        # (the QR cost kernel is built for D = 2, 4, 6: autograd here)
        assert plugin.last_derivs_path == {
            "dynamics": "hip" if native else "autograd", "cost": "autograd"}
        recs.append((s.rec.clone(), s.L.clone(), s.lay, s.n))
    (Za, Ua, Ja, Zna), (Zb, Ub, Jb, Znb) = res
    assert rel_dev(Zna, Znb, 0.0) < 1e-10
    assert float((Znb[:, 1:] - Znb[:, :1]).abs().max()) > 1e-4
    assert torch.isfinite(Za).all() and torch.isfinite(Ja).all()
    for x, y, name in ((Za, Zb, "Zc"), (Ua, Ub, "Uc"), (Ja, Jb, "Jc")):
        assert rel_dev(x, y, 1e-6) < 1e-9, (name, rel_dev(x, y, 1e-6))
    (ra, La, lay, n), (rb, Lb, _, _) = recs
    assert torch.isfinite(ra).all()
    for name, o, w in (("F_z", lay.o_Fz, n * n), ("F_u", lay.o_Fu, n * m),
                       ("L_zz", lay.o_Lzz, n * n), ("L_uz", lay.o_Luz, m * n),
                       ("L_z", lay.o_Lz, n), ("L_uu", lay.o_Luu, m * m),
                       ("L_u", lay.o_Lu, m)):
        e = rel_dev(ra[:, :, o:o + w], rb[:, :, o:o + w], 1e-3)
        assert e < 1e-8, (name, e)
    assert rel_dev(La, Lb, 0.0) < 1e-10


@pytest.mark.gpu
def test_host_wiring_at_the_rendezvous_shape():
    """D = 8, m = 2, no angles (n = 44): the line search runs on the moment
    step's runtime-D kernel and equals the torch path; the Jacobian pair
    refuses the shape, and the derivative rollout says so."""
    torch.manual_seed(8)
    D, m, B, N = 8, 2, 3, 5
    model, cost = made_up_problem(D, m, (), 64, 20)
    res = []
    for native in (True, False):
        s, plugin, gains = host_solver(model, cost, D, m, B, N, native, {})
        s.gains.copy_(gains)
        with torch.no_grad():
            assert plugin._bnn_native_ok(s) == native
            assert not plugin._bnn_jvp_ok(s)
        s.line_search()
        res.append((s.Zc.clone(), s.Uc.clone(), s.Jc.clone()))
        if native:
            model.output = {}
            s.derivs()
            assert plugin.last_derivs_path["dynamics"] == "autograd"
            assert torch.isfinite(s.rec).all()
    for x, y, name in zip(res[0], res[1], ("Zc", "Uc", "Jc")):
        assert torch.isfinite(x).all()
        assert rel_dev(x, y, 1e-6) < 1e-9, (name, rel_dev(x, y, 1e-6))


# --------------------------------------------------------------- CPU tests --
def _package_model(D, m, ang, P, g):
    """A D-state BNNDynamicsModel with an [8, 8] network in float64 on the
    CPU, normalisation as constants() has it, its noise caches set."""
    from pddp_amd.models.bnn import bnn_dynamics_model_factory
    non = qm.non_angular(D, ang)
    torch.manual_seed(5)
    model = bnn_dynamics_model_factory(D, m, [8, 8], list(ang), non)(
        n_particles=P).double().eval()
    c = constants(D, ang, m, 1)
    for k in ("X_mean", "X_std_inv", "dX_mean", "dX_std"):
        setattr(model, k, c[k].clone())
    with torch.no_grad():
        model.model.out.weight.mul_(0.2)
    model.eps_in = {0: standardised(P, D, g), 1: standardised(P, D, g)}
    model.eps_out = {i: standardised(P, D, g) for i in range(3)}
    return model, c


def _stub_cost(D, m, ang, c):
    from pddp_amd.examples._common import AugmentedQRCost

    class Plant(object):
        state_size = D
        action_size = m
        angular_indices = list(ang)
        non_angular_indices = qm.non_angular(D, ang)

    class Cost(AugmentedQRCost):
        model_class = Plant
    return Cost(c["Q"], c["R"], Q_term=c["Q_term"], x_goal=c["x_goal"],
                u_goal=c["u_goal"]).double()


PINNED = pytest.mark.parametrize("D,m,ang", [(3, 2, (1,)), (4, 1, (2,))],
                                 ids=["D3-m2", "cartpole"])
OPTS = pytest.mark.parametrize("opts", [
    {}, {"use_predicted_std": True},
    {"use_predicted_std": True, "independent_noise": True}],
    ids=JVP_VARIANT_IDS)


@PINNED
@OPTS
def test_step_model_vs_package_rollout(D, m, ang, opts):
    """bm.step() against BNNDynamicsModel.forward plus the cost module along a
    three-step rollout of B A = 4 rows under the control law (float64, CPU; the
    goldens pin the package to the reference): states, actions and costs to
    1e-10."""
    import pddp_amd
    enc = pddp_amd.StateEncoding.DEFAULT
    B, A, N, P = 2, 2, 3, 12
    g = torch.Generator().manual_seed(21)
    model, c = _package_model(D, m, ang, P, g)
    cost = _stub_cost(D, m, ang, c)
    ups = bool(opts.get("use_predicted_std"))
    a = dict(step_case(D, ang, m, B, A, N, P, ups))
    a.update({k: c[k] for k in c})
    e0 = model.eps_in[0]
    a["Xp"] = torch.stack([a["Z"][b, 0, :D] + e0 @ bm.upper_of(a["Z"][b, 0], D)
                           for b in range(B)])[:, None].repeat(1, A, 1, 1)
    n = qm.encoded_size(D)
    Xp, J = a["Xp"], a["J"]
    z = a["Z"][:, :1].expand(B, A, n).reshape(B * A, n)
    Jp = torch.zeros(B * A, dtype=torch.float64)
    with torch.no_grad():
        for t in range(N + 1):
            y = None
            if t > 0:
                y = model.model(F.reshape(B * A, P, -1)).reshape(B * A * P, -1)
            o = bm.step(dict(a, Xp=Xp, J=J, net_out=y, out_dim=2 * D,
                             eps_out=model.eps_out[t - 1] if ups and t > 0
                             else None), t)
            Xp, J, F = o["Xp"], o["J"], o["F"]
            assert rel(o["z"].reshape(B * A, n), z) <= 1e-10, t
            if t == N:
                Jp = Jp + cost(z, None, t - 1, terminal=True, encoding=enc)
                assert rel(o["Jc"].reshape(-1), Jp) <= 1e-10
                break
            u = o["u"].reshape(B * A, m)
            Jp = Jp + cost(z, u, t, terminal=False, encoding=enc)
            assert rel(o["J"].reshape(-1), Jp) <= 1e-10, t
            z = model(z, u, t, enc, **opts)
    assert int((o["u"] != o["u"]).sum()) == B * A * m  # (no action at t = N)


@PINNED
@OPTS
def test_jvp_model_vs_package_autograd(D, m, ang, opts):
    """bm.jvp_features, the network in forward mode written out layer by
    layer, bm.jvp_moments - against TorchProblem._dyn_derivs (autograd over
    the replicated input) and the package's forward on the CPU: Z_next, F_z,
    F_u to 1e-10."""
    import pddp_amd
    from pddp_amd.controllers.plugin import TorchProblem
    enc = pddp_amd.StateEncoding.DEFAULT
    B, P, t = 2, 12, JVP_T
    g = torch.Generator().manual_seed(22)
    model, c = _package_model(D, m, ang, P, g)
    ups = bool(opts.get("use_predicted_std"))
    a = dict(jvp_case(D, ang, m, P, ups, bool(opts.get("independent_noise"))))
    a.update({k: c[k] for k in c}, B=B, Z=a["Z"][:B], U=a["U"][:B],
             out_dim=2 * D, eps_out=model.eps_out[t] if ups else None)
    a["Xp"] = torch.stack([
        a["Z"][b, t, :D] + model.eps_in[t] @ bm.upper_of(a["Z"][b, t], D)
        for b in range(B)])
    fe = bm.jvp_features(a, t)
    assert rel(fe["eps"], model.eps_in[t].expand(B, P, D)) <= 1e-10
    net = model.model
    with torch.no_grad():
        net(fe["F"][:, 0].reshape(B, P, -1))  # (draws the masks)
        m1 = net.drops[0]._mask(net.drops[0].noise).repeat(B, 1).unsqueeze(1)
        m2 = net.drops[1]._mask(net.drops[1].noise).repeat(B, 1).unsqueeze(1)
        h = fe["F"] @ net.hidden[0].weight.t()
        h[:, :1] += net.hidden[0].bias
        h = torch.where(h[:, :1] * m1 > 0, h * m1, torch.zeros_like(h))
        h = h @ net.hidden[1].weight.t()
        h[:, :1] += net.hidden[1].bias
        h = torch.where(h[:, :1] * m2 > 0, h * m2, torch.zeros_like(h))
        Y = h @ net.out.weight.t()
        Y[:, :1] += net.out.bias
    mo = bm.jvp_moments(dict(a, eps=fe["eps"], net_out=Y), t)
    plugin = TorchProblem(model, None, enc, dict(opts), {})
    u = torch.maximum(torch.minimum(a["U"][:, t], c["u_max"]), c["u_min"])
    assert bool((u != a["U"][:, t]).any())
    model.output = {}
    F_z, F_u = plugin._dyn_derivs(a["Z"][:, t], u, t)
    model.output = {}
    with torch.no_grad():
        zn = model(a["Z"][:, t], u, t, enc, **opts)
    assert rel(mo["Z_next"], zn) <= 1e-10
    assert rel(mo["F_z"], F_z) <= 1e-10, rel(mo["F_z"], F_z)
    assert rel(mo["F_u"], F_u) <= 1e-10, rel(mo["F_u"], F_u)
    assert float(F_u.abs().max()) > 0


STEP_POINTERS = ("Z", "U", "gains", "alphas", "Q", "Q_term", "R", "x_goal",
                 "u_goal", "X_mean", "X_std_inv", "dX_mean", "dX_std", "Xp",
                 "F", "Zc", "Uc", "J", "Jc")
JVP_POINTERS = ("Z", "U", "X_mean", "X_std_inv", "dX_mean", "dX_std", "Xp",
                "eps", "F")


def _refusal_struct(cls, word, pointers, **change):
    """Cartpole's shape (D = 4, angle 2, m = 1), every required pointer a host
    word nobody reads."""
    st = cls()
    st.B, st.P, st.N, st.t = 2, 10, 3, 1
    if hasattr(st, "A"):
        st.A = 2
    fill_shape(st, 4, (2,), (0, 1, 3), 1)
    st.out_dim = 8
    for k in pointers:
        setattr(st, k, word)
    for k, v in change.items():
        setattr(st, k, v)
    return st


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_entry_points_refuse_before_any_launch(t):
    """CPU (every answer comes before the first HIP call): PDDP_E_BADARG (-1)
    for a NULL struct and each missing pointer; PDDP_E_UNSUPPORTED for D = 9,
    m = 3, P = 129, three angles, n_non + n_ang != D, a wrong in_dim, out_dim
    < 2 D with eps_out given; for the Jacobian pair also D = 7, D + m = 8 and
    t = N (a step of the trajectory, without a Jacobian)."""
    from pddp_amd import _native
    word = (ctypes.c_double * 2)()
    q = ctypes.addressof(word)
    lib = _native.lib()
    UNS = _native.E_UNSUPPORTED
    common = [dict(D=9, n_non=8, in_dim=11), dict(n_ang=3, n_non=1, in_dim=8),
              dict(n_non=2), dict(n_non=4), dict(in_dim=7), dict(in_dim=5),
              dict(out_dim=7, eps_out=q), dict(out_dim=3)]
    step = getattr(lib, "pddp_bnn_moment_step_" + t)
    mk = lambda **ch: _refusal_struct(_native.BnnStep, q,
                                      STEP_POINTERS + ("net_out",), **ch)
    assert step(None, None) == -1
    for k in STEP_POINTERS + ("net_out",):
        assert step(ctypes.byref(mk(**{k: None})), None) == -1, k
    for ch in common + [dict(m=3, in_dim=8), dict(P=129), dict(m=0, in_dim=5)]:
        assert step(ctypes.byref(mk(**ch)), None) == UNS, ch
    assert step(ctypes.byref(mk(t=4)), None) == -1
    for name in ("features", "moments"):
        fn = getattr(lib, "pddp_bnn_jvp_%s_%s" % (name, t))
        need = JVP_POINTERS + (("net_out", "F_z", "F_u")
                               if name == "moments" else ())
        mk = lambda **ch: _refusal_struct(_native.BnnJvp, q, need, **ch)
        assert fn(None, None) == -1
        for k in need:
            assert fn(ctypes.byref(mk(**{k: None})), None) == -1, (name, k)
        for ch in common + [
                dict(D=7, n_non=6, in_dim=9),              # D = 7
                dict(m=4, in_dim=9),                       # D + m = 8
                dict(D=6, n_non=5, m=2, in_dim=9),         # D + m = 8
                dict(t=3)]:                                # t = N
            assert fn(ctypes.byref(mk(**ch)), None) == UNS, (name, ch)
        assert fn(ctypes.byref(mk(t=4)), None) == -1
        assert fn(ctypes.byref(mk(t=-1)), None) == -1
    assert lib.pddp_bnn_jvp_group(4, 2) == 32 and \
        lib.pddp_bnn_jvp_group(3, 2) == 16 and \
        lib.pddp_bnn_jvp_group(6, 2) == 0 and lib.pddp_bnn_jvp_group(7, 1) == 0


MUTANT_BARS = dict(F_z=1e-8, F_u=1e-8)


def _rejected(got, ref):
    bars = {k: MUTANT_BARS.get(k, 1e-10) for k, v in ref.items()
            if torch.is_tensor(v) and v.is_floating_point()
            and rel(v, v) is not None}
    return [k for k, _, _ in failures(got, ref, bars)]


def test_the_comparison_rejects_four_mutants():
    """failures() at the f64 bars, the model against itself broken in one
    place, on the smallest shape of each family: the covariance over P, the
    differential of the factor without the halved diagonal of Phi, the sin
    and cos slots exchanged, `alpha k` without alpha - each is rejected, in
    the blocks it should move; the unbroken model passes against itself."""
    key = (1, (0,), 1, 2, 2, 1, 15, False)
    good = step_model(key, torch.float64)
    a = step_case(*key)
    assert all(not _rejected(o, g) for o, g in zip(
        model_rollout(a, torch.float64), good))
    by = {}
    for mut in ("cov_P", "sincos_swap", "no_alpha"):
        outs = model_rollout(a, torch.float64, mut)
        by[mut] = [_rejected(o, g) for o, g in zip(outs, good)]
    assert by["cov_P"][0] == [] and {"z", "J"} <= set(by["cov_P"][1])
    assert "F" in by["sincos_swap"][0] and "z" not in by["sincos_swap"][0]
    assert {"u", "J", "F"} <= set(by["no_alpha"][0])
    jkey = (1, (0,), 1, 9)
    fe, mo = jvp_model(jkey, torch.float64)
    ja = jvp_case(*jkey)
    assert _rejected(bm.jvp_features(ja, JVP_T, "sincos_swap"), fe) == ["F"]
    args = dict(ja, eps=fe["eps"])
    assert not _rejected(bm.jvp_moments(args, JVP_T), mo)
    assert {"Z_next", "F_z"} <= set(
        _rejected(bm.jvp_moments(args, JVP_T, "cov_P"), mo))
    bad = _rejected(bm.jvp_moments(args, JVP_T, "phi_diag"), mo)
    assert "F_z" in bad and "Z_next" not in bad and "Xp_next" not in bad
