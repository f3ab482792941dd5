"""`pddp_qr_cost_derivs_f32 / _f64` (csrc/qr_cost_derivs.hip) called directly,
against tests/qr_cost_model.py - the cost restated in float64 and
differentiated by torch.autograd.functional - over the whole dispatch table
(D in {2, 4, 6} x 0, 1, 2 angles, index sets no example has), m = 1 and 2, with
and without bounds, an asymmetric Q, Q_term != Q, non-zero goals, and four
regimes of the encoded state:

  (a) Cholesky diagonal^2 in [0.02, 0.07], off-diagonals 0.05 randn, means N(0, 1)
  (b) diagonal^2 in [1e-6, 1e-5], off-diagonals 1e-3 randn
  (c) the Cholesky part exactly zero
  (d) angle variances in [4, 9], angle means 50 randn

And once on the nominal of an ILQRSolver under the DEFAULT encoding, beside
the cost blocks of `pddp_derivs_*` (csrc/default_kernels.hip), which evaluates
the same text (csrc/gauss_cost_body.inc): both against the model, by one rule.

CPU tests: the model against the package's float64 torch path (which the
goldens pin), the entry point's refusals, and the batch invariance of
`encode` under UPPER_TRIANGULAR_CHOLESKY.

The f32 bars are measured inside the test: the package's torch float32
autograd path (the reference's own arithmetic in f32) is run on the CPU on the
same inputs, and the kernel may be 8 x as far from the float64 model as that
path is, per block, and no closer than 16 eps32 is asked of it (DESIGN.md
5.1 holds the measured pairs)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import qr_cost_model as qm

B, N = 3, 4
EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
# (D, angular indices); non-angular = the remaining indices, ascending
SHAPES = [(2, ()), (2, (0,)), (2, (0, 1)),
          (4, ()), (4, (2,)), (4, (0, 3)),
          (6, ()), (6, (4,)), (6, (1, 2)), (6, (0, 5))]
SHAPE_IDS = ["D%d-ang%s" % (D, "".join(map(str, a)) or "none")
             for D, a in SHAPES]
BLOCKS = ("L", "L_z", "L_u", "L_zz", "L_uz", "L_uu")


# ------------------------------------------------------------------ inputs --
def constants(D, ang, m):
    """Q = A^T A + 0.1 I (plus a skew part of the same size for every other
    shape), Q_term = 3 Q^T, R symmetric positive definite with an off-diagonal
    entry, non-zero goals, bounds - float64, all exactly representable in
    float32 so that both dtypes see the same problem."""
    idx = SHAPES.index((D, tuple(ang)))
    g = torch.Generator().manual_seed(1000 + idx)
    NA = D + len(ang)
    A = torch.randn(NA, NA, generator=g, dtype=torch.float64)
    Q = A.t() @ A + 0.1 * torch.eye(NA, dtype=torch.float64)
    if idx % 2 == 1:
        S = torch.randn(NA, NA, generator=g, dtype=torch.float64)
        K = S - S.t()
        if NA > 1:
            Q = Q + K * (Q.norm() / K.norm())
    r32 = lambda t: t.float().double()
    Q = r32(Q)
    R = r32(torch.tensor([[0.7, 0.2], [0.2, 0.4]], dtype=torch.float64)[:m, :m])
    return dict(
        Q=Q, Q_term=r32(3.0 * Q.t()), R=R,
        x_goal=r32(0.5 * torch.randn(NA, generator=g, dtype=torch.float64)),
        u_goal=r32(torch.tensor([0.3, -0.2], dtype=torch.float64)[:m]),
        u_min=r32(torch.tensor([-0.8, -0.6], dtype=torch.float64)[:m]),
        u_max=r32(torch.tensor([0.9, 0.7], dtype=torch.float64)[:m]))


def states(D, ang, regime, count, seed):
    """[count, n] float64 encoded states of one regime."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    uni = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    mean = rnd(count, D)
    U = torch.zeros(count, D, D, dtype=torch.float64)
    if regime in "ad":
        diag, off = (0.02 + 0.05 * uni(count, D)).sqrt(), 0.05 * rnd(count, D, D)
    elif regime == "b":
        diag, off = (1e-6 + 9e-6 * uni(count, D)).sqrt(), 1e-3 * rnd(count, D, D)
    else:
        diag, off = torch.zeros(count, D, dtype=torch.float64), U
    U = torch.triu(off, 1) + torch.diag_embed(diag)
    if regime == "d":
        for a in ang:
            target = 4.0 + 5.0 * uni(count)
            U[:, :, a] *= (target / (U[:, :, a] ** 2).sum(-1)).sqrt()[:, None]
            mean[:, a] = 50.0 * rnd(count)
    iu = torch.triu_indices(D, D)
    return torch.cat([mean, U[:, iu[0], iu[1]]], -1)


def actions(m, seed):
    """[B, N, m]: inside the bounds of constants() except one action per
    trajectory, on either side."""
    g = torch.Generator().manual_seed(seed)
    U = torch.rand(B, N, m, generator=g, dtype=torch.float64) - 0.5
    for b in range(B):
        U[b, (b + 1) % N, b % m] = 2.0 if b % 2 else -2.0
    return U


def case_inputs(D, ang, m, regime, dtype):
    """Constants, Z [B, N+1, n], U [B, N, m] as float64 tensors holding the
    values the run sees (rounded to float32 first for a float32 run)."""
    idx = SHAPES.index((D, tuple(ang)))
    c = constants(D, ang, m)
    Z = states(D, ang, regime, B * (N + 1), 7 * idx + ord(regime)).reshape(
        B, N + 1, -1)
    U = actions(m, 31 * idx + m)
    if dtype == torch.float32:
        Z, U = Z.float().double(), U.float().double()
    return c, Z, U


def model_on(D, ang, m, c, Z, Uc):
    """The float64 model at every (trajectory, step): Z [B, N+1, n], Uc [B, N,
    m] the clamped actions -> dict of blocks in the kernel's layouts, L0 [B,
    N+1] without the jitter term, trQ [B, N+1]."""
    non = qm.non_angular(D, ang)
    Bq, N1, n = Z.shape
    args = (D, list(ang), non, m, c["Q"], c["Q_term"], c["R"], c["x_goal"],
            c["u_goal"])
    st = qm.evaluate_batch(*args, Z[:, :-1].reshape(-1, n), Uc.reshape(-1, m))
    te = qm.evaluate_batch(*args, Z[:, -1], None, terminal=True)
    out = {}
    for k, v in st.items():
        v = v.reshape(Bq, N1 - 1, *v.shape[1:])
        out[k] = torch.cat([v, te[k].unsqueeze(1)], 1) if k in te else v
    return out


def clamped(c, U, bounds):
    return torch.maximum(torch.minimum(U, c["u_max"]), c["u_min"]) \
        if bounds else U


@functools.lru_cache(maxsize=None)
def model_blocks(D, ang, m, regime, dtype, bounds):
    """model_on() at a case's inputs, computed once per case and shared."""
    c, Z, U = case_inputs(D, ang, m, regime, dtype)
    return model_on(D, ang, m, c, Z, clamped(c, U, bounds))


def stub_cost(D, ang, c, m):
    """An AugmentedQRCost whose `model_class` is a plain class."""
    from pddp_amd.examples._common import AugmentedQRCost

    class Plant(object):
        state_size = D
        action_size = m
        angular_indices = list(ang)
        non_angular_indices = qm.non_angular(D, ang)

    class StubCost(AugmentedQRCost):
        model_class = Plant
    return StubCost(c["Q"], c["R"], Q_term=c["Q_term"], x_goal=c["x_goal"],
                    u_goal=c["u_goal"])


def torch_path(cost, Z, Uc, dtype):
    """The package's torch autograd path (controllers/plugin.py:_cost_derivs =
    utils/evaluation.py batch_eval_cost) on the CPU in `dtype`: Z [B, N+1, n],
    Uc [B, N, m] already clamped -> blocks in the kernel's layouts, float64."""
    import pddp_amd
    from pddp_amd.controllers.plugin import TorchProblem
    cost = cost.to(dtype)
    plugin = TorchProblem(None, cost, pddp_amd.StateEncoding.DEFAULT, {}, {})
    Bq, N1, n = Z.shape
    m = Uc.shape[-1]
    z, u = Z.to(dtype), Uc.to(dtype)
    st = plugin._cost_derivs(z[:, :-1].reshape(-1, n), u.reshape(-1, m), 0,
                             False)
    te = plugin._cost_derivs(z[:, -1], None, 0, True)
    cat = lambda a, b_, tail: torch.cat(
        [a.reshape(Bq, N1 - 1, *tail), b_.reshape(Bq, 1, *tail)], 1).double()
    return dict(L=cat(st[0], te[0], ()), L_z=cat(st[1], te[1], (n,)),
                L_zz=cat(st[3], te[3], (n, n)),
                L_u=st[2].reshape(Bq, N1 - 1, m).double(),
                L_uz=st[4].reshape(Bq, N1 - 1, m, n).double(),
                L_uu=st[5].reshape(Bq, N1 - 1, m, m).double())


def rel(a, ref):
    """max |a - ref| relative to the block's largest reference entry."""
    top = float(ref.abs().max())
    if top == 0.0:  # (L_uz: the cost has no term in both z and u)
        return 0.0 if bool((a == 0).all()) else float("inf")
    return float((a - ref).abs().max()) / top


def value_error(L, mo, rungs):
    """The value block against L0 + rung tr(Q) with, per entry, the rung of
    `rungs` that fits best: (error relative to the largest |L0|, the rungs
    chosen [B, N+1])."""
    cand = torch.stack([mo["L0"] + r * mo["trQ"] for r in rungs], -1)
    err, pick = (L.unsqueeze(-1) - cand).abs().min(-1)
    chosen = torch.tensor(rungs, dtype=torch.float64)[pick]
    return float(err.max()) / float(mo["L0"].abs().max()), chosen


# --------------------------------------------------------------- CPU tests --
def _shipped(name):
    import pddp_amd
    mod = getattr(pddp_amd.examples, name)
    cost = [getattr(mod, k) for k in dir(mod) if k.endswith("Cost")
            and k != "AugmentedQRCost"][0]()
    return cost, cost.model_class


@pytest.mark.parametrize("name", ["cartpole", "pendulum", "double_cartpole",
                                  "stub-D4-ang03", "stub-D6-ang12"])
def test_model_vs_package_float64_path(name):
    """tests/qr_cost_model.py against the package's float64 torch path (DEFAULT
    encoding; pinned to the reference by the goldens) for the three shipped
    costs and for a stub cost with index sets no example has and m = 2: the
    model's L0 + 1e-12 tr(Q) and its derivatives, stage and terminal steps, to
    1e-12 of the block's largest entry."""
    if name.startswith("stub"):
        D, ang = {"stub-D4-ang03": (4, (0, 3)), "stub-D6-ang12": (6, (1, 2))}[name]
        m = 2
        c = constants(D, ang, m)
        cost = stub_cost(D, ang, c, m)
    else:
        cost, mc = _shipped(name)
        D, m = mc.state_size, mc.action_size
        ang = tuple(int(i) for i in mc.angular_indices)
        assert qm.non_angular(D, ang) == [int(i) for i in
                                          mc.non_angular_indices]
        NA = D + len(ang)
        f64 = lambda t, k: torch.as_tensor(t).detach().double().expand(
            *k).clone()
        c = dict(Q=f64(cost.Q, (NA, NA)), Q_term=f64(cost.Q_term, (NA, NA)),
                 R=f64(cost.R, (m, m)), x_goal=f64(cost.x_goal, (NA,)),
                 u_goal=f64(cost.u_goal, (m,)))
    non = qm.non_angular(D, ang)
    n = qm.encoded_size(D)
    Z = states(D, ang, "a", B * (N + 1), 5).reshape(B, N + 1, n)
    U = 0.5 * torch.randn(B, N, m, dtype=torch.float64,
                          generator=torch.Generator().manual_seed(6))
    pk = torch_path(cost, Z, U, torch.float64)
    mo = model_on(D, ang, m, c, Z, U)
    assert rel(pk["L"], mo["L0"] + 1e-12 * mo["trQ"]) <= 1e-12
    for k in BLOCKS[1:]:
        assert pk[k].shape == mo[k].shape
        assert rel(pk[k], mo[k]) <= 1e-12, (name, k, rel(pk[k], mo[k]))
    if name != "double_cartpole":
        assert float(mo["L_uu"].abs().min()) > 0 and \
            float(mo["L_zz"].abs().max()) > 0


def test_batched_model_is_the_pointwise_model():
    """evaluate_batch() (torch.func) against evaluate()
    (torch.autograd.functional.jacobian / hessian of the same forward), point
    by point, stage and terminal, at the m = 2 stub shapes: 1e-13 of the
    block's largest entry."""
    for D, ang in ((2, (0, 1)), (4, (0, 3)), (6, (1, 2))):
        m = 2
        c = constants(D, ang, m)
        non = qm.non_angular(D, ang)
        Z = states(D, ang, "d", 3, 9)
        U = torch.tensor([[0.1, -0.4], [0.9, 0.2], [-0.3, 0.7]],
                         dtype=torch.float64)
        args = (D, list(ang), non, m, c["Q"], c["Q_term"], c["R"],
                c["x_goal"], c["u_goal"])
        for term in (False, True):
            bt = qm.evaluate_batch(*args, Z, None if term else U,
                                   terminal=term)
            for i in range(3):
                pt = qm.evaluate(*args, Z[i], None if term else U[i],
                                 terminal=term)
                assert set(pt) == set(bt)
                for k, v in pt.items():
                    assert bt[k][i].shape == v.shape
                    assert rel(bt[k][i], v) <= 1e-13, (D, ang, term, k)
        assert float(bt["trQ"][0]) == float(torch.diagonal(c["Q_term"]).sum())


def test_ladder_and_cholesky_of_the_model():
    """ladder(): the doubles a repeated `*= 10.0` gives, 1e-12 first, 10 last
    or the value just below it; rung(): 1e-12 for a healthy matrix, the first
    rung above -lambda_min for an indefinite one, in both dtypes; None when
    the ladder is exhausted."""
    lad = qm.ladder()
    assert lad[0] == 1e-12 and len(lad) == 14 and lad[-1] <= 10.0 < lad[-1] * 10
    jit = 1e-12
    for v in lad:
        assert v == jit
        jit *= 10.0
    A = np.array([[2.0, 0.5], [0.5, 1.0]])
    for dt in (np.float32, np.float64):
        assert qm.rung(A, dt) == lad[0]
        # eigenvalues 0 and 2, shifted down by 3e-6: 1e-5 is the first rung
        S = np.array([[1.0, 1.0], [1.0, 1.0]]) - 3e-6 * np.eye(2)
        assert qm.rung(S, dt) == lad[7]
        assert qm.rung(-100.0 * np.eye(2), dt) is None
    assert qm.cholesky_ok(A) and not qm.cholesky_ok(-A)


def _qr_struct(D, ang, m, word):
    from pddp_amd import _native
    st = _native.QrCost()
    st.B, st.N, st.D, st.m = B, N, D, m
    non = qm.non_angular(D, ang)
    st.n_ang, st.n_non = len(ang), len(non)
    for i, v in enumerate(ang):
        st.ang[i] = v
    for i, v in enumerate(non):
        st.non[i] = v
    for k in ("Z", "U", "Q", "Q_term", "R", "x_goal", "u_goal", "L", "L_z",
              "L_u", "L_zz", "L_uz", "L_uu"):
        setattr(st, k, word)
    return st


def test_entry_point_refuses_before_any_launch():
    """CPU (every answer comes before the first HIP call; the non-null
    pointers are host words nobody reads), both dtypes: PDDP_E_BADARG (-1)
    for a NULL struct and for each NULL required pointer, PDDP_E_UNSUPPORTED
    for D = 3, m = 0, m = 3, three angles and n_non + n_ang != D."""
    from pddp_amd import _native
    word = (ctypes.c_double * 2)()
    q = ctypes.addressof(word)
    lib = _native.lib()
    for t in ("f32", "f64"):
        fn = getattr(lib, "pddp_qr_cost_derivs_" + t)
        assert fn(None, None) == -1, t
        for k in ("Z", "U", "Q", "Q_term", "R", "x_goal", "u_goal", "L",
                  "L_z", "L_u", "L_zz", "L_uz", "L_uu"):
            st = _qr_struct(4, (2,), 1, q)
            setattr(st, k, None)
            assert fn(ctypes.byref(st), None) == -1, (t, k)

        def refused(**change):
            st = _qr_struct(4, (2,), 1, q)
            for k, v in change.items():
                setattr(st, k, v)
            return fn(ctypes.byref(st), None)

        assert refused(D=3, n_non=2) == _native.E_UNSUPPORTED, t
        assert refused(m=0) == _native.E_UNSUPPORTED, t
        assert refused(m=3) == _native.E_UNSUPPORTED, t
        assert refused(n_ang=3, n_non=1) == _native.E_UNSUPPORTED, t
        assert refused(n_non=2) == _native.E_UNSUPPORTED, t
        assert refused(n_ang=2) == _native.E_UNSUPPORTED, t


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32],
                         ids=["f64", "f32"])
def test_encode_cholesky_is_batch_invariant(dtype):
    """`encode` under UPPER_TRIANGULAR_CHOLESKY escalates the jitter per
    matrix, as the reference does (encoding.py:548-553 recurses over the
    batch): a healthy covariance launched together with one that fails the
    first rung (a singular matrix minus 1e-9 I) is encoded, bit for bit, as it
    is alone, and so is the other."""
    import pddp_amd
    from pddp_amd.utils.encoding import encode
    enc = pddp_amd.StateEncoding.UPPER_TRIANGULAR_CHOLESKY
    g = torch.Generator().manual_seed(11)
    A = torch.randn(4, 4, generator=g, dtype=torch.float64)
    healthy = (A.t() @ A + 0.5 * torch.eye(4, dtype=torch.float64)).to(dtype)
    # v v^T is exact in both dtypes; the shift survives float32's rounding of
    # a diagonal of 0.25 ... 9 only from about 1e-6 on
    v = torch.tensor([[1.0], [-2.0], [0.5], [3.0]], dtype=torch.float64)
    shift = 1e-9 if dtype == torch.float64 else 1e-6
    sick = (v @ v.t() - shift * torch.eye(4, dtype=torch.float64)).to(dtype)
    M = torch.randn(2, 4, generator=g, dtype=torch.float64).to(dtype)
    _, info = torch.linalg.cholesky_ex(
        sick + 1e-12 * torch.eye(4, dtype=dtype), upper=True)
    assert int(info) != 0  # it does fail the first rung
    both = encode(M, C=torch.stack([healthy, sick]), encoding=enc)
    alone_h = encode(M[:1], C=healthy[None], encoding=enc)
    alone_s = encode(M[1:], C=sick[None], encoding=enc)
    assert torch.isfinite(both).all()
    assert torch.equal(both[0], alone_h[0])
    assert torch.equal(both[1], alone_s[0])
    # and unbatched, as the reference takes a single matrix
    assert torch.equal(encode(M[1], C=sick, encoding=enc), both[1])
    # the healthy row is the first rung's factor: U^T U = C + 1e-12 I
    Uh = torch.zeros(4, 4, dtype=dtype)
    iu = torch.triu_indices(4, 4)
    Uh[iu[0], iu[1]] = both[0, 4:]
    ref, _ = torch.linalg.cholesky_ex(
        healthy + 1e-12 * torch.eye(4, dtype=dtype), upper=True)
    assert torch.equal(Uh, ref)
    # the gradient through a batch with an escalated row stays finite
    C = torch.stack([healthy, sick]).requires_grad_()
    encode(M, C=C, encoding=enc).sum().backward()
    assert torch.isfinite(C.grad).all()


# --------------------------------------------------------------- GPU tests --
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32],
                                 ids=["f64", "f32"])
EACH_SHAPE = pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
# every regime at m = 2 with bounds; the other (m, bounds) in regime (a)
CASES = [("a", 2, True), ("b", 2, True), ("c", 2, True), ("d", 2, True),
         ("a", 1, True), ("a", 1, False), ("a", 2, False)]
CASE_IDS = ["%s-m%d-%s" % (r, m, "bounds" if b else "free")
            for r, m, b in CASES]


def launch(D, ang, m, c, Z, U, dtype, bounds):
    """One call of pddp_qr_cost_derivs_<dtype> as TorchProblem._cost_derivs_qr
    makes it.  Every output starts as NaN and has one guard row behind its
    last (trajectory, step).  -> (blocks in `dtype` on the CPU, guard rows)."""
    from pddp_amd import _native
    Bq, N1, n = Z.shape
    Nq = N1 - 1
    assert U.shape == (Bq, Nq, m) and n == qm.encoded_size(D)
    dev = lambda t: t.to(dtype).cuda().contiguous()
    nan = lambda *s: torch.full(s, float("nan"), dtype=dtype, device="cuda")
    out = dict(L=nan(Bq * N1 + 1), L_z=nan(Bq * N1 + 1, n),
               L_zz=nan(Bq * N1 + 1, n, n), L_u=nan(Bq * Nq + 1, m),
               L_uz=nan(Bq * Nq + 1, m, n), L_uu=nan(Bq * Nq + 1, m, m))
    keep = dict(Z=dev(Z), U=dev(U), Q=dev(c["Q"]), Q_term=dev(c["Q_term"]),
                R=dev(c["R"]), x_goal=dev(c["x_goal"]),
                u_goal=dev(c["u_goal"]))
    if bounds:
        keep.update(u_min=dev(c["u_min"]), u_max=dev(c["u_max"]))
    non = qm.non_angular(D, ang)
    assert sorted(list(ang) + non) == list(range(D))  # the kernel trusts them
    st = _native.QrCost()
    st.B, st.N, st.D, st.m = Bq, Nq, D, m
    st.n_ang, st.n_non = len(ang), len(non)
    for i, v in enumerate(ang):
        st.ang[i] = v
    for i, v in enumerate(non):
        st.non[i] = v
    for k, t in list(keep.items()) + list(out.items()):
        setattr(st, k, _native.ptr(t))
    _native.call("pddp_qr_cost_derivs", dtype, ctypes.byref(st),
                 _native.stream_handle(torch.device("cuda")))
    torch.cuda.synchronize()
    lead = dict(L=(Bq, N1), L_z=(Bq, N1), L_zz=(Bq, N1), L_u=(Bq, Nq),
                L_uz=(Bq, Nq), L_uu=(Bq, Nq))
    res = {k: v[:-1].reshape(*lead[k], *v.shape[1:]).cpu()
           for k, v in out.items()}
    guards = {k: v[-1].cpu() for k, v in out.items()}
    return res, guards


def magnitude(D, ang, m, c, Z, Uc):
    """[B, N+1]: the sum of the absolute values of the terms L0 adds up - what
    the rounding error of the value scales with (a skew Q cancels in L0)."""
    non = qm.non_angular(D, ang)
    Ma, Ca = qm.moments(Z, D, list(ang), non)
    S = []
    for Qs, sl in ((c["Q"], slice(0, -1)), (c["Q_term"], slice(-1, None))):
        dx = (Ma[:, sl] - c["x_goal"]).abs()
        S.append(((dx @ Qs.abs()) * dx).sum(-1) +
                 (Ca[:, sl].abs() * Qs.abs().t()).sum((-2, -1)))
    du = (Uc - c["u_goal"]).abs()
    S[0] = S[0] + ((du @ c["R"].abs()) * du).sum(-1)
    return torch.cat(S, 1)


def predicted_rungs(D, ang, Z, np_dtype):
    """[B, N+1]: the model's own Cholesky on the augmented covariance
    evaluated in `np_dtype` with the difference of exponentials."""
    tdt = torch.float32 if np_dtype == np.float32 else torch.float64
    _, Ca = qm.moments(Z.to(tdt), D, list(ang), qm.non_angular(D, ang),
                       exact=False)
    flat = Ca.reshape(-1, *Ca.shape[-2:]).numpy()
    r = [qm.rung(a, np_dtype) for a in flat]
    assert None not in r
    return torch.tensor(r, dtype=torch.float64).reshape(Ca.shape[:-2])


def hold_to_model(out, mo, D, ang, m, c, Z, Uc, dtype, first_rung, tag):
    """The rule of test_kernel_vs_float64_model for one set of blocks `out`
    (in `dtype`, on the CPU) against the model's `mo` at the same inputs;
    `first_rung`: the f32 value must sit on rung 1e-12."""
    for k in BLOCKS:
        assert torch.isfinite(out[k]).all(), k
    assert torch.equal(out["L_zz"], out["L_zz"].transpose(-1, -2))
    assert torch.equal(out["L_uu"], out["L_uu"].transpose(-1, -2))
    out = {k: v.double() for k, v in out.items()}
    lad = qm.ladder()
    if dtype == torch.float64:
        assert (predicted_rungs(D, ang, Z, np.float64) == lad[0]).all()
        S = magnitude(D, ang, m, c, Z, Uc)
        margin = 64 * EPS64 * S / mo["trQ"]
        measured = (out["L"] - mo["L0"]) / mo["trQ"]
        print("QRCOST", *tag, "rung", float(measured.min()),
              float(measured.max()), "margin", float(margin.max()))
        assert float(margin.max()) < 0.9e-12
        assert ((measured - lad[0]).abs() <= margin).all(), measured
        for k in BLOCKS[1:]:
            e = rel(out[k], mo[k])
            print("QRCOST", *tag, k, e)
            assert e <= 1e-10, (k, e)
        assert rel(out["L"], mo["L0"] + lad[0] * mo["trQ"]) <= 1e-10
        return
    ref = torch_path(stub_cost(D, ang, c, m), Z, Uc, torch.float32)
    rungs = lad[:1] if first_rung else [r for r in lad if r <= 1.0001e-4]
    ek, chosen = value_error(out["L"], mo, rungs)
    et, _ = value_error(ref["L"], mo, lad)
    bar = max(8 * et, 16 * EPS32)
    # the lowest rung each entry is consistent with, as far as L resolves it
    fits = torch.stack([(out["L"] - mo["L0"] - r * mo["trQ"]).abs() <=
                        bar * mo["L0"].abs().max() for r in lad], -1)
    lowest = torch.tensor(lad)[fits.double().argmax(-1)]
    pred = predicted_rungs(D, ang, Z, np.float32)
    print("QRCOST", *tag, "L", ek, et, "rung: lowest consistent",
          float(lowest.max()), "best fit", float(chosen.max()),
          "model f32 Cholesky", float(pred.max()))
    assert ek <= bar, ("L", ek, et)
    for k in BLOCKS[1:]:
        ek, et = rel(out[k], mo[k]), rel(ref[k], mo[k])
        print("QRCOST", *tag, k, ek, et)
        assert ek <= max(8 * et, 16 * EPS32), (k, ek, et)


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("regime,m,bounds", CASES, ids=CASE_IDS)
@EACH_SHAPE
def test_kernel_vs_float64_model(shape, regime, m, bounds, dtype):
    """One launch (B = 3, N = 4: 15 workgroups) against the model at the
    run's inputs.  Every entry that exists is written and finite, the guard
    rows are untouched, L_zz and L_uu are exactly symmetric.  f64: blocks to
    1e-10 of the block's largest model entry, and the value pins the rung:
    (L - L0) / tr(Q) is 1e-12 to within 64 eps64 x the value's term sum, a
    margin the test checks to be below 0.9e-12 (so neither no jitter nor the
    next rung would pass), and the model's float64 Cholesky agrees.  f32:
    per block 8 x the error of the package's torch float32 autograd path
    (run here on the CPU on the same inputs) against the same model, at least
    16 eps32; L against L0 + rung tr(Q) with the best rung of ladder() up to
    1e-4 (entry errors of a few eps32 perturb Ca by at most about 8 NA eps32
    = 4e-6 in the 2-norm: rung 1e-5, and one more for the factorisation's own
    rounding); in regimes (a) and (c) - lambda_min / lambda_max >= 1e-5, and a
    covariance that is exactly zero - the rung is 1e-12."""
    D, ang = shape
    c, Z, U = case_inputs(D, ang, m, regime, dtype)
    Uc = clamped(c, U, bounds)
    mo = model_blocks(D, ang, m, regime, dtype, bounds)
    out, guards = launch(D, ang, m, c, Z, U, dtype, bounds)
    for k in BLOCKS:
        assert torch.isnan(guards[k]).all(), k
    tag = (str(dtype)[-3:], SHAPE_IDS[SHAPES.index(shape)], m, bounds, regime)
    hold_to_model(out, mo, D, ang, m, c, Z, Uc, dtype, regime in "ac", tag)


def _sick_rows(D, ang, count):
    """`count` regime-(b) states whose augmented covariance, evaluated in
    float32, fails the first rung (the model's float32 Cholesky says so)."""
    pool = states(D, ang, "b", 96, 77).float().double()
    bad = predicted_rungs(D, ang, pool, np.float32) > qm.ladder()[0]
    assert int(bad.sum()) >= count, int(bad.sum())
    return pool[bad][:count]


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("shape", [(2, (0,)), (4, (0, 3)), (6, (1, 2))],
                         ids=["D2-ang0", "D4-ang03", "D6-ang12"])
def test_kernel_is_batch_invariant(shape, dtype):
    """A regime-(a) trajectory and a regime-(b) one whose float32 augmented
    covariance is indefinite at every step (confirmed with the model's float32
    Cholesky on the CPU), launched together and each alone: the same bits.
    The jitter ladder of one trajectory leaves the other alone."""
    D, ang = shape
    m = 2
    c = constants(D, ang, m)
    healthy = states(D, ang, "a", N + 1, 5).float().double()
    assert (predicted_rungs(D, ang, healthy, np.float32) == 1e-12).all()
    Z = torch.stack([healthy, _sick_rows(D, ang, N + 1)])
    U = actions(m, 3)[:2].float().double()
    both, _ = launch(D, ang, m, c, Z, U, dtype, True)
    for b in range(2):
        alone, _ = launch(D, ang, m, c, Z[b:b + 1], U[b:b + 1], dtype, True)
        for k in BLOCKS:
            assert torch.isfinite(alone[k]).all()
            assert torch.equal(both[k][b], alone[k][0]), (b, k)


@pytest.mark.gpu
@DTYPES
@EACH_SHAPE
def test_terminal_step_reads_q_term_and_no_action_term(shape, dtype):
    """With Q_term = 3 Q^T the step-N outputs are the model's terminal form
    (test_kernel_vs_float64_model holds them to it); here: zeroing R, or
    swapping Q for another matrix, changes no bit at step N, and swapping
    Q_term changes none before it."""
    D, ang = shape
    m = 2
    c, Z, U = case_inputs(D, ang, m, "a", dtype)
    base, _ = launch(D, ang, m, c, Z, U, dtype, True)
    other = dict(c, R=torch.zeros_like(c["R"]), Q=c["Q"].t() * 0.5)
    alt, _ = launch(D, ang, m, other, Z, U, dtype, True)
    for k in ("L", "L_z", "L_zz"):
        assert torch.equal(base[k][:, N], alt[k][:, N]), k
        assert not torch.equal(base[k][:, :N], alt[k][:, :N]), k
    alt, _ = launch(D, ang, m, dict(c, Q_term=c["Q"]), Z, U, dtype, True)
    for k in BLOCKS:
        assert torch.equal(base[k][:, :N], alt[k][:, :N]), k
    assert not torch.equal(base["L_zz"][:, N], alt["L_zz"][:, N])


@pytest.mark.gpu
@DTYPES
@EACH_SHAPE
def test_clamp_equals_passing_the_clamped_action(shape, dtype):
    """With bounds, every output equals, bit for bit, that of a launch that
    is handed the clamped actions and NULL bounds: the derivatives are taken
    at the clamped action, not through the clamp (ilqr.py:461-462)."""
    D, ang = shape
    m = 2
    c, Z, U = case_inputs(D, ang, m, "a", dtype)
    Uc = clamped(c, U, True)
    assert int((Uc != U).sum()) == B  # one clamped action per trajectory
    a, _ = launch(D, ang, m, c, Z, U, dtype, True)
    b, _ = launch(D, ang, m, c, Z, Uc, dtype, False)
    for k in BLOCKS:
        assert torch.equal(a[k], b[k]), k
    free, _ = launch(D, ang, m, c, Z, U, dtype, False)
    assert not torch.equal(a["L_u"], free["L_u"])


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("name", ["cartpole", "pendulum", "double_cartpole"])
def test_records_and_cost_kernel_share_the_cost(name, dtype):
    """The two users of csrc/gauss_cost_body.inc on one nominal: the cost
    blocks of `pddp_derivs_*` under the DEFAULT encoding (ILQRSolver's
    records, B = 2, N = 2, the shipped cost, bounded) and the blocks of
    `pddp_qr_cost_derivs_*` on the same Z, U, Q, Q_term, R and goals, each
    held to the float64 model by the rule and the bars of
    test_kernel_vs_float64_model.  The nominal is a rollout from regime-(a)
    states, whose factors the dynamics turn into diagonals of the same size:
    rung 1e-12 in both dtypes."""
    import pddp_amd
    from pddp_amd.controllers.solver import ILQRSolver
    cost, mc = _shipped(name)
    D, m = mc.state_size, mc.action_size
    ang = tuple(int(i) for i in mc.angular_indices)
    NA, n = D + len(ang), qm.encoded_size(D)
    Bq, Nq = 2, 2
    r = (lambda t: t.float().double()) if dtype == torch.float32 \
        else (lambda t: t)
    f64 = lambda t, k: r(torch.as_tensor(t).detach().double().expand(
        *k).clone())
    c = dict(Q=f64(cost.Q, (NA, NA)), Q_term=f64(cost.Q_term, (NA, NA)),
             R=f64(cost.R, (m, m)), x_goal=f64(cost.x_goal, (NA,)),
             u_goal=f64(cost.u_goal, (m,)),
             u_min=torch.full((m,), -0.25, dtype=torch.float64),
             u_max=torch.full((m,), 0.25, dtype=torch.float64))
    z0 = r(states(D, ang, "a", Bq, 21))
    g = torch.Generator().manual_seed(22)
    U = r(torch.rand(Bq, Nq, m, generator=g, dtype=torch.float64) - 0.5)
    prob = mc(0.05).native_problem(pddp_amd.StateEncoding.DEFAULT, cost)
    s = ILQRSolver(prob, Bq, Nq, dtype, "cuda:0", c["u_min"], c["u_max"])
    s.set_nominal(z0.cuda(), U.cuda())
    s.derivs()
    torch.cuda.synchronize()
    Z = s.Z.cpu().double()
    assert torch.equal(Z[:, 0], z0)
    Uc = clamped(c, U, True)
    assert bool((Uc != U).any())
    _, _, L_z, L_u, L_zz, L_uz, L_uu = s.record_views()
    records = {k: v.cpu().clone() for k, v in dict(
        L=s.L, L_z=L_z, L_u=L_u, L_zz=L_zz, L_uz=L_uz, L_uu=L_uu).items()}
    kernel, guards = launch(D, ang, m, c, Z, U, dtype, True)
    for k in BLOCKS:
        assert torch.isnan(guards[k]).all(), k
    mo = model_on(D, ang, m, c, Z, Uc)
    for who, out in (("records", records), ("qr_cost", kernel)):
        assert all(out[k].shape == mo[k].shape for k in BLOCKS[1:]), who
        hold_to_model(out, mo, D, ang, m, c, Z, Uc, dtype, True,
                      (str(dtype)[-3:], name, who))
