"""The GP step's chunked form (csrc/gp_step_chunked.hip, gp_step_body.hpp `CH`):
training sets larger than one workgroup's LDS.  The resident form keeps every
per-training-point table of a row in LDS and stops where 160 KB stops; the
chunked form keeps a chunk of C points and serves any size.  Checker: the fp64
torch module and autograd through it, one row and one output at a time (the
module builds E^2 M^2 numbers per row: at M = 1000 a replica per output, as
tests/test_gp.py `_torch_step` makes them, would be tens of GB)."""
import contextlib
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pddp_amd  # noqa: E402,F401
from pddp_amd import GaussianVariable, StateEncoding  # noqa: E402
from pddp_amd.models.gp import gp_dynamics_model_factory  # noqa: E402
from gp_util import max_rel, system_model, system_rows  # noqa: E402

LDS = 160 * 1024


@contextlib.contextmanager
def _forced(chunk=0, rows=0):
    """The chunked form with chunks of `chunk` points / `rows` rows a launch
    (0: automatic) for the calls inside; the previous setting comes back."""
    from pddp_amd import _native
    lib = _native.lib()
    pc = lib.pddp_gp_step_force_chunk(chunk)
    pr = lib.pddp_gp_step_force_rows_per_launch(rows)
    try:
        yield
    finally:
        lib.pddp_gp_step_force_chunk(pc)
        lib.pddp_gp_step_force_rows_per_launch(pr)


def _lean_step(model, z, u, encoding, jacobian):
    """The torch module with the kernel switched off, a row at a time;
    Jacobians by autograd, one output at a time through the row's one graph."""
    model.use_native = False
    try:
        R, n = z.shape
        outs, Js = [], []
        for r in range(R):
            x = torch.cat([z[r], u[r]]).detach().clone()
            x.requires_grad_(bool(jacobian))
            with torch.set_grad_enabled(bool(jacobian)):
                zn = model(x[:n].unsqueeze(0), x[n:].unsqueeze(0), 0,
                           encoding)[0]
            outs.append(zn.detach().clone())
            if jacobian:
                Js.append(torch.stack([
                    torch.autograd.grad(zn[k], x, retain_graph=k + 1 < n)[0]
                    for k in range(n)]))
            del zn, x
        out = torch.stack(outs)
        if not jacobian:
            return out
        J = torch.stack(Js)
        return out, J[:, :, :n].contiguous(), J[:, :, n:].contiguous()
    finally:
        model.use_native = True


def _double(model):
    m64 = copy.deepcopy(model).double()
    m64._native_cache = {}
    return m64


def _permuted(model, seed=11):
    """The same GPs with the training points in another order: the same
    mathematics, every sum over the points in another order."""
    p = copy.deepcopy(model)
    M = p.Xt.shape[0]
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(seed)) \
        .to(p.Xt.device)
    p.Xt = p.Xt[perm].contiguous()
    p.beta = p.beta[:, perm].contiguous()
    p.Kinv = p.Kinv[:, perm][:, :, perm].contiguous()
    p._native_cache = {}
    return p


def _check(got, exact, torch_same_dtype, tols, label, noise=None):
    """Kernel results against the fp64 module.  f64 (`torch_same_dtype` None):
    the fixed bars of tests/test_gp.py; f32: no further than 4 x the float
    module's own distance, or the fixed bars.  `noise`: the fp64 module's own
    distances under a permutation of the training points; the bar is never
    below 4 x that."""
    for k, (g, e, tol) in enumerate(zip(got, exact, tols)):
        bar = tol
        if torch_same_dtype is not None:
            bar = max(bar, 4.0 * max_rel(torch_same_dtype[k].double(), e))
        if noise is not None:
            bar = max(bar, 4.0 * noise[k])
        d = max_rel(g.double(), e)
        print("%s [%d]: kernel vs fp64 module %.3e, bar %.3e%s" % (
            label, k, d, bar,
            "" if noise is None else ", module vs permuted module %.3e"
            % noise[k]))
        assert d < bar, (label, k, d, bar)


# ---- CPU: the host queries ---------------------------------------------------
def test_gp_step_form_and_chunk_queries():
    """pddp_gp_step_form is 0 (resident) exactly where pddp_gp_step_lds_bytes
    fits 160 KB - at the boundaries tests/test_gp.py names - and 1 (chunked)
    beyond; -1 for a pair that is not built; the chunked layout at the chunk
    the launcher would use fits 160 KB and holds at least one lane tile."""
    from pddp_amd import _native
    lib = _native.lib()
    assert lib.pddp_gp_step_force_chunk(0) == 0
    assert lib.pddp_gp_step_force_rows_per_launch(0) == 0
    args = lambda M, jac, es: (6, 9, M, 28, jac, es)
    for last, first, jac, es in ((890, 894, 1, 4), (208, 212, 1, 8),
                                 (1278, 1282, 0, 4), (596, 600, 0, 8)):
        assert lib.pddp_gp_step_lds_bytes(*args(last, jac, es)) <= LDS
        assert lib.pddp_gp_step_lds_bytes(*args(first, jac, es)) > LDS
        assert lib.pddp_gp_step_form(*args(last, jac, es)) == 0
        assert lib.pddp_gp_step_chunk(*args(last, jac, es)) == last
        assert lib.pddp_gp_step_form(*args(first, jac, es)) == 1
    for M in range(1, 1400, 7):  # resident exactly where it fits
        for jac in (0, 1):
            for es in (4, 8):
                fits = lib.pddp_gp_step_lds_bytes(*args(M, jac, es)) <= LDS
                assert lib.pddp_gp_step_form(*args(M, jac, es)) == \
                    (0 if fits else 1)
    assert lib.pddp_gp_step_form(5, 9, 100, 28, 1, 4) == -1
    assert lib.pddp_gp_step_chunk(5, 9, 100, 28, 1, 4) == -1
    assert lib.pddp_gp_step_chunked_lds_bytes(5, 9, 64, 28, 1, 4) == -1
    for M in (895, 1000, 4000):
        for jac in (0, 1):
            for es in (4, 8):
                form = lib.pddp_gp_step_form(*args(M, jac, es))
                C = lib.pddp_gp_step_chunk(*args(M, jac, es))
                if form == 0:
                    assert C == M
                    continue
                assert form == 1 and 64 <= C and C % 2 == 0
                need = lib.pddp_gp_step_chunked_lds_bytes(6, 9, C, 28, jac, es)
                assert 0 < need <= LDS, (M, jac, es, C, need)
    # the forced chunk: reported by the queries, bounded by M, and given back
    assert lib.pddp_gp_step_force_chunk(66) == 0
    try:
        assert lib.pddp_gp_step_form(*args(300, 1, 4)) == 1
        assert lib.pddp_gp_step_chunk(*args(300, 1, 4)) == 66
        assert lib.pddp_gp_step_chunk(*args(5, 1, 4)) == 8
        assert lib.pddp_gp_step_chunk(*args(1000, 1, 8)) == 66
    finally:
        assert lib.pddp_gp_step_force_chunk(0) == 66
    assert lib.pddp_gp_step_force_chunk(-3) == 0
    assert lib.pddp_gp_step_force_chunk(0) == 0
    assert lib.pddp_gp_step_form(*args(300, 1, 4)) == 0


# ---- GPU ----------------------------------------------------------------------
_BOTH = [(M, torch.float64) for M in (2, 5, 63, 64, 65, 127, 129, 208)] + \
    [(M, torch.float32) for M in (66, 300, 890)]


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["cartpole", "double_cartpole"])
@pytest.mark.parametrize("M,dtype", _BOTH)
def test_gp_chunked_equals_resident_where_both_exist(system, M, dtype):
    """The chunked form forced with C in {64, 66, 128} at sizes the resident
    form covers too (M below, at and around C, odd M, M not a multiple of C):
    step, Jacobian and the masked entry of BOTH forms against the fp64 torch
    module with the resident form's bars (f64: 1e-10 / 1e-9; f32: 4 x the float
    module's own distance or 2e-5 / 5e-4), DEFAULT and variance-only
    encoding."""
    f64 = dtype == torch.float64
    tols = (1e-10, 1e-9, 1e-9) if f64 else (2e-5, 5e-4, 5e-4)
    model, _ = system_model(system, M, dtype, seed=M)
    m64 = model if f64 else _double(model)
    for enc in (StateEncoding.DEFAULT, StateEncoding.VARIANCE_ONLY):
        z, u = system_rows(system, 3, enc, dtype, seed=M + 1)
        assert model.native_ok(z, enc, jacobian=True)
        assert model.native_form(z, enc, jacobian=True) == "resident"
        exact = _lean_step(m64, z.double(), u.double(), enc, True)
        same = None if f64 else _lean_step(model, z, u, enc, True)
        res = model.native_step(z, u, enc, jacobian=True)
        _check(res, exact, same, tols, "resident M=%d enc=%d" % (M, enc))
        for C in (64, 66, 128):
            with _forced(chunk=C):
                assert model.native_form(z, enc, jacobian=True) == "chunked"
                assert model.native_form(z, enc) == "chunked"
                assert model.native_ok(z, enc, jacobian=True)
                got = model.native_step(z, u, enc, jacobian=True)
                plain = model.native_step(z, u, enc)
                # the masked entry: row 1 skipped, its records left alone
                Fz = torch.full_like(got[1], -7.0)
                Fu = torch.full_like(got[2], -7.0)
                mask = torch.tensor([1, 0, 1], dtype=torch.uint8,
                                    device=z.device)
                om, _, _ = model.native_step(z, u, enc, jacobian=True, Fz=Fz,
                                             Fu=Fu, row_mask=mask)
            label = "chunked C=%d M=%d enc=%d %s" % (C, M, int(enc), system)
            _check(got, exact, same, tols, label)
            _check((plain,), exact[:1], None if f64 else same[:1], tols[:1],
                   label + " step")
            for r in (0, 2):
                assert torch.equal(om[r], got[0][r])
                assert torch.equal(Fz[r], got[1][r])
                assert torch.equal(Fu[r], got[2][r])
            assert bool((Fz[1] == -7.0).all()) and bool((Fu[1] == -7.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("M,dtype,jacobian", [
    (891, torch.float32, True), (1000, torch.float32, True),
    (209, torch.float64, True), (300, torch.float64, True),
    (1000, torch.float64, True), (597, torch.float64, False),
    (1000, torch.float64, False), (1300, torch.float32, False)])
def test_gp_step_at_sizes_beyond_the_resident_form(M, dtype, jacobian):
    """Automatic dispatch at the sizes the resident form does not cover: double
    cartpole, DEFAULT encoding, 2 rows; `native_form` says "chunked",
    `native_ok` False; step (and Jacobian) against the fp64 module + autograd.
    Bars: those of the resident form (f64 1e-10 / 1e-9; f32 4 x the float
    module's distance or 2e-5 / 5e-4), and never below 4 x the checker's own
    noise: the fp64 module against itself with the training points permuted
    (the same sums in another order; measured here, independent of the
    kernel).  Without the chunked form `native_step` raises NativeError.

    Measured on the MI355X (relative to the largest entry; step, F_z, F_u;
    kernel vs fp64 module | fp64 module vs permuted fp64 module):
      f32 jac M = 891:  4.1e-7 1.1e-6 2.8e-6 | 6.5e-16 1.5e-15 7.5e-16
      f32 jac M = 1000: 4.9e-7 1.6e-6 2.3e-6 | 8.3e-16 1.2e-15 7.8e-16
      f64 jac M = 209:  1.0e-16 4.2e-16 9.0e-16 | 1.2e-16 4.0e-16 3.7e-16
      f64 jac M = 300:  5.5e-16 1.1e-15 3.1e-15 | 1.6e-16 6.7e-16 4.0e-16
      f64 jac M = 1000: 1.1e-15 1.9e-15 7.3e-15 | 3.7e-16 1.1e-15 5.5e-16
      f64 step M = 597: 1.5e-15 | 3.6e-16;  M = 1000: 1.0e-15 | 3.7e-16
      f32 step M = 1300: 7.7e-7 | 1.4e-15
    The fixed bars decide everywhere."""
    enc = StateEncoding.DEFAULT
    f64 = dtype == torch.float64
    model, _ = system_model("double_cartpole", M, dtype, seed=M)
    z, u = system_rows("double_cartpole", 2, enc, dtype, seed=M + 1)
    assert model.native_form(z, enc, jacobian=jacobian) == "chunked"
    assert not model.native_ok(z, enc, jacobian=jacobian)
    m64 = model if f64 else _double(model)
    wrap = (lambda t: t) if jacobian else (lambda t: (t,))
    exact = wrap(_lean_step(m64, z.double(), u.double(), enc, jacobian))
    perm = wrap(_lean_step(_permuted(m64), z.double(), u.double(), enc,
                           jacobian))
    noise = [max_rel(p, e) for p, e in zip(perm, exact)]
    del perm
    same = None if f64 else wrap(_lean_step(model, z, u, enc, jacobian))
    got = wrap(model.native_step(z, u, enc, jacobian=jacobian))
    again = wrap(model.native_step(z, u, enc, jacobian=jacobian))
    tols = (1e-10, 1e-9, 1e-9) if f64 else (2e-5, 5e-4, 5e-4)
    _check(got, exact, same, tols, "M=%d %s jac=%s" % (M, dtype, jacobian),
           noise=noise)
    for a, b in zip(got, again):  # deterministic
        assert torch.equal(a, b)
    if not jacobian:
        with torch.no_grad():  # `forward` itself goes through the kernel
            assert torch.equal(model(z, u, 0, enc), got[0])


def _rollout_pair(system, dtype, Md, B=5, N=4):
    """pddp_gp_rollout_* and the per-step line search (`_line_search_gp_torch`:
    the step kernel per time step, the costs in torch) on one problem, as
    tests/test_gp.py test_gp_rollout_kernel_vs_per_step_line_search - with
    smooth targets (those of gp_util.py `system_model`) in place of that
    test's pure-noise ones.  Reason, measured on the MI355X against the fp64
    per-step form on the same gains: noise targets at 66 points of the
    pendulum give weights of |beta| = 824, |Kinv| = 6.5e3, and EVERY float form
    - the per-step reference included - is 5.7 to 8.7 x the 2e-4 bar from the
    fp64 result (24 points, that test's size: 0.01 x); a float reference that
    far from the truth checks nothing.  Smooth targets (|beta| = 10): 0.02 x.
    For float the reference's own distance from the fp64 per-step form is
    measured here and must be within a quarter of the bar."""
    import pddp_amd.examples as ex
    from pddp_amd.controllers.ilqr import fit_alphas
    from pddp_amd.controllers.plugin import TorchProblem
    from pddp_amd.controllers.solver import ILQRSolver
    mod = getattr(ex, system)
    cost_cls = [getattr(mod, k) for k in dir(mod) if k.endswith("Cost") and
                k not in ("AugmentedQRCost", "QRCost")][0]
    enc = StateEncoding.DEFAULT
    MC = [getattr(mod, k) for k in dir(mod) if k.endswith("DynamicsModel") and
          k != "DynamicsModel"][0]
    E, m = MC.state_size, 1
    g = torch.Generator().manual_seed(2)
    Xd = torch.randn(Md, E, generator=g, dtype=torch.float64)
    Ud = torch.randn(Md, m, generator=g, dtype=torch.float64)
    dXd = 0.3 * torch.sin(Xd @ torch.randn(E, E, generator=g,
                                           dtype=torch.float64)) + 0.2 * Ud
    model = gp_dynamics_model_factory(E, m, MC.angular_indices,
                                      MC.non_angular_indices)().double().cuda()
    model.fit(Xd.cuda(), Ud.cuda(), dXd.cuda())
    model = model.to(dtype).eval()
    n = E + E * (E + 1) // 2
    z0 = torch.stack([GaussianVariable(
        0.3 * torch.randn(E, generator=g, dtype=torch.float64),
        var=1e-2 * torch.ones(E, dtype=torch.float64)).encode(enc)
        for _ in range(B)]).to(dtype).cuda()
    U0 = (0.3 * torch.randn(B, N, m, generator=g)).to(dtype).cuda()
    bound = torch.tensor([2.0], dtype=dtype)
    # two step sizes: the torch side is the slow one
    alphas = fit_alphas(dtype, "cuda")[:2].contiguous()
    got = []
    for roll in (True, False):
        plugin = TorchProblem(model, cost_cls().to(dtype).cuda(), enc, {}, {})
        plugin.use_gp_rollout = roll
        s = ILQRSolver(None, B, N, dtype, "cuda", -bound, bound, alphas,
                       plugin=plugin, n=n, m=m)
        s.set_nominal(z0, U0)
        s.derivs()
        s.mu.fill_(1.0)
        s.backward(active=s.active)
        assert plugin._gp_line_search_ok(s)
        s.active[2] = 0
        s.bwd_status[4] = 3
        s.Zc.fill_(-7.0)
        s.Jc.fill_(-7.0)
        s.line_search(active=s.active)
        got.append((s.Zc.clone(), s.Uc.clone(), s.Jc.clone()))
    live = torch.ones(B, dtype=torch.bool)
    live[2] = live[4] = False
    tol = 1e-9 if dtype == torch.float64 else 2e-4
    if dtype == torch.float32:
        # the float reference against the fp64 per-step form of the same
        # (float) model, nominal and gains
        m64 = copy.deepcopy(model).double().eval()
        m64._native_cache = {}
        p64 = TorchProblem(m64, cost_cls().double().cuda(), enc, {}, {})
        p64.use_gp_rollout = False
        s64 = ILQRSolver(None, B, N, torch.float64, "cuda", -bound.double(),
                         bound.double(), alphas.double(), plugin=p64, n=n, m=m)
        s64.set_nominal(z0.double(), U0.double())
        s64.Z.copy_(s.Z.double())
        s64.U.copy_(s.U.double())
        s64.gains.copy_(s.gains.double())
        s64.active.copy_(s.active)
        s64.bwd_status.copy_(s.bwd_status)
        s64.line_search(active=s64.active)
        own = max(float(((a[live].double() - b[live]).abs() /
                         (tol + tol * b[live].abs())).max())
                  for a, b in zip(got[1], (s64.Zc, s64.Uc, s64.Jc)))
        print("%s M=%d: float per-step reference vs fp64 per-step form, "
              "distance / bar %.3f" % (system, Md, own))
        assert own <= 0.25, own
    # distance in units of the bar: |a - b| / (tol + tol |b|), as allclose
    worst = max(float(((a[live] - b[live]).abs() /
                       (tol + tol * b[live].abs())).max())
                for a, b in zip(*got))
    untouched = bool((got[0][0][~live] == -7.0).all()) and \
        bool((got[0][2][~live] == -7.0).all())   # skipped rows
    return model, z0, worst, untouched


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["pendulum", "double_cartpole"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gp_rollout_chunked_vs_per_step_line_search(system, dtype):
    """pddp_gp_rollout_* forced to the chunked form at M = 66 (C = 64: a whole
    chunk and a chunk of two), in slices of 3 rows a launch: candidates,
    actions and costs against the per-step torch line search (1e-9 / 2e-4),
    masked trajectories and a failed sweep included.

    Measured on the MI355X, worst |a - b| / (tol + tol |b|) (1 = the bar),
    resident | chunked: pendulum f64 0.000 | 0.000, f32 0.000 | 0.003; double
    cartpole f64 0.000 | 0.000, f32 0.001 | 0.001; the float reference from
    the fp64 per-step form: pendulum 0.009 / 0.015, double cartpole 0.003."""
    # (for the record: the resident form on the same problem)
    _, _, resident, _ = _rollout_pair(system, dtype, 66)
    with _forced(chunk=64, rows=3):
        model, z0, worst, untouched = _rollout_pair(system, dtype, 66)
        assert model.native_form(z0, StateEncoding.DEFAULT) == "chunked"
    print("%s %s M=66: distance / bar - resident %.3f, chunked %.3f" % (
        system, dtype, resident, worst))
    assert untouched
    assert worst <= 1.0, worst


@pytest.mark.gpu
def test_gp_rollout_f64_beyond_the_resident_form():
    """pddp_gp_rollout_f64 for the double cartpole at M = 700: the resident
    form of the rollout stops at 596 points; automatic dispatch."""
    model, z0, worst, untouched = _rollout_pair("double_cartpole",
                                                torch.float64, 700, B=5, N=3)
    assert model.native_form(z0, StateEncoding.DEFAULT) == "chunked"
    assert not model.native_ok(z0, StateEncoding.DEFAULT)
    print("double_cartpole f64 M=700: distance / bar %.3f" % worst)
    assert untouched and worst <= 1.0, worst


@pytest.mark.gpu
def test_gp_controller_round_on_the_chunked_form_equals_autograd():
    """A TorchProblem + ILQRSolver round in f64 with a cartpole GP of M = 800
    (the resident Jacobian form of the cartpole stops at 772): the records
    come from the kernel (`last_derivs_path["dynamics"] == "hip"`), and
    records, gains and the accepted nominal equal those of the autograd path to
    1e-7 / 1e-8."""
    from pddp_amd.controllers.ilqr import fit_alphas
    from pddp_amd.controllers.plugin import TorchProblem
    from pddp_amd.controllers.solver import ILQRSolver
    from pddp_amd.examples.cartpole import CartpoleCost, CartpoleDynamicsModel
    CM = CartpoleDynamicsModel
    g = torch.Generator().manual_seed(7)
    true = CM(0.1).double()
    Md = 800
    X = torch.cat([torch.randn(Md, 2, generator=g, dtype=torch.float64),
                   3.0 + 0.8 * torch.randn(Md, 1, generator=g,
                                           dtype=torch.float64),
                   torch.randn(Md, 1, generator=g, dtype=torch.float64)], -1)
    U = 3.0 * torch.randn(Md, 1, generator=g, dtype=torch.float64)
    with torch.no_grad():
        dX = true(X, U, 0, StateEncoding.IGNORE_UNCERTAINTY) - X
    model = gp_dynamics_model_factory(4, 1, CM.angular_indices,
                                      CM.non_angular_indices)().double().cuda()
    model.fit(X.cuda(), U.cuda(), dX.cuda())
    model.eval()
    enc = StateEncoding.DEFAULT
    B, N, n, m = 4, 8, 14, 1
    z0 = torch.stack([GaussianVariable(
        torch.tensor([0.0, 0.0, 3.0, 0.0], dtype=torch.float64) +
        0.05 * torch.randn(4, generator=g, dtype=torch.float64),
        var=1e-2 * torch.ones(4, dtype=torch.float64)).encode(enc)
        for _ in range(B)]).cuda()
    U0 = (0.3 * torch.randn(B, N, m, generator=g, dtype=torch.float64)).cuda()
    assert model.native_form(z0, enc, jacobian=True) == "chunked"
    assert not model.native_ok(z0, enc, jacobian=True)
    sol = []
    for native in (True, False):
        plugin = TorchProblem(model, CartpoleCost().double().cuda(), enc, {},
                              {})
        plugin.use_native_gp = native
        model.use_native = native
        try:
            s = ILQRSolver(None, B, N, torch.float64, "cuda",
                           torch.tensor([-10.0], dtype=torch.float64),
                           torch.tensor([10.0], dtype=torch.float64),
                           fit_alphas(torch.float64, "cuda"), plugin=plugin,
                           n=n, m=m)
            s.set_nominal(z0, U0)
            s.round(5e-6, 1e10, 1 << 30)
            assert plugin.last_derivs_path["dynamics"] == \
                ("hip" if native else "autograd")
            sol.append((s.rec.clone(), s.gains.clone(), s.Z.clone(),
                        s.U.clone(), s.J_opt.clone()))
        finally:
            model.use_native = True
        del s, plugin
        torch.cuda.empty_cache()
    for a, b in zip(*sol):
        assert torch.allclose(a, b, rtol=1e-7, atol=1e-8), \
            float((a - b).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gp_chunked_launch_split_is_bit_equal_to_one_launch(dtype):
    """The rows of a chunked call in consecutive launches (3 rows a launch: 11
    rows = four launches, the last of two rows) give bit for bit what one
    launch gives - step, Jacobian and the masked entry - and two calls on the
    same inputs are bit-equal."""
    enc = StateEncoding.DEFAULT
    model, _ = system_model("double_cartpole", 150, dtype, seed=5)
    z, u = system_rows("double_cartpole", 11, enc, dtype, seed=6)
    mask = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8, device=z.device)

    def run():
        got = model.native_step(z, u, enc, jacobian=True)
        plain = model.native_step(z, u, enc)
        Fz = torch.full_like(got[1], -7.0)
        Fu = torch.full_like(got[2], -7.0)
        om, _, _ = model.native_step(z, u, enc, jacobian=True, Fz=Fz, Fu=Fu,
                                     row_mask=mask, rows_per_mask=2)
        keep = mask.bool().repeat_interleave(2)[:11]
        return got + (plain, om[keep], Fz, Fu)

    with _forced(chunk=64):
        one = run()
        two = run()
    with _forced(chunk=64, rows=3):
        split = run()
    for a, b, c in zip(one, two, split):
        assert torch.equal(a, b)
        assert torch.equal(a, c)
    assert bool((one[5][2:4] == -7.0).all()) and bool((one[5][8:10] == -7.0).all())


@pytest.mark.gpu
def test_gp_chunked_rounds_replayed_as_hipgraphs_equal_eager_rounds():
    """`ILQRSolver.fit(graph=True)` with the GP plugin on the chunked form, the
    rows in several launches: the captured rounds leave the state the eager
    rounds leave (tests/test_gp.py
    test_gp_rounds_replayed_as_hipgraphs_equal_eager_rounds)."""
    from pddp_amd.controllers.ilqr import fit_alphas
    from pddp_amd.controllers.plugin import TorchProblem
    from pddp_amd.controllers.solver import ILQRSolver
    from pddp_amd.examples.cartpole import CartpoleCost, CartpoleDynamicsModel
    CM = CartpoleDynamicsModel
    g = torch.Generator().manual_seed(3)
    X = torch.cat([torch.randn(70, 2, generator=g),
                   3.0 + 0.8 * torch.randn(70, 1, generator=g),
                   torch.randn(70, 1, generator=g)], -1)
    U = 3.0 * torch.randn(70, 1, generator=g)
    with torch.no_grad():
        dX = CM(0.1)(X, U, 0, StateEncoding.IGNORE_UNCERTAINTY) - X
    model = gp_dynamics_model_factory(4, 1, CM.angular_indices,
                                      CM.non_angular_indices)().cuda()
    model.fit(X.cuda(), U.cuda(), dX.cuda())
    model.eval()
    enc = StateEncoding.DEFAULT
    B, N, n, m = 8, 10, 14, 1
    z0 = torch.stack([GaussianVariable(
        torch.tensor([0.0, 0.0, 3.0, 0.0]) + 0.05 * torch.randn(4, generator=g),
        var=1e-2 * torch.ones(4)).encode(enc) for _ in range(B)]).cuda()
    U0 = (0.3 * torch.randn(B, N, m, generator=g)).cuda()
    end = []
    with _forced(chunk=64, rows=32):
        assert model.native_form(z0, enc, jacobian=True) == "chunked"
        for graph in (False, True):
            plugin = TorchProblem(model, CartpoleCost().cuda(), enc, {}, {})
            s = ILQRSolver(None, B, N, torch.float32, "cuda",
                           torch.tensor([-10.0]), torch.tensor([10.0]),
                           fit_alphas(torch.float32, "cuda"), plugin=plugin,
                           n=n, m=m)
            s.set_nominal(z0, U0)
            assert s.graph_ok()
            rounds = s.fit(n_iterations=4, graph=graph, max_rounds=6)
            assert plugin.last_derivs_path["dynamics"] == "hip"
            end.append((rounds, s.Z.clone(), s.U.clone(), s.J_opt.clone(),
                        s.state.clone()))
            del s, plugin
    assert end[0][0] == end[1][0] and end[0][0] >= 2
    for a, b in zip(end[0][1:], end[1][1:]):
        assert torch.equal(a, b)
