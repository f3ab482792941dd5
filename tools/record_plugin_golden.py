"""Records what the plugin path (pddp_amd/controllers/plugin.py TorchProblem)
computes at small shapes through every one of its paths: the BNN kernels
(rollout, forward-mode records with and without a mask, line search, with and
without the predicted std, independent noise, f32 and f64), the GP kernels
(records, masked records, the line search by the rollout kernel and per step,
one case per branch of the batched costs), the QR-cost kernel (two leaves and
an expression tree) and the generic autograd path.  It is the fixture of
tests/test_plugin_paths_golden.py, which holds later builds to it byte for
byte.  Record it from the build the change under test STARTS from (its parent
commit), on an MI355X, never from the code under test:

    python tools/record_plugin_golden.py [tests/golden/plugin_paths_parent.npz]

Only TorchProblem's own methods and ILQRSolver's buffers are used, so the same
text runs on either side of a change of the host code.

Every case seeds torch (`torch.manual_seed`): the network's weights, its
dropout masks and every normal the plugin draws are torch's, so the fixture
also holds `torch.__version__` and the test skips under another.  The inputs
come from CPU generators; the GPs are conditioned on the CPU in float64 and
moved.  Every output buffer holds a sentinel before the call, so rows that a
mask skips are part of the bytes.  Stored whole: arrays of up to 2 KB.  Larger
arrays are stored as 8-byte BLAKE2b digests of their bytes, one per
trajectory."""
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

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "plugin_paths_parent.npz")
SENTINEL = base.SENTINEL
WHOLE_UP_TO = 2048  # bytes
B, N = 3, 4

# name: (dtype, model_opts beyond the two every BNN workload passes)
BNN = {
    "f32": ("f32", {}),
    "f32_std": ("f32", {"use_predicted_std": True}),
    "f32_std_independent": ("f32", {"use_predicted_std": True,
                                    "independent_noise": True}),
}
# name: (dtype, encoding): 1 / 2 / 4 take the three branches of the batched
# costs (Cholesky factor, variances, mean only)
GP = {"f64_enc1": ("f64", 1), "f32_enc1": ("f32", 1), "f64_enc2": ("f64", 2),
      "f64_enc4": ("f64", 4)}
QR = ("cartpole_leaf", "pendulum_leaf", "cartpole_tree")

CASES = ([("bnn", k) for k in BNN] + [("bnn64", "native64")] +
         [("gp", k) for k in GP] + [("qr", k) for k in QR] +
         [("generic", "bnn_f32")])


def case_name(family, key):
    return "%s_%s" % (family, key)


def stored(a):
    """The array as the fixture holds it (see the module's text)."""
    a = np.ascontiguousarray(a)
    return a if a.nbytes <= WHOLE_UP_TO else base.digests(a, 1)


def _host(t):  # (waits for the stream)
    return stored(t.detach().cpu().numpy())


def _path(plugin):
    p = plugin.last_derivs_path
    return np.array([p["dynamics"], p["cost"]])


def _inputs(D, mean0, enc, td, seed, m=1):
    """z0 [B, n] and U [B, N, m] from a CPU generator, on the device."""
    import torch
    import pddp_amd
    g = torch.Generator().manual_seed(seed)
    mean = torch.tensor(mean0, dtype=torch.float64)
    z0 = torch.stack([pddp_amd.GaussianVariable(
        mean + 0.05 * torch.randn(D, generator=g, dtype=torch.float64),
        var=1e-2 * torch.ones(D, dtype=torch.float64)).encode(enc)
        for _ in range(B)])
    U = 0.3 * torch.randn(B, N, m, generator=g, dtype=torch.float64)
    return z0.to(td).cuda(), U.to(td).cuda(), g


def _solver(plugin, td, n, m=1, bound=0.4):
    """(a part of the actions lies beyond the bounds)"""
    import torch
    from pddp_amd.controllers.ilqr import fit_alphas
    from pddp_amd.controllers.solver import ILQRSolver
    return ILQRSolver(None, B, N, td, "cuda", torch.tensor([-bound] * m),
                      torch.tensor([bound] * m), fit_alphas(td, "cuda"),
                      plugin=plugin, n=n, m=m)


def _round(out, s, z0, U, g, second_search=None):
    """rollout, records, masked records and the line search of one solver:
    what each leaves in the solver's buffers."""
    import torch
    plugin = s.plugin
    s.Z.fill_(SENTINEL)
    s.set_nominal(z0, U)  # (plugin.rollout)
    out["rollout/Z"] = _host(s.Z)

    def records(tag, mask):
        s._rec.fill_(SENTINEL)
        s.L.fill_(SENTINEL)
        s.J_opt.fill_(SENTINEL)
        s.state.fill_(3)
        plugin.derivs(s, mask)
        for k, t in (("rec", s.rec), ("L", s.L), ("J_opt", s.J_opt),
                     ("state", s.state)):
            out[tag + "/" + k] = _host(t)
        out[tag + "/path"] = _path(plugin)
    records("derivs", None)
    records("derivs_masked", torch.tensor([1, 0, 1], dtype=s.fresh.dtype,
                                          device="cuda"))
    # the line search under seeded gains: trajectory 2 dropped, the sweep of
    # trajectory 1 failed
    s.gains.copy_((0.05 * torch.randn(s.gains.shape, generator=g,
                                      dtype=torch.float64)).to(s.dtype))
    s.active.fill_(1)
    s.active[2] = 0
    s.bwd_status.zero_()
    s.bwd_status[1] = 2

    def search(tag):
        for t in (s.Zc, s.Uc, s.Jc):
            t.fill_(SENTINEL)
        plugin.line_search(s, s.active, True)
        for k, t in (("Zc", s.Zc), ("Uc", s.Uc), ("Jc", s.Jc)):
            out[tag + "/" + k] = _host(t)
    search("line_search")
    if second_search is not None:
        second_search()
        search("line_search_2")


def _bnn_model(H, P, td):
    from pddp_amd.examples import cartpole
    from pddp_amd.models.bnn import bnn_dynamics_model_factory
    import torch
    CM = cartpole.CartpoleDynamicsModel
    model = bnn_dynamics_model_factory(
        4, 1, [H, H], CM.angular_indices, CM.non_angular_indices)(
            n_particles=P).to(td).cuda().eval()
    with torch.no_grad():  # untrained weights: keep the dynamics gentle
        model.model.out.weight.mul_(0.05)
        model.model.out.bias.mul_(0.05)
    return model, cartpole.CartpoleCost().to(td).cuda()


def _gp_model(system, M, td):
    """A GP of one of the example systems, conditioned on the CPU in float64."""
    import torch
    import pddp_amd.examples as ex
    from pddp_amd.models.gp import gp_dynamics_model_factory
    mod = getattr(ex, system)
    MC = [getattr(mod, k) for k in dir(mod) if k.endswith("DynamicsModel") and
          k != "DynamicsModel"][0]
    cost_cls = [getattr(mod, k) for k in dir(mod) if k.endswith("Cost") and
                k not in ("AugmentedQRCost", "QRCost")][0]
    E = MC.state_size
    g = torch.Generator().manual_seed(2)
    X = torch.randn(M, E, generator=g, dtype=torch.float64)
    U = torch.randn(M, 1, generator=g, dtype=torch.float64)
    dX = 0.1 * torch.randn(M, E, generator=g, dtype=torch.float64)
    model = gp_dynamics_model_factory(E, 1, MC.angular_indices,
                                      MC.non_angular_indices)().double()
    model.fit(X, U, dX)
    return model.to(td).cuda().eval(), cost_cls().to(td).cuda(), E


def run_case(family, key):
    """{name: array as stored} of one case."""
    import torch
    import pddp_amd
    from pddp_amd.controllers.plugin import TorchProblem
    from pddp_amd.utils.encoding import infer_encoded_state_size
    DEFAULT = pddp_amd.StateEncoding.DEFAULT
    TD = {"f32": torch.float32, "f64": torch.float64}
    start = [0.0, 0.0, 3.0, 0.0]
    torch.manual_seed(1234)
    out = {}
    if family in ("bnn", "generic"):
        dtype, extra = BNN[key] if family == "bnn" else ("f32", {})
        td = TD[dtype]
        model, cost = _bnn_model(64, 30, td)
        opts = dict({"use_predicted_std": False,
                     "infer_noise_variables": True}, **extra)
        plugin = TorchProblem(model, cost, DEFAULT, opts, {})
        if family == "generic":
            plugin.use_native_bnn = plugin.use_native_bnn_jvp = False
            plugin.use_native_gp = plugin.use_native_cost = False
        s = _solver(plugin, td, 14)
        z0, U, g = _inputs(4, start, DEFAULT, td, 31)
        _round(out, s, z0, U, g)
    elif family == "bnn64":
        # tests/solver_util.py bnn_problem: [200, 200] hidden, 100 particles
        import copy
        tests = os.path.join(ROOT, "tests")
        if tests not in sys.path:
            sys.path.insert(0, tests)
        from solver_util import bnn_problem
        model, cost, z0, U, solver = bnn_problem("cartpole", B, N)
        m64 = copy.deepcopy(model).double()
        m64.eps_in = {k: v.double() for k, v in model.eps_in.items()}
        m64.output = {}
        s = solver(m64, copy.deepcopy(cost).double(), B, torch.float64,
                   native64=True)
        _round(out, s, z0.double(), U.double(),
               torch.Generator().manual_seed(32))
    elif family == "gp":
        dtype, encoding = GP[key]
        td, enc = TD[dtype], pddp_amd.StateEncoding(encoding)
        model, cost, E = _gp_model("cartpole", 24, td)
        plugin = TorchProblem(model, cost, enc, {}, {})
        s = _solver(plugin, td, infer_encoded_state_size(E, enc))
        z0, U, g = _inputs(E, start, enc, td, 33)

        def per_step():
            plugin.use_gp_rollout = False
        _round(out, s, z0, U, g, second_search=per_step)
    else:
        td = torch.float32
        system = key.split("_")[0]
        model, cost, E = _gp_model(system, 8, td)
        if key.endswith("tree"):  # each of + - * / ** once
            cost = (cost + cost * 0.5) / (cost + 1.0) - (cost * 0.1) ** 2
        plugin = TorchProblem(None, cost, DEFAULT, {}, {})
        n = infer_encoded_state_size(E, DEFAULT)
        s = _solver(plugin, td, n)
        z0, U, g = _inputs(E, start[:E], DEFAULT, td, 34)
        # (no model: states along the horizon from the generator)
        Z = z0.unsqueeze(1) + (0.02 * torch.randn(
            B, N + 1, n, generator=g, dtype=torch.float64)).to(td).cuda()
        s.Z.copy_(Z)
        s.U.copy_(U)
        with torch.no_grad():
            out["native_ok"] = np.array(bool(plugin._qr_cost_native_ok(s)))
        kw = dict(dtype=td, device="cuda")
        blocks = [torch.full(shape, SENTINEL, **kw) for shape in (
            (B, N + 1), (B, N + 1, n), (B, N, 1), (B, N + 1, n, n),
            (B, N, 1, n), (B, N, 1, 1))]
        plugin._cost_derivs_qr(s, *blocks)
        for k, t in zip(("L", "L_z", "L_u", "L_zz", "L_uz", "L_uu"), blocks):
            out[k] = _host(t)
    return out


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    blob = {"torch_version": np.array(torch.__version__)}
    for case in CASES:
        for k, v in run_case(*case).items():
            blob[case_name(*case) + "/" + k] = v
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **blob)
    print("%d cases, %d arrays, %d bytes -> %s" % (
        len(CASES), len(blob), os.path.getsize(out), out))


if __name__ == "__main__":
    main()
