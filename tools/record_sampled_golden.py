"""Records what the sampling planners compute at small shapes - pddp_shoot_*,
pddp_mppi_* (plain, _batch, _track, _weighted, _track_weighted),
pddp_shoot_draws_*, pddp_mppi_trial_* and pddp_mppi_trial_goals_*: the fixture
of tests/test_sampled_kernels_golden.py, which holds later builds to it byte
for byte.  Record it from the build the change under test STARTS from (its
parent commit), on an MI355X, never from the code under test:

    python tools/record_sampled_golden.py [tests/golden/sampled_kernels_parent.npz]

(PDDP_HIP_LIB selects the library, pddp_amd/_native.py; only C ABI entry points
are called.)

As in tools/record_problem_golden.py, whose helpers this tool uses: every
output buffer holds a sentinel before the launch, part of every mask is
switched off and the inputs are rounded through float32.  Stored whole: best,
J_best, J_w, the trial's logs (Xlog, Ulog, Jcl, Ylog, J0, J_w, ess), z0, U and
x_true, and the costs and W at S = 3.  Stored as 8-byte BLAKE2b digests of
their bytes, one per trajectory: Z_out and U_out, the costs and W at S = 70 and
260 (whole, the 990 costs of each of the 60 launches would alone be larger than
any fixture here), the trial's Z and plan_log, the draws, and of the trial run
in two launches (2 + 1 control steps) ONE digest over the trajectory's rows of
everything the whole run stores.  Launches of one shape are stacked into one
array (an .npz entry costs a few hundred bytes whatever it holds)."""
import ctypes
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location(
    "record_trial_golden",
    os.path.join(ROOT, "tools", "record_trial_golden.py"))
trial = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(trial)
track, base = trial.track, trial.base

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden",
                           "sampled_kernels_parent.npz")

CASES = base.CASES
case_name = base.case_name

# One lane per candidate, a trajectory on G consecutive lanes: S = 3 (G = 4)
# several trajectories share a wavefront, with idle lanes; S = 70 (G = 128) two
# wavefronts meet in LDS; S = 260 (G = 256) four lanes take a second turn, and
# MPPI carries the running sum in U_out / U_work.  The reference of 4 rows
# starts at row 1: the hold is entered inside the horizon, and during the trial.
SHAPE = dict(B=3, N=6, Ss=(3, 70, 260), ref_len=4, ref_t0=1, sample_offset=5,
             whole_up_to=3, smooths=(0.0, 0.7))
FORMS = ("", "_batch", "_track", "_weighted", "_track_weighted")
# The options of a launch - the rows (Z_out and U_out), J_best (shoot) / W
# (mppi), the table of the suffixed forms / J_best (mppi), the active mask -
# covered pairwise: every two meet in all four on / off combinations over these
# five rows.  Form f at the i-th S and the j-th smooth takes row
# (f + i + 2 j) mod 5, so every form meets every row.
OPTIONS = ("rows", "best", "table", "active")
OPTION_ROWS = ((0, 0, 0, 0), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1),
               (1, 1, 1, 0))
assert all({(r[i], r[j]) for r in OPTION_ROWS} ==
           {(0, 0), (0, 1), (1, 0), (1, 1)}
           for i in range(4) for j in range(i))
DRAWS = dict(B=3, N=6, S=3, sample_offset=5)
# The trial: TT = 3 control steps of K = 2 iterations, once in one launch and
# once as 2 + 1.  (entry point, table, plant, process noise, measurement noise,
# disturbance, reference, weights); variant v runs at the (v mod 3)-th S, with
# smooth 0.7, the logs and the mask where v is odd, every candidate's cost
# logged where v is even.
TRIAL = dict(B=3, N=6, TT=3, K=2, chunks=((3,), (2, 1)), ref_len=4, ref_t0=1,
             cand_offset=7, rollout_offset=5, step_offset=2, whole_up_to=3)
TRIAL_VARIANTS = (
    ("mppi_trial", 0, 0, 0, 0, 0, 0, 0), ("mppi_trial", 1, 0, 0, 0, 0, 0, 0),
    ("mppi_trial", 1, 1, 0, 0, 0, 0, 0), ("mppi_trial", 0, 0, 1, 0, 0, 0, 0),
    ("mppi_trial", 0, 0, 0, 1, 0, 0, 0), ("mppi_trial", 1, 0, 1, 1, 0, 0, 0),
    ("mppi_trial", 0, 1, 0, 0, 1, 0, 0),
    ("mppi_trial_goals", 0, 1, 0, 0, 0, 1, 0),
    ("mppi_trial_goals", 1, 0, 1, 0, 1, 0, 1),
    ("mppi_trial_goals", 1, 1, 1, 1, 0, 1, 1))
SEED = trial.SEED
SENTINEL = base.SENTINEL
joint_digests = trial.joint_digests


def weights_of(prob, B, seed, td):
    """[B][WEIGHT_ROW]: the shared diagonals of Q, Q_term, R x U(1, 2), rounded
    to float32."""
    import torch
    from pddp_amd import _native as N_
    rng = np.random.RandomState(seed)
    na, m = prob.aug_size, prob.action_size
    w = np.zeros((B, N_.WEIGHT_ROW))
    for off, mat, ld, k in ((N_.WEIGHT_Q, prob.Q, N_.MAX_AUG, na),
                            (N_.WEIGHT_Q_TERM, prob.Q_term, N_.MAX_AUG, na),
                            (N_.WEIGHT_R, prob.R, N_.MAX_ACTION, m)):
        w[:, off:off + k] = np.array([mat[i * ld + i] for i in range(k)]) * \
            rng.uniform(1.0, 2.0, (B, k))
    w = w.astype(np.float32).astype(np.float64)
    return torch.from_numpy(w).to(td).cuda().contiguous()


def run_case(problem, dtype, bounded):
    """{name: array as stored} of one (model, dtype, bounds)."""
    import torch
    from pddp_amd import _native as N_
    from pddp_amd.examples.problems import SampleProblems
    from pddp_amd.utils.encoding import StateEncoding
    sp = SampleProblems[problem.upper()]
    prob = sp.get_model_class()(base.DT[problem]).native_problem(
        StateEncoding.IGNORE_UNCERTAINTY, sp.get_cost_class()())
    td = torch.float32 if dtype == "f32" else torch.float64
    n, m = prob.encoded_size, prob.action_size
    lib, p, pp = N_.lib(), N_.ptr, ctypes.addressof(prob)
    st = N_.stream_handle()
    rng = np.random.RandomState(17)
    bound = base.BOUND[problem]
    u_min = torch.full((m,), -bound, dtype=td).cuda() if bounded else None
    u_max = torch.full((m,), bound, dtype=td).cuda() if bounded else None
    digests = base.digests

    def dev(a):
        a = np.ascontiguousarray(a).astype(np.float32).astype(np.float64)
        return torch.from_numpy(a).to(td).cuda()

    def full(*shape):
        return torch.full(shape, SENTINEL, dtype=td, device="cuda")

    def states(*shape):
        return dev(np.asarray(base.MEAN0[problem], np.float64) +
                   0.1 * rng.randn(*shape, n))

    def actions(*shape):  # (a tenth of them beyond the bounds)
        return dev(0.6 * bound * rng.randn(*shape, m))

    def call(name, *args):
        fn = getattr(lib, "pddp_%s_%s" % (name, dtype))
        N_.check(fn(*args), fn.__name__)

    def host(t):  # (waits for the stream)
        return t.detach().cpu().numpy()

    def costs(t, S, upto):  # whole, or a digest per trajectory
        return host(t) if S <= upto else digests(host(t), 1)

    out = {}
    B, N = SHAPE["B"], SHAPE["N"]
    L, t0 = SHAPE["ref_len"], SHAPE["ref_t0"]
    z0_in, U_in = states(B), actions(B, N)
    a_std = dev(0.3 * bound * (1.0 + np.arange(m) / m))
    lam = dev([50.0, 10.0, 200.0])
    table = base.table_of(prob, problem, B, 61, td)
    ref = track.reference_of(prob, B, L, 62, td)
    weights = weights_of(prob, B, 63, td)
    active = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()

    def lead_of(form, with_table):
        tab = p(table if with_table else None)
        return {"": (pp,), "_batch": (pp, p(table)),
                "_track": (pp, tab, p(ref), L, t0),
                "_weighted": (pp, tab, p(weights)),
                "_track_weighted": (pp, tab, p(ref), L, t0, p(weights))}[form]

    # -- shoot and mppi, every form ------------------------------------------------
    stacked = {}
    for i, S in enumerate(SHAPE["Ss"]):
        rows = {"shoot": [], "mppi": []}
        for j, smooth in enumerate(SHAPE["smooths"]):
            for f, form in enumerate(FORMS):
                on = dict(zip(OPTIONS, OPTION_ROWS[(f + i + 2 * j) % 5]))
                lead = lead_of(form, on["table"])
                mask = p(active if on["active"] else None)
                # shoot
                Jc, Z, U = full(B, S), full(B, N + 1, n), full(B, N, m)
                best = torch.full((B,), -9, dtype=torch.int32, device="cuda")
                J_best = full(B)
                call("shoot" + form, *lead, B, N, S, p(z0_in), p(U_in),
                     p(u_min), p(u_max), p(a_std), smooth, SEED,
                     SHAPE["sample_offset"], mask, p(Jc), p(best),
                     p(J_best if on["best"] else None),
                     p(Z if on["rows"] else None),
                     p(U if on["rows"] else None), st)
                rows["shoot"].append(dict(
                    Jc=costs(Jc, S, SHAPE["whole_up_to"]), best=host(best),
                    J_best=host(J_best),
                    Z_U=np.stack([digests(host(Z), 1), digests(host(U), 1)])))
                # mppi (above one turn the running sum lives in U_out)
                keep = bool(on["rows"]) or S > 256
                Jc, Z, U = full(B, S), full(B, N + 1, n), full(B, N, m)
                best = torch.full((B,), -9, dtype=torch.int32, device="cuda")
                J_best, W, J_w = full(B), full(B, S), full(B)
                call("mppi" + form, *lead, B, N, S, p(z0_in), p(U_in),
                     p(u_min), p(u_max), p(a_std), p(lam), smooth, SEED,
                     SHAPE["sample_offset"], mask, p(Jc), p(best),
                     p(J_best if on["table"] else None),
                     p(W if on["best"] else None), p(J_w),
                     p(Z if keep else None), p(U if keep else None), st)
                rows["mppi"].append(dict(
                    Jc=costs(Jc, S, SHAPE["whole_up_to"]), best=host(best),
                    J_best=host(J_best),
                    W=costs(W, S, SHAPE["whole_up_to"]), J_w=host(J_w),
                    Z_U=np.stack([digests(host(Z), 1), digests(host(U), 1)])))
        for name, launches in rows.items():
            for k in launches[0]:
                a = np.stack([r[k] for r in launches])
                if k in ("Jc", "W"):  # (their shape is S's)
                    out["%s/%s_S%d" % (name, k, S)] = a
                else:
                    stacked.setdefault("%s/%s" % (name, k), []).append(a)
    for k, parts in stacked.items():
        out[k] = np.stack(parts)

    # -- the unit normals written out ------------------------------------------------
    E = full(DRAWS["B"], DRAWS["N"], DRAWS["S"], m)
    call("shoot_draws", DRAWS["B"], DRAWS["N"], DRAWS["S"], m, SEED,
         DRAWS["sample_offset"], p(E), st)
    out["draws/E"] = digests(host(E), 2)

    # -- the trial ------------------------------------------------------------------
    TT, K = TRIAL["TT"], TRIAL["K"]
    plant = base.table_of(prob, problem, B, 64, td)
    dist = dev(0.01 * rng.randn(B, TT, n))
    w_std = dev(0.02 * (1.0 + np.arange(n) / n))
    v_std = dev(0.01 * (2.0 - np.arange(n) / n))
    x_in = dev(host(z0_in).astype(np.float64) + 0.01 * rng.randn(B, n))
    logs = {}
    for v, (entry, tb, pl, proc, obs, ds, rf, wt) in enumerate(TRIAL_VARIANTS):
        S = SHAPE["Ss"][v % 3]
        odd = v % 2 == 1
        smooth = 0.7 if odd else 0.0
        log_costs = 0 if odd else 1
        lead = (pp, p(table if tb else None), p(plant if pl else None))
        if entry == "mppi_trial_goals":
            lead += (p(ref if rf else None), TRIAL["ref_len"],
                     TRIAL["ref_t0"], p(weights if wt else None))
        for chunks in TRIAL["chunks"]:
            z0, U, Z = z0_in.clone(), U_in.clone(), full(B, N + 1, n)
            U_work, x_true = full(B, N, m), x_in.clone()
            Jc = full(B, TT, K, S) if log_costs else full(B, S)
            Xlog, Ulog, Jcl = full(B, TT + 1, n), full(B, TT, m), full(B)
            Ylog, J0, Jw = full(B, TT + 1, n), full(B, TT, K), full(B, TT, K)
            ess, plans = full(B, TT), full(B, TT, N, m)
            c0 = 0
            for count in chunks:
                call(entry, *lead, B, N, S, K, TT, c0, count, p(z0), p(U),
                     p(Z), p(U_work), p(u_min), p(u_max), p(a_std), p(lam),
                     smooth, SEED, TRIAL["cand_offset"], B * S,
                     p(dist if ds else None), p(w_std if proc else None),
                     p(v_std if obs else None), TRIAL["rollout_offset"],
                     TRIAL["step_offset"], p(x_true),
                     p(active if odd else None), p(Jc), log_costs, p(Xlog),
                     p(Ulog), p(Jcl), p(Ylog), p(J0 if odd else None),
                     p(Jw if odd else None), p(ess if odd else None),
                     p(plans if odd else None), st)
                c0 += count
            whole = dict(
                z0=host(z0), U=host(U), x_true=host(x_true), Xlog=host(Xlog),
                Ulog=host(Ulog), Jcl=host(Jcl), Ylog=host(Ylog), J0=host(J0),
                Jw=host(Jw), ess=host(ess),
                Jc=costs(Jc, S, TRIAL["whole_up_to"]),
                Z_plans=np.stack([digests(host(Z), 1),
                                  digests(host(plans), 1)]))
            if len(chunks) == 1:
                if S <= TRIAL["whole_up_to"]:  # (its shape is the variant's)
                    out["trial/Jc_%d" % v] = whole.pop("Jc")
                for k, a in whole.items():
                    logs.setdefault("trial/" + k, []).append(a)
            else:
                logs.setdefault("trial/split", []).append(joint_digests(
                    [host(a) for a in (z0, U, x_true, Xlog, Ulog, Jcl, Ylog,
                                       J0, Jw, ess, Jc, Z, plans)]))
    for k, parts in logs.items():
        out[k] = np.stack(parts)
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
