"""Records what the cross-entropy planners compute at small shapes - pddp_cem_*
(plain, _batch, _track, _weighted, _track_weighted) and pddp_cem_trial_*: the
fixture of tests/test_cem_kernels_golden.py, which holds later builds to it
byte for byte.  Record it from the build the change under test STARTS from (its
parent commit), on an MI355X, never from the code under test:

    python tools/record_cem_golden.py [tests/golden/cem_kernels_parent.npz]

(PDDP_HIP_LIB selects the library, pddp_amd/_native.py; only C ABI entry points
are called.)

As in tools/record_sampled_golden.py, whose helpers and shapes this tool uses:
every output buffer, log buffer and work buffer holds a sentinel before the
launch, part of every mask is switched off and the inputs are rounded through
float32.  Stored whole: best, J_best, n_elite, J_m, the trial's logs (Xlog,
Ulog, Jcl, Ylog, J_trace, J_m, n_elite), z0, U and x_true, and the costs and
ranks at S = 3.  Stored as 8-byte BLAKE2b digests of their bytes, one per
trajectory: Z_out, U_out and S_out, the costs and ranks at S = 70 and 260, the
trial's Z, sigma, plan_log, std_log and its four work buffers, and of the trial
run in two launches (2 + 1 control steps) ONE digest over the trajectory's rows
of everything the whole run stores.  Launches of one shape are stacked into one
array."""
import ctypes
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location(
    "record_sampled_golden",
    os.path.join(ROOT, "tools", "record_sampled_golden.py"))
sampled = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sampled)
trial, track, base = sampled.trial, sampled.track, sampled.base

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "cem_kernels_parent.npz")

CASES = base.CASES
case_name = base.case_name

# record_sampled_golden.py's shapes: S = 3 (G = 4) several trajectories share a
# wavefront, with idle lanes; S = 70 (G = 128) two wavefronts meet in LDS - the
# ranking's chunk and the moments' partial sums; S = 260 (G = 256) four lanes
# take a second turn: a second chunk is ranked against, and the running sums
# are carried in U_out / S_out (Um / Sm in the trial).
SHAPE = dict(sampled.SHAPE, mixes=(0.0, 0.25))
FORMS = sampled.FORMS
# The options of a launch - the rows (Z_out, U_out and S_out; above one turn
# they are always there), rank, J_best, std_min, the table of the suffixed
# forms, the active mask - covered pairwise over these six rows.  Form f at the
# i-th S and the j-th smooth takes row (f + i + 3 j) mod 6, so every form meets
# every row; its mix is the ((f + i + j) mod 2)-th and its K the
# ((f + i + j) mod 3)-th of 1, an interior one and S.
OPTIONS = ("rows", "rank", "best", "floor", "table", "active")
OPTION_ROWS = ((0, 0, 0, 0, 0, 0), (1, 1, 1, 0, 1, 0), (1, 1, 0, 1, 0, 1),
               (1, 0, 1, 1, 0, 0), (0, 1, 1, 0, 1, 1), (0, 0, 0, 1, 1, 1))
assert all({(r[i], r[j]) for r in OPTION_ROWS} ==
           {(0, 0), (0, 1), (1, 0), (1, 1)}
           for i in range(6) for j in range(i))
INTERIOR_K = {3: 2, 70: 9, 260: 37}
# One more launch per type at S = 70 with K = S and the width scaled per
# trajectory, so that candidates' costs pass the type's largest number: costs
# that are not finite tie at +inf in the ranking, and Ke < K.  The largest
# scale is where the pendulum's cost overflows under some draws and not under
# others; the cartpoles, whose accelerations hold a squared velocity, compound
# and do so at the smallest one (as recorded, n_elite there is 63 and 55 of 70
# in f32); the rendezvous stays finite.  (Under bounds the clamped actions keep
# every cost finite: the same launch, all ranked.)
WIDE = dict(S=70, scales={"f32": (1e2, 1e7, 3e18),
                          "f64": (1e4, 1e30, 1e153)})
# The trial: TT = 3 control steps of I = 2 iterations, once in one launch and
# once as 2 + 1.  (table, plant, process noise, measurement noise, disturbance,
# sigma0, std_min); variant v runs at the (v mod 3)-th S, with smooth 0.7, the
# logs and the mask where v is odd, every candidate's cost logged where v is
# even, mix 0.25 where v mod 4 >= 2.
TRIAL = dict(sampled.TRIAL, I=2, Ks=(2, 9, 37))
TRIAL_VARIANTS = (
    (0, 0, 0, 0, 0, 1, 0), (1, 0, 0, 0, 0, 1, 1), (1, 1, 0, 0, 0, 0, 1),
    (0, 0, 1, 0, 0, 0, 0), (0, 0, 0, 1, 0, 1, 1), (1, 0, 1, 1, 0, 0, 1),
    (0, 1, 0, 0, 1, 1, 0), (1, 1, 1, 1, 1, 0, 0))
SEED = sampled.SEED
SENTINEL = base.SENTINEL
joint_digests = trial.joint_digests


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
    rng = np.random.RandomState(23)
    bound = base.BOUND[problem]
    u_min = torch.full((m,), -bound, dtype=td).cuda() if bounded else None
    u_max = torch.full((m,), bound, dtype=td).cuda() if bounded else None
    digests = base.digests

    def dev(a):
        a = np.ascontiguousarray(a).astype(np.float32).astype(np.float64)
        return torch.from_numpy(a).to(td).cuda()

    def full(*shape):
        return torch.full(shape, SENTINEL, dtype=td, device="cuda")

    def ints(*shape):
        return torch.full(shape, -9, dtype=torch.int32, device="cuda")

    def call(name, *args):
        fn = getattr(lib, "pddp_%s_%s" % (name, dtype))
        N_.check(fn(*args), fn.__name__)

    def host(t):  # (waits for the stream)
        return t.detach().cpu().numpy()

    def per_candidate(t, S):  # whole, or a digest per trajectory
        return host(t) if S <= SHAPE["whole_up_to"] else digests(host(t), 1)

    out = {}
    B, N = SHAPE["B"], SHAPE["N"]
    L, t0 = SHAPE["ref_len"], SHAPE["ref_t0"]
    z0_in = dev(np.asarray(base.MEAN0[problem], np.float64) +
                0.1 * rng.randn(B, n))
    U_in = dev(0.6 * bound * rng.randn(B, N, m))  # (a tenth beyond the bounds)
    sigma_in = dev(0.3 * bound * rng.uniform(0.5, 1.5, (B, N, m)))
    floor = dev(0.05 * bound * (1.0 + np.arange(m) / m))
    table = base.table_of(prob, problem, B, 71, td)
    ref = track.reference_of(prob, B, L, 72, td)
    weights = sampled.weights_of(prob, B, 73, td)
    active = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()

    def lead_of(form, with_table):
        tab = p(table if with_table else None)
        return {"": (pp,), "_batch": (pp, p(table)),
                "_track": (pp, tab, p(ref), L, t0),
                "_weighted": (pp, tab, p(weights)),
                "_track_weighted": (pp, tab, p(ref), L, t0, p(weights))}[form]

    def cem(form, on, S, K, sigma, smooth, mix):
        keep = bool(on["rows"]) or S > 256
        Jc, rank, best, J_best = full(B, S), ints(B, S), ints(B), full(B)
        n_elite, J_m = ints(B), full(B)
        Z, U, Sg = full(B, N + 1, n), full(B, N, m), full(B, N, m)
        call("cem" + form, *lead_of(form, on["table"]), B, N, S, K, p(z0_in),
             p(U_in), p(u_min), p(u_max), p(sigma),
             p(floor if on["floor"] else None), smooth, mix, SEED,
             SHAPE["sample_offset"], p(active if on["active"] else None),
             p(Jc), p(rank if on["rank"] else None), p(best),
             p(J_best if on["best"] else None), p(n_elite), p(J_m),
             p(Z if keep else None), p(U if keep else None),
             p(Sg if keep else None), st)
        return dict(
            Jc=per_candidate(Jc, S), rank=per_candidate(rank, S),
            best=host(best), J_best=host(J_best), n_elite=host(n_elite),
            J_m=host(J_m),
            Z_U_S=np.stack([digests(host(a), 1) for a in (Z, U, Sg)]))

    # -- cem, every form --------------------------------------------------------
    stacked = {}
    for i, S in enumerate(SHAPE["Ss"]):
        launches = []
        for j, smooth in enumerate(SHAPE["smooths"]):
            for f, form in enumerate(FORMS):
                on = dict(zip(OPTIONS, OPTION_ROWS[(f + i + 3 * j) % 6]))
                K = (1, INTERIOR_K[S], S)[(f + i + j) % 3]
                mix = SHAPE["mixes"][(f + i + j) % 2]
                launches.append(cem(form, on, S, K, sigma_in, smooth, mix))
        for k in launches[0]:
            a = np.stack([r[k] for r in launches])
            if k in ("Jc", "rank"):  # (their shape is S's)
                out["cem/%s_S%d" % (k, S)] = a
            else:
                stacked.setdefault("cem/" + k, []).append(a)
    for k, parts in stacked.items():
        out[k] = np.stack(parts)
    scale = torch.tensor(WIDE["scales"][dtype], dtype=td).cuda()
    wide = cem("", dict(zip(OPTIONS, (1, 1, 1, 0, 0, 0))), WIDE["S"],
               WIDE["S"], sigma_in * scale.reshape(B, 1, 1), 0.7, 0.25)
    for k, a in wide.items():
        out["cem_wide/" + k] = a

    # -- the trial --------------------------------------------------------------
    TT, I = TRIAL["TT"], TRIAL["I"]
    plant = base.table_of(prob, problem, B, 74, td)
    dist = dev(0.01 * rng.randn(B, TT, n))
    w_std = dev(0.02 * (1.0 + np.arange(n) / n))
    v_std = dev(0.01 * (2.0 - np.arange(n) / n))
    x_in = dev(host(z0_in).astype(np.float64) + 0.01 * rng.randn(B, n))
    logs = {}
    for v, (tb, pl, proc, obs, ds, s0, fl) in enumerate(TRIAL_VARIANTS):
        S, K = SHAPE["Ss"][v % 3], TRIAL["Ks"][v % 3]
        odd = v % 2 == 1
        smooth = 0.7 if odd else 0.0
        mix = 0.25 if v % 4 >= 2 else 0.0
        log_costs = 0 if odd else 1
        for chunks in TRIAL["chunks"]:
            z0, U, Z = z0_in.clone(), U_in.clone(), full(B, N + 1, n)
            sigma, x_true = sigma_in.clone(), x_in.clone()
            work = [full(B, N, m) for _ in range(4)]
            Jc = full(B, TT, I, S) if log_costs else full(B, S)
            Xlog, Ulog, Jcl = full(B, TT + 1, n), full(B, TT, m), full(B)
            Ylog, Jtr, Jm = full(B, TT + 1, n), full(B, TT, I + 1), \
                full(B, TT, I)
            nel, plans, stds = ints(B, TT, I), full(B, TT, N, m), \
                full(B, TT, N, m)
            c0 = 0
            for count in chunks:
                call("cem_trial", pp, p(table if tb else None),
                     p(plant if pl else None), B, N, S, K, I, TT, c0, count,
                     p(z0), p(U), p(Z), *[p(w) for w in work], p(u_min),
                     p(u_max), p(sigma), p(sigma_in if s0 else None),
                     p(floor if fl else None), smooth, mix, SEED,
                     TRIAL["cand_offset"], B * S, p(dist if ds else None),
                     p(w_std if proc else None), p(v_std if obs else None),
                     TRIAL["rollout_offset"], TRIAL["step_offset"], p(x_true),
                     p(active if odd else None), p(Jc), log_costs, p(Xlog),
                     p(Ulog), p(Jcl), p(Ylog), p(Jtr if odd else None),
                     p(Jm if odd else None), p(nel if odd else None),
                     p(plans if odd else None), p(stds if odd else None), st)
                c0 += count
            rows = [Z, sigma, plans, stds] + work
            whole = dict(
                z0=host(z0), U=host(U), x_true=host(x_true), Xlog=host(Xlog),
                Ulog=host(Ulog), Jcl=host(Jcl), Ylog=host(Ylog),
                J_trace=host(Jtr), J_m=host(Jm), n_elite=host(nel),
                Jc=per_candidate(Jc, S),
                rows=np.stack([digests(host(a), 1) for a in rows]))
            if len(chunks) == 1:
                if S <= SHAPE["whole_up_to"]:  # (its shape is the variant's)
                    out["trial/Jc_%d" % v] = whole.pop("Jc")
                for k, a in whole.items():
                    logs.setdefault("trial/" + k, []).append(a)
            else:
                logs.setdefault("trial/split", []).append(joint_digests(
                    [host(a) for a in [z0, U, x_true, Xlog, Ulog, Jcl, Ylog,
                                       Jtr, Jm, nel, Jc] + rows]))
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
