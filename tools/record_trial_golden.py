"""Records what the closed-loop rollouts (pddp_closed_loop_*, _noisy_*,
_track_*, with the draws written out by pddp_closed_loop_draws_*) and the MPC
hand-over under noise (pddp_mpc_advance_noisy_*, pddp_mpc_observe_*) compute at
small shapes: the fixture of tests/test_trial_kernels_golden.py, which holds
later builds to it byte for byte.  Record it from the build the change under
test STARTS from (its parent commit), on an MI355X, never from the code under
test:

    python tools/record_trial_golden.py [tests/golden/trial_kernels_parent.npz]

(PDDP_HIP_LIB selects the library, pddp_amd/_native.py; only C ABI entry points
are called.  The untracked and the tracked noise-free hand-over are
tools/record_track_golden.py's.)

As in tools/record_problem_golden.py, whose helpers this tool uses: every
output buffer holds a sentinel before the launch, part of every mask is
switched off and the inputs are rounded through float32.  Stored whole: the
statistics, the hand-over's costs, logs of states and controller words,
observations of pddp_mpc_observe_*, and the costs of the rollouts up to
S = 70.  Stored as 8-byte BLAKE2b digests of their bytes, one per trajectory:
Xc and Uc; the draws (one per trajectory and step); the costs at S = 260 (whole,
the 780 costs of each of the 96 launches would alone be larger than any fixture
here); and of the hand-over, after every control step, ONE digest over the
trajectory's rows of z0, U, Z, Xlog, Ulog, x_true and Ylog."""
import ctypes
import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location(
    "record_track_golden",
    os.path.join(ROOT, "tools", "record_track_golden.py"))
track = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(track)
base = track.base  # (tools/record_problem_golden.py)

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "trial_kernels_parent.npz")

CASES = base.CASES
case_name = base.case_name

# Closed loop, one lane per rollout, a trajectory on G consecutive lanes: S = 3
# (G = 4) several trajectories share a wavefront, with idle lanes; S = 70
# (G = 128) one trajectory spans two wavefronts, whose statistics meet in LDS;
# S = 260 (G = 256) four lanes run a second rollout.  Every kernel runs at every
# S; the reference of 4 rows starts at row 1, so the goals are held from step 2
# on and for the terminal cost.
LOOP = dict(B=3, N=6, Ss=(3, 70, 260), ref_len=4, ref_t0=1, sample_offset=5,
            whole_costs_up_to=70)
# (entry point, process noise, measurement noise)
LOOP_KERNELS = (("plain", False, False), ("noisy", True, False),
                ("noisy", False, True), ("noisy", True, True),
                ("track", False, False), ("track", True, True))
# The options of a launch - z0s, plant rows, gains, keep (Xc and Uc), stats,
# an active mask - covered pairwise: every two options meet in all four on /
# off combinations over these six rows.  Kernel k at the i-th S takes row
# (k + i) mod 6.
OPTIONS = ("z0s", "plant", "gains", "keep", "stats", "active")
OPTION_ROWS = ((0, 0, 0, 0, 0, 0), (1, 1, 1, 0, 0, 1), (1, 1, 0, 1, 0, 0),
               (1, 0, 1, 0, 1, 0), (0, 1, 0, 1, 1, 1), (0, 0, 1, 1, 1, 1))
assert all({(r[i], r[j]) for r in OPTION_ROWS} ==
           {(0, 0), (0, 1), (1, 0), (1, 1)}
           for i in range(6) for j in range(i))
DRAWS = dict(B=3, N=6, S=3, sample_offset=5)
# Hand-over, one lane per trajectory: T = 3 control steps in sequence (the last
# takes the terminal row), N = 1 is the shift's clamps alone (run without a
# table, N = 6 with one); the reference of 4 rows is held from control step 2.
ADVANCE = dict(B=3, Ns=(1, 6), T=3, ref_len=4, ref_t0=1, step_offset=2,
               rollout_offset=5,
               variants=("plain", "plant", "disturbance", "mask"),
               noises=((True, False), (False, True), (True, True)))
OBSERVE = dict(B=3, step=2, rollout_offset=5)
SEED = 0x9E3779B97F4A7C15
SENTINEL, STATE_SENTINEL = base.SENTINEL, base.STATE_SENTINEL
LIVE_SHARDS = 256  # PDDP_LIVE_SHARDS (include/pddp_hip.h)


def joint_digests(arrays):
    """uint64 [B]: one digest per trajectory over its rows of all `arrays`."""
    rows = [np.ascontiguousarray(a).reshape(a.shape[0], -1) for a in arrays]
    return np.array([int.from_bytes(hashlib.blake2b(
        b"".join(r[b].tobytes() for r in rows), digest_size=8).digest(),
        "little") for b in range(rows[0].shape[0])], dtype=np.uint64)


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
    GS = m + m * n
    lib, p, pp = N_.lib(), N_.ptr, ctypes.addressof(prob)
    st = N_.stream_handle()
    rng = np.random.RandomState(13)
    bound = base.BOUND[problem]
    u_min = torch.full((m,), -bound, dtype=td).cuda() if bounded else None
    u_max = torch.full((m,), bound, dtype=td).cuda() if bounded else None
    digests = base.digests

    def dev(a):
        a = np.ascontiguousarray(a).astype(np.float32).astype(np.float64)
        return torch.from_numpy(a).to(td).cuda()

    def full(*shape):
        return torch.full(shape, SENTINEL, dtype=td, device="cuda")

    def ints(B, value, dtype=torch.int32):
        return torch.full((B,), value, dtype=dtype, device="cuda")

    def states(*shape):
        return dev(np.asarray(base.MEAN0[problem], np.float64) +
                   0.1 * rng.randn(*shape, n))

    def actions(*shape):  # (a tenth of them beyond the bounds)
        return dev(0.6 * bound * rng.randn(*shape, m))

    def table_of(B, seed):
        return base.table_of(prob, problem, B, seed, td)

    def call(name, *args):
        fn = getattr(lib, "pddp_%s_%s" % (name, dtype))
        N_.check(fn(*args), fn.__name__)

    def host(t):  # (waits for the stream)
        return t.detach().cpu().numpy()

    w_std = dev(0.02 * (1.0 + np.arange(n) / n))
    v_std = dev(0.01 * (2.0 - np.arange(n) / n))
    out = {}

    # -- closed-loop rollouts ---------------------------------------------------
    B, N = LOOP["B"], LOOP["N"]
    ref = track.reference_of(prob, B, LOOP["ref_len"], 52, td)
    Z, U = states(B, N + 1), actions(B, N)
    gains = dev(0.1 * rng.randn(B, N, GS))
    active = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()
    for i, S in enumerate(LOOP["Ss"]):
        z0s = dev(host(Z)[:, :1].astype(np.float64) + 0.05 * rng.randn(B, S, n))
        plant = table_of(B * S, 53 + i).reshape(B, S, -1).contiguous()
        Jcs, stats_, wide = [], [], []
        for k, (entry, proc, obs) in enumerate(LOOP_KERNELS):
            on = dict(zip(OPTIONS, OPTION_ROWS[(k + i) % 6]))
            Xc, Uc = full(B, N + 1, S, n), full(B, N, S, m)
            Jc, stats = full(B, S), full(B, 4)
            lead = (pp,)
            if entry == "track":
                lead += (p(ref), LOOP["ref_len"], LOOP["ref_t0"])
            noise = () if entry == "plain" else (
                p(w_std if proc else None), p(v_std if obs else None), SEED,
                LOOP["sample_offset"])
            call("closed_loop" + ("" if entry == "plain" else "_" + entry),
                 *lead, B, N, S, p(Z), p(U), p(gains if on["gains"] else None),
                 p(z0s if on["z0s"] else None),
                 p(plant if on["plant"] else None), p(u_min), p(u_max), *noise,
                 p(active if on["active"] else None),
                 p(Xc if on["keep"] else None), p(Uc if on["keep"] else None),
                 p(Jc), p(stats if on["stats"] else None), st)
            Jcs.append(host(Jc) if S <= LOOP["whole_costs_up_to"]
                       else digests(host(Jc), 1))
            stats_.append(host(stats))
            wide.append(np.stack([digests(host(Xc), 1), digests(host(Uc), 1)]))
        out["loop_S%d/Jc" % S] = np.stack(Jcs)
        out["loop_S%d/stats" % S] = np.stack(stats_)
        out["loop_S%d/Xc_Uc" % S] = np.stack(wide)

    # -- the draws written out ----------------------------------------------------
    B, N, S = DRAWS["B"], DRAWS["N"], DRAWS["S"]
    W = []
    for which in (0, 1):
        Wd = full(B, N, S, n)
        call("closed_loop_draws", B, N, S, n, which, SEED,
             DRAWS["sample_offset"], p(Wd), st)
        W.append(digests(host(Wd), 2))
    out["draws/W"] = np.stack(W)

    # -- the first observation of a trial ---------------------------------------------
    B = OBSERVE["B"]
    x, ys = states(B), []
    for mask in (None, torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()):
        y = full(B, n)
        call("mpc_observe", B, n, p(x), p(v_std), SEED,
             OBSERVE["rollout_offset"], OBSERVE["step"], p(mask), p(y), st)
        ys.append(host(y))
    out["observe/y"] = np.stack(ys)

    # -- the MPC hand-over under noise, tracked and untracked ------------------------
    B, T = ADVANCE["B"], ADVANCE["T"]
    plant = table_of(B, 56)
    ref = track.reference_of(prob, B, ADVANCE["ref_len"], 57, td)
    for N in ADVANCE["Ns"]:
        table = table_of(B, 55) if N > 1 else None
        z0_in, U_in = states(B), actions(B, N)
        x_in = dev(host(z0_in).astype(np.float64) + 0.01 * rng.randn(B, n))
        dist_in = dev(0.01 * rng.randn(B, T, n))
        wide, Jcls, words, shards = [], [], [], []
        runs = [(tr, ns, v) for tr in (True, False) for ns in ADVANCE["noises"]
                for v in ADVANCE["variants"]]
        for tracked, (proc, obs), variant in runs:
            z0, U, Z = z0_in.clone(), U_in.clone(), full(B, N + 1, n)
            x_true, Ylog = x_in.clone(), full(B, T + 1, n)
            Xlog, Ulog, Jcl = full(B, T + 1, n), full(B, T, m), full(B)
            state_log = torch.full((B, T), STATE_SENTINEL, dtype=torch.int32,
                                   device="cuda")
            live_log = torch.full((B, T), 9, dtype=torch.uint8, device="cuda")
            # the controller as some rounds left it
            mu = torch.tensor([0.5, 2.0, 8.0], dtype=torch.float64).cuda()
            delta = torch.tensor([1.0, 4.0, 0.25], dtype=torch.float64).cuda()
            state = torch.tensor([3, 1, 2], dtype=torch.int32).cuda()
            it = torch.tensor([4, 7, 2], dtype=torch.int32).cuda()
            active = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()
            fresh = torch.tensor([0, 1, 0], dtype=torch.uint8).cuda()
            n_live = ints(LIVE_SHARDS, 5)
            mask = (torch.tensor([1, 1, 0], dtype=torch.uint8).cuda()
                    if variant == "mask" else None)
            for t in range(T):
                call("mpc_advance_noisy", pp, p(table),
                     p(ref if tracked else None), ADVANCE["ref_len"],
                     ADVANCE["ref_t0"] + t, B, N, T, t, p(z0), p(U), p(Z),
                     p(u_min), p(u_max),
                     p(plant if variant == "plant" else None),
                     p(dist_in if variant == "disturbance" else None),
                     p(w_std if proc else None), p(v_std if obs else None),
                     SEED, ADVANCE["rollout_offset"], ADVANCE["step_offset"],
                     p(x_true), p(Ylog), p(mask), p(Xlog), p(Ulog), p(Jcl),
                     p(state_log), p(live_log), p(mu), p(delta), p(state),
                     p(it), p(active), p(fresh), p(n_live), st)
                wide.append(joint_digests([host(a) for a in (
                    z0, U, Z, Xlog, Ulog, x_true, Ylog)]))
                Jcls.append(host(Jcl))
                words.append(np.concatenate(
                    [host(a).astype(np.float64).ravel() for a in
                     (state_log, live_log, mu, delta, state, it, active,
                      fresh)]))
                shards.append(host(n_live))
                # (the rounds of the next control step leave other words)
                state.copy_(torch.tensor([2, 3, 1], dtype=torch.int32))
                active.copy_(torch.tensor([0, 1, 1], dtype=torch.uint8))
        tag = "advance_N%d/" % N
        R = len(runs)
        out[tag + "wide"] = np.stack(wide).reshape(R, T, B)
        out[tag + "Jcl"] = np.stack(Jcls).reshape(R, T, B)
        out[tag + "words"] = np.stack(words).reshape(R, T, -1)
        out[tag + "n_live"] = np.stack(shards).reshape(R, T, -1)
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
