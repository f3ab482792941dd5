"""Records what the reference-tracking kernels compute under a MOVING reference
(pddp_derivs_track_*, pddp_line_search_track_*, pddp_mpc_advance_track_*) and
what the untracked hand-over (pddp_mpc_advance_*) computes, at small shapes:
the fixture of tests/test_track_kernels_golden.py, which holds later builds to
it byte for byte.  Record it from the build the change under test STARTS from
(its parent commit), on an MI355X, never from the code under test:

    python tools/record_track_golden.py [tests/golden/track_kernels_parent.npz]

(PDDP_HIP_LIB selects the library, pddp_amd/_native.py.)

As in tools/record_problem_golden.py, whose helpers this tool uses: every
output buffer holds a sentinel before the launch and part of every mask is
switched off, the inputs of the three operations are independent draws, and the
wide arrays are stored as 8-byte BLAKE2b digests - the records one per
(trajectory, time step), Zc and Uc one each per trajectory, and of the
hand-over z0, U, Z, Xlog and Ulog one each per trajectory after every control
step.  L (with J), state, Jc, Jcl and the controller words are stored whole."""
import ctypes
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

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "track_kernels_parent.npz")

CASES = [(p, d, bd, tb) for p in base.PROBLEMS for d in ("f32", "f64")
         for bd in (True, False) for tb in (True, False)]

# Records, 64 time steps per chunk: N = 70 is a second chunk with a ragged
# tail; of the reference's 9 rows the horizon starts at row 2, so steps 6 .. 70
# sit on the held last row.  Line search, one lane per (trajectory, step size):
# neither A divides 64, a wavefront straddles trajectories; the reference runs
# out at step 2 of 6.  Hand-over, one lane per trajectory: T = 3 control steps
# in sequence (the last takes the terminal row), N = 1 is the shift's clamps
# alone; the reference of length 4 is held from control step 2 on.
RECORDS = dict(B=3, N=70, ref_len=9, ref_t0=2)
SEARCH = dict(B=3, N=6, As=(3, 11), ref_len=4, ref_t0=1)
ADVANCE = dict(B=3, Ns=(1, 6), T=3, ref_len=4, ref_t0=1,
               variants=("plain", "plant", "disturbance", "mask"))
SENTINEL, STATE_SENTINEL = base.SENTINEL, base.STATE_SENTINEL
LIVE_SHARDS = 256  # PDDP_LIVE_SHARDS (include/pddp_hip.h)


def case_name(problem, dtype, bounded, table):
    return "%s_%s_%s_%s" % (problem, dtype, "bounded" if bounded else "free",
                            "table" if table else "shared")


def reference_of(prob, B, ref_len, seed, td):
    """[B][ref_len][REF_ROW]: the problem's goals + U(-0.5, 0.5) and
    u_goal + U(-0.2, 0.2), another draw in every row, rounded to float32."""
    import torch
    from pddp_amd import _native as N_
    rng = np.random.RandomState(seed)
    na, m = prob.aug_size, prob.action_size
    ref = np.zeros((B, ref_len, N_.REF_ROW))
    ref[..., N_.REF_X_GOAL:N_.REF_X_GOAL + na] = \
        np.asarray(list(prob.x_goal)[:na]) + rng.uniform(-0.5, 0.5,
                                                         (B, ref_len, na))
    ref[..., N_.REF_U_GOAL:N_.REF_U_GOAL + m] = \
        np.asarray(list(prob.u_goal)[:m]) + rng.uniform(-0.2, 0.2,
                                                        (B, ref_len, m))
    ref = ref.astype(np.float32).astype(np.float64)
    return torch.from_numpy(ref).to(td).cuda().contiguous()


def run_case(problem, dtype, bounded, with_table):
    """{name: array as stored} of one (model, dtype, bounds, table)."""
    import torch
    from pddp_amd import _native as N_
    from pddp_amd.examples.problems import SampleProblems
    from pddp_amd.utils.encoding import StateEncoding
    sp = SampleProblems[problem.upper()]
    prob = sp.get_model_class()(base.DT[problem]).native_problem(
        StateEncoding.IGNORE_UNCERTAINTY, sp.get_cost_class()())
    td = torch.float32 if dtype == "f32" else torch.float64
    n, m = prob.encoded_size, prob.action_size
    S = N_.record_layout(n, m).stride
    GS = m + m * n
    lib, p, pp = N_.lib(), N_.ptr, ctypes.addressof(prob)
    st = N_.stream_handle()
    rng = np.random.RandomState(11)
    bound = base.BOUND[problem]
    u_min = torch.full((m,), -bound, dtype=td).cuda() if bounded else None
    u_max = torch.full((m,), bound, dtype=td).cuda() if bounded else None
    digests = base.digests

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(td).cuda()

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
        N_.check(fn(pp, *args), fn.__name__)

    def host(t):  # (waits for the stream)
        return t.detach().cpu().numpy()

    out = {}

    # -- derivative records -----------------------------------------------------
    B, N = RECORDS["B"], RECORDS["N"]
    table = table_of(B, 41) if with_table else None
    ref = reference_of(prob, B, RECORDS["ref_len"], 42, td)
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()
    Z, U = states(B, N + 1), actions(B, N)
    rec, L, J = full(B, N + 1, S), full(B, N + 1), full(B)
    state = ints(B, STATE_SENTINEL)
    call("derivs_track", p(table), p(ref), RECORDS["ref_len"],
         RECORDS["ref_t0"], B, N, p(Z), p(U), p(u_min), p(u_max), p(mask),
         p(rec), p(L), p(J), p(state), st)
    out["records/rec"] = digests(host(rec), 2)
    out["records/L_J"] = np.concatenate([host(L), host(J)[:, None]], axis=1)
    out["records/state"] = host(state)

    # -- line search --------------------------------------------------------------
    B, N = SEARCH["B"], SEARCH["N"]
    table = table_of(B, 43) if with_table else None
    ref = reference_of(prob, B, SEARCH["ref_len"], 44, td)
    active = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()
    bwd_status = torch.tensor([0, 0, 2], dtype=torch.int32).cuda()
    Z, U = states(B, N + 1), actions(B, N)
    gains = dev(0.1 * rng.randn(B, N, GS))
    for A in SEARCH["As"]:
        alphas = dev(np.linspace(1.0, 0.01, A))
        Zc, Uc, Jc = full(B, N + 1, A, n), full(B, N, A, m), full(B, A)
        call("line_search_track", p(table), p(ref), SEARCH["ref_len"],
             SEARCH["ref_t0"], B, N, A, p(Z), p(U), p(gains), p(alphas),
             p(u_min), p(u_max), p(active), p(bwd_status), p(Zc), p(Uc), p(Jc),
             st)
        out["search_A%d/Jc" % A] = host(Jc)
        out["search_A%d/Zc_Uc" % A] = np.stack(
            [digests(host(Zc), 1), digests(host(Uc), 1)], axis=1)

    # -- the MPC hand-over, tracked and untracked -----------------------------------
    B, T = ADVANCE["B"], ADVANCE["T"]
    table = table_of(B, 45) if with_table else None
    plant = table_of(B, 46)
    ref = reference_of(prob, B, ADVANCE["ref_len"], 47, td)
    for N in ADVANCE["Ns"]:
        z0_in, U_in = states(B), actions(B, N)
        dist_in = dev(0.01 * rng.randn(B, T, n))
        for tracked in (True, False):
            wide, Jcls, words = [], [], []
            for variant in ADVANCE["variants"]:
                z0, U, Z = z0_in.clone(), U_in.clone(), full(B, N + 1, n)
                Xlog, Ulog, Jcl = full(B, T + 1, n), full(B, T, m), full(B)
                state_log = torch.full((B, T), STATE_SENTINEL,
                                       dtype=torch.int32, device="cuda")
                live_log = torch.full((B, T), 9, dtype=torch.uint8,
                                      device="cuda")
                # the controller as some rounds left it
                mu = torch.tensor([0.5, 2.0, 8.0], dtype=torch.float64).cuda()
                delta = torch.tensor([1.0, 4.0, 0.25],
                                     dtype=torch.float64).cuda()
                state = torch.tensor([3, 1, 2], dtype=torch.int32).cuda()
                it = torch.tensor([4, 7, 2], dtype=torch.int32).cuda()
                active = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()
                fresh = torch.tensor([0, 1, 0], dtype=torch.uint8).cuda()
                n_live = ints(LIVE_SHARDS, 5)
                mask = (torch.tensor([1, 1, 0], dtype=torch.uint8).cuda()
                        if variant == "mask" else None)
                for t in range(T):
                    tail = (B, N, T, t, p(z0), p(U), p(Z), p(u_min), p(u_max),
                            p(plant if variant == "plant" else None),
                            p(dist_in if variant == "disturbance" else None),
                            p(mask), p(Xlog), p(Ulog), p(Jcl), p(state_log),
                            p(live_log), p(mu), p(delta), p(state), p(it),
                            p(active), p(fresh), p(n_live), st)
                    if tracked:
                        call("mpc_advance_track", p(table), p(ref),
                             ADVANCE["ref_len"], ADVANCE["ref_t0"] + t, *tail)
                    else:
                        call("mpc_advance", p(table), *tail)
                    wide.append(np.stack([digests(host(x), 1) for x in
                                          (z0, U, Z, Xlog, Ulog)]))
                    Jcls.append(host(Jcl))
                    words.append(np.concatenate(
                        [host(x).astype(np.float64).ravel() for x in
                         (state_log, live_log, mu, delta, state, it, active,
                          fresh, n_live)]))
                    # (the rounds of the next control step leave other words)
                    state.copy_(torch.tensor([2, 3, 1], dtype=torch.int32))
                    active.copy_(torch.tensor([0, 1, 1], dtype=torch.uint8))
            tag = "advance_%s_N%d/" % ("track" if tracked else "plain", N)
            V = len(ADVANCE["variants"])
            out[tag + "wide"] = np.stack(wide).reshape(V, T, 5, B)
            out[tag + "Jcl"] = np.stack(Jcls).reshape(V, T, B)
            out[tag + "words"] = np.stack(words).reshape(V, T, -1)
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
