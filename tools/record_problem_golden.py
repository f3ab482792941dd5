"""Records what the nominal rollout, the derivative records and the plain line
search compute at small shapes, in their uniform form (pddp_nominal_rollout_*,
pddp_derivs_*, pddp_line_search_*) and with a per-trajectory table (the
pddp_*_batch_* entry points): the fixture of
tests/test_problem_kernels_golden.py, which holds later builds to it byte for
byte.  Record it from the build the change under test STARTS from (its parent
commit), on an MI355X, never from the code under test:

    python tools/record_problem_golden.py [tests/golden/problem_kernels_parent.npz]

(PDDP_HIP_LIB selects the library, pddp_amd/_native.py.)

Every output buffer holds a sentinel before the launch and part of every mask
is switched off, so the rows a kernel must not touch are compared too.  The
inputs of the three operations are independent draws (the records and the
search do not read the rollout's result): a difference names its kernel.

What is stored: L (with J as one more column), state and Jc whole; the wide
arrays as 8-byte BLAKE2b digests of their bytes - Z one per trajectory, Zc and
Uc one each per trajectory (two columns), the records one per (trajectory, time
step).  Whole, the records and candidates of the 16 cases are several MB of
incompressible floats; equal digests are equal bytes to one part in 2^64, and a
digest that differs still names its trajectory (and step)."""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden",
                           "problem_kernels_parent.npz")

PROBLEMS = ("cartpole", "pendulum", "double_cartpole", "rendezvous")
DT = {"cartpole": 0.1, "pendulum": 0.1, "double_cartpole": 0.05,
      "rendezvous": 0.1}
BOUND = {"cartpole": 10.0, "pendulum": 2.5, "double_cartpole": 20.0,
         "rendezvous": 5.0}
MEAN0 = {"cartpole": [0, 0, 0, 0], "pendulum": [0, 0],
         "double_cartpole": [0, 0, np.pi, 0, np.pi, 0],
         "rendezvous": [-10, -10, 10, 10, 0, -5, 5, 0]}
PARAM_COUNT = {"cartpole": 6, "pendulum": 5, "double_cartpole": 8,
               "rendezvous": 3}  # dt included (include/pddp_problem.h)
CASES = [(p, d, bd) for p in PROBLEMS for d in ("f32", "f64")
         for bd in (True, False)]

# Rollout, one lane per trajectory in workgroups of 64: a second workgroup
# with one lane.  Records, 64 time steps per chunk and a terminal record: one
# partial chunk, exactly one chunk, a second chunk with the terminal record
# alone.  Plain search, one lane per (trajectory, step size): 119 lanes leave a
# ragged second workgroup, and the uniform entry point reaches the plain
# kernel only above 16 step sizes; N = 1 is the prefetch's clamp alone.
ROLLOUT = dict(B=65, Ns=(1, 5))
RECORDS = dict(B=3, Ns=(3, 63, 64))
SEARCH = dict(B=7, Ns=(1, 5), A_uniform=(17,), A_batch=(17, 10))
SENTINEL, STATE_SENTINEL = -7.25, -77


def case_name(problem, dtype, bounded):
    return "%s_%s_%s" % (problem, dtype, "bounded" if bounded else "free")


def digests(a, axes):
    """uint64 [a.shape[:axes]]: a digest of the bytes of each trailing block."""
    a = np.ascontiguousarray(a)
    flat = a.reshape(int(np.prod(a.shape[:axes])), -1)
    out = np.array([int.from_bytes(hashlib.blake2b(
        r.tobytes(), digest_size=8).digest(), "little") for r in flat],
        dtype=np.uint64)
    return out.reshape(a.shape[:axes])


def table_of(prob, problem, B, seed, td):
    """tests/solver_util.py's perturbed(): parameters x U(0.8, 1.2),
    dt x U(0.9, 1.1), goals + U(-0.5, 0.5), u_goal + U(-0.2, 0.2), rounded to
    float32, over rows of the shared problem."""
    import torch
    from pddp_amd import _native as N_
    rng = np.random.RandomState(seed)
    P, na, m = PARAM_COUNT[problem], prob.aug_size, prob.action_size
    row = np.zeros(N_.BATCH_ROW)
    row[N_.BATCH_PARAMS:N_.BATCH_PARAMS + N_.MAX_PARAMS] = list(prob.params)
    row[N_.BATCH_X_GOAL:N_.BATCH_X_GOAL + N_.MAX_AUG] = list(prob.x_goal)
    row[N_.BATCH_U_GOAL:N_.BATCH_U_GOAL + N_.MAX_ACTION] = list(prob.u_goal)
    t = np.tile(row, (B, 1))
    t[:, N_.BATCH_PARAMS] *= rng.uniform(0.9, 1.1, B)
    t[:, N_.BATCH_PARAMS + 1:N_.BATCH_PARAMS + P] *= \
        rng.uniform(0.8, 1.2, (B, P - 1))
    t[:, N_.BATCH_X_GOAL:N_.BATCH_X_GOAL + na] += rng.uniform(-0.5, 0.5,
                                                               (B, na))
    t[:, N_.BATCH_U_GOAL:N_.BATCH_U_GOAL + m] += rng.uniform(-0.2, 0.2, (B, m))
    t = t.astype(np.float32).astype(np.float64)
    return torch.from_numpy(t).to(td).cuda().contiguous()


def run_case(problem, dtype, bounded):
    """{name: array as stored} of one (model, dtype, bounds): the three
    operations in both forms at every shape above."""
    import torch
    from pddp_amd import _native as N_
    from pddp_amd.examples.problems import SampleProblems
    from pddp_amd.utils.encoding import StateEncoding
    sp = SampleProblems[problem.upper()]
    prob = sp.get_model_class()(DT[problem]).native_problem(
        StateEncoding.IGNORE_UNCERTAINTY, sp.get_cost_class()())
    td = torch.float32 if dtype == "f32" else torch.float64
    n, m = prob.encoded_size, prob.action_size
    S = N_.record_layout(n, m).stride
    GS = m + m * n
    lib, p, pp = N_.lib(), N_.ptr, ctypes.addressof(prob)
    st = N_.stream_handle()
    rng = np.random.RandomState(7)
    bound = BOUND[problem]
    u_min = torch.full((m,), -bound, dtype=td).cuda() if bounded else None
    u_max = torch.full((m,), bound, dtype=td).cuda() if bounded else None

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(td).cuda()

    def full(*shape):
        return torch.full(shape, SENTINEL, dtype=td, device="cuda")

    def states(*shape):  # nominal states around the model's starting point
        return dev(np.asarray(MEAN0[problem], np.float64) +
                   0.1 * rng.randn(*shape, n))

    def actions(*shape):  # (a tenth of them beyond the bounds)
        return dev(0.6 * bound * rng.randn(*shape, m))

    def call(name, form, table, *args):
        fn = getattr(lib, "pddp_%s%s_%s" % (name, "_batch" if form == "batch"
                                            else "", dtype))
        head = (pp, p(table)) if form == "batch" else (pp,)
        N_.check(fn(*head, *args), fn.__name__)

    out = {}

    def host(t):  # (waits for the stream)
        return t.detach().cpu().numpy()

    def keep(tag, **arrays):
        for k, v in arrays.items():
            out[tag + "/" + k] = v

    # -- nominal rollout ------------------------------------------------------
    B = ROLLOUT["B"]
    table = table_of(prob, problem, B, 31, td)
    mask = torch.ones(B, dtype=torch.uint8)
    mask[1::4] = 0  # (the second workgroup's one lane, b = 64, stays on)
    mask = mask.cuda()
    for N in ROLLOUT["Ns"]:
        z0, U = states(B), actions(B, N)
        for form in ("uniform", "batch"):
            Z = full(B, N + 1, n)
            call("nominal_rollout", form, table, B, N, p(z0), p(U), p(u_min),
                 p(u_max), p(mask), p(Z), st)
            keep("rollout_%s_N%d" % (form, N), Z=digests(host(Z), 1))

    # -- derivative records -----------------------------------------------------
    B = RECORDS["B"]
    table = table_of(prob, problem, B, 32, td)
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()
    for N in RECORDS["Ns"]:
        Z, U = states(B, N + 1), actions(B, N)
        for form in ("uniform", "batch"):
            rec, L, J = full(B, N + 1, S), full(B, N + 1), full(B)
            state = torch.full((B,), STATE_SENTINEL, dtype=torch.int32,
                               device="cuda")
            call("derivs", form, table, B, N, p(Z), p(U), p(u_min), p(u_max),
                 p(mask), p(rec), p(L), p(J), p(state), st)
            keep("records_%s_N%d" % (form, N), rec=digests(host(rec), 2),
                 L_J=np.concatenate([host(L), host(J)[:, None]], axis=1),
                 state=host(state))

    # -- plain line search --------------------------------------------------------
    B = SEARCH["B"]
    table = table_of(prob, problem, B, 33, td)
    active = torch.ones(B, dtype=torch.uint8)
    active[2] = 0
    active = active.cuda()
    bwd_status = torch.zeros(B, dtype=torch.int32)
    bwd_status[4] = 2
    bwd_status = bwd_status.cuda()
    for N in SEARCH["Ns"]:
        Z, U = states(B, N + 1), actions(B, N)
        gains = dev(0.1 * rng.randn(B, N, GS))
        for form in ("uniform", "batch"):
            for A in SEARCH["A_" + form]:
                alphas = dev(np.linspace(1.0, 0.01, A))
                Zc, Uc = full(B, N + 1, A, n), full(B, N, A, m)
                Jc = full(B, A)
                call("line_search", form, table, B, N, A, p(Z), p(U), p(gains),
                     p(alphas), p(u_min), p(u_max), p(active), p(bwd_status),
                     p(Zc), p(Uc), p(Jc), st)
                keep("search_%s_N%d_A%d" % (form, N, A), Jc=host(Jc),
                     Zc_Uc=np.stack([digests(host(Zc), 1),
                                     digests(host(Uc), 1)], axis=1))
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
