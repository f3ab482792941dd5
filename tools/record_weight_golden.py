"""Records what the derivative records and the line search compute under
per-trajectory cost weights, with one goal per trajectory and along a MOVING
reference (pddp_derivs_weighted_*, pddp_line_search_weighted_*,
pddp_derivs_track_weighted_*, pddp_line_search_track_weighted_*), at small
shapes: the fixture of tests/test_weight_kernels_golden.py, which holds later
builds to it byte for byte.  Record it from the build the change under test
STARTS from (its parent commit), on an MI355X, never from the code under test:

    python tools/record_weight_golden.py [tests/golden/weight_kernels_parent.npz]

(PDDP_HIP_LIB selects the library, pddp_amd/_native.py.)

The cases, the shapes, the masks and the references are
tools/record_track_golden.py's (its CASES, RECORDS and SEARCH; the table, where
a case has one, gives the parameters and - without a reference - the goals),
the helpers that tool's and tools/record_problem_golden.py's: every output
buffer holds a sentinel before the launch, one trajectory is masked off and one
has a non-zero bwd_status, the inputs are rounded through float32, and the wide
arrays are stored as 8-byte BLAKE2b digests - the records one per (trajectory,
time step), Zc and Uc one each per trajectory.  L (with J), state and Jc are
stored whole.

The weights are per trajectory: the shared diagonals of Q, Q_term and R times
a draw in [0.5, 2].  In trajectories 0 and 2 every entry of Q whose SHARED
diagonal is zero (the cartpole's x' and sin, the double cartpole's x' and both
sines; the pendulum and the rendezvous have none) carries a positive weight as
well: the case for which these kernels evaluate the cost under the full mask.
Trajectory 0 is live in both operations."""
import ctypes
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
base = track.base

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden",
                           "weight_kernels_parent.npz")

CASES, case_name = track.CASES, track.case_name
RECORDS, SEARCH = track.RECORDS, track.SEARCH
FORMS = ("weighted", "track_weighted")
LIVE_ROWS = (0, 2)  # trajectories with weights where the shared Q has none
SENTINEL, STATE_SENTINEL = base.SENTINEL, base.STATE_SENTINEL


def weights_of(prob, B, seed, td):
    """[B][WEIGHT_ROW]: the shared diagonals of Q, Q_term, R x U(0.5, 2); in
    LIVE_ROWS a draw of U(0.5, 2) itself where the shared diagonal of Q is
    zero; rounded to float32."""
    import torch
    from pddp_amd import _native as N_
    rng = np.random.RandomState(seed)
    na, m = prob.aug_size, prob.action_size
    w = np.zeros((B, N_.WEIGHT_ROW))
    for off, mat, ld, k in ((N_.WEIGHT_Q, prob.Q, N_.MAX_AUG, na),
                            (N_.WEIGHT_Q_TERM, prob.Q_term, N_.MAX_AUG, na),
                            (N_.WEIGHT_R, prob.R, N_.MAX_ACTION, m)):
        diag = np.array([mat[i * ld + i] for i in range(k)])
        draw = rng.uniform(0.5, 2.0, (B, k))
        w[:, off:off + k] = diag * draw
        if off == N_.WEIGHT_Q:
            for b in LIVE_ROWS:
                w[b, off:off + k][diag == 0.0] = draw[b][diag == 0.0]
    w = w.astype(np.float32).astype(np.float64)
    return torch.from_numpy(w).to(td).cuda().contiguous()


def run_case(problem, dtype, bounded, with_table):
    """{name: array as stored} of one (model, dtype, bounds, table): both
    operations in both forms."""
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
    rng = np.random.RandomState(13)
    bound = base.BOUND[problem]
    u_min = torch.full((m,), -bound, dtype=td).cuda() if bounded else None
    u_max = torch.full((m,), bound, dtype=td).cuda() if bounded else None
    digests = base.digests

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(td).cuda()

    def full(*shape):
        return torch.full(shape, SENTINEL, dtype=td, device="cuda")

    def states(*shape):
        return dev(np.asarray(base.MEAN0[problem], np.float64) +
                   0.1 * rng.randn(*shape, n))

    def actions(*shape):  # (a tenth of them beyond the bounds)
        return dev(0.6 * bound * rng.randn(*shape, m))

    def call(name, form, table, ref, shape, weights, *args):
        """pddp_<name>_<form>_<dtype>: the table, the window if the form
        tracks, the weights, then the operation's own list."""
        fn = getattr(lib, "pddp_%s_%s_%s" % (name, form, dtype))
        window = (p(ref), shape["ref_len"], shape["ref_t0"]) \
            if form == "track_weighted" else ()
        N_.check(fn(pp, p(table), *window, p(weights), *args), fn.__name__)

    def host(t):  # (waits for the stream)
        return t.detach().cpu().numpy()

    out = {}

    # -- derivative records -----------------------------------------------------
    B, N = RECORDS["B"], RECORDS["N"]
    table = base.table_of(prob, problem, B, 51, td) if with_table else None
    ref = track.reference_of(prob, B, RECORDS["ref_len"], 52, td)
    weights = weights_of(prob, B, 53, td)
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()
    Z, U = states(B, N + 1), actions(B, N)
    for form in FORMS:
        rec, L, J = full(B, N + 1, S), full(B, N + 1), full(B)
        state = torch.full((B,), STATE_SENTINEL, dtype=torch.int32,
                           device="cuda")
        call("derivs", form, table, ref, RECORDS, weights, B, N, p(Z), p(U),
             p(u_min), p(u_max), p(mask), p(rec), p(L), p(J), p(state), st)
        tag = "%s/records/" % form
        out[tag + "rec"] = digests(host(rec), 2)
        out[tag + "L_J"] = np.concatenate([host(L), host(J)[:, None]], axis=1)
        out[tag + "state"] = host(state)

    # -- line search --------------------------------------------------------------
    B, N = SEARCH["B"], SEARCH["N"]
    table = base.table_of(prob, problem, B, 54, td) if with_table else None
    ref = track.reference_of(prob, B, SEARCH["ref_len"], 55, td)
    weights = weights_of(prob, B, 56, td)
    active = torch.tensor([1, 0, 1], dtype=torch.uint8).cuda()
    bwd_status = torch.tensor([0, 0, 2], dtype=torch.int32).cuda()
    Z, U = states(B, N + 1), actions(B, N)
    gains = dev(0.1 * rng.randn(B, N, GS))
    for A in SEARCH["As"]:
        alphas = dev(np.linspace(1.0, 0.01, A))
        for form in FORMS:
            Zc, Uc, Jc = full(B, N + 1, A, n), full(B, N, A, m), full(B, A)
            call("line_search", form, table, ref, SEARCH, weights, B, N, A,
                 p(Z), p(U), p(gains), p(alphas), p(u_min), p(u_max),
                 p(active), p(bwd_status), p(Zc), p(Uc), p(Jc), st)
            tag = "%s/search_A%d/" % (form, A)
            out[tag + "Jc"] = host(Jc)
            out[tag + "Zc_Uc"] = np.stack(
                [digests(host(Zc), 1), digests(host(Uc), 1)], axis=1)
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
