"""Records what the matrix-core backward sweeps compute at small shapes: the
fixture of tests/test_matrix_sweeps_golden.py, which holds later builds to it
byte for byte.  The sweeps on records (riccati_mfma16.hpp, riccati_mfma32.hpp,
riccati_mfma32s.hpp) go through pddp_riccati_backward_variant_*, the sweep from
the nominal (riccati_mfma16_nominal.hpp) through pddp_sweep_nominal_*.  Record
it from the build the change under test STARTS from (its parent commit), on an
MI355X, never from the code under test:

    python tools/record_sweep_golden.py [tests/golden/matrix_sweeps_parent.npz]

(PDDP_HIP_LIB selects the library, pddp_amd/_native.py.)

Inputs are seeded numpy draws on the host, rounded to the run's dtype.  Every
output buffer holds a sentinel before the launch (gains 7.0, status -5, L
-7.25, J_opt 123.0) and part of `active` (and `fresh`) is off, so the rows a
kernel must not touch are compared too.  `status` (and L, J_opt, fresh of the
nominal cases) is stored whole, `gains` as an 8-byte BLAKE2b digest per
(trajectory, step): equal digests are equal bytes to one part in 2^64, and a
digest that differs still names its trajectory and step.

Records: the well-conditioned family of tests/test_gpu_parity.py's
test_matrix_core_sweeps_with_active_mask_and_ragged_batches, B = 6 with
`active` off where b % 3 == 1 (half-empty workgroups at 4 and at 2
trajectories per workgroup), a regularisation per trajectory, and
  * trajectories 2 and 3 with their nominal action 0.05 inside u_max / u_min
    (the bounds are one pair per launch: the box of k is 0.05 wide on that
    side), so that steps clamp;
  * trajectory 5 with a NaN in L_uu at the middle step;
  * in the unbounded Cholesky cases, trajectory 0 with L_uu = -1e4 there.
N = 1, 2, 3, 7: the ring of three (16 x 16) has tail steps only, one trip,
trips plus a tail; the ring of two (32 x 32) a single step, one pair, an odd
tail.  n = 2, 6, 9, 14 / 15, 23, 27, 30: every DMA count, row n in different
lane groups and registers.

When it records, main() asserts that the parent's own output holds the
statuses PDDP_BWD_OK, _NAN and _NOT_PD and, in the bounded cases, clamped steps
(K row all zero) as well as free ones - the fixture cannot be vacuous.  The
committed fixture's run printed: statuses of live trajectories OK 1072, NAN
224, NOT_PD 160, BOXQP_FAILED 80; bounded steps 702 clamped, 1170 free.  (The
out-of-line BoxQP loop behind the closed form is not a condition; whether these
inputs reach it is not observable from the outputs and was not measured.)"""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "matrix_sweeps_parent.npz")

BWD_OK, BWD_NAN, BWD_NOT_PD = 0, 1, 2
RECORD_B, RECORD_NS = 6, (1, 2, 3, 7)
NOMINAL_B, NOMINAL_NS = 5, (1, 70)  # 70 crosses a generator block of 64/32/16
DT = {"pendulum": 0.1, "double_cartpole": 0.05}
BOUND = {"pendulum": 2.5, "double_cartpole": 20.0}
MEAN0 = {"pendulum": [0, 0], "double_cartpole": [0, 0, np.pi, 0, np.pi, 0]}
REG = np.array([1e-3, 1e-2, 0.1, 1e-3, 1.0, 0.5, 0.25])
GAIN_SENTINEL, STATUS_SENTINEL, L_SENTINEL, J_SENTINEL = 7.0, -5, -7.25, 123.0

# (kind, n or problem, dtype); the variants, branches, bounds and N of a case
# are looped over inside run_case
CASES = ([("m16", n, d) for n in (2, 6, 9, 14) for d in ("f32", "f64")] +
         [("m32", n, "f32") for n in (15, 23, 27, 30)] +
         [("nominal", p, d) for p in ("pendulum", "double_cartpole")
          for d in ("f32", "f64")])


def case_name(kind, what, dtype):
    return "%s_%s_%s" % (kind, what, dtype)


def variants_of(kind, dtype, branch):
    """16 x 16: 14 (IEEE division) and, f32, 15; 32 x 32: the one-wave kernel
    14 / 15 and, on the eig-clamp branch, the two-wavefront split 26 / 27."""
    if kind == "m16":
        return (14, 15) if dtype == "f32" else (14,)
    return (14, 15) + ((26, 27) if branch == 0 else ())


def digests(a, axes):
    """uint64 [a.shape[:axes]]: a digest of the bytes of each trailing block."""
    a = np.ascontiguousarray(a)
    flat = a.reshape(int(np.prod(a.shape[:axes])), -1)
    out = np.array([int.from_bytes(hashlib.blake2b(
        r.tobytes(), digest_size=8).digest(), "little") for r in flat],
        dtype=np.uint64)
    return out.reshape(a.shape[:axes])


def record_inputs(n, N, dtype, negative_Luu=False):
    """The derivative arrays of one records case (numpy, already rounded to
    `dtype`), u_min / u_max and the `active` mask."""
    npd = np.float32 if dtype == "f32" else np.float64
    B, m = RECORD_B, 1
    rng = np.random.RandomState(1000 * n + N)
    r = rng.standard_normal
    eye = np.eye(n)
    R = 0.2 * r((B, N + 1, n, n))
    d = dict(F_z=eye + 0.05 * r((B, N, n, n)), F_u=0.3 * r((B, N, n, m)),
             L_z=r((B, N + 1, n)), L_u=r((B, N, m)),
             L_zz=eye + R @ R.transpose(0, 1, 3, 2),
             L_uz=0.05 * r((B, N, m, n)),
             L_uu=1.0 + 0.04 * r((B, N, m, m)) ** 2, U=0.5 * r((B, N, m)))
    d["U"][2], d["U"][3] = 0.95, -0.95
    mid = N // 2
    d["L_uu"][5, mid] = np.nan
    if negative_Luu:
        d["L_uu"][0, mid] = -1e4
    d = {k: np.ascontiguousarray(v.astype(npd)) for k, v in d.items()}
    d["u_min"], d["u_max"] = -np.ones(m, npd), np.ones(m, npd)
    d["active"] = (np.arange(B) % 3 != 1).astype(np.uint8)
    d["reg"] = REG[:B].copy()
    return d


def run_records(kind, n, dtype, stats):
    import torch
    from pddp_amd import _native as N_
    td = torch.float32 if dtype == "f32" else torch.float64
    B, m = RECORD_B, 1
    lay = N_.record_layout(n, m)
    p, st = N_.ptr, N_.stream_handle()
    dev = lambda a: torch.from_numpy(a).cuda()
    out = {}
    for N in RECORD_NS:
        for branch in (0, 1):
            for bounded in (True, False):
                d = record_inputs(n, N, dtype, branch == 1 and not bounded)
                t = {k: dev(v) for k, v in d.items()}
                rec = torch.full((B, N + 1, lay.stride), L_SENTINEL, dtype=td,
                                 device="cuda")
                N_.call("pddp_pack_records", td, B, N, n, m, p(t["F_z"]),
                        p(t["F_u"]), p(t["L_z"]), p(t["L_u"]), p(t["L_zz"]),
                        p(t["L_uz"]), p(t["L_uu"]), p(t["U"]), p(rec), st)
                for variant in variants_of(kind, dtype, branch):
                    gains = torch.full((B, N, lay.gain_stride), GAIN_SENTINEL,
                                       dtype=td, device="cuda")
                    status = torch.full((B,), STATUS_SENTINEL,
                                        dtype=torch.int32, device="cuda")
                    N_.call("pddp_riccati_backward_variant", td, B, N, n, m,
                            p(rec), p(t["u_min"]) if bounded else None,
                            p(t["u_max"]) if bounded else None, p(t["reg"]),
                            branch, p(t["active"]), p(gains), p(status), st,
                            variant)
                    g, s = gains.cpu().numpy(), status.cpu().numpy()
                    tag = "N%d_branch%d_%s_v%d/" % (
                        N, branch, "bounded" if bounded else "free", variant)
                    out[tag + "status"] = s
                    out[tag + "gains"] = digests(g, 2)
                    if stats is not None:
                        live = d["active"] != 0
                        stats["status"].update(int(x) for x in s[live])
                        if bounded:
                            ok = live & (s == BWD_OK)
                            zero = (g[ok][:, :, m:] == 0).all(axis=-1)
                            stats["clamped"] += int(zero.sum())
                            stats["free"] += int((~zero).sum())
    return out


def run_nominal(problem, dtype, stats):
    import torch
    from pddp_amd import _native as N_
    from pddp_amd.examples.problems import SampleProblems
    from pddp_amd.utils.encoding import StateEncoding
    sp = SampleProblems[problem.upper()]
    prob = sp.get_model_class()(DT[problem]).native_problem(
        StateEncoding.IGNORE_UNCERTAINTY, sp.get_cost_class()())
    td = torch.float32 if dtype == "f32" else torch.float64
    npd = np.float32 if dtype == "f32" else np.float64
    B, n, m = NOMINAL_B, prob.encoded_size, prob.action_size
    GS = m + m * n
    p, st, pp = N_.ptr, N_.stream_handle(), ctypes.addressof(prob)
    bound = BOUND[problem]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    u_min, u_max = dev(np.full(m, -bound, npd)), dev(np.full(m, bound, npd))
    reg = dev(REG[:B].copy())
    active = dev(np.array([1, 0, 1, 1, 1], np.uint8))
    out = {}
    for N in NOMINAL_NS:
        rng = np.random.RandomState(17 + N)
        Z = dev((np.asarray(MEAN0[problem], np.float64) +
                 0.1 * rng.randn(B, N + 1, n)).astype(npd))
        U = dev((0.6 * bound * rng.randn(B, N, m)).astype(npd))
        for branch in (0, 1):
            for bounded in (True, False):
                gains = torch.full((B, N, GS), GAIN_SENTINEL, dtype=td,
                                   device="cuda")
                status = torch.full((B,), STATUS_SENTINEL, dtype=torch.int32,
                                    device="cuda")
                L = torch.full((B, N + 1), L_SENTINEL, dtype=td, device="cuda")
                J = torch.full((B,), J_SENTINEL, dtype=td, device="cuda")
                fresh = dev(np.array([1, 1, 0, 1, 1], np.uint8))
                N_.call("pddp_sweep_nominal", td, pp, B, N, p(Z), p(U),
                        p(u_min) if bounded else None,
                        p(u_max) if bounded else None, p(reg), branch,
                        p(active), p(fresh), p(gains), p(status), p(L), p(J),
                        st)
                tag = "N%d_branch%d_%s/" % (N, branch,
                                            "bounded" if bounded else "free")
                out[tag + "status"] = status.cpu().numpy()
                out[tag + "gains"] = digests(gains.cpu().numpy(), 2)
                out[tag + "L"] = L.cpu().numpy()
                out[tag + "J_opt"] = J.cpu().numpy()
                out[tag + "fresh"] = fresh.cpu().numpy()
    return out


def run_case(kind, what, dtype, stats=None):
    """{name: array as stored} of one case."""
    if kind == "nominal":
        return run_nominal(what, dtype, stats)
    return run_records(kind, what, dtype, stats)


def main():
    import collections
    out = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    stats = dict(status=collections.Counter(), clamped=0, free=0)
    blob = {}
    for case in CASES:
        for k, v in run_case(*case, stats=stats).items():
            blob[case_name(*case) + "/" + k] = v
    print("statuses of live trajectories %r, bounded steps: %d clamped, %d "
          "free" % (dict(stats["status"]), stats["clamped"], stats["free"]))
    assert all(stats["status"][s] > 0 for s in (BWD_OK, BWD_NAN, BWD_NOT_PD))
    assert stats["clamped"] > 0 and stats["free"] > 0
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **blob)
    print("%d cases, %d arrays, %d bytes -> %s" % (
        len(CASES), len(blob), os.path.getsize(out), out))


if __name__ == "__main__":
    main()
