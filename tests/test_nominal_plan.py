"""The launch plan of the cartpole's nominal path, row by row.

`pddp_n4_nominal_plan` (a host function: no GPU needed) answers what a launch
of pddp_sweep_nominal_f32 / _f64 (rounds = 0) or pddp_round_nominal_f32
(rounds != 0) looks like - csrc/riccati_n4_elem.hpp `n4_nominal_plan`, from
which every such launch is made.

TABLE was written by reading the six launchers of commit 81306cb
("Matrix-core sweeps: one gain block ..."), the last one in which
launch_n4_elem / _f64, launch_n4_branches / _f64, launch_round_n4 and
launch_round_n4_branches each decided their launch themselves - not by calling
the function under test.  A row is
(branch, sparse, overlap, multi, carry, grid, threads, LDS bytes), or the
error the entry point returns before it launches.  The sizes behind the LDS
column (riccati_n4_elem.hpp): a block's images kImgBuf = 4 (16 * 52 + 16) =
3392 words per wavefront, inline; 2 * 3392 + 96 = 6880 per (sweep, generator)
pair; the round adds 24 N words of gain rows and, several rounds per launch
where it fits 159 KB, 340 carried words; four wavefronts (pairs) per
workgroup."""
import ctypes

import pytest

from pddp_amd import _native
from pddp_amd.utils.encoding import StateEncoding

BADARG, UNSUPPORTED = -1, -2
EIG, CHOL = 0, 1                       # PDDP_BRANCH_*
EIG_BOX, EIG_FREE, CHOL_FREE, CHOL_BOX = 0, 1, 2, 3   # n4e::kBr*
INL32, OVL32, INL64 = 16 * 3392, 16 * 6880, 32 * 3392  # 54272, 110080, 108544


def _round_lds(N, carry):
    return 16 * (6880 + 24 * N + (340 if carry else 0))


assert _round_lds(123, True) == 162752 <= 159 * 1024 < _round_lds(124, True)
assert _round_lds(124, False) == 157696 and _round_lds(127, False) == 158848


def _problem(kind):
    import pddp_amd.examples  # noqa: F401
    name, _, what = kind.partition(":")
    mod = getattr(pddp_amd.examples, name)
    model = [getattr(mod, k) for k in dir(mod) if
             k.endswith("DynamicsModel") and k != "DynamicsModel"][0]
    cost = [getattr(mod, k) for k in dir(mod)
            if k.endswith("Cost") and k != "AugmentedQRCost"][0]
    enc = StateEncoding.VARIANCE_ONLY if what == "gaussian" else \
        StateEncoding.IGNORE_UNCERTAINTY
    p = model(0.1).native_problem(enc, cost())
    if what == "fullQ":  # an entry outside {x, sin, cos}: the pole's rate
        p.Q[2 * _native.MAX_AUG + 2] = 0.5
    return p


def _args(problem="cartpole", es=4, B=4096, N=100, A=16, lo=1, hi=1,
          branch=EIG, rounds=0, choice=0):
    return problem, es, B, N, A, lo, hi, branch, rounds, choice


# case -> (arguments, expected)
TABLE = {
    # ---- the sweep alone, f32: gain branches, cost mask
    "sweep-eig-box": (_args(), (EIG_BOX, 1, 1, 0, 0, 256, 512, OVL32)),
    "sweep-eig-free": (_args(lo=0, hi=0),
                       (EIG_FREE, 1, 1, 0, 0, 256, 512, OVL32)),
    "sweep-chol-free": (_args(lo=0, hi=0, branch=CHOL),
                        (CHOL_FREE, 1, 1, 0, 0, 256, 512, OVL32)),
    "sweep-chol-box": (_args(branch=CHOL),
                       (CHOL_BOX, 1, 1, 0, 0, 256, 512, OVL32)),
    "sweep-lower-bound-only": (_args(hi=0), UNSUPPORTED),
    "sweep-upper-bound-only": (_args(lo=0, branch=CHOL), UNSUPPORTED),
    "sweep-fullQ": (_args("cartpole:fullQ"),
                    (EIG_BOX, 0, 1, 0, 0, 256, 512, OVL32)),
    "sweep-fullQ-chol-free": (_args("cartpole:fullQ", lo=0, hi=0, branch=CHOL),
                              (CHOL_FREE, 0, 1, 0, 0, 256, 512, OVL32)),
    # ---- batch: sixteen trajectories per workgroup; beyond 256 workgroups the
    # generator goes inline by itself
    "sweep-B16": (_args(B=16), (EIG_BOX, 1, 1, 0, 0, 1, 512, OVL32)),
    "sweep-B17": (_args(B=17), (EIG_BOX, 1, 1, 0, 0, 2, 512, OVL32)),
    "sweep-B4097": (_args(B=4097), (EIG_BOX, 1, 0, 0, 0, 257, 256, INL32)),
    "sweep-B4097-chol-box": (_args(B=4097, branch=CHOL),
                             (CHOL_BOX, 1, 0, 0, 0, 257, 256, INL32)),
    # ---- generator choice (pddp_sweep_nominal_kernel)
    "sweep-choice3": (_args(choice=3), (EIG_BOX, 1, 0, 0, 0, 256, 256, INL32)),
    "sweep-choice4": (_args(choice=4), (EIG_BOX, 1, 1, 0, 0, 256, 512, OVL32)),
    "sweep-choice4-B4097": (_args(B=4097, choice=4),
                            (EIG_BOX, 1, 1, 0, 0, 257, 512, OVL32)),
    "sweep-choice3-eig-free-B16": (_args(B=16, lo=0, hi=0, choice=3),
                                   (EIG_FREE, 1, 0, 0, 0, 1, 256, INL32)),
    # ---- horizon: the sweep alone takes any
    "sweep-N1": (_args(N=1), (EIG_BOX, 1, 1, 0, 0, 256, 512, OVL32)),
    "sweep-N128": (_args(N=128), (EIG_BOX, 1, 1, 0, 0, 256, 512, OVL32)),
    # ---- f64: always inline, 106 KB
    "sweep64": (_args(es=8), (EIG_BOX, 1, 0, 0, 0, 256, 256, INL64)),
    "sweep64-choice4": (_args(es=8, choice=4),
                        (EIG_BOX, 1, 0, 0, 0, 256, 256, INL64)),
    "sweep64-B4097-fullQ-chol-box": (
        _args("cartpole:fullQ", es=8, B=4097, branch=CHOL),
        (CHOL_BOX, 0, 0, 0, 0, 257, 256, INL64)),
    "sweep64-eig-free-B17": (_args(es=8, B=17, lo=0, hi=0),
                             (EIG_FREE, 1, 0, 0, 0, 2, 256, INL64)),
    "sweep64-one-bound": (_args(es=8, lo=0), UNSUPPORTED),
    # ---- the round: branches, mask, rounds per launch
    "round1-eig-box": (_args(rounds=1), (EIG_BOX, 1, 1, 0, 0, 256, 512,
                                         _round_lds(100, False))),
    "round3-eig-box": (_args(rounds=3), (EIG_BOX, 1, 1, 1, 1, 256, 512,
                                         _round_lds(100, True))),
    "round1-eig-free": (_args(rounds=1, lo=0, hi=0),
                        (EIG_FREE, 1, 1, 0, 0, 256, 512,
                         _round_lds(100, False))),
    "round3-chol-free-fullQ": (
        _args("cartpole:fullQ", rounds=3, lo=0, hi=0, branch=CHOL),
        (CHOL_FREE, 0, 1, 1, 1, 256, 512, _round_lds(100, True))),
    "round1-chol-box-B17": (_args(rounds=1, branch=CHOL, B=17),
                            (CHOL_BOX, 1, 1, 0, 0, 2, 512,
                             _round_lds(100, False))),
    "round1-fullQ-B16": (_args("cartpole:fullQ", rounds=1, B=16),
                         (EIG_BOX, 0, 1, 0, 0, 1, 512,
                          _round_lds(100, False))),
    "round1-one-bound": (_args(rounds=1, hi=0), UNSUPPORTED),
    # (the round has no inline form: the sweep's knob is not looked at)
    "round1-choice3": (_args(rounds=1, choice=3),
                       (EIG_BOX, 1, 1, 0, 0, 256, 512,
                        _round_lds(100, False))),
    # ---- the round's refusals
    "round1-B4097": (_args(rounds=1, B=4097), UNSUPPORTED),
    "round3-B4097-chol-free": (_args(rounds=3, B=4097, lo=0, hi=0,
                                     branch=CHOL), UNSUPPORTED),
    "round1-A17": (_args(rounds=1, A=17), UNSUPPORTED),
    "round1-A17-eig-free": (_args(rounds=1, A=17, lo=0, hi=0), UNSUPPORTED),
    "round1-N128": (_args(rounds=1, N=128), UNSUPPORTED),
    "round3-N128-chol-box": (_args(rounds=3, N=128, branch=CHOL), UNSUPPORTED),
    "round-negative-rounds": (_args(rounds=-1), UNSUPPORTED),
    "round1-f64": (_args(es=8, rounds=1), UNSUPPORTED),
    "round3-f64-eig-free": (_args(es=8, rounds=3, lo=0, hi=0), UNSUPPORTED),
    # ---- the round's horizon: carry up to N = 123, served up to N = 127
    "round1-N1": (_args(rounds=1, N=1), (EIG_BOX, 1, 1, 0, 0, 256, 512,
                                         _round_lds(1, False))),
    "round3-N1": (_args(rounds=3, N=1), (EIG_BOX, 1, 1, 1, 1, 256, 512,
                                         _round_lds(1, True))),
    "round1-N123": (_args(rounds=1, N=123), (EIG_BOX, 1, 1, 0, 0, 256, 512,
                                             157312)),
    "round3-N123": (_args(rounds=3, N=123), (EIG_BOX, 1, 1, 1, 1, 256, 512,
                                             162752)),
    "round3-N123-chol-free": (_args(rounds=3, N=123, lo=0, hi=0, branch=CHOL),
                              (CHOL_FREE, 1, 1, 1, 1, 256, 512, 162752)),
    "round3-N124": (_args(rounds=3, N=124), (EIG_BOX, 1, 1, 1, 0, 256, 512,
                                             157696)),
    "round3-N124-eig-free": (_args(rounds=3, N=124, lo=0, hi=0),
                             (EIG_FREE, 1, 1, 1, 0, 256, 512, 157696)),
    "round1-N127": (_args(rounds=1, N=127), (EIG_BOX, 1, 1, 0, 0, 256, 512,
                                             158848)),
    "round3-N127": (_args(rounds=3, N=127), (EIG_BOX, 1, 1, 1, 0, 256, 512,
                                             158848)),
    "round1-A1": (_args(rounds=1, A=1), (EIG_BOX, 1, 1, 0, 0, 256, 512,
                                             _round_lds(100, False))),
    # ---- other problems and encodings: not this plan's
    "pendulum-sweep": (_args("pendulum"), UNSUPPORTED),
    "pendulum-round": (_args("pendulum", rounds=1), UNSUPPORTED),
    "double_cartpole-sweep": (_args("double_cartpole"), UNSUPPORTED),
    "double_cartpole-sweep64": (_args("double_cartpole", es=8), UNSUPPORTED),
    "double_cartpole-round": (_args("double_cartpole", rounds=3), UNSUPPORTED),
    "gaussian-sweep": (_args("cartpole:gaussian"), UNSUPPORTED),
    "gaussian-round": (_args("cartpole:gaussian", rounds=1), UNSUPPORTED),
    # ---- what the entry points refuse as arguments, before any plan (and
    # before the domain: a bad argument wins over an unsupported one)
    "B0": (_args(B=0), BADARG),
    "N0-round": (_args(N=0, rounds=1), BADARG),
    "A0-round": (_args(A=0, rounds=1), BADARG),
    "A0-sweep": (_args(A=0), (EIG_BOX, 1, 1, 0, 0, 256, 512, OVL32)),
    "branch2": (_args(branch=2), BADARG),
    "branch2-pendulum": (_args("pendulum", branch=2), BADARG),
    "B0-one-bound": (_args(B=0, lo=0), BADARG),
}


@pytest.mark.parametrize("case", sorted(TABLE))
def test_nominal_plan(case):
    (kind, es, B, N, A, lo, hi, branch, rounds, choice), want = TABLE[case]
    p = _problem(kind)
    out = (ctypes.c_int32 * 8)(*([-99] * 8))
    rc = _native.lib().pddp_n4_nominal_plan(
        ctypes.addressof(p), es, B, N, A, lo, hi, branch, rounds, choice,
        ctypes.addressof(out))
    if isinstance(want, int):
        assert rc == want
    else:
        assert rc == 0
        assert tuple(out) == want


def test_null_arguments_are_bad_arguments():
    p = _problem("cartpole")
    out = (ctypes.c_int32 * 8)()
    fn = _native.lib().pddp_n4_nominal_plan
    assert fn(None, 4, 16, 10, 1, 1, 1, 0, 0, 0, ctypes.addressof(out)) == BADARG
    assert fn(ctypes.addressof(p), 4, 16, 10, 1, 1, 1, 0, 0, 0, None) == BADARG
    assert fn(ctypes.addressof(p), 2, 16, 10, 1, 1, 1, 0, 0, 0,
              ctypes.addressof(out)) == BADARG
