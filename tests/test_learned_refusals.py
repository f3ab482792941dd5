"""What the learned-model entry points - the GP step, its masked form and its
rollout (csrc/gp_step.hip), the fused Bayesian network in f32 and f64
(csrc/bnn_mlp.hip, csrc/bnn_mlp_f64.hip) - answer to a wrong call, and in
which order when a call is wrong in two ways.  CPU:
every answer here comes before the first HIP call and the non-null pointers
are host words nobody reads, as in tests/test_qr_cost_kernel.py
test_entry_point_refuses_before_any_launch.  The codes are PDDP_E_BADARG (-1)
and PDDP_E_UNSUPPORTED (-2) of include/pddp_hip.h, written out."""
import ctypes

import pytest

_WORDS = (ctypes.c_double * 16)()
# (32-byte aligned: the f64 network reads its masks 32 bytes at a time)
Q = (ctypes.addressof(_WORDS) + 31) & ~31

GP_POINTERS = ("Xt", "Xt_pairs", "beta", "beta_pairs", "Kinv", "inv_ell2",
               "sf2", "sn2")


def _gp_model(**change):
    """The cartpole's model, (E, D) = (4, 6), variance encoding; `ang0` /
    `non0` replace the first angle / non-angle index."""
    from pddp_amd import _native
    g = _native.GpModel()
    g.state_size, g.action_size, g.M, g.encoding = 4, 1, 5, 2
    g.n_ang, g.n_non = 1, 3
    g.ang[0] = 2
    for i, v in enumerate((0, 1, 3)):
        g.non[i] = v
    for k in GP_POINTERS:
        setattr(g, k, Q)
    for k, v in change.items():
        if k == "ang0":
            g.ang[0] = v
        elif k == "non0":
            g.non[0] = v
        else:
            setattr(g, k, v)
    return g


# (model changes, code): shared by the step and the rollout
GP_MODEL_CASES = (
    [({k: None}, -1) for k in GP_POINTERS] +
    [(dict(n_ang=5), -1), (dict(n_non=9), -1), (dict(n_non=2), -1),
     (dict(M=0), -1), (dict(action_size=0), -1),
     (dict(encoding=0), -2), (dict(encoding=5), -2),
     (dict(encoding=5, ang0=4), -2),       # the encoding before the indices
     (dict(ang0=4), -1), (dict(non0=-1), -1),
     # a consistent model of a pair that is not built
     (dict(state_size=5, n_non=5, n_ang=0, action_size=1), -2)])


@pytest.mark.parametrize("masked", [False, True], ids=["step", "masked"])
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_gp_step_refuses_before_any_launch(t, masked):
    from pddp_amd import _native
    lib = _native.lib()
    fn = getattr(lib, "pddp_gp_step_%s%s" % ("masked_" if masked else "", t))

    def step(g, R=3, z=Q, u=Q, z_next=Q, Fz=None, Fu=None, mask=Q, per=1):
        tail = (mask, per, None) if masked else (None,)
        return fn(None if g is None else ctypes.byref(g), R, z, u, z_next, Fz,
                  Fu, *tail)

    assert step(None) == -1
    assert step(_gp_model(), R=-1) == -1
    for k in ("z", "u", "z_next"):
        assert step(_gp_model(), **{k: None}) == -1, k
    assert step(_gp_model(), Fz=Q) == -1
    assert step(_gp_model(), Fu=Q) == -1
    if masked:
        assert step(_gp_model(), per=0) == -1
    # no rows: nothing to do, and said before the model's shape is looked at
    assert step(_gp_model(), R=0) == 0
    assert step(_gp_model(n_ang=9), R=0) == 0
    # ... but after the row arguments, the model's pointers, Fz / Fu, the mask
    assert step(_gp_model(Kinv=None), R=0) == -1
    assert step(_gp_model(), R=0, Fz=Q) == -1
    for change, code in GP_MODEL_CASES:
        assert step(_gp_model(**change)) == code, change
        assert step(_gp_model(**change), Fz=Q, Fu=Q) == code, change


ROLLOUT_REQUIRED = ("Z", "U", "gains", "alphas", "Zc", "Uc", "Jc", "Q",
                    "Q_term", "R", "x_goal", "u_goal")


def _gp_rollout(**change):
    from pddp_amd import _native
    r = _native.GpRollout()
    r.B, r.N, r.A = 2, 3, 3
    for k in ROLLOUT_REQUIRED + ("u_min", "u_max", "active", "bwd_status"):
        setattr(r, k, Q)
    for k, v in change.items():
        setattr(r, k, v)
    return r


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_gp_rollout_refuses_before_any_launch(t):
    from pddp_amd import _native
    fn = getattr(_native.lib(), "pddp_gp_rollout_" + t)

    def roll(g, r):
        return fn(None if g is None else ctypes.byref(g),
                  None if r is None else ctypes.byref(r), None)

    assert roll(_gp_model(), None) == -1
    for k in ("B", "N", "A"):
        for v in (0, -1):
            assert roll(_gp_model(), _gp_rollout(**{k: v})) == -1, (k, v)
    for k in ROLLOUT_REQUIRED:
        assert roll(_gp_model(), _gp_rollout(**{k: None})) == -1, k
    assert roll(_gp_model(), _gp_rollout(u_max=None)) == -1
    assert roll(_gp_model(), _gp_rollout(u_min=None)) == -1
    assert roll(None, _gp_rollout()) == -1
    for change, code in GP_MODEL_CASES:
        assert roll(_gp_model(**change), _gp_rollout()) == code, change
    # the rollout's own arguments before the model's
    assert roll(_gp_model(encoding=0), _gp_rollout(B=0)) == -1


# ---- the fused network ---------------------------------------------------------
BNN_POINTERS = ("X", "W1", "b1", "MT1", "W2", "b2", "MT2", "W3", "b3", "Y")
# entry point: (f64, takes a group, takes `live`, takes live_rows)
BNN_ENTRIES = {
    "pddp_bnn_mlp_f32": (False, False, False, False),
    "pddp_bnn_mlp_rows_f32": (False, False, False, True),
    "pddp_bnn_mlp_jvp_f32": (False, True, False, False),
    "pddp_bnn_mlp_jvp_live_f32": (False, True, True, False),
    "pddp_bnn_mlp_jvp_rows_f32": (False, True, True, True),
    "pddp_bnn_mlp_f64": (True, False, False, False),
    "pddp_bnn_mlp_rows_f64": (True, False, False, True),
    "pddp_bnn_mlp_jvp_rows_f64": (True, True, True, True),
}


def _bnn(name, R=32, P=7, group=8, live=None, in_dim=6, H=200, out_dim=4,
         **pointers):
    from pddp_amd import _native
    _, grouped, has_live, has_rows = BNN_ENTRIES[name]
    sizes = [R, P]
    if grouped:
        sizes.append(group)
    if has_live:
        sizes.append(group if live is None else live)
    sizes += [in_dim, H, out_dim]
    ptrs = [pointers.get(k, Q) for k in BNN_POINTERS]
    tail = [None, None] if has_rows else [None]  # (live_rows,) stream
    return getattr(_native.lib(), name)(*sizes, *ptrs, *tail)


@pytest.mark.parametrize("name", sorted(BNN_ENTRIES))
def test_bnn_mlp_refuses_before_any_launch(name):
    f64, grouped, has_live, _ = BNN_ENTRIES[name]
    for k in ("R", "P", "in_dim", "H", "out_dim"):
        for v in (0, -1):
            assert _bnn(name, **{k: v}) == -1, (k, v)
    for k in BNN_POINTERS:
        assert _bnn(name, **{k: None}) == -1, k
    if grouped:
        assert _bnn(name, group=4) == -1
        assert _bnn(name, R=36, group=12) == -1
        assert _bnn(name, R=36, group=8) == -1
        assert _bnn(name, R=36, group=12, in_dim=16) == -1  # group first
    if has_live:
        assert _bnn(name, live=0) == -1
        assert _bnn(name, live=9) == -1
        assert _bnn(name, live=9, out_dim=17) == -1
    if name == "pddp_bnn_mlp_jvp_rows_f64":
        assert _bnn(name, group=0, live=1) == -1
    assert _bnn(name, in_dim=16) == -2
    assert _bnn(name, out_dim=17) == -2
    assert _bnn(name, H=100) == -2
    if f64:
        if grouped:
            assert _bnn(name, group=32) == -2
            assert _bnn(name, group=32, MT1=Q + 8) == -2
        assert _bnn(name, MT1=Q + 8) == -1
        assert _bnn(name, MT2=Q + 8) == -1
        assert _bnn(name, MT2=Q + 16) == -1
        assert _bnn(name, in_dim=16, MT1=Q + 8) == -2  # the sizes first
        assert _bnn(name, H=100, MT2=Q + 8) == -1      # ... H last of all
    else:
        # (the f32 network has no alignment demand: H decides)
        assert _bnn(name, H=100, MT1=Q + 8) == -2
