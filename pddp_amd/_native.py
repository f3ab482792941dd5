"""ctypes binding of the C ABI in include/pddp_hip.h (libpddp_hip.so).

There is NO fallback: if the HIP library is missing or a call fails, this
module raises.  PyTorch is only used by callers for device memory and streams;
no torch type crosses this boundary (pointers and sizes only).
"""
import ctypes
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (PDDP_HIP_LIB: another build of the same library - the instrumented ones of
# tools/, e.g. -DPDDP_ELEM_MARKS)
LIB_PATH = os.environ.get("PDDP_HIP_LIB") or os.path.join(
    _HERE, "lib", "libpddp_hip.so")
CSRC = os.path.join(_HERE, "csrc")

MAX_AUG, MAX_ACTION, MAX_PARAMS = 8, 4, 8
# the per-trajectory table of the pddp_*_batch_* entry points: one row per
# trajectory (PDDP_BATCH_* of include/pddp_hip.h)
BATCH_ROW, BATCH_PARAMS, BATCH_X_GOAL, BATCH_U_GOAL = 20, 0, 8, 16
# the reference of the pddp_*_track_* entry points: one row per trajectory and
# time step (PDDP_REF_* of include/pddp_hip.h)
REF_ROW, REF_X_GOAL, REF_U_GOAL = 12, 0, 8
# the cost weights of the pddp_*_weighted_* entry points: one row per
# trajectory, the diagonals of Q, Q_term, R (PDDP_WEIGHT_* of
# include/pddp_hip.h)
WEIGHT_ROW, WEIGHT_Q, WEIGHT_Q_TERM, WEIGHT_R = 20, 0, 8, 16

c_int, c_double, c_void_p = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
c_uint64 = ctypes.c_uint64


class PddpProblem(ctypes.Structure):
    """include/pddp_problem.h `pddp_problem`."""
    _fields_ = [
        ("model", c_int), ("encoding", c_int), ("state_size", c_int),
        ("action_size", c_int), ("encoded_size", c_int), ("aug_size", c_int),
        ("params", c_double * MAX_PARAMS),
        ("Q", c_double * (MAX_AUG * MAX_AUG)),
        ("Q_term", c_double * (MAX_AUG * MAX_AUG)),
        ("R", c_double * (MAX_ACTION * MAX_ACTION)),
        ("x_goal", c_double * MAX_AUG),
        ("u_goal", c_double * MAX_ACTION),
    ]


class RecordLayout(ctypes.Structure):
    """include/pddp_hip.h `pddp_record_layout`."""
    _fields_ = [(k, c_int) for k in (
        "n", "m", "o_Fz", "o_Lzz", "o_Fu", "o_Luz", "o_Lz", "o_Luu", "o_Lu",
        "o_U", "stride", "gain_stride")]


class NativeError(RuntimeError):
    pass


def build(force=False):
    """Compiles libpddp_hip.so for gfx950 with hipcc (no GPU needed)."""
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    return LIB_PATH


_P = c_void_p  # (then: pieces of the closed-loop and hand-over signatures)
_REF, _NOISE = [_P, c_int, c_int], [_P, _P, c_uint64, c_uint64]
_LOOP, _LOOP_OUT = [c_int] * 3 + [_P] * 7, [_P] * 6
_STEP, _STEP_OUT = [c_int] * 4 + [_P] * 7, [_P] * 14
# (sampled shooting: shapes, z0 .. a_std, smooth, seed, offset, mask, outputs)
_SHOOT = [c_int] * 3 + [_P] * 5 + [c_double, c_uint64, c_uint64] + [_P] * 7
# (its weighted update: lam after a_std; W and J_w after J_best)
_MPPI = [c_int] * 3 + [_P] * 6 + [c_double, c_uint64, c_uint64] + [_P] * 9
# (its cross-entropy refit: K after S; sigma, std_min; smooth, mix; the mask,
# Jc, rank, best, J_best, n_elite, J_m, the three row outputs, the stream)
_CEM = [c_int] * 4 + [_P] * 6 + [c_double, c_double, c_uint64, c_uint64] + \
    [_P] * 11
# (the records and the line search, what every form takes behind its leading
# arguments: B N, Z .. state, stream; B N A, Z .. Jc, stream.  The forms lead
# with the problem; _batch adds the table; _track the table and the window;
# _weighted the table and the weights; _track_weighted all three)
_DERIVS, _SEARCH = [c_int] * 2 + [_P] * 10, [c_int] * 3 + [_P] * 12
_SIGS = {
    "pddp_hip_abi_version": [],
    "pddp_hip_device_count": [],
    "pddp_record_layout_of": [c_int, c_int, _P],
    "pddp_riccati_backward": [c_int] * 4 + [_P] * 4 + [c_int] + [_P] * 4,
    "pddp_riccati_backward_variant": [c_int] * 4 + [_P] * 4 + [c_int] +
                                     [_P] * 4 + [c_int],
    "pddp_riccati_backward_timed": [c_int] * 4 + [_P] * 4 + [c_int] +
                                   [_P] * 4 + [c_int, _P, _P],
    "pddp_boxqp_m1": [c_int] + [_P] * 9,
    "pddp_boxqp": [c_int, c_int] + [_P] * 10,
    "pddp_pack_records": [c_int] * 4 + [_P] * 10,
    "pddp_sum_stage_costs": [c_int, c_int, _P, _P, _P],
    "pddp_nominal_rollout": [_P, c_int, c_int] + [_P] * 7,
    "pddp_derivs": [_P] + _DERIVS,
    "pddp_line_search": [_P] + _SEARCH,
    "pddp_nominal_rollout_batch": [_P, _P, c_int, c_int] + [_P] * 7,
    "pddp_derivs_batch": [_P, _P] + _DERIVS,
    "pddp_line_search_batch": [_P, _P] + _SEARCH,
    "pddp_closed_loop": [_P] + _LOOP + _LOOP_OUT,
    "pddp_closed_loop_noisy": [_P] + _LOOP + _NOISE + _LOOP_OUT,
    "pddp_closed_loop_draws": [c_int] * 5 + [c_uint64, c_uint64, _P, _P],
    "pddp_closed_loop_track": [_P] + _REF + _LOOP + _NOISE + _LOOP_OUT,
    "pddp_shoot": [_P] + _SHOOT,
    "pddp_shoot_batch": [_P, _P] + _SHOOT,
    "pddp_shoot_draws": [c_int] * 4 + [c_uint64, c_uint64, _P, _P],
    "pddp_mppi": [_P] + _MPPI,
    "pddp_mppi_batch": [_P, _P] + _MPPI,
    "pddp_cem": [_P] + _CEM,
    "pddp_cem_batch": [_P, _P] + _CEM,
    # (a whole MPPI trial: problem, table, plant; B N S K TT t0 count; z0 ..
    # lam; smooth, seed, cand_offset, iter_stride; disturbance, w_std, v_std;
    # rollout_offset, step_offset; x_true, active, Jc; log_costs; the logs)
    "pddp_mppi_trial": [_P] * 3 + [c_int] * 7 + [_P] * 8 +
                       [c_double] + [c_uint64] * 3 + [_P] * 3 +
                       [c_uint64, c_int] + [_P] * 3 + [c_int] + [_P] * 9,
    # (a whole CEM trial: problem, table, plant; B N S K I TT t0 count; z0, U,
    # Z, mean, width, Um, Sm, u_min, u_max, sigma, sigma0, std_min; smooth,
    # mix; seed, cand_offset, iter_stride; then as the MPPI trial, with the
    # logs Xlog, Ulog, Jcl, Ylog, Jtrace, Jm, nelite, plan, std)
    "pddp_cem_trial": [_P] * 3 + [c_int] * 8 + [_P] * 12 +
                      [c_double] * 2 + [c_uint64] * 3 + [_P] * 3 +
                      [c_uint64, c_int] + [_P] * 3 + [c_int] + [_P] * 10,
    # (the planners under the line search's objective: problem, table, then
    # the window and / or the weights, then the sibling's list; the trial
    # takes both, nullable each, after the plant)
    "pddp_shoot_track": [_P, _P] + _REF + _SHOOT,
    "pddp_shoot_weighted": [_P, _P, _P] + _SHOOT,
    "pddp_shoot_track_weighted": [_P, _P] + _REF + [_P] + _SHOOT,
    "pddp_mppi_track": [_P, _P] + _REF + _MPPI,
    "pddp_mppi_weighted": [_P, _P, _P] + _MPPI,
    "pddp_mppi_track_weighted": [_P, _P] + _REF + [_P] + _MPPI,
    "pddp_cem_track": [_P, _P] + _REF + _CEM,
    "pddp_cem_weighted": [_P, _P, _P] + _CEM,
    "pddp_cem_track_weighted": [_P, _P] + _REF + [_P] + _CEM,
    "pddp_mppi_trial_goals": [_P] * 3 + _REF + [_P] + [c_int] * 7 + [_P] * 8 +
                             [c_double] + [c_uint64] * 3 + [_P] * 3 +
                             [c_uint64, c_int] + [_P] * 3 + [c_int] + [_P] * 9,
    "pddp_mpc_advance":[_P, _P] + _STEP + _STEP_OUT,
    "pddp_derivs_track": [_P, _P] + _REF + _DERIVS,
    "pddp_line_search_track": [_P, _P] + _REF + _SEARCH,
    "pddp_mpc_advance_track": [_P, _P] + _REF + _STEP + _STEP_OUT,
    "pddp_mpc_advance_noisy": [_P, _P] + _REF + _STEP + _NOISE +
                              [c_int, _P, _P] + _STEP_OUT,
    "pddp_mpc_observe": [c_int, c_int, _P, _P, c_uint64, c_uint64, c_int, _P,
                         _P, _P],
    "pddp_derivs_weighted": [_P, _P, _P] + _DERIVS,
    "pddp_line_search_weighted": [_P, _P, _P] + _SEARCH,
    "pddp_derivs_track_weighted": [_P, _P] + _REF + [_P] + _DERIVS,
    "pddp_line_search_track_weighted": [_P, _P] + _REF + [_P] + _SEARCH,
    "pddp_search_accept": [_P, c_int, c_int, c_int] + [_P] * 11 +
                          [c_double, c_double, c_int] +
                          [_P] * 11,
    "pddp_accept": [c_int] * 5 + [_P] * 5 + [c_double, c_double, c_int] +
                   [_P] * 12,
    "pddp_pack_best": [c_int, c_int, c_int, _P, _P, _P, ctypes.c_longlong, _P,
                       _P],
    "pddp_sweep_nominal": [_P, c_int, c_int] + [_P] * 5 + [c_int] +
                          [_P] * 7,
    "pddp_sweep_nominal_kernel": [c_int],
    "pddp_n4_nominal_plan": [_P] + [c_int] * 9 + [_P],
    "pddp_boxqp_m1_lean_f32": [c_int] + [_P] * 11,
    "pddp_round_nominal_f32": [_P, c_int, c_int, c_int] + [_P] * 5 + [c_int] +
                              [_P] * 9 + [c_double, c_double, c_int] +
                              [_P] * 7 + [c_int, _P, _P],
    "pddp_search_candidates": [c_int],
    "pddp_search_form": [c_int],
    "pddp_bnn_mlp_precision": [c_int],
    "pddp_bnn_mlp_deal": [c_int],
    "pddp_bnn_mlp_f32": [c_int] * 5 + [_P] * 11,
    "pddp_bnn_mlp_rows_f32": [c_int] * 5 + [_P] * 12,
    "pddp_bnn_mlp_f64": [c_int] * 5 + [_P] * 11,
    "pddp_bnn_mlp_rows_f64": [c_int] * 5 + [_P] * 12,
    "pddp_bnn_moment_step_f64": [_P, _P],
    "pddp_bnn_mlp_jvp_rows_f64": [c_int] * 7 + [_P] * 12,
    "pddp_bnn_jvp_features_f64": [_P, _P],
    "pddp_bnn_jvp_moments_f64": [_P, _P],
    "pddp_qr_cost_derivs_f64": [_P, _P],
    "pddp_bnn_moment_step_f32": [_P, _P],
    "pddp_bnn_mlp_jvp_f32": [c_int] * 6 + [_P] * 11,
    "pddp_bnn_mlp_jvp_live_f32": [c_int] * 7 + [_P] * 11,
    "pddp_bnn_mlp_jvp_rows_f32": [c_int] * 7 + [_P] * 12,
    "pddp_bnn_jvp_group": [c_int, c_int],
    "pddp_bnn_jvp_features_f32": [_P, _P],
    "pddp_bnn_jvp_moments_f32": [_P, _P],
    "pddp_qr_cost_derivs_f32": [_P, _P],
    "pddp_gp_step": [_P, c_int, _P, _P, _P, _P, _P, _P],
    "pddp_gp_step_masked": [_P, c_int, _P, _P, _P, _P, _P, _P, c_int, _P],
    "pddp_gp_step_lds_bytes": [c_int] * 6,
    "pddp_gp_step_form": [c_int] * 6,
    "pddp_gp_step_chunk": [c_int] * 6,
    "pddp_gp_step_chunked_lds_bytes": [c_int] * 6,
    "pddp_gp_step_force_chunk": [c_int],
    "pddp_gp_step_force_rows_per_launch": [c_int],
    "pddp_gp_rollout": [_P, _P, _P],
    "pddp_event_create": [_P],
    "pddp_event_record": [_P, _P],
    "pddp_event_elapsed_ms": [_P, _P, _P],
    "pddp_event_destroy": [_P],
    "pddp_attach_events": [_P, _P],
}
_TYPED = ("pddp_riccati_backward", "pddp_riccati_backward_variant",
          "pddp_riccati_backward_timed",
          "pddp_boxqp_m1", "pddp_boxqp", "pddp_pack_records", "pddp_sum_stage_costs",
          "pddp_nominal_rollout",
          "pddp_derivs",
          "pddp_line_search", "pddp_search_accept", "pddp_accept",
          "pddp_nominal_rollout_batch", "pddp_derivs_batch",
          "pddp_line_search_batch", "pddp_closed_loop", "pddp_mpc_advance",
          "pddp_closed_loop_noisy", "pddp_closed_loop_draws",
          "pddp_closed_loop_track",
          "pddp_shoot", "pddp_shoot_batch", "pddp_shoot_draws",
          "pddp_mppi", "pddp_mppi_batch", "pddp_mppi_trial",
          "pddp_cem", "pddp_cem_batch", "pddp_cem_trial",
          "pddp_shoot_track", "pddp_shoot_weighted",
          "pddp_shoot_track_weighted", "pddp_mppi_track", "pddp_mppi_weighted",
          "pddp_mppi_track_weighted", "pddp_mppi_trial_goals",
          "pddp_cem_track", "pddp_cem_weighted", "pddp_cem_track_weighted",
          "pddp_derivs_track", "pddp_line_search_track",
          "pddp_mpc_advance_track",
          "pddp_mpc_advance_noisy", "pddp_mpc_observe",
          "pddp_derivs_weighted", "pddp_line_search_weighted",
          "pddp_derivs_track_weighted", "pddp_line_search_track_weighted",
          "pddp_pack_best", "pddp_sweep_nominal", "pddp_gp_step",
          "pddp_gp_step_masked",
          "pddp_gp_rollout")

_lib = None


def exported_symbols():
    """Every symbol include/pddp_hip.h declares."""
    names = []
    for k in _SIGS:
        if k in _TYPED:
            names += [k + "_f32", k + "_f64"]
        else:
            names.append(k)
    names.append("pddp_hip_arch")
    return names


def lib():
    """Loads the HIP library; raises NativeError when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                "libpddp_hip.so is not built (%s). Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` - there "
                "is no CPU fallback." % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        for name, sig in _SIGS.items():
            for full in ([name + "_f32", name + "_f64"]
                         if name in _TYPED else [name]):
                fn = getattr(l, full)
                fn.argtypes = sig
                fn.restype = c_int
        l.pddp_hip_arch.restype = ctypes.c_char_p
        l.pddp_gp_step_lds_bytes.restype = ctypes.c_longlong
        l.pddp_gp_step_chunked_lds_bytes.restype = ctypes.c_longlong
        _lib = l
    return _lib


def suffix(dtype):
    if dtype == torch.float32:
        return "f32"
    if dtype == torch.float64:
        return "f64"
    raise NativeError("unsupported dtype %s (f32 / f64 only)" % dtype)


def ptr(t):
    """Device pointer of a tensor (None -> NULL). Must be contiguous."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise NativeError("non-contiguous tensor passed to the C ABI")
    return t.data_ptr()


def set_pointers(st, **tensors):
    """Pointer fields of a structure from tensors (None -> NULL).  The
    structure holds no reference: the caller keeps the tensors alive."""
    for name, t in tensors.items():
        setattr(st, name, ptr(t))


def set_angles(st, ang, non):
    """n_ang, n_non, ang[], non[] of a structure: the angular and the other
    indices of the state, in the order of the augmented features."""
    st.n_ang, st.n_non = len(ang), len(non)
    for i, v in enumerate(ang):
        st.ang[i] = int(v)
    for i, v in enumerate(non):
        st.non[i] = int(v)


def stream_handle(device=None):
    return torch.cuda.current_stream(device).cuda_stream


def check(rc, what):
    if rc != 0:
        raise NativeError("%s failed with code %d" % (what, rc))


def call(name, dtype, *args):
    fn = getattr(lib(), "%s_%s" % (name, suffix(dtype)))
    check(fn(*args), name)


class BnnStep(ctypes.Structure):
    """pddp_bnn_step of include/pddp_hip.h."""
    _fields_ = (
        [(k, ctypes.c_int32) for k in ("B", "A", "P", "D", "m", "N", "t",
                                       "n_ang")] +
        [("ang", ctypes.c_int32 * 2), ("n_non", ctypes.c_int32),
         ("non", ctypes.c_int32 * 8), ("in_dim", ctypes.c_int32),
         ("out_dim", ctypes.c_int32)] +
        [(k, ctypes.c_void_p) for k in (
            "Z", "U", "gains", "alphas", "u_min", "u_max", "active",
            "bwd_status", "Q", "Q_term", "R", "x_goal", "u_goal", "X_mean",
            "X_std_inv", "dX_mean", "dX_std", "net_out", "Xp", "F", "Zc", "Uc",
            "J", "Jc", "eps_out", "slot")])


class BnnJvp(ctypes.Structure):
    """pddp_bnn_jvp of include/pddp_hip.h."""
    _fields_ = (
        [(k, ctypes.c_int32) for k in ("B", "P", "D", "m", "N", "t", "n_ang")] +
        [("ang", ctypes.c_int32 * 2), ("n_non", ctypes.c_int32),
         ("non", ctypes.c_int32 * 8), ("in_dim", ctypes.c_int32),
         ("out_dim", ctypes.c_int32)] +
        [(k, ctypes.c_void_p) for k in (
            "Z", "U", "u_min", "u_max", "X_mean", "X_std_inv", "dX_mean",
            "dX_std", "net_out", "Xp", "Xp_next", "eps", "F", "Z_next", "F_z",
            "F_u", "eps_out")] +
        [("independent_noise", ctypes.c_int32), ("slot", ctypes.c_void_p)])


class GpModel(ctypes.Structure):
    """pddp_gp_model of include/pddp_hip.h."""
    _fields_ = (
        [(k, ctypes.c_int32) for k in ("state_size", "action_size", "M",
                                       "encoding", "n_ang", "n_non")] +
        [("ang", ctypes.c_int32 * 4), ("non", ctypes.c_int32 * 8)] +
        [(k, ctypes.c_void_p) for k in ("Xt", "Xt_pairs", "beta", "beta_pairs",
                                        "Kinv", "inv_ell2", "sf2", "sn2")])


class GpRollout(ctypes.Structure):
    """pddp_gp_rollout of include/pddp_hip.h."""
    _fields_ = (
        [(k, ctypes.c_int32) for k in ("B", "N", "A")] +
        [(k, ctypes.c_void_p) for k in (
            "Z", "U", "gains", "alphas", "u_min", "u_max", "active",
            "bwd_status", "Zc", "Uc", "Jc", "Q", "Q_term", "R", "x_goal",
            "u_goal")])


class QrCost(ctypes.Structure):
    """pddp_qr_cost of include/pddp_hip.h."""
    _fields_ = (
        [(k, ctypes.c_int32) for k in ("B", "N", "D", "m", "n_ang")] +
        [("ang", ctypes.c_int32 * 2), ("n_non", ctypes.c_int32),
         ("non", ctypes.c_int32 * 8)] +
        [(k, ctypes.c_void_p) for k in (
            "Z", "U", "u_min", "u_max", "Q", "Q_term", "R", "x_goal", "u_goal",
            "L", "L_z", "L_u", "L_zz", "L_uz", "L_uu")])


E_UNSUPPORTED = -2  # PDDP_E_UNSUPPORTED of include/pddp_hip.h


def call_rc(name, dtype, *args):
    """Like call(), but hands PDDP_E_UNSUPPORTED back to the caller (entry
    points that document it as 'make the separate calls instead')."""
    fn = getattr(lib(), "%s_%s" % (name, suffix(dtype)))
    rc = fn(*args)
    if rc != E_UNSUPPORTED:
        check(rc, name)
    return rc


def record_layout(n, m):
    out = RecordLayout()
    check(lib().pddp_record_layout_of(n, m, ctypes.addressof(out)),
          "pddp_record_layout_of")
    return out


def require_gpu(t):
    if not t.is_cuda:
        raise NativeError(
            "pddp_amd runs its hot path on the MI355X only; got a %s tensor "
            "(no CPU fallback)" % t.device)
