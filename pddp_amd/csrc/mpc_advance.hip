// mpc_advance.hip - the hand-over between two control steps of a receding-
// horizon (MPC) trial: apply the first action of every trajectory's
// re-optimised nominal to its plant, log the trial, shift the warm start, roll
// out the new nominal and re-arm the controller state machine, in one launch -
// with ONE goal (pddp_mpc_advance_*) or a goal PER TIME STEP
// (pddp_mpc_advance_track_*).
//
//   the trial step of the outer loop   pddp/controllers/pddp.py:209-245
//                                      (_apply_controller, mpc=True, batched:
//                                      the sample models as the plant)
//   emit U[0], shift the nominal       ilqr.py:355-362 (forward, mpc=True)
//   the regularisation reset           ilqr.py:364-367 (_reset_reg)
//
// A translation unit of its own (csrc/Makefile: FLAGS_mpc_advance).  Both
// kernels' loop is an included text, mpc_advance_body.inc, with the goal hooks
// of mpc_advance_goal_hooks.inc; mpc_advance_noise.hip includes the two as
// well, with draws at the text's state hooks.  The row writers are
// model_params.hpp's.
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "mpc_advance_args.hpp"
#include "ref_args.hpp"

namespace pddp {

// Mapping: one lane per trajectory, as nominal_rollout_kernel; everything of
// trajectory b is read and written by its lane alone, J in t order, no
// atomics.  The shards of n_live belong to no trajectory: the first workgroup
// zeroes them (the rounds before and after this launch are stream-ordered
// around it).
template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void mpc_advance_kernel(
    ProblemT<T> shared, MpcAdvanceArgs<T> a) {
  constexpr bool TRACK = false;
  const RefArgs<T> goals{};
#define PDDP_TABLE a.table
#include "mpc_advance_goal_hooks.inc"
// (no noise: z0 is the plant's state and the controller's)
#define PDDP_PLANT_STATE
#define PDDP_PLANT_STEPPED
#define PDDP_NOMINAL_START
#include "mpc_advance_body.inc"
#undef PDDP_NOMINAL_START
#undef PDDP_PLANT_STEPPED
#undef PDDP_PLANT_STATE
#undef PDDP_TERMINAL_GOALS
#undef PDDP_PLANT_OF_B
#undef PDDP_PROBLEM_OF_B
#undef PDDP_TABLE
}

// The same along a reference: the stage cost logged at control step t is taken
// under reference row ref_t0, the terminal cost at t == T - 1 under row
// ref_t0 + 1 (both clamped).  The plant row supplies the parameters only.
// Dynamics, shift, rollout and re-arm read no goal.
template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void track_mpc_advance_kernel(
    ProblemT<T> shared, TrackAdvanceArgs<T> a, RefArgs<T> goals) {
  constexpr bool TRACK = true;
#define PDDP_TABLE goals.table
#include "mpc_advance_goal_hooks.inc"
#define PDDP_PLANT_STATE
#define PDDP_PLANT_STEPPED
#define PDDP_NOMINAL_START
#include "mpc_advance_body.inc"
#undef PDDP_NOMINAL_START
#undef PDDP_PLANT_STEPPED
#undef PDDP_PLANT_STATE
#undef PDDP_TERMINAL_GOALS
#undef PDDP_PLANT_OF_B
#undef PDDP_PROBLEM_OF_B
#undef PDDP_TABLE
}

template <typename T, int MODEL>
static int launch_mpc_advance(const pddp_problem& p, MpcAdvanceArgs<T> a,
                              hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  PDDP_LAUNCH((mpc_advance_kernel<T, MODEL>), advance_blocks(a), dim3(kWave),
              0, st, P, a);
  return launch_status();
}
// (With<Args, RefArgs<T>>, problem_args.hpp: an argument block and the
// reference of its launch)
template <typename T, int MODEL>
static int launch_track_advance(const pddp_problem& p,
                                With<TrackAdvanceArgs<T>, RefArgs<T>> w,
                                hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  PDDP_LAUNCH((track_mpc_advance_kernel<T, MODEL>), advance_blocks(w.a),
              dim3(kWave), 0, st, P, w.a, w.x);
  return launch_status();
}

template <typename T>
static int mpc_advance_impl(const pddp_problem* p, MpcAdvanceArgs<T> a,
                            void* stream) {
  if (!advance_args_ok(a)) return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_mpc_advance, T, p, a, (hipStream_t)stream)
}

template <typename T>
static int track_advance_impl(const pddp_problem* p, const T* table,
                              const T* ref, int ref_len, int ref_t0,
                              TrackAdvanceArgs<T> a, void* stream) {
  With<TrackAdvanceArgs<T>, RefArgs<T>> w{a, {}};
  if (!advance_args_ok(a) || !ref_args(table, ref, ref_len, ref_t0, &w.x))
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_track_advance, T, p, w, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

#define PDDP_MPC_ADVANCE_ENTRY_POINTS(SUF, T)                                  \
  int pddp_mpc_advance_##SUF(const pddp_problem* p, const T* table,            \
                             PDDP_ADVANCE_STEP_PARAMS(T),                      \
                             PDDP_ADVANCE_LOG_PARAMS(T)) {                     \
    return pddp::mpc_advance_impl<T>(p, {PDDP_MPC_ADVANCE_ARGS}, stream);      \
  }                                                                            \
  int pddp_mpc_advance_track_##SUF(                                            \
      const pddp_problem* p, const T* table, const T* ref, int ref_len,        \
      int ref_t0, PDDP_ADVANCE_STEP_PARAMS(T), PDDP_ADVANCE_LOG_PARAMS(T)) {   \
    return pddp::track_advance_impl<T>(p, table, ref, ref_len, ref_t0,         \
                                       {PDDP_TRACK_ADVANCE_ARGS}, stream);     \
  }

PDDP_MPC_ADVANCE_ENTRY_POINTS(f32, float)
PDDP_MPC_ADVANCE_ENTRY_POINTS(f64, double)
#undef PDDP_MPC_ADVANCE_ENTRY_POINTS
#undef PDDP_MPC_ADVANCE_ARGS
#undef PDDP_TRACK_ADVANCE_ARGS
#undef PDDP_ADVANCE_LOG_PARAMS
#undef PDDP_ADVANCE_STEP_PARAMS

}  // extern "C"
