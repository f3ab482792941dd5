// track_weights.hip - a reference tracked under per-trajectory cost weights:
// the derivative records and the line search with a goal PER TIME STEP
// (tracking.hip) AND the diagonals of Q, Q_term and R of trajectory b taken
// from row b of a table (weights.hip) - the pddp_*_track_weighted_* entry
// points, ILQRSolver.set_reference(keep_weights=True) /
// set_batch_weights(keep_reference=True).
//
//   `ref` [B][ref_len][PDDP_REF_ROW] as in tracking.hip: horizon index
//   i = 0 .. N reads row min(ref_t0 + i, ref_len - 1), the last row is held.
//   `weights` [B][PDDP_WEIGHT_ROW] as in weights.hip.  The off-diagonal
//   entries, the model, the encoding and the bounds stay those of the
//   pddp_problem; the model parameters are row b of `table` where one is given
//   (its goals are not read: they come step by step), else the problem's.
//
// The backward sweep on records and the accept kernel never see the problem,
// so a round with both is derivs(track_weighted), backward,
// line_search(track_weighted), accept; the MPC hand-over and the closed-loop
// rollouts report under the shared matrices and stay tracking's
// (mpc_advance.hip, closed_loop.hip).
//
// A translation unit of its own (csrc/Makefile: FLAGS_track_weights).  Its two
// loops are the included texts of problem_kernels.hip - derivs_body.inc,
// line_search_body.inc - with tracking.hip's goal hooks
// (track_goal_hooks.inc); the row writers are model_params.hpp's (DESIGN.md
// 3.4f, 3.4l).  Both texts evaluate the cost under the full mask (cost_value's
// default QM), as in weights.hip: a weight may make a row live that the shared
// Q leaves dead.
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "ref_args.hpp"

namespace pddp {

// the reference and the weights of a launch (With<Args, TrackWeights<T>>,
// problem_args.hpp)
template <typename T>
struct TrackWeights {
  RefArgs<T> goals;
  const T* weights;  // [B][PDDP_WEIGHT_ROW]: the diagonals of Q, Q_term, R
};

// For the two kernels below: `P` is the shared problem with the model
// parameters of row b of the table, where one is given, and then the diagonals
// of row b of the weights written over it; the goals come step by step at the
// texts' PDDP_GOALS(point).
#define PDDP_PROBLEM_OF_B                                                      \
  ProblemT<T> P = shared;                                                      \
  if (goals.table != nullptr)                                                  \
    write_params<T, MODEL>(P, goals.table + (size_t)b * PDDP_BATCH_ROW);       \
  write_weights<T, MODEL>(P, weights + (size_t)b * PDDP_WEIGHT_ROW);
#include "track_goal_hooks.inc"

// --------------------------------------------------------------------------
// derivative records: one workgroup per trajectory, one lane per time step,
// records staged through LDS (derivs_body.inc); lane t takes its goals from
// its own reference row.  `terminal` a constant in each call of record_of:
// batch_derivs_kernel's note on a run-time choice between two members of a
// copy (problem_kernels.hip)
// --------------------------------------------------------------------------

template <typename T, int MODEL>
__global__ __launch_bounds__(kDerivThreads) void track_weighted_derivs_kernel(
    ProblemT<T> shared, DerivArgs<T> a, RefArgs<T> goals, const T* weights) {
#define PDDP_SPLIT_TERMINAL 1
#include "derivs_body.inc"
#undef PDDP_SPLIT_TERMINAL
}

// --------------------------------------------------------------------------
// line search: one lane per (trajectory, alpha) candidate, any A
// (line_search_body.inc).  The A lanes of a trajectory read the same rows:
// one broadcast each - the weights' ahead of the loop, the goals' of step
// t + 1 with that step's nominal row.
// --------------------------------------------------------------------------

template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void track_weighted_line_search_kernel(
    ProblemT<T> shared, LineSearchArgs<T> a, RefArgs<T> goals,
    const T* weights) {
#include "line_search_body.inc"
}

#undef PDDP_GOALS_TAKE_NEXT
#undef PDDP_GOALS_PREFETCH_NEXT
#undef PDDP_GOALS_NEXT_ROW
#undef PDDP_GOALS_TAKE_FIRST
#undef PDDP_GOALS_TAKE_U
#undef PDDP_GOALS_TAKE_X
#undef PDDP_GOALS
#undef PDDP_PROBLEM_OF_B

// --------------------------------------------------------------------------
// launchers and entry points
// --------------------------------------------------------------------------

template <typename T, int MODEL>
static int launch_track_weighted_derivs(
    const pddp_problem& p, With<DerivArgs<T>, TrackWeights<T>> w,
    hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  PDDP_LAUNCH((track_weighted_derivs_kernel<T, MODEL>), dim3(w.a.B),
              dim3(kDerivThreads), 0, st, P, w.a, w.x.goals, w.x.weights);
  return launch_status();
}
template <typename T, int MODEL>
static int launch_track_weighted_line_search(
    const pddp_problem& p, With<LineSearchArgs<T>, TrackWeights<T>> w,
    hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  PDDP_LAUNCH((track_weighted_line_search_kernel<T, MODEL>), search_lanes(w.a),
              dim3(kWave), 0, st, P, w.a, w.x.goals, w.x.weights);
  return launch_status();
}

template <typename T>
static int track_weighted_derivs_impl(
    const pddp_problem* p, const T* table, const T* ref, int ref_len,
    int ref_t0, const T* weights, int B, int N, const T* Z, const T* U,
    const T* u_min, const T* u_max, const uint8_t* mask, T* rec, T* L, T* J,
    int32_t* state, void* stream) {
  With<DerivArgs<T>, TrackWeights<T>> w{
      {B, N, Z, U, u_min, u_max, mask, rec, L, J, state}, {{}, weights}};
  if (!args_ok(w.a) || !ref_args(table, ref, ref_len, ref_t0, &w.x.goals) ||
      !weights)
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_track_weighted_derivs, T, p, w,
                      (hipStream_t)stream)
}

template <typename T>
static int track_weighted_line_search_impl(
    const pddp_problem* p, const T* table, const T* ref, int ref_len,
    int ref_t0, const T* weights, int B, int N, int A, const T* Z, const T* U,
    const T* gains, const T* alphas, const T* u_min, const T* u_max,
    const uint8_t* active, const int32_t* bwd_status, T* Zc, T* Uc, T* Jc,
    void* stream) {
  With<LineSearchArgs<T>, TrackWeights<T>> w{
      {B, N, A, Z, U, gains, alphas, u_min, u_max, active, bwd_status, Zc, Uc,
       Jc},
      {{}, weights}};
  if (!args_ok(w.a, true) ||
      !ref_args(table, ref, ref_len, ref_t0, &w.x.goals) || !weights)
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_track_weighted_line_search, T, p, w,
                      (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

#define PDDP_TRACK_WEIGHTED_ENTRY_POINTS(SUF, T)                               \
  int pddp_derivs_track_weighted_##SUF(                                        \
      const pddp_problem* p, const T* table, const T* ref, int ref_len,        \
      int ref_t0, const T* weights, int B, int N, const T* Z, const T* U,      \
      const T* u_min, const T* u_max, const uint8_t* mask, T* rec, T* L, T* J, \
      int32_t* state, void* stream) {                                          \
    return pddp::track_weighted_derivs_impl<T>(                                \
        p, table, ref, ref_len, ref_t0, weights, B, N, Z, U, u_min, u_max,     \
        mask, rec, L, J, state, stream);                                       \
  }                                                                            \
  int pddp_line_search_track_weighted_##SUF(                                   \
      const pddp_problem* p, const T* table, const T* ref, int ref_len,        \
      int ref_t0, const T* weights, int B, int N, int A, const T* Z,           \
      const T* U, const T* gains, const T* alphas, const T* u_min,             \
      const T* u_max, const uint8_t* active, const int32_t* bwd_status, T* Zc, \
      T* Uc, T* Jc, void* stream) {                                            \
    return pddp::track_weighted_line_search_impl<T>(                           \
        p, table, ref, ref_len, ref_t0, weights, B, N, A, Z, U, gains, alphas, \
        u_min, u_max, active, bwd_status, Zc, Uc, Jc, stream);                 \
  }

PDDP_TRACK_WEIGHTED_ENTRY_POINTS(f32, float)
PDDP_TRACK_WEIGHTED_ENTRY_POINTS(f64, double)
#undef PDDP_TRACK_WEIGHTED_ENTRY_POINTS

}  // extern "C"
