// tracking.hip - reference tracking: the derivative records and the line
// search with a goal PER TIME STEP (pddp_derivs_track_*,
// pddp_line_search_track_*, ILQRSolver.set_reference).  The MPC hand-over and
// the closed-loop rollouts along a reference stand with their operations:
// mpc_advance.hip, closed_loop.hip.
//
//   `ref` [B][ref_len][PDDP_REF_ROW]: x_goal (augmented coordinates) and u_goal
//   of trajectory b at every step of its reference (include/pddp_hip.h).
//   Horizon index i = 0 .. N reads row min(ref_t0 + i, ref_len - 1): the last
//   row is held.  Q, Q_term, R, the model, the encoding and the bounds stay
//   those of the pddp_problem; the model parameters are row b of `table` where
//   one is given (a run-time case, as in mpc_advance_kernel), else the
//   problem's.
//
// The backward sweep on records and the accept kernel never see the problem,
// so a round with a reference is derivs(track), backward, line_search(track),
// accept; only the integer `ref_t0` moves from one MPC control step to the
// next.
//
// A translation unit of its own (csrc/Makefile: FLAGS_tracking).  Its two
// loops are the included texts of problem_kernels.hip - derivs_body.inc,
// line_search_body.inc - with the goals of `P` taken from a reference row
// (PDDP_COPY, ref_args.hpp) at the texts' hook points, where those kernels read
// one problem: track_goal_hooks.inc, which track_weights.hip includes as
// well; the row writer is model_params.hpp's.
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "ref_args.hpp"

namespace pddp {

// For the two kernels below: `P` is the shared problem with the model
// parameters of row b of the table, where one is given, written over it (the
// goals come step by step), and the texts' PDDP_GOALS(point) is
// track_goal_hooks.inc's PDDP_GOALS_<point>.
#define PDDP_PROBLEM_OF_B                                                      \
  ProblemT<T> P = shared;                                                      \
  if (goals.table != nullptr)                                                  \
    write_params<T, MODEL>(P, goals.table + (size_t)b * PDDP_BATCH_ROW);
#include "track_goal_hooks.inc"

// --------------------------------------------------------------------------
// derivative records: one workgroup per trajectory, one lane per time step,
// records staged through LDS (derivs_body.inc); lane t takes its goals from
// its own reference row.  `terminal` a constant in each call of record_of:
// batch_derivs_kernel's note on a run-time choice between two members of a
// copy (problem_kernels.hip)
// --------------------------------------------------------------------------

template <typename T, int MODEL>
__global__ __launch_bounds__(kDerivThreads) void track_derivs_kernel(
    ProblemT<T> shared, DerivArgs<T> a, RefArgs<T> goals) {
#define PDDP_SPLIT_TERMINAL 1
#include "derivs_body.inc"
#undef PDDP_SPLIT_TERMINAL
}

// --------------------------------------------------------------------------
// line search: one lane per (trajectory, alpha) candidate, any A
// (line_search_body.inc); the goal row of step t + 1 is requested together
// with that step's nominal row and gains, ahead of the dependent chain.  The
// A lanes of a trajectory read the same addresses: one broadcast.
// --------------------------------------------------------------------------

template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void track_line_search_kernel(
    ProblemT<T> shared, LineSearchArgs<T> a, RefArgs<T> goals) {
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

// (With<Args, RefArgs<T>>, problem_args.hpp: an argument block and the
// reference of its launch)
template <typename T, int MODEL>
static int launch_track_derivs(const pddp_problem& p,
                               With<DerivArgs<T>, RefArgs<T>> w,
                               hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  PDDP_LAUNCH((track_derivs_kernel<T, MODEL>), dim3(w.a.B),
              dim3(kDerivThreads), 0, st, P, w.a, w.x);
  return launch_status();
}
template <typename T, int MODEL>
static int launch_track_line_search(const pddp_problem& p,
                                    With<LineSearchArgs<T>, RefArgs<T>> w,
                                    hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  PDDP_LAUNCH((track_line_search_kernel<T, MODEL>), search_lanes(w.a),
              dim3(kWave), 0, st, P, w.a, w.x);
  return launch_status();
}

template <typename T>
static int track_derivs_impl(const pddp_problem* p, const T* table,
                             const T* ref, int ref_len, int ref_t0, int B,
                             int N, const T* Z, const T* U, const T* u_min,
                             const T* u_max, const uint8_t* mask, T* rec, T* L,
                             T* J, int32_t* state, void* stream) {
  With<DerivArgs<T>, RefArgs<T>> w{
      {B, N, Z, U, u_min, u_max, mask, rec, L, J, state}, {}};
  if (!args_ok(w.a) || !ref_args(table, ref, ref_len, ref_t0, &w.x))
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_track_derivs, T, p, w, (hipStream_t)stream)
}

template <typename T>
static int track_line_search_impl(const pddp_problem* p, const T* table,
                                  const T* ref, int ref_len, int ref_t0, int B,
                                  int N, int A, const T* Z, const T* U,
                                  const T* gains, const T* alphas,
                                  const T* u_min, const T* u_max,
                                  const uint8_t* active,
                                  const int32_t* bwd_status, T* Zc, T* Uc,
                                  T* Jc, void* stream) {
  With<LineSearchArgs<T>, RefArgs<T>> w{
      {B, N, A, Z, U, gains, alphas, u_min, u_max, active, bwd_status, Zc, Uc,
       Jc},
      {}};
  if (!args_ok(w.a, true) || !ref_args(table, ref, ref_len, ref_t0, &w.x))
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_track_line_search, T, p, w, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

#define PDDP_TRACK_ENTRY_POINTS(SUF, T)                                        \
  int pddp_derivs_track_##SUF(                                                 \
      const pddp_problem* p, const T* table, const T* ref, int ref_len,        \
      int ref_t0, int B, int N, const T* Z, const T* U, const T* u_min,        \
      const T* u_max, const uint8_t* mask, T* rec, T* L, T* J, int32_t* state, \
      void* stream) {                                                          \
    return pddp::track_derivs_impl<T>(p, table, ref, ref_len, ref_t0, B, N, Z, \
                                      U, u_min, u_max, mask, rec, L, J, state, \
                                      stream);                                 \
  }                                                                            \
  int pddp_line_search_track_##SUF(                                            \
      const pddp_problem* p, const T* table, const T* ref, int ref_len,        \
      int ref_t0, int B, int N, int A, const T* Z, const T* U, const T* gains, \
      const T* alphas, const T* u_min, const T* u_max, const uint8_t* active,  \
      const int32_t* bwd_status, T* Zc, T* Uc, T* Jc, void* stream) {          \
    return pddp::track_line_search_impl<T>(                                    \
        p, table, ref, ref_len, ref_t0, B, N, A, Z, U, gains, alphas, u_min,   \
        u_max, active, bwd_status, Zc, Uc, Jc, stream);                        \
  }

PDDP_TRACK_ENTRY_POINTS(f32, float)
PDDP_TRACK_ENTRY_POINTS(f64, double)
#undef PDDP_TRACK_ENTRY_POINTS

}  // extern "C"
