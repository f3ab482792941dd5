// goal_kernels.hpp - the derivative records and the line search of the forms
// that bring goals or a cost of their own: a goal PER TIME STEP
// (pddp_*_track_*, ILQRSolver.set_reference), the diagonals of Q, Q_term and R
// PER TRAJECTORY (pddp_*_weighted_*, ILQRSolver.set_batch_weights), and both
// (pddp_*_track_weighted_*).  Part of problem_kernels.hip, which holds the
// plain and the _batch kernels and the one host path of all five forms; not a
// translation unit.
//
//   `ref` [B][ref_len][PDDP_REF_ROW]: x_goal (augmented coordinates) and u_goal
//   of trajectory b at every step of its reference (include/pddp_hip.h).
//   Horizon index i = 0 .. N reads row min(ref_t0 + i, ref_len - 1): the last
//   row is held.
//   `weights` [B][PDDP_WEIGHT_ROW]: the diagonals of Q (augmented coordinates),
//   Q_term and R of trajectory b.  Diagonals and not full matrices: a per-lane
//   copy of Q, Q_term and R is 144 words for the double cartpole, the
//   diagonals are at most 20 - and only those leave the scalar operands of the
//   kernel argument.
//   The off-diagonal entries, the model, the encoding and the bounds stay those
//   of the pddp_problem; the model parameters are row b of `table` where one
//   is given (a run-time case, as in mpc_advance_kernel), else the problem's.
//   Without a reference the table's row gives the goals too; with one they are
//   not read: they come step by step.
//
// The nominal rollout reads no cost, the backward sweep on records and the
// accept kernel never see the problem, so a round in any of these forms is
// derivs(form), backward, line_search(form), accept; only the integer `ref_t0`
// moves from one MPC control step to the next.  The MPC hand-over and the
// closed-loop rollouts along a reference report under the shared matrices and
// stand with their operations: mpc_advance.hip, closed_loop.hip.
//
// Every kernel is one of the two included texts - derivs_body.inc,
// line_search_body.inc - behind its PDDP_PROBLEM_OF_B; the row writers are
// model_params.hpp's.  In all six `terminal` is a
// constant in each call of record_of: batch_derivs_kernel's note on a run-time
// choice between two members of a copy.  The weighted texts evaluate the cost
// under the full mask (cost_value's default QM): a weight may make a row live
// that the shared Q leaves dead, and the host cannot see the device table.
// The A lanes of a trajectory's line search read the same rows: one broadcast
// each - the table's and the weights' ahead of the loop, the goal row of step
// t + 1 together with that step's nominal row and gains, ahead of the
// dependent chain.
#pragma once

#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "ref_args.hpp"

namespace pddp {

// ---- a goal per time step ------------------------------------------------------
// `P` is the shared problem with the model parameters of row b of the table,
// where one is given, written over it (the goals come step by step), and the
// texts' PDDP_GOALS(point) is track_goal_hooks.inc's PDDP_GOALS_<point>.
#define PDDP_PROBLEM_OF_B                                                      \
  ProblemT<T> P = shared;                                                      \
  if (goals.table != nullptr)                                                  \
    write_params<T, MODEL>(P, goals.table + (size_t)b * PDDP_BATCH_ROW);
#include "track_goal_hooks.inc"

template <typename T, int MODEL>
__global__ __launch_bounds__(kDerivThreads) void track_derivs_kernel(
    ProblemT<T> shared, DerivArgs<T> a, RefArgs<T> goals) {
#define PDDP_SPLIT_TERMINAL 1
#include "derivs_body.inc"
#undef PDDP_SPLIT_TERMINAL
}

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

// ---- per-trajectory cost weights ---------------------------------------------
// the two per-trajectory tables of a launch: the kernels' argument type
template <typename T>
struct WeightArgs {
  const T* table;    // [B][PDDP_BATCH_ROW] or NULL: parameters and goals
  const T* weights;  // [B][PDDP_WEIGHT_ROW]: the diagonals of Q, Q_term, R
};

// `P` is the shared problem with row b of the table, where one is given, and
// then the diagonals of row b of the weights written over it.
#define PDDP_PROBLEM_OF_B                                                      \
  ProblemT<T> P = shared;                                                      \
  if (wt.table != nullptr)                                                     \
    write_params_and_goals<T, MODEL>(P,                                        \
                                     wt.table + (size_t)b * PDDP_BATCH_ROW);   \
  write_weights<T, MODEL>(P, wt.weights + (size_t)b * PDDP_WEIGHT_ROW);
#define PDDP_GOALS(point)

template <typename T, int MODEL>
__global__ __launch_bounds__(kDerivThreads) void weighted_derivs_kernel(
    ProblemT<T> shared, DerivArgs<T> a, WeightArgs<T> wt) {
#define PDDP_SPLIT_TERMINAL 1
#include "derivs_body.inc"
#undef PDDP_SPLIT_TERMINAL
}

template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void weighted_line_search_kernel(
    ProblemT<T> shared, LineSearchArgs<T> a, WeightArgs<T> wt) {
#include "line_search_body.inc"
}

#undef PDDP_GOALS
#undef PDDP_PROBLEM_OF_B

// ---- a reference under per-trajectory cost weights -----------------------------
// `P` is the shared problem with the model parameters of row b of the table,
// where one is given, and then the diagonals of row b of the weights written
// over it; the goals come step by step at the texts' PDDP_GOALS(point).
#define PDDP_PROBLEM_OF_B                                                      \
  ProblemT<T> P = shared;                                                      \
  if (goals.table != nullptr)                                                  \
    write_params<T, MODEL>(P, goals.table + (size_t)b * PDDP_BATCH_ROW);       \
  write_weights<T, MODEL>(P, weights + (size_t)b * PDDP_WEIGHT_ROW);
#include "track_goal_hooks.inc"

template <typename T, int MODEL>
__global__ __launch_bounds__(kDerivThreads) void track_weighted_derivs_kernel(
    ProblemT<T> shared, DerivArgs<T> a, RefArgs<T> goals, const T* weights) {
#define PDDP_SPLIT_TERMINAL 1
#include "derivs_body.inc"
#undef PDDP_SPLIT_TERMINAL
}

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

}  // namespace pddp
