// model_params.hpp - the number of parameters of each sample model, dt
// included (include/pddp_problem.h; ILQRSolver._PARAM_COUNT holds the same
// numbers on the Python side, tests/test_mpc_closed_loop.py compares the two),
// and the writers of a per-trajectory row over the shared problem.  The one
// copy of each: problem_kernels.hip (with goal_kernels.hpp), closed_loop.hip
// and mpc_advance.hip include it.
#pragma once

#include "models.hpp"

namespace pddp {

template <int MODEL>
constexpr int kModelParamCount = MODEL == PDDP_MODEL_CARTPOLE          ? 6
                                 : MODEL == PDDP_MODEL_DOUBLE_CARTPOLE ? 8
                                 : MODEL == PDDP_MODEL_PENDULUM        ? 5
                                                                       : 3;

// `row` [PDDP_BATCH_ROW] (include/pddp_hip.h: params, x_goal, u_goal) written
// over P; entries of the row beyond the model's sizes are not read.  The
// model parameters alone:
template <typename T, int MODEL>
PDDP_DEV void write_params(ProblemT<T>& P, const T* row) {
  P.dt = row[PDDP_BATCH_PARAMS];
#pragma unroll
  for (int i = 0; i < kModelParamCount<MODEL> - 1; ++i)
    P.p[i] = row[PDDP_BATCH_PARAMS + 1 + i];
}
// ... and the goals with them:
template <typename T, int MODEL>
PDDP_DEV void write_params_and_goals(ProblemT<T>& P, const T* row) {
  using D = ModelDims<MODEL>;
  write_params<T, MODEL>(P, row);
#pragma unroll
  for (int i = 0; i < D::na; ++i) P.goal[i] = row[PDDP_BATCH_X_GOAL + i];
#pragma unroll
  for (int i = 0; i < D::m; ++i) P.ugoal[i] = row[PDDP_BATCH_U_GOAL + i];
}

// `row` [PDDP_WEIGHT_ROW] (include/pddp_hip.h: the diagonals of Q, Q_term, R)
// written over the diagonals of P's cost matrices; the off-diagonal entries
// stay P's, entries of the row beyond the model's sizes are not read
// (goal_kernels.hpp).
template <typename T, int MODEL>
PDDP_DEV void write_weights(ProblemT<T>& P, const T* row) {
  using D = ModelDims<MODEL>;
#pragma unroll
  for (int i = 0; i < D::na; ++i) {
    P.Q[i * PDDP_MAX_AUG + i] = row[PDDP_WEIGHT_Q + i];
    P.Qt[i * PDDP_MAX_AUG + i] = row[PDDP_WEIGHT_Q_TERM + i];
  }
#pragma unroll
  for (int i = 0; i < D::m; ++i)
    P.R[i * PDDP_MAX_ACTION + i] = row[PDDP_WEIGHT_R + i];
}

}  // namespace pddp
