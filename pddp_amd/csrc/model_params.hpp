// model_params.hpp - the number of parameters of each sample model, dt
// included (include/pddp_problem.h; ILQRSolver._PARAM_COUNT holds the same
// numbers on the Python side, tests/test_mpc_closed_loop.py compares the two).
// Included by mpc_advance.hip only: problem_kernels.hip and closed_loop.hip
// keep their own copies, kParamCount and kPlantParamCount, because their text
// does not move (csrc/Makefile: FMA contraction); a new unit takes this one.
#pragma once

#include "../../include/pddp_problem.h"

namespace pddp {

template <int MODEL>
constexpr int kModelParamCount = MODEL == PDDP_MODEL_CARTPOLE          ? 6
                                 : MODEL == PDDP_MODEL_DOUBLE_CARTPOLE ? 8
                                 : MODEL == PDDP_MODEL_PENDULUM        ? 5
                                                                       : 3;

}  // namespace pddp
