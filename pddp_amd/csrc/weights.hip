// weights.hip - per-trajectory cost weights: the derivative records and the
// line search with the diagonals of Q, Q_term and R of trajectory b taken from
// row b of a table (the pddp_*_weighted_* entry points,
// ILQRSolver.set_batch_weights).
//
//   `weights` [B][PDDP_WEIGHT_ROW]: the diagonals of Q (augmented coordinates),
//   Q_term and R of trajectory b (include/pddp_hip.h).  The off-diagonal
//   entries, the model, the encoding and the bounds stay those of the
//   pddp_problem; the model parameters and the goals are row b of `table`
//   where one is given (a run-time case, as in tracking.hip), else the
//   problem's.
//
// Diagonals and not full matrices: a per-lane copy of Q, Q_term and R is 144
// words for the double cartpole, the diagonals are at most 20 - and only those
// leave the scalar operands of the kernel argument.
//
// The nominal rollout reads no cost, the backward sweep on records and the
// accept kernel never see the problem, so a round with weights is
// derivs(weighted), backward, line_search(weighted), accept.
//
// A translation unit of its own (csrc/Makefile: FLAGS_weights).  Its two loops
// are the included texts of problem_kernels.hip - derivs_body.inc,
// line_search_body.inc - with an empty goal hook; the row writers are
// model_params.hpp's.  Both texts evaluate the cost
// under the full mask (cost_value's default QM): a weight may make a row live
// that the shared Q leaves dead, and the host cannot see the device table.
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"

namespace pddp {

// the two per-trajectory tables of a launch
template <typename T>
struct WeightArgs {
  const T* table;    // [B][PDDP_BATCH_ROW] or NULL: parameters and goals
  const T* weights;  // [B][PDDP_WEIGHT_ROW]: the diagonals of Q, Q_term, R
};

// For the two kernels below: `P` is the shared problem with row b of the
// table, where one is given, and then the diagonals of row b of the weights
// written over it.
#define PDDP_PROBLEM_OF_B                                                      \
  ProblemT<T> P = shared;                                                      \
  if (wt.table != nullptr)                                                     \
    write_params_and_goals<T, MODEL>(P,                                        \
                                     wt.table + (size_t)b * PDDP_BATCH_ROW);   \
  write_weights<T, MODEL>(P, wt.weights + (size_t)b * PDDP_WEIGHT_ROW);
#define PDDP_GOALS(point)

// --------------------------------------------------------------------------
// derivative records: one workgroup per trajectory, one lane per time step,
// records staged through LDS (derivs_body.inc).  `terminal` a constant in each
// call of record_of: batch_derivs_kernel's note on a run-time choice between
// two members of a copy (problem_kernels.hip)
// --------------------------------------------------------------------------

template <typename T, int MODEL>
__global__ __launch_bounds__(kDerivThreads) void weighted_derivs_kernel(
    ProblemT<T> shared, DerivArgs<T> a, WeightArgs<T> wt) {
#define PDDP_SPLIT_TERMINAL 1
#include "derivs_body.inc"
#undef PDDP_SPLIT_TERMINAL
}

// --------------------------------------------------------------------------
// line search: one lane per (trajectory, alpha) candidate, any A
// (line_search_body.inc).  The A lanes of a trajectory read the same two
// rows: one broadcast read each ahead of the loop.
// --------------------------------------------------------------------------

template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void weighted_line_search_kernel(
    ProblemT<T> shared, LineSearchArgs<T> a, WeightArgs<T> wt) {
#include "line_search_body.inc"
}

#undef PDDP_GOALS
#undef PDDP_PROBLEM_OF_B

// --------------------------------------------------------------------------
// launchers and entry points
// --------------------------------------------------------------------------

// (With<Args, WeightArgs<T>>, problem_args.hpp: an argument block and the two
// tables of its launch)
template <typename T, int MODEL>
static int launch_weighted_derivs(const pddp_problem& p,
                                  With<DerivArgs<T>, WeightArgs<T>> w,
                                  hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  PDDP_LAUNCH((weighted_derivs_kernel<T, MODEL>), dim3(w.a.B),
              dim3(kDerivThreads), 0, st, P, w.a, w.x);
  return launch_status();
}
template <typename T, int MODEL>
static int launch_weighted_line_search(const pddp_problem& p,
                                       With<LineSearchArgs<T>, WeightArgs<T>> w,
                                       hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  PDDP_LAUNCH((weighted_line_search_kernel<T, MODEL>), search_lanes(w.a),
              dim3(kWave), 0, st, P, w.a, w.x);
  return launch_status();
}

template <typename T>
static int weighted_derivs_impl(const pddp_problem* p, const T* table,
                                const T* weights, int B, int N, const T* Z,
                                const T* U, const T* u_min, const T* u_max,
                                const uint8_t* mask, T* rec, T* L, T* J,
                                int32_t* state, void* stream) {
  With<DerivArgs<T>, WeightArgs<T>> w{
      {B, N, Z, U, u_min, u_max, mask, rec, L, J, state}, {table, weights}};
  if (!args_ok(w.a) || !weights) return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_weighted_derivs, T, p, w, (hipStream_t)stream)
}

template <typename T>
static int weighted_line_search_impl(const pddp_problem* p, const T* table,
                                     const T* weights, int B, int N, int A,
                                     const T* Z, const T* U, const T* gains,
                                     const T* alphas, const T* u_min,
                                     const T* u_max, const uint8_t* active,
                                     const int32_t* bwd_status, T* Zc, T* Uc,
                                     T* Jc, void* stream) {
  With<LineSearchArgs<T>, WeightArgs<T>> w{
      {B, N, A, Z, U, gains, alphas, u_min, u_max, active, bwd_status, Zc, Uc,
       Jc},
      {table, weights}};
  if (!args_ok(w.a, true) || !weights) return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_weighted_line_search, T, p, w,
                      (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

#define PDDP_WEIGHTED_ENTRY_POINTS(SUF, T)                                     \
  int pddp_derivs_weighted_##SUF(                                              \
      const pddp_problem* p, const T* table, const T* weights, int B, int N,   \
      const T* Z, const T* U, const T* u_min, const T* u_max,                  \
      const uint8_t* mask, T* rec, T* L, T* J, int32_t* state,                 \
      void* stream) {                                                          \
    return pddp::weighted_derivs_impl<T>(p, table, weights, B, N, Z, U,        \
                                         u_min, u_max, mask, rec, L, J, state, \
                                         stream);                              \
  }                                                                            \
  int pddp_line_search_weighted_##SUF(                                         \
      const pddp_problem* p, const T* table, const T* weights, int B, int N,   \
      int A, const T* Z, const T* U, const T* gains, const T* alphas,          \
      const T* u_min, const T* u_max, const uint8_t* active,                   \
      const int32_t* bwd_status, T* Zc, T* Uc, T* Jc, void* stream) {          \
    return pddp::weighted_line_search_impl<T>(                                 \
        p, table, weights, B, N, A, Z, U, gains, alphas, u_min, u_max, active, \
        bwd_status, Zc, Uc, Jc, stream);                                       \
  }

PDDP_WEIGHTED_ENTRY_POINTS(f32, float)
PDDP_WEIGHTED_ENTRY_POINTS(f64, double)
#undef PDDP_WEIGHTED_ENTRY_POINTS

}  // extern "C"
