// goal_form.hpp - the five forms of an operation that reads the problem's goals
// and cost (plain, _batch, _track, _weighted, _track_weighted): what a suffix
// brings, the test that it is there, and the five extern "C" fronts over an
// operation's one impl.  Shared by the records and the line search
// (problem_kernels.hip) and by the sampling planners
// (shoot.hip, mppi.hip; mppi_trial.hip takes the carrier: DESIGN.md 3.4q).
// Host side only.
#pragma once

#include "ref_args.hpp"

namespace pddp {

// What an entry point's suffix brings: `batch` promises the table, `track`
// the reference, `weighted` the weights; what a suffix does not name is
// absent.  `goals`: every suffix but the plain one and _batch (the table is
// then nullable, and a family's goals kernels run).
template <typename T>
struct GoalForm {
  bool batch, goals, track, weighted;
  const T* table;
  const T* ref;
  int ref_len, ref_t0;
  const T* weights;
};

// the reference and the weights of a launch
template <typename T>
struct FormGoals {
  RefArgs<T> goals;  // (ref NULL without a reference)
  const T* weights;  // [B][PDDP_WEIGHT_ROW] or NULL
};

// What the form promises is there: the table, the reference with ref_t0
// clamped (ref_args), the weights.
template <typename T>
static bool form_goals(const GoalForm<T>& f, FormGoals<T>* out) {
  *out = FormGoals<T>{RefArgs<T>{f.table, nullptr, 0, 0}, nullptr};
  if (f.batch && f.table == nullptr) return false;
  if (f.track &&
      !ref_args(f.table, f.ref, f.ref_len, f.ref_t0, &out->goals))
    return false;
  if (f.weighted && f.weights == nullptr) return false;
  if (f.weighted) out->weights = f.weights;
  return true;
}

}  // namespace pddp

// The five entry points of one operation (NAME: derivs, line_search, shoot,
// mppi) over its one impl, pddp::NAME_impl<T>(p, form, ARGS); PARAMS(T) is
// what every form takes behind its leading arguments.
#define PDDP_FORM_ENTRY_POINTS(NAME, SUF, T, PARAMS, ARGS)                     \
  int pddp_##NAME##_##SUF(const pddp_problem* p, PARAMS(T)) {                  \
    return pddp::NAME##_impl<T>(                                               \
        p, {false, false, false, false, nullptr, nullptr, 0, 0, nullptr},      \
        ARGS);                                                                 \
  }                                                                            \
  /* the same with a problem per trajectory: row b of `table` */               \
  int pddp_##NAME##_batch_##SUF(const pddp_problem* p, const T* table,         \
                                PARAMS(T)) {                                   \
    return pddp::NAME##_impl<T>(                                               \
        p, {true, false, false, false, table, nullptr, 0, 0, nullptr}, ARGS);  \
  }                                                                            \
  /* a goal per time step, per-trajectory weights, both: table nullable */     \
  int pddp_##NAME##_track_##SUF(const pddp_problem* p, const T* table,         \
                                const T* ref, int ref_len, int ref_t0,         \
                                PARAMS(T)) {                                   \
    return pddp::NAME##_impl<T>(                                               \
        p, {false, true, true, false, table, ref, ref_len, ref_t0, nullptr},   \
        ARGS);                                                                 \
  }                                                                            \
  int pddp_##NAME##_weighted_##SUF(const pddp_problem* p, const T* table,      \
                                   const T* weights, PARAMS(T)) {              \
    return pddp::NAME##_impl<T>(                                               \
        p, {false, true, false, true, table, nullptr, 0, 0, weights}, ARGS);   \
  }                                                                            \
  int pddp_##NAME##_track_weighted_##SUF(                                      \
      const pddp_problem* p, const T* table, const T* ref, int ref_len,        \
      int ref_t0, const T* weights, PARAMS(T)) {                               \
    return pddp::NAME##_impl<T>(                                               \
        p, {false, true, true, true, table, ref, ref_len, ref_t0, weights},    \
        ARGS);                                                                 \
  }
