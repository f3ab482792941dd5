// track_goal_hooks.inc - the goal hooks of derivs_body.inc (TAKE_X, TAKE_U) and
// line_search_body.inc (TAKE_FIRST, NEXT_ROW, PREFETCH_NEXT, TAKE_NEXT) with a
// goal PER TIME STEP: the text the track_* and track_weighted_* kernels of
// goal_kernels.hpp define ahead of their bodies; the including header undefines
// them behind each pair of kernels.  The including kernel has `goals` (RefArgs,
// ref_args.hpp), `P` (its PDDP_PROBLEM_OF_B) and the body's `b`, `t`, `m`, `D`.
#define PDDP_GOALS(point) PDDP_GOALS_##point

// records: lane t takes its goals from its own reference row, the action's
// where the step has one
#define PDDP_GOALS_TAKE_X                                                      \
  const T* row = ref_row(goals, b, t);                                         \
  PDDP_COPY(D::na, P.goal, row + PDDP_REF_X_GOAL)
#define PDDP_GOALS_TAKE_U PDDP_COPY(m, P.ugoal, row + PDDP_REF_U_GOAL)

// line search: the goal row of step t + 1 is requested together with that
// step's nominal row and gains, ahead of the dependent chain
#define PDDP_GOALS_TAKE_FIRST                                                  \
  const T* row0 = ref_row(goals, b, 0);                                        \
  PDDP_COPY(D::na, P.goal, row0 + PDDP_REF_X_GOAL)                             \
  PDDP_COPY(m, P.ugoal, row0 + PDDP_REF_U_GOAL)
#define PDDP_GOALS_NEXT_ROW const T* row = ref_row(goals, b, t + 1);
#define PDDP_GOALS_PREFETCH_NEXT                                               \
  T xg2[D::na], ug2[m];                                                        \
  PDDP_COPY(D::na, xg2, row + PDDP_REF_X_GOAL)                                 \
  PDDP_COPY(m, ug2, row + PDDP_REF_U_GOAL)
#define PDDP_GOALS_TAKE_NEXT                                                   \
  PDDP_COPY(m, P.ugoal, ug2)                                                   \
  PDDP_COPY(D::na, P.goal, xg2)
