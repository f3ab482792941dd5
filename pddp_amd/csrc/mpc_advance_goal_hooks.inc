// mpc_advance_goal_hooks.inc - mpc_advance_body.inc's three goal hooks: the
// text the three hand-over kernels (mpc_advance_kernel and
// track_mpc_advance_kernel of mpc_advance.hip, mpc_advance_noisy_kernel of
// mpc_advance_noise.hip) define
// ahead of the body and undefine behind it.  The including kernel has `a` (its
// argument block), the compile-time flag TRACK, `goals` (RefArgs: where TRACK
// is false nothing reads it, a kernel without the argument holds a
// value-initialised local) and defines PDDP_TABLE, where the controller's table
// travels: a.table, or goals.table in the kernel whose block has none.
//
// the controller's model: a tracked one takes its goals step by step in the
// rounds, the hand-over's rollout reads none
#define PDDP_PROBLEM_OF_B                                                      \
  ProblemT<T> P = shared;                                                      \
  if (PDDP_TABLE != nullptr) {                                                 \
    if constexpr (TRACK)                                                       \
      write_params<T, MODEL>(P, PDDP_TABLE + (size_t)b * PDDP_BATCH_ROW);      \
    else                                                                       \
      write_params_and_goals<T, MODEL>(                                        \
          P, PDDP_TABLE + (size_t)b * PDDP_BATCH_ROW);                         \
  }
// the plant with the goals the stage cost is logged under: the plant row's,
// or reference row ref_t0's (the plant row then supplies parameters only)
#define PDDP_PLANT_OF_B                                                        \
  ProblemT<T> Pl = P;                                                          \
  if (a.plant != nullptr) {                                                    \
    if constexpr (TRACK)                                                       \
      write_params<T, MODEL>(Pl, a.plant + (size_t)b * PDDP_BATCH_ROW);        \
    else                                                                       \
      write_params_and_goals<T, MODEL>(Pl,                                     \
                                       a.plant + (size_t)b * PDDP_BATCH_ROW);  \
  }                                                                            \
  if constexpr (TRACK) {                                                       \
    const T* row = ref_row(goals, b, 0);                                       \
    PDDP_COPY(D::na, Pl.goal, row + PDDP_REF_X_GOAL)                           \
    PDDP_COPY(m, Pl.ugoal, row + PDDP_REF_U_GOAL)                              \
  }
// the terminal cost at t == T - 1: under row ref_t0 + 1 (both clamped), x_goal
// only
#define PDDP_TERMINAL_GOALS                                                    \
  if constexpr (TRACK) {                                                       \
    const T* row1 = ref_row(goals, b, 1);                                      \
    PDDP_COPY(D::na, Pl.goal, row1 + PDDP_REF_X_GOAL)                          \
  }
