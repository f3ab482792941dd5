// mppi_trial.hip - a receding-horizon MPPI trial, every control step inside ONE
// launch: plan (K iterations of mppi.hip's law around the plan U), apply the
// first action to the plant, observe, shift the plan - for control steps
// t0 .. t0 + count - 1 of TT (pddp_mppi_trial_*, ILQRSolver.mppi_closed_loop);
// the same planning under the line search's objective
// (pddp_mppi_trial_goals_*, objective="search").  The reference has no
// counterpart: include/pddp_hip.h states the law, DESIGN.md 3.4o, 3.4p and
// 3.4q the kernels.
//
// The candidate rollout, the argmin, the weighted update, the weight and the
// sums are shoot.hip's and mppi.hip's: one text each
// (sampled_rollout_body.inc, sampled_argmin.inc, mppi_update_body.inc,
// sampled_common.hpp; included texts, not device functions - the Makefile's
// note on contraction).  The first statements, the plant section and the
// closing rollout are texts the CEM trial includes too (trial_prologue.inc,
// trial_plant_body.inc, trial_final_rollout.inc).  Two
// kernels per model and type over ONE text
// (mppi_trial_kernel_body.inc): mppi_trial_kernel with its nullable table,
// mppi_trial_goals_kernel with its nullable reference and weights.
//
// Mapping: mppi_kernel's - a trajectory owns a lane group of G lanes, lane 0
// of the group (the head) does what is done once per trajectory.  A
// trajectory never leaves its workgroup, so a control step needs no launch
// boundary.  What is new against mppi_kernel: lanes read what the head stored
// earlier in the launch - z0[b], and U[b] after a `took` copy or a shift.
// Every such hand-over is the head's stores, hand_over() (the wait on the
// stores, then the workgroup's barrier with its fence), then the group's
// loads; the candidate-0 cost and J_w the head needs for `took` it holds in
// its own registers.  The loops over c, k, the turns and t are launch-uniform
// and every shuffle and barrier sits under them alone: lanes outside the
// batch, masked or without a candidate take part with zeros.  No atomics.
//
// Under the objective, `window` is the launch's reference with ref_t0 as the
// caller gave it (ref_t0 + TT fits an int: the host's test); control step c
// plans under the window that starts at row min(ref_t0 + c, ref_len - 1) -
// `goals` inside the loop over c - and the applied step is logged as
// pddp_mpc_advance_track_* logs it: under that window's row 0, the terminal
// cost under its row 1, the SHARED Q, Q_term, R; the plant row then supplies
// parameters only (mpc_advance_goal_hooks.inc's plant).
#include "sampled_common.hpp"

namespace pddp {

template <typename T>
struct MppiTrialArgs {
  int B, N, S, G, K, TT, t0, count;
  const T* table;  // [B][PDDP_BATCH_ROW] or NULL: the controller's model
  const T* plant;  // [B][PDDP_BATCH_ROW] or NULL: the controller's model
  T* z0;           // [B][n]
  T* U;            // [B][N][m]
  T* Z;            // [B][N+1][n]
  T* U_work;       // [B][N][m]
  const T* u_min;
  const T* u_max;
  const T* a_std;  // [m]
  const T* lam;    // [B]
  T beta, gamma;
  uint64_t seed, cand_offset, iter_stride;
  const T* disturbance;  // [B][TT][n] or NULL
  const T* w_std;        // [n] or NULL
  const T* v_std;        // [n] or NULL
  uint64_t rollout_offset;
  int step_offset;
  T* x_true;  // [B][n], with v_std
  const uint8_t* active;
  T* Jc;  // [B][S], or [B][TT][K][S] with log_costs
  int log_costs;
  T* Xlog;      // [B][TT+1][n]
  T* Ulog;      // [B][TT][m]
  T* Jcl;       // [B]
  T* Ylog;      // [B][TT+1][n] or NULL
  T* J0_log;    // [B][TT][K] or NULL
  T* Jw_log;    // [B][TT][K] or NULL
  T* ess_log;   // [B][TT] or NULL
  T* plan_log;  // [B][TT][N][m] or NULL
};

// The goals kernel's block: MppiTrialArgs without `table` (RefArgs carries
// it) - a type of its own because the kernel's argument layout is.
template <typename T>
struct MppiTrialGoalsArgs {
  int B, N, S, G, K, TT, t0, count;
  const T* plant;
  T *z0, *U, *Z, *U_work;
  const T *u_min, *u_max, *a_std, *lam;
  T beta, gamma;
  uint64_t seed, cand_offset, iter_stride;
  const T *disturbance, *w_std, *v_std;
  uint64_t rollout_offset;
  int step_offset;
  T* x_true;
  const uint8_t* active;
  T* Jc;
  int log_costs;
  T *Xlog, *Ulog, *Jcl, *Ylog, *J0_log, *Jw_log, *ess_log, *plan_log;
};

#define PDDP_SAMPLED_AFTER_E0
#define PDDP_SAMPLED_KEEP_ROW

#define PDDP_PROBLEM_OF_B PDDP_PLAIN_PROBLEM_OF_B
// (the row through the writer, not PDDP_PLAIN_ROW_OF_B's statements: what this
// kernel was compiled from)
#define PDDP_ROW_OF_B                                                          \
  if (a.table != nullptr)                                                      \
    write_params_and_goals<T, MODEL>(P, a.table + (size_t)b * PDDP_BATCH_ROW);
#define PDDP_GOALS(point)
#define PDDP_TRIAL_WINDOW_OF_C
#define PDDP_TRIAL_PLANT_PROBLEM PDDP_PLAIN_TRIAL_PLANT_PROBLEM
#define PDDP_TRIAL_TERMINAL_GOAL PDDP_PLAIN_TRIAL_TERMINAL_GOAL
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void mppi_trial_kernel(
    ProblemT<T> shared, MppiTrialArgs<T> a) {
#include "mppi_trial_kernel_body.inc"
}
#undef PDDP_TRIAL_TERMINAL_GOAL
#undef PDDP_TRIAL_PLANT_PROBLEM
#undef PDDP_TRIAL_WINDOW_OF_C
#undef PDDP_GOALS
#undef PDDP_ROW_OF_B
#undef PDDP_PROBLEM_OF_B

// the controller's model under the planning objective: the weights row written
// over P once, ahead of the turns; with a reference the goals of P are a
// window's rows, `goals` the window of the step (`tracked` from `window`,
// ahead of the copy: the order this kernel was compiled from, nothing else)
#define PDDP_PROBLEM_OF_B                                                     \
  const bool tracked = window.ref != nullptr;                                  \
  RefArgs<T> goals = window;                                                   \
  PDDP_GOALS_P_OF_B
#define PDDP_ROW_OF_B
#define PDDP_GOALS(point) PDDP_GOALS_##point
// the window of control step c (one integer moves, as mpc_closed_loop moves
// it), clamped to the last row
#define PDDP_TRIAL_WINDOW_OF_C                                                 \
  if (tracked) {                                                               \
    const int first = window.ref_t0 + c;                                       \
    goals.ref_t0 = first < window.ref_len - 1 ? first : window.ref_len - 1;    \
  }
// the common yardstick: the SHARED Q, Q_term, R, the goals of the plant row -
// with a reference those of row ref_t0 + c
#define PDDP_TRIAL_PLANT_PROBLEM                                               \
  ProblemT<T> Pl = shared;                                                     \
  if (goals.table != nullptr)                                                  \
    write_params_and_goals<T, MODEL>(                                          \
        Pl, goals.table + (size_t)b * PDDP_BATCH_ROW);                         \
  if (a.plant != nullptr)                                                      \
    write_params_and_goals<T, MODEL>(Pl, a.plant + (size_t)b * PDDP_BATCH_ROW);\
  if (tracked) {                                                               \
    const T* row = ref_row(goals, b, 0);                                       \
    PDDP_COPY(D::na, Pl.goal, row + PDDP_REF_X_GOAL)                           \
    PDDP_COPY(m, Pl.ugoal, row + PDDP_REF_U_GOAL)                              \
  }
// (under row ref_t0 + c + 1, x_goal only)
#define PDDP_TRIAL_TERMINAL_GOAL                                               \
  if (tracked) {                                                               \
    const T* row1 = ref_row(goals, b, 1);                                      \
    PDDP_COPY(D::na, Pl.goal, row1 + PDDP_REF_X_GOAL)                          \
  }
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void mppi_trial_goals_kernel(
    ProblemT<T> shared, MppiTrialGoalsArgs<T> a, RefArgs<T> window,
    const T* weights) {
#include "mppi_trial_kernel_body.inc"
}
#undef PDDP_TRIAL_TERMINAL_GOAL
#undef PDDP_TRIAL_PLANT_PROBLEM
#undef PDDP_TRIAL_WINDOW_OF_C
#undef PDDP_GOALS
#undef PDDP_ROW_OF_B
#undef PDDP_PROBLEM_OF_B

#undef PDDP_SAMPLED_KEEP_ROW
#undef PDDP_SAMPLED_AFTER_E0

// ---- host path ---------------------------------------------------------------

template <typename T, int MODEL>
static int launch_mppi_trial(const pddp_problem& p, MppiTrialArgs<T> a,
                             hipStream_t st) {
  return launch_sampled<T>(mppi_trial_kernel<T, MODEL>, p, a, st);
}

template <typename T, int MODEL>
static int launch_mppi_trial(
    const pddp_problem& p, With<MppiTrialGoalsArgs<T>, FormGoals<T>> w,
    hipStream_t st) {
  return launch_sampled<T>(mppi_trial_goals_kernel<T, MODEL>, p, w.a, st,
                           w.x.goals, w.x.weights);
}

// (the goals kernel's block is the launch's `w.a`)
template <typename T>
static MppiTrialArgs<T>& block_of(MppiTrialArgs<T>& a) { return a; }
template <typename T>
static MppiTrialGoalsArgs<T>& block_of(
    With<MppiTrialGoalsArgs<T>, FormGoals<T>>& w) {
  return w.a;
}

// One impl and one argument test for both entry points.  `l`: the plain
// kernel's block, or the goals kernel's with its reference and weights
// (`with_goals`: a reference or weights or both; the reference's ref_t0 is NOT
// clamped here - the kernel forms ref_t0 + c, which fits an int, and clamps
// the sum).
template <typename T, typename Launch>
static int mppi_trial_impl(const pddp_problem* p, Launch l, bool with_goals,
                           const FormGoals<T>& x, double smooth,
                           void* stream) {
  auto& a = block_of(l);
  if (!check_trial_args(a, smooth) || !a.a_std || !a.lam || a.K < 1 ||
      !a.U_work || a.U_work == a.U)
    return PDDP_E_BADARG;
  if (with_goals) {
    const RefArgs<T>& r = x.goals;
    if (r.ref == nullptr && x.weights == nullptr) return PDDP_E_BADARG;
    if (r.ref != nullptr &&
        (r.ref_len < 1 || r.ref_t0 < 0 || r.ref_t0 > INT_MAX - a.TT))
      return PDDP_E_BADARG;
  }
  if (int rc = check_problem(p)) return rc;
  set_trial_noise<T>(a, smooth);
  PDDP_DISPATCH_MODEL(launch_mppi_trial, T, p, l, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

// what both entry points take behind their leading arguments, and the fields
// of either block that follow `plant`
#define PDDP_MPPI_TRIAL_PARAMS(T)                                              \
  int B, int N, int S, int K, int TT, int t0, int count, T *z0, T *U, T *Z,    \
      T *U_work, const T *u_min, const T *u_max, const T *a_std,               \
      const T *lam, double smooth, uint64_t seed, uint64_t cand_offset,        \
      uint64_t iter_stride, const T *disturbance, const T *w_std,              \
      const T *v_std, uint64_t rollout_offset, int step_offset, T *x_true,     \
      const uint8_t *active, T *Jc, int log_costs, T *Xlog, T *Ulog, T *Jcl,   \
      T *Ylog, T *J0_log, T *Jw_log, T *ess_log, T *plan_log, void *stream
#define PDDP_MPPI_TRIAL_HEAD B, N, S, 0, K, TT, t0, count
#define PDDP_MPPI_TRIAL_REST(T)                                                \
  plant, z0, U, Z, U_work, u_min, u_max, a_std, lam, T(0), T(0), seed,         \
      cand_offset, iter_stride, disturbance, w_std, v_std, rollout_offset,     \
      step_offset, x_true, active, Jc, log_costs, Xlog, Ulog, Jcl, Ylog,       \
      J0_log, Jw_log, ess_log, plan_log

#define PDDP_MPPI_TRIAL_ENTRY_POINTS(SUF, T)                                   \
  int pddp_mppi_trial_##SUF(const pddp_problem* p, const T* table,             \
                            const T* plant, PDDP_MPPI_TRIAL_PARAMS(T)) {       \
    return pddp::mppi_trial_impl<T>(                                           \
        p,                                                                     \
        pddp::MppiTrialArgs<T>{PDDP_MPPI_TRIAL_HEAD, table,                    \
                               PDDP_MPPI_TRIAL_REST(T)},                       \
        false, {}, smooth, stream);                                            \
  }                                                                            \
  int pddp_mppi_trial_goals_##SUF(                                             \
      const pddp_problem* p, const T* table, const T* plant, const T* ref,     \
      int ref_len, int ref_t0, const T* weights, PDDP_MPPI_TRIAL_PARAMS(T)) {  \
    const pddp::FormGoals<T> x{                                                \
        ref != nullptr ? pddp::RefArgs<T>{table, ref, ref_len, ref_t0}         \
                       : pddp::RefArgs<T>{table, nullptr, 0, 0},               \
        weights};                                                              \
    return pddp::mppi_trial_impl<T>(                                           \
        p,                                                                     \
        pddp::With<pddp::MppiTrialGoalsArgs<T>, pddp::FormGoals<T>>{           \
            {PDDP_MPPI_TRIAL_HEAD, PDDP_MPPI_TRIAL_REST(T)}, x},               \
        true, x, smooth, stream);                                              \
  }

PDDP_MPPI_TRIAL_ENTRY_POINTS(f32, float)
PDDP_MPPI_TRIAL_ENTRY_POINTS(f64, double)
#undef PDDP_MPPI_TRIAL_ENTRY_POINTS
#undef PDDP_MPPI_TRIAL_REST
#undef PDDP_MPPI_TRIAL_HEAD
#undef PDDP_MPPI_TRIAL_PARAMS

}  // extern "C"
