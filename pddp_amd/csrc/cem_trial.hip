// cem_trial.hip - a receding-horizon CEM trial, every control step inside ONE
// launch: plan (I iterations of cem.hip's law around a mean and a width, with
// an incumbent that is never worse than the step's start), apply the
// incumbent's first action to the plant, observe, shift the plan and the width
// - for control steps t0 .. t0 + count - 1 of TT (pddp_cem_trial_*,
// ILQRSolver.cem_closed_loop).  The plain objective only: the shared Q, Q_term,
// R, one goal per trajectory.  The reference has no counterpart:
// include/pddp_hip.h states the law, DESIGN.md 3.4t the kernel.
//
// The candidate rollout is the family's one text (sampled_rollout_body.inc)
// through the width-per-step hooks cem.hip uses; the ranking and the refit are
// cem.hip's texts (cem_rank_body.inc, cem_refit_body.inc); the first
// statements, the plant section and the closing rollout are the MPPI trial's
// (trial_prologue.inc, trial_plant_body.inc, trial_final_rollout.inc;
// DESIGN.md 3.4u).  One kernel per model and type
// (cem_trial_kernel_body.inc).
//
// Mapping: mppi_trial_kernel's - a trajectory owns a lane group of G lanes and
// never leaves its workgroup, lane 0 of the group (the head) does what is done
// once per trajectory.  Four things are handed from one iteration or control
// step to the next inside the launch: the mean, the width, the incumbent
// (U[b]) and z0[b].  The head stores each, the whole group reads the mean, the
// width and z0 later (pass 1 reads the two rows from every lane).  Every such
// hand-over is the head's stores, hand_over() (the wait on the stores, then
// the workgroup's barrier with its fence), then the group's loads; the costs
// the head needs for its selects it holds in its own registers.  The LDS words
// of the ranking survive an iteration: the cut is written and read under the
// iteration's own `ok` alone, behind barriers of the same iteration.  Um / Sm
// double as the running sums over a lane's turns (S > 256) and are buffers of
// their own.  The loops over c, k, the turns and t are launch-uniform and
// every shuffle and barrier sits under them alone: lanes outside the batch,
// masked or without a candidate take part with zeros.  No atomics.
#include "sampled_common.hpp"

namespace pddp {

template <typename T>
struct CemTrialArgs {
  int B, N, S, G, K, I, TT, t0, count;
  const T* table;   // [B][PDDP_BATCH_ROW] or NULL: the controller's model
  const T* plant;   // [B][PDDP_BATCH_ROW] or NULL: the controller's model
  T* z0;            // [B][n]
  T* U;             // [B][N][m]: the plan, inside a step the incumbent
  T* Z;             // [B][N+1][n]
  T* mean;          // [B][N][m] work, as width, Um, Sm
  T* width;
  T* Um;
  T* Sm;
  const T* u_min;
  const T* u_max;
  T* sigma;         // [B][N][m]: the width the next control step starts from
  const T* sigma0;  // [B][N][m] or NULL: every step restarts from it
  const T* std_min;  // [m] or NULL: zeros
  T beta, gamma, step;
  uint64_t seed, cand_offset, iter_stride;
  const T* disturbance;  // [B][TT][n] or NULL
  const T* w_std;        // [n] or NULL
  const T* v_std;        // [n] or NULL
  uint64_t rollout_offset;
  int step_offset;
  T* x_true;  // [B][n], with v_std
  const uint8_t* active;
  T* Jc;  // [B][S], or [B][TT][I][S] with log_costs
  int log_costs;
  T* Xlog;              // [B][TT+1][n]
  T* Ulog;              // [B][TT][m]
  T* Jcl;               // [B]
  T* Ylog;              // [B][TT+1][n] or NULL
  T* Jtrace_log;        // [B][TT][I+1] or NULL
  T* Jm_log;            // [B][TT][I] or NULL
  int32_t* nelite_log;  // [B][TT][I] or NULL
  T* plan_log;          // [B][TT][N][m] or NULL
  T* std_log;           // [B][TT][N][m] or NULL
};

#define PDDP_SAMPLED_AFTER_E0 PDDP_WIDTH_ROWS_AFTER_E0
#define PDDP_SAMPLED_WIDTH_REQUEST PDDP_WIDTH_ROWS_REQUEST
#define PDDP_SAMPLED_WIDTH(r) sg[r]
#define PDDP_SAMPLED_KEEP_ROW
#define PDDP_GOALS(point)
#define PDDP_TRIAL_PLANT_PROBLEM PDDP_PLAIN_TRIAL_PLANT_PROBLEM
#define PDDP_TRIAL_TERMINAL_GOAL PDDP_PLAIN_TRIAL_TERMINAL_GOAL
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void cem_trial_kernel(
    ProblemT<T> shared, CemTrialArgs<T> a) {
#include "cem_trial_kernel_body.inc"
}
#undef PDDP_TRIAL_TERMINAL_GOAL
#undef PDDP_TRIAL_PLANT_PROBLEM
#undef PDDP_GOALS
#undef PDDP_SAMPLED_KEEP_ROW
#undef PDDP_SAMPLED_WIDTH
#undef PDDP_SAMPLED_WIDTH_REQUEST
#undef PDDP_SAMPLED_AFTER_E0

// ---- host path ---------------------------------------------------------------

template <typename T, int MODEL>
static int launch_cem_trial(const pddp_problem& p, CemTrialArgs<T> a,
                            hipStream_t st) {
  return launch_sampled<T>(cem_trial_kernel<T, MODEL>, p, a, st);
}

template <typename T>
static int cem_trial_impl(const pddp_problem* p, CemTrialArgs<T> a,
                          double smooth, double mix, void* stream) {
  if (!check_trial_args(a, smooth) || !a.sigma ||
      !(mix >= 0.0 && mix < 1.0) ||  // (NaN fails both)
      a.K < 1 || a.K > a.S || a.I < 1)
    return PDDP_E_BADARG;
  // a work buffer is there and is no other buffer of the call
  const void* work[] = {a.mean, a.width, a.Um, a.Sm};
  const void* others[] = {
      a.table,  a.plant,      a.z0,     a.U,          a.Z,       a.u_min,
      a.u_max,  a.sigma,      a.sigma0, a.std_min,    a.disturbance,
      a.w_std,  a.v_std,      a.x_true, a.active,     a.Jc,      a.Xlog,
      a.Ulog,   a.Jcl,        a.Ylog,   a.Jtrace_log, a.Jm_log,  a.nelite_log,
      a.plan_log, a.std_log};
  for (int i = 0; i < 4; ++i) {
    if (work[i] == nullptr) return PDDP_E_BADARG;
    for (int j = 0; j < i; ++j)
      if (work[i] == work[j]) return PDDP_E_BADARG;
    for (const void* o : others)
      if (work[i] == o) return PDDP_E_BADARG;
  }
  if (int rc = check_problem(p)) return rc;
  set_trial_noise<T>(a, smooth);
  a.step = (T)(1.0 - mix);
  PDDP_DISPATCH_MODEL(launch_cem_trial, T, p, a, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

#define PDDP_CEM_TRIAL_ENTRY_POINT(SUF, T)                                     \
  int pddp_cem_trial_##SUF(                                                    \
      const pddp_problem* p, const T* table, const T* plant, int B, int N,     \
      int S, int K, int I, int TT, int t0, int count, T* z0, T* U, T* Z,       \
      T* mean, T* width, T* Um, T* Sm, const T* u_min, const T* u_max,         \
      T* sigma, const T* sigma0, const T* std_min, double smooth, double mix,  \
      uint64_t seed, uint64_t cand_offset, uint64_t iter_stride,               \
      const T* disturbance, const T* w_std, const T* v_std,                    \
      uint64_t rollout_offset, int step_offset, T* x_true,                     \
      const uint8_t* active, T* Jc, int log_costs, T* Xlog, T* Ulog, T* Jcl,   \
      T* Ylog, T* Jtrace_log, T* Jm_log, int32_t* nelite_log, T* plan_log,     \
      T* std_log, void* stream) {                                              \
    return pddp::cem_trial_impl<T>(                                            \
        p,                                                                     \
        pddp::CemTrialArgs<T>{                                                 \
            B,           N,       S,          0,       K,        I,            \
            TT,          t0,      count,      table,   plant,    z0,           \
            U,           Z,       mean,       width,   Um,       Sm,           \
            u_min,       u_max,   sigma,      sigma0,  std_min,  T(0),         \
            T(0),        T(0),    seed,       cand_offset,       iter_stride,  \
            disturbance, w_std,   v_std,      rollout_offset,    step_offset,  \
            x_true,      active,  Jc,         log_costs,         Xlog,         \
            Ulog,        Jcl,     Ylog,       Jtrace_log,        Jm_log,       \
            nelite_log,  plan_log, std_log},                                   \
        smooth, mix, stream);                                                  \
  }

PDDP_CEM_TRIAL_ENTRY_POINT(f32, float)
PDDP_CEM_TRIAL_ENTRY_POINT(f64, double)
#undef PDDP_CEM_TRIAL_ENTRY_POINT

}  // extern "C"
