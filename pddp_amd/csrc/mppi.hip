// mppi.hip - sampled shooting with a softmin-weighted (MPPI) update of the base
// sequence: shoot.hip's S perturbed candidates per trajectory, costed by the
// same law, and instead of the single cheapest one the weighted mean of ALL the
// perturbations added to the base, that sequence rolled out and costed inside
// the launch (pddp_mppi_*, pddp_mppi_batch_*, ILQRSolver.mppi); the same under
// the line search's objective (pddp_mppi_track_*, _weighted_*,
// _track_weighted_*; objective="search": shoot.hip's header has the law).  The
// reference has no counterpart: include/pddp_hip.h states the law, DESIGN.md
// 3.4n, 3.4p and 3.4q the kernels.
//
//   Jc[b][s], best[b], J_best[b]:  pddp_shoot_*'s, word for word
//   w_s   = exp(-(Jc[b][s] - J_best[b]) / lam[b])   finite Jc, else 0
//   eta   = sum_s w_s;   W[b][s] = w_s / eta
//   ebar_t = (sum_{s>=1} w_s e_{s,t}) / eta         e: the raw AR(1) value
//   Uw[b][t] = clamp(fma(a_std, ebar_t, U[b][t]));  Zw, J_w: its rollout
//
// The candidate rollout, the argmin, the weight and the sums are shoot.hip's
// and mppi_trial.hip's: one text each (sampled_rollout_body.inc,
// sampled_argmin.inc, sampled_common.hpp; included texts, not device
// functions - the Makefile's note on contraction).  Two kernels per model and
// type over ONE text (mppi_kernel_body.inc): mppi_kernel with its nullable
// table, mppi_goals_kernel with its nullable reference and weights.
//
// Three passes over the same ceil(S / G) turns of the lane group:
//   1. the candidates' rollouts and the argmin - shoot's;
//   2. eta: every lane re-reads its own Jc and sums its weights in s order,
//      then the group (below);
//   3. the draws again - Philox and the AR(1), no dynamics: at every step t
//      the m products w_s e_{s,t} are summed over the group, the turns in
//      their order by ONE lane per trajectory, which in the last turn has the
//      whole sum, forms Uw[b][t] and steps the weighted rollout with it
//      (mppi_update_body.inc, the trial's text too).
// A sum over the group: a butterfly over the group's lanes of a wavefront
// (both partners form the same sum, idle lanes add 0), then the workgroup's
// wavefronts in their order through LDS.  Every shuffle and barrier sits under
// launch-uniform control flow: the turn count, N and m are uniform, lanes
// outside the batch, masked or without a weight take part with zeros.  The
// order depends on S alone, never on b or B.  No atomics.
#include "sampled_common.hpp"

namespace pddp {

template <typename T>
struct MppiArgs {
  int B, N, S, G;
  const T* z0;     // [B][n]
  const T* U;      // [B][N][m]
  const T* table;  // [B][PDDP_BATCH_ROW] or NULL: the shared problem
  const T* u_min;
  const T* u_max;
  const T* a_std;  // [m]
  const T* lam;    // [B]
  T beta, gamma;
  uint64_t seed, offset;
  const uint8_t* active;
  T* Jc;          // [B][S]
  int32_t* best;  // [B]
  T* J_best;      // [B] or NULL
  T* W;           // [B][S] or NULL
  T* J_w;         // [B]
  T* Z_out;       // [B][N+1][n], with U_out [B][N][m]: both or neither
  T* U_out;
};

// The goals kernel's block: MppiArgs without `table` (RefArgs carries it) - a
// type of its own because the kernel's argument layout is.
template <typename T>
struct MppiGoalsArgs {
  int B, N, S, G;
  const T* z0;
  const T* U;
  const T* u_min;
  const T* u_max;
  const T* a_std;
  const T* lam;
  T beta, gamma;
  uint64_t seed, offset;
  const uint8_t* active;
  T* Jc;
  int32_t* best;
  T* J_best;
  T* W;
  T* J_w;
  T* Z_out;
  T* U_out;
};

#define PDDP_SAMPLED_AFTER_E0
#define PDDP_SAMPLED_KEEP_ROW

#define PDDP_PROBLEM_OF_B PDDP_PLAIN_PROBLEM_OF_B
#define PDDP_ROW_OF_B PDDP_PLAIN_ROW_OF_B
#define PDDP_GOALS(point)
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void mppi_kernel(
    ProblemT<T> shared, MppiArgs<T> a) {
#include "mppi_kernel_body.inc"
}
#undef PDDP_GOALS
#undef PDDP_ROW_OF_B
#undef PDDP_PROBLEM_OF_B

#define PDDP_PROBLEM_OF_B PDDP_GOALS_PROBLEM_OF_B
#define PDDP_ROW_OF_B
#define PDDP_GOALS(point) PDDP_GOALS_##point
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void mppi_goals_kernel(
    ProblemT<T> shared, MppiGoalsArgs<T> a, RefArgs<T> goals,
    const T* weights) {
#include "mppi_kernel_body.inc"
}
#undef PDDP_GOALS
#undef PDDP_ROW_OF_B
#undef PDDP_PROBLEM_OF_B

#undef PDDP_SAMPLED_KEEP_ROW
#undef PDDP_SAMPLED_AFTER_E0

// ---- host path ---------------------------------------------------------------

template <typename T, int MODEL>
static int launch_mppi(const pddp_problem& p, MppiArgs<T> a, hipStream_t st) {
  return launch_sampled<T>(mppi_kernel<T, MODEL>, p, a, st);
}

template <typename T, int MODEL>
static int launch_mppi_goals(const pddp_problem& p,
                             With<MppiGoalsArgs<T>, FormGoals<T>> w,
                             hipStream_t st) {
  return launch_sampled<T>(mppi_goals_kernel<T, MODEL>, p, w.a, st, w.x.goals,
                           w.x.weights);
}

// One impl and one argument test for the five entry-point families: what a
// form does not bring is null (goal_form.hpp).
template <typename T>
static int mppi_impl(const pddp_problem* p, const GoalForm<T>& f,
                     PDDP_MPPI_PARAMS(T)) {
  if (B <= 0 || N <= 0 || S <= 0 || (long long)B * S > 0x7fffffffLL || !z0 ||
      !U || !a_std || !lam || !Jc || !best || !J_w ||
      (Z_out == nullptr) != (U_out == nullptr) ||
      (U_out != nullptr && (U_out == U || Z_out == z0)) ||
      // (a lane with more than one turn keeps the running sum in U_out)
      (U_out == nullptr && S > kClosedLoopThreads) ||
      !(smooth >= 0.0 && smooth < 1.0))  // (NaN fails both)
    return PDDP_E_BADARG;
  With<MppiGoalsArgs<T>, FormGoals<T>> w{};
  if (!form_goals(f, &w.x)) return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  const T beta = (T)smooth, gamma = (T)std::sqrt(1.0 - smooth * smooth);
  if (f.goals) {
    w.a = MppiGoalsArgs<T>{B,     N,     S,      0,     z0,   U,
                           u_min, u_max, a_std,  lam,   beta, gamma,
                           seed,  sample_offset, active, Jc,  best,
                           J_best, W,    J_w,    Z_out, U_out};
    PDDP_DISPATCH_MODEL(launch_mppi_goals, T, p, w, (hipStream_t)stream)
  }
  const MppiArgs<T> a{B,       N,     S,     0,      z0,   U,
                      f.table, u_min, u_max, a_std,  lam,  beta,
                      gamma,   seed,  sample_offset, active, Jc, best,
                      J_best,  W,     J_w,   Z_out,  U_out};
  PDDP_DISPATCH_MODEL(launch_mppi, T, p, a, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

PDDP_FORM_ENTRY_POINTS(mppi, f32, float, PDDP_MPPI_PARAMS, PDDP_MPPI_ARGS)
PDDP_FORM_ENTRY_POINTS(mppi, f64, double, PDDP_MPPI_PARAMS, PDDP_MPPI_ARGS)

}  // extern "C"
