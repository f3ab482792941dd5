// cem.hip - sampled shooting with a cross-entropy (CEM) refit: shoot.hip's S
// candidates per trajectory, drawn with a width per time step and action
// component (sigma [B][N][m]) around the mean U, costed by the same law, the K
// cheapest ("elites") found inside the launch, and the mean AND the width
// refitted to them; the new mean is rolled out and costed in the same launch
// (pddp_cem_*, pddp_cem_batch_*, ILQRSolver.cem); the same under the line
// search's objective (pddp_cem_track_*, _weighted_*, _track_weighted_*;
// objective="search": shoot.hip's header has the law).  The reference has no
// counterpart: include/pddp_hip.h states the law, DESIGN.md 3.4s the kernels.
//
//   Jc[b][s]      pddp_shoot_*'s, with sigma[b][t][j] in a_std[j]'s place
//   rank[b][s]    the number of finite (Jc, s') lexicographically below
//                 (Jc[b][s], s); -1 for a cost that is not finite
//   elite(s)      0 <= rank < K;  Ke = min(K, finite costs);  best: rank 0
//   s1, s2        the sums of e and of e e (rounded) over the elites s >= 1,
//                 e the raw AR(1) value: of unit scale whatever sigma is
//   ebar = s1 / Ke;  V = max(s2 / Ke - ebar^2, 0)   (0 with Ke == 1)
//   Um = clamp(fma(step sigma, ebar, U));  Sm = max(sigma + step (sigma
//        sqrt(V) - sigma), std_min);  Zm, J_m: Um's rollout and its cost
//
// The candidate rollout is the family's one text (sampled_rollout_body.inc)
// through its width hook; the sums are sampled_common.hpp's group_sum.  Two
// kernels per model and type over ONE text (cem_kernel_body.inc), with
// mppi_kernel's mapping: cem_kernel with its nullable table, cem_goals_kernel
// with its nullable reference and weights.  Passes 2 and 3 are texts of their
// own, which the trial's kernel includes too (cem_rank_body.inc,
// cem_refit_body.inc; cem_trial.hip).
//
// Three passes over the same ceil(S / G) turns of the lane group:
//   1. the candidates' rollouts, row t + 1 of sigma[b] requested a step ahead;
//   2. the ranks: every lane counts, per own candidate, the finite (J, s')
//      below it - the S costs of its trajectory pass through LDS a chunk of G
//      at a time, each staged by the lane that wrote it.  Exact integer work;
//      best, J_best, n_elite and rank are written here, and the elite of the
//      highest rank is handed to the group through LDS: in pass 3 a lane knows
//      an elite by comparing its own (J, s) with that one;
//   3. the draws again for the elites alone - Philox and the AR(1), no
//      dynamics: at every step t the 2m values (e, e e) are summed over the
//      group, the turns in their order by ONE lane per trajectory, which in
//      the last turn has the whole sums, forms Um[b][t] and Sm[b][t] and steps
//      the mean's rollout - in the goals kernel under row ref_t0 + t of the
//      reference, its terminal term under row ref_t0 + N.
// Every shuffle and barrier sits under launch-uniform control flow: the turn
// count, N and m are uniform, lanes outside the batch, masked or without an
// elite take part with zeros.  The order of every sum and of the ranking
// depends on S alone, never on b or B.  No atomics.
#include "sampled_common.hpp"

namespace pddp {

template <typename T>
struct CemArgs {
  int B, N, S, G, K;
  const T* z0;       // [B][n]
  const T* U;        // [B][N][m]: the mean
  const T* table;    // [B][PDDP_BATCH_ROW] or NULL: the shared problem
  const T* u_min;
  const T* u_max;
  const T* sigma;    // [B][N][m]
  const T* std_min;  // [m] or NULL: zeros
  T beta, gamma, step;
  uint64_t seed, offset;
  const uint8_t* active;
  T* Jc;             // [B][S]
  int32_t* rank;     // [B][S] or NULL
  int32_t* best;     // [B]
  T* J_best;         // [B] or NULL
  int32_t* n_elite;  // [B]
  T* J_m;            // [B]
  T* Z_out;          // [B][N+1][n], with U_out and S_out [B][N][m]: all or none
  T* U_out;
  T* S_out;
};

// The goals kernel's block: CemArgs without `table` (RefArgs carries it) - a
// type of its own because the kernel's argument layout is.
template <typename T>
struct CemGoalsArgs {
  int B, N, S, G, K;
  const T* z0;
  const T* U;
  const T* u_min;
  const T* u_max;
  const T* sigma;
  const T* std_min;
  T beta, gamma, step;
  uint64_t seed, offset;
  const uint8_t* active;
  T* Jc;
  int32_t* rank;
  int32_t* best;
  T* J_best;
  int32_t* n_elite;
  T* J_m;
  T* Z_out;
  T* U_out;
  T* S_out;
};

// (the width per step: sampled_common.hpp's PDDP_WIDTH_ROWS_* over `Sb`)
#define PDDP_SAMPLED_AFTER_E0 PDDP_WIDTH_ROWS_AFTER_E0
#define PDDP_SAMPLED_WIDTH_REQUEST PDDP_WIDTH_ROWS_REQUEST
#define PDDP_SAMPLED_WIDTH(r) sg[r]
#define PDDP_SAMPLED_KEEP_ROW

#define PDDP_PROBLEM_OF_B PDDP_PLAIN_PROBLEM_OF_B
#define PDDP_ROW_OF_B PDDP_PLAIN_ROW_OF_B
#define PDDP_GOALS(point)
#define PDDP_CEM_CUT_J Jcut
#define PDDP_CEM_FLOOR(r) smin[r]
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void cem_kernel(
    ProblemT<T> shared, CemArgs<T> a) {
#include "cem_kernel_body.inc"
}
#undef PDDP_CEM_FLOOR
#undef PDDP_CEM_CUT_J
#undef PDDP_GOALS
#undef PDDP_ROW_OF_B
#undef PDDP_PROBLEM_OF_B

#define PDDP_PROBLEM_OF_B PDDP_GOALS_PROBLEM_OF_B
#define PDDP_ROW_OF_B
#define PDDP_GOALS(point) PDDP_GOALS_##point
// (The goals every lane carries through pass 3 take the float64 double
// cartpole and rendezvous past 256 registers; with the cut's cost and the
// floor held across the passes as well, four vector registers spill.  Here
// both are read again where pass 3 uses them - the same words: cut_J[] is not
// written after pass 2's last barrier - and nothing spills.)
#define PDDP_CEM_CUT_J (ok ? cut_J[group] : Jcut)
#define PDDP_CEM_FLOOR(r) (a.std_min != nullptr ? a.std_min[r] : smin[r])
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void cem_goals_kernel(
    ProblemT<T> shared, CemGoalsArgs<T> a, RefArgs<T> goals,
    const T* weights) {
#include "cem_kernel_body.inc"
}
#undef PDDP_CEM_FLOOR
#undef PDDP_CEM_CUT_J
#undef PDDP_GOALS
#undef PDDP_ROW_OF_B
#undef PDDP_PROBLEM_OF_B

#undef PDDP_SAMPLED_KEEP_ROW
#undef PDDP_SAMPLED_WIDTH
#undef PDDP_SAMPLED_WIDTH_REQUEST
#undef PDDP_SAMPLED_AFTER_E0

// ---- host path ---------------------------------------------------------------

template <typename T, int MODEL>
static int launch_cem(const pddp_problem& p, CemArgs<T> a, hipStream_t st) {
  return launch_sampled<T>(cem_kernel<T, MODEL>, p, a, st);
}

template <typename T, int MODEL>
static int launch_cem_goals(const pddp_problem& p,
                            With<CemGoalsArgs<T>, FormGoals<T>> w,
                            hipStream_t st) {
  return launch_sampled<T>(cem_goals_kernel<T, MODEL>, p, w.a, st, w.x.goals,
                           w.x.weights);
}

// One impl and one argument test for the five entry-point families: what a
// form does not bring is null (goal_form.hpp).
template <typename T>
static int cem_impl(const pddp_problem* p, const GoalForm<T>& f,
                    PDDP_CEM_PARAMS(T)) {
  const bool rows = Z_out != nullptr;
  if (B <= 0 || N <= 0 || S <= 0 || (long long)B * S > 0x7fffffffLL || !z0 ||
      !U || !sigma || !Jc || !best || !n_elite || !J_m || K < 1 || K > S ||
      rows != (U_out != nullptr) || rows != (S_out != nullptr) ||
      (rows && (U_out == U || S_out == sigma || Z_out == z0)) ||
      // (a lane with more than one turn keeps the running sums in the rows)
      (!rows && S > kClosedLoopThreads) ||
      !(smooth >= 0.0 && smooth < 1.0) ||  // (NaN fails both)
      !(mix >= 0.0 && mix < 1.0))
    return PDDP_E_BADARG;
  With<CemGoalsArgs<T>, FormGoals<T>> w{};
  if (!form_goals(f, &w.x)) return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  const T beta = (T)smooth, gamma = (T)std::sqrt(1.0 - smooth * smooth);
  const T step = (T)(1.0 - mix);
  if (f.goals) {
    w.a = CemGoalsArgs<T>{B,     N,      S,     0,     K,       z0,
                          U,     u_min,  u_max, sigma, std_min, beta,
                          gamma, step,   seed,  sample_offset,  active,
                          Jc,    rank,   best,  J_best, n_elite, J_m,
                          Z_out, U_out,  S_out};
    PDDP_DISPATCH_MODEL(launch_cem_goals, T, p, w, (hipStream_t)stream)
  }
  const CemArgs<T> a{B,      N,     S,       0,     K,     z0,    U,
                     f.table, u_min, u_max,  sigma, std_min, beta, gamma,
                     step,   seed,  sample_offset, active, Jc,    rank,
                     best,   J_best, n_elite, J_m,  Z_out, U_out, S_out};
  PDDP_DISPATCH_MODEL(launch_cem, T, p, a, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

PDDP_FORM_ENTRY_POINTS(cem, f32, float, PDDP_CEM_PARAMS, PDDP_CEM_ARGS)
PDDP_FORM_ENTRY_POINTS(cem, f64, double, PDDP_CEM_PARAMS, PDDP_CEM_ARGS)

}  // extern "C"
