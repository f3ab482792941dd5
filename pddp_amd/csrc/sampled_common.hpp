// sampled_common.hpp - what the sampling planners share (shoot.hip, mppi.hip,
// mppi_trial.hip, cem.hip, cem_trial.hip):
// the draws' stream, the order of an argmin and of a ranking, the softmin
// weight, the sum over a lane group, the hand-over inside a launch, the hooks
// through which a family's ONE kernel text (*_kernel_body.inc) reaches the
// problem of trajectory b - the plain kernel's table row, or the goals kernel's
// reference and weights -, a plain trial's plant hooks, and the host path's
// common pieces, the trials' argument test among them.
#pragma once

#include <climits>
#include <cmath>
#include <limits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "ref_args.hpp"
#include "goal_form.hpp"
#include "closed_loop_args.hpp"
#include "closed_loop_draws.hpp"

namespace pddp {

constexpr int kSampledStream = 2;  // (0 process, 1 measurement: closed_loop.hip)

// (J, s) ordered lexicographically; (+inf, -1) is "no finite cost" and loses
// against every candidate, whose J is finite.
template <typename T>
PDDP_DEV void take_lower(T& J, int& s, T oJ, int os) {
  const bool take = oJ < J || (oJ == J && os < s);
  J = take ? oJ : J;
  s = take ? os : s;
}

PDDP_DEV float exp_of(float x) { return expf(x); }
PDDP_DEV double exp_of(double x) { return exp(x); }
PDDP_DEV float sqrt_of(float x) { return sqrtf(x); }
PDDP_DEV double sqrt_of(double x) { return sqrt(x); }

// w_s: 1 for the best candidate (the exponent is -0), 0 for a cost that is
// not finite.  The difference and the quotient are rounded one by one.
template <typename T>
PDDP_DEV T softmin_weight(T J, T J_best, T lam) {
  const T arg = -((J - J_best) / lam);
  return is_finite(J) ? exp_of(arg) : T(0);
}

// The sums of v[0..K) over a trajectory's lane group, on every lane of the
// group: the butterfly, then (one trajectory over several wavefronts) the
// wavefronts in their order through `part` [K][waves], read by every lane
// after ONE barrier.  The caller alternates between two `part` blocks from one
// sum to the next, so a wavefront that runs ahead writes the block nobody
// still reads.
template <typename T, int K>
PDDP_DEV void group_sum(T (&v)[K], int span, bool multi,
                        T (&part)[K][kClosedLoopThreads / kWave]) {
  for (int off = 1; off < span; off <<= 1) {
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] += __shfl_xor(v[j], off);
  }
  if (multi) {
    const int tid = threadIdx.x;
    if (tid % kWave == 0) {
#pragma unroll
      for (int j = 0; j < K; ++j) part[j][tid / kWave] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < K; ++j) {
      v[j] = part[j][0];
      for (int w = 1; w < (int)blockDim.x / kWave; ++w) v[j] += part[j][w];
    }
  }
}

// Between the head's stores to z0[b] / U[b] and the group's loads of them: the
// storing wavefront waits for its stores, then the workgroup meets at the
// barrier, whose fence keeps the compiler from moving the loads ahead of it.
// A workgroup's wavefronts share their CU's L1: workgroup scope is enough.
PDDP_DEV void hand_over() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// ---- the hooks of the kernel texts --------------------------------------------
// A kernel defines, ahead of its #include of the family's text,
//   PDDP_PROBLEM_OF_B     first statement: P, the problem of trajectory b
//   PDDP_ROW_OF_B         inside the `if (live)` that loads the bounds: the
//                         plain kernel's table row; empty in the goals kernel,
//                         whose PDDP_PROBLEM_OF_B has written it.  (The two
//                         places are what the two kernels were compiled from:
//                         a hook for the statement's place alone.)
//   PDDP_GOALS(point)     sampled_rollout_body.inc's; empty in a plain kernel
// and #undefs them behind it.
//
// The plain kernels (`a.table` nullable: the _batch entry points' table).  The
// row as statements, as shoot.hip wrote it, not write_params_and_goals: the
// same statements inlined from a function reach the optimiser in another order
// (ref_args.hpp's note), and shoot's and mppi's kernels were compiled from
// these; the trial's from the function, mppi_trial.hip.
#define PDDP_PLAIN_PROBLEM_OF_B ProblemT<T> P = shared;
#define PDDP_PLAIN_ROW_OF_B                                                    \
  if (a.table != nullptr) {                                                    \
    const T* row = a.table + (size_t)b * PDDP_BATCH_ROW;                       \
    P.dt = row[PDDP_BATCH_PARAMS];                                             \
    PDDP_COPY(kModelParamCount<MODEL> - 1, P.p, row + PDDP_BATCH_PARAMS + 1)   \
    PDDP_COPY(D::na, P.goal, row + PDDP_BATCH_X_GOAL)                          \
    PDDP_COPY(D::m, P.ugoal, row + PDDP_BATCH_U_GOAL)                          \
  }
// The goals kernels.  `goals` (RefArgs: table, ref, ref_len, ref_t0; ref NULL
// without a reference) and `weights` (NULL without) are the launch's.  P: the
// shared problem, row b of the table (its goals only where no reference
// supplies them), row b of the weights.  `tracked` is uniform over the
// launch.  (PDDP_GOALS_P_OF_B apart: the trial forms `tracked` from its
// `window` ahead of `goals`, mppi_trial.hip - statement order alone.)
#define PDDP_GOALS_PROBLEM_OF_B                                               \
  const bool tracked = goals.ref != nullptr;                                   \
  PDDP_GOALS_P_OF_B
#define PDDP_GOALS_P_OF_B                                                      \
  ProblemT<T> P = shared;                                                      \
  if (live) {                                                                  \
    if (goals.table != nullptr) {                                              \
      const T* trow = goals.table + (size_t)b * PDDP_BATCH_ROW;                \
      if (tracked)                                                             \
        write_params<T, MODEL>(P, trow);                                       \
      else                                                                     \
        write_params_and_goals<T, MODEL>(P, trow);                             \
    }                                                                          \
    if (weights != nullptr)                                                    \
      write_weights<T, MODEL>(P, weights + (size_t)b * PDDP_WEIGHT_ROW);       \
  }
// track_goal_hooks.inc's line-search hooks with a nullable reference: without
// one the "next row" is the goals P holds.  #define PDDP_GOALS(point)
// PDDP_GOALS_##point.
#define PDDP_GOALS_TAKE_FIRST                                                  \
  if (tracked) {                                                               \
    const T* row0 = ref_row(goals, b, 0);                                      \
    PDDP_COPY(D::na, P.goal, row0 + PDDP_REF_X_GOAL)                           \
    PDDP_COPY(m, P.ugoal, row0 + PDDP_REF_U_GOAL)                              \
  }
#define PDDP_GOALS_REQUEST_NEXT                                                \
  T xg2[D::na], ug2[m];                                                        \
  PDDP_COPY(D::na, xg2, P.goal)                                                \
  PDDP_COPY(m, ug2, P.ugoal)                                                   \
  if (tracked) {                                                               \
    const T* row = ref_row(goals, b, t + 1);                                   \
    PDDP_COPY(D::na, xg2, row + PDDP_REF_X_GOAL)                               \
    PDDP_COPY(m, ug2, row + PDDP_REF_U_GOAL)                                   \
  }
#define PDDP_GOALS_TAKE_NEXT                                                   \
  PDDP_COPY(m, P.ugoal, ug2)                                                   \
  PDDP_COPY(D::na, P.goal, xg2)

// sampled_rollout_body.inc's width hooks for a width per time step (cem.hip,
// cem_trial.hip): `Sb` is the trajectory's [N][m] rows; the width of step t in
// `sg`, that of step t + 1 requested next to `ur2`.  With them a kernel defines
// PDDP_SAMPLED_WIDTH(r) as sg[r].
#define PDDP_WIDTH_ROWS_AFTER_E0                                               \
  T sg[m], sg2[m];                                                             \
  PDDP_COPY(m, sg2, Sb)
#define PDDP_WIDTH_ROWS_REQUEST                                                \
  _Pragma("unroll") for (int j = 0; j < m; ++j) {                              \
    sg[j] = sg2[j];                                                            \
    sg2[j] = Sb[tn * m + j];                                                   \
  }

// trial_plant_body.inc's hooks in a plain trial kernel (mppi_trial_kernel,
// cem_trial_kernel): the applied step is logged under the controller's model
// with row b of the plant table written over it, goals included, and the
// terminal cost under the same goals.
#define PDDP_PLAIN_TRIAL_PLANT_PROBLEM                                         \
  ProblemT<T> Pl = P;                                                          \
  if (a.plant != nullptr)                                                      \
    write_params_and_goals<T, MODEL>(Pl, a.plant + (size_t)b * PDDP_BATCH_ROW);
#define PDDP_PLAIN_TRIAL_TERMINAL_GOAL

// ---- host path -----------------------------------------------------------------

// (GoalForm, FormGoals, form_goals: goal_form.hpp)

// The mapping is closed_loop's: its geometry.  Sets a.G.
template <typename Args>
static dim3 sampled_geometry(Args& a, int* threads) {
  ClosedLoopArgs<float> g{};
  g.B = a.B;
  g.S = a.S;
  dim3 blocks;
  *threads = closed_loop_geometry(g, blocks);
  a.G = g.G;
  return blocks;
}

// One launcher for the six kernels: `extra` are the goals kernel's trailing
// arguments, none for a plain kernel.
template <typename T, typename Args, typename... Extra>
static int launch_sampled(void (*kernel)(ProblemT<T>, Args, Extra...),
                          const pddp_problem& p, Args a, hipStream_t st,
                          Extra... extra) {
  const ProblemT<T> P = convert_problem<T>(p);
  int threads;
  const dim3 blocks = sampled_geometry(a, &threads);
  PDDP_LAUNCH(kernel, blocks, dim3(threads), 0, st, P, a, extra...);
  return launch_status();
}

// What the blocks of the two trials (MppiTrialArgs, MppiTrialGoalsArgs,
// CemTrialArgs) share: false where a shared field refuses the call.  What is a
// trial's own - K, its work buffers, its widths - its impl tests itself.
template <typename Args>
static bool check_trial_args(const Args& a, double smooth) {
  return a.B > 0 && a.N > 0 && a.S > 0 &&
         (long long)a.B * a.S <= 0x7fffffffLL && a.z0 && a.U && a.Jc &&
         smooth >= 0.0 && smooth < 1.0 &&  // (NaN fails both)
         a.TT >= 1 && a.t0 >= 0 && a.count >= 1 &&
         (long long)a.t0 + a.count <= a.TT && a.Z && a.Xlog && a.Ulog &&
         a.Jcl && (a.v_std == nullptr || a.x_true != nullptr) &&
         // (step_offset + c + 1 is a counter word of the draws: an int)
         a.step_offset >= 0 && a.step_offset <= INT_MAX - a.TT;
}

// The AR(1) of the draws; without measurement noise the plant's state is the
// controller's and there is nothing to observe.
template <typename T, typename Args>
static void set_trial_noise(Args& a, double smooth) {
  a.beta = (T)smooth;
  a.gamma = (T)std::sqrt(1.0 - smooth * smooth);
  if (a.v_std == nullptr) a.x_true = a.Ylog = nullptr;
}

}  // namespace pddp

// The parameters the entry points of shoot and of mppi share, and their names.
#define PDDP_SHOOT_PARAMS(T)                                                   \
  int B, int N, int S, const T* z0, const T* U, const T* u_min,                \
      const T* u_max, const T* a_std, double smooth, uint64_t seed,            \
      uint64_t sample_offset, const uint8_t* active, T* Jc, int32_t* best,     \
      T* J_best, T* Z_out, T* U_out, void* stream
#define PDDP_SHOOT_ARGS                                                        \
  B, N, S, z0, U, u_min, u_max, a_std, smooth, seed, sample_offset, active,    \
      Jc, best, J_best, Z_out, U_out, stream
#define PDDP_MPPI_PARAMS(T)                                                    \
  int B, int N, int S, const T* z0, const T* U, const T* u_min,                \
      const T* u_max, const T* a_std, const T* lam, double smooth,             \
      uint64_t seed, uint64_t sample_offset, const uint8_t* active, T* Jc,     \
      int32_t* best, T* J_best, T* W, T* J_w, T* Z_out, T* U_out, void* stream
#define PDDP_MPPI_ARGS                                                         \
  B, N, S, z0, U, u_min, u_max, a_std, lam, smooth, seed, sample_offset,       \
      active, Jc, best, J_best, W, J_w, Z_out, U_out, stream
// (cem: K after S; sigma [B][N][m] in a_std's place, std_min [m] behind it;
// mix next to smooth; rank, n_elite, J_m and the third row output S_out)
#define PDDP_CEM_PARAMS(T)                                                     \
  int B, int N, int S, int K, const T* z0, const T* U, const T* u_min,         \
      const T* u_max, const T* sigma, const T* std_min, double smooth,         \
      double mix, uint64_t seed, uint64_t sample_offset,                       \
      const uint8_t* active, T* Jc, int32_t* rank, int32_t* best, T* J_best,   \
      int32_t* n_elite, T* J_m, T* Z_out, T* U_out, T* S_out, void* stream
#define PDDP_CEM_ARGS                                                          \
  B, N, S, K, z0, U, u_min, u_max, sigma, std_min, smooth, mix, seed,          \
      sample_offset, active, Jc, rank, best, J_best, n_elite, J_m, Z_out,      \
      U_out, S_out, stream
// (the five entry points of one family: PDDP_FORM_ENTRY_POINTS, goal_form.hpp)
