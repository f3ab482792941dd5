// shoot.hip - sampled shooting: S perturbed copies of every trajectory's action
// sequence rolled out open loop under the solver's model and cost, the
// cheapest found INSIDE the launch, and only that one's states and actions
// written (pddp_shoot_*, pddp_shoot_batch_*, ILQRSolver.shoot); the same under
// the line search's objective (pddp_shoot_track_*, _weighted_*,
// _track_weighted_*; objective="search"); the unit normals of the perturbation
// written out (pddp_shoot_draws_*).  The reference has no counterpart:
// include/pddp_hip.h states the law, DESIGN.md 3.4m, 3.4p and 3.4q the kernels.
//
//   candidate (b, s), r = sample_offset + b S + s:
//     xi_t = the m unit normals of (seed, r, t, stream 2)
//     e_0 = xi_0;  e_t = fma(beta, e_{t-1}, gamma xi_t)       AR(1), unit variance
//     u_t = clamp(fma(a_std, e_t, U[b][t]))   s >= 1;   clamp(U[b][t])   s == 0
//     J += l(x_t, u_t);  x_{t+1} = f_b(x_t, u_t);  J += l_f(x_N)
//   under the line search's objective:
//     P_b = the shared problem, the parameters of table row b where a table is
//           given (with a reference the table's goals are not read), then,
//           where weights are given, row b's diagonals over Q, Q_term, R
//     J += l(x_t, u_t) under reference row min(ref_t0 + t, ref_len - 1)
//     J += l_f(x_N)    under row min(ref_t0 + N, ref_len - 1), x_goal only
//
// Mapping, lane groups and the order in which a trajectory's costs meet are
// closed_loop.hip's (closed_loop_args.hpp); the draws are closed_loop_draws.hpp's
// as they are, stream 2.  Two kernels per model and type over ONE text
// (shoot_kernel_body.inc): shoot_kernel, whose table - the _batch entry
// points' - is a nullable kernel argument, as closed_loop_kernel's plant rows
// are; shoot_goals_kernel, whose `goals.ref` and `weights` are nullable kernel
// arguments tested under launch-uniform branches.  The reference row of step
// t + 1 is requested during step t with the next base action and the normals
// and held in registers; the weights row is written over P
// once, ahead of the turns.  The goal hooks and the weights row enclose no
// shuffle and no barrier.
//
// The winner is rolled out a SECOND time in the same launch: the lanes walk one
// loop of ceil(S / G) + 1 turns whose body is the rollout; the last turn starts
// with the argmin, after which the one lane that owned the winner runs the body
// again with `keep` set - the same instructions, their stores enabled by a
// run-time predicate - so Z_out / U_out are the rollout Jc[b][best] was summed
// over, whatever the compiler made of the body.  No [B][N][S][.] tensor exists
// and no rollout's states are held in registers or LDS beyond its own step.
#include "sampled_common.hpp"

namespace pddp {

template <typename T>
struct ShootArgs {
  int B, N, S, G;
  const T* z0;     // [B][n]
  const T* U;      // [B][N][m]
  const T* table;  // [B][PDDP_BATCH_ROW] or NULL: the shared problem
  const T* u_min;
  const T* u_max;
  const T* a_std;  // [m]
  T beta, gamma;
  uint64_t seed, offset;
  const uint8_t* active;
  T* Jc;          // [B][S]
  int32_t* best;  // [B]
  T* J_best;      // [B] or NULL
  T* Z_out;       // [B][N+1][n], with U_out [B][N][m]: both or neither
  T* U_out;
};

// The goals kernel's block: ShootArgs without `table` (RefArgs carries it) - a
// type of its own because the kernel's argument layout is.
template <typename T>
struct ShootGoalsArgs {
  int B, N, S, G;
  const T* z0;
  const T* U;
  const T* u_min;
  const T* u_max;
  const T* a_std;
  T beta, gamma;
  uint64_t seed, offset;
  const uint8_t* active;
  T* Jc;
  int32_t* best;
  T* J_best;
  T* Z_out;
  T* U_out;
};

#define PDDP_PROBLEM_OF_B PDDP_PLAIN_PROBLEM_OF_B
#define PDDP_ROW_OF_B PDDP_PLAIN_ROW_OF_B
#define PDDP_GOALS(point)
#define PDDP_SHOOT_ROWS_AHEAD
#define PDDP_SAMPLED_AFTER_E0 PDDP_SHOOT_ROWS
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void shoot_kernel(
    ProblemT<T> shared, ShootArgs<T> a) {
#include "shoot_kernel_body.inc"
}
#undef PDDP_SAMPLED_AFTER_E0
#undef PDDP_SHOOT_ROWS_AHEAD
#undef PDDP_GOALS
#undef PDDP_ROW_OF_B
#undef PDDP_PROBLEM_OF_B

#define PDDP_PROBLEM_OF_B PDDP_GOALS_PROBLEM_OF_B
#define PDDP_ROW_OF_B
#define PDDP_GOALS(point) PDDP_GOALS_##point
#define PDDP_SHOOT_ROWS_AHEAD PDDP_SHOOT_ROWS
#define PDDP_SAMPLED_AFTER_E0
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void shoot_goals_kernel(
    ProblemT<T> shared, ShootGoalsArgs<T> a, RefArgs<T> goals,
    const T* weights) {
#include "shoot_kernel_body.inc"
}
#undef PDDP_SAMPLED_AFTER_E0
#undef PDDP_SHOOT_ROWS_AHEAD
#undef PDDP_GOALS
#undef PDDP_ROW_OF_B
#undef PDDP_PROBLEM_OF_B

// ---- the unit normals written out ------------------------------------------

template <typename T>
struct ShootDrawArgs {
  int B, N, S, m;
  uint64_t seed, offset;
  T* E;  // [B][N][S][m]
};

// One lane per (b, t, s), s fastest, as closed_loop_draws_kernel.
template <typename T>
__global__ __launch_bounds__(kClosedLoopThreads) void shoot_draws_kernel(
    ShootDrawArgs<T> a) {
  constexpr int kPer = DrawBlock<T>::kPer;
  const size_t total = (size_t)a.B * a.N * a.S;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t bt = i / a.S;
    const int s = (int)(i - bt * a.S);
    const size_t b = bt / a.N;
    const int t = (int)(bt - b * a.N);
    const uint64_t r = a.offset + (uint64_t)b * a.S + s;
    T* out = a.E + i * a.m;
    for (int k = 0; k * kPer < a.m; ++k) {
      T z[kPer];
      draw_block(a.seed, r, t, kSampledStream, k, z);
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (k * kPer + j < a.m) out[k * kPer + j] = z[j];
    }
  }
}

// ---- host path ---------------------------------------------------------------

template <typename T, int MODEL>
static int launch_shoot(const pddp_problem& p, ShootArgs<T> a, hipStream_t st) {
  return launch_sampled<T>(shoot_kernel<T, MODEL>, p, a, st);
}

template <typename T, int MODEL>
static int launch_shoot_goals(const pddp_problem& p,
                              With<ShootGoalsArgs<T>, FormGoals<T>> w,
                              hipStream_t st) {
  return launch_sampled<T>(shoot_goals_kernel<T, MODEL>, p, w.a, st, w.x.goals,
                           w.x.weights);
}

// One impl and one argument test for the five entry-point families: what a
// form does not bring is null (goal_form.hpp).
template <typename T>
static int shoot_impl(const pddp_problem* p, const GoalForm<T>& f,
                      PDDP_SHOOT_PARAMS(T)) {
  if (B <= 0 || N <= 0 || S <= 0 || (long long)B * S > 0x7fffffffLL || !z0 ||
      !U || !a_std || !Jc || !best ||
      (Z_out == nullptr) != (U_out == nullptr) ||
      (U_out != nullptr && (U_out == U || Z_out == z0)) ||
      !(smooth >= 0.0 && smooth < 1.0))  // (NaN fails both)
    return PDDP_E_BADARG;
  With<ShootGoalsArgs<T>, FormGoals<T>> w{};
  if (!form_goals(f, &w.x)) return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  const T beta = (T)smooth, gamma = (T)std::sqrt(1.0 - smooth * smooth);
  if (f.goals) {
    w.a = ShootGoalsArgs<T>{B,      N,     S,     0,     z0,
                            U,      u_min, u_max, a_std, beta,
                            gamma,  seed,  sample_offset, active, Jc,
                            best,   J_best, Z_out, U_out};
    PDDP_DISPATCH_MODEL(launch_shoot_goals, T, p, w, (hipStream_t)stream)
  }
  const ShootArgs<T> a{B,     N,      S,     0,     z0,    U,     f.table,
                       u_min, u_max,  a_std, beta,  gamma, seed,  sample_offset,
                       active, Jc,    best,  J_best, Z_out, U_out};
  PDDP_DISPATCH_MODEL(launch_shoot, T, p, a, (hipStream_t)stream)
}

template <typename T>
static int shoot_draws_impl(int B, int N, int S, int m, uint64_t seed,
                            uint64_t sample_offset, T* E, void* stream) {
  if (B <= 0 || N <= 0 || S <= 0 || m <= 0 || m > PDDP_MAX_ACTION || !E)
    return PDDP_E_BADARG;
  const size_t total = (size_t)B * N * S;
  const size_t want = (total + kClosedLoopThreads - 1) / kClosedLoopThreads;
  const size_t cap = (size_t)1 << 20;  // (the kernel strides over the rest)
  const dim3 blocks((unsigned)(want < cap ? want : cap));
  PDDP_LAUNCH((shoot_draws_kernel<T>), blocks, dim3(kClosedLoopThreads), 0,
              (hipStream_t)stream,
              (ShootDrawArgs<T>{B, N, S, m, seed, sample_offset, E}));
  return launch_status();
}

}  // namespace pddp

extern "C" {

#define PDDP_SHOOT_ENTRY_POINTS(SUF, T)                                        \
  PDDP_FORM_ENTRY_POINTS(shoot, SUF, T, PDDP_SHOOT_PARAMS, PDDP_SHOOT_ARGS) \
  int pddp_shoot_draws_##SUF(int B, int N, int S, int m, uint64_t seed,        \
                             uint64_t sample_offset, T* E, void* stream) {     \
    return pddp::shoot_draws_impl<T>(B, N, S, m, seed, sample_offset, E,       \
                                     stream);                                  \
  }

PDDP_SHOOT_ENTRY_POINTS(f32, float)
PDDP_SHOOT_ENTRY_POINTS(f64, double)
#undef PDDP_SHOOT_ENTRY_POINTS

}  // extern "C"
