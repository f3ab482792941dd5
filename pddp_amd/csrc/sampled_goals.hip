// sampled_goals.hip - the sampling planners under the line search's objective:
// shoot.hip's, mppi.hip's and mppi_trial.hip's laws with every rollout summed
// along a reference (a goal per time step, tracking.hip) and / or under the
// diagonals of Q, Q_term and R of trajectory b (weights.hip) - the
// pddp_shoot_* / pddp_mppi_* entry points with the suffixes _track, _weighted,
// _track_weighted and pddp_mppi_trial_goals_*; ILQRSolver.shoot / mppi /
// mppi_closed_loop with objective="search".  The reference has no
// counterpart: include/pddp_hip.h states the laws, DESIGN.md 3.4p the kernels.
//
//   P_b = the shared problem, the parameters of table row b where a table is
//         given (with a reference the table's goals are not read), then, where
//         weights are given, row b's diagonals written over Q, Q_term, R
//   J += l(x_t, u_t) under reference row min(ref_t0 + t, ref_len - 1)
//   J += l_f(x_N)    under row min(ref_t0 + N, ref_len - 1), x_goal only
//
// Drawing, clamping, selecting, weighting and summing are the siblings', word
// for word, and so are the mapping (closed_loop_geometry), the lane groups,
// the order of every argmin and sum, the turns and the hand-over points.
// shoot.hip, mppi.hip, mppi_trial.hip and their texts are as they were: this
// unit carries its own copies (the Makefile's note on contraction).
//
// ONE kernel per family, model and type: `goals.ref` and `weights` are
// nullable kernel arguments, tested under launch-uniform branches; the
// suffixed entry points are fronts over it.  The candidate rollout is ONE
// included text (sampled_rollout_body.inc) in all three kernels.  The
// reference row of step t + 1 is requested during step t with the next base
// action and the normals and held in registers; the weights
// row is written over P once, ahead of the turns.  Every shuffle and barrier
// sits under the control flow it sits under in the sibling: the goal hooks
// and the weights row enclose none.
#include <climits>
#include <cmath>
#include <limits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "ref_args.hpp"
#include "closed_loop_args.hpp"
#include "closed_loop_draws.hpp"

namespace pddp {

constexpr int kSampledStream = 2;  // (shoot's: the candidates are shoot's)

// shoot.hip's take_lower: (J, s) ordered lexicographically; (+inf, -1) is "no
// finite cost" and loses against every candidate, whose J is finite.
template <typename T>
PDDP_DEV void goals_take_lower(T& J, int& s, T oJ, int os) {
  const bool take = oJ < J || (oJ == J && os < s);
  J = take ? oJ : J;
  s = take ? os : s;
}

PDDP_DEV float goals_exp(float x) { return expf(x); }
PDDP_DEV double goals_exp(double x) { return exp(x); }

// mppi.hip's softmin_weight.
template <typename T>
PDDP_DEV T goals_weight(T J, T J_best, T lam) {
  const T arg = -((J - J_best) / lam);
  return is_finite(J) ? goals_exp(arg) : T(0);
}

// mppi.hip's group_sum: the sums of v[0..K) over a trajectory's lane group,
// on every lane of the group.
template <typename T, int K>
PDDP_DEV void goals_group_sum(T (&v)[K], int span, bool multi,
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

// mppi_trial.hip's hand_over: the storing wavefront waits for its stores, then
// the workgroup meets at the barrier.
PDDP_DEV void goals_hand_over() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// For the three kernels below.  `goals` (RefArgs: table, ref, ref_len, ref_t0;
// ref NULL without a reference) and `weights` (NULL without) are the launch's;
// `tracked` = goals.ref != nullptr.  P: the shared problem, row b of the table
// (its goals only where no reference supplies them), row b of the weights.
#define PDDP_PROBLEM_OF_B                                                      \
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
// one the "next row" is the goals P holds.
#define PDDP_GOALS(point) PDDP_GOALS_##point
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
#define PDDP_SAMPLED_STREAM kSampledStream

// ---- shoot -------------------------------------------------------------------

template <typename T>
struct ShootGoalsArgs {
  int B, N, S, G;
  const T* z0;  // [B][n]
  const T* U;   // [B][N][m]
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

// shoot_kernel (shoot.hip) with the objective above: ceil(S / G) + 1 turns,
// the last one the argmin and the winner again with its rows kept.
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void shoot_goals_kernel(
    ProblemT<T> shared, ShootGoalsArgs<T> a, RefArgs<T> goals,
    const T* weights) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  const int tid = threadIdx.x, G = a.G, N = a.N, S = a.S;
  const int group = tid / G, lane = tid - group * G;
  const long long bl = (long long)blockIdx.x * (blockDim.x / G) + group;
  const bool in_batch = bl < a.B;
  const int b = in_batch ? (int)bl : 0;
  // (nothing of a skipped trajectory is read or written)
  const bool live = in_batch && (a.active == nullptr || a.active[b] != 0);
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  const bool tracked = goals.ref != nullptr;  // (uniform over the launch)

  PDDP_PROBLEM_OF_B
  T umin[m], umax[m], astd[m], z0[n];
#pragma unroll
  for (int r = 0; r < m; ++r) umin[r] = umax[r] = astd[r] = T(0);
#pragma unroll
  for (int j = 0; j < n; ++j) z0[j] = T(0);
  if (live) {
#pragma unroll
    for (int r = 0; r < m; ++r) {
      umin[r] = bounded ? a.u_min[r] : T(0);
      umax[r] = bounded ? a.u_max[r] : T(0);
      astd[r] = a.a_std[r];
    }
#pragma unroll
    for (int j = 0; j < n; ++j) z0[j] = a.z0[(size_t)b * n + j];
  }
  const T* Ub = a.U + (size_t)b * N * m;
  const T inf = std::numeric_limits<T>::infinity();

  // the lane's own candidates meet in s order: ties go to the lower s
  T Jmin = inf;
  int smin = -1;
  const int turns = (S + G - 1) / G;
  for (int turn = 0; turn <= turns; ++turn) {
    const bool keep = turn == turns;  // (uniform over the launch)
    int s = lane + turn * G;
    bool run = live && s < S;
    if (keep) {
      // the argmin, in shoot_kernel's order
      const int span = G < kWave ? G : kWave;
      for (int off = 1; off < span; off <<= 1)
        goals_take_lower(Jmin, smin, __shfl_xor(Jmin, off),
                         __shfl_xor(smin, off));
      if (blockDim.x > kWave) {  // one trajectory over several wavefronts
        constexpr int W = kClosedLoopThreads / kWave;
        __shared__ T part_J[W];
        __shared__ int part_s[W];
        if (tid % kWave == 0) {
          part_J[tid / kWave] = Jmin;
          part_s[tid / kWave] = smin;
        }
        __syncthreads();
        Jmin = part_J[0];
        smin = part_s[0];
        for (int w = 1; w < (int)blockDim.x / kWave; ++w)
          goals_take_lower(Jmin, smin, part_J[w], part_s[w]);
      }
      if (live && lane == 0) {
        a.best[b] = smin;
        if (a.J_best != nullptr) a.J_best[b] = Jmin;
      }
      // the winner again, by the lane that ran it, its rows kept
      s = smin;
      run = live && a.Z_out != nullptr && smin >= 0 && lane == smin % G;
    }
    if (run) {
      const size_t bs = (size_t)b * S + s;
      const uint64_t roll = a.offset + (uint64_t)bs;
      const bool base = s == 0;  // the base sequence is a candidate
      T* Zo = a.Z_out + (size_t)b * (N + 1) * n;
      T* Uo = a.U_out + (size_t)b * N * m;
#define PDDP_SAMPLED_KEEP_ROW                                                  \
  if (keep) {                                                                  \
    PDDP_COPY(n, Zo + (size_t)t * n, z)                                        \
    PDDP_COPY(m, Uo + (size_t)t * m, un)                                       \
  }
#include "sampled_rollout_body.inc"
#undef PDDP_SAMPLED_KEEP_ROW
      if (keep) {
#pragma unroll
        for (int j = 0; j < n; ++j) Zo[(size_t)N * n + j] = z[j];
      } else {
        a.Jc[bs] = J;
        if (is_finite(J) && J < Jmin) {
          Jmin = J;
          smin = s;
        }
      }
    }
  }
}

// ---- mppi --------------------------------------------------------------------

template <typename T>
struct MppiGoalsArgs {
  int B, N, S, G;
  const T* z0;  // [B][n]
  const T* U;   // [B][N][m]
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

#define PDDP_SAMPLED_KEEP_ROW

// mppi_kernel (mppi.hip) with the objective above: its three passes over the
// same turns; the weighted rollout of pass 3 reads the same rows.
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void mppi_goals_kernel(
    ProblemT<T> shared, MppiGoalsArgs<T> a, RefArgs<T> goals,
    const T* weights) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr int kWaves = kClosedLoopThreads / kWave;
  const int tid = threadIdx.x, G = a.G, N = a.N, S = a.S;
  const int group = tid / G, lane = tid - group * G;
  const long long bl = (long long)blockIdx.x * (blockDim.x / G) + group;
  const bool in_batch = bl < a.B;
  const int b = in_batch ? (int)bl : 0;
  // (nothing of a skipped trajectory is read or written)
  const bool live = in_batch && (a.active == nullptr || a.active[b] != 0);
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  const bool multi = blockDim.x > kWave;  // one trajectory, several wavefronts
  const int span = G < kWave ? G : kWave;
  const bool tracked = goals.ref != nullptr;  // (uniform over the launch)

  PDDP_PROBLEM_OF_B
  T umin[m], umax[m], astd[m], z0[n];
#pragma unroll
  for (int r = 0; r < m; ++r) umin[r] = umax[r] = astd[r] = T(0);
#pragma unroll
  for (int j = 0; j < n; ++j) z0[j] = T(0);
  T lam = T(1);
  if (live) {
#pragma unroll
    for (int r = 0; r < m; ++r) {
      umin[r] = bounded ? a.u_min[r] : T(0);
      umax[r] = bounded ? a.u_max[r] : T(0);
      astd[r] = a.a_std[r];
    }
#pragma unroll
    for (int j = 0; j < n; ++j) z0[j] = a.z0[(size_t)b * n + j];
    lam = a.lam[b];
  }
  const T* Ub = a.U + (size_t)b * N * m;
  const T inf = std::numeric_limits<T>::infinity();
  const int turns = (S + G - 1) / G;

  // ---- pass 1: the candidates ------------------------------------------------
  // the lane's own candidates meet in s order: ties go to the lower s
  T Jmin = inf;
  int smin = -1;
  for (int turn = 0; turn < turns; ++turn) {
    const int s = lane + turn * G;
    if (live && s < S) {
      const size_t bs = (size_t)b * S + s;
      const uint64_t roll = a.offset + (uint64_t)bs;
      const bool base = s == 0;  // the base sequence is a candidate
#include "sampled_rollout_body.inc"
      a.Jc[bs] = J;
      if (is_finite(J) && J < Jmin) {
        Jmin = J;
        smin = s;
      }
    }
  }

  // the argmin, in shoot's order
  for (int off = 1; off < span; off <<= 1)
    goals_take_lower(Jmin, smin, __shfl_xor(Jmin, off), __shfl_xor(smin, off));
  if (multi) {
    __shared__ T part_J[kWaves];
    __shared__ int part_s[kWaves];
    if (tid % kWave == 0) {
      part_J[tid / kWave] = Jmin;
      part_s[tid / kWave] = smin;
    }
    __syncthreads();
    Jmin = part_J[0];
    smin = part_s[0];
    for (int w = 1; w < (int)blockDim.x / kWave; ++w)
      goals_take_lower(Jmin, smin, part_J[w], part_s[w]);
  }
  // a temperature that is not positive (or NaN): as without a finite candidate
  if (!(lam > T(0))) {
    Jmin = inf;
    smin = -1;
  }
  const bool ok = live && smin >= 0;
  const bool owner = ok && lane == 0;  // ONE lane per trajectory
  if (live && lane == 0) {
    a.best[b] = smin;
    if (a.J_best != nullptr) a.J_best[b] = Jmin;
    if (!ok) a.J_w[b] = inf;
  }

  // ---- pass 2: eta.  A lane's own weights in s order, then the group. -------
  __shared__ T part_eta[1][kWaves];
  __shared__ T part_sum[2][m][kWaves];
  T eta_[1] = {T(0)};
  for (int turn = 0; turn < turns; ++turn) {
    const int s = lane + turn * G;
    if (ok && s < S)
      eta_[0] += goals_weight(a.Jc[(size_t)b * S + s], Jmin, lam);
  }
  goals_group_sum(eta_, span, multi, part_eta);
  const T eta = eta_[0];

  // ---- pass 3: the weighted perturbation, then the weighted rollout ---------
  T* Zo = a.Z_out + (size_t)b * (N + 1) * n;
  T* Uo = a.U_out + (size_t)b * N * m;
  const bool rows = a.U_out != nullptr;
  int phase = 0;
  for (int turn = 0; turn < turns; ++turn) {
    const bool last = turn == turns - 1;  // (uniform over the launch)
    const int s = lane + turn * G;
    const size_t bs = (size_t)b * S + s;
    const uint64_t roll = a.offset + (uint64_t)bs;
    T w = T(0);
    if (live && s < S) {
      if (ok) w = goals_weight(a.Jc[bs], Jmin, lam);
      if (a.W != nullptr) a.W[bs] = ok ? w / eta : T(0);
    }
    // candidate 0 adds its weight to eta and nothing to the sum; a weight of
    // 0 adds 0 whatever its draws are, so they are not made
    const bool draw = s >= 1 && w > T(0);
    // the sum of the turns before this one: the owner's own stores in U_out
    const bool carry = owner && turn > 0 && rows;
    T e[m], ur[m], prev[m], z[n];
#pragma unroll
    for (int j = 0; j < m; ++j) {
      e[j] = T(0);
      ur[j] = owner ? Ub[j] : T(0);
      prev[j] = carry ? Uo[j] : T(0);
    }
#pragma unroll
    for (int j = 0; j < n; ++j) z[j] = z0[j];
    if (draw) draw_units<T, m>(a.seed, roll, 0, kSampledStream, e);  // e_0
    // (the weighted rollout's goals: every lane takes its trajectory's rows,
    // one broadcast each, under the launch-uniform `tracked` alone)
    PDDP_GOALS(TAKE_FIRST)
    T J = T(0);
    for (int t = 0; t < N; ++t) {
      // the next step's base action, carried sum and goals, ahead of the chain
      T ur2[m], prev2[m], p[m];
      const int tn = (t + 1 < N) ? t + 1 : t;
#pragma unroll
      for (int j = 0; j < m; ++j) {
        ur2[j] = owner ? Ub[tn * m + j] : T(0);
        prev2[j] = carry ? Uo[tn * m + j] : T(0);
        // (an explicit fma: the product is rounded before it meets a sum)
        p[j] = draw ? fma_of(w, e[j], T(0)) : T(0);
      }
      PDDP_GOALS(REQUEST_NEXT)
      if (draw) {
        T xi[m];
        draw_units<T, m>(a.seed, roll, t + 1, kSampledStream, xi);
#pragma unroll
        for (int j = 0; j < m; ++j)
          e[j] = fma_of(a.beta, e[j], a.gamma * xi[j]);
      }
      goals_group_sum(p, span, multi, part_sum[phase]);
      phase ^= 1;
      if (owner) {
        T acc[m];
#pragma unroll
        for (int j = 0; j < m; ++j) acc[j] = turn > 0 ? prev[j] + p[j] : p[j];
        if (!last) {
          if (rows) {
#pragma unroll
            for (int j = 0; j < m; ++j) Uo[(size_t)t * m + j] = acc[j];
          }
        } else {
          T un[m], zn[n];
#pragma unroll
          for (int r = 0; r < m; ++r) {
            const T v = fma_of(astd[r], acc[r] / eta, ur[r]);
            un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
          }
          if (rows) {
#pragma unroll
            for (int j = 0; j < n; ++j) Zo[(size_t)t * n + j] = z[j];
#pragma unroll
            for (int j = 0; j < m; ++j) Uo[(size_t)t * m + j] = un[j];
          }
          const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
          J += cost_value<T, MODEL>(P, z, un, tr, false);
          dynamics<T, MODEL, false>(P, z, un, tr, zn, nullptr, nullptr);
#pragma unroll
          for (int j = 0; j < n; ++j) z[j] = zn[j];
        }
      }
#pragma unroll
      for (int j = 0; j < m; ++j) {
        ur[j] = ur2[j];
        prev[j] = prev2[j];
      }
      PDDP_GOALS(TAKE_NEXT)
    }
    if (owner && last) {
      J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
      if (rows) {
#pragma unroll
        for (int j = 0; j < n; ++j) Zo[(size_t)N * n + j] = z[j];
      }
      a.J_w[b] = J;
    }
  }
}

// ---- the trial ---------------------------------------------------------------

template <typename T>
struct MppiTrialGoalsArgs {
  int B, N, S, G, K, TT, t0, count;
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

// mppi_trial_kernel (mppi_trial.hip) with the objective above.  `window`: the
// launch's reference with ref_t0 as the caller gave it (ref_t0 + TT fits an
// int: the host's test); control step c plans under the window that starts at
// row min(ref_t0 + c, ref_len - 1) - `goals` inside the loop over c - and the
// applied step is logged as pddp_mpc_advance_track_* logs it: under that
// window's row 0, the terminal cost under its row 1, the SHARED Q, Q_term, R.
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void mppi_trial_goals_kernel(
    ProblemT<T> shared, MppiTrialGoalsArgs<T> a, RefArgs<T> window,
    const T* weights) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr int kWaves = kClosedLoopThreads / kWave;
  const int tid = threadIdx.x, G = a.G, N = a.N, S = a.S, K = a.K, TT = a.TT;
  const int group = tid / G, lane = tid - group * G;
  const long long bl = (long long)blockIdx.x * (blockDim.x / G) + group;
  const bool in_batch = bl < a.B;
  const int b = in_batch ? (int)bl : 0;
  // (nothing of a skipped trajectory is read or written)
  const bool live = in_batch && (a.active == nullptr || a.active[b] != 0);
  const bool head = live && lane == 0;  // ONE lane per trajectory
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  const bool multi = blockDim.x > kWave;  // one trajectory, several wavefronts
  const int span = G < kWave ? G : kWave;
  const bool tracked = window.ref != nullptr;  // (uniform over the launch)

  // the controller's model of trajectory b under the planning objective: the
  // weights row written over P once, ahead of the turns; with a reference
  // the goals of P are a window's rows, `goals` the window of the step
  RefArgs<T> goals = window;
  PDDP_PROBLEM_OF_B
  T umin[m], umax[m], astd[m];
#pragma unroll
  for (int r = 0; r < m; ++r) umin[r] = umax[r] = astd[r] = T(0);
  T lam = T(1);
  if (live) {
#pragma unroll
    for (int r = 0; r < m; ++r) {
      umin[r] = bounded ? a.u_min[r] : T(0);
      umax[r] = bounded ? a.u_max[r] : T(0);
      astd[r] = a.a_std[r];
    }
    lam = a.lam[b];
  }
  T* Ub = a.U + (size_t)b * N * m;
  T* Uo = a.U_work + (size_t)b * N * m;
  const T inf = std::numeric_limits<T>::infinity();
  const int turns = (S + G - 1) / G;

  __shared__ T part_J[kWaves];
  __shared__ int part_s[kWaves];
  __shared__ T part_eta[2][kWaves];
  __shared__ T part_sum[2][m][kWaves];
  int phase = 0;

  // the trial's cost so far: the head's own word from step to step
  T Jcl = T(0);
  if (head && a.t0 > 0) Jcl = a.Jcl[b];

  for (int c = a.t0; c < a.t0 + a.count; ++c) {
    // the window of control step c (one integer moves, as mpc_closed_loop
    // moves it), clamped to the last row
    if (tracked) {
      const int first = window.ref_t0 + c;
      goals.ref_t0 = first < window.ref_len - 1 ? first : window.ref_len - 1;
    }

    // what the controller sees at step c (the head's store of step c - 1)
    T z0[n];
#pragma unroll
    for (int j = 0; j < n; ++j) z0[j] = live ? a.z0[(size_t)b * n + j] : T(0);

    for (int k = 0; k < K; ++k) {
      const uint64_t offset =
          a.cand_offset + ((uint64_t)c * (uint64_t)K + (uint64_t)k) * a.iter_stride;
      T* Jcb = a.Jc + (a.log_costs != 0
                           ? (((size_t)b * TT + c) * K + k) * (size_t)S
                           : (size_t)b * S);

      // ---- pass 1: the candidates ------------------------------------------
      T Jmin = inf, J0 = inf;
      int smin = -1;
      for (int turn = 0; turn < turns; ++turn) {
        const int s = lane + turn * G;
        if (live && s < S) {
          const uint64_t roll = offset + (uint64_t)((size_t)b * S + s);
          const bool base = s == 0;  // the base sequence is a candidate
#include "sampled_rollout_body.inc"
          Jcb[s] = J;
          if (base) J0 = J;  // (the head's: lane 0 holds candidate 0)
          if (is_finite(J) && J < Jmin) {
            Jmin = J;
            smin = s;
          }
        }
      }

      // the argmin, in mppi's order
      for (int off = 1; off < span; off <<= 1)
        goals_take_lower(Jmin, smin, __shfl_xor(Jmin, off),
                         __shfl_xor(smin, off));
      if (multi) {
        if (tid % kWave == 0) {
          part_J[tid / kWave] = Jmin;
          part_s[tid / kWave] = smin;
        }
        __syncthreads();
        Jmin = part_J[0];
        smin = part_s[0];
        for (int w = 1; w < (int)blockDim.x / kWave; ++w)
          goals_take_lower(Jmin, smin, part_J[w], part_s[w]);
      }
      // a temperature that is not positive (or NaN): no finite candidate
      if (!(lam > T(0))) {
        Jmin = inf;
        smin = -1;
      }
      const bool ok = live && smin >= 0;
      const bool owner = ok && lane == 0;

      // ---- pass 2: eta, and the sum of the squared weights with it ----------
      T es[2] = {T(0), T(0)};
      for (int turn = 0; turn < turns; ++turn) {
        const int s = lane + turn * G;
        if (ok && s < S) {
          const T w = goals_weight(Jcb[s], Jmin, lam);
          es[0] += w;
          es[1] += w * w;
        }
      }
      goals_group_sum(es, span, multi, part_eta);
      const T eta = es[0];

      // ---- pass 3: the weighted perturbation, then the weighted rollout -----
      T Jw = inf;
      for (int turn = 0; turn < turns; ++turn) {
        const bool last = turn == turns - 1;  // (uniform over the launch)
        const int s = lane + turn * G;
        const uint64_t roll = offset + (uint64_t)((size_t)b * S + s);
        T w = T(0);
        if (ok && s < S) w = goals_weight(Jcb[s], Jmin, lam);
        // candidate 0 adds its weight to eta and nothing to the sum; a weight
        // of 0 adds 0 whatever its draws are, so they are not made
        const bool draw = s >= 1 && w > T(0);
        // the sum of the turns before this one: the owner's stores in U_work
        const bool carry = owner && turn > 0;
        T e[m], ur[m], prev[m], z[n];
#pragma unroll
        for (int j = 0; j < m; ++j) {
          e[j] = T(0);
          ur[j] = owner ? Ub[j] : T(0);
          prev[j] = carry ? Uo[j] : T(0);
        }
#pragma unroll
        for (int j = 0; j < n; ++j) z[j] = z0[j];
        if (draw) draw_units<T, m>(a.seed, roll, 0, kSampledStream, e);
        PDDP_GOALS(TAKE_FIRST)
        T J = T(0);
        for (int t = 0; t < N; ++t) {
          T ur2[m], prev2[m], p[m];
          const int tn = (t + 1 < N) ? t + 1 : t;
#pragma unroll
          for (int j = 0; j < m; ++j) {
            ur2[j] = owner ? Ub[tn * m + j] : T(0);
            prev2[j] = carry ? Uo[tn * m + j] : T(0);
            // (an explicit fma: the product is rounded before it meets a sum)
            p[j] = draw ? fma_of(w, e[j], T(0)) : T(0);
          }
          PDDP_GOALS(REQUEST_NEXT)
          if (draw) {
            T xi[m];
            draw_units<T, m>(a.seed, roll, t + 1, kSampledStream, xi);
#pragma unroll
            for (int j = 0; j < m; ++j)
              e[j] = fma_of(a.beta, e[j], a.gamma * xi[j]);
          }
          goals_group_sum(p, span, multi, part_sum[phase]);
          phase ^= 1;
          if (owner) {
            T acc[m];
#pragma unroll
            for (int j = 0; j < m; ++j)
              acc[j] = turn > 0 ? prev[j] + p[j] : p[j];
            if (!last) {
#pragma unroll
              for (int j = 0; j < m; ++j) Uo[(size_t)t * m + j] = acc[j];
            } else {
              T un[m], zn[n];
#pragma unroll
              for (int r = 0; r < m; ++r) {
                const T v = fma_of(astd[r], acc[r] / eta, ur[r]);
                un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
              }
#pragma unroll
              for (int j = 0; j < m; ++j) Uo[(size_t)t * m + j] = un[j];
              const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
              J += cost_value<T, MODEL>(P, z, un, tr, false);
              dynamics<T, MODEL, false>(P, z, un, tr, zn, nullptr, nullptr);
#pragma unroll
              for (int j = 0; j < n; ++j) z[j] = zn[j];
            }
          }
#pragma unroll
          for (int j = 0; j < m; ++j) {
            ur[j] = ur2[j];
            prev[j] = prev2[j];
          }
          PDDP_GOALS(TAKE_NEXT)
        }
        if (owner && last) {
          J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
          Jw = J;
        }
      }

      // ---- the head: take the weighted sequence or keep the plan ------------
      if (head) {
        const size_t ck = ((size_t)b * TT + c) * K + k;
        if (a.J0_log != nullptr) a.J0_log[ck] = J0;
        if (a.Jw_log != nullptr) a.Jw_log[ck] = Jw;
        const bool took = is_finite(Jw) && Jw <= J0;
        if (k < K - 1) {
          if (took) {
            for (int i = 0; i < N * m; ++i) Ub[i] = Uo[i];
          }
        } else {
          const size_t bc = (size_t)b * TT + c;
          if (a.ess_log != nullptr)
            a.ess_log[bc] = ok ? (eta * eta) / es[1] : T(0);
          // the step's plan is `src`: logged, its first row applied, and U[b]
          // its shift (plain copies of unclamped words, the last row
          // repeated).  In place, row i + 1 is read before row i is written.
          const T* src = took ? Uo : Ub;
          T* Pb = a.plan_log != nullptr ? a.plan_log + bc * N * m : nullptr;
          T cur[m], nxt[m], u[m];
#pragma unroll
          for (int j = 0; j < m; ++j) {
            cur[j] = src[j];
            u[j] = bounded ? clamp1(cur[j], umin[j], umax[j]) : cur[j];
          }
          for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int j = 0; j < m; ++j)
              nxt[j] = i + 1 < N ? src[(i + 1) * m + j] : cur[j];
#pragma unroll
            for (int j = 0; j < m; ++j) {
              if (Pb != nullptr) Pb[i * m + j] = cur[j];
              Ub[i * m + j] = nxt[j];
              cur[j] = nxt[j];
            }
          }

          // apply u to the plant of row b, log the trial on the common
          // yardstick: the SHARED Q, Q_term, R, the goals of the plant row -
          // with a reference those of row ref_t0 + c, the plant row then
          // supplies parameters only (mpc_advance_goal_hooks.inc's plant)
          T x[n], xn[n];
#pragma unroll
          for (int j = 0; j < n; ++j)
            x[j] = a.v_std != nullptr ? a.x_true[(size_t)b * n + j] : z0[j];
          const uint64_t roll = a.rollout_offset + (uint64_t)b;
          const int step = a.step_offset + c;
          {
            ProblemT<T> Pl = shared;
            if (goals.table != nullptr)
              write_params_and_goals<T, MODEL>(
                  Pl, goals.table + (size_t)b * PDDP_BATCH_ROW);
            if (a.plant != nullptr)
              write_params_and_goals<T, MODEL>(
                  Pl, a.plant + (size_t)b * PDDP_BATCH_ROW);
            if (tracked) {
              const T* row = ref_row(goals, b, 0);
              PDDP_COPY(D::na, Pl.goal, row + PDDP_REF_X_GOAL)
              PDDP_COPY(m, Pl.ugoal, row + PDDP_REF_U_GOAL)
            }
#pragma unroll
            for (int j = 0; j < n; ++j)
              a.Xlog[((size_t)b * (TT + 1) + c) * n + j] = x[j];
#pragma unroll
            for (int j = 0; j < m; ++j) a.Ulog[bc * m + j] = u[j];
            const Trig<T, MODEL> tr = trig_of<T, MODEL>(x);
            Jcl += cost_value<T, MODEL>(Pl, x, u, tr, false);
            dynamics<T, MODEL, false>(Pl, x, u, tr, xn, nullptr, nullptr);
            if (a.disturbance != nullptr) {
#pragma unroll
              for (int j = 0; j < n; ++j)
                xn[j] = xn[j] + a.disturbance[bc * n + j];
            }
            if (a.w_std != nullptr) {
              T wn[n];
              draw_units<T, n>(a.seed, roll, step, 0, wn);
              add_scaled<T, n>(a.w_std, wn, xn);
            }
            if (c == TT - 1) {
#pragma unroll
              for (int j = 0; j < n; ++j)
                a.Xlog[((size_t)b * (TT + 1) + TT) * n + j] = xn[j];
              if (tracked) {  // under row ref_t0 + c + 1, x_goal only
                const T* row1 = ref_row(goals, b, 1);
                PDDP_COPY(D::na, Pl.goal, row1 + PDDP_REF_X_GOAL)
              }
              Jcl += cost_value<T, MODEL>(Pl, xn, nullptr,
                                          trig_of<T, MODEL>(xn), true);
            }
            a.Jcl[b] = Jcl;
          }
          // observe: x' stays the plant's, the controller gets y'
          if (a.v_std != nullptr) {
            T vn[n];
#pragma unroll
            for (int j = 0; j < n; ++j) a.x_true[(size_t)b * n + j] = xn[j];
            draw_units<T, n>(a.seed, roll, step + 1, 1, vn);
            add_scaled<T, n>(a.v_std, vn, xn);
            if (a.Ylog != nullptr) {
#pragma unroll
              for (int j = 0; j < n; ++j)
                a.Ylog[((size_t)b * (TT + 1) + c + 1) * n + j] = xn[j];
            }
          }
#pragma unroll
          for (int j = 0; j < n; ++j) a.z0[(size_t)b * n + j] = xn[j];
        }
      }
      goals_hand_over();
    }
  }

  // the rollout of the shifted plan, clamped, from what the controller sees
  // now, under the controller's model (the head re-reads its own stores); it
  // reads no goal and no weight
  if (head) {
    T* Zb = a.Z + (size_t)b * (N + 1) * n;
    T z[n], zn[n], u[m];
#pragma unroll
    for (int j = 0; j < n; ++j) {
      z[j] = a.z0[(size_t)b * n + j];
      Zb[j] = z[j];
    }
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int j = 0; j < m; ++j) {
        u[j] = Ub[i * m + j];
        if (bounded) u[j] = clamp1(u[j], umin[j], umax[j]);
      }
      const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
      dynamics<T, MODEL, false>(P, z, u, tr, zn, nullptr, nullptr);
#pragma unroll
      for (int j = 0; j < n; ++j) {
        z[j] = zn[j];
        Zb[(i + 1) * n + j] = z[j];
      }
    }
  }
}

#undef PDDP_SAMPLED_KEEP_ROW
#undef PDDP_SAMPLED_STREAM
#undef PDDP_GOALS_TAKE_NEXT
#undef PDDP_GOALS_REQUEST_NEXT
#undef PDDP_GOALS_TAKE_FIRST
#undef PDDP_GOALS
#undef PDDP_PROBLEM_OF_B

// ---- host path ---------------------------------------------------------------

// the reference and the weights of a launch (With<Args, SampledGoals<T>>)
template <typename T>
struct SampledGoals {
  RefArgs<T> goals;
  const T* weights;  // [B][PDDP_WEIGHT_ROW] or NULL
};

// What a suffix promises (`track`, `weighted`) is there: the reference with
// ref_t0 clamped (ref_args), the weights; what it does not name is absent.
template <typename T>
static bool sampled_goals(bool track, bool weighted, const T* table,
                          const T* ref, int ref_len, int ref_t0,
                          const T* weights, SampledGoals<T>* out) {
  *out = SampledGoals<T>{RefArgs<T>{table, nullptr, 0, 0}, nullptr};
  if (track && !ref_args(table, ref, ref_len, ref_t0, &out->goals))
    return false;
  if (weighted && weights == nullptr) return false;
  if (weighted) out->weights = weights;
  return true;
}

template <typename Args>
static dim3 sampled_geometry(Args& a, int* threads) {
  ClosedLoopArgs<float> g{};  // (the mapping is closed_loop's: its geometry)
  g.B = a.B;
  g.S = a.S;
  dim3 blocks;
  *threads = closed_loop_geometry(g, blocks);
  a.G = g.G;
  return blocks;
}

template <typename T, int MODEL>
static int launch_shoot_goals(const pddp_problem& p,
                              With<ShootGoalsArgs<T>, SampledGoals<T>> w,
                              hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  int threads;
  const dim3 blocks = sampled_geometry(w.a, &threads);
  PDDP_LAUNCH((shoot_goals_kernel<T, MODEL>), blocks, dim3(threads), 0, st, P,
              w.a, w.x.goals, w.x.weights);
  return launch_status();
}

template <typename T, int MODEL>
static int launch_mppi_goals(const pddp_problem& p,
                             With<MppiGoalsArgs<T>, SampledGoals<T>> w,
                             hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  int threads;
  const dim3 blocks = sampled_geometry(w.a, &threads);
  PDDP_LAUNCH((mppi_goals_kernel<T, MODEL>), blocks, dim3(threads), 0, st, P,
              w.a, w.x.goals, w.x.weights);
  return launch_status();
}

template <typename T, int MODEL>
static int launch_mppi_trial_goals(
    const pddp_problem& p, With<MppiTrialGoalsArgs<T>, SampledGoals<T>> w,
    hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  int threads;
  const dim3 blocks = sampled_geometry(w.a, &threads);
  PDDP_LAUNCH((mppi_trial_goals_kernel<T, MODEL>), blocks, dim3(threads), 0, st,
              P, w.a, w.x.goals, w.x.weights);
  return launch_status();
}

// (the tests of shoot_impl, shoot.hip, then the suffix's)
template <typename T>
static int shoot_goals_impl(const pddp_problem* p, bool track, bool weighted,
                            const T* table, const T* ref, int ref_len,
                            int ref_t0, const T* weights, int B, int N, int S,
                            const T* z0, const T* U, const T* u_min,
                            const T* u_max, const T* a_std, double smooth,
                            uint64_t seed, uint64_t sample_offset,
                            const uint8_t* active, T* Jc, int32_t* best,
                            T* J_best, T* Z_out, T* U_out, void* stream) {
  if (B <= 0 || N <= 0 || S <= 0 || (long long)B * S > 0x7fffffffLL || !z0 ||
      !U || !a_std || !Jc || !best ||
      (Z_out == nullptr) != (U_out == nullptr) ||
      (U_out != nullptr && (U_out == U || Z_out == z0)) ||
      !(smooth >= 0.0 && smooth < 1.0))  // (NaN fails both)
    return PDDP_E_BADARG;
  With<ShootGoalsArgs<T>, SampledGoals<T>> w{};
  if (!sampled_goals(track, weighted, table, ref, ref_len, ref_t0, weights,
                     &w.x))
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  const double gamma = std::sqrt(1.0 - smooth * smooth);
  w.a = ShootGoalsArgs<T>{B,      N,        S,      0,    z0,
                          U,      u_min,    u_max,  a_std, (T)smooth,
                          (T)gamma, seed,   sample_offset, active, Jc,
                          best,   J_best,   Z_out,  U_out};
  PDDP_DISPATCH_MODEL(launch_shoot_goals, T, p, w, (hipStream_t)stream)
}

// (the tests of mppi_impl, mppi.hip, then the suffix's)
template <typename T>
static int mppi_goals_impl(const pddp_problem* p, bool track, bool weighted,
                           const T* table, const T* ref, int ref_len,
                           int ref_t0, const T* weights, int B, int N, int S,
                           const T* z0, const T* U, const T* u_min,
                           const T* u_max, const T* a_std, const T* lam,
                           double smooth, uint64_t seed,
                           uint64_t sample_offset, const uint8_t* active,
                           T* Jc, int32_t* best, T* J_best, T* W, T* J_w,
                           T* Z_out, T* U_out, void* stream) {
  if (B <= 0 || N <= 0 || S <= 0 || (long long)B * S > 0x7fffffffLL || !z0 ||
      !U || !a_std || !lam || !Jc || !best || !J_w ||
      (Z_out == nullptr) != (U_out == nullptr) ||
      (U_out != nullptr && (U_out == U || Z_out == z0)) ||
      // (a lane with more than one turn keeps the running sum in U_out)
      (U_out == nullptr && S > kClosedLoopThreads) ||
      !(smooth >= 0.0 && smooth < 1.0))  // (NaN fails both)
    return PDDP_E_BADARG;
  With<MppiGoalsArgs<T>, SampledGoals<T>> w{};
  if (!sampled_goals(track, weighted, table, ref, ref_len, ref_t0, weights,
                     &w.x))
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  const double gamma = std::sqrt(1.0 - smooth * smooth);
  w.a = MppiGoalsArgs<T>{B,     N,     S,         0,        z0,
                         U,     u_min, u_max,     a_std,    lam,
                         (T)smooth,    (T)gamma,  seed,     sample_offset,
                         active, Jc,   best,      J_best,   W,
                         J_w,   Z_out, U_out};
  PDDP_DISPATCH_MODEL(launch_mppi_goals, T, p, w, (hipStream_t)stream)
}

// (the tests of mppi_trial_impl, mppi_trial.hip, then: a reference or weights
// or both; the reference's ref_t0 is NOT clamped here - the kernel forms
// ref_t0 + c, which fits an int, and clamps the sum)
template <typename T>
static int mppi_trial_goals_impl(const pddp_problem* p, const T* table,
                                 const T* ref, int ref_len, int ref_t0,
                                 const T* weights, MppiTrialGoalsArgs<T> a,
                                 double smooth, void* stream) {
  if (a.B <= 0 || a.N <= 0 || a.S <= 0 ||
      (long long)a.B * a.S > 0x7fffffffLL || !a.z0 || !a.U || !a.a_std ||
      !a.lam || !a.Jc || !(smooth >= 0.0 && smooth < 1.0))  // (NaN fails both)
    return PDDP_E_BADARG;
  if (a.K < 1 || a.TT < 1 || a.t0 < 0 || a.count < 1 ||
      (long long)a.t0 + a.count > a.TT || !a.Z || !a.U_work || !a.Xlog ||
      !a.Ulog || !a.Jcl || a.U_work == a.U ||
      (a.v_std != nullptr && a.x_true == nullptr) ||
      // (step_offset + c + 1 is a counter word of the draws: an int)
      a.step_offset < 0 || a.step_offset > INT_MAX - a.TT)
    return PDDP_E_BADARG;
  if (ref == nullptr && weights == nullptr) return PDDP_E_BADARG;
  With<MppiTrialGoalsArgs<T>, SampledGoals<T>> w{
      a, {RefArgs<T>{table, nullptr, 0, 0}, weights}};
  if (ref != nullptr) {
    if (ref_len < 1 || ref_t0 < 0 || ref_t0 > INT_MAX - a.TT)
      return PDDP_E_BADARG;
    w.x.goals = RefArgs<T>{table, ref, ref_len, ref_t0};
  }
  if (int rc = check_problem(p)) return rc;
  w.a.beta = (T)smooth;
  w.a.gamma = (T)std::sqrt(1.0 - smooth * smooth);
  if (w.a.v_std == nullptr) w.a.x_true = w.a.Ylog = nullptr;
  PDDP_DISPATCH_MODEL(launch_mppi_trial_goals, T, p, w, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

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

// the three suffixes of one family (NAME: shoot, mppi): thin fronts over the
// family's one kernel
#define PDDP_SAMPLED_FRONTS(NAME, SUF, T, PARAMS, ARGS)                        \
  int pddp_##NAME##_track_##SUF(const pddp_problem* p, const T* table,         \
                                const T* ref, int ref_len, int ref_t0,         \
                                PARAMS(T)) {                                   \
    return pddp::NAME##_goals_impl<T>(p, true, false, table, ref, ref_len,     \
                                      ref_t0, nullptr, ARGS);                  \
  }                                                                            \
  int pddp_##NAME##_weighted_##SUF(const pddp_problem* p, const T* table,      \
                                   const T* weights, PARAMS(T)) {              \
    return pddp::NAME##_goals_impl<T>(p, false, true, table, nullptr, 0, 0,    \
                                      weights, ARGS);                          \
  }                                                                            \
  int pddp_##NAME##_track_weighted_##SUF(                                      \
      const pddp_problem* p, const T* table, const T* ref, int ref_len,        \
      int ref_t0, const T* weights, PARAMS(T)) {                               \
    return pddp::NAME##_goals_impl<T>(p, true, true, table, ref, ref_len,      \
                                      ref_t0, weights, ARGS);                  \
  }

#define PDDP_SAMPLED_GOALS_ENTRY_POINTS(SUF, T)                                \
  PDDP_SAMPLED_FRONTS(shoot, SUF, T, PDDP_SHOOT_PARAMS, PDDP_SHOOT_ARGS)       \
  PDDP_SAMPLED_FRONTS(mppi, SUF, T, PDDP_MPPI_PARAMS, PDDP_MPPI_ARGS)          \
  int pddp_mppi_trial_goals_##SUF(                                             \
      const pddp_problem* p, const T* table, const T* plant, const T* ref,     \
      int ref_len, int ref_t0, const T* weights, int B, int N, int S, int K,   \
      int TT, int t0, int count, T* z0, T* U, T* Z, T* U_work,                 \
      const T* u_min, const T* u_max, const T* a_std, const T* lam,            \
      double smooth, uint64_t seed, uint64_t cand_offset,                      \
      uint64_t iter_stride, const T* disturbance, const T* w_std,              \
      const T* v_std, uint64_t rollout_offset, int step_offset, T* x_true,     \
      const uint8_t* active, T* Jc, int log_costs, T* Xlog, T* Ulog, T* Jcl,   \
      T* Ylog, T* J0_log, T* Jw_log, T* ess_log, T* plan_log, void* stream) {  \
    return pddp::mppi_trial_goals_impl<T>(                                     \
        p, table, ref, ref_len, ref_t0, weights,                               \
        {B,          N,           S,           0,           K,                 \
         TT,         t0,          count,       plant,       z0,                \
         U,          Z,           U_work,      u_min,       u_max,             \
         a_std,      lam,         T(0),        T(0),        seed,              \
         cand_offset, iter_stride, disturbance, w_std,      v_std,             \
         rollout_offset, step_offset, x_true,  active,      Jc,                \
         log_costs,  Xlog,        Ulog,        Jcl,         Ylog,              \
         J0_log,     Jw_log,      ess_log,     plan_log},                      \
        smooth, stream);                                                       \
  }

PDDP_SAMPLED_GOALS_ENTRY_POINTS(f32, float)
PDDP_SAMPLED_GOALS_ENTRY_POINTS(f64, double)
#undef PDDP_SAMPLED_GOALS_ENTRY_POINTS
#undef PDDP_SAMPLED_FRONTS
#undef PDDP_MPPI_ARGS
#undef PDDP_MPPI_PARAMS
#undef PDDP_SHOOT_ARGS
#undef PDDP_SHOOT_PARAMS

}  // extern "C"
