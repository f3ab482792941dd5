// shoot_kernel_body.inc - the body of shoot_kernel and of shoot_goals_kernel
// (shoot.hip): ceil(S / G) + 1 turns of the candidate rollout, the last one
// the argmin and the winner again with its rows kept.  The including kernel
// has `shared`, `a` (ShootArgs or ShootGoalsArgs) and sampled_common.hpp's
// hooks, and defines
//   PDDP_SHOOT_ROWS_AHEAD   the rows' declaration (PDDP_SHOOT_ROWS) ahead of
//                           the rollout, or empty where the kernel was
//                           compiled with it behind the first draws
//                           (PDDP_SAMPLED_AFTER_E0): statement order alone
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

  // the problem of trajectory b, in registers for the whole launch; Q, Qt and
  // R stay scalar operands where no weights row is written over them
  PDDP_PROBLEM_OF_B
  T umin[m], umax[m], astd[m], z0[n];
#pragma unroll
  for (int r = 0; r < m; ++r) umin[r] = umax[r] = astd[r] = T(0);
#pragma unroll
  for (int j = 0; j < n; ++j) z0[j] = T(0);
  if (live) {
    PDDP_ROW_OF_B
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
      const int span = G < kWave ? G : kWave;
      __shared__ T part_J[kClosedLoopThreads / kWave];
      __shared__ int part_s[kClosedLoopThreads / kWave];
#include "sampled_argmin.inc"
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
#define PDDP_SHOOT_ROWS                                                        \
  T* Zo = a.Z_out + (size_t)b * (N + 1) * n;                                   \
  T* Uo = a.U_out + (size_t)b * N * m;
      PDDP_SHOOT_ROWS_AHEAD
#define PDDP_SAMPLED_KEEP_ROW                                                  \
  if (keep) {                                                                  \
    PDDP_COPY(n, Zo + (size_t)t * n, z)                                        \
    PDDP_COPY(m, Uo + (size_t)t * m, un)                                       \
  }
#include "sampled_rollout_body.inc"
#undef PDDP_SAMPLED_KEEP_ROW
#undef PDDP_SHOOT_ROWS
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
