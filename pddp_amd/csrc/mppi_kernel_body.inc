// mppi_kernel_body.inc - the body of mppi_kernel and of mppi_goals_kernel
// (mppi.hip): three passes over the same ceil(S / G) turns of the lane group.
// The including kernel has `shared`, `a` (MppiArgs or MppiGoalsArgs) and
// sampled_common.hpp's hooks; in the goals kernel the weighted rollout of
// pass 3 reads the rows the candidates read.
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

  // the problem of trajectory b, as shoot's kernels hold it
  PDDP_PROBLEM_OF_B
  T umin[m], umax[m], astd[m], z0[n];
#pragma unroll
  for (int r = 0; r < m; ++r) umin[r] = umax[r] = astd[r] = T(0);
#pragma unroll
  for (int j = 0; j < n; ++j) z0[j] = T(0);
  T lam = T(1);
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
  __shared__ T part_J[kWaves];
  __shared__ int part_s[kWaves];
#include "sampled_argmin.inc"
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
      eta_[0] += softmin_weight(a.Jc[(size_t)b * S + s], Jmin, lam);
  }
  group_sum(eta_, span, multi, part_eta);
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
      if (ok) w = softmin_weight(a.Jc[bs], Jmin, lam);
      if (a.W != nullptr) a.W[bs] = ok ? w / eta : T(0);
    }
#define PDDP_MPPI_CARRY owner && turn > 0 && rows
#define PDDP_MPPI_KEEP_SUM(acc)                                                \
  if (rows) {                                                                  \
    PDDP_COPY(m, Uo + (size_t)t * m, acc)                                      \
  }
#define PDDP_MPPI_KEEP_ROW                                                     \
  if (rows) {                                                                  \
    PDDP_COPY(n, Zo + (size_t)t * n, z)                                        \
    PDDP_COPY(m, Uo + (size_t)t * m, un)                                       \
  }
#include "mppi_update_body.inc"
#undef PDDP_MPPI_KEEP_ROW
#undef PDDP_MPPI_KEEP_SUM
#undef PDDP_MPPI_CARRY
    if (owner && last) {
      J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
      if (rows) {
#pragma unroll
        for (int j = 0; j < n; ++j) Zo[(size_t)N * n + j] = z[j];
      }
      a.J_w[b] = J;
    }
  }
