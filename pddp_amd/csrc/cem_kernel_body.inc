// cem_kernel_body.inc - the body of cem_kernel and of cem_goals_kernel
// (cem.hip): three passes over the same ceil(S / G) turns of the lane group.
// The including kernel has `shared`, `a` (CemArgs or CemGoalsArgs) and
// sampled_common.hpp's hooks, as mppi_kernel_body.inc's; in the goals kernel
// the mean's rollout of pass 3 reads the rows the candidates read.  Passes 2
// and 3 are the texts the trial includes too (cem_rank_body.inc,
// cem_refit_body.inc); two words of pass 3 are the kernel's (cem.hip):
// PDDP_CEM_CUT_J, the cut's cost, and PDDP_CEM_FLOOR(r), std_min[r] - `Jcut`
// and `smin[r]` in the plain kernel.
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
  T umin[m], umax[m], smin[m], z0[n];
#pragma unroll
  for (int r = 0; r < m; ++r) umin[r] = umax[r] = smin[r] = T(0);
#pragma unroll
  for (int j = 0; j < n; ++j) z0[j] = T(0);
  if (live) {
    PDDP_ROW_OF_B
#pragma unroll
    for (int r = 0; r < m; ++r) {
      umin[r] = bounded ? a.u_min[r] : T(0);
      umax[r] = bounded ? a.u_max[r] : T(0);
      smin[r] = a.std_min != nullptr ? a.std_min[r] : T(0);
    }
#pragma unroll
    for (int j = 0; j < n; ++j) z0[j] = a.z0[(size_t)b * n + j];
  }
  const T* Ub = a.U + (size_t)b * N * m;
  const T* Sb = a.sigma + (size_t)b * N * m;
  const T inf = std::numeric_limits<T>::infinity();
  const int turns = (S + G - 1) / G;

  // ---- pass 1: the candidates, with row t of sigma[b] as the width ----------
  for (int turn = 0; turn < turns; ++turn) {
    const int s = lane + turn * G;
    if (live && s < S) {
      const size_t bs = (size_t)b * S + s;
      const uint64_t roll = a.offset + (uint64_t)bs;
      const bool base = s == 0;  // the mean is a candidate
#include "sampled_rollout_body.inc"
      a.Jc[bs] = J;
    }
  }

  // ---- pass 2: the ranks (cem_rank_body.inc) ---------------------------------
  // What pddp_cem_* keeps of them - rank, best, J_best, n_elite - is written
  // here.  (INDEX: the candidate's index ahead of the turn's first branch, where
  // the ranking had it - a hook for the statement's place alone.)
  __shared__ T stage[kClosedLoopThreads];
  __shared__ T cut_J[kWave];  // per lane group of the workgroup: the elite
  __shared__ int cut_s[kWave];  // of the highest rank, (J, s)
  __shared__ int part_fin[1][kWaves];
#define PDDP_CEM_COST(s) a.Jc[(size_t)b * S + (s)]
#define PDDP_CEM_KEEP(point) PDDP_CEM_KEEP_##point
#define PDDP_CEM_KEEP_INDEX const size_t bs = (size_t)b * S + s;
#define PDDP_CEM_KEEP_RANKED                                                   \
  if (mine && a.rank != nullptr)                                               \
    a.rank[bs] = fin ? below : -1;                                             \
  if (fin && below == 0) {                                                     \
    a.best[b] = s;                                                             \
    if (a.J_best != nullptr) a.J_best[b] = Js;                                 \
  }
#define PDDP_CEM_KEEP_CUT                                                      \
  if (live && lane == 0) {                                                     \
    a.n_elite[b] = Ke;                                                         \
    if (!ok) {                                                                 \
      a.best[b] = -1;                                                          \
      if (a.J_best != nullptr) a.J_best[b] = inf;                              \
      a.J_m[b] = inf;                                                          \
    }                                                                          \
  }
#include "cem_rank_body.inc"
#undef PDDP_CEM_KEEP_CUT
#undef PDDP_CEM_KEEP_RANKED
#undef PDDP_CEM_KEEP_INDEX
#undef PDDP_CEM_KEEP

  // ---- pass 3: the refit, then the mean's rollout (cem_refit_body.inc) -------
  // The owner keeps the running sums in U_out (s1) and S_out (s2) between
  // turns, and in the last turn stores Zm[b][t], Um[b][t] and Sm[b][t] there.
  __shared__ T part_sum[2][2 * m][kWaves];
  T* Zo = a.Z_out + (size_t)b * (N + 1) * n;
  T* Uo = a.U_out + (size_t)b * N * m;
  T* So = a.S_out + (size_t)b * N * m;
  const bool rows = a.U_out != nullptr;
  const T cnt = (T)Ke;
  int phase = 0;
  for (int turn = 0; turn < turns; ++turn) {
    const bool last = turn == turns - 1;  // (uniform over the launch)
    const int s = lane + turn * G;
    const size_t bs = (size_t)b * S + s;
    const uint64_t roll = a.offset + (uint64_t)bs;
    // (more than one turn: S > 256, the rows are there)
#define PDDP_CEM_CARRY owner && turn > 0 && rows
#define PDDP_CEM_KEEP_SUMS(acc)                                                \
  if (rows) {                                                                  \
    PDDP_COPY(m, Uo + (size_t)t * m, acc)                                      \
    PDDP_COPY(m, So + (size_t)t * m, acc + m)                                  \
  }
#define PDDP_CEM_KEEP_ROWS                                                     \
  if (rows) {                                                                  \
    PDDP_COPY(n, Zo + (size_t)t * n, z)                                        \
    PDDP_COPY(m, Uo + (size_t)t * m, un)                                       \
    PDDP_COPY(m, So + (size_t)t * m, sn)                                       \
  }
#include "cem_refit_body.inc"
#undef PDDP_CEM_KEEP_ROWS
#undef PDDP_CEM_KEEP_SUMS
#undef PDDP_CEM_CARRY
#undef PDDP_CEM_COST
    if (owner && last) {
      J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
      if (rows) {
#pragma unroll
        for (int j = 0; j < n; ++j) Zo[(size_t)N * n + j] = z[j];
      }
      a.J_m[b] = J;
    }
  }
