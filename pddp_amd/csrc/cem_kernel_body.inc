// cem_kernel_body.inc - the body of cem_kernel and of cem_goals_kernel
// (cem.hip): three passes over the same ceil(S / G) turns of the lane group.
// The including kernel has `shared`, `a` (CemArgs or CemGoalsArgs) and
// sampled_common.hpp's hooks, as mppi_kernel_body.inc's; in the goals kernel
// the mean's rollout of pass 3 reads the rows the candidates read.  Two words
// of pass 3 are the kernel's (cem.hip): PDDP_CEM_CUT_J, the cut's cost, and
// PDDP_CEM_FLOOR(r), std_min[r] - `Jcut` and `smin[r]` in the plain kernel.
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

  // ---- pass 2: the ranks.  A lane's candidates against all S of its ---------
  // trajectory, a chunk of G at a time through LDS: every lane stages the cost
  // it wrote itself in pass 1 (+inf where it is not finite, or there is no
  // candidate), so no lane reads another lane's global store.  The loops and
  // their barriers are launch-uniform: lanes outside the batch or masked stage
  // +inf and count nothing.  `take_lower`'s order: (J, s) lexicographically.
  __shared__ T stage[kClosedLoopThreads];
  __shared__ T cut_J[kWave];  // per lane group of the workgroup: the elite
  __shared__ int cut_s[kWave];  // of the highest rank, (J, s)
  __shared__ int part_fin[1][kWaves];
  // the finite costs of the trajectory: a lane's own, then the group
  int fin_[1] = {0};
  for (int turn = 0; turn < turns; ++turn) {
    const int s = lane + turn * G;
    if (live && s < S) fin_[0] += is_finite(a.Jc[(size_t)b * S + s]) ? 1 : 0;
  }
  group_sum(fin_, span, multi, part_fin);
  const int n_fin = fin_[0];
  const int Ke = a.K < n_fin ? a.K : n_fin;
  for (int turn = 0; turn < turns; ++turn) {
    const int s = lane + turn * G;
    const size_t bs = (size_t)b * S + s;
    const bool mine = live && s < S;
    const T Js = mine ? a.Jc[bs] : inf;
    const bool fin = mine && is_finite(Js);
    int below = 0;
    for (int c = 0; c < turns; ++c) {
      const int sc = lane + c * G;
      T v = inf;
      if (live && sc < S) {
        v = a.Jc[(size_t)b * S + sc];
        v = is_finite(v) ? v : inf;
      }
      __syncthreads();  // (the chunk before has been read)
      stage[tid] = v;
      __syncthreads();
      // s' = c G + k against s = turn G + lane: every s' of an earlier chunk
      // is below s and every s' of a later one above, so only the lane's own
      // chunk needs the index (c and turn are launch-uniform)
      // (unrolled: the LDS reads of eight costs are in flight together)
      const T* chunk = stage + group * G;
      if (c < turn) {
#pragma unroll 8
        for (int k = 0; k < G; ++k) below += chunk[k] <= Js ? 1 : 0;
      } else if (c > turn) {
#pragma unroll 8
        for (int k = 0; k < G; ++k) below += chunk[k] < Js ? 1 : 0;
      } else {
#pragma unroll 8
        for (int k = 0; k < G; ++k) {
          const T o = chunk[k];
          below += (o < Js || (o == Js && k < lane)) ? 1 : 0;
        }
      }
    }
    if (mine && a.rank != nullptr) a.rank[bs] = fin ? below : -1;
    // the finite costs' ranks are 0 .. n_fin - 1, each once
    if (fin && below == 0) {
      a.best[b] = s;
      if (a.J_best != nullptr) a.J_best[b] = Js;
    }
    if (fin && below == Ke - 1) {
      cut_J[group] = Js;
      cut_s[group] = s;
    }
  }
  __syncthreads();
  const bool ok = live && n_fin > 0;
  const bool owner = ok && lane == 0;  // ONE lane per trajectory
  const T Jcut = ok ? cut_J[group] : -inf;
  const int scut = ok ? cut_s[group] : -1;
  if (live && lane == 0) {
    a.n_elite[b] = Ke;
    if (!ok) {
      a.best[b] = -1;
      if (a.J_best != nullptr) a.J_best[b] = inf;
      a.J_m[b] = inf;
    }
  }

  // ---- pass 3: the refit, then the mean's rollout ----------------------------
  // mppi_update_body.inc's structure with a weight of 0 or 1 and 2m sums per
  // step: s1 (e) and s2 (e e, rounded) of the elites s >= 1 over the group, the
  // turns in their order by the owner, who keeps the running sums in U_out (s1)
  // and S_out (s2) between turns, and in the last turn forms Um[b][t], Sm[b][t]
  // and steps the mean's rollout.  The goal hooks sit where
  // mppi_update_body.inc has them and enclose no shuffle and no barrier: every
  // lane takes its trajectory's rows under the launch-uniform `tracked` alone,
  // TAKE_FIRST in every turn (pass 1 leaves P with the terminal row's goals).
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
    // an elite: a finite cost that is not behind the cut.  Candidate 0 counts
    // in Ke and adds nothing; who is no elite adds 0 and makes no draws.
    bool draw = false;
    if (ok && s >= 1 && s < S) {
      const T Js = a.Jc[bs];
      draw = is_finite(Js) && (Js < PDDP_CEM_CUT_J ||
                               (Js == PDDP_CEM_CUT_J && s <= scut));
    }
    // (more than one turn: S > 256, the rows are there)
    const bool carry = owner && turn > 0 && rows;
    T e[m], ur[m], sg[m], prev[2 * m], z[n];
#pragma unroll
    for (int j = 0; j < m; ++j) {
      e[j] = T(0);
      ur[j] = owner ? Ub[j] : T(0);
      sg[j] = owner ? Sb[j] : T(0);
      prev[j] = carry ? Uo[j] : T(0);
      prev[m + j] = carry ? So[j] : T(0);
    }
#pragma unroll
    for (int j = 0; j < n; ++j) z[j] = z0[j];
    if (draw) draw_units<T, m>(a.seed, roll, 0, kSampledStream, e);  // e_0
    PDDP_GOALS(TAKE_FIRST)
    T J = T(0);
    for (int t = 0; t < N; ++t) {
      // the next step's mean, width, carried sums and goals, ahead of the chain
      T ur2[m], sg2[m], prev2[2 * m], p[2 * m];
      const int tn = (t + 1 < N) ? t + 1 : t;
#pragma unroll
      for (int j = 0; j < m; ++j) {
        ur2[j] = owner ? Ub[tn * m + j] : T(0);
        sg2[j] = owner ? Sb[tn * m + j] : T(0);
        prev2[j] = carry ? Uo[tn * m + j] : T(0);
        prev2[m + j] = carry ? So[tn * m + j] : T(0);
        p[j] = draw ? e[j] : T(0);
        // (an explicit fma: the square is rounded before it meets a sum)
        p[m + j] = draw ? fma_of(e[j], e[j], T(0)) : T(0);
      }
      PDDP_GOALS(REQUEST_NEXT)
      if (draw) {
        T xi[m];
        draw_units<T, m>(a.seed, roll, t + 1, kSampledStream, xi);
#pragma unroll
        for (int j = 0; j < m; ++j)
          e[j] = fma_of(a.beta, e[j], a.gamma * xi[j]);
      }
      group_sum(p, span, multi, part_sum[phase]);
      phase ^= 1;
      if (owner) {
        T acc[2 * m];
#pragma unroll
        for (int j = 0; j < 2 * m; ++j)
          acc[j] = turn > 0 ? prev[j] + p[j] : p[j];
        if (!last) {
          if (rows) {
            PDDP_COPY(m, Uo + (size_t)t * m, acc)
            PDDP_COPY(m, So + (size_t)t * m, acc + m)
          }
        } else {
          T un[m], sn[m], zn[n];
#pragma unroll
          for (int r = 0; r < m; ++r) {
            const T ebar = acc[r] / cnt;
            const T var = fma_of(-ebar, ebar, acc[m + r] / cnt);
            const T V = (Ke > 1 && var > T(0)) ? var : T(0);
            // (explicit fmas: each product is rounded where the law rounds it)
            const T g = fma_of(a.step, sg[r], T(0));
            const T v = fma_of(g, ebar, ur[r]);
            un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
            const T sd = fma_of(sg[r], sqrt_of(V), T(0));
            const T w = fma_of(a.step, sd - sg[r], sg[r]);
            sn[r] = w > PDDP_CEM_FLOOR(r) ? w : PDDP_CEM_FLOOR(r);
          }
          if (rows) {
            PDDP_COPY(n, Zo + (size_t)t * n, z)
            PDDP_COPY(m, Uo + (size_t)t * m, un)
            PDDP_COPY(m, So + (size_t)t * m, sn)
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
        sg[j] = sg2[j];
        prev[j] = prev2[j];
        prev[m + j] = prev2[m + j];
      }
      PDDP_GOALS(TAKE_NEXT)
    }
    if (owner && last) {
      J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
      if (rows) {
#pragma unroll
        for (int j = 0; j < n; ++j) Zo[(size_t)N * n + j] = z[j];
      }
      a.J_m[b] = J;
    }
  }
