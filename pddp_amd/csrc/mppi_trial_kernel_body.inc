// mppi_trial_kernel_body.inc - the body of mppi_trial_kernel and of
// mppi_trial_goals_kernel (mppi_trial.hip): for every control step K
// iterations of mppi's three passes, the head's decision, the plant step and
// the shift, then the rollout of the shifted plan.  The including kernel has
// `shared`, `a` (MppiTrialArgs or MppiTrialGoalsArgs), sampled_common.hpp's
// hooks and defines
//   PDDP_TRIAL_WINDOW_OF_C     first statement of control step c: the goals
//                              kernel moves its reference window, else empty
//   PDDP_TRIAL_PLANT_PROBLEM   `Pl`, the problem the applied step is logged
//                              under
//   PDDP_TRIAL_TERMINAL_GOAL   ahead of the trial's terminal cost: the goals
//                              kernel's row, else empty
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

  // the controller's model of trajectory b, as mppi's kernels hold it
  PDDP_PROBLEM_OF_B
  T umin[m], umax[m], astd[m];
#pragma unroll
  for (int r = 0; r < m; ++r) umin[r] = umax[r] = astd[r] = T(0);
  T lam = T(1);
  if (live) {
    PDDP_ROW_OF_B
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
    PDDP_TRIAL_WINDOW_OF_C

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
#include "sampled_argmin.inc"
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
          const T w = softmin_weight(Jcb[s], Jmin, lam);
          es[0] += w;
          es[1] += w * w;
        }
      }
      group_sum(es, span, multi, part_eta);
      const T eta = es[0];

      // ---- pass 3: the weighted perturbation, then the weighted rollout -----
      T Jw = inf;
      for (int turn = 0; turn < turns; ++turn) {
        const bool last = turn == turns - 1;  // (uniform over the launch)
        const int s = lane + turn * G;
        const uint64_t roll = offset + (uint64_t)((size_t)b * S + s);
        T w = T(0);
        if (ok && s < S) w = softmin_weight(Jcb[s], Jmin, lam);
        // (the running sum and the weighted sequence live in U_work)
#define PDDP_MPPI_CARRY owner && turn > 0
#define PDDP_MPPI_KEEP_SUM(acc) PDDP_COPY(m, Uo + (size_t)t * m, acc)
#define PDDP_MPPI_KEEP_ROW PDDP_COPY(m, Uo + (size_t)t * m, un)
#include "mppi_update_body.inc"
#undef PDDP_MPPI_KEEP_ROW
#undef PDDP_MPPI_KEEP_SUM
#undef PDDP_MPPI_CARRY
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

          // apply u to the plant of row b, log the trial (the hand-over's
          // steps 2 - 4 with its noise hooks) under `Pl`
          T x[n], xn[n];
#pragma unroll
          for (int j = 0; j < n; ++j)
            x[j] = a.v_std != nullptr ? a.x_true[(size_t)b * n + j] : z0[j];
          const uint64_t roll = a.rollout_offset + (uint64_t)b;
          const int step = a.step_offset + c;
          {
            PDDP_TRIAL_PLANT_PROBLEM
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
              PDDP_TRIAL_TERMINAL_GOAL
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
      hand_over();
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
