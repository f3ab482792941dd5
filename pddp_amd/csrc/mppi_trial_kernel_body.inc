// mppi_trial_kernel_body.inc - the body of mppi_trial_kernel and of
// mppi_trial_goals_kernel (mppi_trial.hip): for every control step K
// iterations of mppi's three passes, the head's decision, the plant step and
// the shift, then the rollout of the shifted plan.  The including kernel has
// `shared`, `a` (MppiTrialArgs or MppiTrialGoalsArgs), sampled_common.hpp's
// hooks and defines, for this text and for trial_plant_body.inc,
//   PDDP_TRIAL_WINDOW_OF_C     first statement of control step c: the goals
//                              kernel moves its reference window, else empty
//   PDDP_TRIAL_PLANT_PROBLEM   `Pl`, the problem the applied step is logged
//                              under
//   PDDP_TRIAL_TERMINAL_GOAL   ahead of the trial's terminal cost: the goals
//                              kernel's row, else empty
// The first statements, the plant section and the closing rollout are the CEM
// trial's too (trial_prologue.inc, trial_plant_body.inc,
// trial_final_rollout.inc).
#define PDDP_TRIAL_ITERATIONS K = a.K
#include "trial_prologue.inc"
#undef PDDP_TRIAL_ITERATIONS

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

          // apply u to the plant of row b, log the trial, observe
#include "trial_plant_body.inc"
        }
      }
      hand_over();
    }
  }

#define PDDP_TRIAL_PLAN Ub
#include "trial_final_rollout.inc"
#undef PDDP_TRIAL_PLAN
