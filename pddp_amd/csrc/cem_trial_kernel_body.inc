// cem_trial_kernel_body.inc - the body of cem_trial_kernel (cem_trial.hip):
// for every control step I iterations of cem's three passes around (mean,
// width), the head's selects after each, then the plant step and the shifts;
// at the end the rollout of the shifted plan.  The including kernel has
// `shared`, `a` (CemTrialArgs), an empty PDDP_GOALS(point), cem.hip's width
// hooks for sampled_rollout_body.inc and the plain trial's plant hooks.
//
// The names the included texts read: `Ub` is the MEAN's rows and `Sb` the
// WIDTH's (both work buffers of the call); the incumbent - the plan - is U[b],
// `Ib`.  Passes 2 and 3 are cem_kernel's texts (cem_rank_body.inc,
// cem_refit_body.inc), with the rows always there and nothing kept of the
// ranking; the plant section and the closing rollout are the MPPI trial's
// (trial_plant_body.inc, trial_final_rollout.inc).
#define PDDP_TRIAL_ITERATIONS I = a.I
#include "trial_prologue.inc"
#undef PDDP_TRIAL_ITERATIONS

  // the controller's model of trajectory b, as the MPPI trial holds it
  ProblemT<T> P = shared;
  T umin[m], umax[m], smin[m];
#pragma unroll
  for (int r = 0; r < m; ++r) umin[r] = umax[r] = smin[r] = T(0);
  if (live) {
    if (a.table != nullptr)
      write_params_and_goals<T, MODEL>(P, a.table + (size_t)b * PDDP_BATCH_ROW);
#pragma unroll
    for (int r = 0; r < m; ++r) {
      umin[r] = bounded ? a.u_min[r] : T(0);
      umax[r] = bounded ? a.u_max[r] : T(0);
      smin[r] = a.std_min != nullptr ? a.std_min[r] : T(0);
    }
  }
  const size_t rows_b = (size_t)b * N * m;
  T* Ib = a.U + rows_b;       // the incumbent: the plan
  T* Gb = a.sigma + rows_b;   // the width the next control step starts from
  T* Ub = a.mean + rows_b;    // the mean
  T* Sb = a.width + rows_b;   // the width
  T* Uo = a.Um + rows_b;      // an iteration's refitted mean (and s1's sums)
  T* So = a.Sm + rows_b;      // an iteration's refitted width (and s2's sums)
  const T inf = std::numeric_limits<T>::infinity();
  const int turns = (S + G - 1) / G;

  __shared__ T stage[kClosedLoopThreads];
  __shared__ T cut_J[kWave];    // per lane group of the workgroup: the elite
  __shared__ int cut_s[kWave];  // of the highest rank, (J, s)
  __shared__ int part_fin[1][kWaves];
  __shared__ T part_sum[2][2 * m][kWaves];
  int phase = 0;

  // the trial's cost so far and the incumbent's cost: the head's own words
  T Jcl = T(0), Jinc = inf;
  if (head && a.t0 > 0) Jcl = a.Jcl[b];

  // step 1 of the launch's first control step (every later one: the head's
  // stores at the end of the step before)
  if (head) {
    for (int i = 0; i < N * m; ++i) {
      Ub[i] = Ib[i];
      Sb[i] = Gb[i];
    }
  }
  hand_over();

  for (int c = a.t0; c < a.t0 + a.count; ++c) {
    // what the controller sees at step c (the head's store of step c - 1)
    T z0[n];
#pragma unroll
    for (int j = 0; j < n; ++j) z0[j] = live ? a.z0[(size_t)b * n + j] : T(0);

    for (int k = 0; k < I; ++k) {
      const uint64_t offset =
          a.cand_offset +
          ((uint64_t)c * (uint64_t)I + (uint64_t)k) * a.iter_stride;
      T* Jcb = a.Jc + (a.log_costs != 0
                           ? (((size_t)b * TT + c) * I + k) * (size_t)S
                           : (size_t)b * S);

      // ---- pass 1: the candidates around the mean, row t of the width -------
      T J0 = inf;
      for (int turn = 0; turn < turns; ++turn) {
        const int s = lane + turn * G;
        if (live && s < S) {
          const uint64_t roll = offset + (uint64_t)((size_t)b * S + s);
          const bool base = s == 0;  // the mean is a candidate
#include "sampled_rollout_body.inc"
          Jcb[s] = J;
          if (base) J0 = J;  // (the head's: lane 0 holds candidate 0)
        }
      }

      // ---- pass 2: the ranks; nothing of them is kept ------------------------
#define PDDP_CEM_COST(s) Jcb[s]
#define PDDP_CEM_KEEP(point)
#include "cem_rank_body.inc"
#undef PDDP_CEM_KEEP

      // ---- pass 3: the refit, then the new mean's cost ----------------------
      // (the running sums of a lane's turns live in Um (s1) and Sm (s2), which
      // are neither the mean, the width nor the plan - the host's test)
      const T cnt = (T)Ke;
      T Jm = inf;
      for (int turn = 0; turn < turns; ++turn) {
        const bool last = turn == turns - 1;  // (uniform over the launch)
        const int s = lane + turn * G;
        const uint64_t roll = offset + (uint64_t)((size_t)b * S + s);
#define PDDP_CEM_CARRY owner && turn > 0
#define PDDP_CEM_KEEP_SUMS(acc)                                                \
  PDDP_COPY(m, Uo + (size_t)t * m, acc)                                        \
  PDDP_COPY(m, So + (size_t)t * m, acc + m)
#define PDDP_CEM_KEEP_ROWS                                                     \
  PDDP_COPY(m, Uo + (size_t)t * m, un)                                         \
  PDDP_COPY(m, So + (size_t)t * m, sn)
#define PDDP_CEM_CUT_J Jcut
#define PDDP_CEM_FLOOR(r) smin[r]
#include "cem_refit_body.inc"
#undef PDDP_CEM_FLOOR
#undef PDDP_CEM_CUT_J
#undef PDDP_CEM_KEEP_ROWS
#undef PDDP_CEM_KEEP_SUMS
#undef PDDP_CEM_CARRY
#undef PDDP_CEM_COST
        if (owner && last) {
          J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
          Jm = J;
        }
      }

      // ---- the head: cem's selects, after the last iteration the plant ------
      if (head) {
        const size_t bc = (size_t)b * TT + c;
        const size_t ck = bc * I + k;
        if (k == 0) {  // the mean is candidate 0 and, here, the incumbent
          Jinc = J0;
          if (a.Jtrace_log != nullptr) a.Jtrace_log[bc * (I + 1)] = Jinc;
        }
        if (a.Jm_log != nullptr) a.Jm_log[ck] = Jm;
        if (a.nelite_log != nullptr) a.nelite_log[ck] = Ke;
        // (without a finite cost J_m is +inf and Um, Sm are not written)
        const bool better = is_finite(Jm) && Jm <= Jinc;
        const bool moved = Ke > 0;
        if (better) {
          for (int i = 0; i < N * m; ++i) Ib[i] = Uo[i];
          Jinc = Jm;
        }
        if (a.Jtrace_log != nullptr)
          a.Jtrace_log[bc * (I + 1) + k + 1] = Jinc;
        if (k < I - 1) {
          if (moved) {
            for (int i = 0; i < N * m; ++i) {
              Ub[i] = Uo[i];
              Sb[i] = So[i];
            }
          }
        } else {
          // the step's plan is the incumbent: logged, its first row applied,
          // U[b] and the next step's mean its shift (plain copies of unclamped
          // words, the last row repeated).  The width after the last
          // iteration is logged; the next step starts from sigma0[b], or from
          // its shift.  In place, row i + 1 is read before row i is written.
          const T* wsrc = moved ? So : Sb;
          const T* S0b = a.sigma0 != nullptr ? a.sigma0 + rows_b : nullptr;
          T* Pb = a.plan_log != nullptr ? a.plan_log + bc * N * m : nullptr;
          T* Wl = a.std_log != nullptr ? a.std_log + bc * N * m : nullptr;
          T cur[m], nxt[m], wcur[m], wnxt[m], u[m];
#pragma unroll
          for (int j = 0; j < m; ++j) {
            cur[j] = Ib[j];
            wcur[j] = wsrc[j];
            u[j] = bounded ? clamp1(cur[j], umin[j], umax[j]) : cur[j];
          }
          for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int j = 0; j < m; ++j) {
              nxt[j] = i + 1 < N ? Ib[(i + 1) * m + j] : cur[j];
              wnxt[j] = i + 1 < N ? wsrc[(i + 1) * m + j] : wcur[j];
            }
#pragma unroll
            for (int j = 0; j < m; ++j) {
              if (Pb != nullptr) Pb[i * m + j] = cur[j];
              if (Wl != nullptr) Wl[i * m + j] = wcur[j];
              const T wnew = S0b != nullptr ? S0b[i * m + j] : wnxt[j];
              Ib[i * m + j] = nxt[j];
              Ub[i * m + j] = nxt[j];
              Gb[i * m + j] = wnew;
              Sb[i * m + j] = wnew;
              cur[j] = nxt[j];
              wcur[j] = wnxt[j];
            }
          }

          // apply u to the plant of row b, log the trial, observe
#include "trial_plant_body.inc"
        }
      }
      // the head's stores - the plan, the mean, the width, z0 - ahead of the
      // group's loads; the barrier also separates this iteration's reads of
      // the cut from the next one's stores
      hand_over();
    }
  }

#define PDDP_TRIAL_PLAN Ib
#include "trial_final_rollout.inc"
#undef PDDP_TRIAL_PLAN
