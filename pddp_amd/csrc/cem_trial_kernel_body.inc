// cem_trial_kernel_body.inc - the body of cem_trial_kernel (cem_trial.hip):
// for every control step I iterations of cem's three passes around (mean,
// width), the head's selects after each, then the plant step and the shifts;
// at the end the rollout of the shifted plan.  The including kernel has
// `shared`, `a` (CemTrialArgs), an empty PDDP_GOALS(point) and cem.hip's width
// hooks for sampled_rollout_body.inc.
//
// The names the included rollout text reads: `Ub` is the MEAN's rows and `Sb`
// the WIDTH's (both work buffers of the call); the incumbent - the plan - is
// U[b], `Ib`.  Passes 2 and 3 are cem_kernel_body.inc's, with the rows always
// there, no rank array and no Zm.
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr int kWaves = kClosedLoopThreads / kWave;
  const int tid = threadIdx.x, G = a.G, N = a.N, S = a.S, I = a.I, TT = a.TT;
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

      // ---- pass 2: the ranks (cem_kernel_body.inc's pass 2) -----------------
      // Every lane stages the cost it wrote itself.  cut_J / cut_s are written
      // behind the barriers of this pass and read behind the one that closes
      // it, under `ok` alone: an iteration without a finite cost writes no cut
      // and reads none, whatever the iteration before left there.
      int fin_[1] = {0};
      for (int turn = 0; turn < turns; ++turn) {
        const int s = lane + turn * G;
        if (live && s < S) fin_[0] += is_finite(Jcb[s]) ? 1 : 0;
      }
      group_sum(fin_, span, multi, part_fin);
      const int n_fin = fin_[0];
      const int Ke = a.K < n_fin ? a.K : n_fin;
      for (int turn = 0; turn < turns; ++turn) {
        const int s = lane + turn * G;
        const bool mine = live && s < S;
        const T Js = mine ? Jcb[s] : inf;
        const bool fin = mine && is_finite(Js);
        int below = 0;
        for (int ch = 0; ch < turns; ++ch) {
          const int sc = lane + ch * G;
          T v = inf;
          if (live && sc < S) {
            v = Jcb[sc];
            v = is_finite(v) ? v : inf;
          }
          __syncthreads();  // (the chunk before has been read)
          stage[tid] = v;
          __syncthreads();
          // (ch and turn are launch-uniform: only the lane's own chunk needs
          // the index)
          const T* chunk = stage + group * G;
          if (ch < turn) {
#pragma unroll 8
            for (int q = 0; q < G; ++q) below += chunk[q] <= Js ? 1 : 0;
          } else if (ch > turn) {
#pragma unroll 8
            for (int q = 0; q < G; ++q) below += chunk[q] < Js ? 1 : 0;
          } else {
#pragma unroll 8
            for (int q = 0; q < G; ++q) {
              const T o = chunk[q];
              below += (o < Js || (o == Js && q < lane)) ? 1 : 0;
            }
          }
        }
        if (fin && below == Ke - 1) {
          cut_J[group] = Js;
          cut_s[group] = s;
        }
      }
      __syncthreads();
      const bool ok = live && n_fin > 0;
      const bool owner = ok && lane == 0;
      const T Jcut = ok ? cut_J[group] : -inf;
      const int scut = ok ? cut_s[group] : -1;

      // ---- pass 3: the refit, then the new mean's cost ----------------------
      // (cem_kernel_body.inc's pass 3: the running sums of a lane's turns live
      // in Um (s1) and Sm (s2), which are neither the mean, the width nor the
      // plan - the host's test)
      const T cnt = (T)Ke;
      T Jm = inf;
      for (int turn = 0; turn < turns; ++turn) {
        const bool last = turn == turns - 1;  // (uniform over the launch)
        const int s = lane + turn * G;
        const uint64_t roll = offset + (uint64_t)((size_t)b * S + s);
        bool draw = false;
        if (ok && s >= 1 && s < S) {
          const T Js = Jcb[s];
          draw = is_finite(Js) && (Js < Jcut || (Js == Jcut && s <= scut));
        }
        const bool carry = owner && turn > 0;
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
        T J = T(0);
        for (int t = 0; t < N; ++t) {
          // the next step's mean, width and carried sums, ahead of the chain
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
              PDDP_COPY(m, Uo + (size_t)t * m, acc)
              PDDP_COPY(m, So + (size_t)t * m, acc + m)
            } else {
              T un[m], sn[m], zn[n];
#pragma unroll
              for (int r = 0; r < m; ++r) {
                const T ebar = acc[r] / cnt;
                const T var = fma_of(-ebar, ebar, acc[m + r] / cnt);
                const T V = (Ke > 1 && var > T(0)) ? var : T(0);
                // (explicit fmas: each product is rounded where the law rounds)
                const T g = fma_of(a.step, sg[r], T(0));
                const T v = fma_of(g, ebar, ur[r]);
                un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
                const T sd = fma_of(sg[r], sqrt_of(V), T(0));
                const T w = fma_of(a.step, sd - sg[r], sg[r]);
                sn[r] = w > smin[r] ? w : smin[r];
              }
              PDDP_COPY(m, Uo + (size_t)t * m, un)
              PDDP_COPY(m, So + (size_t)t * m, sn)
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
        }
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

          // apply u to the plant of row b, log the trial (the MPPI trial's
          // plant section) under `Pl`
          T x[n], xn[n];
#pragma unroll
          for (int j = 0; j < n; ++j)
            x[j] = a.v_std != nullptr ? a.x_true[(size_t)b * n + j] : z0[j];
          const uint64_t roll = a.rollout_offset + (uint64_t)b;
          const int step = a.step_offset + c;
          {
            ProblemT<T> Pl = P;
            if (a.plant != nullptr)
              write_params_and_goals<T, MODEL>(
                  Pl, a.plant + (size_t)b * PDDP_BATCH_ROW);
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
      // the head's stores - the plan, the mean, the width, z0 - ahead of the
      // group's loads; the barrier also separates this iteration's reads of
      // the cut from the next one's stores
      hand_over();
    }
  }

  // the rollout of the shifted plan, clamped, from what the controller sees
  // now, under the controller's model (the head re-reads its own stores)
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
        u[j] = Ib[i * m + j];
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
