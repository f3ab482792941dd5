// cem_refit_body.inc - one turn of CEM's pass 3, the text of cem_kernel,
// cem_goals_kernel (cem_kernel_body.inc) and cem_trial_kernel
// (cem_trial_kernel_body.inc): mppi_update_body.inc's structure with a weight
// of 0 or 1 and 2m sums per step.  The draws again for the elites alone -
// Philox and the AR(1), no dynamics; at every step t s1 (e) and s2 (e e,
// rounded) of the elites s >= 1 are summed over the group, the turns in their
// order by ONE lane per trajectory (the owner), who keeps the running sums
// between turns and in the last turn has the whole sums, forms the refitted
// mean and width of step t and steps the mean's rollout.  Every shuffle and
// barrier sits under launch-uniform control flow; the goal hooks sit where
// mppi_update_body.inc has them and enclose none: every lane takes its
// trajectory's rows under the launch-uniform `tracked` alone, TAKE_FIRST in
// every turn (pass 1 leaves P with the terminal row's goals).
//
// The including kernel has the turn's `s`, `roll`, `last`, cem_rank_body.inc's
// `ok`, `owner`, `Ke`, `cnt` (Ke as T), `scut`, PDDP_CEM_COST(s), `Ub` (the
// mean), `Sb`
// (the width), `Uo` / `So` (where s1 / s2 live between turns, and the refitted
// rows), `z0`, `smin`, `span`, `multi`, `part_sum`, `phase`, `P`,
// PDDP_GOALS(point), and defines
//   PDDP_CEM_CARRY           the owner re-reads the sums of the turns before
//   PDDP_CEM_KEEP_SUMS(acc)  the stores of the running sums of step t
//   PDDP_CEM_KEEP_ROWS       the stores of the refitted rows t (`z`, `un`, `sn`)
//   PDDP_CEM_CUT_J           the cut's cost: `Jcut`, or read again
//   PDDP_CEM_FLOOR(r)        std_min[r]: `smin[r]`, or read again
// It leaves `z` (x_N in the owner's last turn) and `J` in the including scope.
    // an elite: a finite cost that is not behind the cut.  Candidate 0 counts
    // in Ke and adds nothing; who is no elite adds 0 and makes no draws.
    bool draw = false;
    if (ok && s >= 1 && s < S) {
      const T Js = PDDP_CEM_COST(s);
      draw = is_finite(Js) && (Js < PDDP_CEM_CUT_J ||
                               (Js == PDDP_CEM_CUT_J && s <= scut));
    }
    const bool carry = PDDP_CEM_CARRY;
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
          PDDP_CEM_KEEP_SUMS(acc)
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
          PDDP_CEM_KEEP_ROWS
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
