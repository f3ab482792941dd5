// mppi_update_body.inc - one turn of MPPI's pass 3, the text of the four
// kernels of mppi.hip and mppi_trial.hip: the draws again - Philox and the
// AR(1), no dynamics; at every step t the m products w_s e_{s,t} are summed
// over the group, the turns in their order by ONE lane per trajectory (the
// owner), which in the last turn has the whole sum, forms the weighted action
// and steps the weighted rollout with it.  Every shuffle and barrier sits
// under launch-uniform control flow; the goal hooks enclose none: every lane
// takes its trajectory's rows (one broadcast each), under the launch-uniform
// `tracked` alone.
//
// The including kernel has the turn's `s`, `roll`, `w`, `last`, and `owner`,
// `Ub`, `Uo` (where the running sum lives between turns), `z0`, `eta`, `span`,
// `multi`, `part_sum`, `phase`, `P`, PDDP_GOALS(point), and defines
//   PDDP_MPPI_CARRY          the owner re-reads the sum of the turns before
//   PDDP_MPPI_KEEP_SUM(acc)  the stores of the running sum of step t
//   PDDP_MPPI_KEEP_ROW       the stores of the weighted rollout's row t
// It leaves `z` (x_N in the owner's last turn) and `J` in the including scope.
    // candidate 0 adds its weight to eta and nothing to the sum; a weight of
    // 0 adds 0 whatever its draws are, so they are not made
    const bool draw = s >= 1 && w > T(0);
    const bool carry = PDDP_MPPI_CARRY;
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
      group_sum(p, span, multi, part_sum[phase]);
      phase ^= 1;
      if (owner) {
        T acc[m];
#pragma unroll
        for (int j = 0; j < m; ++j) acc[j] = turn > 0 ? prev[j] + p[j] : p[j];
        if (!last) {
          PDDP_MPPI_KEEP_SUM(acc)
        } else {
          T un[m], zn[n];
#pragma unroll
          for (int r = 0; r < m; ++r) {
            const T v = fma_of(astd[r], acc[r] / eta, ur[r]);
            un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
          }
          PDDP_MPPI_KEEP_ROW
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
