// sampled_rollout_body.inc - one candidate (b, s) of the sampling planners
// rolled out by its lane: the text of all six kernels (shoot.hip, mppi.hip,
// mppi_trial.hip: the plain kernel and the goals kernel of each) - the
// action's perturbation, the clamp, cost, dynamics and the AR(1) update of e,
// with the goals of `P` taken step by step where the kernel has goal hooks.
//
// The including kernel has `a` (seed, beta, gamma), `P` (its
// PDDP_PROBLEM_OF_B), `z0`, `Ub`, `roll`, `base`, `astd`, `umin`, `umax`,
// `bounded`, `N`, `b` and defines
//   PDDP_SAMPLED_AFTER_E0   behind the first draws: empty, or declarations
//                           the kernel was compiled with at this place (a
//                           hook for statement order alone: shoot.hip)
//   PDDP_SAMPLED_KEEP_ROW   after the clamp: empty, or the stores of row t
//   PDDP_SAMPLED_WIDTH(r)   optional, with PDDP_SAMPLED_WIDTH_REQUEST: the
//                           width of component r at step t, and what asks for
//                           row t + 1 of a width per step next to `ur2`
//                           (cem.hip's sigma[b]).  A kernel that defines
//                           neither draws with `astd[r]` and asks for nothing:
//                           the text of the six kernels as it was.
//   PDDP_GOALS(point)       TAKE_FIRST ahead of the time loop, REQUEST_NEXT
//                           behind the step's draws (row t + 1, ahead of the
//                           dependent chain), TAKE_NEXT at the end of the step
//                           (up to row N, the terminal cost's)
// It leaves `z` (x_N) and `J` in the including scope.  An included text, not
// a device function: csrc/Makefile's note on contraction (DESIGN.md 3.4f).
#ifndef PDDP_SAMPLED_WIDTH
#define PDDP_SAMPLED_WIDTH(r) astd[r]
#define PDDP_SAMPLED_WIDTH_REQUEST
#define PDDP_SAMPLED_WIDTH_IS_ASTD
#endif
      T z[n], zn[n], un[m], ur[m], e[m];
#pragma unroll
      for (int j = 0; j < n; ++j) z[j] = z0[j];
#pragma unroll
      for (int j = 0; j < m; ++j) ur[j] = Ub[j];
      draw_units<T, m>(a.seed, roll, 0, kSampledStream, e);  // e_0 = xi_0
      PDDP_SAMPLED_AFTER_E0
      PDDP_GOALS(TAKE_FIRST)
      T J = T(0);
      for (int t = 0; t < N; ++t) {
        // the next step's base action, normals and goals, ahead of the chain
        T ur2[m], xi[m];
        const int tn = (t + 1 < N) ? t + 1 : t;
#pragma unroll
        for (int j = 0; j < m; ++j) ur2[j] = Ub[tn * m + j];
        PDDP_SAMPLED_WIDTH_REQUEST
        draw_units<T, m>(a.seed, roll, t + 1, kSampledStream, xi);
        PDDP_GOALS(REQUEST_NEXT)
#pragma unroll
        for (int r = 0; r < m; ++r) {
          const T v =
              base ? ur[r] : fma_of(PDDP_SAMPLED_WIDTH(r), e[r], ur[r]);
          un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
        }
        PDDP_SAMPLED_KEEP_ROW
        const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
        J += cost_value<T, MODEL>(P, z, un, tr, false);
        dynamics<T, MODEL, false>(P, z, un, tr, zn, nullptr, nullptr);
#pragma unroll
        for (int j = 0; j < n; ++j) z[j] = zn[j];
#pragma unroll
        for (int j = 0; j < m; ++j) {
          ur[j] = ur2[j];
          e[j] = fma_of(a.beta, e[j], a.gamma * xi[j]);
        }
        PDDP_GOALS(TAKE_NEXT)
      }
      J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
#ifdef PDDP_SAMPLED_WIDTH_IS_ASTD
#undef PDDP_SAMPLED_WIDTH_IS_ASTD
#undef PDDP_SAMPLED_WIDTH_REQUEST
#undef PDDP_SAMPLED_WIDTH
#endif
