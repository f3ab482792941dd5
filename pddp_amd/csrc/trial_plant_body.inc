// trial_plant_body.inc - the plant section of a sampled trial's control step c,
// the text of mppi_trial_kernel, mppi_trial_goals_kernel
// (mppi_trial_kernel_body.inc) and cem_trial_kernel
// (cem_trial_kernel_body.inc): the head applies `u` to the plant of row b and
// logs the trial (the hand-over's steps 2 - 4 with its noise hooks) under
// `Pl`, observes, and stores what the controller sees next in z0[b].
//
// The including kernel is inside `if (head)` of control step c and has `u`
// (the clamped first row of the step's plan), `z0`, `bc` (b TT + c), `TT`,
// `Jcl`, `P`, and defines
//   PDDP_TRIAL_PLANT_PROBLEM   `Pl`, the problem the applied step is logged
//                              under
//   PDDP_TRIAL_TERMINAL_GOAL   ahead of the trial's terminal cost: the goals
//                              kernel's row, else empty
// (the plain kernels': sampled_common.hpp's PDDP_PLAIN_TRIAL_*).
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
