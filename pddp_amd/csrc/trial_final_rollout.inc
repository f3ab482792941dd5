// trial_final_rollout.inc - the end of a sampled trial's launch, the text of
// the kernels of mppi_trial.hip and cem_trial.hip: the rollout of the shifted
// plan, clamped, from what the controller sees now, under the controller's
// model `P` (the head re-reads its own stores); it reads no goal and no
// weight.  The including kernel defines PDDP_TRIAL_PLAN, the plan's rows of
// trajectory b (`Ub` in MPPI, `Ib` in CEM).
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
        u[j] = PDDP_TRIAL_PLAN[i * m + j];
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
