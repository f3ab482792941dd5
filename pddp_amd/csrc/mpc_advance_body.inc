// mpc_advance_body.inc - the hand-over between two MPC control steps of one
// trajectory by its lane: the text of mpc_advance_kernel and
// track_mpc_advance_kernel (mpc_advance.hip).  The goal hooks are one text,
// mpc_advance_goal_hooks.inc: PDDP_PROBLEM_OF_B declares `P`, the
// controller's model (its goals are read only where PDDP_PLANT_OF_B copies
// them); PDDP_PLANT_OF_B declares `Pl`, the plant of row b with the goals the
// step's stage cost is logged under; PDDP_TERMINAL_GOALS, at t == T - 1, is
// empty or writes the terminal cost's goals over Pl's.
// Three hooks separate the plant's state from what the controller sees; both
// kernels above define them empty (z0 is then both), mpc_advance_noisy_kernel
// (mpc_advance_noise.hip) puts its draws there: PDDP_PLANT_STATE, behind the
// read of z0 into `z`, may replace z by the plant's true state;
// PDDP_PLANT_STEPPED, behind the plant step and the disturbance, may add to
// `zn`; PDDP_NOMINAL_START, ahead of the write of z0 and Z[0], may keep the
// plant's `z` elsewhere and turn z into the observation.
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  if (blockIdx.x == 0 && a.n_live != nullptr) {
    for (int i = threadIdx.x; i < PDDP_LIVE_SHARDS; i += blockDim.x)
      a.n_live[i] = 0;
  }
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  if (a.mask != nullptr && a.mask[b] == 0) return;
  const int N = a.N, t = a.t, TT = a.T_;

  // 1. the controller as the step's rounds left it
  a.state_log[(size_t)b * TT + t] = a.state[b];
  a.live_log[(size_t)b * TT + t] = a.active[b] != 0 ? 1 : 0;

  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  T umin[m], umax[m];
#pragma unroll
  for (int r = 0; r < m; ++r) {
    umin[r] = bounded ? a.u_min[r] : T(0);
    umax[r] = bounded ? a.u_max[r] : T(0);
  }
  T* Zb = a.Z + (size_t)b * (N + 1) * n;
  T* Ub = a.U + (size_t)b * N * m;
  T* Xb = a.Xlog + (size_t)b * (TT + 1) * n;

  // the controller's model: the shared problem with row b of the table
  // written over it; Q, Qt and R are never written and stay scalar operands of
  // the kernel argument
  PDDP_PROBLEM_OF_B

  T z[n], zn[n], u[m], cur[m], nxt[m];
#pragma unroll
  for (int j = 0; j < n; ++j) z[j] = a.z0[(size_t)b * n + j];
  PDDP_PLANT_STATE
#pragma unroll
  for (int j = 0; j < m; ++j) {
    u[j] = Ub[j];
    if (bounded) u[j] = clamp1(u[j], umin[j], umax[j]);
  }
  // the warm start's first row, requested ahead of the plant step
  const int i1 = N > 1 ? 1 : 0;
#pragma unroll
  for (int j = 0; j < m; ++j) cur[j] = Ub[i1 * m + j];

  {
    // 2. - 4. apply u to the plant of row b, log the trial
    PDDP_PLANT_OF_B
    T w[n];
#pragma unroll
    for (int j = 0; j < n; ++j) w[j] = T(0);
    if (a.disturbance != nullptr) {
#pragma unroll
      for (int j = 0; j < n; ++j)
        w[j] = a.disturbance[((size_t)b * TT + t) * n + j];
    }
    T J = T(0);
    if (t > 0) J = a.Jcl[b];
#pragma unroll
    for (int j = 0; j < n; ++j) Xb[(size_t)t * n + j] = z[j];
#pragma unroll
    for (int j = 0; j < m; ++j) a.Ulog[((size_t)b * TT + t) * m + j] = u[j];
    const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
    J += cost_value<T, MODEL>(Pl, z, u, tr, false);
    dynamics<T, MODEL, false>(Pl, z, u, tr, zn, nullptr, nullptr);
    if (a.disturbance != nullptr) {
#pragma unroll
      for (int j = 0; j < n; ++j) zn[j] = zn[j] + w[j];
    }
    PDDP_PLANT_STEPPED
#pragma unroll
    for (int j = 0; j < n; ++j) z[j] = zn[j];
    if (t == TT - 1) {
      PDDP_TERMINAL_GOALS
#pragma unroll
      for (int j = 0; j < n; ++j) Xb[(size_t)TT * n + j] = z[j];
      J += cost_value<T, MODEL>(Pl, z, nullptr, trig_of<T, MODEL>(z), true);
    }
    a.Jcl[b] = J;
  }

  // 5. + 6. the shift (a plain copy of unclamped words; new row i is old row
  // i + 1, the last one repeated) and the rollout of the shifted nominal from
  // x' under the controller's model, in one loop over time.  Row i + 2 is read
  // before row i is written; the last row is read for the last time in the
  // iteration before it is written.
  PDDP_NOMINAL_START
#pragma unroll
  for (int j = 0; j < n; ++j) {
    a.z0[(size_t)b * n + j] = z[j];
    Zb[j] = z[j];
  }
  for (int i = 0; i < N; ++i) {
    const int i2 = (i + 2 < N) ? i + 2 : N - 1;
#pragma unroll
    for (int j = 0; j < m; ++j) nxt[j] = Ub[i2 * m + j];
#pragma unroll
    for (int j = 0; j < m; ++j) {
      Ub[i * m + j] = cur[j];
      u[j] = cur[j];
      if (bounded) u[j] = clamp1(u[j], umin[j], umax[j]);
    }
    const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
    dynamics<T, MODEL, false>(P, z, u, tr, zn, nullptr, nullptr);
#pragma unroll
    for (int j = 0; j < n; ++j) {
      z[j] = zn[j];
      Zb[(i + 1) * n + j] = z[j];
    }
#pragma unroll
    for (int j = 0; j < m; ++j) cur[j] = nxt[j];
  }

  // 7. re-arm: the words of reset_controller_state()       (ilqr.py:364-367)
  a.mu[b] = 0.0;
  a.delta[b] = 2.0;
  a.state[b] = PDDP_STATE_UNDEFINED;
  a.iter[b] = 1;
  a.active[b] = 1;
  a.fresh[b] = 1;
