// closed_loop_body.inc - the closed-loop rollouts of a lane and the statistics
// of a controller's costs: the text of closed_loop_kernel,
// closed_loop_noisy_kernel and closed_loop_track_kernel (closed_loop.hip).  The
// including kernel has
// `shared`, `a` (ClosedLoopArgs), `Znom`, `Unom`, `gains` and defines
//   PDDP_NOISE_LEVELS      after the bounds: empty, or the launch's noise levels
//   PDDP_NOISE_OF_ROLLOUT  before the time loop: empty, or what rollout (b, s)
//                          draws ahead of its first step
//   PDDP_NOISE_OF_STEP     after the next row is requested: empty, or this
//                          step's draws
//   PDDP_SEEN(c)           component c of the state the controller sees at this
//                          step: z[c], or with measurement noise
//   PDDP_NEXT(j)           component j of the next state: zn[j], or with process
//                          noise
// and, for the goals of `P` (empty where a rollout has ONE goal: the plant
// row's or the shared problem's; closed_loop_track_kernel takes them from a
// reference row, as track_goal_hooks.inc at line_search_body.inc's hooks)
//   PDDP_GOALS_TAKE_FIRST    ahead of the time loop: row 0's over P's
//   PDDP_GOALS_REQUEST_NEXT  behind the step's draws: row t + 1, ahead of the
//                            dependent chain
//   PDDP_GOALS_TAKE_NEXT     at the end of the step: the requested row over P's
//                            (up to row N, the terminal cost's)
// An included text, not a device function: each kernel compiles to the
// instructions it would have typed out (DESIGN.md 3.4f, 3.4g).
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr int GS = m + m * n;
  const int tid = threadIdx.x, G = a.G, N = a.N, S = a.S;
  const int group = tid / G, lane = tid - group * G;
  const long long bl = (long long)blockIdx.x * (blockDim.x / G) + group;
  const bool in_batch = bl < a.B;
  const int b = in_batch ? (int)bl : 0;
  // (nothing of a skipped trajectory is read or written)
  const bool live = in_batch && (a.active == nullptr || a.active[b] != 0);

  CostStats<T> st{T(0), std::numeric_limits<T>::infinity(),
                  -std::numeric_limits<T>::infinity(), 0};
  if (live) {
    const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
    const bool feedback = gains != nullptr;
    const bool keep = a.Xc != nullptr;
    T umin[m], umax[m];
#pragma unroll
    for (int r = 0; r < m; ++r) {
      umin[r] = bounded ? a.u_min[r] : T(0);
      umax[r] = bounded ? a.u_max[r] : T(0);
    }
    PDDP_NOISE_LEVELS
    const T* Zb = Znom + (size_t)b * (N + 1) * n;
    const T* Ub = Unom + (size_t)b * N * m;
    // (only the K part of a gains row is read)
    const T* Kb = feedback ? gains + (size_t)b * N * GS + m : nullptr;
    const size_t xstep = (size_t)S * n, ustep = (size_t)S * m;

    for (int s = lane; s < S; s += G) {
      const size_t bs = (size_t)b * S + s;
      // the plant of this rollout: the shared problem with row (b, s) written
      // over it, in registers for the whole rollout; Q, Qt and R are never
      // written and stay scalar operands of the kernel argument
      ProblemT<T> P = shared;
      // (write_params_and_goals' statements in place: called, seven of the
      // eight kernels come out as other instructions, DESIGN.md 3.4f)
      if (a.plant != nullptr) {
        const T* row = a.plant + bs * PDDP_BATCH_ROW;
        P.dt = row[PDDP_BATCH_PARAMS];
#pragma unroll
        for (int i = 0; i < kModelParamCount<MODEL> - 1; ++i)
          P.p[i] = row[PDDP_BATCH_PARAMS + 1 + i];
#pragma unroll
        for (int i = 0; i < D::na; ++i) P.goal[i] = row[PDDP_BATCH_X_GOAL + i];
#pragma unroll
        for (int i = 0; i < D::m; ++i) P.ugoal[i] = row[PDDP_BATCH_U_GOAL + i];
      }

      T z[n], zn[n], un[m];
      T zr[n], ur[m], kr[m * n];  // this step's nominal z, u and K
#pragma unroll
      for (int j = 0; j < n; ++j) zr[j] = Zb[j];
#pragma unroll
      for (int j = 0; j < n; ++j) z[j] = zr[j];
      if (a.z0s != nullptr) {
#pragma unroll
        for (int j = 0; j < n; ++j) z[j] = a.z0s[bs * n + j];
      }
#pragma unroll
      for (int j = 0; j < m; ++j) ur[j] = Ub[j];
#pragma unroll
      for (int j = 0; j < m * n; ++j) kr[j] = T(0);
      if (feedback) {
#pragma unroll
        for (int j = 0; j < m * n; ++j) kr[j] = Kb[j];
      }
      PDDP_NOISE_OF_ROLLOUT
      PDDP_GOALS_TAKE_FIRST

      // time-major output [b][t][s][.]: at every step the lanes of a
      // trajectory write one contiguous segment (the note at LineSearchArgs)
      T* Xci = keep ? a.Xc + ((size_t)b * (N + 1) * S + s) * n : nullptr;
      T* Uci = keep ? a.Uc + ((size_t)b * N * S + s) * m : nullptr;
      T J = T(0);
      for (int t = 0; t < N; ++t) {
        // the next step's nominal row, requested ahead of the dependent chain
        T zr2[n], ur2[m], kr2[m * n];
        const int tn = (t + 1 < N) ? t + 1 : t;
#pragma unroll
        for (int j = 0; j < n; ++j) zr2[j] = Zb[tn * n + j];
#pragma unroll
        for (int j = 0; j < m; ++j) ur2[j] = Ub[tn * m + j];
#pragma unroll
        for (int j = 0; j < m * n; ++j) kr2[j] = T(0);
        if (feedback) {
#pragma unroll
          for (int j = 0; j < m * n; ++j) kr2[j] = Kb[(size_t)tn * GS + j];
        }
        PDDP_NOISE_OF_STEP
        PDDP_GOALS_REQUEST_NEXT

#pragma unroll
        for (int r = 0; r < m; ++r) {
          T v = ur[r];
          if (feedback) {  // u + K (x - z)                 (ilqr.py:345-355)
            T du = T(0);
#pragma unroll
            for (int c = 0; c < n; ++c)
              du += (PDDP_SEEN(c) - zr[c]) * kr[r * n + c];
            v = v + du;
          }
          un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
        }
        if (keep) {
#pragma unroll
          for (int j = 0; j < n; ++j) Xci[(size_t)t * xstep + j] = z[j];
#pragma unroll
          for (int j = 0; j < m; ++j) Uci[(size_t)t * ustep + j] = un[j];
        }
        const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
        J += cost_value<T, MODEL>(P, z, un, tr, false);
        dynamics<T, MODEL, false>(P, z, un, tr, zn, nullptr, nullptr);
#pragma unroll
        for (int j = 0; j < n; ++j) {
          z[j] = PDDP_NEXT(j);
          zr[j] = zr2[j];
        }
#pragma unroll
        for (int j = 0; j < m; ++j) ur[j] = ur2[j];
#pragma unroll
        for (int j = 0; j < m * n; ++j) kr[j] = kr2[j];
        PDDP_GOALS_TAKE_NEXT
      }
      if (keep) {
#pragma unroll
        for (int j = 0; j < n; ++j) Xci[(size_t)N * xstep + j] = z[j];
      }
      J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
      a.Jc[bs] = J;
      if (is_finite(J)) merge(st, J, J, J, 1);
    }
  }
  if (a.stats == nullptr) return;  // (the whole launch)

  // The costs of a trajectory meet in a fixed order: the lane's own in s
  // order (above), a butterfly over the group's lanes of a wavefront (both
  // partners of a pair form the same sum: a + b == b + a), then the
  // workgroup's wavefronts in their order through LDS.  Idle lanes hold the
  // neutral element.  No atomics.
  const int span = G < kWave ? G : kWave;
  for (int off = 1; off < span; off <<= 1)
    merge(st, __shfl_xor(st.sum, off), __shfl_xor(st.lo, off),
          __shfl_xor(st.hi, off), __shfl_xor(st.count, off));
  if (blockDim.x > kWave) {  // one trajectory over several wavefronts
    constexpr int W = kClosedLoopThreads / kWave;
    __shared__ T part[W][3];
    __shared__ int part_count[W];
    const int wave = tid / kWave;
    if (tid % kWave == 0) {
      part[wave][0] = st.sum;
      part[wave][1] = st.lo;
      part[wave][2] = st.hi;
      part_count[wave] = st.count;
    }
    __syncthreads();
    if (tid == 0)
      for (int w = 1; w < (int)blockDim.x / kWave; ++w)
        merge(st, part[w][0], part[w][1], part[w][2], part_count[w]);
  }
  if (live && lane == 0) {
    const T inf = std::numeric_limits<T>::infinity();
    const bool any = st.count > 0;
    T* out = a.stats + (size_t)b * 4;
    out[0] = any ? st.sum / T(st.count) : inf;
    out[1] = any ? st.lo : inf;
    out[2] = any ? st.hi : inf;
    out[3] = T(st.count);
  }
