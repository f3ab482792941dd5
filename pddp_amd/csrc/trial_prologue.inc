// trial_prologue.inc - the first statements of a sampled trial's kernel
// (mppi_trial_kernel_body.inc, cem_trial_kernel_body.inc): mppi_kernel's
// mapping - a trajectory owns a lane group of G lanes, lane 0 of the group (the
// head) does what is done once per trajectory.  `a` is the kernel's block.  The
// including text defines
//   PDDP_TRIAL_ITERATIONS   its iterations per control step as a declarator,
//                           `K = a.K` or `I = a.I`: a hook for the place of
//                           the declaration alone (DESIGN.md 3.4u)
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr int kWaves = kClosedLoopThreads / kWave;
  const int tid = threadIdx.x, G = a.G, N = a.N, S = a.S, PDDP_TRIAL_ITERATIONS,
            TT = a.TT;
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
