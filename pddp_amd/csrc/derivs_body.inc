// derivs_body.inc - the derivative records of one trajectory by its workgroup:
// the text of derivs_kernel and batch_derivs_kernel (problem_kernels.hip) and
// of the track_, weighted_ and track_weighted_derivs_kernel (goal_kernels.hpp).
// PDDP_PROBLEM_OF_B as in rollout_body.inc; PDDP_SPLIT_TERMINAL: record_of is
// called under `if (terminal)` with the flag a constant in each call (see
// batch_derivs_kernel).  PDDP_GOALS(point): empty, or with a goal per time
// step what track_goal_hooks.inc does at TAKE_X and TAKE_U (write step t's
// goals over P's, the latter where the step has an action).
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr RecLayout lay(n, m);
  constexpr int S = lay.stride;
  constexpr int LD = kDerivThreads + 1;  // +1: conflict-free transposed reads
  __shared__ T stage[S * LD];
  __shared__ T Lsum[kDerivThreads];

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  if (a.mask != nullptr && a.mask[b] == 0) return;
  PDDP_PROBLEM_OF_B
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  const int N = a.N;
  const T* Zb = a.Z + (size_t)b * (N + 1) * n;
  const T* Ub = a.U + (size_t)b * N * m;
  T* rec_b = a.rec + (size_t)b * (N + 1) * S;
  T Jacc = T(0);  // only meaningful in lane 0

  for (int t0 = 0; t0 <= N; t0 += kDerivThreads) {
    const int t = t0 + tid;
    T l = T(0);
    if (t <= N) {
      T z[n], un[m], w[S];
#pragma unroll
      for (int j = 0; j < n; ++j) z[j] = Zb[t * n + j];
      const bool terminal = (t == N);
#pragma unroll
      for (int j = 0; j < m; ++j) un[j] = terminal ? T(0) : Ub[t * m + j];
      PDDP_GOALS(TAKE_X)
#if PDDP_SPLIT_TERMINAL
      if (terminal) {
        l = record_of<T, MODEL>(P, z, un, true, bounded, a.u_min, a.u_max, w);
      } else {
        PDDP_GOALS(TAKE_U)
        l = record_of<T, MODEL>(P, z, un, false, bounded, a.u_min, a.u_max, w);
      }
#else
      l = record_of<T, MODEL>(P, z, un, terminal, bounded, a.u_min, a.u_max, w);
#endif
      T* col = stage + tid;
#pragma unroll
      for (int j = 0; j < S; ++j) col[j * LD] = w[j];
      a.L[(size_t)b * (N + 1) + t] = l;
    }
    Lsum[tid] = l;
    __syncthreads();
    // coalesced write-out of this chunk's records
    const int nrec = min(kDerivThreads, N + 1 - t0);
    T* dst = rec_b + (size_t)t0 * S;
    for (int o = tid; o < nrec * S; o += kDerivThreads) {
      const int r = o / S, w = o - r * S;
      dst[o] = stage[w * LD + r];
    }
    if (tid == 0)
      for (int r = 0; r < nrec; ++r) Jacc += Lsum[r];  // L.sum(), in t order
    __syncthreads();
  }
  if (tid == 0) {
    a.J[b] = Jacc;
    if (a.state != nullptr) a.state[b] = PDDP_STATE_UNDEFINED;
  }
