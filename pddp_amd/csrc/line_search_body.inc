// line_search_body.inc - one (trajectory, step size) candidate by its lane: the
// text of line_search_kernel and batch_line_search_kernel (problem_kernels.hip)
// and of the track_, weighted_ and track_weighted_line_search_kernel
// (goal_kernels.hpp).
// PDDP_PROBLEM_OF_B as in rollout_body.inc.  PDDP_GOALS(point): empty, or with
// a goal per time step what track_goal_hooks.inc does at TAKE_FIRST (write row
// 0's over P's), NEXT_ROW (name row t + 1, ahead of the nominal prefetch),
// PREFETCH_NEXT (request it, behind the nominal prefetch) and TAKE_NEXT (write it over P's at
// the end of the step; up to row N, the terminal cost's).
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr int GS = m + m * n;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = a.B * a.A;
  if (idx >= total) return;
  const int b = idx / a.A, ai = idx - b * a.A;
  if (a.active != nullptr && a.active[b] == 0) return;
  if (a.bwd_status != nullptr && a.bwd_status[b] != 0) return;
  PDDP_PROBLEM_OF_B
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  T umin[m], umax[m];
#pragma unroll
  for (int r = 0; r < m; ++r) {
    umin[r] = bounded ? a.u_min[r] : T(0);
    umax[r] = bounded ? a.u_max[r] : T(0);
  }
  const int N = a.N;
  const T alpha = a.alphas[ai];
  const T* Zb = a.Z + (size_t)b * (N + 1) * n;
  const T* Ub = a.U + (size_t)b * N * m;
  const T* Gb = a.gains + (size_t)b * N * GS;

  T z[n], zn[n], un[m];
  T zr[n], ur[m], gr[GS];  // this step's nominal z, u and gains
#pragma unroll
  for (int j = 0; j < n; ++j) {
    zr[j] = Zb[j];
    z[j] = zr[j];  // Z_new[0] = Z[0]                             (ilqr.py:690)
  }
#pragma unroll
  for (int j = 0; j < m; ++j) ur[j] = Ub[j];
#pragma unroll
  for (int j = 0; j < GS; ++j) gr[j] = Gb[j];
  PDDP_GOALS(TAKE_FIRST)

  // time-major output [b][t][alpha][.]: at every step the A lanes of a
  // trajectory write one contiguous A*n-word segment (see the note at
  // LineSearchArgs)
  T* Zci = a.Zc + ((size_t)b * (N + 1) * a.A + ai) * n;
  T* Uci = a.Uc + ((size_t)b * N * a.A + ai) * m;
  const size_t zstep = (size_t)a.A * n, ustep = (size_t)a.A * m;
  T J = T(0);
  for (int t = 0; t < N; ++t) {
    // prefetch the next step's nominal data before the dependent chain
    T zr2[n], ur2[m], gr2[GS];
    const int tn = (t + 1 < N) ? t + 1 : t;
    PDDP_GOALS(NEXT_ROW)
#pragma unroll
    for (int j = 0; j < n; ++j) zr2[j] = Zb[tn * n + j];
#pragma unroll
    for (int j = 0; j < m; ++j) ur2[j] = Ub[tn * m + j];
#pragma unroll
    for (int j = 0; j < GS; ++j) gr2[j] = Gb[tn * GS + j];
    PDDP_GOALS(PREFETCH_NEXT)

#pragma unroll
    for (int r = 0; r < m; ++r) {
      T du = alpha * gr[r];  // alpha * k[i]                      (ilqr.py:708)
      T s = T(0);
#pragma unroll
      for (int c = 0; c < n; ++c) s += (z[c] - zr[c]) * gr[m + r * n + c];
      du = du + s;  // + dz K^T                                   (ilqr.py:710)
      T v = ur[r] + du;
      un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
    }
#pragma unroll
    for (int j = 0; j < n; ++j) Zci[(size_t)t * zstep + j] = z[j];
#pragma unroll
    for (int j = 0; j < m; ++j) Uci[(size_t)t * ustep + j] = un[j];
    const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
    J += cost_value<T, MODEL>(P, z, un, tr, false);
    dynamics<T, MODEL, false>(P, z, un, tr, zn, nullptr, nullptr);
#pragma unroll
    for (int j = 0; j < n; ++j) {
      z[j] = zn[j];
      zr[j] = zr2[j];
    }
#pragma unroll
    for (int j = 0; j < m; ++j) ur[j] = ur2[j];
#pragma unroll
    for (int j = 0; j < GS; ++j) gr[j] = gr2[j];
    PDDP_GOALS(TAKE_NEXT)
  }
#pragma unroll
  for (int j = 0; j < n; ++j) Zci[(size_t)N * zstep + j] = z[j];
  const T lf = cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
  a.Jc[idx] = J + lf;  // L.sum(0) + l_f                           (ilqr.py:789)
