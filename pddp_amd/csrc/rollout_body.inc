// rollout_body.inc - the nominal rollout of one trajectory by its lane: the
// text of nominal_rollout_kernel and batch_rollout_kernel (problem_kernels.hip,
// which says why this is an included text and not a device function).
// PDDP_PROBLEM_OF_B declares `P`, the problem of trajectory b, where the kernel
// argument is not it.
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  if (a.mask != nullptr && a.mask[b] == 0) return;
  PDDP_PROBLEM_OF_B
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  T z[n], zn[n], u[m], umin[m], umax[m];
#pragma unroll
  for (int r = 0; r < m; ++r) {
    umin[r] = bounded ? a.u_min[r] : T(0);
    umax[r] = bounded ? a.u_max[r] : T(0);
  }
  T* Zb = a.Z + (size_t)b * (a.N + 1) * n;
  const T* Ub = a.U + (size_t)b * a.N * m;
#pragma unroll
  for (int j = 0; j < n; ++j) {
    z[j] = a.z0[(size_t)b * n + j];
    Zb[j] = z[j];
  }
  for (int t = 0; t < a.N; ++t) {
#pragma unroll
    for (int j = 0; j < m; ++j) {
      u[j] = Ub[t * m + j];
      if (bounded) u[j] = clamp1(u[j], umin[j], umax[j]);
    }
    const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
    dynamics<T, MODEL, false>(P, z, u, tr, zn, nullptr, nullptr);
#pragma unroll
    for (int j = 0; j < n; ++j) {
      z[j] = zn[j];
      Zb[(t + 1) * n + j] = z[j];
    }
  }
