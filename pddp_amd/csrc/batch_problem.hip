// batch_problem.hip - the three problem kernels with a PER-TRAJECTORY problem:
// nominal rollout, derivative records and line search where every trajectory
// b has its own model parameters and goals, row b of `table`
// [B][PDDP_BATCH_ROW] (include/pddp_hip.h: params, x_goal, u_goal).  Q, Q_term,
// R, the model, the encoding and the action bounds stay those of the
// pddp_problem passed by value.
//
// Each lane (rollout, line search) or workgroup (records) copies the by-value
// ProblemT, overwrites dt, p[], goal[] and ugoal[] from its row ONCE ahead of
// the time loop and hands the copy to the device functions of models.hpp
// unchanged: the maths is that of problem_kernels.hip by construction.  The
// overwritten fields live in vector registers from then on (27 words for the
// double cartpole, 12 for the cartpole); Q, Qt and R are never written and stay
// scalar operands of the kernel argument.
//
// The backward sweep and the accept kernel never see the problem, so a round
// with a table is derivs(batch), backward, line_search(batch), accept.
#include "models.hpp"
#include "problem_args.hpp"

namespace pddp {

// parameters of each model, dt included (include/pddp_problem.h)
template <int MODEL>
constexpr int kParamCount = MODEL == PDDP_MODEL_CARTPOLE          ? 6
                            : MODEL == PDDP_MODEL_DOUBLE_CARTPOLE ? 8
                            : MODEL == PDDP_MODEL_PENDULUM        ? 5
                                                                  : 3;

// The shared problem with trajectory b's row written over it.  Entries of the
// row beyond the model's sizes are not read.
template <typename T, int MODEL>
PDDP_DEV ProblemT<T> problem_of_row(const ProblemT<T>& shared, const T* table,
                                    int b) {
  using D = ModelDims<MODEL>;
  const T* row = table + (size_t)b * PDDP_BATCH_ROW;
  ProblemT<T> P = shared;
  P.dt = row[PDDP_BATCH_PARAMS];
#pragma unroll
  for (int i = 0; i < kParamCount<MODEL> - 1; ++i)
    P.p[i] = row[PDDP_BATCH_PARAMS + 1 + i];
#pragma unroll
  for (int i = 0; i < D::na; ++i) P.goal[i] = row[PDDP_BATCH_X_GOAL + i];
#pragma unroll
  for (int i = 0; i < D::m; ++i) P.ugoal[i] = row[PDDP_BATCH_U_GOAL + i];
  return P;
}

// --------------------------------------------------------------------------
// nominal rollout: one lane per trajectory (nominal_rollout_kernel's mapping)
// --------------------------------------------------------------------------
template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void batch_rollout_kernel(
    ProblemT<T> shared, RolloutArgs<T> a, const T* table) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  if (a.mask != nullptr && a.mask[b] == 0) return;
  const ProblemT<T> P = problem_of_row<T, MODEL>(shared, table, b);
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
}

// --------------------------------------------------------------------------
// derivative records: one workgroup per trajectory, one lane per time step,
// records staged through LDS for coalesced writes (derivs_kernel's mapping);
// the row index is the workgroup's
// --------------------------------------------------------------------------
constexpr int kBatchDerivThreads = 64;

template <typename T, int MODEL>
__global__ __launch_bounds__(kBatchDerivThreads) void batch_derivs_kernel(
    ProblemT<T> shared, DerivArgs<T> a, const T* table) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr RecLayout lay(n, m);
  constexpr int S = lay.stride;
  constexpr int LD = kBatchDerivThreads + 1;  // conflict-free transposed reads
  __shared__ T stage[S * LD];
  __shared__ T Lsum[kBatchDerivThreads];

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  if (a.mask != nullptr && a.mask[b] == 0) return;
  const ProblemT<T> P = problem_of_row<T, MODEL>(shared, table, b);
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  const int N = a.N;
  const T* Zb = a.Z + (size_t)b * (N + 1) * n;
  const T* Ub = a.U + (size_t)b * N * m;
  T* rec_b = a.rec + (size_t)b * (N + 1) * S;
  T Jacc = T(0);  // only meaningful in lane 0

  for (int t0 = 0; t0 <= N; t0 += kBatchDerivThreads) {
    const int t = t0 + tid;
    T l = T(0);
    if (t <= N) {
      T z[n], un[m], w[S];
#pragma unroll
      for (int j = 0; j < n; ++j) z[j] = Zb[t * n + j];
      const bool terminal = (t == N);
#pragma unroll
      for (int j = 0; j < m; ++j) un[j] = terminal ? T(0) : Ub[t * m + j];
      // `terminal` as a constant in each call: the cost picks its matrix by
      // `terminal ? P.Qt : P.Q`, and a run-time choice between two members of
      // this per-workgroup COPY would put the whole copy into scratch memory
      // (the uniform kernel's problem is the kernel argument itself)
      if (terminal)
        l = record_of<T, MODEL>(P, z, un, true, bounded, a.u_min, a.u_max, w);
      else
        l = record_of<T, MODEL>(P, z, un, false, bounded, a.u_min, a.u_max, w);
      T* col = stage + tid;
#pragma unroll
      for (int j = 0; j < S; ++j) col[j * LD] = w[j];
      a.L[(size_t)b * (N + 1) + t] = l;
    }
    Lsum[tid] = l;
    __syncthreads();
    // coalesced write-out of this chunk's records
    const int nrec = min(kBatchDerivThreads, N + 1 - t0);
    T* dst = rec_b + (size_t)t0 * S;
    for (int o = tid; o < nrec * S; o += kBatchDerivThreads) {
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
}

// --------------------------------------------------------------------------
// line search: one lane per (trajectory, step size) - line_search_kernel's
// mapping, any A; the lanes of a trajectory read the same row (one broadcast
// read each ahead of the loop), the next step's nominal row and gains are
// requested ahead of the dependent chain
// --------------------------------------------------------------------------
template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void batch_line_search_kernel(
    ProblemT<T> shared, LineSearchArgs<T> a, const T* table) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr int GS = m + m * n;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = a.B * a.A;
  if (idx >= total) return;
  const int b = idx / a.A, ai = idx - b * a.A;
  if (a.active != nullptr && a.active[b] == 0) return;
  if (a.bwd_status != nullptr && a.bwd_status[b] != 0) return;
  const ProblemT<T> P = problem_of_row<T, MODEL>(shared, table, b);
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

  // time-major output [b][t][alpha][.] (the note at LineSearchArgs)
  T* Zci = a.Zc + ((size_t)b * (N + 1) * a.A + ai) * n;
  T* Uci = a.Uc + ((size_t)b * N * a.A + ai) * m;
  const size_t zstep = (size_t)a.A * n, ustep = (size_t)a.A * m;
  T J = T(0);
  for (int t = 0; t < N; ++t) {
    // prefetch the next step's nominal data before the dependent chain
    T zr2[n], ur2[m], gr2[GS];
    const int tn = (t + 1 < N) ? t + 1 : t;
#pragma unroll
    for (int j = 0; j < n; ++j) zr2[j] = Zb[tn * n + j];
#pragma unroll
    for (int j = 0; j < m; ++j) ur2[j] = Ub[tn * m + j];
#pragma unroll
    for (int j = 0; j < GS; ++j) gr2[j] = Gb[tn * GS + j];

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
  }
#pragma unroll
  for (int j = 0; j < n; ++j) Zci[(size_t)N * zstep + j] = z[j];
  const T lf = cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
  a.Jc[idx] = J + lf;  // L.sum(0) + l_f                           (ilqr.py:789)
}

// --------------------------------------------------------------------------
// launchers
// --------------------------------------------------------------------------
template <typename Args, typename T>
struct WithTable {
  Args a;
  const T* table;
};

template <typename T, int MODEL>
static int launch_batch_rollout(const pddp_problem& p,
                                WithTable<RolloutArgs<T>, T> w,
                                hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  const int blocks = (w.a.B + kWave - 1) / kWave;
  PDDP_LAUNCH((batch_rollout_kernel<T, MODEL>), dim3(blocks), dim3(kWave), 0,
              st, P, w.a, w.table);
  return launch_status();
}
template <typename T, int MODEL>
static int launch_batch_derivs(const pddp_problem& p,
                               WithTable<DerivArgs<T>, T> w, hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  PDDP_LAUNCH((batch_derivs_kernel<T, MODEL>), dim3(w.a.B),
              dim3(kBatchDerivThreads), 0, st, P, w.a, w.table);
  return launch_status();
}
template <typename T, int MODEL>
static int launch_batch_line_search(const pddp_problem& p,
                                    WithTable<LineSearchArgs<T>, T> w,
                                    hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  const long long total = (long long)w.a.B * w.a.A;
  const int blocks = (int)((total + kWave - 1) / kWave);
  PDDP_LAUNCH((batch_line_search_kernel<T, MODEL>), dim3(blocks), dim3(kWave),
              0, st, P, w.a, w.table);
  return launch_status();
}

// check_problem()'s domain: the four sample models under IGNORE_UNCERTAINTY
template <typename T>
static int batch_rollout_impl(const pddp_problem* p, const T* table, int B,
                              int N, const T* z0, const T* U, const T* u_min,
                              const T* u_max, const uint8_t* mask, T* Z,
                              void* stream) {
  if (B <= 0 || N <= 0 || !table || !z0 || !U || !Z) return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  WithTable<RolloutArgs<T>, T> w{{B, N, z0, U, u_min, u_max, mask, Z}, table};
  PDDP_DISPATCH_MODEL(launch_batch_rollout, T, p, w, (hipStream_t)stream)
}

template <typename T>
static int batch_derivs_impl(const pddp_problem* p, const T* table, int B,
                             int N, const T* Z, const T* U, const T* u_min,
                             const T* u_max, const uint8_t* mask, T* rec, T* L,
                             T* J, int32_t* state, void* stream) {
  if (B <= 0 || N <= 0 || !table || !Z || !U || !rec || !L || !J)
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  WithTable<DerivArgs<T>, T> w{
      {B, N, Z, U, u_min, u_max, mask, rec, L, J, state}, table};
  PDDP_DISPATCH_MODEL(launch_batch_derivs, T, p, w, (hipStream_t)stream)
}

template <typename T>
static int batch_line_search_impl(const pddp_problem* p, const T* table, int B,
                                  int N, int A, const T* Z, const T* U,
                                  const T* gains, const T* alphas,
                                  const T* u_min, const T* u_max,
                                  const uint8_t* active,
                                  const int32_t* bwd_status, T* Zc, T* Uc,
                                  T* Jc, void* stream) {
  if (B <= 0 || N <= 0 || A <= 0 || !table || !Z || !U || !gains || !alphas ||
      !Zc || !Uc || !Jc)
    return PDDP_E_BADARG;
  if ((long long)B * A > 0x7fffffffLL) return PDDP_E_BADARG;  // (int lane index)
  if (int rc = check_problem(p)) return rc;
  WithTable<LineSearchArgs<T>, T> w{{B, N, A, Z, U, gains, alphas, u_min,
                                     u_max, active, bwd_status, Zc, Uc, Jc},
                                    table};
  PDDP_DISPATCH_MODEL(launch_batch_line_search, T, p, w, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

int pddp_nominal_rollout_batch_f32(const pddp_problem* p, const float* table,
                                   int B, int N, const float* z0,
                                   const float* U, const float* u_min,
                                   const float* u_max, const uint8_t* mask,
                                   float* Z, void* stream) {
  return pddp::batch_rollout_impl<float>(p, table, B, N, z0, U, u_min, u_max,
                                         mask, Z, stream);
}
int pddp_nominal_rollout_batch_f64(const pddp_problem* p, const double* table,
                                   int B, int N, const double* z0,
                                   const double* U, const double* u_min,
                                   const double* u_max, const uint8_t* mask,
                                   double* Z, void* stream) {
  return pddp::batch_rollout_impl<double>(p, table, B, N, z0, U, u_min, u_max,
                                          mask, Z, stream);
}
int pddp_derivs_batch_f32(const pddp_problem* p, const float* table, int B,
                          int N, const float* Z, const float* U,
                          const float* u_min, const float* u_max,
                          const uint8_t* mask, float* rec, float* L, float* J,
                          int32_t* state, void* stream) {
  return pddp::batch_derivs_impl<float>(p, table, B, N, Z, U, u_min, u_max,
                                        mask, rec, L, J, state, stream);
}
int pddp_derivs_batch_f64(const pddp_problem* p, const double* table, int B,
                          int N, const double* Z, const double* U,
                          const double* u_min, const double* u_max,
                          const uint8_t* mask, double* rec, double* L,
                          double* J, int32_t* state, void* stream) {
  return pddp::batch_derivs_impl<double>(p, table, B, N, Z, U, u_min, u_max,
                                         mask, rec, L, J, state, stream);
}
int pddp_line_search_batch_f32(const pddp_problem* p, const float* table,
                               int B, int N, int A, const float* Z,
                               const float* U, const float* gains,
                               const float* alphas, const float* u_min,
                               const float* u_max, const uint8_t* active,
                               const int32_t* bwd_status, float* Zc, float* Uc,
                               float* Jc, void* stream) {
  return pddp::batch_line_search_impl<float>(p, table, B, N, A, Z, U, gains,
                                             alphas, u_min, u_max, active,
                                             bwd_status, Zc, Uc, Jc, stream);
}
int pddp_line_search_batch_f64(const pddp_problem* p, const double* table,
                               int B, int N, int A, const double* Z,
                               const double* U, const double* gains,
                               const double* alphas, const double* u_min,
                               const double* u_max, const uint8_t* active,
                               const int32_t* bwd_status, double* Zc,
                               double* Uc, double* Jc, void* stream) {
  return pddp::batch_line_search_impl<double>(p, table, B, N, A, Z, U, gains,
                                              alphas, u_min, u_max, active,
                                              bwd_status, Zc, Uc, Jc, stream);
}

}  // extern "C"
